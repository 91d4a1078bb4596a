"""numpy float64 restatement of torchio's HistogramStandardization (Nyul & Udupa) on the order statistics of tests/normalize_ref.py: the
reference of tests/test_histstd.py and tests/test_histstd_gpu.py.  Shares no code with the package.  The lines marked `torchio:` are
torchio 0.20's, written out; the landmark of a volume at percentile q is normalize_ref.order_stats' float32 cutoff."""
import numpy as np

import normalize_ref as ref

APPLY_INDEX = [0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12]
EPSILON = 1e-5


def percentiles(cutoff=(0.01, 0.99)) -> np.ndarray:
    cutoff = np.asarray(cutoff, dtype=np.float64)                # torchio: _standardize_cutoff
    cutoff[0] = max(0, cutoff[0])
    cutoff[1] = min(1, cutoff[1])
    cutoff[0] = np.min([cutoff[0], 0.09])
    cutoff[1] = np.max([cutoff[1], 0.91])
    quartiles = np.arange(25, 100, 25).tolist()                  # torchio: _get_percentiles
    deciles = np.arange(10, 100, 10).tolist()
    all_percentiles = list(100 * cutoff) + quartiles + deciles
    return np.array(sorted(set(all_percentiles)))


def landmarks(x: np.ndarray, qs, rule=None):
    """(float64 [len(qs)], n): the volume's landmarks, each the float32 cutoff of the masked voxels taken to float64; n = 0: zeros."""
    _, cut, n = ref.order_stats(x, list(qs), rule)
    return cut.astype(np.float64), n


def average_mapping(database: np.ndarray) -> np.ndarray:
    database = np.asarray(database, dtype=np.float64)
    pc1 = database[:, 0]                                         # torchio: _get_average_mapping
    pc2 = database[:, -1]
    s1, s2 = 0.0, 100.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        slopes = (s2 - s1) / (pc2 - pc1)
        slopes = np.nan_to_num(slopes)
        intercepts = np.mean(s1 - slopes * pc1)
        num_images = len(database)
        final_map = slopes.dot(database) / num_images + intercepts
    return final_map


def train(volumes, rule=None, cutoff=(0.01, 0.99)):
    """(landmarks float64 [13], database float64 [N][13], skipped): volumes with an empty mask are left out and counted."""
    qs = percentiles(cutoff)
    rows, skipped = [], 0
    for v in volumes:
        k, n = landmarks(v, qs, rule)
        if n == 0:
            skipped += 1
        else:
            rows.append(k)
    database = np.array(rows, dtype=np.float64).reshape(len(rows), len(qs))
    return average_mapping(database), database, skipped


def affine_map(knots, targets, epsilon=EPSILON):
    """(slopes, intercepts) of the 10 segments from 11 knots and 11 targets, float64"""
    quantiles, mapping = np.asarray(knots, np.float64), np.asarray(targets, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        diff_mapping = mapping[1:] - mapping[:-1]                # torchio: _normalize
        diff_perc = quantiles[1:] - quantiles[:-1]
        diff_perc[diff_perc < epsilon] = np.inf
        slopes = diff_mapping / diff_perc
        intercepts = mapping[:-1] - slopes * quantiles[:-1]
    return slopes, intercepts


def map_volume(x: np.ndarray, knots, targets, epsilon=EPSILON) -> np.ndarray:
    """y float32: every voxel through the segment np.digitize picks among the nine interior knots"""
    x = np.asarray(x, dtype=np.float32)
    slopes, intercepts = affine_map(knots, targets, epsilon)
    bin_id = np.digitize(x, np.asarray(knots, np.float64)[1:-1], right=False)
    with np.errstate(over="ignore", invalid="ignore"):
        return (slopes[bin_id] * x.astype(np.float64) + intercepts[bin_id]).astype(np.float32)


def standardize(x: np.ndarray, trained, rule=None, cutoff=(0.01, 0.99), epsilon=EPSILON):
    """(y float32, status): status 1 (empty mask) returns the input."""
    x = np.asarray(x, dtype=np.float32)
    qs = percentiles(cutoff)[APPLY_INDEX]
    knots, n = landmarks(x, qs, rule)
    if n == 0:
        return x.copy(), 1
    return map_volume(x, knots, np.asarray(trained, np.float64)[APPLY_INDEX], epsilon), 0
