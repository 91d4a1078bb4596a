"""numpy float64 restatement of the intensity normalisers (torchio's RescaleIntensity with percentiles and a mask, ZNormalization): the
reference of tests/test_normalize.py and tests/test_normalize_gpu.py.  Shares no code with the package.  Order statistics come from
np.sort, cutoffs from np.percentile on float64 values, means from math.fsum, the unbiased std from the fsum mean in float64."""
import math

import numpy as np


def mask_of(x: np.ndarray, rule) -> np.ndarray:
    """None: every voxel; 'mean': x > x.mean() with the mean rounded to float32; a number t: x > t."""
    x = np.asarray(x, dtype=np.float32).ravel()
    if rule is None:
        return np.ones(x.shape, dtype=bool)
    if isinstance(rule, str) and rule == "mean":
        return x > np.float32(math.fsum(x.astype(np.float64).tolist()) / x.size)
    return x > np.float32(rule)


def stats(x: np.ndarray, rule=None) -> dict:
    x = np.asarray(x, dtype=np.float32).ravel()
    x64 = x.astype(np.float64)
    m = mask_of(x, rule)
    vals = x64[m]
    n = int(vals.size)
    out = dict(min=float(x.min()), max=float(x.max()), mean_all=math.fsum(x64.tolist()) / x.size, n=n, mean=0.0, std=0.0,
               mean_abs_all=math.fsum(np.abs(x64).tolist()) / x.size, mean_abs=math.fsum(np.abs(vals).tolist()) / n if n else 0.0)
    if n:
        out["mean"] = math.fsum(vals.tolist()) / n
    if n >= 2:
        out["std"] = math.sqrt(math.fsum(((vals - out["mean"]) ** 2).tolist()) / (n - 1))
    return out


def order_stats(x: np.ndarray, percentiles, rule=None):
    """(pairs float32 [Q][2], cutoffs float32 [Q], n): the i-th and min(i + 1, n - 1)-th smallest masked values for the virtual index
    v = (n - 1) * (q / 100), i = floor(v), and np.percentile of the float64 values rounded to float32.  n = 0: zeros."""
    x = np.asarray(x, dtype=np.float32).ravel()
    vals = np.sort(x[mask_of(x, rule)])
    n = int(vals.size)
    Q = len(percentiles)
    if n == 0:
        return np.zeros((Q, 2), np.float32), np.zeros(Q, np.float32), 0
    pairs = np.zeros((Q, 2), np.float32)
    for j, q in enumerate(percentiles):
        v = np.float64(n - 1) * (np.float64(q) / 100.0)
        i = int(math.floor(v))
        pairs[j] = vals[i], vals[min(i + 1, n - 1)]
    with np.errstate(over="ignore", invalid="ignore"):
        cut = np.percentile(vals.astype(np.float64), [float(q) for q in percentiles]).astype(np.float32)
    return pairs, cut, n


def linear_cutoff(a, b, n: int, q: float) -> np.float32:
    """The rule np.percentile's 'linear' method evaluates on float64 operands, written out: c = a + (b - a) g for g < 0.5, else
    b - (b - a) (1 - g), g the fraction of the virtual index."""
    v = np.float64(n - 1) * (np.float64(q) / 100.0)
    g = v - math.floor(v)
    a, b = np.float64(a), np.float64(b)
    return np.float32(a + (b - a) * g if g < 0.5 else b - (b - a) * (1.0 - g))


def rescale_clipped(x: np.ndarray, lo, hi, out_min=0.0, out_max=1.0):
    """torchio's rescale arithmetic once the float32 cutoffs (lo, hi) are known: (y float32, status).  The whole volume is clipped,
    in_min / in_max are the extremes of the clipped volume, then x -= in_min; x /= in_range; x *= out_range; x += out_min in float32.
    status 2 (in_range == 0) returns the input."""
    a = np.array(x, dtype=np.float32, copy=True)
    clipped = np.clip(a, np.float32(lo), np.float32(hi))
    in_min, in_max = clipped.min(), clipped.max()
    with np.errstate(over="ignore", invalid="ignore"):
        in_range = np.float32(in_max - in_min)
        if in_range == 0:
            return a, 2
        clipped -= in_min
        clipped /= in_range
        clipped *= np.float32(np.float32(out_max) - np.float32(out_min))
        clipped += np.float32(out_min)
    return clipped, 0


def rescale(x: np.ndarray, out_min=0.0, out_max=1.0, percentiles=(0, 100), rule=None):
    """torchio's RescaleIntensity.rescale: the cutoffs are the two percentiles of the masked voxels; status 1 (empty mask) returns the input."""
    _, cut, n = order_stats(x, percentiles, rule)
    if n == 0:
        return np.array(x, dtype=np.float32, copy=True), 1
    return rescale_clipped(x, cut[0], cut[1], out_min, out_max)


def znorm(x: np.ndarray, rule=None):
    """(y float64, status): (x - mean) / std of the masked voxels in float64; status 1 (empty mask) and 2 (n < 2 or std == 0) return x."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    s = stats(x, rule)
    if s["n"] == 0:
        return x64, 1
    if s["n"] < 2 or s["std"] == 0.0:
        return x64, 2
    return (x64 - s["mean"]) / s["std"], 0


# ---- input families of the GPU tests: three different volumes of V voxels each, float32 [3][V] ------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)
FAMILIES = ("normal", "ties", "constant", "zeros60", "special", "ramps", "low10", "high11")
# families whose standard deviation is at least |mean| / 64 under every mask that leaves two voxels or more, so that the relative bound on
# the std is meaningful (tests/test_normalize.py checks it); 'constant' has std 0 exactly, 'low10' spreads 2^-13 of its mean
STD_FAMILIES = ("normal", "ties", "zeros60", "special", "ramps", "high11")


def family(name: str, V: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng([seed, V, FAMILIES.index(name)])
    if name == "normal":                                          # (a) distinct normals x 1000
        x = rng.standard_normal((3, V)) * 1000
    elif name == "ties":                                          # (b) the integers 0..7
        x = rng.integers(0, 8, (3, V))
    elif name == "constant":                                      # (c)
        x = np.repeat(np.array([[3.5], [-2.0], [0.0]]), V, axis=1)
    elif name == "zeros60":                                       # (d) 60 % exact zeros, the rest positive: one hot bin
        x = np.where(rng.random((3, V)) < 0.6, 0.0, np.abs(rng.standard_normal((3, V))) * 500 + 1)
    elif name == "special":                                       # (e) mixed signs, both zeros, denormals, +-3e38
        x = (rng.standard_normal((3, V)) * 10).astype(np.float32)
        # The three large values never cancel (net +2.5e38 f), in no prefix either: a volume whose float64 sum cancels to the level of its
        # denormals has a mean -- and with it the 'mean' mask -- that depends on the order of summation, which no fixed-order sum can pin.
        special = np.array([2.5e38, 3e38, -3e38, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1e-39, 0.0, -0.0], dtype=np.float64)
        for b in range(3):
            k = min(V, len(special))
            sp = special.copy()
            sp[:3] *= 1.0 - 0.125 * b
            x[b, rng.choice(V, size=k, replace=False)] = sp[:k].astype(np.float32)
    elif name == "ramps":                                         # (f) ascending, descending, and one through zero
        r = np.arange(V, dtype=np.float64)
        x = np.stack([r + 7, (V - 1 - r) * 2.0, (r - V // 2) * 0.5])
    elif name == "low10":                                         # (g) keys that differ in the lowest 10 bits only: the last pass decides
        x = (np.uint32(0x44800000) | rng.integers(0, 1024, (3, V)).astype(np.uint32)).view(np.float32)
    elif name == "high11":                                        # (g) keys that differ in the highest 11 bits only: the first pass decides
        top = (rng.integers(0, 2, (3, V)) << 10) | (rng.integers(0, 255, (3, V)) << 2) | rng.integers(0, 4, (3, V))   # sign, exponent < 255, 2 bits
        x = ((top.astype(np.uint32) << np.uint32(21)) | np.uint32(0x155555)).view(np.float32)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x, dtype=np.float32)
