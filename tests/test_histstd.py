"""CPU: the host side of data.HistogramStandardization (the percentile list, average_mapping, its place in DeviceCompose, the forms of the
`normalization` switch) and the numpy reference (tests/histstd_ref.py) against properties it must have.  No kernel runs here;
tests/test_histstd_gpu.py holds the kernels to the same reference."""
import warnings

import numpy as np
import pytest

import histstd_ref as href
import normalize_ref as ref
from gaviko_amd import data

DEFAULT = [1, 10, 20, 25, 30, 40, 50, 60, 70, 75, 80, 90, 99]
GOOD = np.linspace(0.0, 100.0, 13)


# ---- percentiles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff, ends", [((0.01, 0.99), (1, 99)), ((0, 1), (0, 100)), ((0.2, 0.5), (9, 91)), ((-1, 2), (0, 100)),
                                          ((0.05, 0.95), (5, 95)), ((0.001, 0.999), (0.1, 99.9))])
def test_percentile_list(cutoff, ends):
    got = data.landmark_percentiles(cutoff)
    want = sorted({100 * min(max(0, cutoff[0]), 0.09), 100 * max(min(1, cutoff[1]), 0.91), 25, 50, 75, *range(10, 100, 10)})
    assert got.dtype == np.float64 and len(got) == 13 and len(set(got.tolist())) == 13
    assert got.tolist() == want == href.percentiles(cutoff).tolist()
    assert np.allclose(got[[0, -1]], ends, rtol=0, atol=1e-12)
    assert got[list(data.LANDMARK_APPLY_INDEX)].tolist() == [p for p in want if p not in (25, 75)]


def test_default_percentiles():
    assert data.landmark_percentiles().tolist() == DEFAULT == data.HistogramStandardization(GOOD).percentiles.tolist()
    assert list(data.LANDMARK_APPLY_INDEX) == href.APPLY_INDEX
    with pytest.raises(ValueError):
        data.landmark_percentiles((0.01, 0.5, 0.99))


# ---- training arithmetic ----------------------------------------------------------------------------------------------------------------
def test_average_mapping_is_torchios_lines():
    rng = np.random.default_rng(0)
    database = np.sort(rng.standard_normal((5, 13)) * 100 + 300, axis=1)
    database[3] = 7.25                                            # P[i, 12] == P[i, 0]: the slope is inf and nan_to_num makes it finite
    pc1, pc2 = database[:, 0], database[:, -1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        slopes = np.nan_to_num((100.0 - 0.0) / (pc2 - pc1))
        want = slopes.dot(database) / len(database) + np.mean(0.0 - slopes * pc1)
    got = data.average_mapping(database)
    assert got.dtype == np.float64 and got.shape == (13,)
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(got, href.average_mapping(database), equal_nan=True)
    ok = np.delete(database, 3, axis=0)                           # without that volume: the first landmark is 0, the last 100
    got = data.average_mapping(ok)
    assert np.array_equal(got, href.average_mapping(ok)) and abs(got[0]) < 1e-9 and abs(got[-1] - 100) < 1e-9 and np.all(np.diff(got) > 0)
    with pytest.raises(ValueError):
        data.average_mapping(np.zeros((0, 13)))


# ---- the reference's own sanity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["normal", "zeros60", "ramps"])
def test_reference_maps_a_volume_with_the_target_landmarks_to_itself(fam):
    x = ref.family(fam, 4097)
    for b in range(3):
        knots, n = href.landmarks(x[b], href.percentiles()[href.APPLY_INDEX])
        trained = np.zeros(13)
        trained[href.APPLY_INDEX] = knots                          # the targets are the volume's own landmarks: the map is the identity
        y, status = href.standardize(x[b], trained)
        assert status == 0 and n == 4097
        inside = (np.diff(knots) >= href.EPSILON)[np.digitize(x[b], knots[1:-1])]     # a collapsed segment is flat, not the identity
        # slope is 1 within 2^-52 and icpt = k - slope k within one rounding of |k|: |y - x| <= 2^-50 (|x| + |k|) before the float32 rounding
        bound = np.spacing(np.abs(x[b])) * 0.5 + 2.0 ** -50 * (np.abs(x[b]) + np.abs(knots).max())
        assert inside.any() and np.all(np.abs(y.astype(np.float64) - x[b])[inside] <= bound[inside])


def test_reference_map_is_monotone_where_the_targets_are():
    rng = np.random.default_rng(1)
    x = np.sort(ref.family("normal", 4097)[0])
    knots, _ = href.landmarks(x, href.percentiles()[href.APPLY_INDEX])
    for targets in (np.linspace(0, 100, 11), np.sort(rng.random(11)) * 50, np.array([0, 1, 1, 1, 2, 3, 3, 4, 5, 6, 7.0])):
        y = href.map_volume(x, knots, targets)
        assert np.all(np.diff(y.astype(np.float64)) >= 0)
    flat = href.map_volume(x, knots, np.array([0, 1, 1, 1, 2, 3, 3, 4, 5, 6, 7.0]))
    seg = np.digitize(x, knots[1:-1])
    assert np.all(flat[seg == 1] == 1) and np.all(flat[seg == 2] == 1) and np.all(flat[seg == 5] == 3)


def test_reference_puts_a_voxel_on_a_knot_into_the_segment_to_its_right():
    knots = np.arange(11, dtype=np.float64) * 2                  # 0, 2, ..., 20
    targets = np.arange(11, dtype=np.float64) ** 2               # slopes 0.5, 1.5, 2.5, ...: every segment differs
    slopes, icpts = href.affine_map(knots, targets)
    x = knots.astype(np.float32)
    y = href.map_volume(x, knots, targets)
    for j in range(1, 10):                                       # interior knot j opens segment j
        assert y[j] == np.float32(slopes[j] * knots[j] + icpts[j]) and np.digitize(x[j], knots[1:-1]) == j
    assert y[0] == np.float32(icpts[0]) and y[10] == np.float32(slopes[9] * 20 + icpts[9])
    assert href.map_volume(np.float32([-4, 24]), knots, targets).tolist() == [-2.0, 138.0]      # the end segments extrapolate
    slopes, icpts = href.affine_map([0, 1, 1, 1 + 1e-6, 2, 3, 4, 5, 6, 7, 8], np.arange(11.0))  # gaps below epsilon: slope 0, the left target
    assert slopes[1] == 0 and slopes[2] == 0 and icpts[1] == 1 and icpts[2] == 2 and slopes[0] == 1


# ---- DeviceCompose bookkeeping ----------------------------------------------------------------------------------------------------------
def test_compose_runs_it_before_the_second_normaliser(monkeypatch):
    h, z, r = data.HistogramStandardization(GOOD), data.ZNormalization(), data.RescaleIntensity(percentiles=(1, 99))
    for listed in ([h, z], [z, h], [data.RandomFlip(), z, data.RandomNoise(), h]):
        c = data.DeviceCompose(listed)
        assert c.hist == [h] and c.znorm == [z] and c.rescale == [] and c.last_hist_status is None and c.last_norm_status is None
    c = data.DeviceCompose([r, h])
    assert c.hist == [h] and c.rescale == [r]
    assert data.DeviceCompose([h]).hist == [h]
    order = []
    h.apply = lambda x, part: (order.append("hist"), (x, "hs"))[1]
    z.apply = lambda x, part: (order.append("znorm"), (x, "zs"))[1]

    class Fake:                                                   # stands in for a device batch: the compose only passes it on
        is_cuda, dtype, shape = True, data.torch.float32, (2, 1, 4, 4, 4)
        device = "cpu"

        def is_contiguous(self):
            return True

    monkeypatch.setattr(data.ops, "minmax_partials", lambda B, dev: None)
    c = data.DeviceCompose([z, h])
    c(Fake())
    assert order == ["hist", "znorm"] and c.last_hist_status == "hs" and c.last_norm_status == "zs"


def test_apply_is_three_launches(monkeypatch):
    torch, ops, calls = data.torch, data.ops, []
    monkeypatch.setattr(ops, "volume_stats", lambda x, rule, **k: (calls.append(("volume_stats", rule, k)), ("stats", None))[1])
    monkeypatch.setattr(ops, "volume_landmarks", lambda x, stats, q: (calls.append(("volume_landmarks", stats, list(q))), (None, "cutoffs"))[1])
    monkeypatch.setattr(ops, "histogram_standardize", lambda x, y, stats, cutoffs, targets, eps:
                        (calls.append(("histogram_standardize", stats, cutoffs, list(targets), eps)), "status")[1])
    x = torch.zeros(2, 1, 3, 4, 5)
    y, status = data.HistogramStandardization(GOOD, masking_method="mean", epsilon=1e-4).apply(x, None)
    assert status == "status" and y.shape == x.shape and y is not x
    assert calls == [("volume_stats", "mean", dict(want_std=False)), ("volume_landmarks", "stats", [p for p in DEFAULT if p not in (25, 75)]),
                     ("histogram_standardize", "stats", "cutoffs", GOOD[href.APPLY_INDEX].tolist(), 1e-4)]


def test_at_most_one_of_it_and_the_old_rule_stays():
    h = data.HistogramStandardization(GOOD)
    with pytest.raises(NotImplementedError):
        data.DeviceCompose([h, data.HistogramStandardization(GOOD)])
    with pytest.raises(NotImplementedError):
        data.DeviceCompose([h, data.ZNormalization(), data.RescaleIntensity()])
    assert "HistogramStandardization" in data._BUILT and data._BUILT.index("HistogramStandardization") > data._BUILT.index("RandomAnisotropy")


@pytest.mark.parametrize("kw", [dict(), dict(intensity=True, motion=True), dict(elastic=True, intensity=True)])
def test_it_draws_nothing(kw):
    h = data.HistogramStandardization(GOOD, masking_method="mean")
    draws = []
    for norm in ("minmax", h, [h, "znorm"], {"histogram": {"landmarks": GOOD.tolist()}, "then": "percentile"}):
        c = data.train_transforms(seed=11, normalization=norm, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mats, flags = c.sample(5, (24, 32, 40))
        draws.append((mats, flags, repr(c.last_params), repr(c.last_intensity), repr(c.last_elastic), c.rng.random()))
    for d in draws[1:]:
        assert np.array_equal(d[0], draws[0][0]) and np.array_equal(d[1], draws[0][1]) and d[2:] == draws[0][2:]


# ---- the normalization switch -----------------------------------------------------------------------------------------------------------
def test_normalizer_forms(tmp_path):
    h = data.HistogramStandardization(GOOD)
    assert data.normalizer(h) is h
    for name, cls in (("znorm", data.ZNormalization), ("percentile", data.RescaleIntensity), ("minmax", data.RescaleIntensity)):
        assert isinstance(data.normalizer(name), cls)
        both = data.normalizer([h, name])
        assert isinstance(both, list) and both[0] is h and isinstance(both[1], cls)
        for make in (lambda n: data.train_transforms(seed=0, normalization=n), data.eval_transforms):
            c = make([h, name])
            assert c.hist == [h] and len(c.rescale + c.znorm) == 1 and isinstance((c.rescale + c.znorm)[0], cls)
    c = data.eval_transforms(h)
    assert c.hist == [h] and c.rescale == [] and c.znorm == []
    for bad in ("histogram", "hist", [h], [h, h], ["znorm", h], [h, "znorm", "minmax"], [h, "histogram"], {"then": "znorm"},
                {"histogram": {"landmarks": GOOD}, "after": "znorm"}):
        with pytest.raises(ValueError):
            data.normalizer(bad)
    with pytest.raises(ValueError):
        data.train_transforms(normalization="histogram")
    with pytest.raises(ValueError):
        data.eval_transforms("histogram")


def test_preprocessor_reads_the_dict(tmp_path):
    path = tmp_path / "landmarks.npy"
    np.save(path, GOOD)
    norm = {"histogram": {"landmarks": str(path), "masking_method": "mean", "cutoff": [0.02, 0.98]}, "then": "znorm"}
    pre = data.DataPreprocessor({"data": {"normalization": norm}}, seed=0)
    for c in (pre.train_transforms, pre.val_transforms, pre.test_transforms):
        assert len(c.hist) == 1 and c.rescale == [] and isinstance(c.znorm[0], data.ZNormalization) and c.znorm[0].masking_method == "mean"
        t = c.hist[0]
        assert np.array_equal(t.landmarks, GOOD) and t.masking_method == "mean" and t.percentiles[0] == 2 and t.percentiles[-1] == 98
    pre = data.DataPreprocessor({"data": {"normalization": {"histogram": {"landmarks": str(path)}}}}, seed=0)     # no `then`: nothing follows
    for c in (pre.train_transforms, pre.val_transforms, pre.test_transforms):
        assert len(c.hist) == 1 and c.rescale == [] and c.znorm == [] and c.hist[0].masking_method is None and c.hist[0].epsilon == 1e-5


# ---- the constructor ----------------------------------------------------------------------------------------------------------------------
def test_landmarks_from_values_and_from_a_file(tmp_path):
    t = data.HistogramStandardization(GOOD.tolist(), masking_method=3, cutoff=(0, 1), epsilon=1e-3)
    assert t.landmarks.dtype == np.float64 and np.array_equal(t.landmarks, GOOD) and t.masking_method == 3.0 and t.epsilon == 1e-3
    assert t.percentiles[0] == 0 and t.percentiles[-1] == 100 and t.cutoff == (0.0, 1.0)
    np.save(tmp_path / "l.npy", GOOD)
    assert np.array_equal(data.HistogramStandardization(tmp_path / "l.npy").landmarks, GOOD)
    assert np.array_equal(data.HistogramStandardization(str(tmp_path / "l.npy")).landmarks, GOOD)
    flat = GOOD.copy()
    flat[4] = flat[3]                                             # equal neighbours do not decrease: accepted
    data.HistogramStandardization(flat)


@pytest.mark.parametrize("bad", [GOOD[:12], np.append(GOOD, 101.0), GOOD[::-1], np.where(np.arange(13) == 5, np.nan, GOOD),
                                 np.where(np.arange(13) == 12, np.inf, GOOD), GOOD.reshape(1, 13), []])
def test_bad_landmarks_are_refused(bad):
    with pytest.raises(ValueError):
        data.HistogramStandardization(bad)


def test_bad_masks_and_epsilon_are_refused():
    for bad in (lambda x: x > 0, "label", True):
        with pytest.raises(NotImplementedError):
            data.HistogramStandardization(GOOD, masking_method=bad)
    with pytest.raises(ValueError):
        data.HistogramStandardization(GOOD, epsilon=-1.0)


def test_training_needs_device_batches():
    with pytest.raises(RuntimeError):
        data.HistogramStandardization.train([data.torch.zeros(2, 1, 4, 4, 4)])
    with pytest.raises(ValueError):
        data.HistogramStandardization.train([])
