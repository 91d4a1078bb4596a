"""GPU: the normalisation kernels (gaviko_amd/csrc/normalize.hip) through ops.volume_stats / ops.volume_order_stats / ops.normalize_intensity
and through data.DeviceCompose, against the numpy float64 restatement tests/normalize_ref.py.  Every launch carries B = 3 different volumes.
Every test prints its measured maxima before it asserts (`pytest -m gpu -s`; profiles/normalize_parity_report.txt is a copy of those lines).

What is equality and what is a bound:
* order statistics: the pairs (a, b) and n EQUAL the sorted reference (as values: -0.0 == +0.0), the cutoffs EQUAL np.percentile of the
  float64 values rounded to float32 -- for every size, family, percentile and mask rule below.
* min and max are equal.  mean: within (n + 8) 2^-53 mean|x| of math.fsum -- n float64 additions in any fixed order stay within
  (n - 1) 2^-53 sum|x|, plus the division.  std: within (n + 8) 2^-52 std where std >= |mean| / 64 (each squared deviation carries 3
  roundings, the sum n - 1, the square root halves the relative error; the error d of the mean enters as n d^2, second order under that
  condition).  A case whose reference std is 0 must give exactly 0; the one family that does not meet the condition ('low10', a spread
  of 2^-13 of the mean) gets the same bound plus that second-order term d^2 / std written out.
* percentile rescale: bit for bit the reference's four float32 steps on the clipped volume.  Where a float32 step overflows (the
  families with +-3e38 under percentiles (0, 100): in_range = inf, then inf / inf) both sides give NaN there; NaN payloads are not
  compared, every other element is.
* z-normalisation: |y - y_ref| <= 2^-22 max(|y_ref|, 1); the masked mean of y within 1e-6 of 0, its masked std within 1e-6 of 1."""
import functools

import numpy as np
import pytest
import torch

import normalize_ref as ref

pytestmark = pytest.mark.gpu

BIG = 528389                        # past both grid caps: 128 slabs x 4096 voxels of the statistics / select kernels, 512 x 1024 of the apply
SIZES = (1, 2, 3, 7, 64, 65, 1023, 4097, 70001, 262147, BIG)
PERCENTILE_SETS = ((0, 100), (0.5, 99.5), (1, 99), (25, 75), (50, 50), (0, 0), (100, 100))
PACKED = ((0, 100, 0.5, 99.5), (1, 99, 25, 75), (50, 50, 0, 0), (100, 100))   # the seven sets, up to four percentiles per launch
MASKS = (None, "mean", ref.FLT_MAX)                                           # nothing above the largest float: the empty mask
MAXIMA = {}


def _note(key, value):
    MAXIMA[key] = max(MAXIMA.get(key, 0.0), float(value))


def _bits_equal(got, want):
    """bit for bit, except that a NaN is a NaN whatever its payload"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


@functools.lru_cache(maxsize=None)
def _reference(V, fam):
    """the inputs and, per sample and mask rule, the reference's statistics and order statistics at all nine percentiles"""
    x = ref.family(fam, V)
    qs = sorted({q for s in PERCENTILE_SETS for q in s})
    out = {}
    for b in range(3):
        for rule in MASKS:
            pairs, cut, n = ref.order_stats(x[b], qs, rule)
            out[b, rule] = dict(stats=ref.stats(x[b], rule), n=n, pairs=dict(zip(qs, pairs)), cut=dict(zip(qs, cut)))
    return x, out


def _stats(dev, xd, rule, want_std=True):
    from gaviko_amd import ops
    return ops.volume_stats(xd, rule, want_std=want_std)


@pytest.mark.parametrize("fam", ref.FAMILIES)
@pytest.mark.parametrize("V", SIZES)
def test_statistics_and_order_statistics(dev, V, fam):
    from gaviko_amd import ops
    x, want = _reference(V, fam)
    xd = torch.from_numpy(x).to(dev)
    worst_mean = worst_std = 0.0
    for rule in MASKS:
        stats, count = _stats(dev, xd, rule)
        again, count2 = _stats(dev, xd, rule)
        assert torch.equal(stats.view(torch.int64), again.view(torch.int64)) and torch.equal(count, count2), "repeated launches differ"
        st, cnt = stats.cpu().numpy(), count.cpu().numpy()
        for b in range(3):
            w = want[b, rule]["stats"]
            got = dict(zip(ops.STATS_FIELDS, st[b]))
            assert got["min"] == w["min"] and got["max"] == w["max"], (rule, b, got, w)
            assert cnt[b] == w["n"] == got["n"], (rule, b, cnt[b], w["n"])
            bound_all = (V + 8) * 2.0 ** -53 * w["mean_abs_all"]
            assert abs(got["mean_all"] - w["mean_all"]) <= bound_all, (rule, b, got["mean_all"], w["mean_all"], bound_all)
            n = w["n"]
            bound = (n + 8) * 2.0 ** -53 * w["mean_abs"]
            err = abs(got["mean"] - w["mean"])
            if bound > 0:
                worst_mean = max(worst_mean, err / bound)
            assert err <= bound, (rule, b, got["mean"], w["mean"], bound)
            if n < 2 or w["std"] == 0.0:
                assert got["std"] == 0.0, (rule, b, got["std"])
                continue
            sbound = (n + 8) * 2.0 ** -52 * w["std"]
            if w["std"] < abs(w["mean"]) / 64:                        # 'low10' (and nothing else: asserted on the CPU for the other families)
                assert fam not in ref.STD_FAMILIES or V < 64, (fam, V, rule, b)
                sbound += bound * bound / w["std"]
            serr = abs(got["std"] - w["std"])
            worst_std = max(worst_std, serr / sbound)
            assert serr <= sbound, (rule, b, got["std"], w["std"], sbound)
        for qs in PACKED:
            pairs, cutoffs = ops.volume_order_stats(xd, stats, qs)
            pairs, cutoffs = pairs.cpu().numpy(), cutoffs.cpu().numpy()
            for b in range(3):
                w = want[b, rule]
                for j, q in enumerate(qs):
                    assert pairs[b, j, 0] == w["pairs"][q][0] and pairs[b, j, 1] == w["pairs"][q][1], (rule, b, q, pairs[b, j], w["pairs"][q], w["n"])
                    assert cutoffs[b, j] == w["cut"][q], (rule, b, q, cutoffs[b, j], w["cut"][q])
    _note("mean error / bound", worst_mean)
    _note("std error / bound", worst_std)
    print(f"normalize statistics V={V} {fam}: mean error {worst_mean:.3f} of its bound, std error {worst_std:.3f} of its bound; "
          f"{3 * len(MASKS) * 9} order statistics equal")


@pytest.mark.parametrize("fam", ref.FAMILIES)
@pytest.mark.parametrize("V", SIZES)
def test_percentile_rescale_bit_for_bit(dev, V, fam):
    from gaviko_amd import ops
    x, want = _reference(V, fam)
    xd = torch.from_numpy(x).to(dev)
    codes = set()
    for rule in MASKS:
        stats, _ = _stats(dev, xd, rule, want_std=False)
        for qs in PERCENTILE_SETS:
            out_min, out_max = (-1.0, 3.0) if qs == (1, 99) else (0.0, 1.0)
            _, cutoffs = ops.volume_order_stats(xd, stats, qs)
            y = torch.full_like(xd, float("nan"))
            status = ops.normalize_intensity(xd, y, stats, ops.NORMALIZE_RESCALE, cutoffs, out_min, out_max).cpu().numpy()
            y = y.cpu().numpy()
            for b in range(3):
                w = want[b, rule]
                yr, code = (x[b], 1) if w["n"] == 0 else ref.rescale_clipped(x[b], w["cut"][qs[0]], w["cut"][qs[1]], out_min, out_max)
                assert status[b] == code, (rule, qs, b, status[b], code)
                assert _bits_equal(y[b], yr), (rule, qs, b, int(np.sum(y[b].view(np.uint32) != yr.view(np.uint32))))
                codes.add(code)
    print(f"normalize rescale V={V} {fam}: {len(MASKS) * len(PERCENTILE_SETS) * 3} volumes bit for bit, status words met {sorted(codes)}")


@pytest.mark.parametrize("fam", ref.FAMILIES)
@pytest.mark.parametrize("V", SIZES)
def test_znormalization(dev, V, fam):
    from gaviko_amd import ops
    x, want = _reference(V, fam)
    xd = torch.from_numpy(x).to(dev)
    worst = worst_mean = worst_std = 0.0
    for rule in MASKS:
        stats, _ = _stats(dev, xd, rule)
        y = torch.full_like(xd, float("nan"))
        status = ops.normalize_intensity(xd, y, stats, ops.NORMALIZE_ZNORM).cpu().numpy()
        y = y.cpu().numpy()
        for b in range(3):
            yr, code = ref.znorm(x[b], rule)
            assert status[b] == code, (rule, b, status[b], code)
            if code:
                assert np.array_equal(y[b].view(np.uint32), x[b].view(np.uint32)), (rule, b)
                continue
            err = np.abs(y[b].astype(np.float64) - yr) / np.maximum(np.abs(yr), 1.0)
            worst = max(worst, float(err.max()))
            assert err.max() <= 2.0 ** -22, (rule, b, float(err.max()))
            m = ref.mask_of(x[b], rule)
            ym = y[b].astype(np.float64)[m]
            worst_mean, worst_std = max(worst_mean, abs(ym.mean())), max(worst_std, abs(ym.std(ddof=1) - 1.0))
            assert abs(ym.mean()) <= 1e-6 and abs(ym.std(ddof=1) - 1.0) <= 1e-6, (rule, b, ym.mean(), ym.std(ddof=1))
    _note("znorm error / max(|y|, 1)", worst)
    _note("znorm |masked mean|", worst_mean)
    _note("znorm |masked std - 1|", worst_std)
    print(f"normalize znorm V={V} {fam}: max error {worst:.3e} (bound {2.0 ** -22:.3e}), masked mean {worst_mean:.3e}, |masked std - 1| {worst_std:.3e}")


def test_measured_maxima():
    """the worst figures of the parametrised tests above, in one place (empty when this test runs alone)"""
    for k, v in sorted(MAXIMA.items()):
        print(f"normalize maxima: {k} = {v:.3e}")
    assert all(np.isfinite(v) for v in MAXIMA.values())
    _reference.cache_clear()


# ---- (0, 100) without a mask is the plain min-max ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [4097, 70001])
def test_new_path_equals_the_oracle_rescale_on_the_defaults(dev, V):
    from gaviko_amd import ops
    from oracle import data_ref
    x = ref.family("normal", V, seed=1) + np.float32(1000)
    xd = torch.from_numpy(x).to(dev)
    stats, _ = ops.volume_stats(xd, None, want_std=False)
    _, cutoffs = ops.volume_order_stats(xd, stats, (0, 100))
    y = torch.empty_like(xd)
    status = ops.normalize_intensity(xd, y, stats, ops.NORMALIZE_RESCALE, cutoffs, 0.0, 1.0)
    assert status.cpu().tolist() == [0, 0, 0]
    for b in range(3):
        assert np.array_equal(y[b].cpu().numpy().view(np.uint32), data_ref.rescale_intensity(x[b]).view(np.uint32))


def test_default_rescale_keeps_its_two_kernels(dev, monkeypatch):
    from gaviko_amd import data, ops
    x = torch.from_numpy(ref.family("normal", 24 * 32 * 40, seed=2).reshape(3, 1, 24, 32, 40) + np.float32(500)).to(dev)
    part = ops.minmax_partials(3, dev)
    ops.volume_minmax(x, part)
    want = torch.empty_like(x)
    ops.rescale_intensity(x, part, want, 0.0, 1.0)
    calls = []
    for name in ("volume_minmax", "rescale_intensity", "volume_stats", "volume_order_stats", "normalize_intensity"):
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(getattr(ops, name), name))
    c = data.DeviceCompose([data.RescaleIntensity()])
    got = c(x)
    assert calls == ["volume_minmax", "rescale_intensity"] and c.last_norm_status is None
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- status words, neighbours, sentinels ------------------------------------------------------------------------------------------------
def _with_sentinels(dev, B, V):
    """y [B][V] inside a larger buffer of sentinels, 16-byte aligned"""
    full = torch.full((B * V + 32,), -12345.0, device=dev)
    return full, full[16:16 + B * V].view(B, V)


def _sentinels_intact(full, n):
    return bool((full[:16] == -12345.0).all() and (full[16 + n:] == -12345.0).all())


@pytest.mark.parametrize("V", [7, 4099])
@pytest.mark.parametrize("mode", ["rescale", "znorm"])
def test_status_words_and_neighbours(dev, V, mode):
    from gaviko_amd import ops
    good = ref.family("normal", V, seed=3)
    x = np.stack([good[0], np.full(V, 3.5, np.float32), good[1]])                  # a constant volume between two ordinary ones
    xd = torch.from_numpy(x).to(dev)
    full, y = _with_sentinels(dev, 3, V)

    def run(rule, qs=(0.5, 99.5)):
        full.fill_(-12345.0)
        stats, count = ops.volume_stats(xd, rule)
        if mode == "rescale":
            _, cutoffs = ops.volume_order_stats(xd, stats, qs)
            status = ops.normalize_intensity(xd, y, stats, ops.NORMALIZE_RESCALE, cutoffs, 0.0, 1.0)
        else:
            status = ops.normalize_intensity(xd, y, stats, ops.NORMALIZE_ZNORM)
        assert _sentinels_intact(full, 3 * V)
        return status.cpu().tolist(), y.cpu().numpy(), count.cpu().tolist()

    def check(b, rule, qs, got):
        if mode == "rescale":
            assert _bits_equal(got, ref.rescale(x[b], 0.0, 1.0, qs, rule)[0])
        else:
            yr = ref.znorm(x[b], rule)[0]
            assert np.all(np.abs(got.astype(np.float64) - yr) <= 2.0 ** -22 * np.maximum(np.abs(yr), 1.0))

    status, got, _ = run(None)
    assert status == [0, 2, 0]
    assert np.array_equal(got[1].view(np.uint32), x[1].view(np.uint32))           # the constant volume comes back bit for bit ...
    check(0, None, (0.5, 99.5), got[0]), check(2, None, (0.5, 99.5), got[2])      # ... its neighbours normalised
    status, got, count = run(ref.FLT_MAX)
    assert status == [1, 1, 1] and count == [0, 0, 0] and np.array_equal(got.view(np.uint32), x.view(np.uint32))
    one = float(np.sort(x[0])[-2])                                                # exactly one voxel of sample 0 lies above it
    status, got, count = run(one)
    assert count[0] == 1 and status[0] == 2 and np.array_equal(got[0].view(np.uint32), x[0].view(np.uint32))
    if mode == "rescale":
        status, got, _ = run(None, (50, 50))                                      # the two cutoffs coincide: nothing to rescale
        assert status == [2, 2, 2] and np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_wrappers_refuse_what_is_not_built(dev):
    from gaviko_amd import lib, ops
    x = torch.zeros(2, 16, device=dev)
    stats, _ = ops.volume_stats(x)
    for bad in ((), (1, 2, 3, 4, 5), (-1, 50), (0, 101)):
        with pytest.raises(lib.GavikoHipError):
            ops.volume_order_stats(x, stats, bad)
    with pytest.raises(lib.GavikoHipError):
        ops.volume_stats(x, mask=lambda v: v > 0)
    with pytest.raises(lib.GavikoHipError):
        ops.volume_stats(x.double())
    with pytest.raises(lib.GavikoHipError):
        ops.normalize_intensity(x, torch.empty_like(x), stats, ops.NORMALIZE_RESCALE)            # the rescale needs cutoffs
    with pytest.raises(lib.GavikoHipError):
        ops.normalize_intensity(x, torch.empty_like(x), stats, 7)
    with pytest.raises(lib.GavikoHipError):
        ops.normalize_intensity(x, torch.empty(2, 8, device=dev), stats, ops.NORMALIZE_ZNORM)


# ---- the pipeline ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(intensity=True)])
@pytest.mark.parametrize("norm", ["percentile", "znorm"])
def test_pipeline_equals_the_stages_by_hand(dev, norm, kw):
    from gaviko_amd import data, ops
    shape = (24, 32, 40)
    raw = ref.family("zeros60", int(np.prod(shape)), seed=4)
    x = torch.from_numpy(np.concatenate([raw, raw[:1] * 2]).reshape(4, 1, *shape)).to(dev)
    c = data.train_transforms(seed=5, normalization=norm, **kw)
    got = c(x)
    plain = data.train_transforms(seed=5, normalization="minmax", **kw)
    plain(x)
    assert repr(c.last_params) == repr(plain.last_params) and repr(c.last_intensity) == repr(plain.last_intensity)
    assert plain.last_norm_status is None and c.last_norm_status.cpu().tolist() == [0, 0, 0, 0]
    stages = [t for t in (plain.affine + plain.flips + plain.intensity)]
    aug = data.DeviceCompose(stages, seed=5)(x)                                   # the same draws, no normaliser
    y = torch.empty_like(aug)
    if norm == "percentile":
        stats, _ = ops.volume_stats(aug, None, want_std=False)
        _, cutoffs = ops.volume_order_stats(aug, stats, (0.5, 99.5))
        ops.normalize_intensity(aug, y, stats, ops.NORMALIZE_RESCALE, cutoffs, 0.0, 1.0)
    else:
        stats, _ = ops.volume_stats(aug, "mean", want_std=True)
        ops.normalize_intensity(aug, y, stats, ops.NORMALIZE_ZNORM)
    assert torch.equal(got.view(torch.int32), y.view(torch.int32))
    a = aug.cpu().numpy().reshape(4, -1)
    for b in range(4):                                                            # and the stages by hand are the reference's
        if norm == "percentile":
            assert _bits_equal(got[b].cpu().numpy().ravel(), ref.rescale(a[b], 0.0, 1.0, (0.5, 99.5))[0])
        else:
            yr = ref.znorm(a[b], "mean")[0]
            assert np.all(np.abs(got[b].cpu().numpy().ravel().astype(np.float64) - yr) <= 2.0 ** -22 * np.maximum(np.abs(yr), 1.0))
