"""GPU: gvk_ragged_minmax and gvk_conform_volumes (csrc/conform.hip) through ops.ragged_minmax, ops.conform_volumes and data.Conform,
against tests/conform_ref.py.

One batch of four volumes onto (10, 16, 24): (13, 22, 37) at spacing (1, 0.7, 0.6), cropped on one axis and downsampled on two;
(7, 9, 70) at (1.5, 2, 0.34), up-, up- and downsampled (a factor of 2.94: 12 taps); (10, 16, 24) at (1, 1, 1), already conforming;
(1, 5, 3) at (2, 1, 0.8), a length-1 axis and heavy padding.  The samples start at odd element offsets of the packed buffer (3, then gaps
of 1, 2 and 5 elements) and, in one run each, at the multiples of 4 that collate_ragged gives.  Values are normal around 40 +- 25 with
negatives, a -0.0, and per sample a lone extreme voxel on a face (-900 - 50 b: the minimum of that sample alone), so a wrong edge or pad
rule shows.

(a) Crop / pad / identity and nearest move bits: equality with conform_ref is bit for bit, the sign of zero included.
(b) Linear, with and without antialias, is compared with conform_ref.apply_tables, the float64 evaluation of the SAME float32 tables.
    The bound follows from the kernel's order of operations: a pass contracts one axis as v = w[0] x[0]; v = fmaf(w[t], x[t], v), K
    roundings of relative size u = 2^-24 on partial sums that stay within M = max(|x|, |pad|) (the weights are non-negative and sum to 1
    within K u), and stores v as the float32 it already is; the error an earlier pass left is carried through with weights that sum to 1.
    Over the three passes |got - ref| <= (K0 + K1 + K2) u M (1 + O(K u)), and the test asks 2 (K0 + K1 + K2) 2^-24 M per sample, K_a that
    sample's own band on axis a (1 on a gathered axis).  Nothing in it comes from a measurement.
(c) 'minimum' pads with the sample's own minimum (exactly), which for every sample differs from the batch's.
(d) the partials of gvk_ragged_minmax reduce to the exact min and max.   (e) two runs give the same bits.
(f) B = 1, and a batch whose widest band is 16 taps (a factor of 100 / 24 = 4.17).
(g) Conform, then eval_transforms() (the min-max rescale to [0, 1]) equals eval_transforms() of conform_ref's output within
    4 e / R + 4 * 2^-24, e the bound of (b) and R the range of the conformed sample: the subtraction sees 2 e (voxel and minimum), the
    division by a range that is itself off by 2 e another 2 e / R, and the rescale's own float32 steps may each round the other way.
Every test prints its measured maxima before it asserts (pytest -m gpu -s; profiles/conform_parity_report.txt is a copy of those lines)."""
import numpy as np
import pytest
import torch

import conform_ref
from gaviko_amd import lib, ops
from gaviko_amd.data import Conform, CropOrPad, RaggedBatch, Resample, Resize, collate_ragged, conform_tables, eval_transforms

pytestmark = pytest.mark.gpu

N = (10, 16, 24)
SHAPES = [(13, 22, 37), (7, 9, 70), (10, 16, 24), (1, 5, 3)]
SPACING = [(1.0, 0.7, 0.6), (1.5, 2.0, 0.34), (1.0, 1.0, 1.0), (2.0, 1.0, 0.8)]
U = 2.0 ** -24


def _volumes(shapes=SHAPES, seed=7):
    rng = np.random.default_rng(seed)
    vols = []
    for b, s in enumerate(shapes):
        v = (40.0 + 25.0 * rng.normal(size=s)).astype(np.float32)
        v.reshape(-1)[v.size // 2] = -0.0
        face = [0, s[1] // 2, s[2] - 1] if b % 2 else [s[0] - 1, 0, s[2] // 2]
        v[tuple(face)] = -900.0 - 50.0 * b                                # the lone extreme voxel on a face: this sample's own minimum
        vols.append(v)
    return vols


def _pack(vols, spacing, odd=True):
    """A RaggedBatch on the host: odd element offsets (gaps of 3, 1, 2, 5, ... elements filled with a value no sample holds), or collate's."""
    if not odd:
        return collate_ragged([(v, s) for v, s in zip(vols, spacing)])
    gaps, offsets, end = [3, 1, 2, 5, 7, 1], [], 0
    for i, v in enumerate(vols):
        offsets.append(end + gaps[i % len(gaps)])
        end = offsets[-1] + v.size
    data = np.full(end + 1, 12345.0, dtype=np.float32)
    for o, v in zip(offsets, vols):
        data[o:o + v.size] = v.reshape(-1)
    assert any(o % 2 for o in offsets) and any(o % 4 for o in offsets)
    return RaggedBatch(torch.from_numpy(data), torch.tensor(offsets + [end], dtype=torch.int64), torch.tensor([v.shape for v in vols], dtype=torch.int32),
                       torch.tensor(spacing, dtype=torch.float64))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _run(dev, conform, vols, spacing, odd=True):
    rb = _pack(vols, spacing, odd).to(dev)
    out = conform(rb)
    assert out.shape == (len(vols), 1) + tuple(conform.target_shape) and out.dtype == torch.float32 and out.is_cuda
    return out[:, 0].cpu().numpy()


def _pad_of(mode, v):
    return float(v.min()) if mode == "minimum" else float(mode)


@pytest.mark.parametrize("odd", [True, False])
@pytest.mark.parametrize("mode", [0, -3.5, "minimum"])
def test_crop_pad_identity_are_bit_exact(dev, mode, odd):
    vols = _volumes()
    got = _run(dev, Conform([CropOrPad(N, mode)]), vols, [(1, 1, 1)] * 4, odd)
    for b, v in enumerate(vols):
        want = conform_ref.conform(v, (1, 1, 1), None, None, N, pad=mode).astype(np.float32)
        assert np.array_equal(_bits(got[b]), _bits(want)), f"sample {b}"
    assert np.array_equal(_bits(got[2]), _bits(vols[2])) and (_bits(got[2]) == np.int32(-2 ** 31)).sum() == 1       # the -0.0 came through
    print(f"conform crop/pad pad={mode} odd_offsets={odd}: 4 volumes bit for bit")


@pytest.mark.parametrize("kind", ["resample", "resize"])
def test_nearest_is_bit_exact(dev, kind):
    vols = _volumes()
    stages = [Resample(1.0, "nearest"), CropOrPad(N, "minimum")] if kind == "resample" else [Resize(N, "nearest")]
    got = _run(dev, Conform(stages), vols, SPACING)
    for b, v in enumerate(vols):
        want = conform_ref.conform(v, SPACING[b], kind, (1.0,) * 3 if kind == "resample" else N, N, "nearest", pad="minimum").astype(np.float32)
        assert np.array_equal(_bits(got[b]), _bits(want)), f"sample {b}"
    print(f"conform nearest {kind}: 4 volumes bit for bit")


def _check_linear(got, vols, spacing, stages, mode, what):
    """(b): every sample within 2 (K0 + K1 + K2) u M of the float64 evaluation of the same float32 tables.  Returns the bounds."""
    target = Conform(stages).target_shape
    t = conform_tables([v.shape for v in vols], spacing, stages, target)
    worst, bounds = 0.0, []
    for b, v in enumerate(vols):
        pad = _pad_of(mode, v)
        want = conform_ref.apply_tables(v, [t.axis(b, a, target) for a in range(3)], pad)
        bound = 2.0 * int(t.taps[b].sum()) * U * max(float(np.abs(v).max()), abs(pad))
        err = float(np.abs(got[b].astype(np.float64) - want).max())
        worst = max(worst, err / bound)
        bounds.append(bound)
        print(f"conform {what} sample {b} {v.shape} taps {t.taps[b].tolist()}: max error {err:.3e} (bound {bound:.3e})")
        outside = ~(t.axis(b, 0, target)[2][:, None, None] & t.axis(b, 1, target)[2][None, :, None] & t.axis(b, 2, target)[2][None, None, :])
        assert np.array_equal(_bits(got[b][outside]), _bits(np.full(int(outside.sum()), pad, np.float32))), f"sample {b}: padding"
        assert err <= bound, f"sample {b}: {err} > {bound}"
    print(f"conform maxima: {what}: error / bound = {worst:.3e}")
    return bounds


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("mode", [0, "minimum"])
def test_linear_within_the_rounding_bound(dev, mode, antialias):
    vols = _volumes()
    stages = [Resample(1.0, "linear", antialias), CropOrPad(N, mode)]
    got = _run(dev, Conform(stages), vols, SPACING)
    _check_linear(got, vols, SPACING, stages, mode, f"linear antialias={antialias} pad={mode}")
    assert np.array_equal(_bits(got[2]), _bits(vols[2]))                   # the conforming sample rides along bit for bit
    # and the definitions themselves (plain loops, no tables): rounding the weights to float32 moves a row's sum by at most K u M / 2 per
    # axis, so twice the bound of (b) covers both
    t = conform_tables(SHAPES, SPACING, stages, N)
    for b, v in enumerate(vols):
        want = conform_ref.conform(v, SPACING[b], "resample", (1.0,) * 3, N, "linear", antialias, pad=mode)
        assert np.abs(got[b] - want).max() <= 4.0 * int(t.taps[b].sum()) * U * float(np.abs(v).max())


def test_minimum_padding_is_the_samples_own_minimum(dev):
    vols = _volumes()
    mins = [float(v.min()) for v in vols]
    assert len(set(mins)) == 4 and all(m == -900.0 - 50.0 * b for b, m in enumerate(mins))     # no two samples share it; the batch's is sample 3's
    conform = Conform([Resample(1.0), CropOrPad(N, "minimum")])
    got = _run(dev, conform, vols, SPACING)
    t = conform_tables(SHAPES, SPACING, conform.transforms, N)
    for b in (0, 1, 3):
        outside = ~(t.axis(b, 0, N)[2][:, None, None] & t.axis(b, 1, N)[2][None, :, None] & t.axis(b, 2, N)[2][None, None, :])
        assert outside.any() and (got[b][outside] == np.float32(mins[b])).all()
    assert conform.last_geometry.shape == (4, 3, 2) and conform.last_geometry[3].tolist() == [[0.5, 4.0], [1.0, 6.0], [1.25, 11.0]]
    print("conform minimum padding: 3 padded samples carry their own minimum exactly")


@pytest.mark.parametrize("odd", [True, False])
def test_ragged_minmax_is_exact(dev, odd):
    vols = _volumes() + [np.array([[[5.0, -7.0]]], dtype=np.float32)]                          # and a sample smaller than the slab count
    rb = _pack(vols, SPACING + [(1, 1, 1)], odd)
    part = ops.ragged_minmax(rb.data.to(dev), rb.offsets.numpy(), rb.shapes.numpy())
    part = part.cpu().numpy().reshape(len(vols), -1, 2)
    assert part.shape[1] * 2 == lib.load().gvk_minmax_partials()
    for b, v in enumerate(vols):
        assert part[b, :, 0].min() == v.min() and part[b, :, 1].max() == v.max(), f"sample {b}"
    print(f"conform ragged_minmax odd_offsets={odd}: 5 samples exact")


def test_two_runs_give_the_same_bits(dev):
    vols = _volumes()
    conform = Conform([Resample(1.0), CropOrPad(N, "minimum")])
    a, b = _run(dev, conform, vols, SPACING), _run(dev, conform, vols, SPACING)
    assert np.array_equal(_bits(a), _bits(b))
    aligned = _run(dev, conform, vols, SPACING, odd=False)                # where a sample starts changes nothing
    assert np.array_equal(_bits(a), _bits(aligned))
    print("conform determinism: two runs and both packings give the same bits")


def test_one_sample_and_a_sixteen_tap_batch(dev):
    vols = _volumes()
    for b in range(4):                                                    # B = 1: each sample alone gives what it gives in the batch
        stages = [Resample(1.0), CropOrPad(N, 0)]
        alone = _run(dev, Conform(stages), vols[b:b + 1], SPACING[b:b + 1])
        _check_linear(alone, vols[b:b + 1], SPACING[b:b + 1], stages, 0, f"B=1 sample {b}")
    shapes = [(9, 12, 100), (10, 16, 24), (31, 16, 50)]
    wide = _volumes(shapes, seed=11)
    stages = [Resize(N)]
    t = conform_tables(shapes, [(1, 1, 1)] * 3, stages, N)
    assert t.weights.shape[2] == 16 == ops.CONFORM_MAX_TAPS and t.taps.tolist() == [[2, 2, 16], [1, 1, 1], [12, 1, 8]]
    got = _run(dev, Conform(stages), wide, [(1, 1, 1)] * 3)
    _check_linear(got, wide, [(1, 1, 1)] * 3, stages, 0, "T=16 batch")


def test_conform_then_eval_transforms(dev):
    vols = _volumes()
    stages = [Resample(1.0), CropOrPad(N, "minimum")]
    conform, norm = Conform(stages), eval_transforms()
    x = conform(_pack(vols, SPACING).to(dev))
    got = norm(x)[:, 0].cpu().numpy()
    t = conform_tables(SHAPES, SPACING, stages, N)
    ref = np.stack([conform_ref.apply_tables(v, [t.axis(b, a, N) for a in range(3)], float(v.min())) for b, v in enumerate(vols)]).astype(np.float32)
    want = norm(torch.from_numpy(ref).to(dev).unsqueeze(1))[:, 0].cpu().numpy()
    worst = 0.0
    for b, v in enumerate(vols):
        e = 2.0 * int(t.taps[b].sum()) * U * float(np.abs(v).max())
        bound = 4.0 * e / float(ref[b].max() - ref[b].min()) + 4.0 * U
        err = float(np.abs(got[b].astype(np.float64) - want[b]).max())
        worst = max(worst, err / bound)
        print(f"conform + rescale sample {b}: max error {err:.3e} (bound {bound:.3e})")
        assert err <= bound and got[b].min() == 0.0 and got[b].max() == 1.0
    print(f"conform maxima: conform + rescale: error / bound = {worst:.3e}")


def test_out_of_range_arguments_are_refused_on_the_host(dev):
    vols = _volumes()
    rb = _pack(vols, SPACING).to(dev)
    off, shp = rb.offsets.numpy(), rb.shapes.numpy()
    t = conform_tables(SHAPES, SPACING, [Resample(1.0), CropOrPad(N)], N)
    args = lambda **kw: {**dict(data=rb.data, offsets=off, shapes=shp, start=t.start, weights=t.weights, inside=t.inside, taps=t.taps,  # noqa: E731
                                target_shape=N), **kw}
    start = t.start.copy()
    start[1, 10 + 16 + 23] += 1                                            # the last W row of sample 1 would read one voxel past its line
    for bad in (args(start=start), args(offsets=off + 2), args(shapes=shp + [[0, 0, 1]]), args(taps=t.taps + 20), args(target_shape=(10, 16)),
                args(weights=t.weights[:, :, :1]), args(inside=t.inside[:, :-1]), args(out=torch.empty(7, device=dev))):
        with pytest.raises(lib.GavikoHipError):
            ops.conform_volumes(**bad)
    with pytest.raises(lib.GavikoHipError):
        ops.ragged_minmax(rb.data, off + 2, shp)
    with pytest.raises(lib.GavikoHipError):
        ops.ragged_minmax(rb.data, off, shp, partials=torch.empty(8, device=dev))
