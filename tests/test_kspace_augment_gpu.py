"""GPU: the kernels of gaviko_amd/csrc/kspace.hip through ops and data against tests/kspace_ref.py -- ghosting against the literal np.fft
spectrum edit, spikes against the float64 closed form, gamma against float64 np.power, anisotropy bit for bit against the float32
restatement of its stated formula -- and the train_transforms(intensity=True, artifacts=True) pipeline against the numpy pipeline rebuilt
from its recorded draws.  Every test prints its figures before it asserts.

Bounds (the references are float64, so all of it is the kernels' fp32 error), elementwise:
* ghosting  |got - ref| <= (N + 2) 2^-24 (|c| (*) |x|): the standard forward bound of an fp32 dot product of N terms in any order; the + 2
  covers the float32 rounding of the table.  The right-hand side is computed in float64 from the float32 table (the form of _dot_bound in
  tests/test_motion_augment_gpu.py), plus the reference's own error, 64 log2(V) 2^-53 max|x| for the two float64 transforms of V voxels: it
  only matters where the exact answer, and with it the first term, is zero (a single nonzero line).  Raw intensities of ~1e3: an operand rounded to bf16 (2^-9 relative) misses it by orders of magnitude.
* spike     with e = 2^-24: a table entry is within e of cos / sin; a product of two entries within 3e; p = c1 c2 - s1 s2 and q within 7e;
  c0 p and s0 q within 9e; their difference within 19e; the sum of S such terms within (19 S + S^2) e; scale = float32(g |mean|) and the
  product scale * sum add 2 S e |scale|; the final add rounds once: |got - ref| <= 1.01 |scale| (21 S + S^2) e + e |ref| + S g V 2^-53 mean|x|
  (1.01: second-order terms; the last term: the float64 mean of the device and numpy's are sums in different orders).
* gamma     GAMMA_ULP_BOUND ulps of the float32 result: 4x the largest error measured over x in [1e-6, 4e3] and gamma = exp(-0.3), exp(0.3)
  (profiles/kspace_timing.txt), rounded up to a power of two -- powf's error is the device library's, not this package's.
"""
import numpy as np
import pytest
import torch

import intensity_ref
import kspace_ref
from oracle import data_ref

pytestmark = pytest.mark.gpu

SHAPES = [(5, 12, 68), (3, 7, 33), (16, 20, 72), (2, 3, 20)]          # tile tails, odd extents, extents below one 16-tile, several workgroups
GAMMA_ULP_BOUND = 8.0                                                 # measured 1.265 ulp; 4 x 1.265 = 5.06, rounded up to a power of two
E = 2.0 ** -24


def _vol(shape, seed):
    return (np.random.default_rng(seed).standard_normal(shape) * 300 + 1000).astype(np.float32)


def _ramp(shape):
    i0, i1, i2 = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return (i0 * 1e4 + i1 * 1e2 + i2).astype(np.float32)               # exact in float32; every voxel names its own index


def _line(shape, axis):
    x = np.zeros(shape, dtype=np.float32)
    idx = [n // 3 for n in shape]
    idx[axis] = slice(None)
    x[tuple(idx)] = np.arange(1, shape[axis] + 1, dtype=np.float32) * 100                  # one nonzero line along the convolved axis
    return x


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ghost(dev, vols, n, g, axis, live=None):
    from gaviko_amd import data, ops
    B, shape = len(vols), vols.shape[1:]
    ctab = data.ghosting_tables(n, g, [shape[a] for a in axis])
    x = _t(vols, dev)
    out = torch.full_like(x, float("nan"))
    lv = np.ones(B, np.int32) if live is None else np.asarray(live, np.int32)
    ops.axis_circular_conv(x, out, _t(ctab, dev), _t(np.asarray(axis, np.int32), dev), _t(lv, dev))
    return out.cpu().numpy(), ctab


def _ghost_bound(c, vol, axis):
    N = vol.shape[axis]
    return (N + 2) * E * kspace_ref.abs_circular_conv(vol, c, axis) + 64 * 2.0 ** -53 * np.log2(vol.size) * np.abs(vol).max()


def _report(tag, got, ref, bound):
    err = np.abs(got - ref)
    worst = (err / np.maximum(bound, 1e-300)).max()
    print(f"{tag}: max err {err.max():.3e}  smallest bound {bound.min():.3e}  largest err / bound {worst:.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (tag, err.max(), worst)


# ------------------------------------------------------------------------------------------------ ghosting
def _check_ghosting_vs_fft(dev, shape, axis):
    vols = np.stack([_vol(shape, 10 + axis), _ramp(shape), _line(shape, axis), _vol(shape, 20 + axis)])
    n, g = [2, 3, 1, 7], [0.7, 1.0, 0.9, 0.55]                           # n dividing and not dividing the extent, n = 1, g = 1
    got, ctab = _ghost(dev, vols, n, g, [axis] * 4)
    for b in range(4):
        ref = kspace_ref.ghosting_fft(vols[b], n[b], axis, g[b])
        _report(f"ghosting {shape} axis {axis} sample {b} n {n[b]} g {g[b]}", got[b], ref, _ghost_bound(ctab[b], vols[b], axis))
    assert np.abs(got[0] - vols[0]).max() > 10.0                         # an artifact, not a copy


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_ghosting_vs_fft(dev, shape, axis):
    _check_ghosting_vs_fft(dev, shape, axis)


# 240 voxels on the convolved axis: 15 tiles, all 8 accumulators of a wave live, the second wave pair one tile past the axis
@pytest.mark.parametrize("shape,axis", [((2, 3, 240), 2), ((240, 2, 4), 0), ((2, 240, 4), 1)])
def test_ghosting_vs_fft_with_eight_accumulators(dev, shape, axis):
    _check_ghosting_vs_fft(dev, shape, axis)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ghosting_at_the_real_extent(dev, axis):
    shape = (120, 160, 160)
    for tag, vol, n, g in (("random", _vol(shape, 30 + axis), 6, 0.8), ("ramp", _ramp(shape), 4, 1.0)):
        got, ctab = _ghost(dev, vol[None], [n], [g], [axis])
        _report(f"ghosting {shape} axis {axis} {tag}", got[0], kspace_ref.ghosting_fft(vol, n, axis, g), _ghost_bound(ctab[0], vol, axis))


def test_ghosting_mixed_batch_in_one_launch(dev):
    shape = (16, 20, 72)
    vols = np.stack([_vol(shape, 40 + b) for b in range(4)])
    vols[3, 0, 0, :4] = [-0.0, 0.0, np.float32(1e-42), -np.float32(3e38)]           # the dead sample keeps signed zeros, subnormals, large values
    vols[3, -1, -1, -3:] = [np.float32(1e-42), -0.0, -np.float32(3e38)]
    n, g, axis, live = [4, 5, 3, 2], [0.6, 0.9, 1.0, 0.7], [0, 1, 2, 1], [1, 1, 1, 0]
    got, ctab = _ghost(dev, vols, n, g, axis, live)
    same = np.array_equal(got[3].view(np.uint32), vols[3].view(np.uint32))
    print(f"mixed: dead sample bit-identical: {same}")
    assert same
    for b in range(3):
        _report(f"mixed: sample {b} axis {axis[b]}", got[b], kspace_ref.ghosting_fft(vols[b], n[b], axis[b], g[b]), _ghost_bound(ctab[b], vols[b], axis[b]))
    again, _ = _ghost(dev, vols, n, g, axis, live)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))               # no atomics: the same bits on every run


# ------------------------------------------------------------------------------------------------ gamma and spikes
def _gamma_spike(dev, vols, kind, gamma=None, amp=None, positions=None):
    from gaviko_amd import data, ops
    B, shape = len(vols), vols.shape[1:]
    x = _t(vols, dev)
    out = torch.full_like(x, float("nan"))
    tab, nsp = np.zeros((B, ops.SPIKE_MAX, 2, sum(shape)), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        if positions is not None and positions[b] is not None:
            tab[b], nsp[b] = data.spike_tables(positions[b], shape), len(positions[b])
    stats, _ = ops.volume_stats(x, None, want_std=False)
    ops.gamma_spike(x, out, _t(np.asarray(kind, np.int32), dev), _t(np.ones(B, np.float32) if gamma is None else np.asarray(gamma, np.float32), dev),
                    _t(np.zeros(B, np.float32) if amp is None else np.asarray(amp, np.float32), dev), _t(nsp, dev), _t(tab, dev), stats)
    return out.cpu().numpy()


def _spike_bound(vol, positions, g, ref):
    S = len(positions)
    scale = kspace_ref.spike_amplitude(vol, g)
    return 1.01 * abs(scale) * (21 * S + S * S) * E + E * np.abs(ref) + S * abs(g) * vol.size * 2.0 ** -53 * np.abs(vol.astype(np.float64)).mean()


@pytest.mark.parametrize("shape", [(5, 12, 68), (3, 7, 33)])
def test_spike_vs_closed_form(dev, shape):
    from gaviko_amd import ops
    last = 1 - 2.0 ** -30
    positions = [[(0.31, 0.77, 0.52)],                                                                  # S = 1
                 [(0.0, 0.0, 0.0), (last, last, last), (0.0, last, 0.4), (0.62, 0.0, last)],            # S = 4; index 0 and the last index of each axis
                 [(last, 0.5, 0.0), (0.13, 0.98, 0.5)],
                 None]
    g = np.array([2.5, -1.5, 3.0, 2.0], np.float32)
    vols = np.stack([_vol(shape, 50), _vol(shape, 51), _vol(shape, 52) - 2000, _vol(shape, 53)])        # sample 2: a negative mean
    vols[3, 0, 0, :3] = [-0.0, np.float32(1e-42), -np.float32(3e38)]
    kind = [ops.KSPACE_SPIKE] * 3 + [ops.KSPACE_COPY]
    got = _gamma_spike(dev, vols, kind, amp=g, positions=positions)
    assert np.array_equal(got[3].view(np.uint32), vols[3].view(np.uint32))
    for b in range(3):
        ref, total = kspace_ref.spike_cosine(vols[b], positions[b], g[b])
        print(f"spike {shape} sample {b}: indices {kspace_ref.spike_indices(positions[b], shape)} mean {vols[b].mean():.1f} largest stripe "
              f"{np.abs(ref - vols[b]).max():.1f}")
        _report(f"spike {shape} sample {b} S {len(positions[b])}", got[b], ref, _spike_bound(vols[b], positions[b], float(g[b]), ref))
        assert np.abs(got[b] - vols[b]).max() > 100.0
    again = _gamma_spike(dev, vols, kind, amp=g, positions=positions)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def gamma_ulp_error(dev):
    """(largest error in ulps of the float32 result, the x and gamma where it occurs) over x in [1e-6, 4e3] and gamma = exp(-0.3), exp(0.3)"""
    from gaviko_amd import ops
    shape = (8, 64, 256)
    x = np.exp(np.random.default_rng(60).uniform(np.log(1e-6), np.log(4e3), (2,) + shape)).astype(np.float32)
    x[:, 0, 0, :2] = [1e-6, 4e3]
    gam = np.array([np.exp(-0.3), np.exp(0.3)], np.float32)
    got = _gamma_spike(dev, x, [ops.KSPACE_GAMMA] * 2, gamma=gam)
    worst = (0.0, None, None)
    for b in range(2):
        ref = kspace_ref.gamma(x[b], gam[b])
        ulps = np.abs(got[b].astype(np.float64) - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        i = np.unravel_index(np.argmax(ulps), shape)
        if ulps[i] > worst[0]:
            worst = (float(ulps[i]), float(x[b][i]), float(gam[b]))
    return worst


def test_gamma_vs_float64_power(dev):
    from gaviko_amd import ops
    ulps, at_x, at_gamma = gamma_ulp_error(dev)
    print(f"gamma: largest error {ulps:.3f} ulp at x = {at_x!r}, gamma = {at_gamma!r}; bound {GAMMA_ULP_BOUND}")
    assert ulps <= GAMMA_ULP_BOUND
    # exact cases: zeros keep their sign, negatives mirror the positives, gamma == 1 is the identity bit for bit
    shape = (3, 7, 33)
    v = _vol(shape, 61) - 1000
    v[0, 0, :6] = [0.0, -0.0, 2.0, -2.0, np.float32(1e-42), -np.float32(3e38)]
    vols = np.stack([v, v, -v])
    got = _gamma_spike(dev, vols, [ops.KSPACE_GAMMA] * 3, gamma=[1.0, np.exp(0.3), np.exp(0.3)])
    assert np.array_equal(got[0].view(np.uint32), v.view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), (-got[2]).view(np.uint32))                          # sign(x) |x|^gamma is odd
    assert np.array_equal(got[1][0, 0, :2].view(np.uint32), np.array([0.0, -0.0], np.float32).view(np.uint32))
    assert (np.signbit(got[1]) == np.signbit(v)).all()                                               # also where a subnormal underflows to zero
    ref = kspace_ref.gamma(v, np.float32(np.exp(0.3)))
    finite = np.abs(v) < 1e30
    err = np.abs(got[1].astype(np.float64) - ref)[finite] / np.spacing(np.abs(ref[finite]).astype(np.float32))
    print(f"gamma on a signed volume: largest error {err.max():.3f} ulp")
    assert err.max() <= GAMMA_ULP_BOUND


# ------------------------------------------------------------------------------------------------ anisotropy
@pytest.mark.parametrize("shape", SHAPES)
def test_anisotropy_bit_exact(dev, shape):
    from gaviko_amd import data, ops
    cases = [(a, f) for a in (0, 1, 2) for f in (1.0, 1.5, 5.0, 400.0)] + [(1, 2.0)]                   # the last one is dead
    B, n_max = len(cases), max(shape)
    vols = np.random.default_rng(70).integers(0, 4096, (B,) + shape).astype(np.float32)               # integer-valued: kspace_ref.anisotropy
    vols[0, 0, 0, :2] = [-0.0, -7.0]
    vols[-1, 0, 0, :3] = [-0.0, np.float32(1e-42), -np.float32(3e38)]
    src, w = np.zeros((B, n_max, 2), np.int32), np.zeros((B, n_max), np.float32)
    for b, (a, f) in enumerate(cases):
        src[b], w[b] = data.anisotropy_tables(f, shape[a], n_max)
    live = np.ones(B, np.int32)
    live[-1] = 0
    x = _t(vols, dev)
    out = torch.full_like(x, float("nan"))
    ops.axis_gather2(x, out, _t(src, dev), _t(w, dev), _t(np.array([a for a, _ in cases], np.int32), dev), _t(live, dev))
    got = out.cpu().numpy()
    for b, (a, f) in enumerate(cases[:-1]):
        ref = kspace_ref.anisotropy(vols[b], a, f)
        same = np.array_equal(got[b].view(np.uint32), ref.view(np.uint32))
        print(f"anisotropy {shape} axis {a} f {f}: bit-identical {same}, changed voxels {(got[b] != vols[b]).sum()}")
        assert same, (a, f, np.abs(got[b] - ref).max())
        if f == 1.0:
            assert np.array_equal(got[b].view(np.uint32), vols[b].view(np.uint32))
        if f > max(shape):                                                                             # one low sample: constant lines
            assert (np.moveaxis(got[b], a, 0) == np.moveaxis(got[b], a, 0)[:1]).all()
    assert np.array_equal(got[-1].view(np.uint32), vols[-1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections(dev):
    from gaviko_amd import data, lib, ops
    one = torch.ones(1, dtype=torch.int32, device=dev)
    ctab = torch.zeros(1, ops.AXIS_CONV_MAX_N, device=dev)
    for shape in ((1, 4, 8), (4, 1, 8), (4, 8, 1), (257, 2, 4), (2, 257, 4), (2, 4, 257)):
        x = torch.zeros((1,) + shape, device=dev)
        out = torch.full_like(x, float("nan"))
        with pytest.raises(lib.GavikoHipError, match=r"2\.\.256 voxels on the convolved axis are built"):
            ops.axis_circular_conv(x, out, ctab, one, one)
        assert torch.isnan(out).all()
    x = torch.zeros(1, 4, 6, 8, device=dev)
    out = torch.full_like(x, float("nan"))
    flat = torch.zeros(2 * x.numel(), device=dev)
    part = (flat[:x.numel()].view_as(x), flat[x.numel() // 2:x.numel() // 2 + x.numel()].view_as(x))      # partly overlapping views of one buffer
    src, w = torch.zeros(1, 8, 2, dtype=torch.int32, device=dev), torch.zeros(1, 8, device=dev)
    f1, i1 = torch.ones(1, device=dev), one
    tab, stats = torch.zeros(1, ops.SPIKE_MAX, 2, 18, device=dev), torch.zeros(1, ops.NORMALIZE_STATS, dtype=torch.float64, device=dev)
    for a, b in ((x, x), part):
        with pytest.raises(lib.GavikoHipError, match="must not overlap"):
            ops.axis_circular_conv(a, b, ctab, one, one)
        with pytest.raises(lib.GavikoHipError, match="must not overlap"):
            ops.gamma_spike(a, b, i1, f1, f1, i1, tab, stats)
        with pytest.raises(lib.GavikoHipError, match="must not overlap"):
            ops.axis_gather2(a, b, src, w, one, one)
    with pytest.raises(lib.GavikoHipError, match="null pointer"):
        ops.axis_circular_conv(x, out, None, one, one)
    with pytest.raises(lib.GavikoHipError, match="null pointer"):
        ops.gamma_spike(x, out, i1, f1, f1, i1, None, stats)
    with pytest.raises(lib.GavikoHipError, match="null pointer"):
        ops.gamma_spike(x, out, i1, f1, f1, i1, tab, None)
    with pytest.raises(lib.GavikoHipError, match="expected"):
        ops.axis_gather2(x, out, None, w, one, one)
    with pytest.raises(lib.GavikoHipError, match="table rows of 7 entries"):
        ops.axis_gather2(x, out, src[:, :7].contiguous(), w[:, :7].contiguous(), one, one)
    with pytest.raises(lib.GavikoHipError, match="needs >="):
        ops.gamma_spike(x, out, i1, f1, f1, i1, tab[:, :, :, :17].contiguous(), stats)
    with pytest.raises(NotImplementedError, match="1..4 are built"):
        data.RandomSpike(num_spikes=5)
    with pytest.raises(ValueError, match="1..4 are built"):
        data.spike_tables(np.full((5, 3), 0.5), (4, 6, 8))
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and not x.any() and not flat.any()                # nothing was launched


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.mark.parametrize("PIPELINE_SEED", [9, 41])
def test_train_transforms_artifacts_pipeline(dev, PIPELINE_SEED):
    """train_transforms(seed, intensity=True, artifacts=True) on (4, 1, 8, 12, 20) against oracle.data_ref spatial + intensity_ref / kspace_ref +
    rescale rebuilt from last_params and last_intensity.  The seeds were picked on the CPU from the draws alone (sampling is host-side): 9 draws
    gamma, ghosting, nothing and anisotropy behind a live affine, 41 gamma, a spike, gamma and anisotropy.  Bound per volume as in tests/test_motion_augment_gpu.py: the kernel's bound over
    (max - min) plus 2e-3 where an affine resampling is live; the kernel's bound is the module docstring's for the new kinds (one float32 ulp
    for anisotropy, whose blend is exact up to its single rounding) plus the 2e-5 max|x| that test grants the rescale."""
    from gaviko_amd import data
    shape, B = (8, 12, 20), 4
    vols = np.stack([_vol(shape, 80 + b) for b in range(B)])[:, None]
    x = _t(vols, dev)
    tf = data.train_transforms(seed=PIPELINE_SEED, intensity=True, artifacts=True)
    y = tf(x).cpu().numpy()
    drawn = [d[0] if d else None for d in tf.last_intensity]
    print("pipeline draws:", drawn, [bits | (8 if aff is not None else 0) for bits, aff in tf.last_params])
    new = {"RandomGhosting", "RandomSpike", "RandomGamma", "RandomAnisotropy"}
    assert len(set(drawn) & new) >= 3
    assert np.isfinite(y).all() and y.min() >= 0.0 and y.max() <= 1.0
    for b, ((bits, aff), draw) in enumerate(zip(tf.last_params, tf.last_intensity)):
        mat = None if aff is None else data.affine_matrix(*aff, shape).astype(np.float32)
        moved = data_ref.spatial(vols[b, 0], mat, bits)
        if draw and draw[0] in new:
            pre = kspace_ref.apply(moved, draw)
            p = draw[1]
            if draw[0] == "RandomGhosting":
                kb = _ghost_bound(data.ghosting_tables([p["num_ghosts"]], [p["intensity"]], [shape[p["axis"]]])[0], moved, p["axis"])
            elif draw[0] == "RandomSpike":
                kb = _spike_bound(moved, p["positions"], float(np.float32(p["intensity"])), pre)
            elif draw[0] == "RandomGamma":
                kb = GAMMA_ULP_BOUND * 2.0 ** -23 * np.abs(pre)
            else:
                kb = 2.0 ** -23 * np.abs(pre)
            kernel_bound = kb + 2e-5 * np.abs(pre).max()
        else:
            pre = intensity_ref.apply(moved, draw)
            top = np.abs(pre).max()
            std = draw[1]["std"] if draw and draw[0] == "RandomNoise" else 0.0
            kernel_bound = 1e-5 * top + (2e-5 * std + 2.0 ** -22 * top) + 2e-5 * top
        want = data_ref.rescale_intensity(pre.astype(np.float32))
        bound = kernel_bound / (pre.max() - pre.min()) + (2e-3 if aff is not None else 0.0)
        err = np.abs(y[b, 0] - want)
        print(f"pipeline sample {b} {drawn[b]} affine {aff is not None}: max err {err.max():.3e}  smallest bound {np.min(bound):.3e}  "
              f"largest err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), (b, drawn[b], err.max())
    y2 = data.train_transforms(seed=PIPELINE_SEED, intensity=True, artifacts=True)(x).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32))                     # the seed reproduces the batch
