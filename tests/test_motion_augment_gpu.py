"""GPU: the fused RandomMotion kernel (gaviko_amd/csrc/motion.hip) through ops.motion_artifact against torchio's compositing written
literally with np.fft in float64 (tests/motion_ref.py), and the train_transforms(intensity=True, motion=True) pipeline against the numpy
pipeline rebuilt from its recorded draws.  Inputs are randn * 300 + 1000 in fp32.  Every test prints its figures before it asserts.

Bounds (the reference is float64, so all of it is the kernel's fp32 error), elementwise:
* exact   |got - ref| <= ((K+1) W + 2) 2^-24 sum_s (|c_s| (*) |img_s|): the standard forward bound of an fp32 dot product of (K+1) W terms in
  any order; the + 2 covers the float32 rounding of the table.  The right-hand side is computed in float64 from the float32 table.  With
  rotations 0 and integer translations the trilinear weights are exactly 0 or 1, so the moved images are exact shifts padded with the
  minimum, built that way in numpy.
* rotated the same plus 1e-3 max|x| sum_{s>=1} ||c_s||_1: 1e-3 max|x| is what tests/test_data_metrics.py::test_spatial_transform_vs_oracle
  grants this resampling arithmetic against this oracle (oracle.data_ref.affine_resample), the L1 norm its amplification by the convolution.
"""
import functools

import numpy as np
import pytest
import torch

import intensity_ref
import motion_ref
from oracle import data_ref

pytestmark = pytest.mark.gpu


def _vol(shape, seed):
    return (np.random.default_rng(seed).standard_normal(shape) * 300 + 1000).astype(np.float32)


def _partials(x):
    """gvk_volume_minmax of x; it reads 16-byte words, so a volume whose size is no multiple of 4 gets the same table filled by torch."""
    from gaviko_amd import ops
    B = x.shape[0]
    part = ops.minmax_partials(B, x.device)
    if (x.numel() // B) % 4 == 0:
        ops.volume_minmax(x, part)
    else:
        flat = x.reshape(B, -1)
        part.view(B, -1, 2)[:, :, 0] = flat.min(dim=1).values[:, None]
        part.view(B, -1, 2)[:, :, 1] = flat.max(dim=1).values[:, None]
    return part


def _motion(dev, vols, degrees, translation, times, live=None):
    """vols [B][D][H][W], degrees / translation [B][K][3], times [B][K] -> (out [B][D][H][W], ctab float32 [B][K+1][W])"""
    from gaviko_amd import data, ops
    B, shape = len(vols), vols.shape[1:]
    K = len(times[0])
    mats = np.stack([np.stack([data.affine_matrix((1, 1, 1), degrees[b][k], translation[b][k], shape).astype(np.float32) for k in range(K)])
                     for b in range(B)])
    ctab, _ = data.motion_tables(times, shape[-1])
    x = torch.from_numpy(vols).to(dev)
    out = torch.full_like(x, float("nan"))
    lv = np.ones(B, np.int32) if live is None else np.asarray(live, np.int32)
    ops.motion_artifact(x, out, torch.from_numpy(mats).to(dev), torch.from_numpy(ctab).to(dev), torch.from_numpy(lv).to(dev), _partials(x), K)
    return out.cpu().numpy(), ctab


def _dot_bound(ctab, images):
    K1, W = ctab.shape
    return (K1 * W + 2) * 2.0 ** -24 * motion_ref.abs_convolution(ctab, images)


def _rot_bound(ctab, images):
    return _dot_bound(ctab, images) + 1e-3 * np.abs(images[0]).max() * np.abs(ctab[1:].astype(np.float64)).sum()


def _shifted(vol, tr):
    """vol moved by the integer vector tr (out[q] = vol[q - tr]), voxels that come from outside read the minimum"""
    out = np.full_like(vol, vol.min())
    dst, src = [], []
    for n, t in zip(vol.shape, tr):
        t = int(t)
        dst.append(slice(max(0, t), max(0, min(n, n + t))))
        src.append(slice(max(0, -t), max(0, min(n, n - t))))
    out[tuple(dst)] = vol[tuple(src)]
    return out


def _report(tag, got, ref, bound):
    err = np.abs(got - ref)
    worst = (err / bound).max()
    print(f"{tag}: max err {err.max():.3e}  smallest bound {bound.min():.3e}  largest err / bound {worst:.3f}")
    assert np.isfinite(got).all() and (err <= bound).all(), (tag, err.max(), worst)


# ------------------------------------------------------------------------------------------------ exact shifts
# shape, times per sample, translations per sample [K][3]: signs mixed, one component larger than its extent in most cases
EXACT = [
    ((5, 12, 68), [[0.3, 0.7], [0.25, 0.45], [0.55, 0.8]],                                           # line tile tail (60 lines), W no multiple of 32
     [[(1, -2, 3), (7, 0, -5)], [(0, 3, -70), (-2, -1, 4)], [(-1, 13, 0), (2, 2, 2)]]),
    ((16, 20, 72), [[0.2, 0.5, 0.77], [0.26, 0.52, 0.74]],                                            # K = 3, several workgroups
     [[(1, 0, 0), (0, -4, 9), (-17, 2, -3)], [(3, 3, -3), (0, 0, 80), (-1, 1, 1)]]),
    ((3, 7, 33), [[0.3], [0.7]], [[(1, -1, 5)], [(-4, 2, -6)]]),                                      # K = 1 on both sides of 0.5; odd W; 21 lines; V % 4 != 0
    ((2, 3, 20), [[0.31, 0.34], [0.3, 0.7]], [[(0, 1, -2), (1, 0, 3)], [(-1, -1, 1), (0, 4, -1)]]),   # W below one tile pair; an empty slab
    ((2, 3, 240), [[0.3], [0.7]], [[(1, -1, 5)], [(0, 2, -250)]]),                                    # 15 column tiles: 8 accumulators per wave, the
]                                                                                                     # second wave pair one tile past the line


def _check_exact(dev, shape, times, trans, tag):
    B, K = len(times), len(times[0])
    vols = np.stack([_vol(shape, 100 + b) for b in range(B)])
    got, ctab = _motion(dev, vols, np.zeros((B, K, 3)), trans, times)
    for b in range(B):
        images = [vols[b]] + [_shifted(vols[b], tr) for tr in trans[b]]
        _report(f"exact {tag} K {K} sample {b} times {times[b]}", got[b], motion_ref.composite(images, times[b]), _dot_bound(ctab[b], images))


@pytest.mark.parametrize("shape,times,trans", EXACT)
def test_exact_shifts_vs_fft_composite(dev, shape, times, trans):
    _check_exact(dev, shape, times, trans, shape)


def test_exact_shifts_at_the_real_extent(dev):
    _check_exact(dev, (120, 160, 160), [[0.3, 0.7]], [[(3, -7, 11), (-125, 4, -2)]], "(120, 160, 160)")


# ------------------------------------------------------------------------------------------------ rotations
@functools.lru_cache(maxsize=None)
def _rotated_case(shape, seed):
    """(vols, degrees, translation, times, per-sample (images, reference)) of a 2-sample batch; computed once, shared, never modified"""
    rng = np.random.default_rng(seed)
    B, K = 2, 2
    vols = np.stack([_vol(shape, seed + 1 + b) for b in range(B)])
    deg, tr = rng.uniform(-10, 10, (B, K, 3)), rng.uniform(-6.5, 6.5, (B, K, 3))
    times = [[0.3, 0.7], [0.27, 0.61]]
    refs = []
    for b in range(B):
        images = motion_ref.moved_images(vols[b], deg[b], tr[b])
        refs.append((images, motion_ref.composite(images, times[b])))
    return vols, deg, tr, times, refs


@pytest.mark.parametrize("shape", [(16, 20, 72), (24, 32, 64)])
def test_rotations_vs_oracle_resample_and_fft_composite(dev, shape):
    vols, deg, tr, times, refs = _rotated_case(shape, 200)
    got, ctab = _motion(dev, vols, deg, tr, times)
    for b, (images, ref) in enumerate(refs):
        _report(f"rotated {shape} sample {b}", got[b], ref, _rot_bound(ctab[b], images))
        assert np.abs(got[b] - vols[b]).max() > 10.0                                # it is an artifact, not a copy


# ------------------------------------------------------------------------------------------------ live and dead samples in one launch
def test_mixed_batch_in_one_launch(dev):
    shape = (16, 20, 72)
    vols2, deg2, tr2, times2, refs = _rotated_case(shape, 200)
    vols = np.stack([vols2[0], _vol(shape, 301), vols2[1], _vol(shape, 303)])
    vols[1, 0, 0, :4] = [-0.0, 0.0, np.float32(1e-42), -np.float32(3e38)]           # a dead sample keeps signed zeros, subnormals, large values
    vols[3, -1, -1, -3:] = [np.float32(1e-42), -0.0, -np.float32(3e38)]
    deg = np.stack([deg2[0], deg2[0], deg2[1], deg2[1]])
    tr = np.stack([tr2[0], tr2[0], tr2[1], tr2[1]])
    times = [times2[0], [0.3, 0.7], times2[1], [0.3, 0.7]]
    got, ctab = _motion(dev, vols, deg, tr, times, live=[1, 0, 1, 0])
    for b in (1, 3):
        same = np.array_equal(got[b].view(np.uint32), vols[b].view(np.uint32))
        print(f"mixed: dead sample {b} bit-identical: {same}")
        assert same, b
    for b, (images, ref) in zip((0, 2), refs):
        _report(f"mixed: live sample {b}", got[b], ref, _rot_bound(ctab[b], images))
    again, _ = _motion(dev, vols, deg, tr, times, live=[1, 0, 1, 0])
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))               # no atomics: the same bits on every run


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections(dev):
    from gaviko_amd import lib, ops
    x = torch.zeros(1, 2, 4, 8, device=dev)
    big = torch.zeros(8 * 12 * 300, device=dev)
    live, part = torch.ones(1, dtype=torch.int32, device=dev), _partials(x)

    def call(x, out, K):
        ops.motion_artifact(x, out, big, big, live, part, K)

    out = torch.full_like(x, float("nan"))
    for K in (0, 5):
        with pytest.raises(lib.GavikoHipError, match=r"movements \(1\.\.4 are built\)"):
            call(x, out, K)
    for W in (1, 257):
        xw = torch.zeros(1, 2, 4, W, device=dev)
        ow = torch.full_like(xw, float("nan"))
        with pytest.raises(lib.GavikoHipError, match=r"last axis of \d+ voxels \(2\.\.256 are built\)"):
            call(xw, ow, 2)
        assert torch.isnan(ow).all()
    with pytest.raises(lib.GavikoHipError, match="must not overlap"):
        call(x, x, 2)
    flat = torch.zeros(2 * x.numel(), device=dev)
    with pytest.raises(lib.GavikoHipError, match="must not overlap"):                # partly overlapping views of one buffer
        call(flat[:x.numel()].view_as(x), flat[x.numel() // 2:x.numel() // 2 + x.numel()].view_as(x), 2)
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and not x.any()                                   # nothing was launched
    assert (ops.MOTION_MAX_TRANSFORMS, ops.MOTION_MAX_W) == (4, 256)


# ------------------------------------------------------------------------------------------------ the pipeline
def test_train_transforms_motion_pipeline(dev):
    """train_transforms(seed=7, intensity=True, motion=True) on 8 volumes against oracle.data_ref spatial + intensity_ref / motion_ref + rescale
    rebuilt from last_params and last_intensity.  Seed 7 was picked on the CPU from the draws alone (sampling is host-side): its batch holds
    all four kinds, RandomMotion once behind a live affine and once without.  Bound per volume, as in
    tests/test_intensity_augment_gpu.py::test_train_transforms_intensity_pipeline: the kernel's bound over (max - min) -- for a motion sample
    the `rotated` bound of the module docstring, elementwise -- plus 2e-3 where an affine resampling is live."""
    from gaviko_amd import data
    shape, B, S = (24, 32, 64), 8, 7
    vols = np.stack([_vol(shape, 80 + b) for b in range(B)])[:, None]
    x = torch.from_numpy(vols).to(dev)
    tf = data.train_transforms(seed=S, intensity=True, motion=True)
    y = tf(x).cpu().numpy()
    drawn = [d[0] if d else None for d in tf.last_intensity]
    print("pipeline draws:", drawn, [bits | (8 if aff is not None else 0) for bits, aff in tf.last_params])
    assert "RandomMotion" in drawn and len(set(drawn) - {None, "RandomMotion"}) >= 1
    for b, ((bits, aff), draw) in enumerate(zip(tf.last_params, tf.last_intensity)):
        assert y[b].min() == 0.0 and y[b].max() == 1.0, b                            # [0, 1], both ends reached
        mat = None if aff is None else data.affine_matrix(*aff, shape).astype(np.float32)
        moved = data_ref.spatial(vols[b, 0], mat, bits)
        if draw and draw[0] == "RandomMotion":
            images = motion_ref.moved_images(moved, draw[1]["degrees"], draw[1]["translation"])
            pre = motion_ref.composite(images, draw[1]["times"])
            kernel_bound = _rot_bound(data.motion_tables(draw[1]["times"], shape[-1])[0][0], images)
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
    y2 = data.train_transforms(seed=S, intensity=True, motion=True)(x).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32))                     # the seed reproduces the batch
    three = data.train_transforms(seed=S, intensity=True)(x).cpu().numpy()           # without motion: the three-member pipeline, bit for bit
    today = data.DeviceCompose([data.RandomAffine(degrees=15, p=0.5), data.RandomFlip(axes=(0,), flip_probability=0.5),
                                data.OneOf({data.RandomNoise(): 1, data.RandomBiasField(): 1, data.RandomBlur(std=(0, 1.5)): 1}, p=0.75),
                                data.RescaleIntensity((0, 1))], seed=S)(x).cpu().numpy()
    assert np.array_equal(three.view(np.uint32), today.view(np.uint32))
    off = data.train_transforms(seed=S, intensity=True, motion=False)(x).cpu().numpy()
    assert np.array_equal(three.view(np.uint32), off.view(np.uint32))
