"""GPU: the intensity kernels (gaviko_amd/csrc/intensity.hip) through ops.gaussian_blur3d / ops.intensity_pointwise against scipy and
the float64 restatement of tests/intensity_ref.py, and the train_transforms(intensity=True) pipeline against the numpy pipeline rebuilt
from its recorded draws.  Inputs are randn * 300 + 1000 in fp32 (tools/bench_data.py).  Every test prints its figures before it asserts.

Bounds (the reference is float64, so all of it is the kernels' fp32 error):
* blur   max|got - ref| <= 1e-5 max|ref|: fp32 accumulation of <= 13 taps adds <= ~14 * 2^-24 of the maximum per axis, ~2.5e-6 over three
  axes, times 4 for tap order and FMA contraction.
* noise  |got - (x + std z + mean)| <= 2e-5 std + 2^-22 max|x|: |z| <= sqrt(2 * 24 * ln 2) = 5.77; a few ulp in logf, sqrtf, cosf and the
  rounding of the 2 pi u2 argument give ~6e-6 absolute in z; the last term is the rounding of the add.
* bias   |got - ref| <= 2e-5 |ref| elementwise: the exponent is a 20-term fp32 sum of magnitude <= 10 (~3e-6 absolute), expf a few ulp on top.
"""
import numpy as np
import pytest
import torch

import intensity_ref
from oracle import data_ref

pytestmark = pytest.mark.gpu

SMALL = [(5, 12, 68), (16, 20, 72)]
SEEDS = [0x9E3779B97F4A7C15, 12345, 2 ** 64 - 3, 7]


def _vol(shape, seed):
    return (np.random.default_rng(seed).standard_normal(shape) * 300 + 1000).astype(np.float32)


def _blur(dev, vols, sigmas):
    from gaviko_amd import data, ops
    x = torch.from_numpy(vols).to(dev)
    out, scratch = torch.full_like(x, float("nan")), torch.empty_like(x)
    w, r = data.blur_tables(sigmas)
    ops.gaussian_blur3d(x, out, scratch, torch.from_numpy(w).to(dev), torch.from_numpy(r).to(dev), int(r.max()))
    return out.cpu().numpy()


def _pointwise(dev, vols, kind, noise=None, seeds=None, coeff=None, order=3):
    from gaviko_amd import ops
    B = len(vols)
    x = torch.from_numpy(vols).to(dev)
    y = torch.full_like(x, float("nan"))
    noise = np.zeros((B, 2), np.float32) if noise is None else np.asarray(noise, np.float32)
    seeds = np.zeros(B, np.uint64) if seeds is None else np.array(seeds, dtype=np.uint64)
    cf = np.zeros((B, ops.BIAS_COEFFS), np.float32)
    if coeff is not None:
        for b, c in enumerate(coeff):
            cf[b, :len(c)] = c
    ops.intensity_pointwise(x, y, torch.from_numpy(np.asarray(kind, np.int32)).to(dev), torch.from_numpy(noise).to(dev),
                            torch.from_numpy(seeds.view(np.int64)).to(dev), torch.from_numpy(cf).to(dev), order)
    return y.cpu().numpy()


def _check_blur(got, vol, sig, tag):
    ref = intensity_ref.blur(vol, sig)
    err, bound = np.abs(got - ref).max(), 1e-5 * np.abs(ref).max()
    print(f"blur {tag} sigma {tuple(sig)}: max err {err:.3e}  bound {bound:.3e}")
    assert err <= bound, (tag, err, bound)


# ------------------------------------------------------------------------------------------------ blur vs scipy
@pytest.mark.parametrize("shape,sig", [((5, 12, 68), (1.5, 1.5, 1.5)),       # radius 6 > D = 5: reflects twice; W no multiple of 64
                                       ((5, 12, 68), (0.1, 0.9, 0.0)),       # radius 0 and a skipped axis
                                       ((16, 20, 72), (1.5, 0.3, 1.2)),
                                       ((120, 160, 160), (1.5, 1.5, 1.5))])  # the tiling at the real extent
def test_blur_vs_scipy(dev, shape, sig):
    vol = _vol(shape, 3)
    _check_blur(_blur(dev, vol[None], [sig])[0], vol, sig, shape)


def test_blur_per_sample_sigmas_in_one_launch(dev):
    shape = (16, 20, 72)
    vols = np.stack([_vol(shape, 40 + b) for b in range(3)])
    sig = [(1.5, 0.3, 1.2), (0.0, 0.0, 0.0), (0.6, 2.5, 4.0)]               # sample 2 reaches the radius cap of 16 on the W axis
    got = _blur(dev, vols, sig)
    assert np.array_equal(got[1].view(np.uint32), vols[1].view(np.uint32))  # all-zero sigma: the input's bits
    for b in (0, 2):
        _check_blur(got[b], vols[b], sig[b], f"sample {b}")


def test_blur_rejects_sigma_above_4(dev):
    from gaviko_amd import lib, ops
    x = torch.zeros(1, 4, 4, 4, device=dev)
    w, r = torch.zeros(1, 3, 33, device=dev), torch.zeros(1, 3, dtype=torch.int32, device=dev)
    with pytest.raises(lib.GavikoHipError, match="sigma above 4"):
        ops.gaussian_blur3d(x, torch.empty_like(x), torch.empty_like(x), w, r, 17)
    with pytest.raises(lib.GavikoHipError, match="three different buffers"):
        ops.gaussian_blur3d(x, x, torch.empty_like(x), w, r, 0)


# ------------------------------------------------------------------------------------------------ noise vs the host hash
@pytest.mark.parametrize("shape", SMALL)
def test_noise_vs_host_field(dev, shape):
    par = [(0.25, 0.0), (0.25, 3.0), (40.0, 0.0), (40.0, 3.0)]              # (std, mean)
    vols = np.stack([_vol(shape, 50 + b) for b in range(4)])
    got = _pointwise(dev, vols, [1] * 4, noise=par, seeds=SEEDS)
    for b, (std, mean) in enumerate(par):
        ref = intensity_ref.noise(vols[b], std, mean, SEEDS[b])
        err, bound = np.abs(got[b] - ref).max(), 2e-5 * std + 2.0 ** -22 * np.abs(vols[b]).max()
        print(f"noise {shape} std {std} mean {mean}: max err {err:.3e}  bound {bound:.3e}")
        assert err <= bound, (b, err, bound)
        z = (got[b].astype(np.float64) - vols[b] - mean) / std
        assert abs(z.mean()) < 0.1 and 0.9 < z.std() < 1.1                  # it is noise, not a constant
    again = _pointwise(dev, vols, [1] * 4, noise=par, seeds=SEEDS)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))       # same seed: same bits
    other = _pointwise(dev, vols, [1] * 4, noise=par, seeds=[s ^ 1 for s in SEEDS])
    assert all((other[b] != got[b]).mean() > 0.9 for b in range(4))         # another seed: another field


# ------------------------------------------------------------------------------------------------ bias field
@pytest.mark.parametrize("shape", SMALL + [(1, 12, 68)])                    # (1, ..): the n = 1 axis rule
@pytest.mark.parametrize("order", [3, 1])
def test_bias_field_vs_numpy(dev, shape, order):
    n = len(intensity_ref.bias_terms(order))
    coeff = np.random.default_rng(77).uniform(-0.5, 0.5, (2, n)).astype(np.float32)
    vols = np.stack([_vol(shape, 60 + b) for b in range(2)])
    got = _pointwise(dev, vols, [2, 2], coeff=coeff, order=order)
    for b in range(2):
        ref = intensity_ref.bias(vols[b], coeff[b], order)
        rel = (np.abs(got[b] - ref) / np.abs(ref)).max()
        print(f"bias {shape} order {order}: max rel err {rel:.3e}  bound 2e-5")
        assert (np.abs(got[b] - ref) <= 2e-5 * np.abs(ref)).all(), (b, rel)


# ------------------------------------------------------------------------------------------------ kinds mixed in one launch
def test_mixed_kinds_in_one_launch(dev):
    shape = (5, 12, 68)
    vols = np.stack([_vol(shape, 70 + b) for b in range(4)])
    vols[0, 0, 0, :4] = [-0.0, 0.0, np.float32(1e-42), -np.float32(3e38)]   # a copy keeps signed zeros, subnormals and large values
    coeff = np.random.default_rng(78).uniform(-0.5, 0.5, (4, 20)).astype(np.float32)
    got = _pointwise(dev, vols, [0, 1, 2, 0], noise=[(0, 0), (40.0, 3.0), (0, 0), (9.0, 9.0)], seeds=SEEDS, coeff=coeff, order=3)
    for b in (0, 3):
        assert np.array_equal(got[b].view(np.uint32), vols[b].view(np.uint32)), b
    ref = intensity_ref.noise(vols[1], 40.0, 3.0, SEEDS[1])
    assert np.abs(got[1] - ref).max() <= 2e-5 * 40.0 + 2.0 ** -22 * np.abs(vols[1]).max()
    ref = intensity_ref.bias(vols[2], coeff[2], 3)
    assert (np.abs(got[2] - ref) <= 2e-5 * np.abs(ref)).all()


# ------------------------------------------------------------------------------------------------ the pipeline
def test_train_transforms_intensity_pipeline(dev):
    """train_transforms(seed=7, intensity=True) on 8 volumes against oracle.data_ref spatial + intensity_ref + rescale rebuilt from last_params
    and last_intensity.  Bound per volume: (blur + noise + bias bounds of the module docstring, at that volume's maximum and drawn std) /
    (max - min), plus 2e-3 where an affine resampling is live -- the bound tests/test_data_metrics.py::test_train_transforms_pipeline sets
    for that same pass (fp32 trilinear weights against the oracle's)."""
    from gaviko_amd import data
    shape, B = (24, 32, 64), 8
    vols = np.stack([_vol(shape, 80 + b) for b in range(B)])[:, None]
    x = torch.from_numpy(vols).to(dev)
    tf = data.train_transforms(seed=7, intensity=True)
    y = tf(x).cpu().numpy()
    drawn = [d[0] if d else None for d in tf.last_intensity]
    print("pipeline draws:", drawn, [bits | (8 if aff is not None else 0) for bits, aff in tf.last_params])
    assert len(set(drawn) - {None}) >= 2                                     # this seed exercises more than one kind
    for b, ((bits, aff), draw) in enumerate(zip(tf.last_params, tf.last_intensity)):
        assert y[b].min() == 0.0 and y[b].max() == 1.0, b                    # [0, 1], both ends reached
        mat = None if aff is None else data.affine_matrix(*aff, shape).astype(np.float32)
        pre = intensity_ref.apply(data_ref.spatial(vols[b, 0], mat, bits), draw)
        want = data_ref.rescale_intensity(pre.astype(np.float32))
        top, rng_ = np.abs(pre).max(), pre.max() - pre.min()
        std = draw[1]["std"] if draw and draw[0] == "RandomNoise" else 0.0
        bound = (1e-5 * top + (2e-5 * std + 2.0 ** -22 * top) + 2e-5 * top) / rng_ + (2e-3 if aff is not None else 0.0)
        err = np.abs(y[b, 0] - want).max()
        print(f"pipeline sample {b} {drawn[b]} affine {aff is not None}: max err {err:.3e}  bound {bound:.3e}")
        assert err <= bound, (b, drawn[b], err, bound)
    y2 = data.train_transforms(seed=7, intensity=True)(x).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32))             # the seed reproduces the batch
    plain = data.train_transforms(seed=7, intensity=False)(x).cpu().numpy()
    today = data.DeviceCompose([data.RandomAffine(degrees=15, p=0.5), data.RandomFlip(axes=(0,), flip_probability=0.5),
                                data.RescaleIntensity((0, 1))], seed=7)(x).cpu().numpy()
    assert np.array_equal(plain.view(np.uint32), today.view(np.uint32))
    assert np.array_equal(plain.view(np.uint32), data.train_transforms(seed=7)(x).cpu().numpy().view(np.uint32))
