"""GPU: the RandomElasticDeformation kernel (gaviko_amd/csrc/elastic.hip) through ops.elastic_deform against the float64 restatement
(tests/elastic_ref.py), and the DeviceCompose pipelines that contain it against the same stages issued by hand.  Inputs are
randn * 300 + 1000 in fp32, the control points come from data.RandomElasticDeformation.sample.  Every test prints its maxima before it asserts.

Bounds (the reference is float64 on the same float32 control points, so all of it is the kernel's fp32 error), elementwise:
* field   |field - d64| <= 2^-24 (24 M + 160) Phi, M the largest mesh size n - 3, Phi the largest |control displacement|.
  Position: u = (q + 0.5) M / S is one exact add and two roundings of a value <= M, within 2^-22 M; the spline's slope per unit u is at most
  2 Phi on each of three axes: 6 Phi 2^-22 M = 24 M 2^-24 Phi.  (Where fp32 and float64 disagree on the cell of a u that lies on a knot, both
  evaluate the same C2 function, so this term covers it.)  Weights: 96 2^-24 Phi for the rounding of the three axes' 1-D weights, 64 2^-24 Phi
  for a 64-term accumulation.  The kernel contracts separably -- 4 fused multiply-adds over axis 1, 4 over axis 0, 4 over axis 2, weights
  that sum to 1 -- which rounds 12 times where the 64-term sum rounds 64 times, and each of its weights takes at most 8 roundings of
  intermediate values <= 6, divided by 6: within the 32 2^-24 per axis granted.  So the constants stand as an upper bound for this operation
  order as well; none of them is fitted.
* gather  |out - read64(float32(q) + field)| <= 16 2^-24 max(|x|, |pad|): the positions are the kernel's own (one fp32 add per axis), the
  fraction p - floor(p) is exact, eight products carry three roundings each, plus the accumulation.
* shift   a constant coarse field (0, 0, 3): the gather bound plus G_W 2^-24 (24 M + 160) 3, G_W the largest neighbour difference along W of
  the volume continued with its minimum -- a field that is off by e moves the read by e voxels."""
import functools
import warnings

import numpy as np
import pytest
import torch

import elastic_ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


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


def _deform(dev, vols, ctrl, live=None, want_field=True):
    """vols [B][D][H][W] f32, ctrl [B][n0][n1][n2][3] f32 -> (out, field or None) as numpy; both start as NaN"""
    from gaviko_amd import ops
    B = len(vols)
    x = torch.from_numpy(vols).to(dev)
    out = torch.full_like(x, float("nan"))
    field = torch.full((B, 3) + tuple(vols.shape[1:]), float("nan"), device=dev) if want_field else None
    lv = np.ones(B, np.int32) if live is None else np.asarray(live, np.int32)
    ops.elastic_deform(x, out, torch.from_numpy(ctrl).to(dev), torch.from_numpy(lv).to(dev), _partials(x), field)
    return out.cpu().numpy(), None if field is None else field.cpu().numpy()


def _coarse(n, max_displacement, locked, seed):
    from gaviko_amd import data
    el = data.RandomElasticDeformation(num_control_points=n, max_displacement=max_displacement, locked_borders=locked)
    return el.sample(np.random.default_rng(seed)).astype(np.float32)


def _field_bound(n, ctrl):
    return EPS * (24 * (max(n) - 3) + 160) * float(np.abs(ctrl).max())


# shape, control points, locked borders, max displacement.  (5, 6, 70): W no multiple of 64, H no multiple of 4, D below the spline support;
# (4, 4, 4) is the minimum (one mesh cell), (16, 16, 16) the cap; locked borders 0 let the read leave the volume (the pad value is read);
# locked borders 2 need more than 4 points on every axis
CASES = [(s, n, lk, md) for s in [(5, 6, 70), (9, 13, 33), (24, 32, 40)] for n in [(4, 4, 4), (7, 7, 7), (4, 7, 10)]
         for lk, md in [(0, 7.5), (1, (0, 3, 12)), (2, 7.5)] if not (lk == 2 and 4 in n)]
CASES += [((24, 32, 40), (16, 16, 16), 0, (0, 3, 12)), ((24, 32, 40), (16, 16, 16), 2, 7.5)]


@functools.lru_cache(maxsize=None)
def _case(dev, shape, n, locked, md):
    """one launch per case, shared by the field and the gather test, never modified"""
    vol, ctrl = _vol(shape, 40 + sum(shape)), _coarse(n, md, locked, 7 + sum(n) + locked)
    out, field = _deform(dev, vol[None], ctrl[None])
    return vol, ctrl, out[0], field[0]


@pytest.mark.parametrize("shape,n,locked,md", CASES)
def test_field_vs_float64_bspline(dev, shape, n, locked, md):
    vol, ctrl, out, field = _case(dev, shape, n, locked, md)
    want = elastic_ref.dense_field(ctrl, shape)
    err, bound = np.abs(field - want).max(), _field_bound(n, ctrl)
    print(f"field {shape} n {n} locked {locked} max {md}: max |d| {np.abs(want).max():.3f}  max err {err:.3e}  bound {bound:.3e}  err / bound {err / bound:.3f}")
    assert np.isfinite(field).all() and err <= bound
    assert np.abs(want).max() > 0.5                                                     # a deformation, not the identity
    if md != 7.5:
        assert not field[0].any()                                                       # max_displacement 0 on axis 0: exactly none


@pytest.mark.parametrize("shape,n,locked,md", CASES)
def test_gather_at_the_kernels_own_positions(dev, shape, n, locked, md):
    vol, ctrl, out, field = _case(dev, shape, n, locked, md)
    pad = float(vol.min())
    pos = (elastic_ref.grid(shape).astype(np.float32) + field).astype(np.float64)       # float32(q) + d: one fp32 add per axis
    want = elastic_ref.trilinear_read(vol, pos, pad)
    outside = ((pos < 0) | (pos > np.array(shape, dtype=np.float64)[:, None, None, None] - 1)).any(axis=0).mean()
    err, bound = np.abs(out - want).max(), 16 * EPS * max(float(np.abs(vol).max()), abs(pad))
    print(f"gather {shape} n {n} locked {locked} max {md}: reads with a pad neighbour {outside:.3f}  max err {err:.3e}  bound {bound:.3e}  "
          f"err / bound {err / bound:.3f}")
    assert np.isfinite(out).all() and err <= bound
    assert np.abs(out - vol).max() > 10.0                                               # noise volumes: a wrong index shows at full size
    if locked == 0:
        assert outside > 0                                                              # the pad value was read


@pytest.mark.parametrize("shape,n", [((5, 6, 70), (7, 7, 7)), ((9, 13, 33), (4, 4, 4)), ((24, 32, 40), (4, 7, 10)), ((24, 32, 40), (16, 16, 16))])
def test_constant_field_is_an_exact_shift(dev, shape, n):
    vol = _vol(shape, 60 + sum(shape))
    ctrl = np.zeros(n + (3,), dtype=np.float32)
    ctrl[..., 2] = 3.0
    out, field = _deform(dev, vol[None], ctrl[None])
    pad = vol.min()
    want = np.full_like(vol, pad)
    want[:, :, :-3] = vol[:, :, 3:]                                                     # out[x] = in[x + 3]; the vacated columns read the minimum
    padded = np.concatenate([np.full(shape[:2] + (1,), pad), vol, np.full(shape[:2] + (1,), pad)], axis=2).astype(np.float64)
    G = np.abs(np.diff(padded, axis=2)).max()
    fb = EPS * (24 * (max(n) - 3) + 160) * 3.0
    bound = 16 * EPS * float(np.abs(vol).max()) + G * fb
    ferr = max(np.abs(field[0, 0]).max(), np.abs(field[0, 1]).max(), np.abs(field[0, 2] - 3.0).max())
    err, edge = np.abs(out[0] - want).max(), np.abs(out[0][:, :, -3:] - pad).max()
    print(f"shift {shape} n {n}: field err {ferr:.3e} (bound {fb:.3e})  max err {err:.3e}  vacated columns vs minimum {edge:.3e}  bound {bound:.3e}  "
          f"err / bound {err / bound:.3f}")
    assert ferr <= fb and err <= bound


def test_mixed_batch_single_launches_and_repeatability(dev):
    shape, n = (9, 13, 33), (7, 7, 7)
    vols = np.stack([_vol(shape, 70 + b) for b in range(3)])
    vols[1, 0, 0, :4] = [-0.0, 0.0, np.float32(1e-42), -np.float32(3e38)]               # a dead sample keeps signed zeros, subnormals, large values
    ctrl = np.stack([_coarse(n, 7.5, lk, 90 + lk) for lk in (0, 1, 2)])
    out, field = _deform(dev, vols, ctrl, live=[1, 0, 1])
    same = np.array_equal(out[1].view(np.uint32), vols[1].view(np.uint32))
    print(f"batch: dead sample bit-identical {same}, its field max {np.abs(field[1]).max():.1e}")
    assert same and not field[1].any() and not np.signbit(field[1]).any()
    for b in (0, 2):
        o1, f1 = _deform(dev, vols[b:b + 1], ctrl[b:b + 1])
        eq = np.array_equal(o1[0].view(np.uint32), out[b].view(np.uint32)) and np.array_equal(f1[0].view(np.uint32), field[b].view(np.uint32))
        print(f"batch: sample {b} equals its single launch bit for bit: {eq}; max |out - in| {np.abs(out[b] - vols[b]).max():.1f}")
        assert eq and np.abs(out[b] - vols[b]).max() > 10.0
    again, fagain = _deform(dev, vols, ctrl, live=[1, 0, 1])
    assert np.array_equal(out.view(np.uint32), again.view(np.uint32)) and np.array_equal(field.view(np.uint32), fagain.view(np.uint32))
    nofield, none = _deform(dev, vols, ctrl, live=[1, 0, 1], want_field=False)          # field is optional and changes nothing
    assert none is None and np.array_equal(out.view(np.uint32), nofield.view(np.uint32))


def test_rejections(dev):
    from gaviko_amd import lib, ops
    x = torch.zeros(1, 4, 8, 8, device=dev)
    out = torch.full_like(x, float("nan"))
    live, part = torch.ones(1, dtype=torch.int32, device=dev), _partials(x)
    ctrl = lambda *n: torch.ones((1,) + n + (3,), device=dev)                           # noqa: E731
    with pytest.raises(lib.GavikoHipError, match="must not overlap"):
        ops.elastic_deform(x, x, ctrl(4, 4, 4), live, part)
    flat = torch.zeros(2 * x.numel(), device=dev)
    with pytest.raises(lib.GavikoHipError, match="must not overlap"):                    # partly overlapping views of one buffer
        ops.elastic_deform(flat[:x.numel()].view_as(x), flat[x.numel() // 2:x.numel() // 2 + x.numel()].view_as(x), ctrl(4, 4, 4), live, part)
    for n in [(3, 4, 4), (4, 4, 3), (17, 4, 4), (4, 17, 4), (7, 7, 17)]:
        with pytest.raises(lib.GavikoHipError, match=r"control points \(4\.\.16 per axis are built\)"):
            ops.elastic_deform(x, out, ctrl(*n), live, part)
    for bad in (torch.ones(4 * 4 * 4 * 3, device=dev), torch.ones(2, 4, 4, 4, 3, device=dev), torch.ones(1, 4, 4, 4, 2, device=dev),
                torch.ones(1, 4, 4, 4, 3, device=dev, dtype=torch.float64), torch.ones(1, 4, 4, 8, 3, device=dev)[:, :, :, ::2]):
        with pytest.raises(lib.GavikoHipError, match="elastic_deform ctrl"):
            ops.elastic_deform(x, out, bad, live, part)
    with pytest.raises(lib.GavikoHipError, match="elastic_deform field"):
        ops.elastic_deform(x, out, ctrl(4, 4, 4), live, part, field=torch.zeros(2 * x.numel(), device=dev))
    big, V = torch.zeros(4 * x.numel(), device=dev), x.numel()
    with pytest.raises(lib.GavikoHipError, match="field must not overlap"):              # a field that starts inside the input buffer
        ops.elastic_deform(big[:V].view_as(x), out, ctrl(4, 4, 4), live, part, field=big[V // 2:V // 2 + 3 * V])
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and not x.any()                                       # nothing was launched
    assert ops.ELASTIC_MAX_CONTROL_POINTS == 16


# ------------------------------------------------------------------------------------------------ the pipelines
def _by_hand(tf, x, rescale=True):
    """the stages DeviceCompose issues, rebuilt from last_elastic and last_params (tf has just been called on a batch like x)"""
    from gaviko_amd import data, ops
    dev, B, shape = x.device, x.shape[0], tuple(x.shape[-3:])
    part = ops.minmax_partials(B, dev)
    launches = []
    if any(f is not None for f in tf.last_elastic):
        n = next(f for f in tf.last_elastic if f is not None).shape[:3]
        ctrl, live = np.zeros((B,) + n + (3,), np.float32), np.zeros(B, np.int32)
        for b, f in enumerate(tf.last_elastic):
            if f is not None:
                ctrl[b], live[b] = f, 1
        ops.volume_minmax(x, part)
        y = torch.empty_like(x)
        ops.elastic_deform(x, y, torch.from_numpy(ctrl).to(dev), torch.from_numpy(live).to(dev), part)
        x = y
        launches.append("elastic")
    mats, flags = np.tile(np.eye(3, 4, dtype=np.float32), (B, 1, 1)), np.zeros(B, np.int32)
    for b, (bits, aff) in enumerate(tf.last_params):
        flags[b] = bits | (8 if aff is not None else 0)
        if aff is not None:
            mats[b] = data.affine_matrix(*aff, shape).astype(np.float32)
    if flags.any():
        ops.volume_minmax(x, part)
        y = torch.empty_like(x)
        ops.spatial_transform(x, y, torch.from_numpy(mats).to(dev), torch.from_numpy(flags).to(dev), part)
        x = y
        launches.append("spatial")
    ops.volume_minmax(x, part)
    y = torch.empty_like(x)
    ops.rescale_intensity(x, part, y, 0.0, 1.0)
    return y, launches


def _pipeline_volumes(dev):
    return torch.from_numpy(np.stack([_vol((24, 32, 40), 120 + b) for b in range(6)])[:, None]).to(dev)


def test_compose_pipeline_equals_the_stages_issued_by_hand(dev):
    """DeviceCompose([RandomElasticDeformation(p=.5), RandomAffine(degrees=15, p=.5), RandomFlip(0), RescaleIntensity()], seed=1) on 6
    volumes of (24, 32, 40), bit for bit.  Seed 1 was picked on the CPU from the draws alone (sampling is host-side): its batch holds all
    four combinations of elastic and affine, and both flip states."""
    from gaviko_amd import data
    x = _pipeline_volumes(dev)
    tf = data.DeviceCompose([data.RandomElasticDeformation(p=.5), data.RandomAffine(degrees=15, p=.5), data.RandomFlip(0), data.RescaleIntensity()], seed=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                                 # 7.5 voxels against cells of 6, 8, 10: the folding warning
        y = tf(x)
    combos = [(e is not None, aff is not None) for e, (_, aff) in zip(tf.last_elastic, tf.last_params)]
    print("compose draws (elastic, affine):", combos, "flips:", [bits for bits, _ in tf.last_params])
    assert len(set(combos)) == 4
    want, launches = _by_hand(tf, x)
    same = np.array_equal(y.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    print(f"compose: bit-identical to {launches} + rescale by hand: {same}")
    assert same and launches == ["elastic", "spatial"]
    yn = y.cpu().numpy()
    assert all(yn[b].min() == 0.0 and yn[b].max() == 1.0 for b in range(6))
    # the elastic pass changes the samples that drew it, and only those, against the same compose without it
    plain = data.DeviceCompose([data.RescaleIntensity()])(x).cpu().numpy()
    for b, (e, a) in enumerate(combos):
        if not a and not tf.last_params[b][0]:
            assert np.array_equal(yn[b], plain[b]) == (not e), b


def test_train_transforms_elastic_pipeline_equals_the_stages_issued_by_hand(dev):
    """train_transforms(seed=0, elastic=True) on the same 6 volumes, bit for bit.  Seed 0 was picked on the CPU from the draws alone: its
    batch holds two elastic samples, three affine ones and one that drew neither; no sample ever holds both."""
    from gaviko_amd import data
    x = _pipeline_volumes(dev)
    tf = data.train_transforms(seed=0, elastic=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        y = tf(x)
    kinds = ["elastic" if e is not None else "affine" if aff is not None else None for e, (_, aff) in zip(tf.last_elastic, tf.last_params)]
    print("train_transforms(elastic=True) draws:", kinds)
    assert kinds.count("elastic") >= 2 and kinds.count("affine") >= 2 and None in kinds
    assert not any(e is not None and aff is not None for e, (_, aff) in zip(tf.last_elastic, tf.last_params))
    want, launches = _by_hand(tf, x)
    same = np.array_equal(y.cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
    print(f"train_transforms(elastic=True): bit-identical to {launches} + rescale by hand: {same}")
    assert same and launches == ["elastic", "spatial"]
    # elastic=False is today's pipeline: no elastic launch, the same bits as the compose written out
    off = data.train_transforms(seed=0, elastic=False)
    today = data.DeviceCompose([data.RandomAffine(degrees=15, p=0.5), data.RandomFlip(axes=(0,), flip_probability=0.5), data.RescaleIntensity((0, 1))], seed=0)
    assert np.array_equal(off(x).cpu().numpy().view(np.uint32), today(x).cpu().numpy().view(np.uint32)) and off.last_elastic == [None] * 6
