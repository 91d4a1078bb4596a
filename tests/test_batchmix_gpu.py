"""GPU: gvk_batch_mix (csrc/batchmix.hip) through ops.batch_mix, the library itself and data.BatchMix against tests/batchmix_ref.py.

Copy and CutMix move values: equality is bit for bit.  Mixup is held to the rounding bound of its float32 evaluation,
|got - ref| <= 3.01 * 2^-24 * (|lam x_a| + |(1 - lam) x_b|) elementwise (batchmix_ref.mixup_bound).  Inputs: ramps whose every voxel names its
own (sample, d, h, w) exactly in float32, so a wrong index shows, and random volumes around 1e3 +- 300, so that an operand rounded to bf16
(relative 2^-9) is orders of magnitude outside the bound.  (3, 7, 33) has V = 693, odd: every second sample is off the 16-byte grid and the rows
end inside the groups of four; (2, 3, 20) is below one workgroup's tile, (16, 20, 72) spans several workgroups."""
import numpy as np
import pytest
import torch

import batchmix_ref
from gaviko_amd import lib, ops
from gaviko_amd.data import BatchMix, MixedTarget, train_transforms

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 20), (3, 7, 33), (5, 12, 68), (16, 20, 72)]
PERMS = {1: [[0]], 5: [[1, 0, 3, 4, 2], [0, 3, 2, 4, 1]]}     # a 2-cycle with a 3-cycle; a 3-cycle with two fixed points; the fixed point alone
LAMS = [0.0, 2.0 ** -20, 0.3, 0.5, 1.0 - 2.0 ** -20, 1.0]


def _ramp(B, shape):
    i0, i1, i2 = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    vol = (i0 * 1e4 + i1 * 1e2 + i2).astype(np.float32)               # exact in float32; every voxel names its own index
    return np.stack([vol + np.float32(1e6 * b) for b in range(B)])     # ... and its sample: below 2^24, still exact


def _random(B, shape, seed):
    rng = np.random.default_rng(seed)
    return (1e3 + 300.0 * rng.uniform(-1, 1, size=(B,) + shape)).astype(np.float32)


def _volumes(kind, B, shape):
    return _ramp(B, shape) if kind == "ramp" else _random(B, shape, 17 + B)


def _boxes(shape):
    D, H, W = shape
    inner = [(1, n - 1) if n > 2 else (0, n) for n in shape]
    faces = []
    for a, n in enumerate(shape):
        for rng in ((0, max(1, n // 2)), (n // 2, n)):                 # touching the low and the high face of axis a
            r = list(inner)
            r[a] = rng
            faces.append(tuple(v for pair in r for v in pair))
    w1 = W - 1 if (W - 1) % 2 else W - 2
    return faces + [(D // 2, D // 2 + 1, H // 2, H // 2 + 1, W // 2, W // 2 + 1),      # one voxel
                    (0, D, 0, H, 0, W),                                                 # the whole volume: x[p]
                    (1, 1, 0, H, 0, W),                                                 # empty: x[b]
                    (0, D, 0, H, 3, w1)]                                                # w0 and w1 odd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _run_ops(dev, x, mode, lam, perm, box):
    xt = torch.from_numpy(x).to(dev)
    out = torch.full_like(xt, float("nan"))
    ops.batch_mix(xt, out, mode, lam, perm, box)
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["ramp", "random"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_copy_and_cutmix_are_bit_exact(dev, shape, B, kind):
    x = _volumes(kind, B, shape)
    boxes = _boxes(shape)
    assert len(boxes) == 10 and (boxes[-1][4] % 2, boxes[-1][5] % 2) == (1, 1)
    live = [b for b in range(B) if B == 1 or b != 1]                    # sample 1 of a batch of 5 stays dead among live ones
    launches = 0
    for perm in PERMS[B]:
        for first in range(0, len(boxes), len(live)):
            mode, lam, box = np.zeros(B, np.int32), np.ones(B, np.float32), np.zeros((B, 6), np.int32)
            for b, bx in zip(live, boxes[first:first + len(live)]):
                mode[b], box[b] = ops.MIX_CUTMIX, bx
            want = batchmix_ref.mix(x, mode, lam, perm, box).astype(np.float32)
            got = _run_ops(dev, x, mode, lam, perm, box)
            assert np.array_equal(_bits(got), _bits(want)), (perm, first)
            for b in range(B):                                          # said directly: the partner inside the box, itself outside
                d0, d1, h0, h1, w0, w1 = box[b]
                inside = np.zeros(shape, bool)
                inside[d0:d1, h0:h1, w0:w1] = mode[b] == ops.MIX_CUTMIX
                assert np.array_equal(got[b][inside], x[perm[b]][inside]) and np.array_equal(got[b][~inside], x[b][~inside])
            # the dead samples' entries are not read: garbage there, on tables handed straight to the library (ops.batch_mix rejects them)
            gl, gp, gb = lam.copy(), np.array(perm, np.int32), box.copy()
            dead = mode == ops.MIX_COPY
            gl[dead], gp[dead], gb[dead] = np.nan, -1, (-7, 10 ** 6, 10 ** 6, -3, 5, 2)
            gl[~dead] = np.nan                                          # CutMix does not read lam either
            xt = torch.from_numpy(x).to(dev)
            out = torch.full_like(xt, float("nan"))
            tabs = [torch.from_numpy(t).to(dev) for t in (mode, gl, gp, gb)]
            lib.check(lib.load().gvk_batch_mix(lib.ptr(xt), lib.ptr(out), *[lib.ptr(t) for t in tabs], B, *shape, lib.stream_ptr()), "gvk_batch_mix")
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), ("garbage", perm, first)
            launches += 1
    print(f"{shape} B={B} {kind}: {launches} table sets, 2 launches each, all bit-exact")


@pytest.mark.parametrize("kind", ["ramp", "random"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_mixup_within_the_rounding_bound(dev, shape, B, kind):
    x = _volumes(kind, B, shape)
    worst = 0.0
    for perm in PERMS[B]:
        for first in range(len(LAMS) if B == 1 else 2):
            lam = np.array([LAMS[(first + b) % len(LAMS)] for b in range(B)], np.float32)
            mode, box = np.full(B, ops.MIX_MIXUP, np.int32), np.zeros((B, 6), np.int32)
            got = _run_ops(dev, x, mode, lam, perm, box)
            ref = batchmix_ref.mix(x, mode, lam, perm, box)
            for b in range(B):
                bound = batchmix_ref.mixup_bound(x, lam, perm, b)
                err = np.abs(got[b].astype(np.float64) - ref[b])
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                assert (err <= bound).all(), (perm, float(lam[b]), float(err.max()))
                if lam[b] == 1.0:
                    assert np.array_equal(_bits(got[b]), _bits(x[b]))
                if lam[b] == 0.0:
                    assert np.array_equal(_bits(got[b]), _bits(x[perm[b]]))
    print(f"{shape} B={B} {kind}: worst error / bound = {worst:.3f}")


def test_mixed_batch_in_one_launch(dev):
    """copy, Mixup and CutMix samples side by side at the odd volume, partners of another mode"""
    shape, B = (3, 7, 33), 5
    x = _ramp(B, shape) + _random(B, shape, 5) * np.float32(1e-3)
    mode = np.array([ops.MIX_MIXUP, ops.MIX_COPY, ops.MIX_CUTMIX, ops.MIX_MIXUP, ops.MIX_CUTMIX], np.int32)
    lam, perm = np.array([0.3, 1.0, 1.0, 0.7, 1.0], np.float32), [1, 0, 3, 4, 2]
    box = np.zeros((B, 6), np.int32)
    box[2], box[4] = (1, 3, 2, 6, 5, 30), (0, 2, 0, 7, 1, 2)
    got = _run_ops(dev, x, mode, lam, perm, box)
    ref = batchmix_ref.mix(x, mode, lam, perm, box)
    for b in range(B):
        if mode[b] == ops.MIX_MIXUP:
            assert (np.abs(got[b] - ref[b]) <= batchmix_ref.mixup_bound(x, lam, perm, b)).all()
        else:
            assert np.array_equal(_bits(got[b]), _bits(ref[b].astype(np.float32)))


def test_ops_wrapper_rejects_bad_tables(dev):
    x = torch.zeros(2, 2, 3, 20, device=dev)
    out = torch.empty_like(x)
    ok = dict(mode=[1, 2], lam=[0.5, 1.0], perm=[1, 0], box=[[0] * 6, [0, 1, 0, 1, 0, 4]])
    ops.batch_mix(x, out, **ok)
    for bad in (dict(mode=[1, 3]), dict(perm=[2, 0]), dict(perm=[-1, 0]), dict(lam=[float("nan"), 1.0]), dict(lam=[1.5, 1.0]),
                dict(box=[[0] * 6, [0, 3, 0, 1, 0, 4]]), dict(box=[[0] * 6, [1, 0, 0, 1, 0, 4]]), dict(mode=[1])):
        with pytest.raises(lib.GavikoHipError):
            ops.batch_mix(x, out, **dict(ok, **bad))
    with pytest.raises(lib.GavikoHipError, match="overlap"):
        ops.batch_mix(x, x, **ok)


def test_batchmix_pipeline(dev):
    shape, B = (5, 12, 68), 5
    x = _random(B, shape, 23)[:, None]                                  # [B, 1, D, H, W]
    labels = torch.tensor([3, 0, 4, 1, 2])
    xt = torch.from_numpy(x).to(dev)
    mix = BatchMix(seed=3)
    got, target = mix(xt, labels.to(dev))
    t = mix.last_mix
    print("modes", t["mode"].tolist(), "lam", t["lam"].tolist(), "perm", t["perm"].tolist())
    assert set(t["mode"].tolist()) == {ops.MIX_COPY, ops.MIX_MIXUP, ops.MIX_CUTMIX}       # seed 3 draws all three
    assert got.shape == xt.shape and got.data_ptr() != xt.data_ptr()
    lam32 = t["lam"].astype(np.float32)
    ref = batchmix_ref.mix(x[:, 0], t["mode"], lam32, t["perm"], t["box"])
    g = got.cpu().numpy()[:, 0]
    for b in range(B):
        if t["mode"][b] == ops.MIX_MIXUP:
            assert (np.abs(g[b] - ref[b]) <= batchmix_ref.mixup_bound(x[:, 0], lam32, t["perm"], b)).all()
        else:
            assert np.array_equal(_bits(g[b]), _bits(ref[b].astype(np.float32)))
    assert isinstance(target, MixedTarget)
    assert torch.equal(target.a.cpu(), labels) and torch.equal(target.b.cpu(), labels[torch.from_numpy(t["perm"].astype(np.int64))])
    assert target.lam.dtype == torch.float32 and np.array_equal(target.lam.cpu().numpy(), lam32)
    for b in range(B):                                                  # the corrected lam is the share of the volume a sample keeps
        if t["mode"][b] == ops.MIX_CUTMIX:
            d0, d1, h0, h1, w0, w1 = t["box"][b]
            assert t["lam"][b] == 1.0 - (d1 - d0) * (h1 - h0) * (w1 - w0) / float(np.prod(shape))
    again, target2 = BatchMix(seed=3)(xt, labels.to(dev))
    assert torch.equal(again.view(torch.int32), got.view(torch.int32)) and torch.equal(target2.lam, target.lam) and torch.equal(target2.b, target.b)


def test_batchmix_leaves_the_compose_stream_alone(dev):
    xt = torch.from_numpy(_random(4, (5, 12, 68), 2)[:, None]).to(dev)
    labels = torch.arange(4, device=dev)
    with_mix, without = train_transforms(seed=7), train_transforms(seed=7)
    mix = BatchMix(seed=1)
    for _ in range(2):
        a = with_mix(xt)
        mix(a, labels)
        b = without(xt)
        assert repr(with_mix.last_params) == repr(without.last_params)
        assert torch.equal(a, b)
