"""CPU: the host side of Mixup / CutMix -- BatchMix's sampling (draw order, box rule, dead samples), MixedTarget.dense, and the errors of
BatchMix and of the losses' new arguments.  The kernels are in test_batchmix_gpu.py and test_mixed_loss_gpu.py."""
import numpy as np
import pytest
import torch

import batchmix_ref
from gaviko_amd import ops
from gaviko_amd.data import BatchMix, DataPreprocessor, MixedTarget
from gaviko_amd.losses import CrossEntropyLoss, FocalLoss

SHAPE = (5, 12, 68)


def _same(t, u):
    return all(np.array_equal(t[k], u[k]) and t[k].dtype == u[k].dtype for k in ("mode", "lam", "box", "perm"))


def test_same_seed_same_tables_and_batch_mode_is_uniform():
    a, b = BatchMix(seed=11), BatchMix(seed=11)
    for _ in range(3):
        assert _same(a.sample(6, SHAPE), b.sample(6, SHAPE))
    assert a.last_mix is not None and set(a.last_mix) == {"mode", "lam", "box", "perm"}
    assert not _same(BatchMix(seed=12).sample(6, SHAPE), BatchMix(seed=11).sample(6, SHAPE))
    seen = set()
    for seed in range(40):
        t = BatchMix(mode="batch", seed=seed).sample(6, SHAPE)
        assert (t["mode"] == t["mode"][0]).all() and (t["lam"] == t["lam"][0]).all() and (t["box"] == t["box"][0]).all()
        assert sorted(t["perm"]) == list(range(6))
        seen.add(int(t["mode"][0]))
    assert seen >= {ops.MIX_MIXUP, ops.MIX_CUTMIX}


@pytest.mark.parametrize("kw", [dict(), dict(prob=0.6, switch_prob=0.3), dict(mixup_alpha=0.0), dict(cutmix_alpha=0.0, prob=0.5)])
def test_elem_mode_follows_the_stated_draw_order(kw):
    """per sample: uniform for prob, uniform for the switch, beta of the chosen kind, three box centres; then one permutation"""
    cfg = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5)
    cfg.update(kw)
    B = 7
    for seed in range(25):
        got = BatchMix(seed=seed, **kw).sample(B, SHAPE)
        rng = np.random.default_rng(seed)
        mode, lam, box = np.zeros(B, np.int32), np.ones(B), np.zeros((B, 6), np.int32)
        for b in range(B):
            applied = rng.random() < cfg["prob"]
            u = rng.random()
            cut = (u < cfg["switch_prob"]) if cfg["mixup_alpha"] > 0 and cfg["cutmix_alpha"] > 0 else cfg["cutmix_alpha"] > 0
            alpha = cfg["cutmix_alpha"] if cut else cfg["mixup_alpha"]
            l = rng.beta(alpha, alpha)
            c = [int(rng.integers(n)) for n in SHAPE]
            if not applied:
                continue
            if cut:
                bx, l = batchmix_ref.rand_box(l, c, SHAPE)
                if min(bx[1] - bx[0], bx[3] - bx[2], bx[5] - bx[4]) > 0:
                    mode[b], lam[b], box[b] = ops.MIX_CUTMIX, l, bx
            else:
                mode[b], lam[b] = ops.MIX_MIXUP, l
        perm = rng.permutation(B)
        own = perm == np.arange(B)
        mode[own], lam[own], box[own] = ops.MIX_COPY, 1.0, 0
        assert np.array_equal(got["perm"], perm)
        assert np.array_equal(got["mode"], mode) and np.array_equal(got["lam"], lam) and np.array_equal(got["box"], box), seed


def test_boxes_over_200_seeds():
    D, H, W = SHAPE
    V = D * H * W
    kinds = {0: 0, 1: 0, 2: 0}
    empties = own = 0
    for seed in range(200):
        m = BatchMix(mixup_alpha=0.0, cutmix_alpha=1.0 if seed % 2 else 0.3, seed=seed)
        t = m.sample(5, SHAPE)
        rng = np.random.default_rng(seed)                                  # the raw draws, to find the boxes that came out empty
        raw = []
        for b in range(5):
            rng.random(), rng.random()
            l = rng.beta(m.cutmix_alpha, m.cutmix_alpha)
            raw.append(batchmix_ref.rand_box(l, [int(rng.integers(n)) for n in SHAPE], SHAPE)[0])
        for b in range(5):
            d0, d1, h0, h1, w0, w1 = [int(v) for v in t["box"][b]]
            assert 0 <= d0 <= d1 <= D and 0 <= h0 <= h1 <= H and 0 <= w0 <= w1 <= W
            vol = (d1 - d0) * (h1 - h0) * (w1 - w0)
            kinds[int(t["mode"][b])] += 1
            if t["mode"][b] == ops.MIX_CUTMIX:
                assert vol > 0 and t["lam"][b] == 1.0 - vol / V and tuple(t["box"][b]) == raw[b]
            else:
                assert t["mode"][b] == ops.MIX_COPY and t["lam"][b] == 1.0 and vol == 0
            rb = raw[b]
            if min(rb[1] - rb[0], rb[3] - rb[2], rb[5] - rb[4]) <= 0:
                empties += 1
                assert t["mode"][b] == ops.MIX_COPY and t["lam"][b] == 1.0
            if t["perm"][b] == b:
                own += 1
                assert t["mode"][b] == ops.MIX_COPY and t["lam"][b] == 1.0
    print(f"modes {kinds}, empty boxes {empties}, self-partners {own}")
    assert kinds[ops.MIX_CUTMIX] > 300 and empties > 10 and own > 50 and kinds[ops.MIX_MIXUP] == 0


def test_prob_zero_is_all_copies():
    for mode in ("elem", "batch"):
        t = BatchMix(prob=0.0, mode=mode, seed=5).sample(9, SHAPE)
        assert (t["mode"] == ops.MIX_COPY).all() and (t["lam"] == 1.0).all() and (t["box"] == 0).all()
    # the draws are consumed all the same: the permutation is the one a live instance of the same seed gets
    assert np.array_equal(BatchMix(prob=0.0, seed=5).sample(9, SHAPE)["perm"], BatchMix(prob=1.0, seed=5).sample(9, SHAPE)["perm"])


def test_mixed_target_dense():
    gen = torch.Generator().manual_seed(3)
    B, K = 12, 5
    a, b = torch.randint(0, K, (B,), generator=gen), torch.randint(0, K, (B,), generator=gen)
    lam = torch.rand(B, generator=gen)
    lam[0], lam[1], lam[2] = 0.0, 0.5, 1.0
    t = MixedTarget(a, b, lam)
    for e in (0.0, 0.1):
        d = t.dense(K, e)
        assert d.shape == (B, K) and d.dtype == torch.float64
        assert (d.sum(1) - 1).abs().max().item() < 1e-15
        want = np.zeros((B, K))
        for i in range(B):
            want[i, a[i]] += float(lam[i])
            want[i, b[i]] += 1.0 - float(lam[i])
        want = (1 - e) * want + e / K
        assert np.abs(d.numpy() - want).max() < 1e-15
    one = MixedTarget(a, b, torch.ones(B)).dense(K)
    assert torch.equal(one, torch.nn.functional.one_hot(a, K).double())


def test_errors():
    for kw in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(mixup_alpha=0.0, cutmix_alpha=0.0), dict(prob=1.5), dict(prob=-0.1),
               dict(switch_prob=2.0), dict(switch_prob=-1e-3), dict(mode="pair")):
        with pytest.raises(ValueError):
            BatchMix(**kw)
    with pytest.raises(RuntimeError):
        BatchMix(seed=0)(torch.zeros(2, 1, 4, 4, 4), torch.zeros(2, dtype=torch.int64))
    for crit in (CrossEntropyLoss(), FocalLoss(gamma=1.2)):
        with pytest.raises(NotImplementedError, match="MixedTarget"):
            crit(torch.zeros(3, 5), torch.full((3, 5), 0.2))
    for e in (-0.01, 1.01):
        with pytest.raises(ValueError):
            CrossEntropyLoss(label_smoothing=e)
    assert CrossEntropyLoss(label_smoothing=1.0).label_smoothing == 1.0 and CrossEntropyLoss().label_smoothing == 0.0
    assert (ops.MIX_COPY, ops.MIX_MIXUP, ops.MIX_CUTMIX) == (0, 1, 2)


def test_preprocessor_builds_batch_mix_only_when_asked():
    assert DataPreprocessor({"data": {}}, seed=0).batch_mix is None
    m = DataPreprocessor({"data": {"batch_mix": dict(mixup_alpha=0.2, cutmix_alpha=0.0, seed=4)}}, seed=0).batch_mix
    assert isinstance(m, BatchMix) and m.mixup_alpha == 0.2 and m.cutmix_alpha == 0.0
