"""GPU: gvk_loss_mixed_fwd_bwd (csrc/loss.hip) through ops.loss_mixed_fwd_bwd and the loss modules -- mixed targets (Mixup / CutMix) and label
smoothing in one launch.

Logits are rand * 1.6 - 0.3 as in test_losses_gpu.py, so the focal loss's clamps are live on both sides.  Per-sample losses, every gradient
element and the 'mean' scalar are held to 5e-6 absolute, the bound test_loss_reduction_none_vs_oracle uses for weighted per-sample values of
this magnitude.  The 'sum' SCALAR is a float32 sum of B such values: at B = 257 it is about 440, where float32's spacing alone is 3e-5, so no
float32 result can be held to 5e-6 there.  It is held to what that bound becomes under the sum, B * 5e-6 for the B terms plus the rounding of
the float32 additions on a term's way through the kernel's fixed tree, depth * 2^-24 * sum |l_i| with depth = ceil(log2(min(B, 256))) + (B > 256)
(adding to zero is exact) -- 5e-6 itself at B = 1."""
import math

import pytest
import torch
import torch.nn.functional as F

import oracle
from gaviko_amd import ops
from gaviko_amd.data import MixedTarget
from gaviko_amd.losses import CrossEntropyLoss, FocalLoss, StepMeter

pytestmark = pytest.mark.gpu

TOL = 5e-6
W5 = [0.5, 1.0, 2.0, 1.5, 0.25]
GRID = [(1, 2), (1, 5), (5, 5), (5, 7), (64, 2), (64, 5), (257, 5), (257, 7)]
RED = ("mean", "sum", "none")


def _weights(K):
    return torch.tensor(W5) if K == 5 else torch.linspace(0.5, 2.0, K)


def _case(B, K, seed=0):
    gen = torch.Generator().manual_seed(1000 * B + 10 * K + seed)
    x = torch.rand(B, K, generator=gen) * 1.6 - 0.3
    a, b = torch.randint(0, K, (B,), generator=gen), torch.randint(0, K, (B,), generator=gen)
    lam = torch.rand(B, generator=gen)
    for i, v in enumerate((0.0, 0.5, 1.0)):                                # some exactly 0, 0.5 and 1
        if B > 3:
            lam[i + 1] = v
    if B == 1:
        lam[0] = (0.0, 0.5, 1.0, 0.37)[(K + seed) % 4]
    return x, a, b, lam


def _sum_bound(B, per_row):
    depth = math.ceil(math.log2(min(B, 256))) + (1 if B > 256 else 0)
    return B * TOL + 1.01 * depth * 2.0 ** -24 * float(per_row.abs().sum())


def _mixed(dev, x, a, b, lam, kind, red, w=None, e=0.0, gamma=0.0, meter=None):
    B = x.shape[0]
    loss = torch.full((B if red == "none" else 1,), float("nan"), device=dev)
    dl = torch.full(x.shape, float("nan"), device=dev)
    ops.loss_mixed_fwd_bwd(x.to(dev), a.to(dev), None if b is None else b.to(dev), None if lam is None else lam.to(dev), loss, dl, kind, gamma=gamma,
                           smoothing=e, weights=None if w is None else w.to(dev), meter=meter, reduction=red)
    return loss.cpu(), dl.cpu()


def _pair_ref(x, a, b, lam, kind, w, e=0.0, gamma=0.0):
    """float64, with autograd: (per-row losses, the 'mean' denominator) of lam l(x, a) + (1 - lam) l(x, b); rows with an ignored label give 0"""
    ign = (a == -100) | (b == -100)
    a0, b0 = a.masked_fill(ign, 0), b.masked_fill(ign, 0)
    w64 = None if w is None else w.double()
    if kind == ops.LOSS_CE:
        la = F.cross_entropy(x, a0, weight=w64, label_smoothing=e, reduction="none")
        lb = F.cross_entropy(x, b0, weight=w64, label_smoothing=e, reduction="none")
    else:
        la = oracle.focal_loss(x, a0, gamma=gamma, weights=w64, reduction="none")
        lb = oracle.focal_loss(x, b0, gamma=gamma, weights=w64, reduction="none")
    lam = lam.double()
    wa, wb = (torch.ones(len(a)).double(), torch.ones(len(a)).double()) if w is None else (w64[a0], w64[b0])
    keep = (~ign).double()
    return (lam * la + (1 - lam) * lb) * keep, ((lam * wa + (1 - lam) * wb) * keep).sum()


def _check(tag, got, x64, per_row, den, red, up=None):
    """one launch (loss, dlogits) against the float64 rows `per_row`, which autograd connects to the leaf x64"""
    got_loss, got_grad = got
    if red == "none":
        want, bound = per_row, TOL
        (per_row * up.double()).sum().backward()
        gwant = x64.grad / up.double().view(-1, 1)                          # each row's own gradient
    elif red == "sum":
        want, bound = per_row.sum().view(1), _sum_bound(per_row.shape[0], per_row.detach())
        want.sum().backward()
        gwant = x64.grad
    else:
        want, bound = (per_row.sum() / den).view(1), TOL
        want.sum().backward()
        gwant = x64.grad
    el = (got_loss.double() - want.detach()).abs().max().item()
    eg = (got_grad.double() - gwant).abs().max().item()
    print(f"{tag} {red}: loss err {el:.2e} (bound {bound:.2e}), grad err {eg:.2e} (bound {TOL:.0e})")
    assert el <= bound and eg <= TOL


def _leaf(x):
    return x.double().clone().requires_grad_(True)


@pytest.mark.parametrize("B,K", GRID)
def test_identity_with_the_plain_kernel_is_bitwise(dev, B, K):
    """smoothing 0, b = a, lam = 1 -- and no partner at all -- return the bits of gvk_loss_fwd_bwd: both kinds, all reductions, weights on and off,
    two ignored rows, and the meter gains the same three numbers"""
    x, a, _, _ = _case(B, K)
    if B >= 5:
        a[1] = a[B - 2] = -100
    ones = torch.ones(B)
    for kind, gamma in ((ops.LOSS_CE, 0.0), (ops.LOSS_FOCAL, 1.2)):
        for red in RED:
            for w in (None, _weights(K)):
                m0 = torch.tensor([0.25, 3.0, 7.0], device=dev)
                loss = torch.full((B if red == "none" else 1,), float("nan"), device=dev)
                dl = torch.full(x.shape, float("nan"), device=dev)
                ops.loss_fwd_bwd(x.to(dev), a.to(dev), loss, dl, kind, gamma=gamma, weights=None if w is None else w.to(dev), meter=m0, reduction=red)
                for b_, lam_ in ((a, ones), (None, None)):
                    m1 = torch.tensor([0.25, 3.0, 7.0], device=dev)
                    l1, d1 = _mixed(dev, x, a, b_, lam_, kind, red, w, 0.0, gamma, meter=m1)
                    assert torch.equal(l1.view(torch.int32), loss.cpu().view(torch.int32)), (kind, red, w is None)
                    assert torch.equal(d1.view(torch.int32), dl.cpu().view(torch.int32)), (kind, red, w is None)
                    assert torch.equal(m1.view(torch.int32), m0.view(torch.int32))
                assert not torch.isnan(dl).any() and not torch.isnan(loss).any()


@pytest.mark.parametrize("e", [0.0, 0.1])
@pytest.mark.parametrize("B,K", GRID)
def test_cross_entropy_against_torch_probability_targets(dev, B, K, e):
    """F.cross_entropy on the dense rows of MixedTarget.dense, CPU float64: 'none' under a random per-row upstream gradient, and 'sum'; 'mean'
    against the float64 pair form with the kernel's own denominator (torch's probability-target mean divides by B: the documented deviation)"""
    x, a, b, lam = _case(B, K, seed=int(e * 10))
    up = torch.rand(B, generator=torch.Generator().manual_seed(B + K)) + 0.5
    dense = MixedTarget(a, b, lam).dense(K)
    for w in (None, _weights(K)):
        for red in ("none", "sum"):
            x64 = _leaf(x)
            rows = F.cross_entropy(x64, dense, weight=None if w is None else w.double(), label_smoothing=e, reduction="none")
            got = _mixed(dev, x, a, b, lam, ops.LOSS_CE, red, w, e)
            _check(f"CE B={B} K={K} e={e} w={'on' if w is not None else 'off'}", got, x64, rows, None, red, up)
        x64 = _leaf(x)
        rows, den = _pair_ref(x64, a, b, lam, ops.LOSS_CE, w, e)
        _check(f"CE B={B} K={K} e={e} w={'on' if w is not None else 'off'}", _mixed(dev, x, a, b, lam, ops.LOSS_CE, "mean", w, e), x64, rows, den, "mean")


@pytest.mark.parametrize("red", RED)
def test_label_smoothing_on_class_indices_against_torch(dev, red):
    """CrossEntropyLoss(label_smoothing=0.1) on int64 targets = F.cross_entropy(..., label_smoothing=0.1), weights and ignored rows included"""
    B, K = 64, 5
    x, y, _, _ = _case(B, K, seed=4)
    y[3] = y[40] = -100
    up = (torch.rand(B, generator=torch.Generator().manual_seed(9)) + 0.5) if red == "none" else torch.ones(1)
    for w in (None, _weights(K)):
        w64 = None if w is None else w.double()
        x64 = _leaf(x)
        want = F.cross_entropy(x64, y, weight=w64, label_smoothing=0.1, reduction=red)
        (want * up.double()).sum().backward()
        xg = x.to(dev).requires_grad_(True)
        got = CrossEntropyLoss(weight=w, reduction=red, label_smoothing=0.1)(xg, y.to(dev))
        (got * up.to(dev)).sum().backward()
        bound = _sum_bound(B, F.cross_entropy(x.double(), y, weight=w64, label_smoothing=0.1, reduction="none")) if red == "sum" else TOL
        el = (got.detach().cpu().double() - want.detach()).abs().max().item()
        eg = ((xg.grad.cpu().double() - x64.grad).abs() / up.double().view(-1, 1)).max().item()      # each row's own gradient
        print(f"smoothing {red} w={'on' if w is not None else 'off'}: loss err {el:.2e} (bound {bound:.2e}), grad err {eg:.2e} (bound {TOL:.0e})")
        assert el <= bound and eg <= TOL
        if red == "none":
            assert float(got.detach()[3]) == 0.0 and float(got.detach()[40]) == 0.0
        assert (xg.grad[3] == 0).all() and (xg.grad[40] == 0).all()


@pytest.mark.parametrize("gamma", [0.5, 1.2, 2.0])
@pytest.mark.parametrize("B,K", GRID)
def test_focal_against_the_float64_pair_form(dev, B, K, gamma):
    x, a, b, lam = _case(B, K, seed=7)
    up = torch.rand(B, generator=torch.Generator().manual_seed(B * K)) + 0.5
    for w in (None, _weights(K)):
        for red in RED:
            x64 = _leaf(x)
            rows, den = _pair_ref(x64, a, b, lam, ops.LOSS_FOCAL, w, 0.0, gamma)
            got = _mixed(dev, x, a, b, lam, ops.LOSS_FOCAL, red, w, 0.0, gamma)
            _check(f"focal B={B} K={K} g={gamma} w={'on' if w is not None else 'off'}", got, x64, rows, den, red, up)
            outside = (x < 1e-16) | (x > 1 - 1e-16)                       # the clamp kills these gradients exactly
            assert (got[1][outside] == 0).all() and (B * K < 10 or outside.any())


@pytest.mark.parametrize("kind", [ops.LOSS_CE, ops.LOSS_FOCAL])
def test_ignored_rows(dev, kind):
    """a row whose a OR b is ignore_index: loss 0, gradient row 0, and no share of the mean's denominator"""
    B, K = 64, 5
    x, a, b, lam = _case(B, K, seed=2)
    a[5], b[9], b[20], a[20] = -100, -100, -100, -100
    w = _weights(K)
    gamma = 1.2 if kind == ops.LOSS_FOCAL else 0.0
    loss, dl = _mixed(dev, x, a, b, lam, kind, "none", w, 0.0, gamma)
    for i in (5, 9, 20):
        assert float(loss[i]) == 0.0 and (dl[i] == 0).all()
    for red in ("mean", "sum"):
        x64 = _leaf(x)
        rows, den = _pair_ref(x64, a, b, lam, kind, w, 0.0, gamma)
        got = _mixed(dev, x, a, b, lam, kind, red, w, 0.0, gamma)
        _check(f"ignored kind={kind}", got, x64, rows, den, red)
        assert (got[1][[5, 9, 20]] == 0).all()
    with pytest.raises(ValueError):
        ops.loss_mixed_fwd_bwd(x.to(dev), a.to(dev), b.to(dev), None, loss.to(dev), dl.to(dev), kind)
    with pytest.raises(ValueError):
        ops.loss_mixed_fwd_bwd(x.to(dev), a.to(dev), None, None, loss.to(dev), dl.to(dev), ops.LOSS_FOCAL, smoothing=0.1)
    with pytest.raises(ValueError):
        ops.loss_mixed_fwd_bwd(x.to(dev), a.to(dev), None, None, loss.to(dev), dl.to(dev), ops.LOSS_CE, smoothing=1.5)


def test_meter_counts_once_and_by_the_dominant_label(dev):
    B, K = 64, 5
    x, a, b, lam = _case(B, K, seed=3)
    # rows 0..4: the argmax is b and not a, lam on either side of 0.5 and exactly 0.5; rows 5, 6: the argmax is a and not b
    for i, l in enumerate((0.3, 0.7, 0.5, 0.49999997, 0.0)):
        a[i], b[i], lam[i] = 1, 3, l
        x[i] = torch.tensor([0.1, 0.2, 0.3, 0.9, 0.0])
    for i, l in ((5, 0.7), (6, 0.3)):
        a[i], b[i], lam[i] = 2, 0, l
        x[i] = torch.tensor([0.1, 0.2, 0.95, 0.3, 0.0])
    am = x.argmax(-1)
    dominant = torch.where(lam >= 0.5, a, b)
    correct = int((am == dominant).sum())
    assert [bool(am[i] == dominant[i]) for i in range(7)] == [True, False, False, True, True, True, False]
    for crit, kind, gamma in ((CrossEntropyLoss(), ops.LOSS_CE, 0.0), (FocalLoss(gamma=1.2), ops.LOSS_FOCAL, 1.2)):
        meter = StepMeter(dev)
        crit.attach_meter(meter)
        for _ in range(2):                                              # two steps accumulate; one launch each counts the batch once
            crit(x.to(dev), MixedTarget(a.to(dev), b.to(dev), lam.to(dev)))
        rows, den = _pair_ref(x.double(), a, b, lam, kind, None, 0.0, gamma)
        want = float(rows.sum() / den)
        mean_loss, acc, n = meter.read()
        print(f"meter kind={kind}: mean loss {mean_loss:.7f} vs {want:.7f}, accuracy {acc:.4f} vs {correct / B:.4f}, n {n}")
        assert n == 2 * B and abs(mean_loss - want) <= 1e-5 * max(1.0, abs(want)) and abs(acc - correct / B) < 1e-6


@pytest.mark.parametrize("red", ["mean", "none"])
def test_autograd_scales_the_kernel_gradient(dev, red):
    B, K = 5, 5
    x, a, b, lam = _case(B, K, seed=6)
    w = _weights(K)
    t = MixedTarget(a.to(dev), b.to(dev), lam.to(dev))
    for crit, kind, gamma, e in ((CrossEntropyLoss(weight=w, reduction=red, label_smoothing=0.1), ops.LOSS_CE, 0.0, 0.1),
                                 (FocalLoss(gamma=1.2, weights=w, reduction=red), ops.LOSS_FOCAL, 1.2, 0.0)):
        loss, dl = _mixed(dev, x, a, b, lam, kind, red, w, e, gamma)
        xg = x.to(dev).requires_grad_(True)
        out = crit(xg, t)
        assert torch.equal(out.detach().cpu().view(-1), loss.view(-1))
        up = torch.tensor([0.5, 1.5, 2.0, 0.25, 3.0]) if red == "none" else torch.tensor(2.5)
        (out * up.to(dev)).sum().backward()
        assert torch.equal(xg.grad.cpu(), dl * (up.view(-1, 1) if red == "none" else up))
