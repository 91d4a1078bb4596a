"""GPU: the loss seeds of csrc/loss.hip (gvk_loss_fwd_bwd, gvk_loss_mixed_fwd_bwd) at their edges, through ops.loss_fwd_bwd and
ops.loss_mixed_fwd_bwd, against oracle.cross_entropy / oracle.focal_loss in float64.

Every case runs in three MODES: "plain" (gvk_loss_fwd_bwd), "nopartner" (the mixed kernel with target_b = lam = None) and "pair" (the mixed
kernel with a partner label and lam in {0, 0.3, 0.5, 1} by row).  The reference of a pair is the float64 pair form of test_mixed_loss_gpu.py,
lam l(x, a) + (1 - lam) l(x, b) on the oracle's reduction='none' rows; plain and nopartner are that form with b = a, lam = 1.

Bounds (the existing tests'): 5e-6 for per-sample losses, gradient elements and the cross entropy's 'mean' scalar, 2e-6 for the focal 'mean'
scalar, each relative to max(1, |want|) where a value is larger than 1.  The 'sum' scalar follows _sum_bound of test_mixed_loss_gpu.py, for the
reason given there, with the per-row part taken relative in the same way: sum_i 5e-6 max(1, |l_i|) + depth 2^-24 sum_i |l_i|.  No bound here
was derived from the kernel's output, and none had to be widened by the measured-float32-oracle rule."""
import math

import numpy as np
import pytest
import torch

import oracle
from gaviko_amd import ops
from test_mixed_loss_gpu import TOL, W5, _pair_ref

pytestmark = pytest.mark.gpu

MODES = ("plain", "nopartner", "pair")
RED = ("mean", "sum", "none")
KINDS = ((ops.LOSS_CE, 0.0), (ops.LOSS_FOCAL, 1.2))
LAMS = (0.0, 0.3, 0.5, 1.0)
FOCAL_MEAN_TOL = 2e-6
IGN = -100
NAN = float("nan")


# ---- running and checking --------------------------------------------------------------------------------------------------------------
def _lam(B):
    return torch.tensor([LAMS[i % 4] for i in range(B)])


def _effective(mode, a, b, lam):
    """the (a, b, lam) the mode computes with: plain and nopartner have no partner"""
    return (a, b, lam) if mode == "pair" else (a, a, torch.ones(len(a)))


def _launch(dev, mode, x, a, b, lam, kind, red, w=None, gamma=0.0, meter=None):
    """one launch on device tensors x [B, K], w [K] (views are fine); a, b, lam are CPU tensors"""
    B = x.shape[0]
    loss = torch.full((B if red == "none" else 1,), 3.0, device=dev)
    dl = torch.full(tuple(x.shape), 3.0, device=dev)
    if mode == "plain":
        ops.loss_fwd_bwd(x, a.to(dev), loss, dl, kind, gamma=gamma, weights=w, meter=meter, reduction=red)
    else:
        pair = mode == "pair"
        ops.loss_mixed_fwd_bwd(x, a.to(dev), b.to(dev) if pair else None, lam.to(dev) if pair else None, loss, dl, kind, gamma=gamma,
                               weights=w, meter=meter, reduction=red)
    return loss.cpu(), dl.cpu()


def _run(dev, mode, x, a, b, lam, kind, red, w=None, gamma=0.0, meter=None):
    return _launch(dev, mode, x.to(dev), a, b, lam, kind, red, None if w is None else w.to(dev), gamma, meter)


def _reference(x, a, b, lam, kind, w, gamma):
    """float64: per-row losses [B], each row's own gradient [B, K], the 'mean' denominator"""
    x64 = x.double().clone().requires_grad_(True)
    rows, den = _pair_ref(x64, a, b, lam, kind, w, 0.0, gamma)
    rows.sum().backward()                                                  # row i of x64.grad is d rows_i / d x_i: the rows do not mix
    return rows.detach(), x64.grad.clone(), float(den)


def _rel_err(got, want):
    return ((got.double() - want).abs() / want.abs().clamp(min=1.0)).max().item()


def _sum_bound(rows):
    B = rows.numel()
    depth = math.ceil(math.log2(min(B, 256))) + (1 if B > 256 else 0) if B > 1 else 0
    return float((TOL * rows.abs().clamp(min=1.0)).sum()) + 1.01 * depth * 2.0 ** -24 * float(rows.abs().sum())


def _check(tag, got, ref, kind, red):
    """(loss, dlogits) of one launch against _reference's (rows, row gradients, den)"""
    (loss, dl), (rows, grads, den) = got, ref
    if red == "none":
        el, bound, eg = _rel_err(loss, rows), TOL, _rel_err(dl, grads)
    elif red == "sum":
        el, bound, eg = abs(float(loss[0]) - float(rows.sum())), _sum_bound(rows), _rel_err(dl, grads)
    else:
        want = float(rows.sum()) / den
        el, bound = abs(float(loss[0]) - want) / max(1.0, abs(want)), (TOL if kind == ops.LOSS_CE else FOCAL_MEAN_TOL)
        eg = _rel_err(dl, grads / den)
    print(f"{tag} {red}: loss err {el:.2e} (bound {bound:.2e}), grad err {eg:.2e} (bound {TOL:.0e})")
    assert el <= bound and eg <= TOL, tag


def _logits(kind, B, K, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == ops.LOSS_CE:
        return torch.randn(B, K, generator=gen) * 1.5
    return torch.rand(B, K, generator=gen) * 1.6 - 0.3                    # the focal clamps are live on both sides


def _labels(B, K, seed):
    gen = torch.Generator().manual_seed(seed + 77)
    return torch.randint(0, K, (B,), generator=gen), torch.randint(0, K, (B,), generator=gen)


def _same_nan_pattern(got, want):
    got, want = got.double(), want.double()
    return bool((torch.isnan(got) == torch.isnan(want)).all()) and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


# ---- thread stride and reduction tree --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 511, 513])
def test_rows_at_the_thread_stride(dev, B, mode):
    """B around the 256 threads of the one workgroup and their second lap.  Row b's logits are scaled by 1 + b / B, so its loss depends on b:
    a row dropped, counted twice or swapped moves the per-sample vector and the scalars by far more than the bounds"""
    K = 5
    w = torch.tensor(W5)
    scale = (1.0 + torch.arange(B) / B).view(B, 1)
    for kind, gamma in KINDS:
        x = _logits(kind, B, K, 10 * B + kind) * scale
        a, b = _labels(B, K, B)
        if B >= 5:
            a[1] = a[B - 2] = IGN
            b[3] = IGN                                                    # ignored through the partner (pair mode only)
        a, b, lam = _effective(mode, a, b, _lam(B))
        ref = _reference(x, a, b, lam, kind, w, gamma)
        if B >= 5:
            assert float(ref[0][1]) == 0.0 and float(ref[0][0]) != float(ref[0][B - 1])
        for red in RED:
            got = _run(dev, mode, x, a, b, lam, kind, red, w, gamma)
            _check(f"stride {mode} kind={kind} B={B}", got, ref, kind, red)
            ign = (a == IGN) | (b == IGN)
            assert (got[1][ign] == 0).all() and (red != "none" or (got[0][ign] == 0).all())


# ---- class counts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", [2, 64, 1000, 4096])
def test_class_counts_up_to_the_entry_points_limit(dev, K, mode):
    """B = 3: the target is the first class, the last class and the argmax"""
    B = 3
    w = torch.linspace(0.5, 2.0, K)
    for kind, gamma in KINDS:
        x = _logits(kind, B, K, 100 + K + kind)
        a = torch.tensor([0, K - 1, int(x[2].argmax())])
        b = torch.tensor([K - 1, int(x[1].argmax()), 0])
        a, b, lam = _effective(mode, a, b, torch.tensor([0.3, 0.5, 0.0]))
        ref = _reference(x, a, b, lam, kind, w, gamma)
        for red in RED:
            _check(f"classes {mode} kind={kind} K={K}", _run(dev, mode, x, a, b, lam, kind, red, w, gamma), ref, kind, red)


def test_the_entry_points_refuse_more_classes(dev):
    from gaviko_amd.lib import GavikoHipError
    x = torch.zeros(2, 4097, device=dev)
    y = torch.zeros(2, dtype=torch.int64, device=dev)
    loss, dl = torch.zeros(1, device=dev), torch.zeros(2, 4097, device=dev)
    with pytest.raises(GavikoHipError):
        ops.loss_fwd_bwd(x, y, loss, dl, ops.LOSS_CE)
    with pytest.raises(GavikoHipError):
        ops.loss_mixed_fwd_bwd(x, y, None, None, loss, dl, ops.LOSS_CE)


# ---- logit range, cross entropy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_cross_entropy_over_the_logit_range(dev, mode):
    """rows shifted by +-1e4, rows with a spread of 200 (exp(-200) is exactly 0 in float32; the target at the bottom and at the top), a row of
    all-equal logits: finite, and the float64 value.  The shifted rows hold log s + (m - x_t) to the bound only if m - x_t is formed first."""
    K = 5
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(7, K, generator=gen)
    x = base.clone()
    x[0] += 1e4
    x[1] -= 1e4
    x[2] = base[2] / 8 - 100
    x[2, 3] += 200                                                         # the target (1) is 200 below the maximum: loss about 200
    x[3] = base[3] / 8 - 100
    x[3, 2] += 200                                                         # the target is the maximum: loss about 0
    x[4] = 0.75
    x[5] = base[5] * 3 + 1e4
    a = torch.tensor([1, 4, 1, 2, 3, 0, 2])
    b = torch.tensor([3, 0, 3, 1, 0, 0, 4])
    w = torch.tensor(W5)
    a, b, lam = _effective(mode, a, b, _lam(7))
    assert float(torch.exp(torch.tensor(-200.0))) == 0.0
    for weights in (None, w):
        ref = _reference(x, a, b, lam, ops.LOSS_CE, weights, 0.0)
        assert torch.isfinite(ref[0]).all() and float(ref[0].max()) > 100
        for red in RED:
            got = _run(dev, mode, x, a, b, lam, ops.LOSS_CE, red, weights)
            assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
            _check(f"range {mode} w={'on' if weights is not None else 'off'}", got, ref, ops.LOSS_CE, red)


# ---- focal clamp edges -----------------------------------------------------------------------------------------------------------------
def _edge_rows():
    """float32 logits at the clamp's edges [1e-16, 1 - 1e-16], and the float64 rows the oracle is given for them.  float32 cannot tell
    1 - 1e-16 from 1: the clamp's upper bound IS 1.0f there, a logit of 1.0f lies inside it, and the reference class (float32) lets its gradient
    through -- so the float64 oracle is given 1 - 1e-16 = 0.9999999999999999, the largest double inside its clamp, wherever the kernel gets 1.0f.
    Every other value is the same number in both.  Returns (x32, x64, inside) with inside = the logits whose gradient is not clamped away."""
    f = np.float32
    lo, one = f(1e-16), f(1.0)
    below0, above1 = np.nextafter(f(0), f(-1)), np.nextafter(one, f(2))
    edges = [f(0), lo, one, one, below0, above1, f(-1e-30), np.nextafter(one, f(0)), f(2e-16), np.nextafter(lo, f(0))]
    inside = [False, True, True, True, False, False, False, True, True, False]
    rows, ins = [], []
    E = len(edges)
    for s in range(E):                                                     # five consecutive edges per row, every edge in every column
        rows.append([edges[(s + k) % E] for k in range(5)])
        ins.append([inside[(s + k) % E] for k in range(5)])
    for e, i in zip(edges, inside):                                        # one edge among ordinary logits, and whole rows of one edge
        rows.append([f(0.3), e, f(0.7), f(0.55), f(0.1)])
        ins.append([True, i, True, True, True])
        rows.append([e] * 5)
        ins.append([i] * 5)
    x32 = torch.from_numpy(np.array(rows, dtype=np.float32))
    x64 = x32.double()
    x64[x32 == 1.0] = 1.0 - 1e-16
    return x32, x64, torch.tensor(ins)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 1.2, 2.0])
def test_focal_at_the_clamp_edges(dev, gamma, mode):
    """the gradient is exactly 0 for every logit outside the clamp and the oracle's inside it; gamma = 0 and gamma = 1 are the special values of
    powf(1 - pt, gamma - 1)"""
    x32, x64, inside = _edge_rows()
    B, K = x32.shape
    a = torch.arange(B) % K
    b = (torch.arange(B) * 2 + 1) % K
    a, b, lam = _effective(mode, a, b, _lam(B))
    w = torch.tensor(W5)
    leaf = x64.clone().requires_grad_(True)
    rows, den = _pair_ref(leaf, a, b, lam, ops.LOSS_FOCAL, w, 0.0, gamma)
    rows.sum().backward()
    ref = (rows.detach(), leaf.grad.clone(), float(den))
    assert (ref[1][~inside] == 0).all() and (ref[1][inside] != 0).all()    # the oracle agrees on what is inside
    # the reference in float32, as it executes, draws the same line (CPU)
    l32 = x32.clone().requires_grad_(True)
    oracle.focal_loss(l32, a, gamma=gamma, weights=w, reduction="sum").backward()
    assert ((l32.grad != 0) == inside).all()
    for red in RED:
        got = _run(dev, mode, x32, a, b, lam, ops.LOSS_FOCAL, red, w, gamma)
        assert (got[1][~inside] == 0).all(), f"gamma={gamma} {red}: a clamped logit has a gradient"
        assert (got[1][inside] != 0).all()
        _check(f"clamp {mode} gamma={gamma}", got, ref, ops.LOSS_FOCAL, red)


# ---- zero class weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_zero_class_weights_for_some_rows(dev, mode):
    B, K = 40, 5
    w = torch.tensor([0.5, 0.0, 2.0, 0.0, 1.0])
    for kind, gamma in KINDS:
        x = _logits(kind, B, K, 500 + kind)
        a, b = _labels(B, K, 5)
        a[7] = IGN
        a, b, lam = _effective(mode, a, b, _lam(B))
        zero = (w[a.clamp(min=0)] == 0) & (w[b.clamp(min=0)] == 0) & (a != IGN)
        assert zero.any() and not zero.all()
        ref = _reference(x, a, b, lam, kind, w, gamma)
        assert (ref[0][zero] == 0).all()
        for red in RED:
            got = _run(dev, mode, x, a, b, lam, kind, red, w, gamma)
            _check(f"zero weights {mode} kind={kind}", got, ref, kind, red)
            assert (got[1][zero] == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_zero_class_weights_for_every_row_that_counts(dev, mode):
    """'mean' with a zero denominator that is not an all-ignored batch: whatever the oracle returns (float32 on the CPU, the pattern does not
    depend on the precision).  torch's cross entropy: NaN loss, NaN rows, zero rows where ignored.  The focal oracle: NaN everywhere."""
    B, K = 9, 5
    w = torch.tensor([0.5, 0.0, 2.0, 0.0, 1.0])
    a = torch.tensor([1, 3, 1, IGN, 3, 3, 1, IGN, 1])
    b = torch.tensor([3, 3, 1, 2, 1, 3, 1, 0, 3])                        # zero-weight partners: the loss is the one of a alone, for every lam
    for kind, gamma in KINDS:
        x = _logits(kind, B, K, 600 + kind)
        leaf = x.clone().requires_grad_(True)
        want = (oracle.cross_entropy(leaf, a, weight=w) if kind == ops.LOSS_CE else oracle.focal_loss(leaf, a, gamma=gamma, weights=w))
        want.backward()
        assert torch.isnan(want)
        loss, dl = _run(dev, mode, x, *_effective(mode, a, b, _lam(B)), kind, "mean", w, gamma)
        assert torch.isnan(loss).all()
        assert _same_nan_pattern(dl, leaf.grad), f"kind={kind}\n{dl}\n{leaf.grad}"


# ---- every row ignored -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 257])
def test_every_row_ignored(dev, B, mode):
    """cross entropy: torch's answer on the CPU -- NaN under 'mean', 0 under 'sum', zeros under 'none', and all-zero gradients every time (a NaN
    gradient here would poison every trainable tensor at the next step).  Focal: the oracle's NaN pattern (NaN loss and gradients under 'mean')."""
    K = 5
    a = torch.full((B,), IGN)
    _, b = _labels(B, K, 9)
    b[::2] = IGN                                                           # the partner is a class on some rows: ignored all the same
    w = torch.tensor(W5)
    for kind, gamma in KINDS:
        x = _logits(kind, B, K, 700 + kind)
        for weights in (None, w):
            for red in RED:
                leaf = x.clone().requires_grad_(True)
                want = (oracle.cross_entropy(leaf, a, weight=weights, reduction=red) if kind == ops.LOSS_CE
                        else oracle.focal_loss(leaf, a, gamma=gamma, weights=weights, reduction=red))
                want.sum().backward()
                loss, dl = _run(dev, mode, x, *_effective(mode, a, b, _lam(B)), kind, red, weights, gamma)
                assert _same_nan_pattern(loss, want.detach().view(-1)), (kind, red, loss, want)
                assert _same_nan_pattern(dl, leaf.grad), (kind, red)
                if kind == ops.LOSS_CE:
                    assert (dl == 0).all() and (red != "mean" or torch.isnan(loss).all()) and (red == "mean" or (loss == 0).all())
                elif red == "mean":                                       # NaN wherever the clamp lets a gradient through, 0 where it does not
                    inside = (x >= np.float32(1e-16)) & (x <= 1.0)
                    assert inside.any() and not inside.all() and torch.equal(torch.isnan(dl), inside)
                else:
                    assert (dl == 0).all()


# ---- meter -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_meter_ties_ignored_rows_and_three_reductions(dev, mode):
    """meter += (loss * B, correct, B) per step.  An exact argmax tie counts as correct only when the label is the FIRST maximum (torch.argmax);
    ignored rows count in the samples and not in correct; three steps of three reductions add up to a hand sum: 'mean' adds mean * B, 'sum'
    adds sum * B, 'none' adds the sum of the per-sample losses (losses.StepMeter).  The loss sum is held to 1e-5 relative, as the existing
    meter tests hold it; the counts are integers in float32 and exact."""
    K = 5
    rows = [([0.9, 0.1, 0.9, 0.2, 0.0], 0, True),                          # a tie: the label is the first maximum
            ([0.9, 0.1, 0.9, 0.2, 0.0], 2, False),                         # ... the second
            ([0.5, 0.5, 0.5, 0.5, 0.5], 0, True),                          # all equal: class 0
            ([0.5, 0.5, 0.5, 0.5, 0.5], 4, False),
            ([0.1, 0.3, 0.2, 0.8, 0.8], 3, True),
            ([0.2, 0.6, 0.6, 0.6, 0.1], 1, True),                          # three maxima: the first counts,
            ([0.2, 0.6, 0.6, 0.6, 0.1], 2, False),                         # the middle one does not
            ([0.1, 0.7, 0.2, 0.3, 0.4], 1, True),                          # no tie
            ([0.1, 0.7, 0.2, 0.3, 0.4], IGN, False),                       # rows 8, 9 are ignored: samples, never correct
            ([0.7, 0.1, 0.2, 0.3, 0.4], IGN, False),
            ([0.1, 0.7, 0.2, 0.3, 0.4], 3, False)]
    # more first-maximum labels than last-maximum ones: an argmax that takes the LAST maximum counts fewer rows
    assert sum(r[2] for r in rows) == 5 and sum(r[1] != IGN and r[1] == max(k for k in range(K) if r[0][k] == max(r[0])) for r in rows) == 3
    x = torch.tensor([r[0] for r in rows])
    lab = torch.tensor([r[1] for r in rows])
    B = len(rows)
    other = torch.tensor([(r[1] + 1) % K if r[1] != IGN else 0 for r in rows])
    if mode == "pair":                                                     # the dominant label carries the row's label: a where lam >= 0.5, else b
        lam = _lam(B)
        a, b = torch.where(lam >= 0.5, lab, other), torch.where(lam >= 0.5, other, lab)
        b[8], a[9] = IGN, IGN                                              # ignored through either side
    else:
        a, b, lam = lab, lab, torch.ones(B)
    correct = sum(r[2] for r in rows)
    w = torch.tensor(W5)
    for kind, gamma in KINDS:
        ref_rows, _, den = _reference(x, a, b, lam, kind, w, gamma)
        total = float(ref_rows.sum())
        meter = torch.zeros(3, device=dev)
        for red in RED:
            _run(dev, mode, x, a, b, lam, kind, red, w, gamma, meter=meter)
        got = meter.cpu().double()
        want = total / den * B + total * B + total
        print(f"meter {mode} kind={kind}: loss sum {got[0]:.6f} vs {want:.6f}, correct {got[1]:.0f} vs {3 * correct}, samples {got[2]:.0f}")
        assert abs(float(got[0]) - want) <= 1e-5 * max(1.0, abs(want))
        assert float(got[1]) == 3 * correct and float(got[2]) == 3 * B


# ---- labels that are not classes -------------------------------------------------------------------------------------------------------
PAD_ROWS = 8
SENTINEL = 7.0
BAD = (5, 6, -1, -7, 2 ** 32 + 1)                                         # K, K + 1, -1, -7 and 2^32 + 1 at K = 5: no other values


def _middle(dev, t, pad):
    """t in the middle of a larger allocation whose other elements hold SENTINEL"""
    big = torch.full((t.numel() + 2 * pad,), SENTINEL, device=dev)
    view = big[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return big, view


def _intact(big, pad):
    return bool((big[:pad] == SENTINEL).all()) and bool((big[-pad:] == SENTINEL).all())


@pytest.mark.parametrize("mode", MODES)
def test_labels_that_are_not_classes(dev, mode):
    """A label that is neither ignore_index nor in [0, K) -- a label file numbered 1..K, or 2^32 + 1, which an int cast would take for class 1 --
    makes its row NaN in loss and gradient and the 'mean' / 'sum' scalar NaN, adds nothing to the meter's correct count, and leaves every other
    row the oracle's value on the good rows alone.  logits and weights are views into the middle of larger allocations with 8 rows / 8 weights
    of a finite sentinel on either side: an index formed from such a label would stay inside memory this test owns and read a finite number."""
    K = 5
    B = 14
    w = torch.tensor(W5)
    bad_rows = [1, 4, 6, 9, B - 1]
    for kind, gamma in KINDS:
        x = _logits(kind, B, K, 800 + kind)
        a, b = _labels(B, K, 13)
        a[2] = IGN
        for r in bad_rows:                                                 # the row's argmax is class 1: what 2^32 + 1 truncates to
            x[r, 1] = x[r].max() + 0.25
        lam = _lam(B)
        bad_in = []
        for n, (r, v) in enumerate(zip(bad_rows, BAD)):
            if mode == "pair" and n % 2 == 1:
                b[r] = v                                                   # through the partner; lam[r] is 0, 0.3, 0.5 or 1 by its row
                bad_in.append("b")
            else:
                a[r] = v
                bad_in.append("a")
        if mode == "pair":
            assert "b" in bad_in and 0.0 < float(lam[9]) < 0.5 and float(lam[4]) == 0.0
            b[6], lam[6] = BAD[0], 1.0                                     # both labels bad; and a bad partner whose coefficient is zero
            a[11], b[11], lam[11] = 0, BAD[3], 1.0
            bad_rows_m = bad_rows + [11]
        else:
            bad_rows_m = bad_rows
        a, b, lam = _effective(mode, a, b, lam)
        bad = torch.zeros(B, dtype=torch.bool)
        bad[bad_rows_m] = True
        good = ~bad
        dominant = torch.where(lam >= 0.5, a, b)
        x[0, dominant[0]] = x[0].max() + 0.25                              # one good row is right for certain
        ref = _reference(x[good], a[good], b[good], lam[good], kind, w, gamma)
        correct = int(((x.argmax(1) == dominant) & good & (a != IGN) & (b != IGN)).sum())
        assert correct > 0 and good[0]
        big_x, xd = _middle(dev, x, PAD_ROWS * K)
        big_w, wd = _middle(dev, w, PAD_ROWS)
        for red in RED:
            meter = torch.zeros(3, device=dev)
            loss, dl = _launch(dev, mode, xd, a, b, lam, kind, red, wd, gamma, meter=meter)
            assert torch.isnan(dl[bad]).all(), f"{mode} kind={kind} {red}: a bad row has a gradient"
            assert not torch.isnan(dl[good]).any()
            if red == "none":
                assert torch.isnan(loss[bad]).all() and not torch.isnan(loss[good]).any()
                _check(f"bad labels {mode} kind={kind}", (loss[good], dl[good]), ref, kind, red)
            else:
                assert torch.isnan(loss).all(), f"{mode} kind={kind} {red}: the scalar hides a bad label"
                eg = _rel_err(dl[good], ref[1] / (ref[2] if red == "mean" else 1.0))
                print(f"bad labels {mode} kind={kind} {red}: good rows' grad err {eg:.2e} (bound {TOL:.0e})")
                assert eg <= TOL
            m = meter.cpu()
            assert float(m[1]) == correct and float(m[2]) == B
            assert _intact(big_x, PAD_ROWS * K) and _intact(big_w, PAD_ROWS)
            assert torch.equal(xd.cpu(), x) and torch.equal(wd.cpu(), w)
