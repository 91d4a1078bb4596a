"""-m gpu: Monte-Carlo dropout and flip test-time augmentation (gaviko_amd.uncertainty) against the reference fixtures of
tools/gen_uncertainty_golden.py, against direct model calls on batches assembled with torch.flip (bit for bit), against the oracle run
with exactly the dropout masks the kernels drew (tests/dropmask.py), and the structure the feature promises: reproducibility from the
seed, non-interference with module flags, gradients and a pending backward, errors."""
import ast

import numpy as np
import pytest
import torch

import dropmask
import oracle
from conftest import golden
from gaviko_amd import uncertainty
from gaviko_amd.lib import GavikoHipError
from test_input_grad_gpu import GAVIKO, METHODS, build, volumes
from test_model_dropout_gpu import build as build_dropout
from test_model_dropout_gpu import masks_for
from test_perturbation_gpu import oracle_logits
from test_uncertainty_golden import stats64

pytestmark = pytest.mark.gpu

FLOATS = ("probs", "entropy", "expected_entropy", "mutual_info", "std", "variation_ratio")
CODES = list(range(8))


def flipped(x, code):
    dims = [a + 2 for a in range(3) if code >> a & 1]
    return torch.flip(x, dims).contiguous() if dims else x


def check_stats(res, ref_logits, tol_abs, what):
    """The statistics against their float64 restatement on the reference member logits [B, S, K], within the absolute bound of the logits
    (the argument of test_perturbation_gpu.check_curve: a logit error t moves a softmax probability by at most t / 2 to first order)."""
    want = stats64(ref_logits)
    errs = {k: float(np.abs(getattr(res, k).double().cpu().numpy() - want[k]).max()) for k in FLOATS if k != "variation_ratio"}
    print(f"{what}: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"  (bound {tol_abs:.3e})")
    for k, v in errs.items():
        assert v <= tol_abs, (what, k, v, tol_abs)


def flags(m):
    return [(n, mod.training) for n, mod in m.named_modules()]


# ------------------------------------------------------------------ tta
@pytest.mark.parametrize("method", ["gaviko", "linear", "evp"])
def test_tta_matches_reference_fixture_fp32_and_bf16(dev, method):
    """fp32 path: within 1e-5 of the largest reference logit.  bf16 path: within max(1e-2, 1.25 x floor) of it, the floor being the oracle's
    own BF16_OPERANDS error on the same flipped volumes (the rule of tests/test_model_gpu.py and tests/test_perturbation_gpu.py).  probs
    and the entropies within the same absolute bound."""
    from gaviko_amd.registry import build_model
    from gaviko_amd.utils import synth
    g = golden(f"uncertainty_tta_{method}_t16")
    cfg = dict(ast.literal_eval(str(g["meta/cfg"])), precision="fp32")
    B = int(g["meta/batch"])
    m = build_model(cfg)
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev).train()
    x = torch.from_numpy(synth.volumes(0, B))
    ref = g["logits"].astype(np.float64)                                          # [B, 8, K]
    scale = float(np.abs(ref).max())
    for prec in ("fp32", "bf16"):
        if prec == "bf16":
            m.set_precision("bf16")
            vols = [flipped(x, c) for c in CODES]
            hi = oracle_logits(method, m, cfg, vols)
            low = oracle_logits(method, m, cfg, vols, bf16=True)
            floor = max((a - b).abs().max().item() for a, b in zip(low, hi)) / scale
            tol = max(1e-2, 1.25 * floor) * scale
        else:
            assert m._engine().fp32
            tol = 1e-5 * scale
        res = uncertainty.tta(m, x.to(dev), flips="all")
        assert res.epochs == [] and tuple(res.member_logits.shape) == ref.shape and res.member_logits.dtype == torch.float32
        err = float(np.abs(res.member_logits.double().cpu().numpy() - ref).max())
        print(f"{method} {prec} tta: member logits {err:.3e} (bound {tol:.3e})")
        assert err <= tol, (method, prec, err, tol)
        check_stats(res, ref, tol, f"{method} {prec} tta")
        top2 = np.sort(ref, axis=2)[:, :, -2:]
        if prec == "fp32" and (top2[:, :, 1] - top2[:, :, 0]).min() > 2 * tol:    # every member's own decision is clear of the bound: votes exact
            assert np.array_equal(res.votes.cpu().numpy(), g["stats/votes"])


@pytest.mark.parametrize("method,extra", METHODS, ids=[m for m, _ in METHODS])
def test_tta_members_are_bit_identical_to_direct_eval_calls(dev, method, extra):
    """The same rows in the same order at the same batch size: chunk c of tta(flips='all', batch=8) is the 8 flips of volume c."""
    B = 2
    x, _ = volumes(B)
    m, cfg = build(method, extra, dev)
    xd = x.to(dev)
    before = flags(m)
    res = uncertainty.tta(m, xd, flips="all", batch=8)
    assert flags(m) == before
    sub = uncertainty.tta(m, xd, flips=[(), (0,), (2, 1)], batch=6)
    train = uncertainty.tta(m, xd, flips="train", batch=4)
    m.eval()
    with torch.no_grad():
        for b in range(B):
            direct = m(torch.cat([flipped(xd[b:b + 1], c) for c in CODES])).clone()
            assert torch.equal(res.member_logits[b], direct), (method, b)
        d6 = m(torch.cat([flipped(xd[b:b + 1], c) for b in range(B) for c in (0, 1, 6)])).clone()
        d4 = m(torch.cat([flipped(xd[b:b + 1], c) for b in range(B) for c in (0, 1)])).clone()
    assert torch.equal(sub.member_logits.view(6, -1), d6) and torch.equal(train.member_logits.view(4, -1), d4)
    m.train()
    st = stats64(res.member_logits.cpu().numpy())
    assert np.array_equal(res.votes.cpu().numpy(), st["votes"]) and np.abs(res.probs.double().cpu().numpy() - st["probs"]).max() <= 2e-6


# ------------------------------------------------------------------ mc_dropout
def gaviko_masks(eng, word, B, p):
    t = lambda a: torch.from_numpy(a)  # noqa: E731
    masks = {}
    for i in range(eng.depth):
        masks[("mwsa_attn", i)] = t(dropmask.window_attn_mask(2 * i + word, B, eng.N, p))
        masks[("mwsa_proj", i)] = t(dropmask.rows_mask(2 * i + 1 + word, B * eng.N, eng.C, p)).view(B, eng.N, eng.C)
    return masks


MC_CASES = [("gaviko", dict(GAVIKO, attn_drop=0.2, proj_drop=0.2, dropout=0.0, emb_dropout=0.0)),
            ("linear", dict(dropout=0.1, emb_dropout=0.1))]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("method,extra", MC_CASES, ids=[m for m, _ in MC_CASES])
def test_mc_dropout_matches_oracle_with_the_kernels_masks(dev, method, extra, prec):
    """B = 2, S = 4, batch = 8: one chunk.  The masks of the 8-row batch are rebuilt from result.epochs[0] (tests/dropmask.py, as
    tests/test_model_dropout_gpu.py does) and the oracle runs on the replicated batch with them.  Member logits within 1.5e-2 max|ref|
    (bf16) / 2e-5 max(1, max|ref|) (fp32): the bounds of the existing live-dropout tests."""
    B, S = 2, 4
    m, cfg = build_dropout(method, dict(extra, precision=prec), dev)
    x, _ = volumes(B)
    eng = m._engine()
    assert eng.fp32 == (prec == "fp32")
    res = uncertainty.mc_dropout(m, x.to(dev), samples=S, batch=8, seed=20261017)
    assert res.epochs == [20261017 + 7919] and tuple(res.member_logits.shape) == (B, S, eng.K)
    word = res.epochs[0]
    rep = x.repeat_interleave(S, 0)                                               # row o = b * S + s
    if method == "gaviko":
        masks = gaviko_masks(eng, word, B * S, 0.2)
    else:
        masks = masks_for(eng, word, B * S, 0.1, 0.1, 0.0)
    ocfg = {k: v for k, v in cfg.items() if k != "precision"}
    osd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = oracle.FORWARD[method](osd, rep, dict(ocfg, _masks=masks), None).double()
        plain = oracle.FORWARD[method](osd, rep, ocfg, None).double()
    scale = ref.abs().max().item()
    tol = 1.5e-2 * scale if prec == "bf16" else 2e-5 * max(1.0, scale)
    got = res.member_logits.double().cpu().view(B * S, -1)
    err = (got - ref).abs().max().item()
    away = (got - plain).abs().max().item()
    print(f"{method} {prec} mc_dropout: member logits {err:.3e} (bound {tol:.3e}); away from the plain eval logits {away:.3e}")
    assert err <= tol, (method, prec, err, tol)
    assert away > 3 * err                                                         # the masks matter
    ml = res.member_logits
    for b in range(B):
        for s in range(1, S):
            assert not torch.equal(ml[b, s], ml[b, 0])                            # members of one volume differ from each other
    check_stats(res, ref.view(B, S, -1).numpy(), tol, f"{method} {prec} mc_dropout")
    assert (res.votes.sum(1) == S).all() and float(res.mutual_info.min()) >= 0.0


def test_mc_dropout_is_reproducible_from_the_seed(dev):
    B, S = 2, 4
    x, _ = volumes(B)
    m, cfg = build("gaviko", dict(GAVIKO, attn_drop=0.2, proj_drop=0.2), dev)
    xd = x.to(dev)
    a = uncertainty.mc_dropout(m, xd, samples=S, seed=7)
    b = uncertainty.mc_dropout(m, xd, samples=S, seed=7)
    assert torch.equal(a.member_logits, b.member_logits) and a.epochs == b.epochs == [7 + 7919]
    for u, v in zip(a[:8], b[:8]):
        assert torch.equal(u, v)
    c = uncertainty.mc_dropout(m, xd, samples=S, seed=8)
    assert not torch.equal(a.member_logits, c.member_logits) and c.epochs == [8 + 7919]
    d = uncertainty.mc_dropout(m, xd, samples=S)
    e = uncertainty.mc_dropout(m, xd, samples=S)
    assert not torch.equal(d.member_logits, e.member_logits)
    assert d.epochs == [c.epochs[0] + 7919] and e.epochs == [d.epochs[0] + 7919]  # seed=None continues from wherever the word stands
    # a multi-chunk sweep: the word advances by 7919 per chunk, and the same seed gives the same bits again (eager, recorded, replayed)
    runs = [uncertainty.mc_dropout(m, xd, samples=S, batch=4, seed=1000) for _ in range(3)]
    assert runs[0].epochs == [1000 + 7919, 1000 + 2 * 7919]
    for r in runs[1:]:
        assert r.epochs == runs[0].epochs and torch.equal(r.member_logits, runs[0].member_logits)
    # drop= overrides the rates; a padded last chunk (6 rows in chunks of 4) keeps every real row
    o = uncertainty.mc_dropout(m, xd, samples=3, batch=4, seed=5, drop={"attn_drop": 0.0, "proj_drop": 0.5})
    assert tuple(o.member_logits.shape) == (B, 3, m._engine().K) and len(o.epochs) == 2 and bool(torch.isfinite(o.member_logits).all())
    assert not torch.equal(o.member_logits[1, 0], o.member_logits[1, 2])


@pytest.mark.parametrize("method,extra", [("gaviko", dict(GAVIKO, attn_drop=0.2, proj_drop=0.2)), ("fft", dict(dropout=0.1, emb_dropout=0.1))],
                         ids=["gaviko", "fft"])
def test_calls_leave_flags_gradients_and_a_pending_backward_alone(dev, method, extra):
    B = 2
    x, y = volumes(B)
    if method == "fft":
        m, cfg = build_dropout(method, extra, dev)
    else:
        m, cfg = build(method, extra, dev)
    xd, yd = x.to(dev), y.to(dev)

    def both():
        uncertainty.mc_dropout(m, xd, samples=2, batch=4, seed=3)
        uncertainty.tta(m, xd, flips="train", batch=4)

    # module flags, from train mode and from eval mode
    before = flags(m)
    both()
    assert flags(m) == before and any(f for _, f in before)
    m.eval()
    ev = flags(m)
    with torch.no_grad():
        plain = m(xd).clone()
    both()
    assert flags(m) == ev
    with torch.no_grad():
        assert torch.equal(m(xd), plain)                                          # eval bits the same before and after
    assert uncertainty.training_drop_config(m) == uncertainty.training_drop_config(m) and flags(m) == ev
    m.train()
    assert flags(m) == before

    # a call between a training forward and its backward: every gradient bit-identical to the same step without the call.  The training
    # forward draws its own masks from the training workspace's word, so both variants start from the same word.
    eng = m._engine()

    def step(between):
        for p in m.parameters():
            p.grad = None
        eng.workspace(B, xd.device, True)["seed"].fill_(4242)
        loss = torch.nn.functional.cross_entropy(m(xd), yd)
        if between:
            both()
        loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    ref = [step(False) for _ in range(3)][-1]
    for _ in range(3):
        got = step(True)
        assert got.keys() == ref.keys() and len(ref) > 0
        for n in ref:
            assert torch.equal(got[n], ref[n]), n
    # .grad (and with it the flat gradient buffer its tensors are views of) untouched by calls outside a step
    flat = eng._flat_grad["buf"].clone() if eng._flat_grad is not None else None
    held = {n: (p.grad, p.grad.clone()) for n, p in m.named_parameters() if p.grad is not None}
    both()
    for n, p in m.named_parameters():
        if n in held:
            assert p.grad is held[n][0] and torch.equal(p.grad, held[n][1]), n
        else:
            assert p.grad is None, n
    if flat is not None:
        assert torch.equal(eng._flat_grad["buf"], flat)


def test_documented_errors(dev):
    B = 2
    x, _ = volumes(B)
    xd = x.to(dev)
    E = GavikoHipError
    frozen, _ = build("gaviko", dict(GAVIKO), dev)                                # attn_drop = proj_drop = 0, frozen backbone: nothing is live
    with pytest.raises(E, match="identical"):
        uncertainty.mc_dropout(frozen, xd, samples=4)
    with pytest.raises(E, match="identical"):
        uncertainty.mc_dropout(frozen, xd, samples=4, drop={"attn_drop": 0.0})
    m, _ = build("gaviko", dict(GAVIKO, attn_drop=0.2, proj_drop=0.2), dev)
    for samples in (0, -1, 2.0, True):
        with pytest.raises(E):
            uncertainty.mc_dropout(m, xd, samples=samples)
    for batch in (0, -2, 1.5, True):
        with pytest.raises(E):
            uncertainty.mc_dropout(m, xd, samples=2, batch=batch)
        with pytest.raises(E):
            uncertainty.tta(m, xd, batch=batch)
    with pytest.raises(E):
        uncertainty.mc_dropout(m, x, samples=2)                                   # CPU tensor
    with pytest.raises(E):
        uncertainty.tta(m, x)
    with pytest.raises(E):
        uncertainty.mc_dropout(m, xd[:, :, :60], samples=2)                       # wrong shape
    with pytest.raises(E):
        uncertainty.tta(m, xd[0])
    with pytest.raises(E):
        uncertainty.tta(m, xd.double())                                           # wrong dtype
    with pytest.raises(E):
        uncertainty.mc_dropout(m, xd, samples=2, seed=-1)
    with pytest.raises(E):
        uncertainty.mc_dropout(m, xd, samples=2, drop={"no_such_dropout": 0.1})
    with pytest.raises(E):
        uncertainty.mc_dropout(m, xd, samples=2, drop={"attn_drop": 1.0})
    for flips in ([(3,)], [(0, 0)], [(-1,)], "both", [], [(0.0,)], 5):
        with pytest.raises(E):
            uncertainty.tta(m, xd, flips=flips)
    before = flags(m)
    r = uncertainty.tta(m, xd, flips=[()])                                        # S = 1: the volume itself, no spread
    assert float(r.mutual_info.abs().max()) == 0.0 and float(r.std.abs().max()) == 0.0 and flags(m) == before
