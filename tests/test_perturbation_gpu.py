"""-m gpu: deletion / insertion curves and occlusion sensitivity (gaviko_amd.explain) against the oracle (plain torch on CPU) run on
volumes this file perturbs itself with torch indexing, against the reference fixtures of tools/gen_perturbation_golden.py, and the
structure the feature promises (bit-identities, replay, non-interference with a pending backward, errors)."""
import ast

import pytest
import torch

import oracle
from conftest import golden
from gaviko_amd import explain
from gaviko_amd.lib import GavikoHipError
from test_input_grad_gpu import METHODS, build, volumes

pytestmark = pytest.mark.gpu

STEPS = 4


def synthetic_relevance(B, N, seed=0):
    """Quantised random values (ties are frequent) with a block of exact zeros."""
    g = torch.Generator().manual_seed(100 + seed)
    r = torch.randint(0, 64, (B, N), generator=g).float() / 64
    r[:, : N // 8] = 0.0
    return r


def stable_rank(rel):
    order = torch.argsort(rel, dim=1, descending=True, stable=True)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(rel.shape[1]).expand_as(order))
    return rank


def upsample(mask, grid, patch):
    m = mask.view((mask.shape[0], 1) + tuple(grid))
    for ax, p in enumerate(patch):
        m = m.repeat_interleave(p, ax + 2)
    return m


def oracle_logits(method, m, cfg, vols, bf16=False):
    """Oracle logits (CPU) of a list of [B,1,D,H,W] volume batches, one forward over all of them -> list of [B, K] (float64)."""
    from oracle import vit_ref
    ocfg = {k: v for k, v in cfg.items() if k != "precision"}
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    old = vit_ref.BF16_OPERANDS
    vit_ref.BF16_OPERANDS = bf16
    try:
        with torch.no_grad():
            out = [oracle.FORWARD[method](sd, v.contiguous(), ocfg, None).double() for v in vols]
    finally:
        vit_ref.BF16_OPERANDS = old
    return out


def curve_volumes(x, rel, ks, fill, grid, patch):
    """The deletion and insertion volumes of every step, built with torch indexing -> (deletion list, insertion list)."""
    rank = stable_rank(rel)
    dele, ins = [], []
    for k in ks:
        top = upsample(rank < k, grid, patch)
        dele.append(torch.where(top, fill, x))
        ins.append(torch.where(top, x, fill))
    return dele, ins


def check_curve(res, ref_steps, tgt, tol_abs, ks, N, what):
    """step_logits within tol_abs; prob and auc within the same absolute bound (a logit error t moves a softmax probability by at most
    t / 2 to first order; the factor 2 covers the second-order term; auc is a convex combination of prob values)."""
    ref = torch.stack(ref_steps, 1)                                               # [B, P, K] float64
    got = res.step_logits.double().cpu()
    err = (got - ref).abs().max().item()
    idx = tgt.view(-1, 1, 1).expand(-1, ref.shape[1], 1)
    p_ref = torch.softmax(ref, 2).gather(2, idx)[..., 0]
    perr = (res.prob.double().cpu() - p_ref).abs().max().item()
    lerr = (res.logit.double().cpu() - ref.gather(2, idx)[..., 0]).abs().max().item()
    auc_ref = torch.trapezoid(p_ref, torch.tensor(ks, dtype=torch.float64) / N, dim=1)
    aerr = (res.auc.double().cpu() - auc_ref).abs().max().item()
    print(f"{what}: logits {err:.3e}  prob {perr:.3e}  auc {aerr:.3e}  (bound {tol_abs:.3e})")
    assert err <= tol_abs and lerr <= tol_abs, (what, err, lerr, tol_abs)
    assert perr <= tol_abs, (what, perr, tol_abs)
    assert aerr <= tol_abs, (what, aerr, tol_abs)


@pytest.mark.parametrize("method,extra", METHODS, ids=[m for m, _ in METHODS])
def test_curves_match_oracle_fp32_and_bf16(dev, method, extra):
    """fp32 path: within 1e-5 of the largest reference logit (test_fp32_path_vs_golden's bound).  bf16 path: within max(1e-2, 1.25 x
    floor) of it, the floor being the oracle's own BF16_OPERANDS error on the same perturbed volumes (the rule of tests/test_model_gpu.py)."""
    B = 2
    x, _ = volumes(B)
    m, cfg = build(method, dict(extra, precision="fp32"), dev)
    eng = m._engine()
    N, grid, patch = eng.N, tuple(eng.grid), tuple(eng.patch)
    rel = synthetic_relevance(B, N)
    ks = [(s * N) // STEPS for s in range(STEPS + 1)]
    fill = x.reshape(B, -1).amin(1).view(B, 1, 1, 1, 1).expand_as(x)
    dele, ins = curve_volumes(x, rel, ks, fill, grid, patch)
    # insertion at k is deletion's complement: ins[0] == dele[-1] and ins[-1] == dele[0] as volumes, so the oracle runs 8 batches, not 10
    uniq = dele + ins[1:-1]
    ref = oracle_logits(method, m, cfg, uniq)
    ref_d, ref_i = ref[:len(ks)], [ref[len(ks) - 1]] + ref[len(ks):] + [ref[0]]
    scale = max(r.abs().max().item() for r in ref)
    tgt = torch.tensor([1, 3])
    xd, reld = x.to(dev), rel.to(dev)
    for prec in ("fp32", "bf16"):
        if prec == "bf16":
            m.set_precision("bf16")
            low = oracle_logits(method, m, cfg, uniq, bf16=True)
            floor = max((a - b).abs().max().item() for a, b in zip(low, ref)) / scale
            tol = max(1e-2, 1.25 * floor) * scale
        else:
            tol = 1e-5 * scale
        d = explain.deletion_curve(m, xd, reld, tgt, steps=STEPS)
        i = explain.insertion_curve(m, xd, reld.view((B,) + grid), tgt.to(dev), steps=STEPS)
        assert d.ks.tolist() == ks and i.ks.tolist() == ks and d.ks.dtype == torch.int64
        assert tuple(d.step_logits.shape) == (B, STEPS + 1, eng.K) and tuple(d.prob.shape) == (B, STEPS + 1) and tuple(d.auc.shape) == (B,)
        check_curve(d, ref_d, tgt, tol, ks, N, f"{method} {prec} deletion")
        check_curve(i, ref_i, tgt, tol, ks, N, f"{method} {prec} insertion")
        assert (d.logits.double().cpu() - ref[0]).abs().max().item() <= tol


FIXTURES = ["gaviko_t16_b2", "linear_t16_b2", "evp_t16_b2"]


@pytest.mark.parametrize("name", FIXTURES)
def test_curves_and_occlusion_match_reference_fixture_fp32(dev, name):
    """The reference classes' own logits on perturbed volumes (built with numpy in the generator): fp32 path, 1e-5 of the largest logit."""
    from gaviko_amd.registry import build_model
    from gaviko_amd.utils import synth
    g = golden("perturb_" + name)
    cfg = dict(ast.literal_eval(str(g["meta/cfg"])), precision="fp32")
    B = int(g["meta/batch"])
    m = build_model(cfg)
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev).train()
    eng = m._engine()
    assert eng.fp32
    x = torch.from_numpy(synth.volumes(0, B)).to(dev)
    rel = torch.from_numpy(g["relevance"]).to(dev)
    ks = [int(k) for k in g["ks"]]
    tgt = torch.tensor([(2 + 2 * b) % eng.K for b in range(B)])
    scale = max(abs(g[k]).max() for k in ("logits", "deletion_min", "insertion_min", "deletion_vol", "insertion_vol", "occlusion_min"))
    tol = 1e-5 * float(scale)
    vol = torch.from_numpy(synth.volumes(100, 1)).to(dev)
    for tag, baseline in (("min", "min"), ("vol", vol)):
        for kind, fn in (("deletion", explain.deletion_curve), ("insertion", explain.insertion_curve)):
            res = fn(m, x, rel, tgt, ks=ks, baseline=baseline)
            ref = [torch.from_numpy(g[f"{kind}_{tag}"][:, s]).double() for s in range(len(ks))]
            check_curve(res, ref, tgt, tol, ks, eng.N, f"{name} {kind} {tag}")
            assert (res.logits.double().cpu() - torch.from_numpy(g["logits"]).double()).abs().max().item() <= tol
    occ = explain.occlusion_sensitivity(m, x, tgt, window=tuple(int(w) for w in g["meta/window"]))
    assert occ.boxes.tolist() == g["occlusion_boxes"].tolist()
    p0 = torch.softmax(torch.from_numpy(g["logits"]).double(), 1).gather(1, tgt.view(-1, 1))
    pw = torch.softmax(torch.from_numpy(g["occlusion_min"]).double(), 2).gather(2, tgt.view(-1, 1, 1).expand(-1, 8, 1))[..., 0]
    derr = (occ.drops.double().cpu() - (p0 - pw)).abs().max().item()
    print(f"{name} occlusion: drops {derr:.3e} (bound {tol:.3e})")
    assert derr <= tol                                                            # each probability moves by at most tol / 2 to first order


@pytest.mark.parametrize("method,extra", [METHODS[0], METHODS[1], METHODS[10]], ids=["gaviko", "linear", "evp"])
def test_occlusion_sensitivity_matches_oracle(dev, method, extra):
    assert method in ("gaviko", "linear", "evp")
    B = 2
    x, _ = volumes(B)
    m, cfg = build(method, dict(extra, precision="fp32"), dev)
    eng = m._engine()
    grid, patch = tuple(eng.grid), tuple(eng.patch)
    assert grid == (10, 10, 10)
    tgt = torch.tensor([0, 2])
    fill = x.reshape(B, -1).amin(1).view(B, 1, 1, 1, 1).expand_as(x)
    want_boxes = [[d, d + 5, h, h + 5, w, w + 5] for d in (0, 5) for h in (0, 5) for w in (0, 5)]
    vols = [x]
    for d0, d1, h0, h1, w0, w1 in want_boxes:
        mk = torch.zeros((B,) + grid, dtype=torch.bool)
        mk[:, d0:d1, h0:h1, w0:w1] = True
        vols.append(torch.where(upsample(mk, grid, patch), fill, x))
    ref = oracle_logits(method, m, cfg, vols)
    scale = max(r.abs().max().item() for r in ref)
    pr = [torch.softmax(r, 1).gather(1, tgt.view(-1, 1))[:, 0] for r in ref]
    want = torch.stack([pr[0] - p for p in pr[1:]], 1)                            # [B, 8]
    for prec in ("fp32", "bf16"):
        if prec == "bf16":
            m.set_precision("bf16")
            low = oracle_logits(method, m, cfg, vols, bf16=True)
            floor = max((a - b).abs().max().item() for a, b in zip(low, ref)) / scale
            tol = max(1e-2, 1.25 * floor) * scale
        else:
            tol = 1e-5 * scale
        occ = explain.occlusion_sensitivity(m, x.to(dev), tgt, window=(5, 5, 5))
        assert occ.boxes.tolist() == want_boxes and occ.boxes.dtype == torch.int64
        # the probability bound of check_curve: a logit error of at most tol moves a probability by at most tol / 2 to first order, so
        # a drop (the difference of two probabilities) lies within tol as well
        p_plain = torch.softmax(occ.logits.double().cpu(), 1).gather(1, tgt.view(-1, 1))[:, 0]
        perr = (p_plain - pr[0]).abs().max().item()
        derr = (occ.drops.double().cpu() - want).abs().max().item()
        print(f"{method} {prec} occlusion: plain probability {perr:.3e}, drops {derr:.3e} (bound {tol:.3e})")
        assert perr <= tol, (perr, tol)
        assert derr <= tol, (derr, tol)
        bmap = torch.zeros((B,) + grid)
        for w, (d0, d1, h0, h1, w0, w1) in enumerate(want_boxes):
            bmap[:, d0:d1, h0:h1, w0:w1] = occ.drops.cpu()[:, w].view(B, 1, 1, 1)
        assert torch.equal(occ.map.cpu(), bmap)                                   # disjoint windows: the drop broadcast over its box
    # overlapping along W, last window clipped: the map is the mean over the covering windows (fp32 round-off)
    occ = explain.occlusion_sensitivity(m, x.to(dev), tgt, window=(5, 5, 5), stride=(5, 5, 3))
    assert occ.boxes.shape == (16, 6) and occ.boxes[3].tolist() == [0, 5, 0, 5, 9, 10] and occ.boxes[1].tolist() == [0, 5, 0, 5, 3, 8]
    acc, cnt = torch.zeros((B,) + grid, dtype=torch.float64), torch.zeros(grid, dtype=torch.float64)
    for w, (d0, d1, h0, h1, w0, w1) in enumerate(occ.boxes.tolist()):
        acc[:, d0:d1, h0:h1, w0:w1] += occ.drops.double().cpu()[:, w].view(B, 1, 1, 1)
        cnt[d0:d1, h0:h1, w0:w1] += 1
    assert cnt.min() >= 1 and cnt.max() == 2
    assert (occ.map.double().cpu() - acc / cnt).abs().max().item() <= 1e-6


@pytest.mark.parametrize("method,extra", [METHODS[0], METHODS[10]], ids=["gaviko", "evp"])
def test_curve_structure_is_bit_exact(dev, method, extra):
    B = 2
    x, _ = volumes(B)
    m, cfg = build(method, extra, dev)
    eng = m._engine()
    N = eng.N
    xd = x.to(dev)
    rel = synthetic_relevance(B, N, 1).to(dev)
    tgt = torch.tensor([1, 3])
    fillv = -0.125
    plain = eng.eval_forward(xd).clone()
    blank = eng.eval_forward(torch.full_like(xd, fillv)).clone()
    # batch == B: every chunk holds one step of both samples, the batch eval_forward(img) ran
    d = explain.deletion_curve(m, xd, rel, tgt, ks=[0, 300, N], baseline=fillv, batch=B)
    i = explain.insertion_curve(m, xd, rel, tgt, ks=[0, 300, N], baseline=fillv, batch=B)
    assert torch.equal(d.logits, plain) and torch.equal(d.step_logits[:, 0], plain)
    assert torch.equal(d.step_logits[:, -1], blank) and torch.equal(i.step_logits[:, 0], blank)
    assert torch.equal(i.step_logits[:, -1], d.step_logits[:, 0])
    assert torch.equal(d.prob[:, 0], torch.softmax(plain, 1).gather(1, tgt.to(dev).view(-1, 1))[:, 0]) or \
        (d.prob[:, 0] - torch.softmax(plain, 1).gather(1, tgt.to(dev).view(-1, 1))[:, 0]).abs().max().item() < 1e-6
    # target=None: the argmax of the unperturbed logits, per sample
    dn = explain.deletion_curve(m, xd, rel, ks=[0, 300, N], baseline=fillv, batch=B)
    am = plain.argmax(1)
    assert torch.equal(dn.logit[:, 0], plain.gather(1, am.view(-1, 1))[:, 0]) and torch.equal(dn.step_logits, d.step_logits)
    # a chunked sweep (batch = 3, padded last chunk) against batch = 8, bit for bit per sample -- if the engine's forward is batch-size
    # (and batch-position) invariant for this config.  That premise is a property of the existing forward kernels and is checked with
    # plain eval_forward calls only: the same two volumes repeated to a batch of 3 and to a batch of 8.
    v3 = torch.cat([xd, xd[:1]])
    v8 = torch.cat([xd] * 4)
    l3, l8 = eng.eval_forward(v3).clone(), eng.eval_forward(v8).clone()
    invariant = all(torch.equal(l3[i], plain[i % B]) for i in range(3)) and all(torch.equal(l8[i], plain[i % B]) for i in range(8))
    if invariant:
        a = explain.deletion_curve(m, xd, rel, tgt, steps=STEPS, baseline=fillv, batch=3)
        b = explain.deletion_curve(m, xd, rel, tgt, steps=STEPS, baseline=fillv, batch=8)
        assert torch.equal(a.logits, b.logits) and torch.equal(a.step_logits, b.step_logits)
        assert torch.equal(a.prob, b.prob) and torch.equal(a.logit, b.logit) and torch.equal(a.auc, b.auc)
        print(f"{method}: eval_forward is batch-size invariant in bits (B = 2, 3, 8): chunk-size identity asserted")
    else:
        print(f"{method}: eval_forward of the same volumes at B = 2, 3 and 8 differs in bits (a property of the existing forward kernels): "
              "chunk-size identity not asserted")


def test_three_calls_eager_eager_replayed_are_bit_identical(dev):
    method, extra = METHODS[0]
    B = 2
    x, _ = volumes(B)
    m, cfg = build(method, extra, dev)
    xd = x.to(dev)
    rel = synthetic_relevance(B, m._engine().N, 2).to(dev)
    runs = [explain.deletion_curve(m, xd, rel, 1, steps=STEPS, batch=5) for _ in range(3)]
    occ = [explain.occlusion_sensitivity(m, xd, 1, window=(5, 5, 5), batch=5) for _ in range(2)]
    eng = m._engine()
    from gaviko_amd import engine as E
    if E.USE_GRAPHS:
        assert any(k[0] == "fwd" and k[1] == 5 for k in eng._graphs), "the chunk forward was never recorded into a launch plan"
    for r in runs[1:]:
        for a, b in zip(r, runs[0]):
            assert torch.equal(a, b)
    for a, b in zip(occ[1], occ[0]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("method,extra", [METHODS[0], METHODS[2]], ids=["gaviko", "fft"])
def test_call_between_forward_and_backward_leaves_gradients_bit_identical(dev, method, extra):
    B = 2
    x, y = volumes(B)
    m, cfg = build(method, extra, dev)
    xd, yd = x.to(dev), y.to(dev)
    rel = synthetic_relevance(B, m._engine().N, 3).to(dev)

    def step(between):
        for p in m.parameters():
            p.grad = None
        loss = torch.nn.functional.cross_entropy(m(xd), yd)
        if between:
            explain.deletion_curve(m, xd, rel, steps=2, batch=B)
            explain.occlusion_sensitivity(m, xd, window=(5, 5, 5), batch=B)
        loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    ref = [step(False) for _ in range(3)][-1]
    for _ in range(3):
        got = step(True)
        assert got.keys() == ref.keys() and len(ref) > 0
        for n in ref:
            assert torch.equal(got[n], ref[n]), n


def test_documented_errors(dev):
    B = 2
    x, _ = volumes(B)
    m, cfg = build("linear", {}, dev)
    N = m._engine().N
    xd = x.to(dev)
    rel = synthetic_relevance(B, N).to(dev)
    E = GavikoHipError
    with pytest.raises(E):
        explain.deletion_curve(m, x, rel)                                         # CPU volume
    with pytest.raises(E):
        explain.deletion_curve(m, xd, rel.cpu())                                  # CPU relevance
    with pytest.raises(E):
        explain.deletion_curve(m, xd[:, :, :60], rel)                             # wrong geometry
    with pytest.raises(E, match="patch_grid"):
        explain.deletion_curve(m, xd, torch.zeros((B, m._engine().T), device=dev))   # a token-level map
    bad = rel.clone()
    bad[1, 5] = float("nan")
    with pytest.raises(E, match="NaN"):
        explain.insertion_curve(m, xd, bad)
    with pytest.raises(E, match="NaN"):
        explain.patch_ranks(m, bad)
    for ks in ([0, N + 1], [-1, 5], [5, 5], [7, 3], []):
        with pytest.raises(E):
            explain.deletion_curve(m, xd, rel, ks=ks)
    for batch in (0, -2, 1.5, True):
        with pytest.raises(E):
            explain.deletion_curve(m, xd, rel, batch=batch)
    with pytest.raises(E):
        explain.deletion_curve(m, xd, rel, steps=0)
    with pytest.raises(E):
        explain.deletion_curve(m, xd, rel, target=7)
    with pytest.raises(E):
        explain.deletion_curve(m, xd, rel, baseline="mean")
    with pytest.raises(E):
        explain.deletion_curve(m, xd, rel, baseline=torch.zeros((3, 1, 120, 160, 160), device=dev))
    with pytest.raises(E):
        explain.deletion_curve(m, xd, rel, baseline=torch.zeros((1, 1, 120, 160, 160)))
    with pytest.raises(E):
        explain.occlusion_sensitivity(m, xd, window=(2, 2, 2), stride=(3, 2, 2))  # a gap between windows
    with pytest.raises(E):
        explain.occlusion_sensitivity(m, xd, window=(0, 2, 2))
    with pytest.raises(E):
        explain.occlusion_sensitivity(m, xd, window=(2, 2))
    ranks = explain.patch_ranks(m, rel.view(B, 10, 10, 10))
    assert ranks.dtype == torch.int32 and torch.equal(ranks.cpu().long(), stable_rank(rel.cpu()))
