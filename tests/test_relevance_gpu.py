"""-m gpu: class-specific attention relevance, gradient x attention (gaviko_amd/explain.py, csrc/attention_map.hip).

  * the gradient column-sum kernel against float64 torch on the exact bf16 operands;
  * the relevance step kernel;
  * the engine's relevance and gradient maps against float64 ones rebuilt from the engine's own qkv / lse / per-layer dctx (kernel
    error alone);
  * relevance and gradient maps against the reference's (tests/golden/relv_*.npz, tools/gen_relevance_golden.py), on the part added to
    w_pool: a comparison on r itself would pass with the kernels returning zeros;
  * dead-row pruning changes no bit; an explanation between a training forward and its backward changes nothing of that step or the
    next and creates no .grad."""
import os

import pytest
import torch

from conftest import golden
from test_attention_maps_gpu import _build, _input, _operands, _probs, _rel, _weights, LOG2E

pytestmark = pytest.mark.gpu

REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The measured errors of this module, written to $GAVIKO_RELEVANCE_REPORT when that names a file (also printed: run with -s)."""
    yield
    out = os.environ.get("GAVIKO_RELEVANCE_REPORT")
    if REPORT and out:
        with open(out, "w") as f:
            f.write("\n".join(REPORT) + "\n")


def _dctx(B, T, H, amp, seed, dev):
    """bf16 dO [pad(B*T), H*64] and the float64 values it represents as [B, H, T, 64]."""
    from gaviko_amd import ops
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand((B, T, H * 64), generator=g) * 2 - 1) * amp).bfloat16()
    D = ops.act_zeros(B * T, H * 64, torch.bfloat16, dev)
    D[: B * T] = x.reshape(B * T, -1).to(dev)
    return D, x.to(dev).double().reshape(B, T, H, 64).transpose(1, 2)


def _values(Q, B, T, H):
    inner = H * 64
    return Q[: B * T].view(B, T, -1)[..., 2 * inner:].double().reshape(B, T, H, 64).transpose(1, 2)


@pytest.mark.parametrize("damp", [1e-3, 1.0])
@pytest.mark.parametrize("T", [1, 31, 65, 129, 257, 1033])
@pytest.mark.parametrize("H", [1, 3, 12])
@pytest.mark.parametrize("B", [1, 4])
def test_gradcolsum_kernel(dev, B, H, T, damp):
    """Bound: the column-sum test's relative term 1e-4 applied to max over (b, h, j) of sum_i |w_i| P |dP| -- the un-rectified magnitude,
    which bounds the accumulated terms; no absolute term."""
    from gaviko_amd import ops
    Q, s2 = _operands(B, T, H, 2.5, 3000 + 7 * T + H + B, dev)
    D, dO = _dctx(B, T, H, damp, 5000 + 3 * T + H + B, dev)
    P, lse = _probs(s2)
    dP = dO @ _values(Q, B, T, H).transpose(-1, -2)
    lse32 = lse.float().contiguous()
    n = B * H * T
    worst = 0.0
    for kind in ("onehot", "range", "dense"):
        w, wref, q0, q1 = _weights(kind, B, T, dev, T + H)
        buf = torch.full((n + 4096,), float("nan"), device=dev)
        out = buf[:n]
        ops.attention_gradcolsum(Q, lse32, D, w, out, B, T, H, q0=q0, q1=q1)
        torch.cuda.synchronize()
        ref = torch.einsum("bi,bhij->bhj", wref, P * dP.clamp_min(0.0))
        mag = torch.einsum("bi,bhij->bhj", wref.abs(), P * dP.abs()).max().item()
        err = (out.view(B, H, T).double() - ref).abs().max().item()
        bound = 1e-4 * mag
        worst = max(worst, err / max(mag, 1e-300))
        print(f"gradcolsum B={B} H={H} T={T} damp={damp:g} {kind}: err {err:.3e} bound {bound:.3e} (ratio to magnitude {err / max(mag, 1e-300):.3e})")
        assert err < bound, f"{kind}: err {err:.3e} bound {bound:.3e}"
        assert torch.isnan(buf[n:]).all()                                   # nothing written past j < T of the last (b, h)
        again = torch.empty_like(out)
        ops.attention_gradcolsum(Q, lse32, D, w, again, B, T, H, q0=q0, q1=q1)
        assert torch.equal(again, out)                                       # no atomics: bit-identical
    if (B, H, T) == (4, 12, 1033):
        REPORT.append(f"gradcolsum kernel B=4 H=12 T=1033 dO amplitude {damp:g}: worst err / magnitude {worst:.3e} (bound 1e-4)")


@pytest.mark.parametrize("B,T,H", [(1, 1, 1), (4, 1033, 12), (2, 1001, 3), (2, 257, 16)])
def test_relevance_step_kernel(dev, B, T, H):
    from gaviko_amd import ops
    g = torch.Generator().manual_seed(T * H + 1)
    r = torch.rand((B, T), generator=g).to(dev)
    cs = torch.rand((B, H, T), generator=g).to(dev)
    out = torch.empty_like(r)
    ops.relevance_step(r, cs, out, B, T, H)
    ref = r.double() + cs.double().mean(dim=1)
    assert (out.double() - ref).abs().max().item() < 1e-6 * max(1.0, ref.abs().max().item())
    again = r.clone()
    ops.relevance_step(again, cs, again, B, T, H)                            # in place
    assert torch.equal(again, out)


# ------------------------------------------------------------------------------------------------ whole model
def _w_pool(eng, B, dev):
    from gaviko_amd import explain
    r0, R = explain._pool_range(eng, eng.depth - 1)
    w = torch.zeros((B, eng.T), dtype=torch.float64, device=dev)
    w[:, r0:r0 + R] = 1.0 / R
    return w


def _targets(z, tag, dev):
    return torch.from_numpy(z[f"meta/target_{tag}"]).to(dev)


@pytest.mark.parametrize("case", ["gaviko_t16_b2", "cfg1_linear_t16_b1"])
def test_against_engine_buffers(dev, case):
    """Rebuild every P and dP in float64 from the engine's own qkv, lse and per-layer dctx (keep_dctx), propagate in torch: the kernels'
    own error."""
    from gaviko_amd import explain
    z = golden("relv_" + case)
    model, x = _build(z, dev), _input(z, dev)
    tgt = _targets(z, "argmax", dev)
    _, rel = explain.attention_relevance(model, x, target=tgt)
    _, maps = explain.attention_gradmaps(model, x, target=tgt)
    eng = model._engine()
    seed = lambda logits: torch.nn.functional.one_hot(tgt, eng.K).to(logits.dtype)
    _, ws, rv = eng.relevance_backward(x, seed, mode="relevance", keep_dctx=True)
    assert torch.equal(rv["r"], rel)                                          # the debug switch changes no bit of the result
    B, H, T, inner = x.shape[0], eng.heads, eng.T, eng.heads * 64
    w = _w_pool(eng, B, dev)
    r = w.clone()
    worst = 0.0
    for l in range(eng.depth - 1, -1, -1):
        e = ws["qkv"][l][: B * T].view(B, T, -1).double()
        q, k, v = (e[..., j * inner: (j + 1) * inner].reshape(B, T, H, 64).transpose(1, 2) for j in range(3))
        dO = rv["keep"][l][: B * T].view(B, T, H, 64).double().transpose(1, 2)
        P = torch.exp2(q @ k.transpose(-1, -2) - ws["lse"][l].view(B, H, T).double()[..., None] * LOG2E)
        G = P * (dO @ v.transpose(-1, -2)).clamp_min(0.0)
        worst = max(worst, _rel(maps[l], torch.einsum("bi,bhij->bhj", w, G)))
        r = r + torch.einsum("bi,bij->bj", r, G.mean(dim=1))
        del P, G
    err = _rel(rel.double() - w, r - w)
    REPORT.append(f"engine-buffer cross-check {case}: relevance (r - w_pool) rel {err:.3e}, gradient maps rel (worst layer) {worst:.3e}; "
                  f"largest added value {float((r - w).max()):.3e}")
    print(REPORT[-1])
    assert err < 1e-4
    assert worst < 1e-4


FIXTURES = ["gaviko_t16_b2", "cfg1_linear_t16_b1", "dvpt_t16_b2_mean_p8", "cfg2_gaviko_b16_b4"]


@pytest.mark.parametrize("case", FIXTURES)
def test_against_reference_fixtures(dev, case):
    """Bound: max(2e-2, 3 x max(floor/operand, floor/weights)) per quantity, the floors measured on the reference alone."""
    from gaviko_amd import explain
    z = golden("relv_" + case)
    model, x = _build(z, dev), _input(z, dev)
    eng = model._engine()
    w = _w_pool(eng, x.shape[0], dev)
    errs, bounds = {}, {}

    def bound(key):
        return max(2e-2, 3 * max(float(z[f"floor/operand/{key}"]), float(z[f"floor/weights/{key}"])))

    for tag in ("argmax", "alt"):
        logits, rel = explain.attention_relevance(model, x, target=_targets(z, tag, dev))
        key = f"relevance/{tag}"
        ref = torch.from_numpy(z[key]).to(dev).double() - w
        errs[key], bounds[key] = _rel(rel.double() - w, ref), bound(key)
        assert (rel.double() >= w - 1e-7).all()
    _, maps = explain.attention_gradmaps(model, x, target=_targets(z, "argmax", dev))
    for i in (0, eng.depth - 1):
        key = f"gradmaps/argmax/layer{i}"
        errs[key], bounds[key] = _rel(maps[i], z[key]), bound(key)
    for m in maps:
        assert m.min().item() >= 0.0
    REPORT.append(f"reference {case}: " + ", ".join(f"{k} {errs[k]:.3e} (bound {bounds[k]:.3e})" for k in sorted(errs))
                  + f"; logits rel {_rel(logits, z['logits']):.2e}")
    print(REPORT[-1])
    for k in errs:
        assert errs[k] < bounds[k], REPORT[-1]


def test_pruning_changes_no_bit(dev):
    from gaviko_amd import explain
    z = golden("relv_gaviko_t16_b2")
    model, x = _build(z, dev), _input(z, dev)
    eng = model._engine()
    assert eng.prune_dead_rows                                                # the default of a frozen GAViKO
    l0, r0 = explain.attention_relevance(model, x)
    _, m0 = explain.attention_gradmaps(model, x)
    eng.set_prune(False)
    l1, r1 = explain.attention_relevance(model, x)
    _, m1 = explain.attention_gradmaps(model, x)
    assert torch.equal(l0, l1) and torch.equal(r0, r1)
    for a, b in zip(m0, m1):
        assert torch.equal(a, b)
    w = _w_pool(eng, x.shape[0], dev)
    assert float((r0.double() - w).max()) > 0.0


def test_rows_int_and_other_methods(dev):
    """rows=int is attention_maps' form; deep VPT gets per-layer maps (no propagated relevance); an unfrozen backbone works."""
    from gaviko_amd import explain
    from gaviko_amd.lib import GavikoHipError
    z = golden("relv_gaviko_t16_b2")
    model, x = _build(z, dev), _input(z, dev)
    eng = model._engine()
    _, one = explain.attention_gradmaps(model, x, rows=eng.P)                # the CLS row
    _, pool = explain.attention_gradmaps(model, x)
    assert one[0].shape == pool[0].shape and one[0].min().item() >= 0.0 and one[0].max().item() > 0.0
    assert not torch.equal(one[0], pool[0])
    zd = golden("attn_deep_vpt_t16_b2")
    deep, xd = _build(zd, dev), _input(zd, dev)
    with pytest.raises(GavikoHipError, match="deep VPT"):
        explain.attention_relevance(deep, xd)
    _, dm = explain.attention_gradmaps(deep, xd)
    Ts = deep._engine().Ts
    assert [tuple(m.shape[1:]) for m in dm] == [(deep._engine().heads, t) for t in Ts]
    assert all(m.max().item() > 0.0 and torch.isfinite(m).all() for m in dm)
    zu = golden("adaptformer_t16_b2_unfrozen")
    un, xu = _build(zu, dev), _input(zu, dev)
    _, ru = explain.attention_relevance(un, xu, target=1)
    wu = _w_pool(un._engine(), xu.shape[0], dev)
    assert (ru.double() >= wu - 1e-7).all() and float((ru.double() - wu).max()) > 0.0
    assert all(p.grad is None for p in un.parameters())


def test_logits_and_patch_grid(dev):
    from gaviko_amd import explain
    z = golden("relv_gaviko_t16_b2")
    model, x = _build(z, dev), _input(z, dev)
    with torch.no_grad():
        ref = model(x)
    logits, rel = explain.attention_relevance(model, x)
    assert not logits.requires_grad and logits.grad_fn is None
    assert _rel(logits, ref) <= 1e-5
    logits2, _ = explain.attention_gradmaps(model, x)
    assert not logits2.requires_grad and logits2.grad_fn is None
    assert _rel(logits2, ref) <= 1e-5
    assert explain.patch_grid(model, rel).shape == (x.shape[0],) + tuple(model._engine().grid)


def test_between_forward_and_backward(dev):
    """Two identical models run the same two SGD steps; the second calls attention_relevance and attention_gradmaps between its first
    forward and backward."""
    from gaviko_amd import explain
    z = golden("relv_gaviko_t16_b2")
    x = _input(z, dev)
    y = torch.tensor([1, 3], device=dev)
    runs = []
    for explain_between in (False, True):
        model = _build(z, dev, train=True)
        params = [p for p in model.parameters() if p.requires_grad]
        if explain_between:                                                  # the explanation calls alone create no .grad
            explain.attention_relevance(model, x)
            explain.attention_gradmaps(model, x)
            assert all(p.grad is None for p in model.parameters())
        opt = torch.optim.SGD(params, lr=0.1)
        steps = []
        for step in range(2):
            opt.zero_grad(set_to_none=True)
            logits = model(x)
            if explain_between and step == 0:
                explain.attention_relevance(model, x)
                explain.attention_gradmaps(model, x, target=2)
                assert all(p.grad is None for p in model.parameters())
            torch.nn.functional.cross_entropy(logits, y).backward()
            steps.append((logits.detach().clone(), [p.grad.detach().clone() for p in params]))
            if explain_between and step == 1:                                # nor do they change one that exists
                explain.attention_relevance(model, x, target=0)
                for p, g in zip(params, steps[-1][1]):
                    assert torch.equal(p.grad, g)
            opt.step()
        runs.append(steps)
    for step in range(2):
        (la, ga), (lb, gb) = runs[0][step], runs[1][step]
        assert torch.equal(la, lb), f"step {step}: logits differ"
        for a, b in zip(ga, gb):
            assert torch.equal(a, b), f"step {step}: gradients differ"
