"""-m gpu: attention maps and attention rollout (gaviko_amd/explain.py, csrc/attention_map.hip).

  * the column-sum kernel against float64 torch on the exact bf16 operands, and with the forward's own lse;
  * the rollout step kernel;
  * the engine's rollout against a float64 rollout rebuilt from the engine's own saved qkv / lse (kernel error alone);
  * maps and rollout against the reference's (tests/golden/attn_*.npz, tools/gen_attention_golden.py);
  * an explanation between a training forward and its backward changes nothing of that step or the next."""
import ast
import math
import os

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
ATTN_C = 0.125 * LOG2E
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The measured errors of this module, written to $GAVIKO_ATTN_REPORT when that names a file (also printed: run with -s)."""
    yield
    out = os.environ.get("GAVIKO_ATTN_REPORT")
    if REPORT and out:
        with open(out, "w") as f:
            f.write("\n".join(REPORT) + "\n")


def _operands(B, T, H, amp, seed, dev):
    """bf16 qkv [pad(B*T), 3*H*64] with the q block pre-scaled by scale*log2(e) (one rounding, as the engine's qkv GEMM delivers it), and
    the float64 scores in log2 units those operands represent exactly."""
    from gaviko_amd import ops
    inner = H * 64
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((B, T, 3 * inner), generator=g) * 2 - 1) * amp
    x[..., :inner] *= ATTN_C
    op = x.bfloat16()
    Q = ops.act_zeros(B * T, 3 * inner, torch.bfloat16, dev)
    Q[: B * T] = op.reshape(B * T, -1).to(dev)
    e = op.to(dev).double()
    q = e[..., :inner].reshape(B, T, H, 64).transpose(1, 2)
    k = e[..., inner: 2 * inner].reshape(B, T, H, 64).transpose(1, 2)
    return Q, q @ k.transpose(-1, -2)                              # S' = q'.k  [B, H, T, T]


def _probs(s2):
    lse = torch.logsumexp(s2 * math.log(2.0), dim=-1)                # natural log, float64
    return torch.exp(s2 * math.log(2.0) - lse[..., None]), lse


def _weights(kind, B, T, dev, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.full((B, T), 7.0)                                        # rows outside [q0, q1) must not be read
    if kind == "onehot":
        q0 = T // 2
        q1 = q0 + 1
        w[:, q0] = 1.0
    elif kind == "range":
        q0, q1 = T // 3, max(T // 3 + 1, (3 * T) // 4)
        w[:, q0:q1] = 1.0 / (q1 - q0)
    else:
        q0, q1 = 0, T
        w = torch.rand((B, T), generator=g)
    wref = torch.zeros((B, T), dtype=torch.float64)
    wref[:, q0:q1] = w[:, q0:q1].double()
    return w.to(dev), wref.to(dev), q0, q1


@pytest.mark.parametrize("amp", [0.5, 2.5])
@pytest.mark.parametrize("T", [1, 31, 65, 129, 257, 1033])
@pytest.mark.parametrize("H", [1, 3, 12])
@pytest.mark.parametrize("B", [1, 4])
def test_colsum_kernel(dev, B, H, T, amp):
    from gaviko_amd import ops
    Q, s2 = _operands(B, T, H, amp, 1000 + 7 * T + H + B, dev)
    P, lse = _probs(s2)
    lse32 = lse.float().contiguous()
    n = B * H * T
    for kind in ("onehot", "range", "dense"):
        w, wref, q0, q1 = _weights(kind, B, T, dev, T + H)
        buf = torch.full((n + 4096,), float("nan"), device=dev)
        out = buf[:n]
        ops.attention_colsum(Q, lse32, w, out, B, T, H, q0=q0, q1=q1)
        torch.cuda.synchronize()
        ref = torch.einsum("bi,bhij->bhj", wref, P)
        err = (out.view(B, H, T).double() - ref).abs().max().item()
        bound = 1e-5 + 1e-4 * ref.abs().max().item()
        assert err < bound, f"{kind}: err {err:.3e} bound {bound:.3e}"
        assert torch.isnan(buf[n:]).all()                                   # nothing written past j < T of the last (b, h)
        again = torch.empty_like(out)
        ops.attention_colsum(Q, lse32, w, again, B, T, H, q0=q0, q1=q1)
        assert torch.equal(again, out)                                       # no atomics: bit-identical


@pytest.mark.parametrize("B,T,H", [(2, 1033, 3), (1, 1001, 12), (4, 65, 2)])
def test_colsum_with_forward_lse(dev, B, T, H):
    """lse from the flash forward itself: one row of P sums to 1."""
    from gaviko_amd import ops
    Q, _ = _operands(B, T, H, 2.0, 77 + T, dev)
    O = ops.act_zeros(B * T, H * 64, torch.bfloat16, dev)
    lse = torch.zeros((B, H, T), device=dev)
    ops.attention_fwd(Q, O, lse, B, T, H, 0.125, q_prescaled=True)
    out = torch.empty((B, H, T), device=dev)
    for row in (0, T // 2, T - 1):
        w = torch.zeros((B, T), device=dev)
        w[:, row] = 1.0
        ops.attention_colsum(Q, lse, w, out, B, T, H, q0=row, q1=row + 1)
        torch.cuda.synchronize()
        assert out.min().item() >= 0.0
        assert (out.double().sum(-1) - 1.0).abs().max().item() < 2e-3


@pytest.mark.parametrize("B,T,H", [(1, 1, 1), (4, 1033, 12), (2, 1001, 3), (2, 257, 16)])
def test_rollout_step_kernel(dev, B, T, H):
    from gaviko_amd import ops
    g = torch.Generator().manual_seed(T * H)
    r = torch.rand((B, T), generator=g).to(dev)
    cs = torch.rand((B, H, T), generator=g).to(dev)
    out = torch.empty_like(r)
    ops.rollout_step(r, cs, out, B, T, H)
    ref = 0.5 * r.double() + 0.5 * cs.double().mean(dim=1)
    assert (out.double() - ref).abs().max().item() < 1e-6 * max(1.0, ref.abs().max().item())
    again = r.clone()
    ops.rollout_step(again, cs, again, B, T, H)                              # in place
    assert torch.equal(again, out)


# ------------------------------------------------------------------------------------------------ whole model
def _build(z, dev, train=False):
    from gaviko_amd.registry import build_model
    from gaviko_amd.utils import synth
    m = build_model(ast.literal_eval(str(z["meta/cfg"])))
    sd = m.state_dict()
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev)
    m.train(train)
    return m


def _input(z, dev):
    from gaviko_amd.utils import synth
    return torch.from_numpy(synth.volumes(0, int(z["meta/batch"]))).to(dev)


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() / max(1e-300, b.abs().max().item())


@pytest.mark.parametrize("case", ["gaviko_t16_b2", "cfg1_linear_t16_b1"])
def test_rollout_against_engine_buffers(dev, case):
    """Rebuild every full P in float64 from the engine's saved qkv / lse, roll out in torch: the kernels' own error, apart from the bf16
    noise of the forward."""
    from gaviko_amd import explain
    z = golden("attn_" + case)
    model, x = _build(z, dev), _input(z, dev)
    logits, rel = explain.attention_rollout(model, x)
    _, maps = explain.attention_maps(model, x)
    eng = model._engine()
    _, ws = eng.attention_forward(x)
    B, H, T, inner = x.shape[0], eng.heads, eng.T, eng.heads * 64
    r0, R = explain._pool_range(eng, eng.depth - 1)
    w = torch.zeros((B, T), dtype=torch.float64, device=dev)
    w[:, r0:r0 + R] = 1.0 / R
    r = w.clone()
    worst = 0.0
    for l in range(eng.depth - 1, -1, -1):
        e = ws["qkv"][l][: B * T].view(B, T, -1).double()
        q = e[..., :inner].reshape(B, T, H, 64).transpose(1, 2)
        k = e[..., inner: 2 * inner].reshape(B, T, H, 64).transpose(1, 2)
        P = torch.exp2(q @ k.transpose(-1, -2) - ws["lse"][l].view(B, H, T).double()[..., None] * LOG2E)
        worst = max(worst, _rel(maps[l], torch.einsum("bi,bhij->bhj", w, P)))
        r = 0.5 * r + 0.5 * torch.einsum("bi,bhij->bhj", r, P).mean(dim=1)
        del P
    err = _rel(rel, r)
    REPORT.append(f"engine-buffer cross-check {case}: rollout rel {err:.3e}, pooled maps rel (worst layer) {worst:.3e}")
    print(REPORT[-1])
    assert err < 1e-4
    assert worst < 1e-4


FIXTURES = ["gaviko_t16_b2", "cfg1_linear_t16_b1", "dvpt_t16_b2_mean_p8", "deep_vpt_t16_b2", "cfg2_gaviko_b16_b4"]


@pytest.mark.parametrize("case", FIXTURES)
def test_against_reference_fixtures(dev, case):
    from gaviko_amd import explain
    z = golden("attn_" + case)
    model, x = _build(z, dev), _input(z, dev)
    floor = max(float(z[k]) for k in z.files if k.startswith("floor/"))
    bound = max(2e-2, 3 * floor)
    logits, maps = explain.attention_maps(model, x)
    errs = {}
    for k in z.files:
        if k.startswith("pool/layer"):
            errs[k] = _rel(maps[int(k[len("pool/layer"):])], z[k])
    assert errs
    L = model._engine().depth
    _, cls = explain.attention_maps(model, x, rows=int(z["meta/cls_row"]))
    for i in (0, L - 1):
        errs[f"cls/layer{i}"] = _rel(cls[i], z[f"cls/layer{i}"])
    for m in maps + cls:
        assert m.min().item() >= 0.0
    if "rollout" in z.files:
        _, rel = explain.attention_rollout(model, x)
        errs["rollout"] = _rel(rel, z["rollout"])
        assert (rel.double().sum(-1) - 1.0).abs().max().item() < 1e-5
        assert rel.min().item() >= 0.0
    worst = max(errs, key=errs.get)
    REPORT.append(f"reference {case}: bound {bound:.3e} (bf16 floor {floor:.3e}); worst {worst} {errs[worst]:.3e}; "
                  + ", ".join(f"{k} {v:.2e}" for k, v in sorted(errs.items())))
    print(REPORT[-1])
    assert errs[worst] < bound, REPORT[-1]


def test_logits_match_no_grad_forward(dev):
    from gaviko_amd import explain
    z = golden("attn_gaviko_t16_b2")
    model, x = _build(z, dev), _input(z, dev)
    with torch.no_grad():
        ref = model(x)
    logits, _ = explain.attention_rollout(model, x)
    assert not logits.requires_grad and logits.grad_fn is None
    assert _rel(logits, ref) <= 1e-5
    logits2, _ = explain.attention_maps(model, x)
    assert _rel(logits2, ref) <= 1e-5


def test_between_forward_and_backward(dev):
    """Two identical models run the same two SGD steps; the second calls attention_rollout between its first forward and backward."""
    from gaviko_amd import explain
    z = golden("attn_gaviko_t16_b2")
    x = _input(z, dev)
    y = torch.tensor([1, 3], device=dev)
    runs = []
    for explain_between in (False, True):
        model = _build(z, dev, train=True)
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.SGD(params, lr=0.1)
        steps = []
        for step in range(2):
            opt.zero_grad(set_to_none=True)
            logits = model(x)
            if explain_between and step == 0:
                explain.attention_rollout(model, x)
                explain.attention_maps(model, x)
            torch.nn.functional.cross_entropy(logits, y).backward()
            steps.append((logits.detach().clone(), [p.grad.detach().clone() for p in params]))
            opt.step()
        runs.append(steps)
    for step in range(2):
        (la, ga), (lb, gb) = runs[0][step], runs[1][step]
        assert torch.equal(la, lb), f"step {step}: logits differ"
        for a, b in zip(ga, gb):
            assert torch.equal(a, b), f"step {step}: gradients differ"


def test_rejections(dev):
    from gaviko_amd import explain
    from gaviko_amd.lib import GavikoHipError
    z = golden("attn_gaviko_t16_b2")
    model, x = _build(z, dev), _input(z, dev)
    with pytest.raises(GavikoHipError, match="HIP device"):
        explain.attention_maps(model, x.cpu())
    for which in ("local", "gpa"):
        with pytest.raises(GavikoHipError, match="global self-attention"):
            explain.attention_maps(model, x, attention=which)
    with pytest.raises(GavikoHipError, match="query row"):
        explain.attention_maps(model, x, rows=model._engine().T)
    model.set_precision("fp32")
    with pytest.raises(GavikoHipError, match="fp32"):
        explain.attention_rollout(model, x)
    zd = golden("attn_deep_vpt_t16_b2")
    deep = _build(zd, dev)
    with pytest.raises(GavikoHipError, match="deep VPT"):
        explain.attention_rollout(deep, _input(zd, dev))
