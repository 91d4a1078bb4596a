"""-m gpu: gradients with respect to the input volume -- img.grad through the autograd bridge, torch.autograd.grad(out, img), and the
attribution functions of gaviko_amd.explain -- against the oracle's autograd (plain torch on CPU), finite differences, and the invariances
the engine promises (parameter gradients bit-identical with and without img.requires_grad; an input-only sweep changes no parameter
gradient; launch-plan replay reproduces the eager result)."""
import pytest
import torch

import dropmask
import oracle

pytestmark = pytest.mark.gpu

BASE = dict(image_size=160, image_patch_size=16, frames=120, frame_patch_size=12, num_classes=5, channels=1, pool="cls", dim_head=64,
            dropout=0.0, emb_dropout=0.0)
GAVIKO = dict(num_prompts=8, prompt_latent_dim=20, local_dim=20, local_k=(3, 6, 6), DHW=(10, 10, 10), attn_drop=0.0, proj_drop=0.0,
              freeze_vit=True, share_factor=1)
METHODS = [("gaviko", dict(GAVIKO)), ("linear", {}), ("fft", {}), ("bitfit", {}),
           ("deep_vpt", dict(num_prompts=8, prompt_dim=64, prompt_dropout=0.0, freeze_vit=True, deep_prompt=True)),
           ("shallow_vpt", dict(num_prompts=8, prompt_dim=64, prompt_dropout=0.0, freeze_vit=True, deep_prompt=False)),
           ("adaptformer", dict(freeze_vit=True)), ("melo", dict(r=4, alpha=4)), ("ssf", dict(freeze_vit=True)),
           ("dvpt", dict(num_prompts=8, freeze_vit=True)), ("evp", dict(freeze_vit=True))]


def build(method, extra, dev, backbone="vit-t16"):
    from gaviko_amd.registry import build_model
    from gaviko_amd.utils import synth
    cfg = dict(BASE, backbone=backbone, method=method, **extra)
    m = build_model(cfg)
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev)
    m.train()
    return m, cfg


def volumes(B, first=0):
    from gaviko_amd.utils import synth
    return torch.from_numpy(synth.volumes(first, B)), torch.from_numpy(synth.labels(first, B))


def oracle_img_grad(method, m, cfg, x, y, masks=None, bf16=False):
    """img.grad of cross_entropy(oracle(x), y) on CPU (bf16: the oracle's bf16-operand noise-floor mode)."""
    from oracle import vit_ref
    ocfg = {k: v for k, v in cfg.items() if k != "precision"}
    sd = {k: v.detach().cpu().clone().requires_grad_(oracle.trainable(method, k, ocfg)) for k, v in m.state_dict().items()}
    xi = x.clone().requires_grad_()
    old = vit_ref.BF16_OPERANDS
    vit_ref.BF16_OPERANDS = bf16
    try:
        out = oracle.FORWARD[method](sd, xi, dict(ocfg, _masks=masks) if masks else ocfg, None)
        torch.nn.functional.cross_entropy(out, y).backward()
    finally:
        vit_ref.BF16_OPERANDS = old
    return xi.grad.double()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() / max(1e-30, b.abs().max().item())


def step_img_grad(m, x, y, dev):
    xi = x.to(dev).clone().requires_grad_()
    torch.nn.functional.cross_entropy(m(xi), y.to(dev)).backward()
    torch.cuda.synchronize()
    return xi.grad


@pytest.mark.parametrize("method,extra", METHODS, ids=[m for m, _ in METHODS])
def test_img_grad_matches_oracle_fp32_and_bf16(dev, method, extra):
    """loss.backward() with img.requires_grad fills img.grad (None before this feature): fp32 path within 1e-4 of max|ref| (the model
    tests' fp32 gradient bound); bf16 path within max(2e-2, 3 x the floor), the floor = the oracle's own bf16-operand error on this input."""
    x, y = volumes(2)
    m, cfg = build(method, dict(extra, precision="fp32"), dev)
    want = oracle_img_grad(method, m, cfg, x, y)
    got = step_img_grad(m, x, y, dev)
    assert got is not None and got.shape == x.shape
    assert rel(got, want) < 1e-4, rel(got, want)
    floor = rel(oracle_img_grad(method, m, cfg, x, y, bf16=True), want)
    for p in m.parameters():
        p.grad = None
    m.set_precision("bf16")
    got16 = step_img_grad(m, x, y, dev)
    assert rel(got16, want) < max(2e-2, 3 * floor), (rel(got16, want), floor)


@pytest.mark.parametrize("method,extra,live", [("fft", dict(dropout=0.1, emb_dropout=0.1), (0.1, 0.1)),
                                               ("gaviko", dict(GAVIKO, freeze_vit=False, dropout=0.1, emb_dropout=0.1), (0.1, 0.1)),
                                               ("melo", dict(r=4, alpha=4, dropout=0.1, emb_dropout=0.1), (0.1, 0.1))])
def test_img_grad_with_live_dropout_matches_oracle_with_the_same_masks(dev, method, extra, live):
    """Training mode with the backbone and embedding dropouts live (fp32 path): the oracle run with the kernels' masks."""
    from gaviko_amd import engine as E
    B = 2
    x, y = volumes(B)
    m, cfg = build(method, dict(extra, precision="fp32"), dev)
    got = step_img_grad(m, x, y, dev)
    eng = m._engine()
    word = int(eng._ws["seed"].item())
    t = torch.from_numpy
    bp, ep = live
    masks = {("emb", 0): t(dropmask.rows_mask(E.SEED_EMB + word, B * eng.T, eng.C, ep)).view(B, eng.T, eng.C)}
    if eng.kind == "gaviko":
        masks[("emb_local", 0)] = t(dropmask.rows_mask(E.SEED_EMB + 1 + word, B * eng.N, eng.C, ep)).view(B, eng.N, eng.C)
    for i in range(eng.depth):
        T, s = eng.Ts[i], E.SEED_LAYER + 8 * i + word
        masks[("attn", i)] = t(dropmask.attn_mask(s, B, eng.heads, T, bp))
        masks[("proj", i)] = t(dropmask.rows_mask(s + 1, B * T, eng.C, bp)).view(B, T, eng.C)
        masks[("act", i)] = t(dropmask.rows_mask(s + 2, B * T, eng.mlp, bp)).view(B, T, eng.mlp)
        masks[("ff", i)] = t(dropmask.rows_mask(s + 3, B * T, eng.C, bp)).view(B, T, eng.C)
    want = oracle_img_grad(method, m, cfg, x, y, masks=masks)
    assert rel(got, want) < 2e-4, rel(got, want)


def test_img_grad_matches_finite_differences_fp32(dev):
    """(f(x + eps v) - f(x - eps v)) / 2 eps against <g, v> for a random direction v, f = the sum of the target logits."""
    from gaviko_amd import explain
    m, cfg = build("gaviko", dict(GAVIKO, precision="fp32"), dev)
    x, _ = volumes(2)
    x = x.to(dev)
    tgt = torch.tensor([1, 3], device=dev)
    _, g = explain.input_gradient(m, x, tgt)
    gen = torch.Generator().manual_seed(7)
    v = torch.randn(x.shape, generator=gen).to(dev)
    eng = m._engine()
    eps = 1e-2 * x.abs().max().item()
    f = lambda z: eng.eval_forward(z).double().gather(1, tgt[:, None]).sum().item()   # noqa: E731
    with torch.no_grad():
        fd = (f(x + eps * v) - f(x - eps * v)) / (2 * eps)
    dot = (g.double() * v.double()).sum().item()
    assert abs(fd - dot) < 2e-3 * max(abs(dot), (g.double().abs() * v.double().abs()).sum().item() * 1e-2), (fd, dot)


INVARIANT = [("gaviko", dict(GAVIKO)), ("linear", {}), ("adaptformer", dict(freeze_vit=True)), ("evp", dict(freeze_vit=True)),
             ("ssf", dict(freeze_vit=True)), ("fft", {})]


@pytest.mark.parametrize("method,extra", INVARIANT, ids=[m for m, _ in INVARIANT])
def test_param_grads_bitwise_unchanged_by_img_requires_grad(dev, method, extra):
    """The same step with and without img.requires_grad: every parameter gradient bit-identical (GAViKO frozen: the bottom dead-row
    restriction is lifted for the input gradient, the rows the parameters read are the same bits).  Three rounds: eager, record, replay."""
    x, y = volumes(2)
    x, y = x.to(dev), y.to(dev)
    m, _ = build(method, extra, dev)
    named = dict(m.named_parameters())
    for _ in range(3):
        for req in (False, True):
            for p in m.parameters():
                p.grad = None
            xi = x.clone().requires_grad_(req)
            torch.nn.functional.cross_entropy(m(xi), y).backward()
            torch.cuda.synchronize()
            grads = {n: p.grad.clone() for n, p in named.items() if p.grad is not None}
            if req:
                assert xi.grad is not None and torch.isfinite(xi.grad).all()
                assert grads.keys() == ref.keys()
                for n in grads:
                    assert torch.equal(grads[n], ref[n]), n
            else:
                ref = grads


def test_autograd_grad_is_input_only_and_equals_backward(dev):
    """torch.autograd.grad(out, img) and backward(inputs=[img]): every p.grad and the flat gradient buffer bitwise unchanged, the result
    equal to img.grad from a plain backward(); gradients of parameters through autograd.grad keep raising."""
    from gaviko_amd.lib import GavikoHipError
    x, y = volumes(2)
    x, y = x.to(dev), y.to(dev)
    m, _ = build("gaviko", dict(GAVIKO), dev)
    eng = m._engine()
    xi = x.clone().requires_grad_()
    torch.nn.functional.cross_entropy(m(xi), y).backward()
    want = xi.grad.clone()
    before = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    flat = eng.flat_grad.clone()
    for how in ("grad", "inputs"):
        xj = x.clone().requires_grad_()
        loss = torch.nn.functional.cross_entropy(m(xj), y)
        if how == "grad":
            (g,) = torch.autograd.grad(loss, xj)
        else:
            loss.backward(inputs=[xj])
            g = xj.grad
        torch.cuda.synchronize()
        assert torch.equal(g, want), how
        assert torch.equal(eng.flat_grad, flat), how
        for n, p in m.named_parameters():
            if n in before:
                assert torch.equal(p.grad, before[n]), (how, n)
    anchor = next(p for p in m.parameters() if p.requires_grad)
    with pytest.raises(GavikoHipError, match="loss.backward"):
        torch.autograd.grad(torch.nn.functional.cross_entropy(m(x.clone().requires_grad_()), y), [anchor])


def test_frozen_model_and_non_leaf_input(dev):
    """Nothing trainable: the output still has a grad_fn when img needs a gradient; a non-leaf img = f(raw) chains to raw.grad."""
    x, y = volumes(2)
    x, y = x.to(dev), y.to(dev)
    m, _ = build("linear", dict(precision="fp32"), dev)
    want = step_img_grad(m, x, y, dev).clone()
    for p in m.parameters():
        p.requires_grad_(False)
        p.grad = None
    xi = x.clone().requires_grad_()
    out = m(xi)
    assert out.grad_fn is not None
    torch.nn.functional.cross_entropy(out, y).backward()
    assert rel(xi.grad, want) < 1e-6
    assert all(p.grad is None for p in m.parameters())
    raw = (x / 2).clone().requires_grad_()
    torch.nn.functional.cross_entropy(m(raw * 2.0), y).backward()
    assert rel(raw.grad, 2.0 * want) < 1e-6


def test_explain_between_forward_and_backward_leaves_the_step_unchanged(dev):
    """explain.input_gradient / smoothgrad / integrated_gradients between a training forward and its backward: that step's gradients are
    bit-identical to the same step without them."""
    from gaviko_amd import explain
    x, y = volumes(2)
    x, y = x.to(dev), y.to(dev)
    m, _ = build("gaviko", dict(GAVIKO), dev)

    def step(between):
        for p in m.parameters():
            p.grad = None
        out = m(x)
        if between:
            explain.input_gradient(m, x)
            explain.integrated_gradients(m, x, steps=2)
        torch.nn.functional.cross_entropy(out, y).backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    for _ in range(3):                                   # eager, record, replay of the training plans
        a_out, a = step(False)
        b_out, b = step(True)
        assert torch.equal(a_out, b_out)
        for n in a:
            assert torch.equal(a[n], b[n]), n


def test_relevance_backward_whose_seed_raises_leaves_the_step_unchanged(dev):
    """The exception path of the engine's state guard: relevance_backward between a training forward and its backward, with a seed
    callable that raises on the host.  The error comes through, _relv is cleared, the pending backward's gradients are bit-identical to the
    same step without the call, and a later relevance_backward equals a fresh engine's bit for bit."""
    x, y = volumes(1)
    x, y = x.to(dev), y.to(dev)
    m, _ = build("gaviko", dict(GAVIKO), dev)
    eng = m._engine()

    def failing_seed(logits):
        raise ValueError("no seed today")

    def step(interrupted):
        for p in m.parameters():
            p.grad = None
        out = m(x)
        if interrupted:
            with pytest.raises(ValueError, match="no seed today"):
                eng.relevance_backward(x, failing_seed)
            assert eng._relv is None
        torch.nn.functional.cross_entropy(out, y).backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    for _ in range(3):                                   # eager, record, replay of the training plans
        a_out, a = step(False)
        b_out, b = step(True)
        assert a and torch.equal(a_out, b_out)
        for n in a:
            assert torch.equal(a[n], b[n]), n

    seed = lambda logits: torch.nn.functional.one_hot(torch.tensor([2], device=dev), eng.K).to(logits.dtype)      # noqa: E731
    logits, _, rv = eng.relevance_backward(x, seed)
    fresh, _ = build("gaviko", dict(GAVIKO), dev)
    want_logits, _, want = fresh._engine().relevance_backward(x, seed)
    torch.cuda.synchronize()
    assert eng._relv is None
    assert torch.equal(logits, want_logits) and torch.equal(rv["r"], want["r"])
    assert float((rv["r"] - rv["w0"]).max()) > 0.0       # the relevance kernels did run


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_explain_replay_smoothgrad_and_batch_split(dev, precision):
    """Eager, recorded and replayed input-only sweeps give the same bits; smoothgrad(samples=1, sigma=0) is input_gradient; IG over steps
    split into engine batches of 2 equals one batch of 4 (same per-row gradients up to the GEMM's batch-size dependence)."""
    from gaviko_amd import explain
    x, _ = volumes(2)
    x = x.to(dev)
    m, _ = build("evp", dict(freeze_vit=True, precision=precision), dev)
    runs = [explain.input_gradient(m, x, 2) for _ in range(4)]
    for lg, g in runs[1:]:
        assert torch.equal(g, runs[0][1]) and torch.equal(lg, runs[0][0])
    lg_s, g_s = explain.smoothgrad(m, x, 2, samples=1, sigma=0.0)
    assert torch.equal(g_s, runs[0][1])
    _, gx = explain.input_gradient(m, x, 2, times_input=True)
    assert torch.equal(gx, runs[0][1] * x)
    _, a1, d1 = explain.integrated_gradients(m, x[:1], 2, steps=4, batch=4)
    _, a2, d2 = explain.integrated_gradients(m, x[:1], 2, steps=4, batch=2)
    assert rel(a2, a1) < (1e-5 if precision == "fp32" else 1e-2)
    grid = explain.patch_saliency(m, runs[0][1])
    assert grid.shape == (2,) + tuple(m._engine().grid)
    assert rel(grid, runs[0][1].abs().reshape(2, 10, 12, 10, 16, 10, 16).sum((2, 4, 6))) < 1e-5


def test_integrated_gradients_completeness_gap_shrinks_fp32(dev):
    from gaviko_amd import explain
    x, _ = volumes(1)
    x = x.to(dev)
    m, _ = build("linear", dict(precision="fp32"), dev)
    lg, _, d8 = explain.integrated_gradients(m, x, steps=8, batch=8)
    _, _, d64 = explain.integrated_gradients(m, x, steps=64, batch=16)
    span = (lg.max() - lg.min()).item()
    assert abs(d64.item()) < abs(d8.item()), (d8, d64)
    assert abs(d64.item()) < 2e-2 * max(1.0, span), (d64, span)


def test_explain_rejects_bad_input(dev):
    from gaviko_amd import explain
    from gaviko_amd.lib import GavikoHipError
    m, _ = build("linear", {}, dev)
    x, _ = volumes(1)
    with pytest.raises(GavikoHipError, match="HIP device"):
        explain.input_gradient(m, x)
    with pytest.raises(GavikoHipError, match="expected img"):
        explain.input_gradient(m, torch.zeros(1, 1, 120, 160, 128, device=dev))
    for bad in (5, -1, torch.tensor([7], device=dev), torch.tensor([0, 1], device=dev)):
        with pytest.raises(GavikoHipError, match="target"):
            explain.input_gradient(m, x.to(dev), bad)
    with pytest.raises(GavikoHipError, match="steps"):
        explain.integrated_gradients(m, x.to(dev), steps=0)
    with pytest.raises(GavikoHipError, match="reduce"):
        explain.patch_saliency(m, x.to(dev), reduce="max")
