"""-m gpu: MWSA local-attention and GPA prompt-attention maps (gaviko_amd/explain.py, csrc/gaviko_maps.hip).

  * ops.window_attn_colsum / ops.gpa_attn_maps against float64 torch at every latent width, with exact statistics and with the forward's;
  * the host functions against float64 maps rebuilt from the engine's own kept buffers (kernel error alone);
  * against the reference's probabilities (tests/golden/gmaps_*.npz, tools/gen_gaviko_maps_golden.py) on the fp32 path (1e-4 of the largest
    element, the fp32 contract for derived quantities) and on the bf16 path (max(2e-2, 3 * the fixture's own bf16 floor));
  * an explanation between a training forward and its backward changes nothing of that step or the next; the rejections."""
import ast
import os

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

WIDTHS = [4, 8, 16, 20, 32]
CASES = ["gaviko_t16_b2", "gaviko_t16_b2_k366_p8", "gaviko_t16_b2_lat16", "gaviko_t16_b1_share2", "cfg2_gaviko_b16_b4"]
REPORT = []
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The measured errors of this module, written to $GAVIKO_MAPS_REPORT when that names a file (also printed: run with -s)."""
    yield
    out = os.environ.get("GAVIKO_MAPS_REPORT")
    if REPORT and out:
        with open(out, "w") as f:
            f.write("\n".join(REPORT) + "\n")


def _note(line):
    REPORT.append(line)
    print(line)


def _guarded(shape, dev):
    """A float32 output of `shape` with GUARD NaN words behind it -> (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), device=dev)
    return buf[:n].view(*shape), buf


def _guard_ok(buf):
    return bool(torch.isnan(buf[-GUARD:]).all()) and not bool(torch.isnan(buf[:-GUARD]).any())


def _close(got, ref, what):
    """The sibling kernel tests' bound: 1e-5 + 1e-4 * max|ref|."""
    got, ref = got.double().cpu(), ref.double().cpu()
    err, bound = (got - ref).abs().max().item(), 1e-5 + 1e-4 * ref.abs().max().item()
    return err, bound, f"{what}: max abs err {err:.3e} (bound {bound:.3e})"


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return (a - b).abs().max().item() / max(1e-300, b.abs().max().item())


def _weights(kind, B, N, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros((B, N))
    if kind == "onehot":
        w[:, N // 2] = 1.0
    elif kind == "range":
        w[:, N // 3: max(N // 3 + 1, (3 * N) // 4)] = 1.0 / (max(N // 3 + 1, (3 * N) // 4) - N // 3)
    else:
        w = torch.rand((B, N), generator=g)
    return w


# (grid, window, B): the three shipped windows, the degenerate one, one larger than the grid, non-cubic grids
WIN_CASES = [((10, 10, 10), (3, 3, 3), 1), ((10, 10, 10), (3, 6, 6), 4), ((10, 10, 10), (6, 6, 6), 4), ((10, 10, 10), (1, 1, 1), 1),
             ((4, 5, 6), (9, 13, 8), 4), ((7, 3, 5), (3, 6, 6), 1)]


@pytest.mark.parametrize("grid,win,B", WIN_CASES)
@pytest.mark.parametrize("Lat", WIDTHS)
def test_window_attn_colsum_kernel(dev, Lat, grid, win, B):
    from gaviko_amd import ops
    from oracle.gaviko_ref import window_mask
    N, C_ = grid[0] * grid[1] * grid[2], 192
    scale = C_ ** -0.5
    g = torch.Generator().manual_seed(1000 * Lat + N + B)
    qkv = ((torch.rand((B, N, 3 * Lat), generator=g) * 2 - 1) * 6.0).float()
    q, k, _ = qkv.double().chunk(3, -1)
    s = q @ k.transpose(-2, -1) * scale + window_mask(grid, win, dtype=torch.float64)
    P = s.softmax(-1)
    qkv_d = qkv.reshape(B * N, -1).to(dev).contiguous()
    lse_exact = torch.logsumexp(s, -1).float().reshape(-1).to(dev)
    lse_fwd = torch.zeros(B * N, device=dev)
    ctx = torch.zeros((B * N, Lat), device=dev)
    ops.window_attn_fwd(qkv=qkv_d, ctx=ctx, lse=lse_fwd, B=B, D=grid[0], H=grid[1], W=grid[2], kd=win[0], kh=win[1], kw=win[2], L=Lat, scale=scale)
    worst = 0.0
    for kind in ("onehot", "range", "dense"):
        w = _weights(kind, B, N, 7 * Lat + B)
        ref = torch.einsum("bi,bij->bj", w.double(), P)
        for lse, name in ((lse_exact, "exact lse"), (lse_fwd, "forward lse")):
            out, buf = _guarded((B, N), dev)
            ops.window_attn_colsum(qkv_d, lse, w.to(dev), out, B, *grid, *win, Lat, scale)
            err, bound, msg = _close(out, ref, f"window colsum L={Lat} grid={grid} window={win} B={B} w={kind} {name}")
            worst = max(worst, err / bound)
            assert err < bound, msg
            assert _guard_ok(buf), msg + ": guard words written"
            again, _ = _guarded((B, N), dev)
            ops.window_attn_colsum(qkv_d, lse, w.to(dev), again, B, *grid, *win, Lat, scale)
            assert torch.equal(out, again), msg + ": second run differs"
    _note(f"window_attn_colsum L={Lat} grid={grid} window={win} B={B}: worst err / bound {worst:.3f}")


def _gpa_forward(dev, B, N, P, Lat, seed):
    """Random latents and gate / query weights through ops.gpa_fwd -> everything it saves (device tensors)."""
    from gaviko_amd import ops
    g = torch.Generator().manual_seed(seed)
    T = P + 1 + N
    r = lambda *s, a=1.0: ((torch.rand(s, generator=g) * 2 - 1) * a).to(dev)
    z = lambda *s: torch.zeros(s, device=dev)
    t = dict(xl=r(B * T, Lat, a=2.0), ll=r(B * N, Lat, a=2.0), ca0_g=1 + r(Lat, a=0.2), ca0_b=r(Lat, a=0.2), ca1_w=r(64, Lat, a=0.4), ca1_b=r(64, a=0.2),
             ca3_w=r(max(P, 1), 64, a=0.4), ca3_b=r(P, a=0.2), gl0_g=1 + r(Lat, a=0.2), gl0_b=r(Lat, a=0.2), gl1_w=r(Lat, a=0.5), gl1_b=r(1, a=0.5),
             wgq=r(Lat, Lat, a=0.8), bgq=r(Lat, a=0.3), wlq=r(Lat, Lat, a=0.8), blq=r(Lat, a=0.3),
             imp=z(B, P), gw=z(B), enh=z(B, P, Lat), prm=z(B, P, Lat), qg=z(B, P, Lat), ql=z(B, P, Lat), cg=z(B, P, Lat), cl=z(B, P, Lat),
             lse_g=z(B, P), lse_l=z(B, P))
    ops.gpa_fwd(B=B, T=T, N=N, P=P, L=Lat, scale=Lat ** -0.5, **t)
    return t


@pytest.mark.parametrize("N", [1000, 27])
@pytest.mark.parametrize("P", [1, 8, 32])
@pytest.mark.parametrize("Lat", WIDTHS)
def test_gpa_attn_maps_kernel(dev, Lat, P, N):
    from gaviko_amd import ops
    from gaviko_amd.lib import GavikoHipError
    B = 3
    T = P + 1 + N
    z = lambda *s: torch.zeros(s, device=dev)
    if N <= P + 1:
        # P = 32 prompts on 27 patches: the reference's double slice (gaviko.py:161,107) leaves the global softmax no token at all, and
        # gvk_gpa_fwd rejects the shape -- so must the map kernel, before any launch
        with pytest.raises(GavikoHipError, match="double"):
            ops.gpa_attn_maps(z(B * T, Lat), z(B * N, Lat), z(B, P, Lat), z(B, P, Lat), z(B, P), z(B, P), z(B, P), z(B), B, T, N, P, Lat,
                              fused=z(B, P, N))
        return
    t = _gpa_forward(dev, B, N, P, Lat, 31 * Lat + P + N)
    xl, ll = t["xl"].double().view(B, T, Lat), t["ll"].double().view(B, N, Lat)
    # float64 reference from the forward's own (pre-scaled) queries: true softmax, no use of the saved statistics
    sg = torch.einsum("bpd,bnd->bpn", t["qg"].double(), xl[:, 2 * P + 2:])
    sl = torch.einsum("bpd,bnd->bpn", t["ql"].double(), ll)
    pg = torch.zeros((B, P, N), dtype=torch.float64, device=dev)
    pg[:, :, P + 1:] = sg.softmax(-1)
    pl = sl.softmax(-1)
    imp, gw = t["imp"].double()[:, :, None], t["gw"].double()[:, None, None]
    fu = imp * (gw * pg + (1 - gw) * pl)
    worst = 0.0
    for name, lg, ll_ in (("forward lse", t["lse_g"], t["lse_l"]),
                          ("exact lse", torch.logsumexp(sg, -1).float().contiguous(), torch.logsumexp(sl, -1).float().contiguous())):
        outs = [_guarded((B, P, N), dev) for _ in range(3)]
        args = (t["xl"], t["ll"], t["qg"], t["ql"], lg, ll_, t["imp"], t["gw"], B, T, N, P, Lat)
        ops.gpa_attn_maps(*args, global_=outs[0][0], local=outs[1][0], fused=outs[2][0])
        for (o, buf), ref, what in zip(outs, (pg, pl, fu), ("global", "local", "fused")):
            err, bound, msg = _close(o, ref, f"gpa maps L={Lat} P={P} N={N} {what} {name}")
            worst = max(worst, err / bound)
            assert err < bound, msg
            assert _guard_ok(buf), msg + ": guard words written"
            assert o.min().item() >= 0.0
        assert (outs[0][0][:, :, :P + 1] == 0).all()
        # nullable outputs: each alone gives the same bits; a second run too
        for idx, key in enumerate(("global_", "local", "fused")):
            o, buf = _guarded((B, P, N), dev)
            ops.gpa_attn_maps(*args, **{key: o})
            assert torch.equal(o, outs[idx][0]) and _guard_ok(buf), f"{key} alone"
    with pytest.raises(GavikoHipError, match="no output"):
        ops.gpa_attn_maps(*args)
    _note(f"gpa_attn_maps L={Lat} P={P} N={N}: worst err / bound {worst:.3f}")


def test_kernel_wrappers_reject(dev):
    from gaviko_amd import ops
    from gaviko_amd.lib import GavikoHipError
    z = lambda *s, dt=torch.float32: torch.zeros(s, device=dev, dtype=dt)
    B, N, Lat = 1, 27, 8
    ok = dict(qkv=z(B * N, 3 * Lat), lse=z(B * N), w=z(B, N), out=z(B, N))
    call = lambda **kw: ops.window_attn_colsum(*(dict(ok, **kw)[k] for k in ("qkv", "lse", "w", "out")), B, 3, 3, 3, 3, 3, 3, kw.get("Lat", Lat), 0.1)
    call()
    with pytest.raises(GavikoHipError, match="unsupported"):
        ops.window_attn_colsum(z(B * N, 36), ok["lse"], ok["w"], ok["out"], B, 3, 3, 3, 3, 3, 3, 12, 0.1)
    with pytest.raises(GavikoHipError, match="expected torch.float32"):
        call(w=z(B, N, dt=torch.float64))
    with pytest.raises(GavikoHipError, match="elements"):
        call(out=z(B, N - 1))
    with pytest.raises(GavikoHipError, match="HIP device"):
        call(lse=torch.zeros(B * N))
    with pytest.raises(GavikoHipError, match="positive ints"):
        ops.window_attn_colsum(ok["qkv"], ok["lse"], ok["w"], ok["out"], B, 3, 3, 3, 0, 3, 3, Lat, 0.1)
    P, T = 4, 4 + 1 + N
    g = (z(B * T, Lat), z(B * N, Lat), z(B, P, Lat), z(B, P, Lat), z(B, P), z(B, P), z(B, P), z(B))
    ops.gpa_attn_maps(*g, B, T, N, P, Lat, fused=z(B, P, N))
    with pytest.raises(GavikoHipError, match="unsupported"):
        ops.gpa_attn_maps(*g, B, T, N, P, 12, fused=z(B, P, N))
    with pytest.raises(GavikoHipError, match="T = P \\+ 1 \\+ N"):
        ops.gpa_attn_maps(*g, B, T + 1, N, P, Lat, fused=z(B, P, N))
    with pytest.raises(GavikoHipError, match="elements"):
        ops.gpa_attn_maps(*g, B, T, N, P, Lat, fused=z(B, P, N - 1))
    with pytest.raises(GavikoHipError, match="expected torch.float32"):
        ops.gpa_attn_maps(*g, B, T, N, P, Lat, local=z(B, P, N, dt=torch.bfloat16))


# ---- whole model -----------------------------------------------------------------------------------------------------------------
def _build(z, dev, train=False, precision=None):
    from gaviko_amd.registry import build_model
    from gaviko_amd.utils import synth
    m = build_model(ast.literal_eval(str(z["meta/cfg"])))
    sd = m.state_dict()
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev)
    if precision:
        m.set_precision(precision)
    m.train(train)
    return m


def _input(z, dev):
    from gaviko_amd.utils import synth
    return torch.from_numpy(synth.volumes(0, int(z["meta/batch"]))).to(dev)


@pytest.mark.parametrize("case", ["gaviko_t16_b2", "gaviko_t16_b2_k366_p8"])
def test_against_engine_buffers(dev, case):
    """Rebuild every probability block in float64 from the engine's own kept buffers (true softmax, no use of the saved statistics):
    the map kernels' own error plus that of the forward's lse, apart from whatever noise the forward itself carries."""
    from gaviko_amd import explain
    from oracle.gaviko_ref import window_mask
    z = golden("gmaps_" + case)
    model, x = _build(z, dev), _input(z, dev)
    _, lmaps = explain.local_attention_maps(model, x)
    _, gpa = explain.gpa_attention_maps(model, x)
    _, roll = explain.local_rollout(model, x)
    eng = model._engine()
    _, ws = eng.attention_forward(x)
    B, N, P, T, Lat = x.shape[0], eng.N, eng.P, eng.T, eng.Lat
    mask = window_mask(tuple(eng.grid), tuple(eng.win), dtype=torch.float64).to(dev)
    r = torch.full((B, N), 1.0 / N, dtype=torch.float64, device=dev)
    errs = {}
    for l in range(eng.depth - 1, -1, -1):
        q, k, _ = ws["mw"][l]["qkv"].double().view(B, N, 3 * Lat).chunk(3, -1)
        Pm = (q @ k.transpose(-2, -1) * eng.C ** -0.5 + mask).softmax(-1)
        errs["local"] = max(errs.get("local", 0.0), _rel(lmaps[l], Pm.mean(1)))
        r = 0.5 * r + 0.5 * torch.einsum("bi,bij->bj", r, Pm)
        g = ws["gp"][l]
        xl, ll = g["xl"].double().view(B, T, Lat), g["ll"].double().view(B, N, Lat)
        pg = torch.zeros((B, P, N), dtype=torch.float64, device=dev)
        pg[:, :, P + 1:] = torch.einsum("bpd,bnd->bpn", g["qg"].double(), xl[:, 2 * P + 2:]).softmax(-1)
        pl = torch.einsum("bpd,bnd->bpn", g["ql"].double(), ll).softmax(-1)
        fu = g["imp"].double()[:, :, None] * (g["gw"].double()[:, None, None] * pg + (1 - g["gw"].double()[:, None, None]) * pl)
        for name, got, ref in (("global", gpa[l].global_, pg), ("local_gpa", gpa[l].local, pl), ("fused", gpa[l].fused, fu)):
            errs[name] = max(errs.get(name, 0.0), _rel(got, ref))
        assert torch.equal(gpa[l].importance, g["imp"]) and torch.equal(gpa[l].global_weight, g["gw"])
        assert gpa[l].importance.data_ptr() != g["imp"].data_ptr()                  # clones, not views into the workspace
    errs["rollout"] = _rel(roll, r)
    _note(f"engine-buffer cross-check {case}: " + ", ".join(f"{k} rel {v:.3e}" for k, v in sorted(errs.items())))
    for k, v in errs.items():
        assert v < 1e-4, (k, v)


def _measure(model, x, z):
    """{fixture key: (error, 'rel' | 'abs')} of everything a gmaps fixture stores, plus the structural checks on the maps."""
    from gaviko_amd import explain
    logits, lmaps = explain.local_attention_maps(model, x)
    _, gpa = explain.gpa_attention_maps(model, x)
    _, roll = explain.local_rollout(model, x)
    L = int(z["meta/depth"])
    sel = [int(p) for p in z["meta/block_prompts"]]
    errs = {}
    for i in (int(v) for v in z["meta/layers"]):
        errs[f"local/all/layer{i}"] = (_rel(lmaps[i], z[f"local/all/layer{i}"]), "rel")
        for name, t in (("global", gpa[i].global_), ("local", gpa[i].local), ("fused", gpa[i].fused)):
            errs[f"gpa/{name}_mean/layer{i}"] = (_rel(t.double().mean(1), z[f"gpa/{name}_mean/layer{i}"]), "rel")
            if i in (0, L - 1):
                errs[f"gpa/{name}/layer{i}"] = (_rel(t[:, sel], z[f"gpa/{name}/layer{i}"]), "rel")
        for name, t in (("importance", gpa[i].importance), ("global_weight", gpa[i].global_weight)):
            ref = torch.as_tensor(z[f"gpa/{name}/layer{i}"]).double()
            errs[f"gpa/{name}/layer{i}"] = ((t.double().cpu() - ref).abs().max().item(), "abs")
        assert (gpa[i].fused.double().sum(-1) - gpa[i].importance.double()).abs().max().item() < 1e-5
        for t in (lmaps[i], gpa[i].global_, gpa[i].local, gpa[i].fused):
            assert t.min().item() >= 0.0
    for q in (int(v) for v in z["meta/rows"]):
        _, rows = explain.local_attention_maps(model, x, rows=q)
        for i in (0, L - 1):
            errs[f"local/row{q}/layer{i}"] = (_rel(rows[i], z[f"local/row{q}/layer{i}"]), "rel")
            assert ((rows[i] != 0).cpu().numpy() == (z[f"local/row{q}/layer{i}"] != 0)).all()      # zeros exactly outside the window
    errs["local_rollout"] = (_rel(roll, z["local_rollout"]), "rel")
    assert (roll.double().sum(-1) - 1.0).abs().max().item() < 1e-5 and roll.min().item() >= 0.0
    return logits, errs


@pytest.mark.parametrize("case", CASES)
def test_fp32_path_against_reference_fixtures(dev, case):
    """The exact-fp32 path reproduces the reference's own probabilities to 1e-4 of the largest element (the project's fp32 contract for
    derived quantities, tests/test_model_gpu.py::test_fp32_path_vs_golden); the two gates are sigmoids in (0, 1) and are held to the
    same figure absolutely."""
    z = golden("gmaps_" + case)
    model, x = _build(z, dev, precision="fp32"), _input(z, dev)
    logits, errs = _measure(model, x, z)
    worst = max(errs, key=lambda k: errs[k][0])
    _note(f"reference fp32 {case}: bound 1e-4; logits rel {_rel(logits, z['logits']):.3e}; worst {worst} {errs[worst][0]:.3e}; "
          + ", ".join(f"{k} {v[0]:.2e}" for k, v in sorted(errs.items())))
    assert errs[worst][0] < 1e-4, REPORT[-1]


@pytest.mark.parametrize("case", CASES)
def test_bf16_path_against_reference_fixtures(dev, case):
    """bf16 backbone: max(2e-2, 3 * floor) with the fixture's own floor/* (tests/test_attention_maps_gpu.py::test_against_reference_fixtures'
    rule), relative to the largest element; importance and global_weight absolutely."""
    z = golden("gmaps_" + case)
    model, x = _build(z, dev), _input(z, dev)
    floor = max(float(z[k]) for k in z.files if k.startswith("floor/"))
    bound = max(2e-2, 3 * floor)
    _, errs = _measure(model, x, z)
    worst = max(errs, key=lambda k: errs[k][0])
    _note(f"reference bf16 {case}: bound {bound:.3e} (bf16 floor {floor:.3e}); worst {worst} {errs[worst][0]:.3e}; "
          + ", ".join(f"{k} {v[0]:.2e}" for k, v in sorted(errs.items())))
    assert errs[worst][0] < bound, REPORT[-1]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_rows_start_and_layer(dev, precision):
    """rows as a weight tensor equals the int / 'all' forms; local_rollout from a start at an inner layer is the documented recurrence."""
    from gaviko_amd import explain
    z = golden("gmaps_gaviko_t16_b2_k366_p8")
    model, x = _build(z, dev, precision=precision), _input(z, dev)
    eng = model._engine()
    B, N = x.shape[0], eng.N
    _, all_maps = explain.local_attention_maps(model, x)
    _, same = explain.local_attention_maps(model, x, rows=torch.full((B, N), 1.0 / N, device=dev))
    q = int(z["meta/rows"][1])
    onehot = torch.zeros((B, N), device=dev)
    onehot[:, q] = 1.0
    _, row_t = explain.local_attention_maps(model, x, rows=onehot)
    _, row_i = explain.local_attention_maps(model, x, rows=q)
    for i in range(eng.depth):
        assert torch.equal(all_maps[i], same[i]) and torch.equal(row_t[i], row_i[i])
        assert (row_i[i].double().sum(-1) - 1.0).abs().max().item() < 1e-5
    _, gpa = explain.gpa_attention_maps(model, x)
    layer = 3
    start = gpa[layer].local.mean(1)
    _, rel = explain.local_rollout(model, x, start=start, layer=layer)
    r = start.clone()
    for l in range(layer, -1, -1):
        _, step = explain.local_attention_maps(model, x, rows=r)
        r = 0.5 * r + 0.5 * step[l]
    assert _rel(rel, r) < 1e-5
    assert (rel.double().sum(-1) - start.double().sum(-1)).abs().max().item() < 1e-5
    assert start.data_ptr() != rel.data_ptr() and torch.equal(start, gpa[layer].local.mean(1))       # start is not written


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_logits_match_no_grad_forward(dev, precision):
    from gaviko_amd import explain
    z = golden("gmaps_gaviko_t16_b2")
    model, x = _build(z, dev, precision=precision), _input(z, dev)
    with torch.no_grad():
        ref = model(x)
    for fn in (explain.local_attention_maps, explain.gpa_attention_maps, explain.local_rollout):
        logits, _ = fn(model, x)
        assert not logits.requires_grad and logits.grad_fn is None
        assert _rel(logits, ref) <= 1e-5


def test_between_forward_and_backward(dev):
    """Two identical models run the same two SGD steps; the second calls the three functions between its first forward and backward."""
    from gaviko_amd import explain
    z = golden("gmaps_gaviko_t16_b2")
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
                explain.local_attention_maps(model, x)
                explain.gpa_attention_maps(model, x)
                explain.local_rollout(model, x)
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
    z = golden("gmaps_gaviko_t16_b2")
    model, x = _build(z, dev), _input(z, dev)
    B, N = x.shape[0], model._engine().N
    fns = (explain.local_attention_maps, explain.gpa_attention_maps, explain.local_rollout)
    for fn in fns:
        with pytest.raises(GavikoHipError, match="HIP device"):
            fn(model, x.cpu())
    for bad in (N, -1, True, "pool", 1.5):
        with pytest.raises(GavikoHipError, match="rows"):
            explain.local_attention_maps(model, x, rows=bad)
    for bad in (torch.zeros((B, N + 1), device=dev), torch.zeros((B, N), device=dev, dtype=torch.float64), torch.zeros((B, N))):
        with pytest.raises(GavikoHipError, match="rows"):
            explain.local_attention_maps(model, x, rows=bad)
        with pytest.raises(GavikoHipError, match="start"):
            explain.local_rollout(model, x, start=bad)
    for bad in (12, -1, True, 1.0):
        with pytest.raises(GavikoHipError, match="layer"):
            explain.local_rollout(model, x, layer=bad)
    zl = golden("attn_cfg1_linear_t16_b1")
    plain, xp = _build(zl, dev), _input(zl, dev)
    for fn in fns:
        with pytest.raises(GavikoHipError, match="GAViKO models only"):
            fn(plain, xp)
    # existing behaviour stays: the global functions refuse the side-path attentions, and the fp32 path
    for which in ("local", "gpa"):
        with pytest.raises(GavikoHipError, match="global self-attention"):
            explain.attention_maps(model, x, attention=which)
    model.set_precision("fp32")
    with pytest.raises(GavikoHipError, match="fp32"):
        explain.attention_rollout(model, x)
