"""-m gpu: the rank-L kernels of GAViKO's side paths at every latent width L and on every implementation their dispatchers pick, each
through the C-ABI against a float64 torch computation on the CPU (the default L = 20 shapes are in test_sidepath_kernels_gpu.py).

Dispatch table, from the guards in csrc/ (every parametrized case names the row it lands on):

  skinny_down   tier 1  launch_side_down (sidepass.hip)    L = 20, C in {192, 768, 1024}; w2 with L2 <= 64; act_in goes on to tier 2
                tier 2  launch_row_down (rowwise.hip)      L in {4, 8, 16, 20, 24}, 128 <= C <= 1024, C % 4 == 0, L2 <= 64
                tier 3  skinny_down_kernel<L> (skinny.hip) L in {4, 8, 16, 20, 32}, C % 4 == 0, C <= 1024; no act_in
  skinny_up     tier 1  launch_side_up                     L = 20, C in {192, 768, 1024}; no alpha_ptr / gg_x
                tier 2  launch_row_up                      L in {4, 8, 16, 20, 24}, 128 <= C <= 1024
                tier 3  skinny_up_kernel<L>                L in {4, 8, 16, 20, 32}; no alpha_ptr / gg_x
  outer_reduce          outer_partial_kernel<L>            L in {4, 8, 16, 20, 24, 32, 64}, M (+ M2) <= 64 x 160 = 10240
  window attn   mfma    win_mfma_{fwd,bwd}_kernel          L = 20, every grid side <= 1023, N <= 12288
                rows    win_{fwd,bwd_q,bwd_kv}_kernel<L>   L in {4, 8, 16, 20, 32}, every other shape
  gpa                   gpa_{fwd,bwd}_kernel<L>            L in {4, 8, 16, 20, 32}, 0 < P <= 64, T > 2P + 2
"""
import math

import pytest
import torch
import torch.nn.functional as F

import dropmask
from test_sidepath_kernels_gpu import _close, _rand, gpa_core_check

pytestmark = pytest.mark.gpu

M_ROWS = (1, 15, 17, 1033)


def _r32(t):
    """float64 values the fp32 device operand holds exactly"""
    return t.float().double()


def _f(dev):
    return lambda t: t.detach().float().to(dev).contiguous()


def _qg(t):
    return t * torch.sigmoid(1.702 * t)


def _qg_grad(t):
    s = torch.sigmoid(1.702 * t)
    return s + 1.702 * t * s * (1 - s)


def _mask(seed, M, C_, p):
    return torch.from_numpy(dropmask.rows_mask(seed, M, C_, p)).double()


def _nan(*shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _seed_word(dev, v):
    return torch.tensor([v], dtype=torch.int64, device=dev)


# ------------------------------------------------------------------------------------------------------------------------- skinny_down

DOWN = [(1, 20, 192), (1, 20, 768), (1, 20, 1024),
        (2, 4, 132), (2, 8, 260), (2, 16, 768), (2, 20, 260), (2, 24, 132), (2, 24, 768),
        (3, 4, 64), (3, 8, 96), (3, 16, 64), (3, 20, 96), (3, 32, 64), (3, 32, 260), (3, 32, 1024)]


def _down_inputs(M, C_, Lat, seed):
    x = _r32(_rand((M, C_), seed, 1.5) + 0.2)
    w = _r32(_rand((Lat, C_), seed + 1, 1 / math.sqrt(C_)))
    bias = _r32(_rand((Lat,), seed + 2, 0.1))
    g = _r32(1 + _rand((C_,), seed + 3, 0.2))
    bt = _r32(_rand((C_,), seed + 4, 0.1))
    w2 = _r32(_rand((3 * Lat, Lat), seed + 5, 0.5))
    return x, w, bias, g, bt, w2


@pytest.mark.parametrize("M", M_ROWS)
@pytest.mark.parametrize("tier,Lat,C_", DOWN, ids=[f"tier{t}-L{l}-C{c}" for t, l, c in DOWN])
def test_skinny_down(dev, tier, Lat, C_, M):
    from gaviko_amd import ops
    f = _f(dev)
    x, w, bias, g, bt, w2 = _down_inputs(M, C_, Lat, 201)
    L2 = 3 * Lat
    with_w2 = not (tier == 2 and L2 > 64)          # L = 24: L2 = 72 leaves the row kernel, and tier 3 has no L = 24 (test_skinny_down_rejects)
    n = F.layer_norm(x, (C_,), g, bt, 1e-5)
    mu, rs = x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()
    # LayerNorm (statistics saved) + second stage, act 0, w_layout 0
    z, y, mean, rstd = _nan(M, Lat, dev=dev), _nan(M, Lat, dev=dev), _nan(M, dev=dev), _nan(M, dev=dev)
    y2 = _nan(M, L2, dev=dev) if with_w2 else None
    ops.skinny_down(x=f(x), w=f(w), bias=f(bias), ln_gamma=f(g), ln_beta=f(bt), mean=mean, rstd=rstd, z=z, y=y,
                    w2=f(w2) if with_w2 else None, y2=y2, M=M, C=C_, L=Lat, L2=L2 if with_w2 else 0, act=0, w_layout=0, eps=1e-5)
    pre = n @ w.T + bias
    _close(mean, mu, 2e-5, "mean")
    _close(rstd, rs, 2e-5, "rstd")
    _close(z, pre, 2e-5, "LN z")
    _close(y, pre, 2e-5, "LN y")
    if with_w2:
        _close(y2, pre @ w2.T, 3e-5, "LN second stage")
    # LayerNorm + QuickGELU + w_layout 1 (+ second stage of the activated rows)
    z, y = _nan(M, Lat, dev=dev), _nan(M, Lat, dev=dev)
    y2 = _nan(M, L2, dev=dev) if with_w2 else None
    ops.skinny_down(x=f(x), w=f(w.T), bias=f(bias), ln_gamma=f(g), ln_beta=f(bt), z=z, y=y, w2=f(w2) if with_w2 else None, y2=y2,
                    M=M, C=C_, L=Lat, L2=L2 if with_w2 else 0, act=1, w_layout=1)
    _close(z, pre, 2e-5, "LN act z")
    _close(y, _qg(pre), 2e-5, "LN act y")
    if with_w2:
        _close(y2, _qg(pre) @ w2.T, 3e-5, "LN act second stage")
    # no LayerNorm: act 1 / w_layout 0, act 0 / w_layout 1
    raw = x @ w.T + bias
    for act, lay in ((1, 0), (0, 1)):
        z, y = _nan(M, Lat, dev=dev), _nan(M, Lat, dev=dev)
        ops.skinny_down(x=f(x), w=f(w if lay == 0 else w.T), bias=f(bias), z=z, y=y, M=M, C=C_, L=Lat, act=act, w_layout=lay)
        _close(z, raw, 2e-5, f"act{act} layout{lay} z")
        _close(y, _qg(raw) if act else raw, 2e-5, f"act{act} layout{lay} y")
    # input dropout (the backward of proj_drop): mask index m*C + c; seed alone, then seed + the device word
    for seed, word in ((1234, None), (77, 5151)):
        mk = _mask(seed + (word or 0), M, C_, 0.2)
        y = _nan(M, Lat, dev=dev)
        ops.skinny_down(x=f(x), w=f(w), bias=f(bias), y=y, M=M, C=C_, L=Lat, act=0, w_layout=0, drop_p=0.2, seed=seed,
                        seed_ptr=None if word is None else _seed_word(dev, word))
        _close(y, (x * mk) @ w.T + bias, 2e-5, f"dropout seed={seed} word={word}")
    # act_in = 1 (DVPT share_MLP: QuickGELU on the input rows): the row-per-wave kernel only
    y = torch.full((M, Lat), 7.0, device=dev)
    if tier == 3:
        with pytest.raises(ops.L.GavikoHipError, match="act_in needs the row-per-wave kernel"):
            ops.skinny_down(x=f(x), w=f(w), bias=f(bias), y=y, M=M, C=C_, L=Lat, act=0, w_layout=0, act_in=1)
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()), "a rejected act_in call wrote its output"
    else:
        ops.skinny_down(x=f(x), w=f(w.T), bias=f(bias), y=y, M=M, C=C_, L=Lat, act=1, w_layout=1, act_in=1)
        _close(y, _qg(_qg(x) @ w.T + bias), 2e-5, "act_in")


OFFSET_CASES = [(1, 20, 768), (2, 16, 768), (2, 20, 260), (3, 32, 768), (3, 8, 64), (3, 20, 96)]


@pytest.mark.parametrize("offset", [0.0, 40.0, 3000.0])
@pytest.mark.parametrize("tier,Lat,C_", OFFSET_CASES, ids=[f"tier{t}-L{l}-C{c}" for t, l, c in OFFSET_CASES])
def test_skinny_down_ln_large_common_offset(dev, tier, Lat, C_, offset):
    """Rows whose mean dwarfs their spread (|mean| / std up to ~5000), every tier that fuses a LayerNorm: mean / rstd as the two-pass
    statistics give them.  Before the tier-3 kernel centred its rows it took var = E[x^2] - mean^2 in fp32: rstd rel err 7e-4 at offset 40
    and 2e2 at offset 3000 (rstd ~ 1/sqrt(eps)), while tiers 1 and 2 stayed at 5e-7.  y is held to the offset-0 bound against the float64 LayerNorm centred on the mean the kernel
    returned: rounding that mean to fp32 (half an ulp of 3000 is 1.2e-4) moves every normalised value by ~2e-4 of the row's std, which
    no fp32 kernel avoids; that mean itself is held to 2e-6 of |mean| (as test_fold_row_statistics_with_large_common_offset)."""
    from gaviko_amd import ops
    f = _f(dev)
    M = 67
    _, w, bias, g, bt, w2 = _down_inputs(M, C_, Lat, 221)
    x = _r32(offset + _rand((M, C_), 231, 1.0) + _rand((M, 1), 232, 0.3) * (offset / 10))
    z, mean, rstd = _nan(M, Lat, dev=dev), _nan(M, dev=dev), _nan(M, dev=dev)
    y2 = _nan(M, 3 * Lat, dev=dev)
    ops.skinny_down(x=f(x), w=f(w), bias=f(bias), ln_gamma=f(g), ln_beta=f(bt), mean=mean, rstd=rstd, z=z, w2=f(w2), y2=y2,
                    M=M, C=C_, L=Lat, L2=3 * Lat, act=0, w_layout=0)
    torch.cuda.synchronize()
    mu, rs = x.mean(1), (x.var(1, unbiased=False) + 1e-5).rsqrt()
    gm, gr = mean.cpu().double(), rstd.cpu().double()
    e_mu = (gm - mu).abs().max().item()
    e_rs = ((gr - rs) / rs).abs().max().item()
    print(f"skinny_down tier {tier} L={Lat} C={C_} offset {offset}: mean err {e_mu:.2e}, rstd rel err {e_rs:.2e}")
    assert e_mu < 2e-6 * max(1.0, mu.abs().max().item()), f"mean: max err {e_mu:.3e}"
    assert e_rs < 2e-5, f"rstd: max rel err {e_rs:.3e}"
    pre = ((x - gm[:, None]) * rs[:, None] * g + bt) @ w.T + bias
    _close(z, pre, 2e-5, "z")
    _close(y2, pre @ w2.T, 3e-5, "second stage")


def test_skinny_down_rejects(dev):
    """Requests no tier covers raise with the library's message and leave the outputs alone."""
    from gaviko_amd import ops
    f = _f(dev)
    M = 40

    def rejected(match, C_, Lat, **kw):
        x, w, bias, g, bt, _ = _down_inputs(M, C_, Lat, 241)
        y = torch.full((M, Lat), 7.0, device=dev)
        with pytest.raises(ops.L.GavikoHipError, match=match):
            ops.skinny_down(x=f(x), w=f(w), bias=f(bias), y=y, M=M, C=C_, L=Lat, act=0, w_layout=0,
                            **{k: (f(v) if torch.is_tensor(v) else v) for k, v in kw.items()})
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()), f"rejected call ({match}) wrote its output"
        return g, bt

    rejected(r"L=24 unsupported", 64, 24)                                   # L = 24 below the row kernel's C >= 128
    rejected(r"L=12 unsupported", 256, 12)
    rejected(r"L=24 unsupported", 768, 24, w2=_rand((72, 24), 242), y2=torch.zeros((M, 72)), L2=72)    # L2 > 64: no row kernel
    g, bt = _down_inputs(M, 768, 20, 241)[3:5]
    rejected(r"act_in=1 \(QuickGELU on the input\) takes no LN", 768, 20, act_in=1, ln_gamma=g, ln_beta=bt)
    rejected(r"act_in=1 \(QuickGELU on the input\) takes no LN / dropout", 768, 20, act_in=1, drop_p=0.2, seed=3)
    rejected(r"C=66 must be a multiple of 4", 66, 8)


# --------------------------------------------------------------------------------------------------------------------------- skinny_up

UP = [(1, 20, 192), (1, 20, 768), (1, 20, 1024),
      (2, 4, 132), (2, 8, 260), (2, 16, 768), (2, 20, 260), (2, 24, 132), (2, 24, 1024),
      (3, 4, 64), (3, 8, 96), (3, 16, 64), (3, 20, 96), (3, 32, 64), (3, 32, 768), (3, 32, 1024)]


@pytest.mark.parametrize("M", M_ROWS)
@pytest.mark.parametrize("tier,Lat,C_", UP, ids=[f"tier{t}-L{l}-C{c}" for t, l, c in UP])
def test_skinny_up(dev, tier, Lat, C_, M):
    from gaviko_amd import ops
    f = _f(dev)
    lat = _r32(_rand((M, Lat), 301, 1.0))
    wu = _r32(_rand((C_, Lat), 302, 0.3))
    bu = _r32(_rand((C_,), 303, 0.1))
    res = _r32(_rand((M, C_), 304, 1.0))
    v = lat @ wu.T + bu
    # res, w_layout 0, with the bf16 copy: exactly out.bfloat16(), one rounding
    out = _nan(M, C_, dev=dev)
    o16 = torch.zeros((M, C_), dtype=torch.bfloat16, device=dev)
    ops.skinny_up(lat=f(lat), w=f(wu), bias=f(bu), res=f(res), out=out, out_bf16=o16, M=M, C=C_, L=Lat, w_layout=0)
    _close(out, res + v, 2e-5, "res")
    torch.cuda.synchronize()
    assert torch.equal(o16, out.bfloat16()), "out_bf16 is not out rounded once"
    # accumulate, w_layout 1, prompt-row override with P = 1 and P = T - 1 (samples of T rows, the last one possibly short)
    T = max(1, (M + 2) // 3)
    nb = (M + T - 1) // T
    for P in sorted({1, T - 1} - {0}):
        ov = _r32(_rand((nb, P, Lat), 305 + P, 1.0))
        lat2 = lat.clone()
        for s in range(nb):
            k = min(P, M - s * T)
            lat2[s * T: s * T + k] = ov[s, :k]
        acc0 = _r32(_rand((M, C_), 306, 1.0))
        out = f(acc0)
        ops.skinny_up(lat=f(lat), w=f(wu.T), bias=f(bu), out=out, lat_override=f(ov), M=M, C=C_, L=Lat, T=T, P=P, w_layout=1, accumulate=1)
        _close(out, acc0 + lat2 @ wu.T + bu, 2e-5, f"accumulate + override T={T} P={P}")
    # dropout on the projected value (mask index m*C + c): seed alone, then seed + the device word
    for seed, word in ((4321, None), (99, 60606)):
        mk = _mask(seed + (word or 0), M, C_, 0.2)
        out = _nan(M, C_, dev=dev)
        ops.skinny_up(lat=f(lat), w=f(wu), bias=f(bu), res=f(res), out=out, M=M, C=C_, L=Lat, w_layout=0, drop_p=0.2, seed=seed,
                      seed_ptr=None if word is None else _seed_word(dev, word))
        _close(out, res + v * mk, 2e-5, f"dropout seed={seed} word={word}")
    # DVPT's epilogue: alpha (device scalar) and QuickGELU'(gg_x), then the dropout mask -- the row-per-wave kernel only
    gg = _r32(_rand((M, C_), 307, 2.0))
    for alpha, use_gg, p in ((0.0, False, 0.0), (-0.75, True, 0.2), (1.3, False, 0.0), (1.0, True, 0.0)):
        out = torch.full((M, C_), 7.0, device=dev)
        kw = dict(lat=f(lat), w=f(wu), bias=f(bu), res=f(res), out=out, M=M, C=C_, L=Lat, w_layout=0, alpha_ptr=f(torch.tensor([alpha])),
                  gg_x=f(gg) if use_gg else None, drop_p=p, seed=55)
        if tier == 3:
            with pytest.raises(ops.L.GavikoHipError, match="alpha_ptr / gg_x need the row-per-wave kernel"):
                ops.skinny_up(**kw)
            torch.cuda.synchronize()
            assert bool((out == 7.0).all()), "a rejected alpha_ptr call wrote its output"
            break
        ops.skinny_up(**kw)
        want = alpha * v * (_qg_grad(gg) if use_gg else 1.0) * (_mask(55, M, C_, p) if p else 1.0)
        _close(out, res + want, 2e-5, f"alpha={alpha} gg_x={use_gg} p={p}")
    # LayerNorm-backward epilogue: out = res + d/dx <LN(x; g), lat . W^T>, statistics given
    x = _r32(_rand((M, C_), 308, 1.5) + 0.3)
    g = _r32(1 + _rand((C_,), 309, 0.2))
    mu = _r32(x.mean(1))
    rs = _r32((x.var(1, unbiased=False) + 1e-5).rsqrt())
    xa = x.clone().requires_grad_(True)
    F.layer_norm(xa, (C_,), g, None, 1e-5).backward(lat @ wu.T)
    out = _nan(M, C_, dev=dev)
    ops.skinny_up(lat=f(lat), w=f(wu), res=f(res), out=out, ln_x=f(x), ln_mean=f(mu), ln_rstd=f(rs), ln_gamma=f(g), M=M, C=C_, L=Lat,
                  w_layout=0)
    _close(out, res + xa.grad, 5e-5, "LN backward epilogue")


def test_skinny_up_rejects(dev):
    from gaviko_amd import ops
    f = _f(dev)
    M = 40
    for Lat, C_, match in ((24, 64, "L=24 unsupported"), (12, 256, "L=12 unsupported")):
        out = torch.full((M, C_), 7.0, device=dev)
        with pytest.raises(ops.L.GavikoHipError, match=match):
            ops.skinny_up(lat=f(_rand((M, Lat), 311)), w=f(_rand((C_, Lat), 312)), out=out, M=M, C=C_, L=Lat, w_layout=0)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------------ outer_reduce

@pytest.mark.parametrize("M", [1, 160, 161, 10240])
@pytest.mark.parametrize("Lat", [4, 8, 16, 20, 24, 32, 64])
def test_outer_reduce(dev, Lat, M):
    """outer_partial_kernel<L> (every L) over 1, one slab row count, one more, and the 10240-row limit."""
    from gaviko_amd import ops
    f = _f(dev)
    C_ = 260
    nar = _r32(_rand((M, Lat), 401, 1.0))
    wide = _r32(_rand((M, C_), 402, 1.0) + 0.1)
    g = _r32(1 + _rand((C_,), 403, 0.2)); bt = _r32(_rand((C_,), 404, 0.1))
    mu = _r32(wide.mean(1)); rs = _r32((wide.var(1, unbiased=False) + 1e-5).rsqrt())
    n = (wide - mu[:, None]) * rs[:, None] * g + bt
    scratch = torch.zeros(ops.outer_scratch_elems(Lat, C_), device=dev)
    # LayerNorm operands, transposed 0
    dW = _nan(Lat, C_, dev=dev)
    ops.outer_reduce(narrow=f(nar), wide=f(wide), mean=f(mu), rstd=f(rs), ln_gamma=f(g), ln_beta=f(bt), scratch=scratch, out=dW,
                     M=M, C=C_, L=Lat, transposed=0, accumulate=0)
    _close(dW, nar.T @ n, 5e-5, "LN")
    # plain, transposed 1, accumulate, column sums
    dWt = torch.ones((C_, Lat), device=dev); cs = torch.ones(C_, device=dev)
    ops.outer_reduce(narrow=f(nar), wide=f(wide), scratch=scratch, out=dWt, colsum=cs, M=M, C=C_, L=Lat, transposed=1, accumulate=1)
    _close(dWt, 1 + wide.T @ nar, 5e-5, "transposed accumulate")
    _close(cs, 1 + wide.sum(0), 5e-5, "colsum")
    # dropout mask on the wide rows: seed alone, then seed + the device word
    for seed, word in ((31, None), (8, 1000)):
        mk = _mask(seed + (word or 0), M, C_, 0.2)
        dW = _nan(Lat, C_, dev=dev)
        ops.outer_reduce(narrow=f(nar), wide=f(wide), scratch=scratch, out=dW, M=M, C=C_, L=Lat, transposed=0, drop_p=0.2, seed=seed,
                         seed_ptr=None if word is None else _seed_word(dev, word))
        _close(dW, nar.T @ (wide * mk), 5e-5, f"dropout seed={seed} word={word}")
    if M > 1:
        # second source: rows M1 .. M-1 from (narrow2, wide2)
        M1 = M - M // 3
        dW = _nan(Lat, C_, dev=dev)
        ops.outer_reduce(narrow=f(nar[:M1]), wide=f(wide[:M1]), narrow2=f(nar[M1:]), wide2=f(wide[M1:]), M2=M - M1, scratch=scratch, out=dW,
                         M=M1, C=C_, L=Lat, transposed=0)
        _close(dW, nar.T @ wide, 5e-5, "second source")


def test_outer_reduce_rejects_rows_over_limit(dev):
    from gaviko_amd import ops
    f = _f(dev)
    Lat, C_ = 20, 64
    scratch = torch.zeros(ops.outer_scratch_elems(Lat, C_), device=dev)
    out = torch.full((Lat, C_), 7.0, device=dev)
    nar, wide = f(_rand((10241, Lat), 411)), f(_rand((10241, C_), 412))
    with pytest.raises(ops.L.GavikoHipError, match="M=10241 exceeds 10240 rows"):
        ops.outer_reduce(narrow=nar, wide=wide, scratch=scratch, out=out, M=10241, C=C_, L=Lat)
    with pytest.raises(ops.L.GavikoHipError, match=r"M \+ M2 = 10241 exceeds 10240 rows"):
        ops.outer_reduce(narrow=nar[:10000], wide=wide[:10000], narrow2=nar[10000:], wide2=wide[10000:], M2=241, scratch=scratch, out=out,
                         M=10000, C=C_, L=Lat)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------- window attention

def _win_ref(qkv, dctx, grid, win, scale, mask_p=None):
    """dense float64: ctx, lse (natural log of the window's sum of exp(scale q.k): what both kernels store and their backward reads),
    delta = rowsum(dctx * ctx), dqkv"""
    from oracle.gaviko_ref import window_mask
    q, k, v = qkv.chunk(3, -1)
    s = q @ k.transpose(-2, -1) * scale + window_mask(grid, win, dtype=torch.float64)
    lse = torch.logsumexp(s, -1)
    attn = s.softmax(-1)
    if mask_p is not None:
        attn = attn * mask_p
    ctx = attn @ v
    ctx.backward(dctx)
    return ctx.detach(), lse.detach(), (dctx * ctx.detach()).sum(-1)


def _win_run(dev, qkv, dctx, B, grid, win, Lat, scale, **kw):
    from gaviko_amd import ops
    f = _f(dev)
    N = grid[0] * grid[1] * grid[2]
    ctx, lse, delta, dq = _nan(B * N, Lat, dev=dev), _nan(B * N, dev=dev), _nan(B * N, dev=dev), _nan(B * N, 3 * Lat, dev=dev)
    a = dict(qkv=f(qkv.reshape(B * N, -1)), ctx=ctx, lse=lse, B=B, D=grid[0], H=grid[1], W=grid[2], kd=win[0], kh=win[1], kw=win[2], L=Lat,
             scale=scale, **kw)
    ops.window_attn_fwd(**a)
    ops.window_attn_bwd(dctx=f(dctx.reshape(B * N, -1)), delta=delta, dqkv=dq, **a)
    torch.cuda.synchronize()
    return (ctx.cpu().double().view(B, N, Lat), lse.cpu().double().view(B, N), delta.cpu().double().view(B, N),
            dq.cpu().double().view(B, N, 3 * Lat))


def _impl(Lat, grid):
    return "mfma" if Lat == 20 and max(grid) <= 1023 and grid[0] * grid[1] * grid[2] <= 12288 else "rows"


GRID_WIN = [((10, 10, 10), (3, 6, 6)), ((10, 10, 10), (2, 4, 6)), ((10, 10, 10), (1, 1, 1)), ((10, 10, 10), None),
            ((4, 6, 9), (3, 6, 6)), ((4, 6, 9), (2, 4, 6)), ((4, 6, 9), (1, 1, 1)), ((4, 6, 9), None),
            ((1, 2, 3), (3, 6, 6)), ((1, 2, 3), (1, 1, 1)), ((1, 2, 3), None)]
WIN_CASES = [(Lat, B, g, w) for Lat in (4, 8, 16, 20, 32) for B in (1, 3) for g, w in GRID_WIN]


@pytest.mark.parametrize("Lat,B,grid,win", WIN_CASES,
                         ids=[f"{_impl(l, g)}-L{l}-B{b}-{'x'.join(map(str, g))}-{'x'.join(map(str, w)) if w else 'DHWnone'}" for l, b, g, w in WIN_CASES])
def test_window_attention(dev, Lat, B, grid, win):
    """win=None: the engine's DHW=None window, 2g+1 per axis -- every key of the grid."""
    if win is None:
        win = tuple(2 * n + 1 for n in grid)
    N = grid[0] * grid[1] * grid[2]
    scale = (32 * Lat) ** -0.5
    qkv = _r32(_rand((B, N, 3 * Lat), 501 + Lat, 6.0)).requires_grad_(True)
    dctx = _r32(_rand((B, N, Lat), 502, 1.0))
    ctx, lse, delta, dq = _win_run(dev, qkv.detach(), dctx, B, grid, win, Lat, scale)
    c_ref, l_ref, d_ref = _win_ref(qkv, dctx, grid, win, scale)
    _close(ctx, c_ref, 3e-5, "ctx")
    _close(lse, l_ref, 2e-5, "lse")
    _close(delta, d_ref, 5e-5, "delta")
    _close(dq, qkv.grad, 5e-5, "dqkv")
    if win == (1, 1, 1):
        # one key per query, itself: p = exp(s - lse) = 1 exactly, so ctx = v bit for bit
        v = qkv.detach()[..., 2 * Lat:]
        assert torch.equal(ctx, v), "window (1,1,1): ctx != v"
        dqk = dq[..., :2 * Lat]
        if _impl(Lat, grid) == "rows":
            assert int(dqk.count_nonzero()) == 0, "window (1,1,1): dq / dk not exactly 0"
        else:
            # the MFMA kernel sums dctx . v on the matrix cores and delta = dctx . ctx on the VALU: two orders of the same Lat products,
            # so dp - delta is a rounding residue (|.| <= Lat ulp of |dctx| |v|), not an exact 0
            bound = Lat * 2.0 ** -23 * dctx.abs().max().item() * v.abs().max().item() * scale * v.abs().max().item() * Lat
            assert dqk.abs().max().item() <= bound, f"window (1,1,1): |dq|,|dk| {dqk.abs().max().item():.3e} > {bound:.3e}"


def test_window_attention_long_axis(dev):
    """L = 20 on a grid side > 1023: the row-per-wave kernel at the product width, against float64 and against the MFMA kernel on the
    same tokens (the grid cut to 1023 along w; queries / keys whose windows the cut does not reach)."""
    Lat, B, grid, win = 20, 1, (1, 2, 1030), (3, 4, 6)
    N = 2 * 1030
    scale = 768 ** -0.5
    qkv = _r32(_rand((B, N, 3 * Lat), 511, 6.0)).requires_grad_(True)
    dctx = _r32(_rand((B, N, Lat), 512, 1.0))
    ctx, lse, delta, dq = _win_run(dev, qkv.detach(), dctx, B, grid, win, Lat, scale)
    c_ref, l_ref, d_ref = _win_ref(qkv, dctx, grid, win, scale)
    _close(ctx, c_ref, 3e-5, "ctx")
    _close(lse, l_ref, 2e-5, "lse")
    _close(delta, d_ref, 5e-5, "delta")
    _close(dq, qkv.grad, 5e-5, "dqkv")
    cut = (1, 2, 1023)
    sub = lambda t: t.view(B, 2, 1030, -1)[:, :, :1023].reshape(B, 2 * 1023, -1)
    c2, l2, d2, q2 = _win_run(dev, sub(qkv.detach()), sub(dctx), B, cut, win, Lat, scale)
    keep = lambda t: t.view(B, 2, 1023, -1)[:, :, :1015]
    full = lambda t: t.view(B, 2, 1030, -1)[:, :, :1015]
    _close(keep(c2), full(ctx), 3e-5, "mfma vs rows ctx")
    _close(keep(l2.unsqueeze(-1)), full(lse.unsqueeze(-1)), 2e-5, "mfma vs rows lse")
    _close(keep(d2.unsqueeze(-1)), full(delta.unsqueeze(-1)), 5e-5, "mfma vs rows delta")
    _close(keep(q2), full(dq), 5e-5, "mfma vs rows dqkv")


@pytest.mark.parametrize("Lat", [20, 16], ids=["mfma-L20", "rows-L16"])
@pytest.mark.parametrize("word", [None, 987654321], ids=["seed", "seed_ptr"])
def test_window_attention_dropout(dev, Lat, word):
    """attn_drop = 0.2 on the probabilities, mask index (b*N + i)*N + j (tests/dropmask.window_attn_mask); with seed_ptr the device word
    is added to the seed at run time."""
    B, grid, win = 2, (10, 10, 10), (3, 6, 6)
    N = 1000
    scale = (32 * Lat) ** -0.5
    seed = 424242
    qkv = _r32(_rand((B, N, 3 * Lat), 521, 6.0)).requires_grad_(True)
    dctx = _r32(_rand((B, N, Lat), 522, 1.0))
    ctx, lse, delta, dq = _win_run(dev, qkv.detach(), dctx, B, grid, win, Lat, scale, drop_p=0.2, seed=seed,
                                   seed_ptr=None if word is None else _seed_word(dev, word))
    mk = torch.from_numpy(dropmask.window_attn_mask(seed + (word or 0), B, N, 0.2)).double()
    c_ref, l_ref, d_ref = _win_ref(qkv, dctx, grid, win, scale, mask_p=mk)
    _close(ctx, c_ref, 3e-5, "ctx")
    _close(lse, l_ref, 2e-5, "lse")
    _close(delta, d_ref, 5e-5, "delta")
    _close(dq, qkv.grad, 5e-5, "dqkv")


# ------------------------------------------------------------------------------------------------------------------------------ GPA core

@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("N", [67, 130, 1000])
@pytest.mark.parametrize("P", [1, 64])
@pytest.mark.parametrize("Lat", [4, 8, 16, 32])
def test_gpa_core(dev, Lat, P, N, B):
    """gpa_{fwd,bwd}_kernel<L>: the checks of test_gpa_core_fwd_bwd (T = P + 1 + N > 2P + 2 in every case)."""
    gpa_core_check(dev, B, P, N, Lat)


def test_gpa_rejects(dev):
    from gaviko_amd import ops
    f = _f(dev)
    Lat, B = 16, 2
    for P, N, match in ((65, 200, r"need 0 < P <= 64 \(P=65\)"), (8, 9, r"T=18 leaves no global image tokens"),
                        (1, 1, r"T=3 leaves no global image tokens")):      # T = 2P + 2: the last T the guard must refuse
        T = P + 1 + N
        xl, ll = f(_rand((B * T, Lat), 601)), f(_rand((B * N, Lat), 602))
        with pytest.raises(ops.L.GavikoHipError, match=match):
            ops.gpa_fwd(xl=xl, ll=ll, B=B, T=T, N=N, P=P, L=Lat, scale=Lat ** -0.5)
        with pytest.raises(ops.L.GavikoHipError, match=match):
            ops.gpa_bwd(xl=xl, ll=ll, B=B, T=T, N=N, P=P, L=Lat, scale=Lat ** -0.5)
