"""-m gpu: the PEFT, split-bf16 and auxiliary kernels, each against a plain float64 reference of the same operation on the CPU.

Inputs are seeded; bf16 operands are rounded on the host first, so the reference multiplies exactly what the kernel does.  Outputs
are pre-filled with a sentinel and the test asserts that nothing outside the logical region was written.  Tolerances follow from the
arithmetic, never from a measured error:
  - data movement: bit-exact;
  - one fp32 operation per element: bit-exact against the same fp32 operation on the host (or 1 ulp where the kernel may fuse);
  - fp32 reductions over n terms: RED * sqrt(n) * sum |terms|, RED = 4e-7 (a few units of 2^-24 times the random-walk growth);
  - bf16 stores: 2^-8 of the value (round to nearest, 8 significant bits).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

RED = 4e-7
SENT = 7.0          # sentinel of the regions a kernel must not write
LOG2E = 1.4426950408889634


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _bf16_round(x):
    return x.to(torch.bfloat16).float()


def _hilo(x):
    """Split-bf16 form of an fp32 tensor: hi = bf16(x), lo = bf16(x - hi) (the subtraction is exact in fp32)."""
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def _within(got, ref, tol, what):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements outside the bound; first at flat index {i}: "
                             f"got {got.flatten()[i].item():.9g}, want {ref.flatten()[i].item():.9g}, bound {tol.flatten()[i].item():.3g}; "
                             f"max err/bound {(err / tol.clamp_min(1e-300)).max().item():.3g}")


def _ulp(x):
    """1 ulp of fp32 at |x| (as float64)."""
    x = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 23)


# ---------------------------------------------------------------------------------------------------------------------
# split-bf16 fused up-projection (engine: GPA proj_up riding the fc2 GEMM as 3L + 2 extra K columns)
def _gpa_params(Lat, P, seed):
    names = {"ca0_g": (Lat,), "ca0_b": (Lat,), "ca1_w": (64, Lat), "ca1_b": (64,), "ca3_w": (P, 64), "ca3_b": (P,),
             "gl0_g": (Lat,), "gl0_b": (Lat,), "gl1_w": (1, Lat), "gl1_b": (1,),
             "wgq": (Lat, Lat), "bgq": (Lat,), "wlq": (Lat, Lat), "blq": (Lat,)}
    out = {}
    for i, (k, shp) in enumerate(names.items()):
        t = _rand(shp, seed + i, 0.6)
        out[k] = 1 + 0.3 * t if k in ("ca0_g", "gl0_g") else t
    return out


@pytest.mark.parametrize("C,Lt,B,T,P", [(192, 20, 1, 1033, 8), (768, 16, 3, 701, 32), (1024, 20, 3, 701, 8)])
def test_split_bf16_fused_up_projection(dev, C, Lt, B, T, P):
    """W' = [W_fc2 | Wup_hi | Wup_hi | Wup_lo | b_hi | b_lo] (gvk_pack_split_bf16, weight side) against A' = [act | lat_hi | lat_lo | lat_hi | 1 | 1]
    whose latent columns the real writers fill: gvk_layernorm_fwd_proj (y_split) on every row, gvk_gpa_fwd (enh16) on the prompt rows.
    Then the fc2 GEMM with the engine's epilogue: x + act . W_fc2^T + b + lat' . Wup^T + b_up in one launch (engine.py _fuse_up)."""
    from gaviko_amd import ops
    assert 3 * Lt + 2 <= 64
    M, mlp, N = B * T, 4 * C, T - P - 1
    ld, c0 = mlp + 64, mlp
    Mp = ops.pad_rows(M)
    sl_lat, sl_b, sl_end = slice(c0, c0 + 3 * Lt), slice(c0 + 3 * Lt, c0 + 3 * Lt + 2), c0 + 3 * Lt + 2
    # ---- weight side
    wup = _rand((C, Lt), 1, 1 / math.sqrt(Lt))
    bup = _rand((C,), 2, 0.1)
    wfc2 = _bf16_round(_rand((C, mlp), 3, 1 / math.sqrt(mlp)))
    bfc2 = _rand((C,), 4, 0.1)
    W = torch.full((C, ld), SENT, dtype=torch.bfloat16)
    W[:, :mlp] = wfc2.bfloat16()
    Wd = W.to(dev)
    ops.pack_split_bf16(wup.to(dev), Wd, c0, C, b=bup.to(dev), weight_side=True)
    got = Wd.cpu()
    hi, lo = _hilo(wup)
    bhi, blo = _hilo(bup)
    assert torch.equal(got[:, c0: c0 + Lt], hi) and torch.equal(got[:, c0 + Lt: c0 + 2 * Lt], hi), "weight side: w_hi columns"
    assert torch.equal(got[:, c0 + 2 * Lt: c0 + 3 * Lt], lo), "weight side: w_lo columns"
    assert torch.equal(got[:, c0 + 3 * Lt], bhi) and torch.equal(got[:, c0 + 3 * Lt + 1], blo), "weight side: bias columns"
    assert torch.equal(got[:, :mlp], W[:, :mlp]) and (got[:, sl_end:] == SENT).all(), "weight side wrote outside its 3L + 2 columns"
    Wd[:, sl_end:] = 0                                       # (the engine's operand carries zeros there)
    # ---- activation side: [act | slot | 1 | 1 | 0...], the slot pre-filled with a sentinel on every row (rows >= M must keep it)
    A = torch.zeros((Mp, ld), dtype=torch.bfloat16)
    A[:, sl_lat] = SENT
    A[:, sl_b] = 1.0
    Ad = A.to(dev)
    x = _rand((M, C), 5, 2.0)
    gamma, beta = 1 + _rand((C,), 6, 0.2), _rand((C,), 7, 0.2)
    wdown, bdown = _rand((Lt, C), 8, 1 / math.sqrt(C)), _rand((Lt,), 9, 0.1)
    lat, zz = torch.zeros((M, Lt), device=dev), torch.zeros((M, Lt), device=dev)
    ops.layernorm_fwd_proj(x.to(dev), gamma.to(dev), beta.to(dev), M, C, y16=ops.act_zeros(M, C, torch.bfloat16, dev),
                           mean=torch.zeros(M, device=dev), rstd=torch.zeros(M, device=dev), w=wdown.to(dev), bias=bdown.to(dev), z=zz, y=lat,
                           L_=Lt, w_layout=0, act=1, y_split=Ad, col_split=c0)
    latc = lat.cpu()
    hi, lo = _hilo(latc)
    got = Ad.cpu()
    assert torch.equal(got[:M, sl_lat], torch.cat([hi, lo, hi], 1)), "layernorm_fwd_proj y_split != [hi | lo | hi] of its own y"
    # ---- GPA forward writes the prompt rows' split copy of enh
    ll = _rand((B * N, Lt), 10, 1.0)
    z = lambda *s: torch.zeros(s, device=dev)
    bufs = dict(imp=z(B, P), gw=z(B), enh=z(B, P, Lt), prm=z(B, P, Lt), qg=z(B, P, Lt), ql=z(B, P, Lt), cg=z(B, P, Lt), cl=z(B, P, Lt),
                lse_g=z(B, P), lse_l=z(B, P))
    prm = {k: v.to(dev) for k, v in _gpa_params(Lt, P, 200).items()}
    ops.gpa_fwd(xl=lat, ll=ll.to(dev), B=B, T=T, N=N, P=P, L=Lt, scale=Lt ** -0.5, enh16=Ad, ld16=ld, col16=c0, **prm, **bufs)
    enh = bufs["enh"].cpu()
    lat_eff = latc.clone().view(B, T, Lt)
    lat_eff[:, :P] = enh
    lat_eff = lat_eff.reshape(M, Lt)
    hi, lo = _hilo(lat_eff)
    got = Ad.cpu()
    assert torch.equal(got[:M, sl_lat], torch.cat([hi, lo, hi], 1)), "prompt rows: gpa_fwd enh16 != [hi | lo | hi] of its own enh"
    assert (got[M:, sl_lat] == SENT).all(), "a split writer stored rows >= M"
    assert (got[:, :mlp] == 0).all() and (got[:, sl_end:] == 0).all(), "a split writer stored outside its 3L columns"
    assert (got[:, sl_b] == 1).all(), "the two constant-1 bias columns were overwritten"
    Ad[M:, sl_lat] = 0
    # ---- the fc2 GEMM (EPI_BIAS_RES_F32 over K = mlp + 64, as the engine launches it)
    res = _rand((M, C), 11, 1.0)
    R = torch.zeros((Mp, C))
    R[:M] = res
    up = lat_eff.double() @ wup.double().T + bup.double()
    absup = lat_eff.double().abs() @ wup.double().abs().T + bup.double().abs()
    for dense in (False, True):
        if dense:
            act = _bf16_round(_rand((M, mlp), 12, 1.0))
            Ad[:M, :mlp] = act.bfloat16().to(dev)
        out = torch.full((Mp, C), SENT, device=dev)
        ops.gemm_nt(Ad, Wd, M, out, epilogue=ops.EPI_BIAS_RES_F32, bias=bfc2.to(dev), res=R.to(dev), K=ld)
        ref = up + bfc2.double() + res.double()
        # split-bf16 product: the dropped lo.lo term and the residuals of the two splits are each <= 2^-18 of |a||w|, the fp32 sum of
        # 3L + 2 exact products adds ~(3L + 2) 2^-24: about 2^-15 of sum |lat||w| in all; then the fp32 adds of bias and residual
        tol = 2.0 ** -15 * absup + 2.0 ** -22 * (res.double().abs() + bfc2.double().abs() + ref.abs())
        if dense:
            ref = ref + act.double() @ wfc2.double().T
            tol = tol + RED * math.sqrt(ld) * (act.double().abs() @ wfc2.double().abs().T)
        _within(out[:M], ref, tol, f"fc2 + split-bf16 up-projection (dense part {'random' if dense else 'zero'})")
        assert (out[M:] == SENT).all(), "fc2 GEMM stored rows >= M"


# ---------------------------------------------------------------------------------------------------------------------
# prompt-row fix: x[b*T + p] += (enh[b][p] - lat[b*T + p]) . Wup^T  (then LayerNorm, for the fused form)
def _fix_ref(x, enh, lat, wup, B, T, P):
    """float64 fixed rows and the |terms| bound of their dot products."""
    d = (enh.double() - lat.double().view(B, T, -1)[:, :P])                       # [B, P, L]
    xf = x.double().clone().view(B, T, -1)
    xf[:, :P] += d @ wup.double().T
    absd = d.abs() @ wup.double().abs().T
    return xf.view(B * T, -1), absd


@pytest.mark.parametrize("B,T,P,C", [(3, 64, 8, 192), (2, 67, 32, 768), (1, 130, 32, 1024)])
def test_prompt_fix_and_layernorm_fwd_fix(dev, B, T, P, C):
    """gvk_prompt_up_fix and gvk_layernorm_fwd_fix (4-row blocks: T = 64 is a multiple of the block, 67 and 130 are not)."""
    from gaviko_amd import ops
    Lt, M = 20, B * T
    x = _rand((M, C), 21, 2.0)
    enh, lat = _rand((B, P, Lt), 22, 1.0), _rand((M, Lt), 23, 1.0)
    wup = _rand((C, Lt), 24, 1 / math.sqrt(Lt))
    gamma, beta = 1 + _rand((C,), 25, 0.3), _rand((C,), 26, 0.3)
    xf, absd = _fix_ref(x, enh, lat, wup, B, T, P)
    prm = (lambda t: t.view(B, T, -1)[:, :P].reshape(B * P, -1))
    # fixed rows: fp32 sum of L products, then one fp32 add onto x
    tol_fix = RED * math.sqrt(Lt) * absd.reshape(B * P, C) + 2.0 ** -24 * prm(xf).abs()
    # ---- gvk_prompt_up_fix
    out = x.to(dev)
    ops.prompt_up_fix(enh.to(dev), lat.to(dev), wup.to(dev), out, B, T, P, C, Lt)
    got = out.cpu()
    _within(prm(got), prm(xf), tol_fix, "prompt_up_fix: prompt rows")
    keep = torch.ones(B, T, dtype=torch.bool)
    keep[:, :P] = False
    keep = keep.flatten()
    assert torch.equal(got[keep], x[keep]), "prompt_up_fix touched a non-prompt row"
    # ---- gvk_layernorm_fwd_fix: the same fix written back in place, then LayerNorm of every row
    xd = x.to(dev)
    y16 = torch.full((ops.pad_rows(M), C), SENT, dtype=torch.bfloat16, device=dev)
    mean, rstd = torch.full((M + 4,), SENT, device=dev), torch.full((M + 4,), SENT, device=dev)
    ops.layernorm_fwd_fix(xd, gamma.to(dev), beta.to(dev), M, C, y16=y16, mean=mean, rstd=rstd, enh=enh.to(dev), lat=lat.to(dev), wup=wup.to(dev),
                          T=T, P=P, L_=Lt)
    got = xd.cpu()
    _within(prm(got), prm(xf), tol_fix, "layernorm_fwd_fix: fixed rows written back")
    assert torch.equal(got[keep], x[keep]), "layernorm_fwd_fix changed a non-prompt row of x"
    mu = xf.mean(1)
    var = xf.var(1, unbiased=False)
    rs = (var + 1e-5).rsqrt()
    yref = (xf - mu[:, None]) * rs[:, None] * gamma.double() + beta.double()
    # statistics: fp32 sums over C terms (relative to the row's second moment); y: the bf16 store plus that error carried by gamma
    m2 = (xf * xf).mean(1)
    e_mean = RED * math.sqrt(C) * xf.abs().mean(1)
    _within(mean[:M], mu, e_mean, "layernorm_fwd_fix: mean")
    rel = 2 * RED * math.sqrt(C) * m2 / var
    _within(rstd[:M], rs, rel * rs, "layernorm_fwd_fix: rstd")
    xh = ((xf - mu[:, None]) * rs[:, None]).abs()
    _within(y16[:M], yref, 2.0 ** -8 * yref.abs() + gamma.double().abs() * (rel[:, None] * xh + (e_mean * rs)[:, None]), "layernorm_fwd_fix: y")
    assert (y16[M:] == SENT).all() and (mean[M:] == SENT).all() and (rstd[M:] == SENT).all(), "layernorm_fwd_fix wrote past row M"


# ---------------------------------------------------------------------------------------------------------------------
# SSF
@pytest.mark.parametrize("N,K", [(5, 192), (200, 72), (64, 64)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_ssf_fold_weight(dev, N, K, dt):
    """out[n][k] = w[n][k] * s[n] (one fp32 multiply, then the store's rounding) and its transpose, N and K not multiples of the 64 tile."""
    from gaviko_amd import ops
    w, s = _rand((N, K), 31, 1.0), 0.3 + 1.7 * torch.rand(N, generator=torch.Generator().manual_seed(32))
    out = torch.full((N * K + 64,), SENT, dtype=dt, device=dev)
    out_t = torch.full((N * K + 64,), SENT, dtype=dt, device=dev)
    ops.ssf_fold_weight(w.to(dev), s.to(dev), out, out_t)
    want = (w * s[:, None]).to(dt)
    assert torch.equal(out[: N * K].cpu().view(N, K), want)
    assert torch.equal(out_t[: N * K].cpu().view(K, N), want.T)
    assert (out[N * K:] == SENT).all() and (out_t[N * K:] == SENT).all()
    out2 = torch.full((N * K + 64,), SENT, dtype=dt, device=dev)
    ops.ssf_fold_weight(w.to(dev), s.to(dev), out2)          # out_t = NULL
    assert torch.equal(out2[: N * K].cpu().view(N, K), want) and (out2[N * K:] == SENT).all()


def test_ssf_fold_vec_and_ln_grad(dev):
    from gaviko_amd import ops
    n = 1000
    g = torch.Generator().manual_seed(41)
    a, t = torch.randn(n, generator=g), torch.randn(n, generator=g)
    s = 0.3 + 1.7 * torch.rand(n, generator=g)
    for aa, tt in ((a, t), (None, t), (a, None)):
        out = torch.full((n + 8,), SENT, device=dev)
        ops.ssf_fold_vec(None if aa is None else aa.to(dev), s.to(dev), None if tt is None else tt.to(dev), out)
        if aa is not None and tt is not None:
            # a*s + t: two roundings, or one when fused: <= 1 ulp of |a s| plus 1 ulp of the result
            ref = aa.double() * s.double() + tt.double()
            _within(out[:n], ref, _ulp(aa.double() * s.double()) + _ulp(ref), "ssf_fold_vec")
        elif tt is None:
            assert torch.equal(out[:n].cpu(), aa * s), "t = NULL: one fp32 multiply"
        else:
            assert torch.equal(out[:n].cpu(), tt), "a = NULL: out = t"
        assert (out[n:] == SENT).all()
    # ssf_ln_grad: ds = gamma*dgamma' + beta*dbeta', dt = dbeta'
    dgp, dbp, gam, bet = (torch.randn(n, generator=g) for _ in range(4))
    ds, dt = torch.full((n + 8,), SENT, device=dev), torch.full((n + 8,), SENT, device=dev)
    ops.ssf_ln_grad(dgp.to(dev), dbp.to(dev), gam.to(dev), bet.to(dev), ds, dt)
    ref = gam.double() * dgp.double() + bet.double() * dbp.double()
    _within(ds[:n], ref, _ulp((gam * dgp).abs()) + _ulp((bet * dbp).abs()) + _ulp(ref), "ssf_ln_grad ds")
    assert torch.equal(dt[:n].cpu(), dbp) and (ds[n:] == SENT).all() and (dt[n:] == SENT).all()


SSF_CASES = {
    # name: M, N, dy dtype, y0 dtype, extra.  The kernel cuts M into 64 slabs of ceil(M / 64) rows: at M = 1020, 2048 and 256 the last slab
    # holds rows (63 ceil(M / 64) < M), at 1033, 500, 40 and 7 it is empty
    "bf16": (1020, 768, torch.bfloat16, torch.bfloat16, {}),
    "bf16_ragged": (1033, 192, torch.bfloat16, torch.bfloat16, {}),
    "f32_full_slabs": (2048, 192, torch.float32, torch.float32, {}),
    "f32_y1_dropout": (500, 200, torch.float32, torch.float32, dict(y1=True, y_mul=0.9, ld=208)),
    "rows_pos": (256, 192, torch.float32, torch.float32, dict(rows=(64, 67, 2), pos=True)),
    "rows_pos_small": (40, 200, torch.bfloat16, torch.float32, dict(rows=(20, 25, 3), pos=True, y1=True)),
    "q_prescaled": (300, 576, torch.bfloat16, torch.bfloat16, dict(y0_cols=192, y0_mul=1 / (0.125 * LOG2E), ld=584)),
    "tiny": (7, 64, torch.float32, torch.bfloat16, {}),
}


@pytest.mark.parametrize("case", list(SSF_CASES))
def test_ssf_colgrad(dev, case):
    """dt[n] = sum_m dy[m][n],  ds[n] = sum_m dy[m][n] (y[m][n] - t[n]) / s[n],  y = y_mul (y0 [* y0_mul on the q block] - y1) - pos[m % rows_in],
    with a trained-looking s in [0.3, 2] and |t| ~ 1.  64 row slabs: M below 64, M not a multiple of 64, and the row mapping."""
    from gaviko_amd import ops
    M, N, dyt, y0t, ex = SSF_CASES[case]
    ld = ex.get("ld", N)
    g = torch.Generator().manual_seed(190 + list(SSF_CASES).index(case))
    if "rows" in ex:
        rin, rout, roff = ex["rows"]
        Bs = M // rin
        rows = torch.tensor([(m // rin) * rout + roff + m % rin for m in range(M)])
        nbuf = Bs * rout
    else:
        rin = rout = roff = 0
        rows = torch.arange(M)
        nbuf = M
    dy = torch.randn(nbuf, ld, generator=g).to(dyt).float()
    y0 = (torch.randn(nbuf, ld, generator=g) * 2).to(y0t).float()
    y1 = torch.randn(nbuf, ld, generator=g) if ex.get("y1") else None
    pos = torch.randn(rin, N, generator=g) if ex.get("pos") else None
    s = 0.3 + 1.7 * torch.rand(N, generator=g)
    t = torch.randn(N, generator=g)
    y_mul, y0_cols, y0_mul = ex.get("y_mul", 1.0), ex.get("y0_cols", 0), ex.get("y0_mul", 1.0)
    # float64 reference over the logical rows
    dyl, y = dy[rows, :N].double(), y0[rows, :N].double()
    y[:, :y0_cols] *= y0_mul
    if y1 is not None:
        y = y - y1[rows, :N].double()
    y = y * y_mul
    if pos is not None:
        y = y - pos.double()[torch.arange(M) % rin]
    dt_ref = dyl.sum(0)
    ds_ref = (dyl * (y - t.double())).sum(0) / s.double()
    ds_o, dt_o = torch.full((N + 8,), SENT, device=dev), torch.full((N + 8,), SENT, device=dev)
    scratch = torch.zeros(64 * 2 * N, device=dev)
    ops.ssf_colgrad(dy.to(dyt).to(dev), y0.to(y0t).to(dev), s.to(dev), t.to(dev), ds_o, dt_o, scratch, M, N, y1=None if y1 is None else y1.to(dev),
                    pos=None if pos is None else pos.contiguous().to(dev), ld_dy=ld, ld_y=ld, rows_in=rin, rows_out=rout, row_off=roff,
                    y0_cols=y0_cols, y0_mul=y0_mul, y_mul=y_mul)
    # kernel: (sum dy*y - t sum dy) / s with both sums in fp32 over M rows (each y itself a few fp32 roundings)
    _within(dt_o[:N], dt_ref, RED * math.sqrt(M) * dyl.abs().sum(0) + 1e-30, f"{case}: dt")
    tol = (RED * math.sqrt(M) * ((dyl * y).abs().sum(0) + t.double().abs() * dyl.abs().sum(0)) + 2.0 ** -23 * (dyl * y).abs().sum(0)) / s.double()
    _within(ds_o[:N], ds_ref, tol + _ulp(ds_ref), f"{case}: ds")
    assert (ds_o[N:] == SENT).all() and (dt_o[N:] == SENT).all()


@pytest.mark.parametrize("B,C,pool", [(1, 192, "cls"), (3, 192, "mean"), (3, 1024, "cls"), (1, 1024, "mean")])
def test_ssf_head_grad(dev, B, C, pool):
    """Final norm + ssf in front of the head: only the pooled rows r0 .. r0+R carry gradient (R = 1: cls pooling; R = T - 1: mean pooling
    over the patch rows, the bitfit / fft form with pool='mean').  Against float64 autograd of  logits = mean_r(xhat*gamma' + beta') . Wh^T."""
    from gaviko_amd import ops
    T, K = 65, 5
    r0, R = (0, 1) if pool == "cls" else (1, T - 1)
    gx = _rand((B * T, C), 51, 2.0) + 0.5
    mean = gx.mean(1)
    rstd = (gx.var(1, unbiased=False) + 1e-5).rsqrt()
    wh, dl = _rand((K, C), 52, 0.1), _rand((B, K), 53, 1.0)
    g = torch.Generator().manual_seed(54)
    gamma, beta = 1 + 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
    s = (0.3 + 1.7 * torch.rand(C, generator=g)).double().requires_grad_(True)
    tt = torch.randn(C, generator=g).double().requires_grad_(True)
    xh = ((gx.double() - mean.double()[:, None]) * rstd.double()[:, None]).view(B, T, C)
    yn = xh * (gamma.double() * s) + (beta.double() * s + tt)
    logits = yn[:, r0: r0 + R].mean(1) @ wh.double().T
    logits.backward(dl.double())
    ds, dt = torch.full((C + 8,), SENT, device=dev), torch.full((C + 8,), SENT, device=dev)
    ops.ssf_head_grad(gx.to(dev), mean.to(dev), rstd.to(dev), wh.to(dev), dl.to(dev), gamma.to(dev), beta.to(dev), ds, dt, B, T, C, K, r0, R)
    # fp32 sums: K terms for dpn, then B*R terms per column; |terms| from the absolute values of the same products
    adpn = (dl.double().abs() @ wh.double().abs()) / R                                  # [B, C]
    sg = (adpn[:, None, :] * xh[:, r0: r0 + R].abs()).sum((0, 1))
    sb = R * adpn.sum(0)
    n = K + B * R
    _within(dt[:C], tt.grad, RED * math.sqrt(n) * sb, "ssf_head_grad dt")
    _within(ds[:C], s.grad, RED * math.sqrt(n) * (gamma.double().abs() * sg + beta.double().abs() * sb) + _ulp(s.grad), "ssf_head_grad ds")
    assert (ds[C:] == SENT).all() and (dt[C:] == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------
# DVPT
@pytest.mark.parametrize("B,P,Np", [(1, 1, 300), (3, 8, 600), (3, 50, 700)])
def test_dvpt_fwd_bwd(dev, B, P, Np):
    """Prompt latents (scaled by `scale`) attend to the patch latents (keys = values); lat' = [enh | cls | patches]; the step's output adds
    gate * (lat' . W_u^T + b_u).  Given dcomb = dy . W_u and colsum_dy: dgate = <dcomb, lat'> + <b_u, colsum_dy>, dz = d<gate dcomb, lat'>/dz."""
    from gaviko_amd import ops
    Lt, C = 20, 192
    T = P + 1 + Np
    assert (T - P) % 256 != 0
    scale = C ** -0.5
    z = _rand((B, T, Lt), 61, 3.0).double().requires_grad_(True)
    q = z[:, :P] * scale
    kv = z[:, P + 1:]
    sc = q @ kv.transpose(1, 2)
    lse_ref = torch.logsumexp(sc, -1)
    enh_ref = sc.softmax(-1) @ kv
    latp = torch.cat([enh_ref, z[:, P:]], 1)
    dcomb, bu, cs = _rand((B, T, Lt), 62, 1.0), _rand((C,), 63, 0.2), _rand((C,), 64, 5.0)
    gate = torch.tensor([0.37])
    (latp * (gate.double() * dcomb.double())).sum().backward()
    dgate_ref = (dcomb.double() * latp.detach()).sum() + (bu.double() * cs.double()).sum()
    f = lambda t: t.float().contiguous().to(dev)
    zd = f(z.detach().reshape(B * T, Lt))
    enh, lse = torch.full((B, P, Lt), SENT, device=dev), torch.full((B, P), SENT, device=dev)
    ops.dvpt_fwd(z=zd, enh=enh, lse=lse, B=B, T=T, P=P, L=Lt, C=C, scale=scale)
    # softmax over Np keys in fp32: the sums (RED sqrt(Np)) plus __expf of a rounded argument (|s| 2^-23 relative, |s| <~ 10 here)
    smax = sc.detach().abs().max().item()
    rel = RED * math.sqrt(Np) + 4 * smax * 2.0 ** -23
    _within(lse, lse_ref.detach(), rel * (smax + math.log(Np)), "dvpt lse")
    _within(enh, enh_ref.detach(), rel * kv.detach().abs().max().item(), "dvpt enh")
    bw = dict(dcomb=f(dcomb.reshape(B * T, Lt)), gate=f(gate), bu=f(bu), colsum_dy=f(cs), delta=torch.zeros(B, P, device=dev),
              dz=torch.full((B * T, Lt), SENT, device=dev), dgate=torch.full((1,), SENT, device=dev))
    ops.dvpt_bwd(z=zd, enh=enh, lse=lse, B=B, T=T, P=P, L=Lt, C=C, scale=scale, **bw)
    # backward: the same softmax error carried through two more sums over the keys (dq) and over the P prompts (dk, dv)
    rel_b = 4 * (rel + RED * math.sqrt(P))
    _within(bw["dz"].view(B, T, Lt), z.grad, rel_b * z.grad.abs().max().item(), "dvpt dz")
    absg = (dcomb.double().abs() * latp.detach().abs()).sum() + (bu.double() * cs.double()).abs().sum()
    _within(bw["dgate"], dgate_ref.view(1), RED * math.sqrt(B * T * Lt + C) * absg + rel * absg, "dvpt dgate")
    dg1 = bw["dgate"].clone()
    ops.dvpt_bwd(z=zd, enh=enh, lse=lse, B=B, T=T, P=P, L=Lt, C=C, scale=scale, **bw)
    assert torch.equal(bw["dgate"], dg1), "dgate is one workgroup: two launches must agree bit for bit"
    # scale_dev_: x *= alpha[0] (one fp32 multiply)
    x = _rand((1000,), 65, 3.0)
    xd = x.to(dev)
    ops.scale_dev_(xd[:997], bw["dgate"])
    assert torch.equal(xd[:997].cpu(), x[:997] * dg1.cpu()) and torch.equal(xd[997:].cpu(), x[997:])


def test_scale_and_seed_advance(dev):
    from gaviko_amd import ops
    x = _rand((1001,), 66, 3.0)
    xd = x.to(dev)
    ops.scale_(xd[:999], 0.7)
    assert torch.equal(xd[:999].cpu(), x[:999] * torch.tensor(0.7)) and torch.equal(xd[999:].cpu(), x[999:])
    seed = torch.tensor([2 ** 62 + 5, 11], dtype=torch.int64, device=dev)
    ops.seed_advance(seed[:1], 7919)
    ops.seed_advance(seed[:1], 2 ** 62)
    assert seed.cpu().tolist() == [2 ** 62 + 5 + 7919 + 2 ** 62 - 2 ** 64, 11], "uint64 epoch += inc (wrapping), the next word untouched"


# ---------------------------------------------------------------------------------------------------------------------
# EVP and its glue
@pytest.mark.parametrize("H,W", [(160, 100), (100, 160), (37, 37)])
def test_evp_highpass(dev, H, W):
    """out[b,d] = |Hp . X[b,d]| on the depth slices the mask selects, |X[b,d]| elsewhere."""
    from gaviko_amd import ops
    B, D = 2, 5
    img = _rand((B, 1, D, H, W), 71, 1.0)
    hp = _rand((H, H), 72, 1 / math.sqrt(H))
    mask = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32)
    out = torch.full((B * D * H * W + 64,), SENT, device=dev)
    ops.evp_highpass(img.to(dev), hp.to(dev), mask.to(dev), out)
    got = out[: B * D * H * W].cpu().view(B, D, H, W)
    x = img[:, 0]
    for d in range(D):
        if mask[d]:
            ref = (hp.double() @ x[:, d].double()).abs()
            _within(got[:, d], ref, RED * math.sqrt(H) * (hp.double().abs() @ x[:, d].double().abs()), f"evp_highpass filtered slice {d}")
        else:
            assert torch.equal(got[:, d], x[:, d].abs()), f"evp_highpass pass-through slice {d}"
    assert (out[B * D * H * W:] == SENT).all()


def test_pad2d_and_add2d(dev):
    from gaviko_amd import ops
    rows, cols, ld_src = 37, 6, 10
    src = _rand((rows, ld_src), 81, 1.0)
    for transpose, drows, dcols, ld_dst in ((False, 40, 8, 12), (True, 8, 40, 44)):
        dst = torch.full((drows, ld_dst), SENT, device=dev)
        ops.pad2d(src.to(dev), rows, cols, dst, drows, dcols, ld_src=ld_src, ld_dst=ld_dst, transpose=transpose)
        want = torch.zeros(drows, dcols)
        s = src[:, :cols].T if transpose else src[:, :cols]
        want[: s.shape[0], : s.shape[1]] = s
        got = dst.cpu()
        assert torch.equal(got[:, :dcols], want), f"pad2d transpose={transpose}"
        assert (got[:, dcols:] == SENT).all(), f"pad2d transpose={transpose} wrote the padding columns"
    a, b = _rand((33, 70), 82, 3.0), _rand((33, 50), 83, 3.0)
    out = torch.full((33, 48), SENT, device=dev)
    ops.add2d(a.to(dev), 70, b.to(dev), 50, out, 48, 33, 45)
    got = out.cpu()
    assert torch.equal(got[:, :45], a[:, :45] + b[:, :45]) and (got[:, 45:] == SENT).all()


def test_gelu_fwd_bwd(dev):
    """Exact (erf) GELU and dy * GELU'(x) over [-10, 10], signed zeros and large |x|."""
    from gaviko_amd import ops
    x = torch.cat([torch.linspace(-10, 10, 20001), torch.tensor([0.0, -0.0, 1e4, -1e4, 1e30, -1e30, 3e38, -3e38])])
    n = x.numel()
    dy = _rand((n,), 91, 2.0)
    y = torch.full((n + 8,), SENT, device=dev)
    dx = torch.full((n + 8,), SENT, device=dev)
    ops.gelu_fwd(x.to(dev), y[:n])
    ops.gelu_bwd(dy.to(dev), x.to(dev), dx[:n])
    xd = x.double()
    cdf = 0.5 * (1 + torch.erf(xd / math.sqrt(2)))
    pdf = torch.exp(-0.5 * xd * xd) / math.sqrt(2 * math.pi)
    # fp32 erff / __expf: a few 2^-24 of 1 + erf (absolute), carried by 0.5 |x|; the exponential's rounded argument x^2/2 adds |x^2/2| 2^-23
    _within(y[:n], xd * cdf, 2.0 ** -21 * xd.abs() + _ulp(xd * cdf), "gelu_fwd")
    g = cdf + xd * pdf
    _within(dx[:n], dy.double() * g, dy.double().abs() * (2.0 ** -21 + (xd * pdf).abs() * (2.0 ** -21 + 0.5 * xd * xd * 2.0 ** -23)) + _ulp(dy.double() * g),
            "gelu_bwd")
    assert torch.equal(y[n - 8: n - 6].cpu(), torch.tensor([0.0, 0.0])) and (dx[n - 8: n - 6].cpu() == dy[n - 8: n - 6] * 0.5).all()
    assert (y[n:] == SENT).all() and (dx[n:] == SENT).all()


@pytest.mark.parametrize("row_off", [0, 1])
def test_rows_patch_and_gather(dev, row_off):
    """tok[b][row_off + n] (= or +=) src[b*N + n] (+ pos[n]): other rows untouched; rows_gather reads the same rows back."""
    from gaviko_amd import ops
    B, N, C = 3, 37, 196
    T = N + row_off + 2
    tok0 = _rand((B, T, C), 101, 1.0)
    src, pos = _rand((B * N, C), 102, 1.0), _rand((N, C), 103, 1.0)
    s3 = src.view(B, N, C)
    for use_pos, acc in ((False, False), (True, False), (True, True), (False, True)):
        tok = tok0.to(dev)
        ops.rows_patch(tok, src.to(dev), pos.to(dev) if use_pos else None, B, T, N, C, row_off, acc)
        want = tok0.clone()
        v = s3 + pos if use_pos else s3.clone()
        want[:, row_off: row_off + N] = v + tok0[:, row_off: row_off + N] if acc else v
        assert torch.equal(tok.cpu(), want), f"rows_patch pos={use_pos} accumulate={acc}"
    dst = torch.full((B * N + 3, C), SENT, device=dev)
    ops.rows_gather(tok0.to(dev), dst, B, T, N, C, row_off)
    assert torch.equal(dst[: B * N].cpu(), tok0[:, row_off: row_off + N].reshape(B * N, C)) and (dst[B * N:] == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------
# small linear, VPT repack, strided cast, LoRA merge
@pytest.mark.parametrize("R,K,C", [(8, 24, 200), (3, 50, 768)])
def test_small_linear(dev, R, K, C):
    from gaviko_amd import ops
    x, w, b = _rand((R, K), 111, 1.0), _rand((C, K), 112, 1 / math.sqrt(K)), _rand((C,), 113, 0.2)
    dout = _rand((R, C), 114, 1.0)
    xd, wd, dd = x.double(), w.double(), dout.double()
    for bias in (b, None):
        out = torch.full((R * C + 8,), SENT, device=dev)
        ops.small_linear_fwd(x.to(dev), w.to(dev), None if bias is None else bias.to(dev), out, R, K, C)
        ref = xd @ wd.T + (0 if bias is None else bias.double())
        tol = RED * math.sqrt(K + 1) * (xd.abs() @ wd.abs().T + (0 if bias is None else bias.double().abs()))
        _within(out[: R * C].view(R, C), ref, tol, f"small_linear_fwd bias={bias is not None}")
        assert (out[R * C:] == SENT).all()
    dw_ref, db_ref, dx_ref = dd.T @ xd, dd.sum(0), dd @ wd
    dw_tol = RED * math.sqrt(R) * (dd.abs().T @ xd.abs())
    db_tol = RED * math.sqrt(R) * dd.abs().sum(0)
    dx_tol = RED * math.sqrt(C) * (dd.abs() @ wd.abs())
    for acc in (False, True):
        for with_db in (True, False):
            p_dw, p_db, p_dx = _rand((C, K), 115, 1.0), _rand((C,), 116, 1.0), _rand((R, K), 117, 1.0)
            dw = torch.full((C * K + 8,), SENT, device=dev)
            db = torch.full((C + 8,), SENT, device=dev)
            dx = torch.full((R * K + 8,), SENT, device=dev)
            if acc:
                dw[: C * K] = p_dw.flatten().to(dev)
                dx[: R * K] = p_dx.flatten().to(dev)
                if with_db:
                    db[:C] = p_db.to(dev)
            ops.small_linear_bwd(x.to(dev), w.to(dev), dout.to(dev), dw, db if with_db else None, dx, R, K, C, accumulate=acc)
            base = (lambda p: p.double()) if acc else (lambda p: 0)
            ulp = (lambda p, r: _ulp(r) if acc else 0)
            _within(dw[: C * K].view(C, K), dw_ref + base(p_dw), dw_tol + ulp(p_dw, dw_ref + base(p_dw)), f"small_linear_bwd dw acc={acc}")
            _within(dx[: R * K].view(R, K), dx_ref + base(p_dx), dx_tol + ulp(p_dx, dx_ref + base(p_dx)), f"small_linear_bwd dx acc={acc}")
            if with_db:
                _within(db[:C], db_ref + base(p_db), db_tol + ulp(p_db, db_ref + base(p_db)), f"small_linear_bwd db acc={acc}")
            else:
                assert (db[:C] == SENT).all(), "db = NULL must not be written"
            assert (dw[C * K:] == SENT).all() and (db[C:] == SENT).all() and (dx[R * K:] == SENT).all()


@pytest.mark.parametrize("P,skip", [(4, 10), (6, 6), (10, 3)])
def test_vpt_repack_round_trip(dev, P, skip):
    """out = [in[:, 0] | prompt | in[:, 1 + skip:]]; the backward scatters back with rows 1 .. skip of din zero."""
    from gaviko_amd import ops
    B, Tin, C = 3, 40, 196
    Tout = Tin - skip + P
    inp, prompt = _rand((B, Tin, C), 121, 1.0), _rand((P, C), 122, 1.0)
    out = torch.full((B * Tout * C + 8,), SENT, device=dev)
    ops.vpt_repack_fwd(inp.to(dev), prompt.to(dev), out, B, Tin, Tout, P, skip, C)
    want = torch.cat([inp[:, :1], prompt.expand(B, P, C), inp[:, 1 + skip:]], 1)
    assert torch.equal(out[: B * Tout * C].cpu().view(B, Tout, C), want) and (out[B * Tout * C:] == SENT).all()
    din = torch.full((B * Tin * C + 8,), SENT, device=dev)
    ops.vpt_repack_bwd(out, din, B, Tin, Tout, P, skip, C)
    back = inp.clone()
    back[:, 1: 1 + skip] = 0
    assert torch.equal(din[: B * Tin * C].cpu().view(B, Tin, C), back) and (din[B * Tin * C:] == SENT).all()


def test_cast_bf16_f32_strided(dev):
    from gaviko_amd import ops
    M, ld, C, col0 = 1033, 200, 64, 68
    x = _rand((M, ld), 131, 3.0)
    for src in (x.bfloat16(), x):
        out = torch.full((M * C + 8,), SENT, device=dev)
        ops.cast_bf16_f32_strided(src.to(dev), out, M, C, ld, col0=col0)
        assert torch.equal(out[: M * C].cpu().view(M, C), src[:, col0: col0 + C].float()) and (out[M * C:] == SENT).all()


@pytest.mark.parametrize("C,r", [(192, 1), (192, 8), (1024, 4)])
def test_lora_merge(dev, C, r):
    """out [3C][C] = W + s [B_q A_q ; 0 ; B_v A_v] with a non-integer s; the k rows stay bit-identical to W."""
    from gaviko_amd import ops
    s = 0.7
    w = _rand((3 * C, C), 141, 0.05)
    aq, bq, av, bv = _rand((r, C), 142, 1.0), _rand((C, r), 143, 1.0), _rand((r, C), 144, 1.0), _rand((C, r), 145, 1.0)
    out = torch.full((3 * C * C + 8,), SENT, device=dev)
    ops.lora_merge(w.to(dev), aq.to(dev), bq.to(dev), av.to(dev), bv.to(dev), out, C, r, s)
    got = out[: 3 * C * C].cpu().view(3 * C, C)
    assert torch.equal(got[C: 2 * C], w[C: 2 * C]), "k rows must stay bit-identical to W"
    for sl, a, b in ((slice(0, C), aq, bq), (slice(2 * C, 3 * C), av, bv)):
        d = b.double() @ a.double()
        ref = w[sl].double() + s * d
        # r-term fp32 sum (sequential: (r + 1) 2^-24 of sum |b a|), the scale and the add: one rounding each
        tol = (r + 3) * 2.0 ** -24 * s * (b.double().abs() @ a.double().abs()) + _ulp(ref)
        _within(got[sl], ref, tol, f"lora_merge rows {sl}")
    assert (out[3 * C * C:] == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------
# AdaptFormer's ReLU epilogues (bf16 GEMM and f32 GEMM)
@pytest.mark.parametrize("path,tile", [("bf16", 0), ("bf16", 64064), ("f32", 0)])
def test_relu_epilogues(dev, path, tile):
    """h = max(x . Wd^T + b, 0) stored (EPI_BIAS_RELU_BF16); dh = (dG . Wu) * [h > 0] with the mask taken from the STORED h (EPI_RELU_BWD_BF16).
    N = 64 (the adapter width), ragged M, and units whose pre-activation is exactly 0 (zero weight row, zero bias)."""
    from gaviko_amd import ops
    M, C, N = 1033, 192, 64
    dt = torch.bfloat16 if path == "bf16" else torch.float32
    rnd = _bf16_round if path == "bf16" else (lambda t: t)
    x = rnd(_rand((M, C), 151, 1.0))
    wd = rnd(_rand((N, C), 152, 1 / math.sqrt(C)))
    b = _rand((N,), 153, 0.1)
    dead = [0, 5, 63]
    wd[dead] = 0
    b[dead] = 0
    dG = rnd(_rand((M, C), 154, 1.0))
    wuT = rnd(_rand((N, C), 155, 1 / math.sqrt(N)))          # [N][C]: the transposed up-projection the dgrad GEMM reads
    Mp = ops.pad_rows(M)
    X = torch.zeros((Mp, C), dtype=dt)
    X[:M] = x.to(dt)
    h = torch.full((Mp, N), SENT, dtype=dt, device=dev)
    ops.gemm_nt(X.to(dev), wd.to(dt).to(dev), M, h, epilogue=ops.EPI_BIAS_RELU_BF16, bias=b.to(dev), tile=tile)
    pre = x.double() @ wd.double().T + b.double()
    st = 2.0 ** -8 if path == "bf16" else 2.0 ** -24
    _within(h[:M], pre.clamp_min(0), st * pre.abs() + RED * math.sqrt(C) * (x.double().abs() @ wd.double().abs().T + b.double().abs()), "relu fwd")
    assert (h[:M, dead] == 0).all() and (h[M:] == SENT).all()
    hs = h[:M].cpu()
    G = torch.zeros((Mp, C), dtype=dt)
    G[:M] = dG.to(dt)
    hh = h.clone()
    hh[M:] = 0
    dh = torch.full((Mp, N), SENT, dtype=dt, device=dev)
    ops.gemm_nt(G.to(dev), wuT.to(dt).to(dev), M, dh, epilogue=ops.EPI_RELU_BWD_BF16, aux=hh, tile=tile)
    mask = (hs.double() > 0).double()
    acc = dG.double() @ wuT.double().T
    ref = acc * mask
    _within(dh[:M], ref, (st * acc.abs() + RED * math.sqrt(C) * (dG.double().abs() @ wuT.double().abs().T)) * mask, "relu bwd (mask of the stored h)")
    assert (dh[:M, dead] == 0).all(), "units with pre-activation exactly 0 must pass no gradient"
    assert (mask == 0).any() and (mask == 1).any()
    assert (dh[M:] == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------
# fft / bitfit gradient helpers
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_transpose_any(dev, dt):
    from gaviko_amd import ops
    rows, cols = 1033, 200
    x = _rand((rows, cols), 161, 3.0).to(dt)
    out = torch.full((rows * cols + 8,), SENT, dtype=dt, device=dev)
    ops.transpose_any(x.to(dev), out, rows, cols)
    assert torch.equal(out[: rows * cols].cpu().view(cols, rows), x.T) and (out[rows * cols:] == SENT).all()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("mapped", [False, True])
def test_colsum_any(dev, dt, mapped):
    """out[n] = sum_m x[m][n], optionally over the rows (m / rows_in) * rows_out + row_off + m % rows_in of the buffer."""
    from gaviko_amd import ops
    N = 200
    if mapped:
        rin, rout, roff, Bs = 100, 103, 2, 3
        M, nbuf = rin * Bs, rout * Bs
        rows = torch.tensor([(m // rin) * rout + roff + m % rin for m in range(M)])
    else:
        rin = rout = roff = 0
        M = nbuf = 1033
        rows = torch.arange(M)
    x = _rand((nbuf, N), 171, 2.0).to(dt)
    out = torch.full((N + 8,), SENT, device=dev)
    ones, zeros, junk = torch.ones(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    ops.colsum_any(x.to(dev), out, ones, zeros, junk, torch.zeros(64 * 2 * N, device=dev), M, N, rows_in=rin, rows_out=rout, row_off=roff)
    xl = x[rows].double()
    _within(out[:N], xl.sum(0), RED * math.sqrt(M) * xl.abs().sum(0), f"colsum_any {dt} mapped={mapped}")
    assert (out[N:] == SENT).all()


# ---------------------------------------------------------------------------------------------------------------------
# loss seed with the running meter
def _loss_ref(x, y, kind, w, gamma, eps=1e-16, ignore=-100):
    """float64 per-row losses (0 on ignored rows) and weights, as loss.hip computes them (focal: the double clamp + softmax that executes)."""
    x = x.double()
    ok = y != ignore
    t = torch.where(ok, y, torch.zeros_like(y))
    wt = (w.double()[t] if w is not None else torch.ones(len(y), dtype=torch.float64)) * ok
    if kind == 0:
        l = torch.logsumexp(x, 1) - x.gather(1, t[:, None])[:, 0]
    else:
        p1 = x.clamp(eps, 1 - eps).softmax(1)
        pt = p1.clamp(eps, 1 - eps).softmax(1).gather(1, t[:, None])[:, 0]
        l = (1 - pt) ** gamma * -torch.log(eps + pt)
    return wt * l, wt, ok


@pytest.mark.parametrize("B", [3, 300])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_loss_meter_every_reduction(dev, B, kind, reduction):
    """meter[0] gains the reduced loss * B under 'mean' / 'sum' (train.py:327) and the sum of the per-sample losses under 'none' (the loss is
    already a vector there); meter[1] the correct argmax predictions of the rows not ignored; meter[2] the samples.  Two steps accumulate."""
    from gaviko_amd import ops
    K = 5
    g = torch.Generator().manual_seed(181 + B + kind)
    x = torch.rand(B, K, generator=g) * 1.6 - 0.3 if kind == 1 else torch.randn(B, K, generator=g) * 3
    y = torch.randint(0, K, (B,), generator=g)
    y[1] = -100
    if B > 3:
        y[100:110] = -100
    w = torch.rand(K, generator=g) + 0.5
    lrow, wt, ok = _loss_ref(x, y, kind, w, 1.2)
    red = {"mean": lrow.sum() / wt.sum(), "sum": lrow.sum(), "none": lrow}[reduction]
    meter = torch.zeros(3, device=dev)
    loss = torch.full((B if reduction == "none" else 1,), SENT, device=dev)
    dl = torch.zeros((B, K), device=dev)
    for _ in range(2):
        ops.loss_fwd_bwd(x.to(dev), y.to(dev), loss, dl, kind, gamma=1.2, weights=w.to(dev), meter=meter, reduction=reduction)
    # every loss term carries a few fp32 roundings through exp / log / pow (<= 2e-6 relative); the batch sums add RED sqrt(B); terms are >= 0
    rel = 2e-6 + RED * math.sqrt(B)
    _within(loss, red.reshape(-1), rel * red.reshape(-1).abs() + rel * lrow.abs().max(), f"loss ({reduction})")
    want0 = 2 * (lrow.sum() if reduction == "none" else red * B)
    m = meter.cpu().double()
    assert abs(m[0] - want0) <= rel * abs(want0), f"meter[0] {m[0].item():.7g} vs {want0.item():.7g} ({reduction})"
    correct = ((x.argmax(1) == y) & ok).sum().item()
    assert m[1].item() == 2 * correct and m[2].item() == 2 * B
