"""-m gpu: the row kernels every step of every method goes through -- LayerNorm forward / backward in all their forms (layernorm.hip and the
projection forms it dispatches to rowwise.hip / sidepass.hip), the pooled head and the token assembly (head.hip) -- at their edges, each
against a plain float64 computation on the CPU over exactly the fp32 / bf16 values the kernel receives.

Inputs are seeded and built once (section "inputs"): rows whose mean dwarfs their spread (offset 0 / 40 / 3000), constant rows (var = 0,
rstd = 1 / sqrt(eps)) mixed in among ordinary rows so that a four-wave workgroup holds both kinds, and rows with one channel at +-300
planted at the first and last column of every 256-column chunk the width reaches.  Widths run over every partially filled chunk
(C = 4 .. 1024), row counts over the 4-rows-per-workgroup and the 64-slab boundaries.  Every output is allocated longer than its logical
size and pre-filled with a sentinel; nothing outside the logical region may change.

Every bound is one of three kinds, none taken from a measured error of the kernel:
  bit-exact       token assembly (one fp32 add, or B adds in the kernel's order); constant rows (mean = the row value, y = beta, the bf16
                  output = bf16(beta)); layernorm_fwd_fix with enh == lat (x comes back unchanged); rows outside a selection or past M keep
                  their sentinel bits; outputs of refused calls; results of the same kernel with an optional output omitted;
                  layernorm_bwd_up's dx16 = bf16(dx) (test_layernorm_bwd_up_matches_two_kernels).
  project bounds  forward statistics: mean 2e-6 max(1, |mean|), rstd 2e-5 relative, fp32 y 2e-5 against the float64 LayerNorm centred on
                  the mean the kernel returned, bf16 y 2^-8 of the value on top of that (test_skinny_down_ln_large_common_offset says why
                  the centre is the kernel's own mean; test_rank_l_kernels_gpu.py, test_kernels_gpu.py).
                  backward: LN_BWD_DX_TOL / LN_BWD_DX16_TOL of test_kernels_gpu.py; the fused projection y = dx . W within atol 3e-5 + rtol
                  1e-5 of the float64 product of the kernel's own dx (test_layernorm_bwd_with_fused_projection); layernorm_bwd_up's dx
                  within 2e-6 of |dx|max (test_layernorm_bwd_up_matches_two_kernels).
                  head: logits 3e-5, dG / dWh / dbh 5e-5 of the tensor's maximum (test_head_fwd_bwd); pooled as the fp32 y above.
                  The statistics and dx bounds are applied PER ROW here (the scale is the row's own maximum, not the tensor's), so that a
                  constant row with |dx| ~ 300 next to an ordinary one cannot widen the ordinary row's bound: never looser than the originals.
  RED model       fp32 reductions over n terms: RED sqrt(n) sum |terms|, RED = 4e-7 (test_aux_kernels_gpu.py): the affine gradients, the
                  raw-row projection of layernorm_fwd_proj, the prompt fix of layernorm_fwd_fix (plus one ulp of a value an fp32 add lands on).
"""
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu          # (the planted-column checks at the top run without a device, so the mark is per test)

RED = 4e-7
SENT = 7.0                     # sentinel of the regions a kernel must not write
EPS = 1e-5
LN_BWD_DX_TOL = 2e-5           # fp32 dx against fp64, relative to max(1, |dx|max)      (tests/test_kernels_gpu.py)
LN_BWD_DX16_TOL = 2 ** -7      # its bf16 copy, relative to |dx|max                    (tests/test_kernels_gpu.py)

C_LIST = (4, 64, 252, 256, 260, 512, 516, 768, 1020, 1024)
M_HARD = 67
KINDS = ("off0", "off40", "off3000", "const", "outlier")
CONST_VALUES = (3000.0, 0.5, -17.25, 0.0)                     # few mantissa bits: every summation order gives the exact mean
# (L, C) of the projection forms: every L with a partial and a full last chunk, L = 20 at every width from 128 up (768 / 1024: 16-row tiles)
PROJ_CASES = [(20, 252), (20, 256), (20, 260), (20, 512), (20, 516), (20, 768), (20, 1020), (20, 1024),
              (4, 252), (4, 1024), (8, 260), (8, 768), (16, 516), (16, 1020)]
# ... each at M_HARD rows; the row counts 1, 3, 5 at the boundary subset (a partial chunk and the 16-row-tile form, two other L)
PROJ_M_CASES = [(Lt, C, M_HARD) for Lt, C in PROJ_CASES] + [(Lt, C, M) for Lt, C in ((20, 260), (20, 1024), (4, 252), (8, 768)) for M in (1, 3, 5)]
UP_C = (192, 768, 1024)


# ---------------------------------------------------------------------------------------------------------------------- helpers
def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


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


def _sent(shape, dev, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device=dev)


def _intact(t, n, what):
    """rows (or elements) n.. of a sentinel-filled buffer still hold the sentinel"""
    assert t.shape[0] > n and bool((t[n:] == SENT).all()), f"{what}: wrote past its {n} logical rows / elements"


def _rowmax(t):
    return t.abs().amax(dim=-1, keepdim=True)


# ----------------------------------------------------------------------------------------------------------------------- inputs
def _planted_cols(C):
    """columns of the +-300 outlier: 0, C - 1, and the first and last column of every 256-column chunk C reaches"""
    cols = {0, C - 1}
    for k in range((C + 255) // 256):
        cols |= {256 * k, min(256 * k + 255, C - 1)}
    return sorted(cols)


def _const_rows(M):
    return tuple(i for i in range(M) if i % 5 == 1)


@functools.lru_cache(maxsize=None)
def _hard(C, M, kind):
    """(x fp32 [M][C], indices of its constant rows).  Cached: callers never write into it."""
    if kind.startswith("off"):
        off = float(kind[3:])
        return (off + _rand((M, C), 231) + _rand((M, 1), 232, 0.3) * (off / 10)).float(), ()
    if kind == "const":                                       # rows 1, 6, 11, ...: each 4-row workgroup that has one also has ordinary rows
        x = _rand((M, C), 233) + 0.3
        idx = _const_rows(M) or (0,)
        for n, i in enumerate(idx):
            x[i] = CONST_VALUES[n % len(CONST_VALUES)]
        return x, idx
    assert kind == "outlier"
    x = _rand((M, C), 234)
    cols = _planted_cols(C)
    for i in range(M):
        x[i, cols[i % len(cols)]] = 300.0 if (i // len(cols)) % 2 == 0 else -300.0
    return x, ()


def _affine(C, seed):
    return 1 + _rand((C,), seed, 0.2), _rand((C,), seed + 1, 0.1)


def _stats64(x):
    """float64 mean and rstd of fp32 rows"""
    xd = x.double()
    return xd.mean(-1), (xd.var(-1, unbiased=False) + EPS).rsqrt()


# the pooled head: (B, T, C, K, r0, R).  R and K step over the head's sixteen waves, C over the chunk edges; every boundary R (15, 16, 17, 49)
# and every boundary K (1, 16, 17) meets every boundary C (4, 260, 1020, 1024): K = a latin square over (R, C); r0 + R == T in every other case
HEAD_CASES = [(3 if (ri + ci) % 2 == 0 else 1, (5 if ri % 2 else 0) + R + (0 if (ri + ci) % 2 else 2), C, (1, 16, 17, 5)[(ri + ci) % 4], 5 if ri % 2 else 0, R)
              for ci, C in enumerate((4, 260, 1020, 1024)) for ri, R in enumerate((15, 16, 17, 49))]
HEAD_CASES += [(3, 9, 192, 5, 5, 1), (1, 33, 192, 17, 0, 33), (3, 40, 192, 1, 5, 33), (1, 1, 1024, 16, 0, 1), (3, 3, 4, 5, 0, 1)]


# --------------------------------------------------------------------------------------------- CPU: the test's own inputs and case lists
def test_planted_columns_cover_every_chunk_boundary():
    assert _planted_cols(4) == [0, 3] and _planted_cols(256) == [0, 255] and _planted_cols(260) == [0, 255, 256, 259]
    assert _planted_cols(1020) == [0, 255, 256, 511, 512, 767, 768, 1019]
    for C in C_LIST + UP_C:
        cols = _planted_cols(C)
        assert C % 4 == 0 and all(0 <= c < C for c in cols) and 0 in cols and C - 1 in cols
        # a lane holds columns 256 k + 4 lane .. + 3 of chunk k: the first column is lane 0 element 0, the last column of a chunk is element 3
        # of its last active lane (lane 63 of a full chunk, lane (C - 256 k) / 4 - 1 of a partial one)
        for k in range((C + 255) // 256):
            width = min(256, C - 256 * k)
            first, last = 256 * k, 256 * k + width - 1
            assert first in cols and last in cols, (C, k)
            assert (first % 256) // 4 == 0 and first % 4 == 0 and (last % 256) // 4 == width // 4 - 1 and last % 4 == 3
        assert len(cols) <= M_HARD                            # M_HARD rows: every planted column is used, with both signs from 2 len(cols) rows on
        x, _ = _hard(C, M_HARD, "outlier")
        big = x.abs() == 300
        assert bool((big.sum(1) == 1).all()) and sorted(set(big.nonzero()[:, 1].tolist())) == cols, C
        assert bool(((x == 300).any(0) | ~big.any(0)).all()) and (2 * len(cols) > M_HARD or bool((x == -300).any()))


def test_hard_rows_are_what_they_claim():
    k = torch.arange(1, 1025, dtype=torch.float32)
    for v in CONST_VALUES:                                    # every partial sum k * v of a constant row is an fp32 number: the mean is exact in any order
        assert torch.equal((k * v).double(), k.double() * v)
    for M in (1, 2, 5, M_HARD):
        x, idx = _hard(260, M, "const")
        assert idx == (_const_rows(M) or (0,)) and all(bool((x[i] == x[i, 0]).all()) for i in idx)
        groups = {i // 4 for i in idx}
        assert M < 4 or all(any(j not in idx for j in range(4 * g, min(4 * g + 4, M))) for g in groups), "a workgroup of constant rows only"
    assert {CONST_VALUES[n % 4] for n in range(len(_const_rows(M_HARD)))} == set(CONST_VALUES)
    x, _ = _hard(768, M_HARD, "off3000")
    mu, rs = _stats64(x)
    assert mu.abs().min() > 2500 and (mu.abs() * rs).max() > 3000, "|mean| / std in the thousands"


def test_head_cases_cover_every_axis():
    ax = lambda i: {c[i] for c in HEAD_CASES}
    assert ax(0) == {1, 3} and ax(2) == {4, 192, 260, 1020, 1024} and ax(3) == {1, 5, 16, 17} and ax(4) == {0, 5}
    assert ax(5) == {1, 15, 16, 17, 33, 49}
    assert all(r0 + R <= T for _, T, _, _, r0, R in HEAD_CASES) and any(r0 + R == T and r0 > 0 for _, T, _, _, r0, R in HEAD_CASES)
    for C in (4, 260, 1020, 1024):
        assert {c[5] for c in HEAD_CASES if c[2] == C} >= {15, 16, 17, 49}, C
        assert {c[3] for c in HEAD_CASES if c[2] == C} >= {1, 16, 17}, C
    assert len(HEAD_CASES) == len(set(HEAD_CASES)) <= 24


# ---------------------------------------------------------------------------------------------------- 2. forward statistics and outputs
def _check_fwd(what, x, gamma, beta, M, const, mean=None, rstd=None, y32=None, y16=None, centre=None):
    """x: the fp32 rows the kernel normalised (CPU).  Statistics per row against float64; y against the float64 LayerNorm centred on the mean the
    kernel returned (centre = that mean, when this call did not return one).  Constant rows: mean = the value, y = beta, bit for bit."""
    xd = x[:M].double()
    mu, rs = _stats64(x[:M])
    if mean is not None:
        _within(mean[:M], mu, 2e-6 * mu.abs().clamp_min(1.0), f"{what}: mean")
        _within(rstd[:M], rs, 2e-5 * rs, f"{what}: rstd")
        centre = mean[:M].cpu().double()
        e_mu = ((centre - mu).abs() / mu.abs().clamp_min(1.0)).max().item()
        e_rs = ((rstd[:M].cpu().double() - rs).abs() / rs).max().item()
        print(f"{what}: mean err / max(1, |mean|) {e_mu:.2e}, rstd rel err {e_rs:.2e}")
    yref = (xd - centre[:, None]) * rs[:, None] * gamma.double() + beta.double()
    if y32 is not None:
        _within(y32[:M], yref, 2e-5, f"{what}: fp32 y")
    if y16 is not None:
        _within(y16[:M], yref, 2.0 ** -8 * yref.abs() + 2e-5, f"{what}: bf16 y")
    for i in const:
        if mean is not None:
            assert mean[i].item() == x[i, 0].item(), f"{what}: constant row {i}: mean {mean[i].item()!r} != {x[i, 0].item()!r}"
        if y32 is not None:
            assert torch.equal(y32[i].cpu(), beta), f"{what}: constant row {i}: fp32 y != beta"
        if y16 is not None:
            assert torch.equal(y16[i].cpu(), beta.bfloat16()), f"{what}: constant row {i}: bf16 y != bf16(beta)"
    for t, n in ((mean, "mean"), (rstd, "rstd"), (y32, "y32"), (y16, "y16")):
        if t is not None:
            _intact(t, M, f"{what}: {n}")


def _run_layernorm_fwd(dev, C, M, kind):
    from gaviko_amd import ops
    x, const = _hard(C, M, kind)
    gamma, beta = _affine(C, 301)
    X, G, Bt = x.to(dev), gamma.to(dev), beta.to(dev)
    out = {}
    for form in ("f32", "bf16", "both", "nostats"):
        y32 = _sent((M + 3, C), dev) if form != "bf16" else None
        y16 = _sent((M + 3, C), dev, torch.bfloat16) if form != "f32" else None
        mean, rstd = (None, None) if form == "nostats" else (_sent((M + 4,), dev), _sent((M + 4,), dev))
        ops.layernorm_fwd(X, G, Bt, M, C, y32=y32, y16=y16, mean=mean, rstd=rstd)
        what = f"layernorm_fwd[{form}] C={C} M={M} {kind}"
        _check_fwd(what, x, gamma, beta, M, const, mean, rstd, y32, y16, centre=out.get("centre"))
        if form == "f32":
            out.update(centre=mean[:M].cpu().double(), y32=y32, mean=mean, rstd=rstd)
        elif form == "bf16":
            out.update(y16=y16)
            assert torch.equal(mean, out["mean"]) and torch.equal(rstd, out["rstd"]), f"{what}: statistics differ from the fp32-output call"
        else:
            assert torch.equal(y32, out["y32"]) and torch.equal(y16, out["y16"]), f"{what}: y differs from the single-output calls"
    return out


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", C_LIST)
def test_layernorm_fwd_hard_rows(dev, C, kind):
    """gvk_layernorm_fwd with the fp32 output, the bf16 output, both, and with mean / rstd omitted, on the rows of section 1 at every width."""
    _run_layernorm_fwd(dev, C, M_HARD, kind)


@gpu
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("C", [4, 260, 1024])
def test_layernorm_fwd_row_counts(dev, C, M):
    """Four rows per workgroup: M = 1 .. 5 (M_HARD = 67 is the sweep above); the spare rows after M keep the sentinel."""
    for kind in ("off3000", "const"):
        _run_layernorm_fwd(dev, C, M, kind)


@gpu
@pytest.mark.parametrize("C", C_LIST)
def test_layernorm_fwd_fix_adding_zero(dev, C):
    """gvk_layernorm_fwd_fix with enh == lat: the fix adds exactly zero, x comes back bit-identical, and y16 / mean / rstd meet the bounds of
    gvk_layernorm_fwd on the same rows (T = M_HARD, B = 1: the first P rows take the fix path, the others do not)."""
    from gaviko_amd import ops
    M = T = M_HARD
    P, Lt = 32, 20
    lat = _rand((M, Lt), 311)
    enh = lat[:P].clone().view(1, P, Lt)
    wup = _rand((C, Lt), 312, 1 / math.sqrt(Lt))
    gamma, beta = _affine(C, 301)
    for kind in KINDS:
        x, const = _hard(C, M, kind)
        X = x.to(dev)
        y16, mean, rstd = _sent((M + 3, C), dev, torch.bfloat16), _sent((M + 4,), dev), _sent((M + 4,), dev)
        ops.layernorm_fwd_fix(X, gamma.to(dev), beta.to(dev), M, C, y16=y16, mean=mean, rstd=rstd, enh=enh.to(dev), lat=lat.to(dev),
                              wup=wup.to(dev), T=T, P=P, L_=Lt)
        what = f"layernorm_fwd_fix[enh == lat] C={C} {kind}"
        assert torch.equal(X.cpu(), x), f"{what}: x changed"
        _check_fwd(what, x, gamma, beta, M, const, mean, rstd, y16=y16)
        y16b, mean_b, rstd_b = _sent((M + 3, C), dev, torch.bfloat16), _sent((M + 4,), dev), _sent((M + 4,), dev)
        ops.layernorm_fwd(X, gamma.to(dev), beta.to(dev), M, C, y16=y16b, mean=mean_b, rstd=rstd_b)
        print(f"{what}: bitwise equal to layernorm_fwd: y16 {torch.equal(y16, y16b)}, mean {torch.equal(mean, mean_b)}, rstd {torch.equal(rstd, rstd_b)}")


@gpu
@pytest.mark.parametrize("B,T,P,C", [(3, 64, 8, 192), (2, 67, 32, 768), (1, 130, 32, 1024)])
def test_layernorm_fwd_fix_hard_rows(dev, B, T, P, C):
    """A real fix on the offset-3000 rows: the prompt rows come back as x + (enh - lat) . Wup^T (fp32 sum of L products, one fp32 add: RED model
    plus half an ulp of the sum), every other row bit-identical, and the LayerNorm is that of the rows as written back."""
    from gaviko_amd import ops
    Lt, M = 20, B * T
    x, _ = _hard(C, M, "off3000")
    enh, lat = _rand((B, P, Lt), 321), _rand((M, Lt), 322)
    wup = _rand((C, Lt), 323, 1 / math.sqrt(Lt))
    gamma, beta = _affine(C, 301)
    d = enh.double() - lat.double().view(B, T, Lt)[:, :P]
    xf = x.double().clone().view(B, T, C)
    xf[:, :P] += d @ wup.double().T
    absd = d.abs() @ wup.double().abs().T
    X = x.to(dev)
    y16, mean, rstd = _sent((M + 3, C), dev, torch.bfloat16), _sent((M + 4,), dev), _sent((M + 4,), dev)
    ops.layernorm_fwd_fix(X, gamma.to(dev), beta.to(dev), M, C, y16=y16, mean=mean, rstd=rstd, enh=enh.to(dev), lat=lat.to(dev), wup=wup.to(dev),
                          T=T, P=P, L_=Lt)
    got = X.cpu()
    g3 = got.view(B, T, C)
    _within(g3[:, :P], xf[:, :P], RED * math.sqrt(Lt) * absd + 2.0 ** -24 * xf[:, :P].abs(), "layernorm_fwd_fix: fixed rows written back")
    assert torch.equal(g3[:, P:], x.view(B, T, C)[:, P:]), "layernorm_fwd_fix changed a non-prompt row of x"
    _check_fwd(f"layernorm_fwd_fix[real fix] C={C}", got, gamma, beta, M, (), mean, rstd, y16=y16)


def _proj_weight(Lt, C, seed):
    """(w [L][C] as float64 math sees it, the tensor handed to the kernel, its w_layout): L = 4 and 16 take the [C][L] layout"""
    w = _rand((Lt, C), seed, 1 / math.sqrt(C))
    lay = 1 if Lt in (4, 16) else 0
    return w, (w.T.contiguous() if lay else w), lay


@gpu
@pytest.mark.parametrize("Lt,C,M", PROJ_M_CASES)
def test_layernorm_fwd_proj_hard_rows(dev, Lt, C, M):
    """gvk_layernorm_fwd_proj: bf16 LayerNorm + statistics as gvk_layernorm_fwd, and z = x . W^T + b of the RAW rows (fp32 sum over C: RED model)."""
    from gaviko_amd import ops
    w, wk, lay = _proj_weight(Lt, C, 331)
    bias = _rand((Lt,), 332, 0.1)
    gamma, beta = _affine(C, 301)
    for kind in KINDS if M == M_HARD else ("off3000", "const"):
        x, const = _hard(C, M, kind)
        y16, mean, rstd = _sent((M + 3, C), dev, torch.bfloat16), _sent((M + 4,), dev), _sent((M + 4,), dev)
        z, y = _sent((M + 3, Lt), dev), _sent((M + 3, Lt), dev)
        ops.layernorm_fwd_proj(x.to(dev), gamma.to(dev), beta.to(dev), M, C, y16=y16, mean=mean, rstd=rstd, w=wk.to(dev), bias=bias.to(dev), z=z, y=y,
                               L_=Lt, w_layout=lay, act=0)
        what = f"layernorm_fwd_proj L={Lt} C={C} {kind}"
        _check_fwd(what, x, gamma, beta, M, const, mean, rstd, y16=y16)
        ref = x.double() @ w.double().T + bias.double()
        _within(z[:M], ref, RED * math.sqrt(C + 1) * (x.double().abs() @ w.double().abs().T + bias.double().abs()), f"{what}: z")
        assert torch.equal(y, z), f"{what}: act = 0: y != z"
        _intact(z, M, f"{what}: z")


# --------------------------------------------------------------------------------------------------------------- 3. backward forms: dx
def _bwd_inputs(C, M, kind, seed=341):
    """x, gamma, dy, dres (fp32, CPU) and mean / rstd = the float64 statistics rounded to fp32 -- NOT the forward kernel's"""
    x, const = _hard(C, M, kind)
    gamma, _ = _affine(C, 301)
    mu, rs = _stats64(x)
    return x, const, gamma, _rand((M, C), seed), _rand((M, C), seed + 1), mu.float(), rs.float()


def _bwd_ref(x, dy, gamma, mean32, rstd32, dres):
    """dx = dres + rstd (g dy - mean(g dy) - xhat mean(g dy xhat)), xhat = (x - mean) rstd, in float64 on the fp32 mean / rstd the kernel is handed"""
    m, r = mean32.double()[:, None], rstd32.double()[:, None]
    xh = (x.double() - m) * r
    dh = dy.double() * gamma.double()
    dx = r * (dh - dh.mean(-1, keepdim=True) - xh * (dh * xh).mean(-1, keepdim=True))
    return dx if dres is None else dx + dres.double()


def _check_dx(what, want, dx, dx16=None):
    """per row: LN_BWD_DX_TOL max(1, |dx|max of the row), and LN_BWD_DX16_TOL |dx|max of the row for the bf16 copy"""
    n = want.shape[0]
    _within(dx[:n], want, LN_BWD_DX_TOL * _rowmax(want).clamp_min(1.0), f"{what}: dx")
    if dx16 is not None:
        _within(dx16[:n], want, LN_BWD_DX16_TOL * _rowmax(want), f"{what}: dx16")


def _run_layernorm_bwd(dev, C, M, kind):
    from gaviko_amd import ops
    x, const, gamma, dy, dres, mean, rstd = _bwd_inputs(C, M, kind)
    X, G, Mn, Rs = x.to(dev), gamma.to(dev), mean.to(dev), rstd.to(dev)
    for dy16, with_dres, with_dx16 in ((False, True, True), (True, False, False), (False, False, True), (True, True, True)):
        dyk = dy.bfloat16() if dy16 else dy
        dx = _sent((M + 3, C), dev)
        dx16 = _sent((M + 3, C), dev, torch.bfloat16) if with_dx16 else None
        ops.layernorm_bwd(dyk.to(dev), X, Mn, Rs, G, M, C, dx=dx, dres=dres.to(dev) if with_dres else None, dx16=dx16)
        what = f"layernorm_bwd C={C} M={M} {kind} dy={'bf16' if dy16 else 'fp32'} dres={with_dres} dx16={with_dx16}"
        want = _bwd_ref(x, dyk.float(), gamma, mean, rstd, dres if with_dres else None)
        _check_dx(what, want, dx, dx16)
        _intact(dx, M, what)
        if dx16 is not None:
            _intact(dx16, M, what + " dx16")
    if const:
        assert _rowmax(want[list(const)]).min().item() > 10, "constant rows: rstd ~ 316 makes dx large"


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", C_LIST)
def test_layernorm_bwd_hard_rows(dev, C, kind):
    """gvk_layernorm_bwd, fp32 and bf16 dy, with and without dres / dx16, on the rows of section 1 at every width."""
    _run_layernorm_bwd(dev, C, M_HARD, kind)


@gpu
@pytest.mark.parametrize("M", [1, 3, 5])
@pytest.mark.parametrize("C", [4, 260, 1024])
def test_layernorm_bwd_row_counts(dev, C, M):
    for kind in ("off3000", "const"):
        _run_layernorm_bwd(dev, C, M, kind)


@gpu
@pytest.mark.parametrize("dy16", [False, True], ids=["dy_fp32", "dy_bf16"])
@pytest.mark.parametrize("rows", [(1, 1, 9), (3, 1, 9), (2, 3, 9), (2, 9, 9)], ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("C", [260, 1024])
def test_layernorm_bwd_row_subsets(dev, C, rows, dy16):
    """rows = (groups, rows_per_group, group_stride) over a [3 * 9][C] buffer: the selected rows get dx and dx16, every other row keeps its
    sentinel bits in both."""
    from gaviko_amd import ops
    T = 9
    M = 3 * T
    groups, rpg, gs = rows
    assert gs == T
    sel = torch.zeros(M, dtype=torch.bool)
    for g in range(groups):
        sel[g * gs: g * gs + rpg] = True
    assert int(sel.sum()) == groups * rpg
    for kind in ("off3000", "const"):
        x, const, gamma, dy, dres, mean, rstd = _bwd_inputs(C, M, kind)
        dyk = dy.bfloat16() if dy16 else dy
        dx, dx16 = _sent((M, C), dev), _sent((M, C), dev, torch.bfloat16)
        ops.layernorm_bwd(dyk.to(dev), x.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), M, C, dx=dx, dres=dres.to(dev), dx16=dx16, rows=rows)
        want = _bwd_ref(x, dyk.float(), gamma, mean, rstd, dres)
        what = f"layernorm_bwd rows={rows} C={C} {kind}"
        _check_dx(what, want[sel], dx.cpu()[sel], dx16.cpu()[sel])
        assert bool((dx.cpu()[~sel] == SENT).all()) and bool((dx16.cpu()[~sel] == SENT).all()), f"{what}: a row outside the selection was written"


@gpu
@pytest.mark.parametrize("Lt,C,M", PROJ_M_CASES)
def test_layernorm_bwd_proj_hard_rows(dev, Lt, C, M):
    """gvk_layernorm_bwd with proj: dx / dx16 as the plain form, and y = dx . W within atol 3e-5 + rtol 1e-5 of the float64 product of the
    kernel's own dx (the bound of test_layernorm_bwd_with_fused_projection)."""
    from gaviko_amd import ops
    w, wk, lay = _proj_weight(Lt, C, 351)
    for kind in KINDS if M == M_HARD else ("off3000", "const"):
        x, const, gamma, dy, dres, mean, rstd = _bwd_inputs(C, M, kind)
        for dy16 in (False, True):
            dyk = dy.bfloat16() if dy16 else dy
            dx, dx16, y = _sent((M + 3, C), dev), _sent((M + 3, C), dev, torch.bfloat16), _sent((M + 3, Lt), dev)
            ops.layernorm_bwd(dyk.to(dev), x.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), M, C, dx=dx, dres=dres.to(dev), dx16=dx16,
                              proj=dict(w=wk.to(dev), y=y, L_=Lt, w_layout=lay))
            what = f"layernorm_bwd[proj] L={Lt} C={C} M={M} {kind} dy={'bf16' if dy16 else 'fp32'}"
            _check_dx(what, _bwd_ref(x, dyk.float(), gamma, mean, rstd, dres), dx, dx16)
            yref = dx[:M].cpu().double() @ w.double().T
            _within(y[:M], yref, 3e-5 + 1e-5 * yref.abs(), f"{what}: y = dx . W")
            for t, n in ((dx, "dx"), (dx16, "dx16"), (y, "y")):
                _intact(t, M, f"{what}: {n}")


@gpu
@pytest.mark.parametrize("M", [1, 3, 5, M_HARD])
@pytest.mark.parametrize("C", UP_C)
def test_layernorm_bwd_up_hard_rows(dev, C, M):
    """gvk_layernorm_bwd_up: dx = dres + LN'(dy) + lat . W.  Bounds: LN_BWD_DX_TOL per row; 2e-6 of |dx|max over the tensor and dx16 == bf16(dx)
    bit for bit (both from test_layernorm_bwd_up_matches_two_kernels); both weight layouts."""
    from gaviko_amd import ops
    Lt = 20
    lat, w = _rand((M, Lt), 361), _rand((Lt, C), 362, 0.05)
    for kind in KINDS:
        x, const, gamma, dy, dres, mean, rstd = _bwd_inputs(C, M, kind)
        want = _bwd_ref(x, dy, gamma, mean, rstd, dres) + lat.double() @ w.double()
        for lay, wk in ((1, w), (0, w.T.contiguous())):
            dx, dx16 = _sent((M + 3, C), dev), _sent((M + 3, C), dev, torch.bfloat16)
            ops.layernorm_bwd_up(dy.to(dev), x.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), M, C, dx=dx, dres=dres.to(dev), dx16=dx16,
                                 lat=lat.to(dev), w=wk.to(dev), L_=Lt, w_layout=lay)
            what = f"layernorm_bwd_up C={C} M={M} {kind} w_layout={lay}"
            _check_dx(what, want, dx)
            _within(dx[:M], want, 2e-6 * want.abs().max().item(), f"{what}: dx (2e-6 of |dx|max)")
            assert torch.equal(dx16[:M], dx[:M].bfloat16()), f"{what}: dx16 != bf16(dx)"
            _intact(dx, M, what)
            _intact(dx16, M, what + " dx16")


@gpu
def test_projection_forms_refuse_what_they_do_not_cover(dev):
    """One call outside each launcher's set: the documented refusal, and untouched outputs."""
    from gaviko_amd import ops
    M = 5

    def operands(C, Lt):
        x, _, gamma, dy, dres, mean, rstd = _bwd_inputs(C, M, "off0")
        t = lambda a: a.to(dev)
        return t(x), t(gamma), t(dy), t(dres), t(mean), t(rstd), t(_rand((Lt, C), 371, 0.05)), t(_rand((M, Lt), 372))

    def untouched(*ts):
        torch.cuda.synchronize()
        assert all(bool((t == SENT).all()) for t in ts), "a refused call wrote an output"

    # gvk_layernorm_fwd_proj: C = 64 < 128 and L = 12
    for C, Lt in ((64, 20), (256, 12)):
        x, gamma, dy, dres, mean, rstd, w, lat = operands(C, Lt)
        y16, mo, ro, y = _sent((M, C), dev, torch.bfloat16), _sent((M,), dev), _sent((M,), dev), _sent((M, Lt), dev)
        with pytest.raises(ops.L.GavikoHipError, match=r"the fused projection covers L in \{4, 8, 16, 20\} and C >= 128"):
            ops.layernorm_fwd_proj(x, gamma, gamma, M, C, y16=y16, mean=mo, rstd=ro, w=w, y=y, L_=Lt)
        untouched(y16, mo, ro, y)
        # gvk_layernorm_bwd with proj: the same set
        dx, dx16 = _sent((M, C), dev), _sent((M, C), dev, torch.bfloat16)
        with pytest.raises(ops.L.GavikoHipError, match=r"the fused projection covers L in \{4, 8, 16, 20\} and C >= 128"):
            ops.layernorm_bwd(dy, x, mean, rstd, gamma, M, C, dx=dx, dres=dres, dx16=dx16, proj=dict(w=w, y=y, L_=Lt, w_layout=0))
        untouched(dx, dx16, y)
    # gvk_layernorm_bwd: the projection form with a row subset, and a width that is no multiple of 4
    x, gamma, dy, dres, mean, rstd, w, lat = operands(256, 20)
    dx, y = _sent((M, 256), dev), _sent((M, 20), dev)
    with pytest.raises(ops.L.GavikoHipError, match="rows and proj are exclusive"):
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, M, 256, dx=dx, rows=(1, 1, M), proj=dict(w=w, y=y, L_=20, w_layout=0))
    with pytest.raises(ops.L.GavikoHipError, match="C=254 must be a multiple of 4"):
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, M, 254, dx=dx)
    with pytest.raises(ops.L.GavikoHipError, match="do not fit M=5"):
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, M, 256, dx=dx, rows=(2, 2, 4))
    untouched(dx, y)
    # gvk_layernorm_bwd_up: L = 20 at a width outside {192, 768, 1024}, and L = 16 at one inside
    for C, Lt in ((260, 20), (768, 16)):
        x, gamma, dy, dres, mean, rstd, w, lat = operands(C, Lt)
        dx, dx16 = _sent((M, C), dev), _sent((M, C), dev, torch.bfloat16)
        with pytest.raises(ops.L.GavikoHipError, match=r"covers L = 20 and C in \{192, 768, 1024\}"):
            ops.layernorm_bwd_up(dy, x, mean, rstd, gamma, M, C, dx=dx, dres=dres, dx16=dx16, lat=lat, w=w, L_=Lt, w_layout=1)
        untouched(dx, dx16)


# ------------------------------------------------------------------------------------------------------------------ 4. affine gradients
@gpu
@pytest.mark.parametrize("M", [1, 63, 64, 65, 128, 129, 300])
@pytest.mark.parametrize("C", [4, 252, 260, 768, 1024])
def test_layernorm_bwd_affine_slabs(dev, C, M):
    """dgamma[c] = sum_m dy xhat, dbeta[c] = sum_m dy over 64 slabs of ceil(M / 64) rows: empty slabs for M < 64 (the scratch starts as NaN, so a
    slab read before it is written shows), a short last slab otherwise; accumulate off and on.  Rows at offset 3000 with constant rows mixed in.
    RED sqrt(M) sum |terms| per column, plus one ulp of the prior value when accumulating."""
    from gaviko_amd import ops
    x = _hard(C, M, "off3000")[0].clone()
    for n, i in enumerate(_const_rows(M)):
        x[i] = CONST_VALUES[n % len(CONST_VALUES)]
    mu, rs = _stats64(x)
    mean, rstd = mu.float(), rs.float()
    dy = _rand((M, C), 401)
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    dg_ref, db_ref = (dy.double() * xh).sum(0), dy.double().sum(0)
    dg_tol = RED * math.sqrt(M) * (dy.double() * xh).abs().sum(0)
    db_tol = RED * math.sqrt(M) * dy.double().abs().sum(0)
    X, D, Mn, Rs = x.to(dev), dy.to(dev), mean.to(dev), rstd.to(dev)
    for acc in (False, True):
        p_dg, p_db = _rand((C,), 402, 3.0), _rand((C,), 403, 3.0)
        dg, db = _sent((C + 8,), dev), _sent((C + 8,), dev)
        if acc:
            dg[:C], db[:C] = p_dg.to(dev), p_db.to(dev)
        scratch = torch.full((128 * C,), float("nan"), device=dev)
        ops.layernorm_bwd_affine(D, X, Mn, Rs, dg, db, scratch, M, C, accumulate=acc)
        what = f"layernorm_bwd_affine C={C} M={M} accumulate={acc}"
        _within(dg[:C], dg_ref + (p_dg.double() if acc else 0), dg_tol + (_ulp(p_dg) if acc else 0), f"{what}: dgamma")
        _within(db[:C], db_ref + (p_db.double() if acc else 0), db_tol + (_ulp(p_db) if acc else 0), f"{what}: dbeta")
        _intact(dg, C, what)
        _intact(db, C, what)
        assert not bool(torch.isnan(scratch).any()), f"{what}: a slab of the scratch was never written"


# --------------------------------------------------------------------------------------------------------------------- 5. the pooled head
def _head_ref(g, lg, lb, wh, bh, dl, B, T, C, K, r0, R, centre=None):
    """float64 head: LayerNorm of rows r0 .. r0+R of every sample (centred on `centre` [B][R] when given, else on the float64 mean), their mean,
    the linear layer; and its backward."""
    x = g.double().view(B, T, C)[:, r0: r0 + R]
    mu = x.mean(-1) if centre is None else centre
    d = x - mu[..., None]
    rs = ((d * d).mean(-1) + EPS).rsqrt()[..., None]
    xh = d * rs
    pooled = (xh * lg.double() + lb.double()).mean(1)
    logits = pooled @ wh.double().T + bh.double()
    dh = ((dl.double() @ wh.double()) / R)[:, None, :] * lg.double()
    dG = rs * (dh - dh.mean(-1, keepdim=True) - xh * (dh * xh).mean(-1, keepdim=True))
    return pooled, logits, dG, dl.double().T @ pooled, dl.double().sum(0)


def _close(got, want, rtol, what):
    """the bound of test_head_fwd_bwd: rtol of the tensor's maximum"""
    _within(got, want, rtol * max(1e-6, want.abs().max().item()), what)


def _run_head(dev, g, B, T, C, K, r0, R, what, centre=None, pooled_tol=2e-5):
    from gaviko_amd import ops
    lg, lb = _affine(C, 501)
    wh, bh, dl = _rand((K, C), 503, 0.1), _rand((K,), 504, 0.1), _rand((B, K), 505)
    pooled_ref, logits_ref, dG_ref, dwh_ref, dbh_ref = _head_ref(g, lg, lb, wh, bh, dl, B, T, C, K, r0, R, centre)
    t = lambda a: a.to(dev)
    lo_f, po_f = _sent((B * K + 8,), dev), _sent((B * C + 8,), dev)
    kw = dict(g=t(g), ln_gamma=t(lg), ln_beta=t(lb), wh=t(wh), bh=t(bh), B=B, T=T, C=C, K=K, r0=r0, R=R)
    ops.head_fwd(logits=lo_f[: B * K], pooled=po_f[: B * C], **kw)
    _within(po_f[: B * C].view(B, C), pooled_ref, pooled_tol, f"{what}: pooled")
    _close(lo_f[: B * K].view(B, K), logits_ref, 3e-5, f"{what}: logits")
    _intact(lo_f, B * K, f"{what}: logits")
    _intact(po_f, B * C, f"{what}: pooled")
    lo2 = _sent((B * K + 8,), dev)
    ops.head_fwd(logits=lo2[: B * K], **kw)                                            # pooled = NULL
    assert torch.equal(lo2, lo_f), f"{what}: pooled = None changed the logits"
    # ---- backward: dG pre-filled with the sentinel -- the rows outside r0 .. r0+R of every sample are NOT written (the engine zero-fills first)
    inside = torch.zeros(B, T, dtype=torch.bool)
    inside[:, r0: r0 + R] = True
    bw = dict(dlogits=t(dl), pooled=po_f[: B * C], **kw)
    dG, dwh_f, dbh_f = _sent((B * T + 2, C), dev), _sent((K * C + 8,), dev), _sent((K + 8,), dev)
    ops.head_bwd(dg=dG[: B * T], dwh=dwh_f[: K * C], dbh=dbh_f[:K], accumulate=0, **bw)
    got = dG[: B * T].cpu().view(B, T, C)
    _close(got[inside].view(B, R, C), dG_ref, 5e-5, f"{what}: dG")
    _within(got[inside].view(B, R, C), dG_ref, 5e-5 * _rowmax(dG_ref), f"{what}: dG (5e-5 of every row's own maximum)")
    assert bool((got[~inside] == SENT).all()), f"{what}: head_bwd wrote a row of dG outside r0 .. r0+R"
    _intact(dG, B * T, f"{what}: dG")
    _close(dwh_f[: K * C].view(K, C), dwh_ref, 5e-5, f"{what}: dwh")
    _close(dbh_f[:K], dbh_ref, 5e-5, f"{what}: dbh")
    _intact(dwh_f, K * C, f"{what}: dwh")
    _intact(dbh_f, K, f"{what}: dbh")
    dwh2, dbh2 = _sent((K * C + 8,), dev), _sent((K + 8,), dev)
    ops.head_bwd(dwh=dwh2[: K * C], dbh=dbh2[:K], accumulate=0, **bw)                 # dg = NULL (frozen backbone)
    assert torch.equal(dwh2, dwh_f) and torch.equal(dbh2, dbh_f), f"{what}: dg = None changed dwh / dbh"
    # ---- accumulate = 1: dwh / dbh += (one fp32 add onto the prior value, inside the 5e-5 of the sum's maximum); dG is written as before
    p_w, p_b = _rand((K, C), 506, 0.5), _rand((K,), 507, 0.5)
    dwh3, dbh3, dG3 = _sent((K * C + 8,), dev), _sent((K + 8,), dev), _sent((B * T + 2, C), dev)
    dwh3[: K * C], dbh3[:K] = t(p_w.flatten()), t(p_b)
    ops.head_bwd(dg=dG3[: B * T], dwh=dwh3[: K * C], dbh=dbh3[:K], accumulate=1, **bw)
    _close(dwh3[: K * C].view(K, C), dwh_ref + p_w.double(), 5e-5, f"{what}: dwh accumulate")
    _close(dbh3[:K], dbh_ref + p_b.double(), 5e-5, f"{what}: dbh accumulate")
    assert torch.equal(dG3, dG), f"{what}: accumulate = 1 changed dG"
    _intact(dwh3, K * C, f"{what}: dwh accumulate")
    _intact(dbh3, K, f"{what}: dbh accumulate")
    return po_f[: B * C].cpu().view(B, C), lb


@gpu
@pytest.mark.parametrize("B,T,C,K,r0,R", HEAD_CASES, ids=lambda v: str(v))
def test_head_fwd_bwd_edges(dev, B, T, C, K, r0, R):
    """R and K across the sixteen waves, C across the chunk edges, r0 > 0, r0 + R == T, pooled = None, dg = None, accumulate = 1, and a dG that
    starts as sentinels.  Inputs and bounds of test_head_fwd_bwd (logits 3e-5, gradients 5e-5 of the maximum); pooled as an fp32 LayerNorm output."""
    g = (_rand((B * T, C), 511, 3.0) + 0.5).contiguous()
    _run_head(dev, g, B, T, C, K, r0, R, f"head B={B} T={T} C={C} K={K} r0={r0} R={R}")


@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [4, 260, 1024])
def test_head_hard_rows(dev, C, kind):
    """The rows of section 1 as the pooled rows (B = 2, rows 5 .. 22 of 24).  The head's private LayerNorm is the code of ln_fwd_kernel, the same
    fp32 operations in the same order, and returns no mean: the float64 reference is centred on the mean gvk_layernorm_fwd returns for the same
    rows (itself held to 2e-6 above) -- if the head's own mean differed from it, pooled would miss its bound, which is the point."""
    from gaviko_amd import ops
    B, T, K, r0, R = 2, 24, 5, 5, 17
    g, _ = _hard(C, B * T, kind)
    lg, lb = _affine(C, 501)
    mean, rstd = _sent((B * T,), dev), _sent((B * T,), dev)
    ops.layernorm_fwd(g.to(dev), lg.to(dev), lb.to(dev), B * T, C, y32=torch.empty(B * T, C, device=dev), mean=mean, rstd=rstd)
    centre = mean.cpu().double().view(B, T)[:, r0: r0 + R]
    _run_head(dev, g, B, T, C, K, r0, R, f"head[{kind}] C={C}", centre=centre)


@gpu
@pytest.mark.parametrize("R", [1, 16, 17])
@pytest.mark.parametrize("C", [4, 260, 1024])
def test_head_constant_rows_pool_to_beta(dev, C, R):
    """All R pooled rows constant: every normalised row is ln_beta exactly.  pooled = (sum of R copies, in fp32) * (1 / R): with ln_beta on a
    2^-10 grid every partial sum is exact, so for R a power of two pooled == ln_beta bit for bit; for R = 17 the rounded 1 / R and the product
    are two roundings: within one ulp."""
    from gaviko_amd import ops
    B, K, r0 = 3, 5, 5
    T = r0 + R + 1
    g = (_rand((B * T, C), 521) + 0.3).view(B, T, C).clone()
    for b in range(B):
        for r in range(R):
            g[b, r0 + r] = CONST_VALUES[(b + r) % len(CONST_VALUES)]
    lg = 1 + _rand((C,), 522, 0.2)
    lb = torch.round(_rand((C,), 523, 0.9) * 1024) / 1024
    wh, bh = _rand((K, C), 524, 0.1), _rand((K,), 525, 0.1)
    t = lambda a: a.contiguous().to(dev)
    lo, po = _sent((B * K,), dev), _sent((B * C + 8,), dev)
    ops.head_fwd(g=t(g.view(B * T, C)), ln_gamma=t(lg), ln_beta=t(lb), wh=t(wh), bh=t(bh), logits=lo, pooled=po[: B * C], B=B, T=T, C=C, K=K, r0=r0, R=R)
    got = po[: B * C].cpu().view(B, C)
    if R & (R - 1) == 0:
        assert torch.equal(got, lb.expand(B, C)), f"pooled != ln_beta over {R} constant rows at C={C}"
    else:
        _within(got, lb.expand(B, C), _ulp(lb).expand(B, C), f"pooled over {R} constant rows at C={C}")
    _intact(po, B * C, "pooled")
    _close(lo.view(B, K), lb.double() @ wh.double().T + bh.double(), 3e-5, "logits of pooled = ln_beta")


# ---------------------------------------------------------------------------------------------------------------- 6. token assembly, exact
@gpu
@pytest.mark.parametrize("B,T,R,C", [(3, 50, 8, 196), (3, 301, 300, 768)], ids=["small", "grid_stride"])
def test_rows_broadcast_exact(dev, B, T, R, C):
    """out[b][row_off + r] = src[r] + add[r] (one fp32 add: bit-equal to the host's) or src[r] (add = None); every other element keeps the
    sentinel.  B R C = 691200 > 2048 * 256 elements in the second case: the grid-stride loop takes a second trip."""
    from gaviko_amd import ops
    src, add = _rand((R, C), 601), _rand((R, C), 602)
    n = B * T * C
    assert (B * R * C > 2048 * 256) == (R == 300)
    for row_off in sorted({0, 1, T - R}):
        for a in (add, None):
            out = _sent((n + 8,), dev)
            ops.rows_broadcast(out[:n], src.to(dev), None if a is None else a.to(dev), B, T, row_off, R, C)
            want = torch.full((n + 8,), SENT)
            want[:n].view(B, T, C)[:, row_off: row_off + R] = src if a is None else src + a
            assert torch.equal(out.cpu(), want), f"rows_broadcast row_off={row_off} add={'given' if a is not None else None}"


@gpu
@pytest.mark.parametrize("B,T,R,C", [(1, 50, 8, 196), (3, 50, 8, 196), (2, 701, 700, 768)], ids=["B1", "B3", "grid_stride"])
def test_rows_batch_sum_exact(dev, B, T, R, C):
    """out[r] (+)= sum_b dg[b][row_off + r], b ascending from 0, the prior value added last: bit-equal to the same fp32 additions on the host.
    out2 receives the same sum: identical to out when both start equal, independently right when they start different."""
    from gaviko_amd import ops
    dg = _rand((B, T, C), 611)
    n = R * C
    assert (n > 2048 * 256) == (R == 700)
    for row_off in sorted({0, 1, T - R}):
        s = torch.zeros(R, C)
        for b in range(B):
            s = s + dg[b, row_off: row_off + R]
        p1, p2 = _rand((R, C), 612, 2.0), _rand((R, C), 613, 2.0)
        for acc in (False, True):
            for second in (None, "equal", "different"):
                out, out2 = _sent((n + 8,), dev), _sent((n + 8,), dev)
                q2 = p1 if second == "equal" else p2
                if acc:
                    out[:n], out2[:n] = p1.flatten().to(dev), q2.flatten().to(dev)
                ops.rows_batch_sum(dg.view(B * T, C).to(dev), out[:n], None if second is None else out2[:n], B, T, row_off, R, C, accumulate=acc)
                what = f"rows_batch_sum B={B} row_off={row_off} accumulate={acc} out2={second}"
                assert torch.equal(out[:n].cpu().view(R, C), p1 + s if acc else s), f"{what}: out"
                _intact(out, n, what)
                if second is None:
                    assert torch.equal(out2[:n].cpu().view(R, C), q2 if acc else torch.full((R, C), SENT)), f"{what}: out2 = None was written"
                else:
                    assert torch.equal(out2[:n].cpu().view(R, C), q2 + s if acc else s), f"{what}: out2"
                    assert second != "equal" or torch.equal(out2, out), f"{what}: out2 != out"
                _intact(out2, n, what + " out2")


@gpu
def test_token_assembly_refusals(dev):
    from gaviko_amd import ops
    B, T, R, C = 2, 10, 4, 64
    src, dg = _rand((R, C), 621).to(dev), _rand((B * T, C), 622).to(dev)
    for row_off in (T - R + 1, -1):
        out, o1, o2 = _sent((B * T, C), dev), _sent((R, C), dev), _sent((R, C), dev)
        with pytest.raises(ops.L.GavikoHipError, match="gvk_rows_broadcast: bad arguments"):
            ops.rows_broadcast(out, src, src, B, T, row_off, R, C)
        with pytest.raises(ops.L.GavikoHipError, match="gvk_rows_batch_sum: bad arguments"):
            ops.rows_batch_sum(dg, o1, o2, B, T, row_off, R, C)
        torch.cuda.synchronize()
        assert bool((out == SENT).all()) and bool((o1 == SENT).all()) and bool((o2 == SENT).all()), "a refused call wrote an output"
