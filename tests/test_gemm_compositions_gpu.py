"""-m gpu: the GEMM descriptor's features in the COMBINATIONS the engine uses, every case against float64 on the CPU.

gvk_gemm_nt_bf16 / gvk_gemm_nt_f32 select among eleven tile forms, nine epilogues, free leading dimensions, strided row panels, dropout,
aux_is_grad, out0 = NULL and a contraction length shorter than the operand rows.  tests/test_kernels_gpu.py exercises each feature once,
alone; this module runs the products.  Every shape is tiny (M <= 256, N <= 320, K <= 448).

Conventions of every case (the helpers below enforce them):
  * outputs are [pad_rows(M)][ld] buffers filled with 7.0 before the call; rows >= M and columns N .. ld-1 must still hold 7.0 afterwards;
  * A's padding rows M .. pad_rows(M)-1 and the columns K .. ld-1 of A and W hold 1e4, and the result must equal, bit for bit, the run
    with contiguous zero-padded operands;
  * fp32 outputs:  |got - ref| <= 2e-4 max(1, max|ref|)                       (test_gemm_store_bf16_and_f32's bound)
    bf16 outputs:  |got - ref| <= 2^-8 |ref| + 2e-4 max(1, max|ref|)          (one rounding at twice its half-ulp + the accumulation term)
    GELU outputs:  2^-7 max(1, max|g|), 2^-6 max|want|, 6e-3                  (test_gemm_epilogues, test_gemm_gelu_derivative_stored_by_the_forward)
    fp32 GEMM:     atol 2e-5, rtol 1e-5                                       (test_gemm_f32_epilogues)
    dropout, kept: 2e-3 / 3e-2 / 4e-2 absolute                                (test_gemm_dropout_epilogues)
    row partials:  1e-5 max(1, max|ref|) -- the relative bound test_layernorm_folded_into_gemm puts on the row mean, which is the sum of
                   these partials / C; an fp32 sum of 64 terms is off by at most 64 * 2^-24 * sum|x| ~ 4e-6 sum|x|
  * every tile accumulates an element's products in the same order (k-tile by k-tile, two 32-wide MFMA steps each), so each tile's output
    is also compared bit for bit with the two-stage four-wave 128 x 128 tile.
Each check prints "gemmcomp <bound> <case> <error / bound>" before it asserts.

The row-panel cases (test_row_panels_as_the_engine_composes_them) follow the call sites of gaviko_amd/engine.py that splice _panels(...):

    _mlp_block_fwd (pk = panels or {}):
        self._gemm(ws["xn"], w[f"fc1{i}"], M, ws["pre"][si] if train else None, epilogue=ops.EPI_BIAS_GELU_BF16, out1=ws["act"],
                   bias=..., ldo=self.ldx, drop_p=pdrop, seed=..., seed_ptr=ws["seed"], aux_is_grad=int(gg), **pk)
        so = dict(epilogue=ops.EPI_BIAS_RES_F32_BF16, out1=ws["xg16"], stat_part=ws["spart"], stat_pivot=ws["stat"][si][2]) if stats_out
             else dict(epilogue=ops.EPI_BIAS_RES_F32)
        self._gemm(ws["act"], w[f"fc2{i}"], M, gout, bias=..., res=g1, K=self.ldx if up_in_fc2 else self.mlp, drop_p=pdrop, seed=...,
                   seed_ptr=ws["seed"], **so, **pk)
    _mlp_block_bwd (top):
        self._gemm(ws["dG16"], w[f"fc2{i}_t"], M, ws["dpre"], epilogue=ops.EPI_GELU_BWD_BF16, aux=ws["pre"][i], ldaux=self.ldx,
                   drop_p=pd_, seed=..., seed_ptr=ws["seed"], aux_is_grad=int(sv.get("pre_is_grad", False)), **top)
        self._gemm(ws["dpre"], w[f"fc1{i}_t"], M, ws["dx16b"] if dy16 else ws["dx32"],
                   epilogue=ops.EPI_STORE_BF16 if dy16 else ops.EPI_STORE_F32, **top)
    _attn_block_bwd (bot):
        self._gemm(ws["dqkv"], w[f"qkv{i}_t"], M, ws["dx16b"] if dy16 else ws["dx32"],
                   epilogue=ops.EPI_STORE_BF16 if dy16 else ops.EPI_STORE_F32, **bot)

(The engine asks for panels only while its dropout rate is 0; drop_p is still a keyword of those calls and dispatch_tile has a branch
for it -- the 64 x 64 fallback -- so the panel cases run it live as well.)
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import dropmask

pytestmark = pytest.mark.gpu

SENT, GARB = 7.0, 1.0e4
BF16, F32 = torch.bfloat16, torch.float32
P_DROP, SEED, WORD = 0.1, 9, 42

FOUR_WAVE = (64064, 64128, 128064, 128128, 3064128, 3096128, 3128128, 4064128)
EIGHT_PHASE = (8256256, 7256256)
ALL_TILES = FOUR_WAVE + (256256,) + EIGHT_PHASE
NO_DROP_BUILD = (3064128, 3096128, 3128128, 4064128, 256256) + EIGHT_PHASE
ALL_EPILOGUES = ("STORE_BF16", "BIAS_RES_F32", "BIAS_GELU_BF16", "PATCH_F32", "GELU_BWD_BF16", "STORE_F32", "BIAS_RES_F32_BF16", "BIAS_RELU_BF16",
                 "RELU_BWD_BF16")
# what each tile is built for: gemm_bf16.hip dispatch_tile (the four-wave tiles: every epilogue; 256256: three) and gemm8p_bf16.hip launch8p_var
BUILT = {t: set(ALL_EPILOGUES) for t in FOUR_WAVE}
BUILT[256256] = {"STORE_BF16", "BIAS_GELU_BF16", "GELU_BWD_BF16"}
for _t in EIGHT_PHASE:
    BUILT[_t] = {"STORE_BF16", "BIAS_RES_F32", "BIAS_GELU_BF16", "GELU_BWD_BF16", "STORE_F32"}
F32_OUT = ("BIAS_RES_F32", "PATCH_F32", "STORE_F32", "BIAS_RES_F32_BF16")


@functools.lru_cache(maxsize=None)
def _problem(M, N, K, f32=False):
    """Operands (bf16-rounded on the bf16 path) and the float64 product, computed once per shape and never modified."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + (7 if f32 else 0))
    q = (lambda x: x) if f32 else (lambda x: x.bfloat16().float())
    p = SimpleNamespace(M=M, N=N, K=K, f32=f32)
    p.a = q(torch.randn(M, K, generator=g))
    p.w = q(torch.randn(N, K, generator=g) / math.sqrt(K))
    p.bias = torch.randn(N, generator=g) * 0.5
    p.res = torch.randn(M, N, generator=g)
    p.aux = q(torch.randn(M, N, generator=g))
    p.pivot = torch.randn(M, generator=g)
    p.pos = torch.randn(M, N, generator=g) * 0.3                 # PATCH_F32 reads its first rows_in rows
    p.acc = p.a.double() @ p.w.double().T
    return p


_DEV_OPERANDS = {}


def _operands(dev, p, garbage):
    """A [pad_rows(M)][lda], W [N][ldw]: garbage = 1e4 in A's padding rows and in the columns K .. ld-1 of both; else contiguous, zero padding."""
    from gaviko_amd import ops
    key = (p.M, p.N, p.K, p.f32, garbage)
    if key not in _DEV_OPERANDS:
        adt = F32 if p.f32 else BF16
        xk = (16 if p.f32 else 64) if garbage else 0
        fill = GARB if garbage else 0.0
        A = torch.full((ops.pad_rows(p.M), p.K + xk), fill, dtype=adt, device=dev)
        A[:p.M, :p.K] = p.a.to(dev).to(adt)
        W = torch.full((p.N, p.K + xk), fill, dtype=adt, device=dev)
        W[:, :p.K] = p.w.to(dev).to(adt)
        _DEV_OPERANDS[key] = (A, W)
    return _DEV_OPERANDS[key]


def _launch(dev, p, epi, *, tile=0, garbage=True, xo=None, bias=True, inplace=False, out0_none=False, out1_none=False, stat=None, aux_is_grad=0,
            patch=None, drop=False, panels=None, raises=None):
    """One ops.gemm_nt call on fresh sentinel-filled outputs; returns the whole buffers on the CPU.  xo: extra columns of the output / res /
    aux rows (ldo = ldres = ldaux = N + xo).  patch: (rows_in, rows_out, row_off).  panels: (B, T).  raises: the call must be refused."""
    from gaviko_amd import ops
    M, N, K = p.M, p.N, p.K
    adt = F32 if p.f32 else BF16
    xo = (16 if p.f32 else 64) if xo is None else xo
    ldo = N if epi == "PATCH_F32" else N + xo
    ldx = N + xo
    A, W = _operands(dev, p, garbage)
    rows = ops.pad_rows(M)

    def sent(r, ld, dt):
        return torch.full((r, ld), SENT, dtype=dt, device=dev)

    def side(src, dt):                                           # a [rows][ldx] side operand whose padding is never to be read
        t = torch.full((rows, ldx), GARB, dtype=dt, device=dev)
        t[:M, :N] = src.to(dev).to(dt)
        return t

    out_dt = F32 if epi in F32_OUT else adt
    rows0 = ops.pad_rows((M // patch[0]) * patch[1]) if patch else rows
    out0 = None if out0_none else sent(rows0, ldo, out_dt)
    out1 = res = aux = pos = part = pivot = word = None
    rows_in = rows_out = row_off = 0
    if epi in ("BIAS_RES_F32", "BIAS_RES_F32_BF16"):
        if inplace:
            out0[:M, :N] = p.res.to(dev)
            res, ldres = out0, ldo
        else:
            res, ldres = side(p.res, F32), ldx
    else:
        ldres = ldx
    if epi in ("GELU_BWD_BF16", "RELU_BWD_BF16"):
        aux = side(p.aux, adt)
    if epi in ("BIAS_GELU_BF16", "BIAS_RES_F32_BF16"):
        out1 = sent(rows, ldo, adt)
    if patch:
        rows_in, rows_out, row_off = patch
        pos = p.pos[:rows_in].to(dev).contiguous()
        out1 = None if out1_none else sent(rows, N, F32)
    if stat:
        part = torch.full(((N // 64) * M * 2,), SENT, dtype=F32, device=dev)
        pivot = p.pivot.to(dev) if stat == "pivot" else None
    if drop:
        word = torch.tensor([WORD], dtype=torch.int64, device=dev)
    mp, ms = panels if panels else (0, 0)

    def call():
        ops.gemm_nt(A, W, M, out0, epilogue=getattr(ops, "EPI_" + epi), tile=tile, K=K, out1=out1, bias=p.bias.to(dev) if bias else None, res=res, aux=aux,
                    pos=pos, ldo=ldo, ldres=ldres, ldaux=ldx, rows_in=rows_in, rows_out=rows_out, row_off=row_off,
                    drop_p=P_DROP if drop else 0.0, seed=SEED, seed_ptr=word, stat_part=part, stat_pivot=pivot, m_panels=mp, m_stride=ms,
                    aux_is_grad=aux_is_grad)
        torch.cuda.synchronize()

    if raises:
        with pytest.raises(Exception, match=raises):
            call()
        torch.cuda.synchronize()
    else:
        call()
    return SimpleNamespace(out0=None if out0 is None else out0.cpu(), out1=None if out1 is None else out1.cpu(),
                           part=None if part is None else part.cpu().view(N // 64, M, 2), pivot=stat == "pivot", patch=patch)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same_bits(x, y, label):
    d = (_bits(x) != _bits(y)).nonzero()
    assert d.numel() == 0, f"{label}: {d.shape[0]} elements differ, the first at {tuple(d[0].tolist())}"


def _within(name, label, got, ref, bound):
    """|got - ref| <= bound (a tensor or a number), the ratio printed first; a miss names the first wrong element."""
    err = (got.double() - ref).abs()
    b = bound if torch.is_tensor(bound) else torch.full_like(err, float(bound))
    ratio = err / b
    print(f"gemmcomp {name} {label} {ratio.max().item():.4f}")
    bad = (~(err <= b)).nonzero()
    assert bad.numel() == 0, (f"{label}: {name} bound missed at {bad.shape[0]} elements, the first at {tuple(bad[0].tolist())}: got "
                              f"{got[tuple(bad[0])].item()!r}, want {ref[tuple(bad[0])].item()!r}; largest error / bound {ratio.max().item():.3f}")


def _b32(ref):
    return 2e-4 * max(1.0, ref.abs().max().item())


def _b16(ref):
    return 2.0 ** -8 * ref.abs() + 2e-4 * max(1.0, ref.abs().max().item())


def _f32_bound(ref):
    return 2e-5 + 1e-5 * ref.abs()


def _gelu_grad64(h):
    return 0.5 * (1 + torch.erf(h / 2 ** 0.5)) + h * torch.exp(-0.5 * h * h) / (2 * math.pi) ** 0.5


def _untouched(buf, keep, label):
    """Where the boolean map `keep` is set, buf must still hold the sentinel."""
    bad = (keep & (buf.float() != SENT)).nonzero()
    assert bad.numel() == 0, f"{label}: {bad.shape[0]} elements outside the result were stored, the first at {tuple(bad[0].tolist())}"


def _check_sentinels(p, o, label, live_rows=None):
    """Rows >= M (or outside the boolean row map live_rows) and columns >= N of every output keep the sentinel; PATCH_F32's out0 keeps it
    outside the rows the epilogue maps to."""
    M, N = p.M, p.N
    live = torch.ones(M, dtype=torch.bool) if live_rows is None else live_rows
    for name, buf in (("out0", o.out0), ("out1", o.out1)):
        if buf is None:
            continue
        keep = torch.ones(buf.shape, dtype=torch.bool)
        if name == "out0" and o.patch:
            rin, rout, off = o.patch
            m = torch.arange(M)
            keep[(m // rin) * rout + off + m % rin, :N] = False
        else:
            head = keep[:M]                                      # (a view: the assignment below lands in keep)
            head[live, :N] = False
        _untouched(buf, keep, f"{label} {name}")
    if o.part is not None:
        keep = torch.ones(o.part.shape, dtype=torch.bool)
        keep[:, live] = False
        _untouched(o.part, keep, f"{label} stat_part")
        assert bool((o.part[:, live] != SENT).any()), f"{label}: stat_part was not written"


def _check_values(p, epi, o, label, *, bias=True, aux_is_grad=0, drop=False):
    """Rows < M of every output against float64, at the bound of its kind (module docstring)."""
    M, N = p.M, p.N
    b = p.bias.double() if bias else torch.zeros(N, dtype=torch.float64)
    acc, pre = p.acc, p.acc + b
    aux = p.aux.double()
    mask = torch.from_numpy(dropmask.rows_mask(SEED + WORD, M, N, P_DROP)).double() if drop else None
    o0 = None if o.out0 is None else o.out0[:M, :N]
    o1 = None if o.out1 is None else o.out1[:M, :N]
    f32 = p.f32

    def plain(name, got, ref):                                   # a value stored once, no special function on the way
        if f32:
            _within("f32gemm", f"{label} {name}", got, ref, _f32_bound(ref))
        elif got.dtype == F32:
            _within("fp32", f"{label} {name}", got, ref, _b32(ref))
        else:
            _within("bf16", f"{label} {name}", got, ref, _b16(ref))

    def dropped(name, got, ref, kept_bound, exact, what):
        if f32:
            _within("f32gemm", f"{label} {name}", got, ref, _f32_bound(ref))
        else:
            _within(f"drop{kept_bound:g}", f"{label} {name}", got, ref, kept_bound)
        gone = mask == 0
        assert abs(gone.double().mean().item() - P_DROP) < 0.01
        assert torch.equal(got[gone].float(), exact[gone].float()), f"{label} {name}: a dropped element is not exactly {what}"

    if epi in ("STORE_BF16", "STORE_F32"):
        plain("out0", o0, pre)
    elif epi in ("BIAS_RES_F32", "BIAS_RES_F32_BF16"):
        if drop:
            dropped("out0", o0, p.res.double() + pre * mask, 2e-3, p.res, "the residual")
        else:
            plain("out0", o0, pre + p.res.double())
        if epi == "BIAS_RES_F32_BF16":
            if f32:
                _same_bits(o1, o0, f"{label}: out1 is out0")
            else:
                _same_bits(o1, o0.bfloat16(), f"{label}: out1 is the rounding of out0")
                plain("out1", o1, pre + p.res.double())
        if o.part is not None:
            x = o0.double() - (p.pivot.double()[:, None] if o.pivot else 0.0)
            xs = x.view(M, N // 64, 64)
            want = torch.stack([xs.sum(2).T, (xs * xs).sum(2).T], dim=2)              # [N / 64][M][2]
            for c, nm in ((0, "sum"), (1, "sumsq")):
                _within("partials", f"{label} {nm}", o.part[:, :, c], want[:, :, c], 1e-5 * max(1.0, want[:, :, c].abs().max().item()))
    elif epi == "BIAS_GELU_BF16":
        g = torch.nn.functional.gelu(pre)
        if o0 is not None:
            if aux_is_grad:
                _within("gelu'6e-3", f"{label} out0", o0, _gelu_grad64(pre), 6e-3)
            elif drop and not f32:
                _within("drop0.03", f"{label} out0", o0, pre, 3e-2)
            else:
                plain("out0", o0, pre)
        if drop:
            dropped("out1", o1, g * mask, 4e-2, torch.zeros(M, N), "0")
        elif f32:
            plain("out1", o1, g)
        else:
            _within("gelu2^-7", f"{label} out1", o1, g, 2.0 ** -7 * max(1.0, g.abs().max().item()))
    elif epi == "GELU_BWD_BF16":
        if aux_is_grad:
            plain("out0", o0, acc * aux)
        elif drop:
            dropped("out0", o0, acc * mask * _gelu_grad64(aux), 4e-2, torch.zeros(M, N), "0")
        elif f32:
            plain("out0", o0, acc * _gelu_grad64(aux))
        else:
            want = acc * _gelu_grad64(aux)
            _within("gelu'2^-6", f"{label} out0", o0, want, 2.0 ** -6 * want.abs().max().item())
    elif epi == "PATCH_F32":
        rin, rout, off = o.patch
        m = torch.arange(M)
        want = pre + p.pos[:rin].double()[m % rin]
        got = o.out0[(m // rin) * rout + off + m % rin, :N]
        plain("out0", got, want)
        if o1 is not None:
            _same_bits(o1, got, f"{label}: out1 is out0's rows")
    elif epi == "BIAS_RELU_BF16":
        plain("out0", o0, pre.clamp_min(0))
    elif epi == "RELU_BWD_BF16":
        plain("out0", o0, acc * (aux > 0))
    else:
        raise AssertionError(epi)


def _check_same_outputs(x, y, M, N, label):
    for name in ("out0", "out1"):
        bx, by = getattr(x, name), getattr(y, name)
        assert (bx is None) == (by is None)
        if bx is not None:
            rows = bx.shape[0] if x.patch and name == "out0" else M
            _same_bits(bx[:rows, :N], by[:rows, :N], f"{label} {name}")
    if x.part is not None:
        _same_bits(x.part, y.part, f"{label} stat_part")


def _run_case(dev, p, epi, label, *, tile=0, check_kw=None, **kw):
    """Garbage-padded run checked for values and sentinels, and bit for bit against the run on contiguous zero-padded operands."""
    o = _launch(dev, p, epi, tile=tile, garbage=True, **kw)
    _check_sentinels(p, o, label)
    _check_values(p, epi, o, label, **(check_kw or {}))
    clean = _launch(dev, p, epi, tile=tile, garbage=False, **kw)
    _check_same_outputs(o, clean, p.M, p.N, f"{label}: padding garbage reached the result")
    return o


# ---------------------------------------------------------------------------------------------------------------- 1. k-tile count sweep
_TWO_STAGE = {}


def _two_stage(dev, p, epi, key, **kw):
    """The same call on the two-stage four-wave 128 x 128 tile, once per case: every other tile must give the same bits."""
    k = (p.M, p.N, p.K, epi, key)
    if k not in _TWO_STAGE:
        _TWO_STAGE[k] = _launch(dev, p, epi, tile=128128, **kw)
    return _TWO_STAGE[k]


@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 448])
@pytest.mark.parametrize("tile", ALL_TILES)
def test_k_tile_count_sweep(dev, tile, K):
    """nt = K / 64 = 1, 2, 3, 4, 5, 7 k-tiles on every tile form: the prologue and the tail of the two-, three- and four-stage loops take
    their own path (and their own s_waitcnt immediates) for nt = 1 .. NS and nt > NS.  M = 1 and M = 200: a ragged last row tile at every
    tile height; the 96- and 256-row tiles reach past the 128-row padding of A (the clamp).  K = 64 is outside the eight-phase kernel's
    contract (K >= 128): the launcher must refuse it."""
    N = 256
    for M in (1, 200):
        p = _problem(M, N, K)
        for epi, bias in (("STORE_BF16", True), ("STORE_F32", False)):
            label = f"tile={tile} M={M} K={K} {epi}"
            if epi not in BUILT[tile]:
                continue
            if tile in EIGHT_PHASE and K < 128:
                o = _launch(dev, p, epi, tile=tile, bias=bias, raises="K >= 128")
                _check_sentinels_refused(p, o, {}, label)
                continue
            o = _run_case(dev, p, epi, label, tile=tile, bias=bias, check_kw=dict(bias=bias))
            _check_same_outputs(o, _two_stage(dev, p, epi, "sweep", bias=bias), M, N, f"{label}: differs from tile 128128")


# ------------------------------------------------------------------------------------- 2. tile x epilogue with free leading dimensions
VARIANTS = {
    "store_bf16": ("STORE_BF16", {}),
    "store_f32": ("STORE_F32", dict(bias=False)),
    "res": ("BIAS_RES_F32", {}),
    "res_inplace": ("BIAS_RES_F32", dict(inplace=True)),
    "res16": ("BIAS_RES_F32_BF16", {}),
    "res16_stat": ("BIAS_RES_F32_BF16", dict(stat="part", inplace=True)),
    "res16_stat_pivot": ("BIAS_RES_F32_BF16", dict(stat="pivot")),
    "gelu": ("BIAS_GELU_BF16", {}),
    "gelu_no_out0": ("BIAS_GELU_BF16", dict(out0_none=True)),
    "gelu_grad": ("BIAS_GELU_BF16", dict(aux_is_grad=1)),
    "gelu_bwd": ("GELU_BWD_BF16", dict(bias=False)),
    "gelu_bwd_grad": ("GELU_BWD_BF16", dict(bias=False, aux_is_grad=1)),
    "patch_off0": ("PATCH_F32", dict(patch=(50, 53, 0))),
    "patch_off1": ("PATCH_F32", dict(patch=(50, 53, 1))),
    "patch_off0_no_out1": ("PATCH_F32", dict(patch=(50, 53, 0), out1_none=True)),
    "patch_off1_no_out1": ("PATCH_F32", dict(patch=(50, 53, 1), out1_none=True)),
    "relu": ("BIAS_RELU_BF16", {}),
    "relu_bwd": ("RELU_BWD_BF16", dict(bias=False)),
}


def _check_kw(kw):
    return dict(bias=kw.get("bias", True), aux_is_grad=kw.get("aux_is_grad", 0), drop=kw.get("drop", False))


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("tile", ALL_TILES)
def test_tile_x_epilogue_with_free_leading_dimensions(dev, tile, variant):
    """M = 200, N = 256, K = 192 with lda = ldw = K + 64 and ldo = ldres = ldaux = N + 64 (PATCH_F32: ldo = N, its contract): every tile runs
    every epilogue it is built for, in every form the engine uses (in place / out of place, with and without the second output, the
    row partials with and without a pivot, aux_is_grad on both GEMMs of the MLP).  The 64 spare columns are where the engine keeps the
    GPA latents: they must keep the sentinel.  A tile asked for an epilogue it is not built for, and the row partials on a 64-column
    tile, must be refused with every output untouched."""
    M, N, K = 200, 256, 192
    p = _problem(M, N, K)
    epi, kw = VARIANTS[variant]
    label = f"tile={tile} {variant}"
    if epi not in BUILT[tile]:
        o = _launch(dev, p, epi, tile=tile, raises="not built|built for|stat_part", **kw)
        _check_sentinels_refused(p, o, kw, label)
        return
    if kw.get("stat") and tile % 1000 != 128:
        o = _launch(dev, p, epi, tile=tile, raises="stat_part", **kw)
        _check_sentinels_refused(p, o, kw, label)
        return
    o = _run_case(dev, p, epi, label, tile=tile, check_kw=_check_kw(kw), **kw)
    _check_same_outputs(o, _two_stage(dev, p, epi, variant, **kw), M, N, f"{label}: differs from tile 128128")
    if variant in ("gelu_no_out0", "gelu_grad"):                   # the activation does not depend on what out0 is asked to hold
        _same_bits(o.out1[:M, :N], _two_stage(dev, p, epi, "gelu").out1[:M, :N], f"{label}: out1 differs from the plain call's")


def _check_sentinels_refused(p, o, kw, label):
    """A refused call stored nothing (an in-place residual buffer keeps the residual it was given)."""
    for name, buf in (("out0", o.out0), ("out1", o.out1), ("stat_part", o.part)):
        if buf is None:
            continue
        keep = torch.ones(buf.shape, dtype=torch.bool)
        if name == "out0" and kw.get("inplace"):
            keep[:p.M, :p.N] = False
            assert torch.equal(buf[:p.M, :p.N], p.res), f"{label}: the refused call changed its in-place residual"
        _untouched(buf, keep, f"{label} (refused) {name}")


# -------------------------------------------------------------------------------- 3. row panels composed as the engine composes them
PANEL_CASES = {
    "fc1": ("BIAS_GELU_BF16", {}),
    "fc1_inference": ("BIAS_GELU_BF16", dict(out0_none=True)),
    "fc1_grad": ("BIAS_GELU_BF16", dict(aux_is_grad=1)),
    "fc1_dropout": ("BIAS_GELU_BF16", dict(drop=True)),
    "fc2": ("BIAS_RES_F32", {}),
    "fc2_dropout": ("BIAS_RES_F32", dict(drop=True)),
    "fc2_stats": ("BIAS_RES_F32_BF16", dict(stat="pivot")),
    "fc2_dgrad": ("GELU_BWD_BF16", dict(bias=False)),
    "fc2_dgrad_grad": ("GELU_BWD_BF16", dict(bias=False, aux_is_grad=1)),
    "fc2_dgrad_dropout": ("GELU_BWD_BF16", dict(bias=False, drop=True)),
    "dgrad_bf16": ("STORE_BF16", dict(bias=False)),
    "dgrad_f32": ("STORE_F32", dict(bias=False)),
}


@pytest.mark.parametrize("case", list(PANEL_CASES))
@pytest.mark.parametrize("N,K", [(256, 192), (256, 320), (192, 192), (192, 320)])
def test_row_panels_as_the_engine_composes_them(dev, N, K, case):
    """m_panels = 3, m_stride = 70 (M = 210) with every epilogue and keyword the engine passes beside _panels(...) (module docstring), with
    ldo = ldaux = N + 64 and K < lda.  tile = 0 as the engine leaves it: four stages of 64 x 128 at N = 256 (three k-tiles: fewer than its
    stages; five: more), the 64 x 64 fallback at N = 192 and under dropout.  The 64 rows of every panel carry the bits of the full launch
    on that tile, every other row keeps the sentinel, and the full launch meets the float64 bounds.  The row partials need 128-column
    tiles: at N = 192 they must be refused."""
    B, T = 3, 70
    M = B * T
    p = _problem(M, N, K)
    epi, kw = PANEL_CASES[case]
    label = f"panels N={N} K={K} {case}"
    if kw.get("stat") and N % 128 != 0:
        o = _launch(dev, p, epi, panels=(B, T), raises="stat_part", **kw)
        _check_sentinels_refused(p, o, kw, label)
        return
    tile = 4064128 if (N % 128 == 0 and not kw.get("drop")) else 64064
    full = _run_case(dev, p, epi, f"{label} (full launch, tile {tile})", tile=tile, check_kw=_check_kw(kw), **kw)
    part = _launch(dev, p, epi, panels=(B, T), **kw)
    live = torch.zeros(M, dtype=torch.bool)
    for b in range(B):
        live[b * T: b * T + 64] = True
    _check_sentinels(p, part, label, live_rows=live)
    for name in ("out0", "out1"):
        x, y = getattr(part, name), getattr(full, name)
        if x is not None:
            _same_bits(x[:M][live, :N], y[:M][live, :N], f"{label} {name}: panel rows differ from the full launch")
    if part.part is not None:
        _same_bits(part.part[:, live], full.part[:, live], f"{label} stat_part: panel rows differ from the full launch")


# ------------------------------------------------------------------------------ 4. dropout on every DROP instantiation, any leading dimension
@pytest.mark.parametrize("epi", ["BIAS_RES_F32", "BIAS_GELU_BF16", "GELU_BWD_BF16"])
@pytest.mark.parametrize("tile", [64064, 64128, 128064, 128128, "f32"])
def test_dropout_on_every_drop_build_and_any_ldo(dev, tile, epi):
    """The DROP instantiations of the four two-stage tiles (64 x 64 is what every N = 192 GEMM of an unfrozen vit-t16 runs) and the fp32
    GEMM's dropout epilogues, once with ldo = ldaux = N and once with N + 64.  The mask index is m * N + n whatever ldo is -- fc1 forward
    (ldo = ldx) and its dgrad must draw the same mask -- so both runs match the host's rebuild of the mask, drop exactly the same
    elements (to exactly the residual, or exactly 0) and agree bit for bit on the columns < N."""
    f32 = tile == "f32"
    M, K = 200, 128
    N = 192 if (f32 or tile % 1000 == 64) else 256
    p = _problem(M, N, K, f32)
    kw = dict(drop=True, bias=epi != "GELU_BWD_BF16")
    outs = []
    for xo in (0, 64):
        label = f"dropout tile={tile} {epi} ldo=N+{xo}"
        outs.append(_run_case(dev, p, epi, label, tile=0 if f32 else tile, xo=xo, check_kw=_check_kw(kw), **kw))
    _check_same_outputs(outs[0], outs[1], M, N, f"dropout tile={tile} {epi}: the result depends on ldo")


@pytest.mark.parametrize("tile", NO_DROP_BUILD)
def test_dropout_is_refused_where_it_is_not_built(dev, tile):
    """The multi-stage and 256-wide tiles have no DROP build; aux_is_grad and dropout exclude each other; the plain stores take no dropout."""
    p = _problem(200, 256, 128)
    for epi in ("BIAS_RES_F32", "BIAS_GELU_BF16", "GELU_BWD_BF16"):
        kw = dict(drop=True, bias=epi != "GELU_BWD_BF16")
        o = _launch(dev, p, epi, tile=tile, raises="unsupported tile|gemm8p|dropout|drop_p", **kw)
        _check_sentinels_refused(p, o, kw, f"dropout tile={tile} {epi}")
    o = _launch(dev, p, "BIAS_GELU_BF16", tile=64128, drop=True, aux_is_grad=1, raises="aux_is_grad")
    _check_sentinels_refused(p, o, {}, "dropout with aux_is_grad")
    o = _launch(dev, p, "STORE_BF16", tile=64128, drop=True, raises="drop_p")
    _check_sentinels_refused(p, o, {}, "dropout with STORE_BF16")


# ----------------------------------------------------------------------------------------------------- 5. fp32 GEMM leading dimensions
F32_VARIANTS = {k: v for k, v in VARIANTS.items() if not v[1].get("stat") and not v[1].get("aux_is_grad")}


@pytest.mark.parametrize("variant", list(F32_VARIANTS))
def test_gemm_f32_leading_dimensions(dev, variant):
    """gvk_gemm_nt_f32, every epilogue, M = 130, N = 128, K = 80 with lda = ldw = K + 16 and ldo = ldres = ldaux = N + 16 (PATCH_F32: ldo = N),
    the same sentinel and garbage-padding checks as on the bf16 path; exact-erf GELU, atol 2e-5 / rtol 1e-5."""
    M, N, K = 130, 128, 80
    p = _problem(M, N, K, True)
    epi, kw = F32_VARIANTS[variant]
    if kw.get("patch"):
        kw = dict(kw, patch=(65, 68, kw["patch"][2]))
    _run_case(dev, p, epi, f"f32 {variant}", check_kw=_check_kw(kw), **kw)


def test_gemm_f32_refuses_the_bf16_only_options(dev):
    p = _problem(130, 128, 80, True)
    for epi, kw, msg in (("BIAS_RES_F32_BF16", dict(stat="part"), "bf16-path"), ("BIAS_GELU_BF16", dict(aux_is_grad=1), "aux_is_grad"),
                         ("STORE_F32", dict(panels=(2, 65)), "row panels")):
        o = _launch(dev, p, epi, raises=msg, **kw)
        _check_sentinels_refused(p, o, kw, f"f32 {epi} {sorted(kw)}")
