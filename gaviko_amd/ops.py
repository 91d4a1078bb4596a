"""Host-side launchers: torch tensors in, C-ABI calls out (include/gaviko_hip.h).

Every wrapper validates device / dtype / contiguity / row padding on the host before launching --
a hand-written kernel never sees a shape it was not built for.  All launches go to torch's current HIP
stream, so they are capturable into a HIP graph with torch.cuda.graph().
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as L
from .lib import (EPI_BIAS_GELU_BF16, EPI_BIAS_RELU_BF16, EPI_BIAS_RES_F32, EPI_BIAS_RES_F32_BF16, EPI_GELU_BWD_BF16,  # noqa: F401
                  EPI_PATCH_F32, EPI_RELU_BWD_BF16, EPI_STORE_BF16, EPI_STORE_F32)

ROW_PAD = 128


def pad_rows(m: int) -> int:
    return (m + ROW_PAD - 1) // ROW_PAD * ROW_PAD


def act_zeros(m: int, c: int, dtype, device) -> torch.Tensor:
    """Activation matrix with rows padded to the MFMA panel height (padding rows stay finite)."""
    return torch.zeros((pad_rows(m), c), dtype=dtype, device=device)


def _chk(t, dtype, what, min_elems=0):
    if t is None:
        return
    if not t.is_cuda:
        raise L.GavikoHipError(f"{what}: tensor must live on the HIP device (no CPU path)")
    if t.dtype != dtype:
        raise L.GavikoHipError(f"{what}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise L.GavikoHipError(f"{what}: tensor must be contiguous")
    if t.numel() < min_elems:
        raise L.GavikoHipError(f"{what}: needs >= {min_elems} elements, has {t.numel()}")


def gemm_nt(a, w, M, out0, *, epilogue, out1=None, bias=None, res=None, aux=None, pos=None,
            lda=None, ldo=None, ldres=None, ldaux=None, rows_in=0, rows_out=0, row_off=0, tile=0, N=None, K=None,
            drop_p=0.0, seed=0, seed_ptr=None, scale_cols=0, col_scale=1.0, ln_mean=None, ln_rstd=None, ln_c1=None, stat_part=None, stat_pivot=None,
            m_panels=0, m_stride=0, splitk_ws=None, ksplit=0, aux_is_grad=0):
    """Y[M,N] = A[M,K] . W[N,K]^T with a fused epilogue.  The operand dtype picks the kernel: bf16 -> gvk_gemm_nt_bf16 (MFMA
    bf16, fp32 accumulate), fp32 -> gvk_gemm_nt_f32 (every 16-bit slot of the epilogue table then carries fp32).
    m_panels / m_stride (bf16): only the row tiles starting at rows 0, m_stride, 2 m_stride, ... are computed (gvk_gemm_desc)."""
    adt = a.dtype
    if adt not in (torch.bfloat16, torch.float32):
        raise L.GavikoHipError(f"gemm A: expected bf16 or fp32 operands, got {adt}")
    N = w.shape[0] if N is None else N
    K = w.shape[1] if K is None else K
    lda = a.shape[-1] if lda is None else lda
    ldw = w.shape[-1]
    ldo = N if ldo is None else ldo
    _chk(a, adt, "gemm A", pad_rows(M) * lda if lda == a.shape[-1] else 0)
    _chk(w, adt, "gemm W", N * ldw)
    out_dt = torch.float32 if epilogue in (EPI_BIAS_RES_F32, EPI_PATCH_F32, EPI_STORE_F32, EPI_BIAS_RES_F32_BF16) else adt
    _chk(out0, out_dt, "gemm out0")
    if out1 is not None:
        _chk(out1, torch.float32 if epilogue == EPI_PATCH_F32 else adt, "gemm out1")
    _chk(bias, torch.float32, "gemm bias", N)
    _chk(res, torch.float32, "gemm res")
    _chk(aux, adt, "gemm aux")
    _chk(pos, torch.float32, "gemm pos", rows_in * N)
    d = L.GemmDesc(L.ptr(a), L.ptr(w), L.ptr(out0), L.ptr(out1), L.ptr(bias), L.ptr(res), L.ptr(aux), L.ptr(pos),
                   L.ptr(seed_ptr) if (seed_ptr is not None and drop_p > 0) else None,
                   M, N, K, lda, ldw, ldo, (N if ldres is None else ldres), (N if ldaux is None else ldaux),
                   epilogue, rows_in, rows_out, row_off, tile, float(drop_p), int(seed), int(scale_cols), float(col_scale),
                   L.ptr(ln_mean), L.ptr(ln_rstd), L.ptr(ln_c1), L.ptr(stat_part), L.ptr(stat_pivot), int(m_panels), int(m_stride),
                   L.ptr(splitk_ws), 0 if splitk_ws is None else splitk_ws.numel() * splitk_ws.element_size(), int(ksplit), int(aux_is_grad))
    _chk(ln_mean, torch.float32, "gemm ln_mean", M)
    _chk(ln_rstd, torch.float32, "gemm ln_rstd", M)
    _chk(ln_c1, torch.float32, "gemm ln_c1", N)
    _chk(stat_part, torch.float32, "gemm stat_part", (N // 64) * M * 2)
    _chk(stat_pivot, torch.float32, "gemm stat_pivot", M)
    (L.launch.gvk_gemm_nt_f32 if adt == torch.float32 else L.launch.gvk_gemm_nt_bf16)(C.byref(d))


def cast_bf16(x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    _chk(x, torch.float32, "cast in")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _chk(out, torch.bfloat16, "cast out", x.numel())
    L.launch.gvk_cast_f32_bf16(x, out, x.numel())
    return out


def pack_split_bf16(a, dst, col0, rows, b=None, weight_side=False):
    """Split-bf16 packing (hi + lo) of a narrow fp32 operand into 3*ca + 2 spare K columns of a bf16 GEMM operand (gaviko_hip.h)."""
    _chk(a, torch.float32, "pack a", rows * a.shape[-1])
    _chk(dst, torch.bfloat16, "pack dst", rows * dst.shape[-1])
    _chk(b, torch.float32, "pack b", rows)
    L.launch.gvk_pack_split_bf16(a, a.shape[-1], b, dst, dst.shape[-1], col0, rows, int(weight_side))


def layernorm_fwd_fix(x, gamma, beta, M, C_, *, y16, mean, rstd, enh, lat, wup, T, P, L_, eps=1e-5):
    """LayerNorm forward (bf16 output) that first applies the previous layer's GPA prompt fix to rows (m % T) < P of x, in place."""
    _chk(x, torch.float32, "ln_fix x", M * C_)
    _chk(gamma, torch.float32, "ln_fix gamma", C_)
    _chk(beta, torch.float32, "ln_fix beta", C_)
    _chk(y16, torch.bfloat16, "ln_fix y16", M * C_)
    _chk(mean, torch.float32, "ln_fix mean", M)
    _chk(rstd, torch.float32, "ln_fix rstd", M)
    _chk(enh, torch.float32, "ln_fix enh", (M // T) * P * L_)
    _chk(lat, torch.float32, "ln_fix lat", M * L_)
    _chk(wup, torch.float32, "ln_fix wup", C_ * L_)
    L.launch.gvk_layernorm_fwd_fix(x, gamma, beta, y16, mean, rstd, M, C_, eps, enh, lat, wup, T, P, L_)


def prompt_up_fix(enh, lat, w, out, B, T, P, C_, L_):
    """out rows b*T + p (p < P) += (enh[b][p] - lat[b*T + p]) . w^T (gaviko_hip.h: gvk_prompt_up_fix)."""
    _chk(enh, torch.float32, "prompt_up_fix enh", B * P * L_)
    _chk(lat, torch.float32, "prompt_up_fix lat", B * T * L_)
    _chk(w, torch.float32, "prompt_up_fix w", C_ * L_)
    _chk(out, torch.float32, "prompt_up_fix out", B * T * C_)
    L.launch.gvk_prompt_up_fix(enh, lat, w, out, B, T, P, C_, L_)


def prompt_up_fix_stats(enh, lat, w, out, out16, part, mean, rstd, B, T, P, C_, L_, eps=1e-5, pivot=None):
    """prompt_up_fix + the bf16 copy of the fixed rows + mean / rstd of EVERY row from the fc2 GEMM's per-row partials (the first LayerNorm of
    the next layer is folded into its qkv projection; gaviko_hip.h: gvk_prompt_up_fix_stats)."""
    _chk(enh, torch.float32, "prompt_up_fix enh", B * P * L_)
    _chk(lat, torch.float32, "prompt_up_fix lat", B * T * L_)
    _chk(w, torch.float32, "prompt_up_fix w", C_ * L_)
    _chk(out, torch.float32, "prompt_up_fix out", B * T * C_)
    _chk(out16, torch.bfloat16, "prompt_up_fix out16", B * T * C_)
    nparts = L.load().gvk_gemm_stat_parts(C_)
    _chk(part, torch.float32, "prompt_up_fix part", nparts * B * T * 2)
    _chk(mean, torch.float32, "prompt_up_fix mean", B * T)
    _chk(rstd, torch.float32, "prompt_up_fix rstd", B * T)
    _chk(pivot, torch.float32, "prompt_up_fix pivot", B * T)
    L.launch.gvk_prompt_up_fix_stats(enh, lat, w, out, out16, part, nparts, pivot, mean, rstd, B, T, P, C_, L_, eps)


def copy_(dst: torch.Tensor, src: torch.Tensor) -> None:
    """Stream-ordered device copy of src into dst (same dtype, contiguous; dst may be larger): the library's copy kernel
    (gvk_copy_async), recorded into a launch plan like any other launch."""
    if dst.dtype != src.dtype or not dst.is_contiguous() or not src.is_contiguous() or dst.numel() < src.numel():
        raise L.GavikoHipError("copy_: need contiguous tensors of one dtype with dst at least as large as src")
    L.launch.gvk_copy_async(dst, src, src.numel() * src.element_size())


def to_operand(x: torch.Tensor, out: torch.Tensor = None, dtype=torch.bfloat16) -> torch.Tensor:
    """GEMM-operand form of an fp32 matrix: a bf16 copy (MFMA path) or, on the fp32 path, the matrix itself / an fp32 copy."""
    if dtype == torch.bfloat16:
        return cast_bf16(x, out)
    if out is None:
        return x
    copy_(out, x)
    return out


def transpose_operand(x: torch.Tensor, out: torch.Tensor = None, dtype=torch.bfloat16) -> torch.Tensor:
    """x f32 [rows, cols] -> [cols, rows] in the operand dtype."""
    if dtype == torch.bfloat16:
        return transpose_cast_bf16(x, out)
    _chk(x, torch.float32, "transpose in")
    rows, cols = x.shape
    if out is None:
        out = torch.empty((cols, rows), dtype=torch.float32, device=x.device)
    _chk(out, torch.float32, "transpose out", rows * cols)
    L.launch.gvk_transpose_f32(x, out, rows, cols)
    return out


def transpose_any(x: torch.Tensor, out: torch.Tensor, rows: int, cols: int) -> None:
    """out [cols][rows] = x[rows][cols]^T within one dtype (bf16 or fp32): operand transposes of the wgrad GEMMs."""
    if x.dtype != out.dtype or x.dtype not in (torch.bfloat16, torch.float32):
        raise L.GavikoHipError("transpose_any: x and out must both be bf16 or both fp32")
    _chk(x, x.dtype, "transpose_any x", rows * cols)
    _chk(out, x.dtype, "transpose_any out", rows * cols)
    (L.launch.gvk_transpose_f32 if x.dtype == torch.float32 else L.launch.gvk_transpose_bf16)(x, out, rows, cols)


def colsum_any(x, out, ones, zeros, junk, scratch, M, N, *, ld=None, rows_in=0, rows_out=0, row_off=0):
    """out[n] = sum_m x[m][n] for a bf16 / fp32 matrix (optionally through the PATCH row mapping): the column-sum half of gvk_ssf_colgrad."""
    ssf_colgrad(x, x, ones, zeros, junk, out, scratch, M, N, ld_dy=ld, ld_y=ld, rows_in=rows_in, rows_out=rows_out, row_off=row_off)


def memset_zero(t: torch.Tensor) -> None:
    """Stream-ordered zero fill: the library's fill kernel (gvk_memset_async), recorded into a launch plan like any other launch.
    The tensor must start 16-byte aligned and span a multiple of 4 bytes."""
    if not t.is_contiguous():
        raise L.GavikoHipError("memset_zero: tensor must be contiguous")
    L.launch.gvk_memset_async(t, 0, t.numel() * t.element_size())


def seed_advance(seed: torch.Tensor, inc: int) -> None:
    if seed.dtype != torch.int64 or seed.numel() != 1:
        raise L.GavikoHipError("seed_advance: the dropout epoch is one int64 device word")
    L.launch.gvk_seed_advance(seed, inc)


def scale_(t: torch.Tensor, alpha: float) -> None:
    _chk(t, torch.float32, "scale_")
    L.launch.gvk_scale_f32(t, alpha, t.numel())


def transpose_cast_bf16(x: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """x f32 [rows, cols] -> bf16 [cols, rows]."""
    _chk(x, torch.float32, "transpose_cast in")
    rows, cols = x.shape
    if out is None:
        out = torch.empty((cols, rows), dtype=torch.bfloat16, device=x.device)
    _chk(out, torch.bfloat16, "transpose_cast out", rows * cols)
    L.launch.gvk_transpose_cast_f32_bf16(x, out, rows, cols)
    return out


def patchify(img: torch.Tensor, out: torch.Tensor, patch) -> None:
    _chk(img, torch.float32, "patchify img")
    B, ch, D, H, W = img.shape
    if ch != 1:
        raise L.GavikoHipError("patchify: single-channel MRI volumes only (channels=1)")
    pd, ph, pw = patch
    n = (D // pd) * (H // ph) * (W // pw)
    if out.dtype == torch.float32:
        _chk(out, torch.float32, "patchify out", B * n * pd * ph * pw)
        L.launch.gvk_patchify_f32(img, out, B, D, H, W, pd, ph, pw)
        return
    _chk(out, torch.bfloat16, "patchify out", B * n * pd * ph * pw)
    L.launch.gvk_patchify_bf16(img, out, B, D, H, W, pd, ph, pw)


def unpatchify(dcols: torch.Tensor, out: torch.Tensor, patch, *, x=None, x0=None, alpha=1.0, beta=0.0, nsum=1) -> None:
    """The inverse index map of patchify with attribution arithmetic: out[b] = beta out[b] + sum_{j<nsum} alpha V(b nsum + j) (x[b] - x0[b]),
    V(s) the volume of the fp32 im2col rows of sample s (x None: no factor; x0 None: 0).  out / x / x0 f32 [B,1,D,H,W]."""
    _chk(out, torch.float32, "unpatchify out")
    B, ch, D, H, W = out.shape
    if ch != 1:
        raise L.GavikoHipError("unpatchify: single-channel volumes only (channels=1)")
    pd, ph, pw = patch
    _chk(dcols, torch.float32, "unpatchify dcols", B * int(nsum) * D * H * W)
    if x0 is not None and x is None:
        raise L.GavikoHipError("unpatchify: x0 without x")
    for t, n in ((x, "x"), (x0, "x0")):
        if t is not None:
            _chk(t, torch.float32, "unpatchify " + n, out.numel())
            if tuple(t.shape) != tuple(out.shape):
                raise L.GavikoHipError(f"unpatchify {n}: shape {tuple(t.shape)} != out {tuple(out.shape)}")
    L.launch.gvk_unpatchify_f32(dcols, out, x, x0, B, D, H, W, pd, ph, pw, int(nsum), float(alpha), float(beta))


def patch_reduce(vol: torch.Tensor, out: torch.Tensor, patch, absval=True) -> None:
    """out [B, D/pd, H/ph, W/pw] = per-patch sum of |vol| (absval) or of vol, vol f32 [B,1,D,H,W]."""
    _chk(vol, torch.float32, "patch_reduce vol")
    B, ch, D, H, W = vol.shape
    if ch != 1:
        raise L.GavikoHipError("patch_reduce: single-channel volumes only (channels=1)")
    pd, ph, pw = patch
    _chk(out, torch.float32, "patch_reduce out", B * (D // pd) * (H // ph) * (W // pw))
    L.launch.gvk_patch_reduce_f32(vol, out, B, D, H, W, pd, ph, pw, int(bool(absval)))


# ---- perturbation of the input volume at patch granularity (csrc/perturb.hip) ----
def _tab(t, what, n):
    """A per-output-sample int32 device table of exactly n entries (only dtype and length are checked: the values are the caller's
    contract, and the kernels clamp them rather than read out of bounds)."""
    if t is None:
        raise L.GavikoHipError(f"{what}: the table is required")
    _chk(t, torch.int32, what)
    if t.numel() != n:
        raise L.GavikoHipError(f"{what}: expected {n} int32 entries, got {tuple(t.shape)}")


def patch_rank(rel: torch.Tensor, rank: torch.Tensor = None) -> torch.Tensor:
    """rel f32 [S, N] -> rank i32 [S, N]: the position of every patch in the stable descending order of its row (the inverse permutation
    of torch.argsort(rel, descending=True, stable=True)).  NaN is not ordered: the caller rejects it."""
    _chk(rel, torch.float32, "patch_rank rel")
    if rel.dim() != 2 or rel.shape[0] < 1 or rel.shape[1] < 1:
        raise L.GavikoHipError(f"patch_rank rel: expected [S, N], got {tuple(rel.shape)}")
    S, N = rel.shape
    if N > 16384:
        raise L.GavikoHipError(f"patch_rank: N = {N} patches exceed the 16384 one workgroup keeps in LDS")
    if rank is None:
        rank = torch.empty((S, N), dtype=torch.int32, device=rel.device)
    _chk(rank, torch.int32, "patch_rank rank")
    if tuple(rank.shape) != (S, N):
        raise L.GavikoHipError(f"patch_rank rank: shape {tuple(rank.shape)} != rel {tuple(rel.shape)}")
    L.launch.gvk_patch_rank(rel, rank, S, N)
    return rank


def patch_mask_rank(rank: torch.Tensor, src: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, mask: torch.Tensor) -> None:
    """mask u8 [Bout, N] = lo[o] <= rank[src[o], n] < hi[o]; rank i32 [S, N], src / lo / hi i32 [Bout] device tables (src within [0, S))."""
    _chk(rank, torch.int32, "patch_mask_rank rank")
    _chk(mask, torch.uint8, "patch_mask_rank mask")
    if rank.dim() != 2 or mask.dim() != 2 or mask.shape[1] != rank.shape[1] or mask.shape[0] < 1:
        raise L.GavikoHipError(f"patch_mask_rank: expected rank [S, N] and mask [Bout, N], got {tuple(rank.shape)} and {tuple(mask.shape)}")
    Bout, N = mask.shape
    for t, n in ((src, "src"), (lo, "lo"), (hi, "hi")):
        _tab(t, "patch_mask_rank " + n, Bout)
    L.launch.gvk_patch_mask_rank(rank, src, lo, hi, mask, Bout, rank.shape[0], N)


def patch_mask_box(boxes: torch.Tensor, mask: torch.Tensor, grid) -> None:
    """mask u8 [Bout, N] = patch inside boxes[o] = (d0, d1, h0, h1, w0, w1), half-open, in units of the patch grid `grid` = (nd, nh, nw);
    boxes i32 [Bout, 6] device table."""
    nd, nh, nw = (int(g) for g in grid)
    _chk(mask, torch.uint8, "patch_mask_box mask")
    if mask.dim() != 2 or mask.shape[0] < 1 or mask.shape[1] != nd * nh * nw or min(nd, nh, nw) < 1:
        raise L.GavikoHipError(f"patch_mask_box: expected mask [Bout, {nd * nh * nw}] for the grid {(nd, nh, nw)}, got {tuple(mask.shape)}")
    _tab(boxes, "patch_mask_box boxes", mask.shape[0] * 6)
    L.launch.gvk_patch_mask_box(boxes, mask, mask.shape[0], nd, nh, nw)


def perturb_volume(x: torch.Tensor, mask: torch.Tensor, src: torch.Tensor, out: torch.Tensor, patch, *, fill_scalar=None, base=None) -> None:
    """out[o] = where(mask[o] upsampled to the voxels, fill, x[src[o]]), bit for bit.  x f32 [S,1,D,H,W], out f32 [Bout,1,D,H,W] (not
    overlapping x), mask u8 [Bout, N], src i32 [Bout] (within [0, S)); fill: fill_scalar f32 [S] (one value per source) or base f32
    [1 or S,1,D,H,W] (a baseline volume, shared or one per source)."""
    _chk(x, torch.float32, "perturb_volume x")
    _chk(out, torch.float32, "perturb_volume out")
    if x.dim() != 5 or out.dim() != 5 or x.shape[1] != 1 or tuple(out.shape[1:]) != tuple(x.shape[1:]) or x.shape[0] < 1 or out.shape[0] < 1:
        raise L.GavikoHipError(f"perturb_volume: expected x [S,1,D,H,W] and out [Bout,1,D,H,W], got {tuple(x.shape)} and {tuple(out.shape)}")
    S, _, D, H, W = x.shape
    Bout = out.shape[0]
    pd, ph, pw = (int(p) for p in patch)
    if min(pd, ph, pw) < 1 or D % pd or H % ph or W % pw:
        raise L.GavikoHipError(f"perturb_volume: volume {D}x{H}x{W} not divisible by patch {pd}x{ph}x{pw}")
    N = (D // pd) * (H // ph) * (W // pw)
    _chk(mask, torch.uint8, "perturb_volume mask")
    if tuple(mask.shape) != (Bout, N):
        raise L.GavikoHipError(f"perturb_volume mask: expected [{Bout}, {N}], got {tuple(mask.shape)}")
    _tab(src, "perturb_volume src", Bout)
    if (fill_scalar is None) == (base is None):
        raise L.GavikoHipError("perturb_volume: exactly one of fill_scalar and base")
    nbase = 0
    if fill_scalar is not None:
        _chk(fill_scalar, torch.float32, "perturb_volume fill_scalar")
        if fill_scalar.numel() != S:
            raise L.GavikoHipError(f"perturb_volume fill_scalar: expected {S} values (one per source), got {tuple(fill_scalar.shape)}")
    else:
        _chk(base, torch.float32, "perturb_volume base")
        if base.dim() != 5 or tuple(base.shape[1:]) != tuple(x.shape[1:]) or base.shape[0] not in (1, S):
            raise L.GavikoHipError(f"perturb_volume base: expected [1 or {S}, 1, {D}, {H}, {W}], got {tuple(base.shape)}")
        nbase = base.shape[0]
    xe, oe = x.data_ptr() + x.numel() * 4, out.data_ptr() + out.numel() * 4
    if not (oe <= x.data_ptr() or xe <= out.data_ptr()):
        raise L.GavikoHipError("perturb_volume: out must not overlap x")
    if base is not None and not (oe <= base.data_ptr() or base.data_ptr() + base.numel() * 4 <= out.data_ptr()):
        raise L.GavikoHipError("perturb_volume: out must not overlap base")
    if Bout * D * H * W >= 1 << 31:
        raise L.GavikoHipError(f"perturb_volume: {Bout} x {D * H * W} voxels per launch exceed the kernel's 32-bit index range")
    L.launch.gvk_perturb_volume(x, mask, src, fill_scalar, base, nbase, out, Bout, S, D, H, W, pd, ph, pw)


def perturb_scores(logits: torch.Tensor, src: torch.Tensor, target: torch.Tensor, slot: torch.Tensor, prob: torch.Tensor, logit: torch.Tensor,
                   rows: torch.Tensor = None) -> None:
    """For every output sample o with slot[o] >= 0: prob.flat[slot[o]] = softmax(logits[o])[target[src[o]]], logit.flat[slot[o]] = that logit,
    rows.view(-1, K)[slot[o]] = logits[o] (optional).  logits f32 [Bout, K]; src / slot i32 [Bout], target i32 [S] device tables (target
    within [0, K)).  prob = logit = None (then src and target are not read): the rows only."""
    _chk(logits, torch.float32, "perturb_scores logits")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise L.GavikoHipError(f"perturb_scores logits: expected [Bout, K], got {tuple(logits.shape)}")
    Bout, K = logits.shape
    _tab(slot, "perturb_scores slot", Bout)
    if (prob is None) != (logit is None) or (prob is None and rows is None):
        raise L.GavikoHipError("perturb_scores: prob and logit go together, and without them rows is required")
    if prob is not None:
        if target is None:
            raise L.GavikoHipError("perturb_scores: prob / logit need a target table")
        _tab(src, "perturb_scores src", Bout)
        _chk(target, torch.int32, "perturb_scores target", 1)
        _chk(prob, torch.float32, "perturb_scores prob", 1)
        _chk(logit, torch.float32, "perturb_scores logit", 1)
    nslots = prob.numel() if prob is not None else rows.numel() // K
    _chk(rows, torch.float32, "perturb_scores rows", K)
    if (logit is not None and logit.numel() != nslots) or (rows is not None and rows.numel() != nslots * K):
        raise L.GavikoHipError(f"perturb_scores: {nslots} slots; logit needs as many and rows {nslots} x {K}")
    S = target.numel() if prob is not None else 0
    L.launch.gvk_perturb_scores(logits, src if prob is not None else None, target if prob is not None else None, slot, prob, logit, rows, Bout, S, K, nslots)


def curve_auc(prob: torch.Tensor, ks: torch.Tensor, N: int, auc: torch.Tensor = None) -> torch.Tensor:
    """prob f32 [S, P], ks i32 [P] (device) -> auc f32 [S]: the trapezoid area of every curve over x = ks / N."""
    _chk(prob, torch.float32, "curve_auc prob")
    if prob.dim() != 2 or prob.shape[0] < 1 or prob.shape[1] < 1 or int(N) < 1:
        raise L.GavikoHipError(f"curve_auc: expected prob [S, P] and N >= 1, got {tuple(prob.shape)} and N = {N}")
    S, P = prob.shape
    _tab(ks, "curve_auc ks", P)
    if auc is None:
        auc = torch.empty(S, dtype=torch.float32, device=prob.device)
    _chk(auc, torch.float32, "curve_auc auc", S)
    L.launch.gvk_curve_auc(prob, ks, auc, S, P, int(N))
    return auc


def layernorm_fwd(x, gamma, beta, M, C_, *, y16=None, y32=None, mean=None, rstd=None, eps=1e-5):
    if y16 is not None and y16.dtype == torch.float32:       # fp32 compute path: the "operand" output is fp32
        y16, y32 = None, y16
    _chk(x, torch.float32, "ln x", M * C_)
    _chk(gamma, torch.float32, "ln gamma", C_)
    _chk(beta, torch.float32, "ln beta", C_)
    _chk(y16, torch.bfloat16, "ln y16", M * C_)
    _chk(y32, torch.float32, "ln y32", M * C_)
    _chk(mean, torch.float32, "ln mean", M)
    _chk(rstd, torch.float32, "ln rstd", M)
    L.launch.gvk_layernorm_fwd(x, gamma, beta, y16, y32, mean, rstd, M, C_, eps)


ROWPROJ_L = 20      # default latent width (configs/gaviko.yaml prompt_latent_dim)


def side_tile_supported(L_: int, C_: int) -> bool:
    """Shapes the 16-row-tile fp32-MFMA projections (csrc/sidepass.hip) cover -- and with them the second projection fused into
    gvk_skinny_up (w2 / z2 / y2) and the chained layer-boundary forms.  Mirrors the C side exactly (sidepass.hip: kSL = 20,
    groups_per_wave(C) != 0 only for C in {192, 768, 1024}); any other latent width or channel count runs the generic
    row-per-wave / MFMA-tile kernels of rowwise.hip / skinny.hip without the fusions."""
    return str(L.diag_env("GAVIKO_HIP_SIDE", "1"))[:1] != "0" and L_ == 20 and C_ in (192, 768, 1024)


def rowproj_supported(L_: int, C_: int) -> bool:
    """Shapes the fused LayerNorm+projection kernels (row-per-wave form) cover."""
    return L_ in (4, 8, 16, 20) and C_ % 4 == 0 and 128 <= C_ <= 1024


def _rowproj(M, C_, w, y, bias, z, L_, w_layout, act, y_split=None, col_split=0):
    _chk(w, torch.float32, "rowproj w", L_ * C_)
    _chk(y, torch.float32, "rowproj y", M * L_)
    _chk(bias, torch.float32, "rowproj bias", L_)
    _chk(z, torch.float32, "rowproj z", M * L_)
    _chk(y_split, torch.bfloat16, "rowproj y_split", 0 if y_split is None else M * y_split.shape[-1])
    return L.RowProjDesc(w=L.ptr(w), bias=L.ptr(bias), y=L.ptr(y), z=L.ptr(z), y_split=L.ptr(y_split), L=L_, w_layout=w_layout, act=act,
                         ld_split=0 if y_split is None else y_split.shape[-1], col_split=col_split)


def layernorm_fwd_proj(x, gamma, beta, M, C_, *, y16, mean=None, rstd=None, eps=1e-5, w, y, bias=None, z=None, L_=ROWPROJ_L, w_layout=0, act=0,
                       y_split=None, col_split=0):
    """LayerNorm forward + rank-L projection of the raw input rows (one pass over x)."""
    _chk(x, torch.float32, "ln x", M * C_)
    _chk(gamma, torch.float32, "ln gamma", C_)
    _chk(beta, torch.float32, "ln beta", C_)
    _chk(y16, torch.bfloat16, "ln y16", M * C_)
    _chk(mean, torch.float32, "ln mean", M)
    _chk(rstd, torch.float32, "ln rstd", M)
    d = _rowproj(M, C_, w, y, bias, z, L_, w_layout, act, y_split, col_split)
    L.launch.gvk_layernorm_fwd_proj(x, gamma, beta, y16, mean, rstd, M, C_, eps, C.byref(d))


def layernorm_bwd_up(dy, x, mean, rstd, gamma, M, C_, *, dx, dres, dx16, lat, w, L_, w_layout):
    """dx = dres + LN'(dy) + lat . W^T (+ bf16 copy): the MLP block's LayerNorm backward and GPA's dG1 += dzx . W_d in one pass."""
    for t, n in ((dy, "dy"), (x, "x"), (dx, "dx"), (dres, "dres")):
        _chk(t, torch.float32, "ln_bwd_up " + n, M * C_)
    _chk(dx16, torch.bfloat16, "ln_bwd_up dx16", M * C_)
    _chk(mean, torch.float32, "ln_bwd_up mean", M)
    _chk(rstd, torch.float32, "ln_bwd_up rstd", M)
    _chk(gamma, torch.float32, "ln_bwd_up gamma", C_)
    _chk(lat, torch.float32, "ln_bwd_up lat", M * L_)
    _chk(w, torch.float32, "ln_bwd_up w", L_ * C_)
    L.launch.gvk_layernorm_bwd_up(dy, x, mean, rstd, gamma, dres, dx, dx16, lat, w, w_layout, M, C_, L_)


def layernorm_bwd(dy, x, mean, rstd, gamma, M, C_, *, dx, dres=None, dx16=None, rows=None, proj=None):
    """dx = dres + LN'(dy) (+ bf16 copy dx16); dy in fp32 or bf16 (its dtype selects the kernel).  rows = (groups, rows_per_group, group_stride)
    restricts it to the first rows_per_group rows of every group of group_stride rows (every sample's leading tokens); the other rows of
    dx / dx16 are left as they are.  proj = dict(w=, y=, L_=, w_layout=) adds the rank-L projection y = dx . W of the output rows."""
    if rows is not None and proj is not None:
        raise L.GavikoHipError("ln_bwd: the projection form covers all rows (rows and proj are exclusive)")
    if dx16 is not None and dx16.dtype == torch.float32 and rows is None:     # fp32 compute path: the operand copy is a plain copy of dx
        layernorm_bwd(dy, x, mean, rstd, gamma, M, C_, dx=dx, dres=dres, proj=proj)
        copy_(dx16, dx)
        return
    dy_bf16 = dy.dtype == torch.bfloat16
    _chk(dy, torch.bfloat16 if dy_bf16 else torch.float32, "ln_bwd dy", M * C_)
    for t, n in ((x, "x"), (dx, "dx")):
        _chk(t, torch.float32, "ln_bwd " + n, M * C_)
    _chk(dres, torch.float32, "ln_bwd dres", M * C_)
    _chk(dx16, torch.bfloat16, "ln_bwd dx16", M * C_)
    _chk(mean, torch.float32, "ln_bwd mean", M)
    _chk(rstd, torch.float32, "ln_bwd rstd", M)
    _chk(gamma, torch.float32, "ln_bwd gamma", C_)
    g, rpg, gs = rows if rows is not None else (0, 0, 0)
    pj = None
    if proj is not None:
        pj = _rowproj(M, C_, proj["w"], proj["y"], None, None, proj.get("L_", ROWPROJ_L), proj.get("w_layout", 1), 0)
    d = L.LnBwdDesc(L.ptr(dy), L.ptr(x), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), L.ptr(dres), L.ptr(dx), L.ptr(dx16),
                    C.cast(C.pointer(pj), C.c_void_p) if pj is not None else None, M, C_, int(g), int(rpg), int(gs), int(dy_bf16))
    L.launch.gvk_layernorm_bwd(C.byref(d))


def layernorm_bwd_affine(dy, x, mean, rstd, dgamma, dbeta, scratch, M, C_, accumulate=False):
    for t, n in ((dy, "dy"), (x, "x")):
        _chk(t, torch.float32, "ln_affine " + n, M * C_)
    _chk(dgamma, torch.float32, "ln_affine dgamma", C_)
    _chk(dbeta, torch.float32, "ln_affine dbeta", C_)
    _chk(scratch, torch.float32, "ln_affine scratch", 128 * C_)
    L.launch.gvk_layernorm_bwd_affine(dy, x, mean, rstd, dgamma, dbeta, scratch, M, C_, int(accumulate))


LOG2E = 1.4426950408889634


def qkv_prescale(qkv, rows, H, scale):
    """In place: q block of a raw bf16 to_qkv output -> q * scale * log2(e), the form the bf16 attention kernels take (the engine gets it from the
    qkv projection's epilogue instead: gemm_nt(scale_cols=H*64, col_scale=scale*LOG2E))."""
    _chk(qkv, torch.bfloat16, "qkv_prescale qkv", rows * 3 * H * 64)
    L.launch.gvk_qkv_prescale_bf16(qkv, rows, H, qkv.shape[-1], scale)


def _prescaled_copy(qkv, rows, H, scale):
    c = qkv.clone()
    qkv_prescale(c, rows, H, scale)
    return c


def attention_fwd(qkv, out, lse, B, T, H, scale, drop_p=0.0, seed=0, seed_ptr=None, q_prescaled=False):
    """qkv bf16 [pad(B*T), 3*H*64] -> out bf16 [pad(B*T), H*64], lse f32 [B,H,T].  drop_p > 0: dropout on the probabilities (bf16 path).
    bf16 path: the kernels take the q block pre-scaled by scale*log2(e) (include/gaviko_hip.h); q_prescaled=False (tests, tools) makes a
    scaled copy of a raw qkv first -- an allocation and one more rounding of q, never on the engine's path."""
    inner, f32, drop = H * 64, qkv.dtype == torch.float32, drop_p > 0
    dt, rows = (torch.float32, B * T) if f32 else (torch.bfloat16, pad_rows(B * T))
    for t, n, dtype, elems in ((qkv, "qkv", dt, rows * 3 * inner), (out, "out", dt, B * T * inner), (lse, "lse", torch.float32, B * H * T)):
        _chk(t, dtype, "attn " + n, elems)
    if not f32 and not q_prescaled:
        qkv = _prescaled_copy(qkv, B * T, H, scale)
    d = L.AttentionDesc(qkv=L.ptr(qkv), out=L.ptr(out), lse=L.ptr(lse), seed_ptr=L.ptr(seed_ptr) if drop else None, B=B, T=T, H=H,
                        ld_qkv=3 * inner, ld_out=inner, f32=int(f32), scale=scale, drop_p=float(drop_p), seed=int(seed) if drop else 0)
    L.launch.gvk_attention_fwd(C.byref(d))


def attention_colsum(qkv, lse, w, out, B, T, H, q0=0, q1=None):
    """out f32 [B,H,T] = sum_{q0 <= i < q1} w[b,i] * P[b,h,i,:] -- the weighted rows of the attention probabilities, recomputed from the
    bf16 forward's qkv (q block pre-scaled, gvk_attention_desc's layout) and lse f32 [B,H,T].  w f32 [B, >= T] (row stride = its last dim)."""
    q1 = T if q1 is None else q1
    _chk(qkv, torch.bfloat16, "colsum qkv", pad_rows(B * T) * 3 * H * 64)
    _chk(lse, torch.float32, "colsum lse", B * H * T)
    _chk(out, torch.float32, "colsum out", B * H * T)
    _chk(w, torch.float32, "colsum w", B * T)
    ld_w = w.shape[-1] if w.dim() == 2 else T
    if ld_w < T or w.numel() < B * ld_w:
        raise L.GavikoHipError(f"colsum w: expected [B, >= T] = [{B}, >= {T}], got {tuple(w.shape)}")
    if not 0 <= q0 < q1 <= T:
        raise L.GavikoHipError(f"colsum: query rows [{q0}, {q1}) outside [0, {T})")
    L.launch.gvk_attention_colsum_bf16(qkv, lse, w, ld_w, out, B, T, H, 3 * H * 64, int(q0), int(q1))


def rollout_step(r_in, colsum, r_out, B, T, H):
    """r_out f32 [B,T] = 0.5 r_in + (0.5 / H) sum_h colsum[:, h] (r_out may be r_in)."""
    _chk(r_in, torch.float32, "rollout r_in", B * T)
    _chk(r_out, torch.float32, "rollout r_out", B * T)
    _chk(colsum, torch.float32, "rollout colsum", B * H * T)
    L.launch.gvk_rollout_step(r_in, colsum, r_out, B, T, H)


def attention_gradcolsum(qkv, lse, dctx, w, out, B, T, H, q0=0, q1=None):
    """out f32 [B,H,T] = sum_{q0 <= i < q1} w[b,i] * P[b,h,i,:] * max(0, dP[b,h,i,:]), dP = dO . v^T -- gradient x attention, recomputed
    from the bf16 forward's qkv / lse (attention_colsum's operands) and the backward sweep's dctx bf16 [pad(B*T), H*64] (= dO)."""
    q1 = T if q1 is None else q1
    _chk(qkv, torch.bfloat16, "gradcolsum qkv", pad_rows(B * T) * 3 * H * 64)
    _chk(dctx, torch.bfloat16, "gradcolsum dctx", pad_rows(B * T) * H * 64)
    _chk(lse, torch.float32, "gradcolsum lse", B * H * T)
    _chk(out, torch.float32, "gradcolsum out", B * H * T)
    _chk(w, torch.float32, "gradcolsum w", B * T)
    ld_w = w.shape[-1] if w.dim() == 2 else T
    if ld_w < T or w.numel() < B * ld_w:
        raise L.GavikoHipError(f"gradcolsum w: expected [B, >= T] = [{B}, >= {T}], got {tuple(w.shape)}")
    if not 0 <= q0 < q1 <= T:
        raise L.GavikoHipError(f"gradcolsum: query rows [{q0}, {q1}) outside [0, {T})")
    L.launch.gvk_attention_gradcolsum_bf16(qkv, lse, dctx, H * 64, w, ld_w, out, B, T, H, 3 * H * 64, int(q0), int(q1))


def relevance_step(r_in, cs, r_out, B, T, H):
    """r_out f32 [B,T] = r_in + (1 / H) sum_h cs[:, h] (cs f32 [B,H,T], attention_gradcolsum's output; r_out may be r_in)."""
    _chk(r_in, torch.float32, "relevance r_in", B * T)
    _chk(r_out, torch.float32, "relevance r_out", B * T)
    _chk(cs, torch.float32, "relevance cs", B * H * T)
    L.launch.gvk_relevance_step(r_in, cs, r_out, B, T, H)


def _desc(cls, what, **kw):
    """Fill a descriptor struct: tensors -> device pointers (validated fp32, contiguous, on device), None -> NULL."""
    d = cls()
    for name, ctype in cls._fields_:
        v = kw.pop(name, None)
        if ctype is C.c_void_p:
            if v is not None:
                _chk(v, torch.int64 if name == "seed_ptr" else torch.bfloat16 if name in ("out_bf16", "enh16") else torch.float32, f"{what}.{name}")
            setattr(d, name, L.ptr(v))
        elif v is not None:
            setattr(d, name, v)
    if kw:
        raise TypeError(f"{what}: unknown fields {sorted(kw)}")
    return d


def skinny_down(**kw):
    L.launch.gvk_skinny_down(C.byref(_desc(L.SkinnyDownDesc, "skinny_down", **kw)))


def skinny_up(**kw):
    L.launch.gvk_skinny_up(C.byref(_desc(L.SkinnyUpDesc, "skinny_up", **kw)))


def outer_reduce(**kw):
    L.launch.gvk_outer_reduce(C.byref(_desc(L.OuterDesc, "outer_reduce", **kw)))


OUTER_MAX_ROWS = 10240        # rows one gvk_outer_reduce launch covers (64 slabs x 160 rows), second source included


def outer_scratch_elems(Lat, C_):
    return 128 * (Lat + 1) * C_


def _reduce_jobs(jobs, what):
    arr = (L.ReduceJob * max(1, len(jobs)))()
    for k, job in enumerate(jobs):
        a, b, out, acc = job[:4]
        a2 = job[4] if len(job) > 4 else None
        for t, n in ((a, "a"), (b, "b"), (out, "out"), (a2, "a2")):
            _chk(t, torch.float32, f"{what} {n}")
        M, J = a.shape[0], a.numel() // a.shape[0]
        Lb = 0 if b is None else b.numel() // b.shape[0]
        if b is not None and b.shape[0] != M:
            raise L.GavikoHipError(f"{what}: a and b must have the same number of rows")
        if out.numel() < (J * Lb if b is not None else J):
            raise L.GavikoHipError(f"{what}: out too small")
        if a2 is not None and (b is not None or a2.numel() // a2.shape[0] != J):
            raise L.GavikoHipError(f"{what}: a2 goes with column sums of the same width only")
        arr[k] = L.ReduceJob(L.ptr(a), L.ptr(b), L.ptr(out), L.ptr(a2), M, J, Lb, int(bool(acc)), 0 if a2 is None else a2.shape[0])
    return arr


def param_grads_supported(Lat, C_):
    return C_ % 4 == 0 and 0 < Lat <= 28 and Lat % 4 == 0


PGRAD_TICKETS = 256           # ticket words one gvk_param_grads call may need: column tiles of the outer jobs + 64-output chunks of the small jobs (56 for the GPA gates)


def param_grads(outer, small, scratch, tickets, C_, Lat, seed_ptr=None):
    """One launch for every parameter gradient of a rank-L side-path module of one layer (gaviko_hip.h: gvk_param_grads).
    outer: list of dicts with the gvk_pgrad_outer fields (tensors or None); small: list of (a, b or None, out, accumulate[, a2])."""
    arr = (L.PgradOuter * max(1, len(outer)))()
    fields = [f for f, _ in L.PgradOuter._fields_]
    for k, o in enumerate(outer):
        bad = set(o) - set(fields)
        if bad:
            raise L.GavikoHipError(f"param_grads: unknown field(s) {sorted(bad)}")
        vals = {}
        for f, ct in L.PgradOuter._fields_:
            v = o.get(f)
            if ct is C.c_void_p:
                _chk(v, torch.float32, f"param_grads outer[{k}].{f}")
                vals[f] = L.ptr(v)
            elif ct is C.c_float:
                vals[f] = float(v or 0.0)
            else:
                vals[f] = int(v or 0)
        M, M2, Cj = vals["M"], vals["M2"], vals["C"] or C_
        for f, n in (("narrow", M * Lat), ("wide", M * Cj), ("narrow2", M2 * Lat), ("wide2", M2 * Cj), ("mean", M), ("rstd", M), ("colsum", Cj),
                     ("out", Lat * Cj), ("aff_w", Lat * Cj), ("aff_gamma", Cj), ("aff_beta", Cj), ("aff_dgamma", Cj), ("aff_dbeta", Cj), ("aff_dbias", Lat)):
            if o.get(f) is not None and o[f].numel() < n:
                raise L.GavikoHipError(f"param_grads outer[{k}].{f}: needs >= {n} elements, has {o[f].numel()}")
        arr[k] = L.PgradOuter(**vals)
    jobs = _reduce_jobs(small, "param_grads small")
    _chk(scratch, torch.float32, "param_grads scratch")
    if tickets is None or tickets.dtype != torch.int32 or not tickets.is_cuda:
        raise L.GavikoHipError("param_grads: tickets must be an int32 tensor on the HIP device (zero at allocation)")
    L.launch.gvk_param_grads(arr, len(outer), jobs, len(small), scratch, scratch.numel(), tickets, tickets.numel(), seed_ptr, C_, Lat)


def param_grads_scratch_elems(Lat, col_tiles, small_outputs):
    """Upper bound of the scratch floats of one gvk_param_grads call: col_tiles = 64-column tiles of each outer job (the kernel deals the
    jobs' rows to ~240 workgroups, at most 64 row ranges per column tile), small_outputs = outputs of each small job."""
    slabs = min(240 + sum(col_tiles), 64 * sum(col_tiles))
    return slabs * (Lat + 2) * 64 + sum(((o + 63) // 64) * 32 * 64 for o in small_outputs)


def small_wgrad(a, b, out, scratch, M, J, Lb, accumulate=False):
    for t, n in ((a, "a"), (b, "b"), (out, "out"), (scratch, "scratch")):
        _chk(t, torch.float32, "small_wgrad " + n)
    if scratch.numel() < 64 * J * Lb or a.numel() < M * J or b.numel() < M * Lb or out.numel() < J * Lb:
        raise L.GavikoHipError("small_wgrad: buffer too small")
    L.launch.gvk_small_wgrad(a, b, out, scratch, M, J, Lb, int(accumulate))


def colsum(x, out, scratch, M, C_, accumulate=False):
    for t, n in ((x, "x"), (out, "out"), (scratch, "scratch")):
        _chk(t, torch.float32, "colsum " + n)
    if scratch.numel() < 64 * C_ or x.numel() < M * C_ or out.numel() < C_:
        raise L.GavikoHipError("colsum: buffer too small")
    L.launch.gvk_colsum(x, out, scratch, M, C_, int(accumulate))


def window_attn_fwd(**kw):
    L.launch.gvk_window_attn_fwd(C.byref(_desc(L.WindowAttnDesc, "window_attn", **kw)))


def window_attn_bwd(**kw):
    L.launch.gvk_window_attn_bwd(C.byref(_desc(L.WindowAttnDesc, "window_attn", **kw)))


def gpa_fwd(**kw):
    L.launch.gvk_gpa_fwd(C.byref(_desc(L.GpaDesc, "gpa", **kw)))


def gpa_bwd(**kw):
    L.launch.gvk_gpa_bwd(C.byref(_desc(L.GpaDesc, "gpa", **kw)))


_MAP_WIDTHS = (4, 8, 16, 20, 32)


def window_attn_colsum(qkv, lse, w, out, B, D, H, W, kd, kh, kw, L_, scale):
    """out f32 [B, N] = sum_i w[b, i] * P[b, i, :] -- the weighted rows of the MWSA probabilities (N = D*H*W), recomputed from
    window_attn_fwd's operands: qkv f32 [B*N, 3L], lse f32 [B*N], the grid (D, H, W), the window (kd, kh, kw), scale.  w f32 [B, N]."""
    dims = (B, D, H, W, kd, kh, kw)
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in dims):
        raise L.GavikoHipError(f"window_attn_colsum: B, grid and window must be positive ints, got {dims}")
    if L_ not in _MAP_WIDTHS:
        raise L.GavikoHipError(f"window_attn_colsum: L={L_} unsupported {_MAP_WIDTHS}")
    N = D * H * W
    _chk(qkv, torch.float32, "window_attn_colsum qkv", B * N * 3 * L_)
    _chk(lse, torch.float32, "window_attn_colsum lse", B * N)
    _chk(w, torch.float32, "window_attn_colsum w", B * N)
    _chk(out, torch.float32, "window_attn_colsum out", B * N)
    if any(t is None for t in (qkv, lse, w, out)):
        raise L.GavikoHipError("window_attn_colsum: qkv, lse, w and out are all required")
    d = _desc(L.WindowColsumDesc, "window_attn_colsum", qkv=qkv, lse=lse, w=w, out=out, B=B, D=D, H=H, W=W, kd=kd, kh=kh, kw=kw, L=L_,
              scale=float(scale))
    L.launch.gvk_window_attn_colsum(C.byref(d))


def gpa_attn_maps(xl, ll, qg, ql, lse_g, lse_l, imp, gw, B, T, N, P, L_, *, global_=None, local=None, fused=None):
    """The cross-attention probabilities of one GPA layer from gpa_fwd's saved buffers (xl f32 [B*T, L], ll [B*N, L], qg / ql [B, P, L]
    pre-scaled, lse_g / lse_l / imp [B, P], gw [B]) -> global_, local, fused f32 [B, P, N], each optional (at least one):
    fused = imp * (gw * global_ + (1 - gw) * local).  global_ is 0 at the first P + 1 patch positions (the reference's double slice)."""
    dims = (B, T, N, P)
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in dims):
        raise L.GavikoHipError(f"gpa_attn_maps: B, T, N, P must be positive ints, got {dims}")
    if L_ not in _MAP_WIDTHS:
        raise L.GavikoHipError(f"gpa_attn_maps: L={L_} unsupported {_MAP_WIDTHS}")
    if P > 64 or T != P + 1 + N or N <= P + 1:
        raise L.GavikoHipError(f"gpa_attn_maps: need P <= 64, T = P + 1 + N and N > P + 1 (global image tokens left after the double "
                               f"slice), got T={T} N={N} P={P}")
    ins = dict(xl=(xl, B * T * L_), ll=(ll, B * N * L_), qg=(qg, B * P * L_), ql=(ql, B * P * L_), lse_g=(lse_g, B * P), lse_l=(lse_l, B * P),
               imp=(imp, B * P), gw=(gw, B))
    for name, (t, n) in ins.items():
        if t is None:
            raise L.GavikoHipError(f"gpa_attn_maps: {name} is required")
        _chk(t, torch.float32, "gpa_attn_maps " + name, n)
    if global_ is None and local is None and fused is None:
        raise L.GavikoHipError("gpa_attn_maps: no output requested")
    for name, t in (("global_", global_), ("local", local), ("fused", fused)):
        _chk(t, torch.float32, "gpa_attn_maps " + name, B * P * N)
    d = _desc(L.GpaMapsDesc, "gpa_attn_maps", xl=xl, ll=ll, qg=qg, ql=ql, lse_g=lse_g, lse_l=lse_l, imp=imp, gw=gw, pg=global_, pl=local,
              fused=fused, B=B, T=T, N=N, P=P, L=L_)
    L.launch.gvk_gpa_attn_maps(C.byref(d))


def gpa_gate_param_count(Lat, P):
    return L.load().gvk_gpa_gate_param_count(Lat, P)


def rows_broadcast(out, src, add, B, T, row_off, R, C_):
    _chk(out, torch.float32, "rows_broadcast out", B * T * C_)
    _chk(src, torch.float32, "rows_broadcast src", R * C_)
    _chk(add, torch.float32, "rows_broadcast add", R * C_)
    L.launch.gvk_rows_broadcast(out, src, add, B, T, row_off, R, C_)


def rows_batch_sum(dg, out, out2, B, T, row_off, R, C_, accumulate=False):
    _chk(dg, torch.float32, "rows_batch_sum dg", B * T * C_)
    _chk(out, torch.float32, "rows_batch_sum out", R * C_)
    _chk(out2, torch.float32, "rows_batch_sum out2", R * C_)
    L.launch.gvk_rows_batch_sum(dg, out, out2, B, T, row_off, R, C_, int(accumulate))


def head_fwd(**kw):
    L.launch.gvk_head_fwd(C.byref(_desc(L.HeadDesc, "head", **kw)))


def head_bwd(**kw):
    L.launch.gvk_head_bwd(C.byref(_desc(L.HeadDesc, "head", **kw)))


def attention_bwd_workspace(B, T, H, device):
    """Zeroed workspace of the one-pass bf16 backward (gvk_attention_desc.ws): progress words + the running dQ sums of the
    ordered hand-off.  One per stream that issues the call (launches sharing it must be ordered)."""
    n = int(L.load().gvk_attention_bwd_ws_bytes(B, T, H))
    return torch.zeros((n + 3) // 4, dtype=torch.int32, device=device)


def attention_bwd_timeouts(ws) -> int:
    """Hand-off waits of the one-pass backward that ran into their bound since the workspace was made (0 unless a launch was broken)."""
    return int(ws[int(L.load().gvk_attention_bwd_status_offset(ws.numel() * 4)) // 4].item())


def attention_bwd(qkv, out, dout, lse, delta, dqkv, B, T, H, scale, drop_p=0.0, seed=0, seed_ptr=None, q_prescaled=False, ws=None, need_rows=None):
    """Gradients [dq | dk | dv] of the unscaled q, k, v into dqkv; delta is scratch.  One form runs per call, by this precedence:
      fp32 operands:          the plain two-pass kernels -- need_rows and ws are ignored;
      drop_p > 0:             the two-pass dropout kernels -- need_rows and ws are ignored;
      need_rows (not None):   the two-pass kernels on the first need_rows tokens of every sample only -- ws is ignored;
      ws (attention_bwd_workspace): the one-pass kernel (five products, ordered dQ hand-off);
      otherwise:              the two-pass kernels.
    The library refuses a descriptor that asks for two of these at once; the engine passes drop_p and need_rows together
    (_attn_block_bwd), so the choice is made here, once, before the descriptor is filled."""
    inner, f32, drop = H * 64, qkv.dtype == torch.float32, drop_p > 0
    need_rows = 0 if f32 or drop or need_rows is None else int(need_rows)
    if f32 or drop or need_rows:
        ws = None
    dt, rows = (torch.float32, B * T) if f32 else (torch.bfloat16, pad_rows(B * T))
    for t, n, dtype, elems in ((qkv, "qkv", dt, rows * 3 * inner), (out, "out", dt, rows * inner), (dout, "dout", dt, rows * inner),
                               (dqkv, "dqkv", dt, B * T * 3 * inner), (lse, "lse", torch.float32, B * H * T),
                               (delta, "delta", torch.float32, B * H * T)):
        _chk(t, dtype, "attn_bwd " + n, elems)
    if ws is not None:
        _chk(ws, torch.int32, "attn_bwd ws", (int(L.load().gvk_attention_bwd_ws_bytes(B, T, H)) + 3) // 4)
    if not f32 and not q_prescaled:                          # see attention_fwd
        qkv = _prescaled_copy(qkv, B * T, H, scale)
    d = L.AttentionDesc(qkv=L.ptr(qkv), out=L.ptr(out), lse=L.ptr(lse), dout=L.ptr(dout), delta=L.ptr(delta), dqkv=L.ptr(dqkv),
                        seed_ptr=L.ptr(seed_ptr) if drop else None, ws=L.ptr(ws), B=B, T=T, H=H, ld_qkv=3 * inner, ld_out=inner, f32=int(f32),
                        need_rows=need_rows, scale=scale, drop_p=float(drop_p), seed=int(seed) if drop else 0,
                        ws_bytes=ws.numel() * 4 if ws is not None else 0)
    L.launch.gvk_attention_bwd(C.byref(d))


def small_linear_fwd(x, w, b, out, R, K, C_):
    for t, n in ((x, "x"), (w, "w"), (b, "b"), (out, "out")):
        _chk(t, torch.float32, "small_linear " + n)
    if x.numel() < R * K or w.numel() < C_ * K or out.numel() < R * C_:
        raise L.GavikoHipError("small_linear_fwd: buffer too small")
    L.launch.gvk_small_linear_fwd(x, w, b, out, R, K, C_)


def small_linear_bwd(x, w, dout, dw, db, dx, R, K, C_, accumulate=False):
    for t, n in ((x, "x"), (w, "w"), (dout, "dout"), (dw, "dw"), (db, "db"), (dx, "dx")):
        _chk(t, torch.float32, "small_linear_bwd " + n)
    L.launch.gvk_small_linear_bwd(x, w, dout, dw, db, dx, R, K, C_, int(accumulate))


def vpt_repack_fwd(inp, prompt, out, B, Tin, Tout, P, skip, C_):
    _chk(inp, torch.float32, "vpt_repack in", B * Tin * C_)
    _chk(prompt, torch.float32, "vpt_repack prompt", P * C_)
    _chk(out, torch.float32, "vpt_repack out", B * Tout * C_)
    L.launch.gvk_vpt_repack_fwd(inp, prompt, out, B, Tin, Tout, P, skip, C_)


def vpt_repack_bwd(dout, din, B, Tin, Tout, P, skip, C_):
    _chk(dout, torch.float32, "vpt_repack_bwd dout", B * Tout * C_)
    _chk(din, torch.float32, "vpt_repack_bwd din", B * Tin * C_)
    L.launch.gvk_vpt_repack_bwd(dout, din, B, Tin, Tout, P, skip, C_)


def cast_bf16_f32_strided(inp, out, M, C_, ld_in, col0=0):
    """f32 out[M][C] = inp[M][ld_in] columns col0 .. col0+C (inp bf16, or fp32 on the fp32 compute path)."""
    if inp.dtype == torch.float32:
        _chk(inp, torch.float32, "copy_strided in", M * ld_in)
        _chk(out, torch.float32, "copy_strided out", M * C_)
        L.launch.gvk_copy_f32_strided(inp.data_ptr() + 4 * col0, out, M, C_, ld_in)
        return
    _chk(inp, torch.bfloat16, "cast_bf16_f32 in", M * ld_in)
    _chk(out, torch.float32, "cast_bf16_f32 out", M * C_)
    L.launch.gvk_cast_bf16_f32_strided(inp.data_ptr() + 2 * col0, out, M, C_, ld_in)


def lora_merge(w, a_q, b_q, a_v, b_v, out, C_, r, s):
    for t, n in ((w, "w"), (a_q, "a_q"), (b_q, "b_q"), (a_v, "a_v"), (b_v, "b_v"), (out, "out")):
        _chk(t, torch.float32, "lora_merge " + n)
    if w.numel() != 3 * C_ * C_ or out.numel() < 3 * C_ * C_ or a_q.numel() != r * C_ or b_q.numel() != C_ * r:
        raise L.GavikoHipError("lora_merge: shape mismatch")
    L.launch.gvk_lora_merge_f32(w, a_q, b_q, a_v, b_v, out, C_, r, float(s))


def reduce_batch(jobs, scratch):
    """jobs: list of (a [M,J], b [M,L] or None, out, accumulate[, a2 [M2,J]]).  One launch pair for up to 8 small column-sum / J x L
    wgrad reductions; a2 (column sums only) appends more rows to the same sum.  scratch f32 >= 32 * total outputs."""
    arr = (L.ReduceJob * len(jobs))()
    total = 0
    for k, job in enumerate(jobs):
        a, b, out, acc = job[:4]
        a2 = job[4] if len(job) > 4 else None
        _chk(a2, torch.float32, "reduce_batch a2")
        _chk(a, torch.float32, "reduce_batch a")
        _chk(b, torch.float32, "reduce_batch b")
        _chk(out, torch.float32, "reduce_batch out")
        M, J = a.shape[0], a.numel() // a.shape[0]
        Lb = 0 if b is None else b.numel() // b.shape[0]
        if b is not None and b.shape[0] != M:
            raise L.GavikoHipError("reduce_batch: a and b must have the same number of rows")
        if out.numel() < (J * Lb if b is not None else J):
            raise L.GavikoHipError("reduce_batch: out too small")
        total += J * Lb if b is not None else J
        if a2 is not None and (b is not None or a2.numel() // a2.shape[0] != J):
            raise L.GavikoHipError("reduce_batch: a2 goes with column sums of the same width only")
        arr[k] = L.ReduceJob(L.ptr(a), L.ptr(b), L.ptr(out), L.ptr(a2), M, J, Lb, int(bool(acc)), 0 if a2 is None else a2.shape[0])
    _chk(scratch, torch.float32, "reduce_batch scratch", 32 * total)
    L.launch.gvk_reduce_batch(arr, len(jobs), scratch)


def ln_lowrank_affine(Q, S, W, gamma, beta, dW, dgamma, dbeta, dbias, Lat, C_, accumulate=False):
    for t, n in ((Q, "Q"), (S, "S"), (W, "W"), (gamma, "gamma"), (beta, "beta"), (dW, "dW"), (dgamma, "dgamma"), (dbeta, "dbeta"), (dbias, "dbias")):
        _chk(t, torch.float32, "ln_lowrank_affine " + n)
    if Q.numel() < Lat * C_ or W.numel() < Lat * C_ or dW.numel() < Lat * C_ or S.numel() < Lat:
        raise L.GavikoHipError("ln_lowrank_affine: buffer too small")
    L.launch.gvk_ln_lowrank_affine(Q, S, W, gamma, beta, dW, dgamma, dbeta, dbias, Lat, C_, int(bool(accumulate)))


# ---- SSF (model/ssf.py): effective parameters and scale/shift gradients ---------------------------------------------------
def ssf_fold_weight(w, s, out, out_t=None):
    """out[n][k] = w[n][k] * s[n] in out's dtype (bf16 / fp32); out_t [K][N] = the transpose (optional)."""
    _chk(w, torch.float32, "ssf_fold_weight w")
    N = w.shape[0]
    K = w.numel() // N
    _chk(s, torch.float32, "ssf_fold_weight s", N)
    if out.dtype not in (torch.bfloat16, torch.float32) or (out_t is not None and out_t.dtype != out.dtype):
        raise L.GavikoHipError("ssf_fold_weight: outputs must be bf16 or fp32 (both the same)")
    _chk(out, out.dtype, "ssf_fold_weight out", N * K)
    _chk(out_t, out.dtype, "ssf_fold_weight out_t", N * K)
    L.launch.gvk_ssf_fold_weight(w, s, out, out_t, N, K, int(out.dtype == torch.float32))


def ssf_fold_vec(a, s, t, out):
    n = s.numel()
    for x, nm in ((a, "a"), (s, "s"), (t, "t"), (out, "out")):
        _chk(x, torch.float32, "ssf_fold_vec " + nm, n)
    L.launch.gvk_ssf_fold_vec(a, s, t, out, n)


def ssf_colgrad(dy, y0, s, t, ds, dt, scratch, M, N, *, y1=None, pos=None, ld_dy=None, ld_y=None, rows_in=0, rows_out=0, row_off=0,
                y0_cols=0, y0_mul=1.0, y_mul=1.0):
    for x, nm in ((s, "s"), (t, "t"), (ds, "ds"), (dt, "dt")):
        _chk(x, torch.float32, "ssf_colgrad " + nm, N)
    _chk(scratch, torch.float32, "ssf_colgrad scratch", 64 * 2 * N)
    _chk(y1, torch.float32, "ssf_colgrad y1")
    _chk(pos, torch.float32, "ssf_colgrad pos")
    for x, nm in ((dy, "dy"), (y0, "y0")):
        if x.dtype not in (torch.bfloat16, torch.float32) or not x.is_cuda or not x.is_contiguous():
            raise L.GavikoHipError(f"ssf_colgrad {nm}: expected a contiguous bf16 / fp32 device tensor")
    d = L.SsfColgradDesc(dy=L.ptr(dy), y0=L.ptr(y0), y1=L.ptr(y1), pos=L.ptr(pos), s=L.ptr(s), t=L.ptr(t), ds=L.ptr(ds), dt=L.ptr(dt),
                         scratch=L.ptr(scratch), M=M, N=N, ld_dy=N if ld_dy is None else ld_dy, ld_y=N if ld_y is None else ld_y,
                         dy_f32=int(dy.dtype == torch.float32), y0_f32=int(y0.dtype == torch.float32), rows_in=rows_in, rows_out=rows_out,
                         row_off=row_off, y0_cols=int(y0_cols), y0_mul=float(y0_mul), y_mul=float(y_mul))
    L.launch.gvk_ssf_colgrad(C.byref(d))


def ssf_ln_grad(dgamma_eff, dbeta_eff, gamma, beta, ds, dt):
    n = gamma.numel()
    for x, nm in ((dgamma_eff, "dgamma'"), (dbeta_eff, "dbeta'"), (gamma, "gamma"), (beta, "beta"), (ds, "ds"), (dt, "dt")):
        _chk(x, torch.float32, "ssf_ln_grad " + nm, n)
    L.launch.gvk_ssf_ln_grad(dgamma_eff, dbeta_eff, gamma, beta, ds, dt, n)


def ssf_head_grad(g, mean, rstd, wh, dlogits, gamma, beta, ds, dt, B, T, C_, K, r0, R):
    for x, nm in ((g, "g"), (mean, "mean"), (rstd, "rstd"), (wh, "wh"), (dlogits, "dlogits"), (gamma, "gamma"), (beta, "beta"), (ds, "ds"), (dt, "dt")):
        _chk(x, torch.float32, "ssf_head_grad " + nm)
    L.launch.gvk_ssf_head_grad(g, mean, rstd, wh, dlogits, gamma, beta, ds, dt, B, T, C_, K, r0, R)


# ---- DVPT (model/dvpt.py) ------------------------------------------------------------------------------------------------
def dvpt_fwd(**kw):
    L.launch.gvk_dvpt_fwd(C.byref(_desc(L.DvptDesc, "dvpt_fwd", **kw)))


def dvpt_bwd(**kw):
    L.launch.gvk_dvpt_bwd(C.byref(_desc(L.DvptDesc, "dvpt_bwd", **kw)))


def scale_dev_(t: torch.Tensor, alpha: torch.Tensor) -> None:
    """t *= alpha[0] with alpha a device scalar (no host read)."""
    _chk(t, torch.float32, "scale_dev_ x")
    _chk(alpha, torch.float32, "scale_dev_ alpha", 1)
    L.launch.gvk_scale_dev(t, alpha, t.numel())


# ---- EVP (model/evp.py) --------------------------------------------------------------------------------------------------
def evp_highpass(img, hp, depth_mask, out):
    _chk(img, torch.float32, "evp_highpass img")
    B, ch, D, H, W = img.shape
    _chk(hp, torch.float32, "evp_highpass hp", H * H)
    _chk(depth_mask, torch.int32, "evp_highpass depth_mask", D)
    _chk(out, torch.float32, "evp_highpass out", img.numel())
    L.launch.gvk_evp_highpass(img, hp, depth_mask, out, B * ch, D, H, W)


def evp_highpass_sign(img, hp, depth_mask, dout, out):
    """out = dout o sign(hp . img) on the filtered slices, dout o sign(img) on the others: the modulus step of evp_highpass's backward."""
    _chk(img, torch.float32, "evp_highpass_sign img")
    B, ch, D, H, W = img.shape
    _chk(hp, torch.float32, "evp_highpass_sign hp", H * H)
    _chk(depth_mask, torch.int32, "evp_highpass_sign depth_mask", D)
    _chk(dout, torch.float32, "evp_highpass_sign dout", img.numel())
    _chk(out, torch.float32, "evp_highpass_sign out", img.numel())
    L.launch.gvk_evp_highpass_sign(img, hp, depth_mask, dout, out, B * ch, D, H, W)


def evp_highpass_linear(x, op, depth_mask, out, accumulate=False):
    """out (+)= op . x on the filtered slices, x on the others (op = hp^T: the adjoint of the high-pass's linear part)."""
    _chk(x, torch.float32, "evp_highpass_linear x")
    B, ch, D, H, W = x.shape
    _chk(op, torch.float32, "evp_highpass_linear op", H * H)
    _chk(depth_mask, torch.int32, "evp_highpass_linear depth_mask", D)
    _chk(out, torch.float32, "evp_highpass_linear out", x.numel())
    if out.data_ptr() == x.data_ptr():
        raise L.GavikoHipError("evp_highpass_linear: out must not alias x")
    L.launch.gvk_evp_highpass_linear(x, op, depth_mask, out, int(bool(accumulate)), B * ch, D, H, W)


def pad2d(src, rows, cols, dst, drows, dcols, *, ld_src=None, ld_dst=None, transpose=False):
    """dst[drows x dcols] = src[rows x cols] (optionally transposed) zero-padded."""
    _chk(src, torch.float32, "pad2d src")
    _chk(dst, torch.float32, "pad2d dst")
    L.launch.gvk_pad2d_f32(src, cols if ld_src is None else ld_src, rows, cols, int(transpose), dst, dcols if ld_dst is None else ld_dst, drows, dcols)


def add2d(a, lda, b, ldb, out, ldo, rows, cols):
    for t, n in ((a, "a"), (b, "b"), (out, "out")):
        _chk(t, torch.float32, "add2d " + n)
    L.launch.gvk_add2d_f32(a, lda, b, ldb, out, ldo, rows, cols)


def gelu_fwd(x, y):
    _chk(x, torch.float32, "gelu_fwd x")
    _chk(y, torch.float32, "gelu_fwd y", x.numel())
    L.launch.gvk_gelu_fwd_f32(x, y, x.numel())


def gelu_bwd(dy, x, dx):
    for t, n in ((dy, "dy"), (x, "x"), (dx, "dx")):
        _chk(t, torch.float32, "gelu_bwd " + n, x.numel())
    L.launch.gvk_gelu_bwd_f32(dy, x, dx, x.numel())


def rows_patch(tok, src, pos, B, T, N, C_, row_off, accumulate):
    _chk(tok, torch.float32, "rows_patch tok", B * T * C_)
    _chk(src, torch.float32, "rows_patch src", B * N * C_)
    _chk(pos, torch.float32, "rows_patch pos", N * C_)
    L.launch.gvk_rows_patch(tok, src, pos, B, T, N, C_, row_off, int(accumulate))


def rows_gather(tok, dst, B, T, N, C_, row_off):
    _chk(tok, torch.float32, "rows_gather tok", B * T * C_)
    _chk(dst, torch.float32, "rows_gather dst", B * N * C_)
    L.launch.gvk_rows_gather(tok, dst, B, T, N, C_, row_off)


# ---- loss seed (train.py:176-179, 283/306, 327-328) -------------------------------------------------------------------------
LOSS_CE, LOSS_FOCAL = 0, 1


def loss_fwd_bwd(logits, target, loss, dlogits, kind, gamma=0.0, eps=1e-16, ignore_index=-100, weights=None, meter=None, reduction="mean"):
    """loss[0] = criterion(logits, target), dlogits = its gradient, meter += (loss*B, #correct, B): one launch, no host read.
    reduction='none': loss receives the B per-sample values and meter[0] their sum (losses.StepMeter).
    A label that is neither ignore_index nor within [0, K) (compared as the int64 it is: 2^32 + 1 is not class 1) makes its row a bad row.
    The kernel reads nothing at that index; there is no host read, so it cannot raise as torch does ("Target 5 is out of bounds") and
    answers with NaN instead: the row's per-sample loss and its whole dlogits row are NaN, 'mean' and 'sum' return NaN, and the meter's
    correct count gains nothing.  'mean' with a zero denominator (every row ignored, or zero class weights on all the others) returns
    NaN; the cross entropy then leaves the ignored rows' gradient at zero and makes the others NaN, as torch does, and the focal loss
    makes every row NaN, ignored ones too, except at the logits outside its clamp (their gradient stays 0), as its reference does."""
    _chk(logits, torch.float32, "loss logits")
    B, K = logits.shape
    if target.dtype != torch.int64 or not target.is_contiguous() or target.numel() != B:
        raise ValueError("loss target must be a contiguous int64 [B] tensor")
    _chk(loss, torch.float32, "loss out", B if reduction == "none" else 1)
    _chk(dlogits, torch.float32, "loss dlogits", B * K)
    if weights is not None:
        _chk(weights, torch.float32, "loss weights", K)
    if meter is not None:
        _chk(meter, torch.float32, "loss meter", 3)
    d = L.LossDesc(logits=L.ptr(logits), target=L.ptr(target), weights=L.ptr(weights) if weights is not None else None,
                   loss=L.ptr(loss), dlogits=L.ptr(dlogits), meter=L.ptr(meter) if meter is not None else None,
                   B=B, K=K, kind=kind, reduction={"mean": 0, "sum": 1, "none": 2}[reduction], gamma=gamma, eps=eps, ignore_index=ignore_index)
    L.launch.gvk_loss_fwd_bwd(C.byref(d))


def loss_mixed_fwd_bwd(logits, target_a, target_b, lam, loss, dlogits, kind, gamma=0.0, eps=1e-16, smoothing=0.0, ignore_index=-100, weights=None,
                       meter=None, reduction="mean"):
    """The loss seed for mixed targets: row i costs lam[i] * l(x_i, target_a[i]) + (1 - lam[i]) * l(x_i, target_b[i]), l the per-sample loss of
    loss_fwd_bwd (class weight included; cross entropy with label smoothing `smoothing` by torch's rule for class-index targets, focal without).
    target_b and lam (f32 [B]) may both be None: no partner, lam = 1 -- plain label smoothing.  'mean' divides by the sum over the rows that are
    not ignored of lam w_a + (1 - lam) w_b; a row is ignored when either target is ignore_index; meter[1] counts argmax == the dominant label
    (target_a where lam >= 0.5).  With smoothing = 0 and lam = 1 the bits are those of loss_fwd_bwd.  One launch, no host read.
    A row that is not ignored and whose target_a or target_b lies outside [0, K) (as an int64), whatever its lam, is a bad row as in
    loss_fwd_bwd: nothing is read at that index, its loss and dlogits row are NaN, 'mean' and 'sum' return NaN, the meter's correct count
    gains nothing.  'mean' with a zero denominator behaves as there too."""
    _chk(logits, torch.float32, "loss_mixed logits")
    B, K = logits.shape
    for t, what in ((target_a, "target_a"), (target_b, "target_b")):
        if t is not None and (not t.is_cuda or t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != B):
            raise ValueError(f"loss_mixed {what} must be a contiguous int64 [B] tensor on the device")
    if target_a is None or (target_b is None) != (lam is None):
        raise ValueError("loss_mixed: target_a is required; target_b and lam come together (both None: no partner, lam = 1)")
    if lam is not None:
        _chk(lam, torch.float32, "loss_mixed lam", B)
        if lam.numel() != B:
            raise ValueError("loss_mixed lam must be a float32 [B] tensor")
    if not 0.0 <= smoothing <= 1.0:
        raise ValueError(f"loss_mixed: smoothing must be in [0, 1], got {smoothing}")
    if kind != LOSS_CE and smoothing != 0.0:
        raise ValueError("loss_mixed: label smoothing is built for the cross entropy only")
    _chk(loss, torch.float32, "loss_mixed out", B if reduction == "none" else 1)
    _chk(dlogits, torch.float32, "loss_mixed dlogits", B * K)
    if weights is not None:
        _chk(weights, torch.float32, "loss_mixed weights", K)
    if meter is not None:
        _chk(meter, torch.float32, "loss_mixed meter", 3)
    d = L.LossMixedDesc(logits=L.ptr(logits), target_a=L.ptr(target_a), target_b=L.ptr(target_b) if target_b is not None else None,
                        lam=L.ptr(lam) if lam is not None else None, weights=L.ptr(weights) if weights is not None else None,
                        loss=L.ptr(loss), dlogits=L.ptr(dlogits), meter=L.ptr(meter) if meter is not None else None,
                        B=B, K=K, kind=kind, reduction={"mean": 0, "sum": 1, "none": 2}[reduction], gamma=gamma, eps=eps, smoothing=smoothing,
                        ignore_index=ignore_index)
    L.launch.gvk_loss_mixed_fwd_bwd(C.byref(d))


# ---- data side + evaluation metrics (train.py:38-62, eval.py:103-122) --------------------------------------------------------
def minmax_partials(B: int, device) -> torch.Tensor:
    return torch.empty(B * L.load().gvk_minmax_partials(), dtype=torch.float32, device=device)


def volume_minmax(x: torch.Tensor, partials: torch.Tensor) -> None:
    _chk(x, torch.float32, "volume_minmax x")
    B = x.shape[0]
    _chk(partials, torch.float32, "volume_minmax partials", B * L.load().gvk_minmax_partials())
    L.launch.gvk_volume_minmax(x, partials, B, x.numel() // B)


def rescale_intensity(x, partials, y, out_min=0.0, out_max=1.0, minmax=None) -> None:
    _chk(x, torch.float32, "rescale_intensity x")
    _chk(y, torch.float32, "rescale_intensity y", x.numel())
    B = x.shape[0]
    if minmax is not None:
        _chk(minmax, torch.float32, "rescale_intensity minmax", 2 * B)
    L.launch.gvk_rescale_intensity(x, partials, y, minmax, B, x.numel() // B, out_min, out_max)


def spatial_transform(x, out, mats, flags, partials) -> None:
    _chk(x, torch.float32, "spatial_transform in")
    _chk(out, torch.float32, "spatial_transform out", x.numel())
    B, D, H, W = x.shape[0], x.shape[-3], x.shape[-2], x.shape[-1]
    _chk(mats, torch.float32, "spatial_transform mats", 12 * B)
    _chk(flags, torch.int32, "spatial_transform flags", B)
    L.launch.gvk_spatial_transform(x, out, mats, flags, partials, B, D, H, W)


BLUR_MAX_RADIUS, BLUR_TAPS, BIAS_COEFFS = 16, 33, 20                     # GVK_BLUR_MAX_RADIUS, its table row length, GVK_BIAS_COEFFS
INTENSITY_COPY, INTENSITY_NOISE, INTENSITY_BIAS = 0, 1, 2                # kind[b] of intensity_pointwise


def _one_channel(x, out, what):
    """The x / out checks every one-channel volume pass shares; returns (B, D, H, W)."""
    _chk(x, torch.float32, f"{what} in")
    _chk(out, torch.float32, f"{what} out", x.numel())
    if x.dim() < 4 or x.numel() != x.shape[0] * x.shape[-3] * x.shape[-2] * x.shape[-1]:
        raise L.GavikoHipError(f"{what} in: one channel, [B, D, H, W] or [B, 1, D, H, W]")
    return x.shape[0], x.shape[-3], x.shape[-2], x.shape[-1]


def gaussian_blur3d(x, out, scratch, weights, radius, max_radius) -> None:
    """out = scipy.ndimage.gaussian_filter(x[b], sigma_b) per sample (mode='reflect', truncate=4): weights f32 [B][3][33] and radius i32
    [B][3] are device tables built on the host (data.blur_tables), max_radius their largest radius; scratch is a third buffer of x's size."""
    B, D, H, W = _one_channel(x, out, "gaussian_blur3d")
    _chk(scratch, torch.float32, "gaussian_blur3d scratch", x.numel())
    _chk(weights, torch.float32, "gaussian_blur3d weights", 3 * BLUR_TAPS * B)
    _chk(radius, torch.int32, "gaussian_blur3d radius", 3 * B)
    L.launch.gvk_gaussian_blur3d(x, out, scratch, weights, radius, int(max_radius), B, D, H, W)


def intensity_pointwise(x, y, kind, noise, seeds, coeff, order=3) -> None:
    """y[b] = x[b] (kind 0), x[b] + (std z + mean) (kind 1: noise f32 [B][2] = (std, mean), seeds i64 [B] holding the uint64 bit patterns) or
    x[b] exp(P) (kind 2: coeff f32 [B][20], polynomial order <= 3 for the launch); kind i32 [B].  y may be x."""
    B, D, H, W = _one_channel(x, y, "intensity_pointwise")
    _chk(kind, torch.int32, "intensity_pointwise kind", B)
    _chk(noise, torch.float32, "intensity_pointwise noise", 2 * B)
    _chk(seeds, torch.int64, "intensity_pointwise seeds", B)
    _chk(coeff, torch.float32, "intensity_pointwise coeff", BIAS_COEFFS * B)
    L.launch.gvk_intensity_pointwise(x, y, kind, noise, seeds, coeff, int(order), B, D, H, W)


MOTION_MAX_TRANSFORMS, MOTION_MAX_W = 4, 256                             # GVK_MOTION_MAX_TRANSFORMS, GVK_MOTION_MAX_W


def motion_artifact(x, out, mats, ctab, live, partials, K) -> None:
    """tio.RandomMotion in one fused pass: out[b] = sum over the K+1 images (x[b] and x[b] resampled through mats f32 [B][K][12], the maps of
    `data.affine_matrix`) of the circular convolution along the last axis with ctab f32 [B][K+1][W] (data.motion_tables).  live i32 [B]: a
    sample with 0 is copied bit for bit; partials = volume_minmax of x (the pad value).  out must not overlap x."""
    B, D, H, W = _one_channel(x, out, "motion_artifact")
    K = int(K)
    _chk(mats, torch.float32, "motion_artifact mats", 12 * max(K, 0) * B)
    _chk(ctab, torch.float32, "motion_artifact ctab", (max(K, 0) + 1) * W * B)
    _chk(live, torch.int32, "motion_artifact live", B)
    _chk(partials, torch.float32, "motion_artifact partials", B * L.load().gvk_minmax_partials())
    L.launch.gvk_motion_artifact(x, out, mats, ctab, live, partials, K, B, D, H, W)


ELASTIC_MAX_CONTROL_POINTS = 16                                           # GVK_ELASTIC_MAX_CONTROL_POINTS


def elastic_deform(x, out, ctrl, live, partials, field=None) -> None:
    """tio.RandomElasticDeformation in one pass: out[b] at voxel q = x[b] read (trilinear, pad = the volume minimum) at q + d(q), d the cubic
    B-spline interpolation of the control-point displacements ctrl f32 [B][n0][n1][n2][3] (voxels, component a along array axis a; 4..16
    points per axis).  live i32 [B]: a sample with 0 is copied bit for bit; partials = volume_minmax of x; field (optional) f32
    [B][3][D][H][W] receives d.  out must not overlap x."""
    B, D, H, W = _one_channel(x, out, "elastic_deform")
    _chk(ctrl, torch.float32, "elastic_deform ctrl")
    if ctrl.dim() != 5 or ctrl.shape[0] != B or ctrl.shape[4] != 3:
        raise L.GavikoHipError(f"elastic_deform ctrl: [B = {B}][n0][n1][n2][3] expected, got {tuple(ctrl.shape)}")
    n0, n1, n2 = ctrl.shape[1:4]
    _chk(live, torch.int32, "elastic_deform live", B)
    _chk(partials, torch.float32, "elastic_deform partials", B * L.load().gvk_minmax_partials())
    if field is not None:
        _chk(field, torch.float32, "elastic_deform field", 3 * x.numel())
    L.launch.gvk_elastic_deform(x, out, field, ctrl, live, partials, B, D, H, W, n0, n1, n2)


NORMALIZE_SLABS, NORMALIZE_STATS, NORMALIZE_MAX_PERCENTILES = 128, 8, 4     # GVK_NORMALIZE_SLABS, _STATS, _MAX_PERCENTILES
NORMALIZE_ORDER_WS_WORDS = 32 + 3 * 8 * 2048                              # GVK_NORMALIZE_ORDER_WS_WORDS
NORMALIZE_RESCALE, NORMALIZE_ZNORM = 1, 2                                 # mode of normalize_intensity
STATS_FIELDS = ("min", "max", "mean_all", "threshold", "n", "mean", "std")    # columns of the stats table


def _volumes(x, what):
    _chk(x, torch.float32, what)
    B = x.shape[0]
    V = x.numel() // B
    if x.dim() < 2 or V < 1 or V >= 2 ** 31:
        raise L.GavikoHipError(f"{what}: [B][...] with 1 <= voxels per sample < 2^31, got {tuple(x.shape)}")
    return B, V


def _mask_rule(mask, what):
    """(mask_mode, threshold) of gvk_volume_stats for a mask rule None, 'mean' or a number."""
    if mask is None:
        return 0, 0.0
    if isinstance(mask, str) and mask == "mean":
        return 1, 0.0
    if isinstance(mask, (int, float)) and not isinstance(mask, bool):
        return 2, float(mask)
    raise L.GavikoHipError(f"{what}: the mask rule is None, 'mean' or a number, not {mask!r}")


def volume_stats(x: torch.Tensor, mask=None, want_std: bool = True, stats: torch.Tensor = None, count: torch.Tensor = None,
                 partials: torch.Tensor = None):
    """Per-sample statistics of float32 volumes x [B][...] (any voxel count below 2^31): (stats, count), stats float64 [B][8] with the columns
    STATS_FIELDS = min, max and mean of ALL voxels, the mask threshold, then n, mean and unbiased std (0 unless want_std) of the masked
    voxels; count int64 [B] = n.  mask: None (every voxel), 'mean' (x > the float32 mean of all voxels) or a number t (x > t).  Float64
    sums in a fixed order: the same bits on every run.  No host read.  stats, count and the scratch `partials` (float64,
    B * NORMALIZE_SLABS * 4) are allocated here unless given."""
    B, V = _volumes(x, "volume_stats x")
    mode, t = _mask_rule(mask, "volume_stats")
    if stats is None:
        stats = torch.empty((B, NORMALIZE_STATS), dtype=torch.float64, device=x.device)
    if count is None:
        count = torch.empty(B, dtype=torch.int64, device=x.device)
    _chk(stats, torch.float64, "volume_stats stats", B * NORMALIZE_STATS)
    _chk(count, torch.int64, "volume_stats count", B)
    if partials is None:
        partials = torch.empty(B * NORMALIZE_SLABS * 4, dtype=torch.float64, device=x.device)
    _chk(partials, torch.float64, "volume_stats partials", B * NORMALIZE_SLABS * 4)
    L.launch.gvk_volume_stats(x, partials, stats, count, mode, t, int(bool(want_std)), B, V)
    return stats, count


def volume_order_stats(x: torch.Tensor, stats: torch.Tensor, percentiles, pairs: torch.Tensor = None, cutoffs: torch.Tensor = None,
                       workspace: torch.Tensor = None):
    """Exact order statistics of the masked voxels of x (threshold and n come from `stats` = volume_stats of the same x) for up to 4
    percentiles in [0, 100]: (pairs float32 [B][Q][2], cutoffs float32 [B][Q]) -- the two neighbouring sorted values of each percentile and
    numpy's 'linear' percentile of the float64 values, rounded to float32.  No sort, no host read.  The outputs and the scratch `workspace`
    (int32, B * NORMALIZE_ORDER_WS_WORDS) are allocated here unless given."""
    B, V = _volumes(x, "volume_order_stats x")
    _chk(stats, torch.float64, "volume_order_stats stats", B * NORMALIZE_STATS)
    q = [float(p) for p in percentiles]
    if not 1 <= len(q) <= NORMALIZE_MAX_PERCENTILES or any(not 0.0 <= p <= 100.0 for p in q):
        raise L.GavikoHipError(f"volume_order_stats: 1..{NORMALIZE_MAX_PERCENTILES} percentiles in [0, 100], got {percentiles!r}")
    qf = [p / 100.0 for p in q] + [0.0] * (NORMALIZE_MAX_PERCENTILES - len(q))
    ws = torch.empty(B * NORMALIZE_ORDER_WS_WORDS, dtype=torch.int32, device=x.device) if workspace is None else workspace
    pairs = torch.empty((B, len(q), 2), dtype=torch.float32, device=x.device) if pairs is None else pairs
    cutoffs = torch.empty((B, len(q)), dtype=torch.float32, device=x.device) if cutoffs is None else cutoffs
    _chk(ws, torch.int32, "volume_order_stats workspace", B * NORMALIZE_ORDER_WS_WORDS)
    _chk(pairs, torch.float32, "volume_order_stats pairs", 2 * B * len(q))
    _chk(cutoffs, torch.float32, "volume_order_stats cutoffs", B * len(q))
    L.launch.gvk_volume_order_stats(x, stats, ws, pairs, cutoffs, len(q), *qf, B, V)
    return pairs, cutoffs


def normalize_intensity(x: torch.Tensor, y: torch.Tensor, stats: torch.Tensor, mode: int, cutoffs: torch.Tensor = None, out_min: float = 0.0,
                        out_max: float = 1.0, status: torch.Tensor = None, params: torch.Tensor = None) -> torch.Tensor:
    """The apply pass.  mode NORMALIZE_RESCALE: torchio's rescale with the volume clipped to cutoffs[b][0:2] (volume_order_stats);
    NORMALIZE_ZNORM: y = float32((x - mean) / std) in float64 with the masked mean and std of `stats`.  Returns status int32 [B] (0 normalised,
    1 empty mask, 2 zero range / zero std / fewer than two voxels: such a sample is copied bit for bit), a device tensor nobody waits on."""
    B, V = _volumes(x, "normalize_intensity x")
    _chk(y, torch.float32, "normalize_intensity y", x.numel())
    _chk(stats, torch.float64, "normalize_intensity stats", B * NORMALIZE_STATS)
    if mode not in (NORMALIZE_RESCALE, NORMALIZE_ZNORM):
        raise L.GavikoHipError("normalize_intensity: mode is NORMALIZE_RESCALE or NORMALIZE_ZNORM")
    Q = 0
    if mode == NORMALIZE_RESCALE:
        if cutoffs is None or cutoffs.dim() != 2 or cutoffs.shape[0] != B or not 2 <= cutoffs.shape[1] <= NORMALIZE_MAX_PERCENTILES:
            raise L.GavikoHipError("normalize_intensity: the rescale needs cutoffs [B][Q >= 2] (low, high first)")
        _chk(cutoffs, torch.float32, "normalize_intensity cutoffs")
        Q = cutoffs.shape[1]
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=x.device)
    if params is None:
        params = torch.empty((B, 8), dtype=torch.float64, device=x.device)
    _chk(status, torch.int32, "normalize_intensity status", B)
    _chk(params, torch.float64, "normalize_intensity params", 8 * B)
    L.launch.gvk_normalize_intensity(x, y, stats, cutoffs if Q else None, Q, params, status, mode, float(out_min), float(out_max), B, V)
    return status


LANDMARKS_MAX, LANDMARKS_WS_WORDS = 16, 128 + 4 * 32 * 256                # GVK_LANDMARKS_MAX, GVK_LANDMARKS_WS_WORDS
HISTSTD_KNOTS, HISTSTD_PARAMS = 11, 32                                    # GVK_HISTSTD_KNOTS, GVK_HISTSTD_PARAMS


def volume_landmarks(x: torch.Tensor, stats: torch.Tensor, percentiles, pairs: torch.Tensor = None, cutoffs: torch.Tensor = None,
                     workspace: torch.Tensor = None):
    """`volume_order_stats` for up to 16 percentiles in one call and a fixed four sweeps over the volume: (pairs float32 [B][Q][2], cutoffs
    float32 [B][Q]), equal to its results bit for bit for the same percentile.  The percentiles go to the kernels by value.  No sort, no host
    read.  The outputs and the scratch `workspace` (int32, B * LANDMARKS_WS_WORDS) are allocated here unless given."""
    B, V = _volumes(x, "volume_landmarks x")
    _chk(stats, torch.float64, "volume_landmarks stats", B * NORMALIZE_STATS)
    q = [float(p) for p in percentiles]
    if not 1 <= len(q) <= LANDMARKS_MAX or any(not 0.0 <= p <= 100.0 for p in q):
        raise L.GavikoHipError(f"volume_landmarks: 1..{LANDMARKS_MAX} percentiles in [0, 100], got {percentiles!r}")
    qf = (C.c_double * len(q))(*[p / 100.0 for p in q])
    ws = torch.empty(B * LANDMARKS_WS_WORDS, dtype=torch.int32, device=x.device) if workspace is None else workspace
    pairs = torch.empty((B, len(q), 2), dtype=torch.float32, device=x.device) if pairs is None else pairs
    cutoffs = torch.empty((B, len(q)), dtype=torch.float32, device=x.device) if cutoffs is None else cutoffs
    _chk(ws, torch.int32, "volume_landmarks workspace", B * LANDMARKS_WS_WORDS)
    _chk(pairs, torch.float32, "volume_landmarks pairs", 2 * B * len(q))
    _chk(cutoffs, torch.float32, "volume_landmarks cutoffs", B * len(q))
    L.launch.gvk_volume_landmarks(x, stats, ws, pairs, cutoffs, len(q), qf, B, V)
    return pairs, cutoffs


def histogram_standardize(x: torch.Tensor, y: torch.Tensor, stats: torch.Tensor, cutoffs: torch.Tensor, targets, epsilon: float = 1e-5,
                          status: torch.Tensor = None, params: torch.Tensor = None) -> torch.Tensor:
    """torchio's HistogramStandardization apply step: the piecewise-linear map that takes each volume's own 11 landmarks, cutoffs float32
    [B][11] (`volume_landmarks`), onto the 11 trained `targets` (host floats), y = float32(slope_j x + icpt_j) in float64 with j the number
    of interior landmarks <= x.  Every voxel is mapped.  Returns status int32 [B] (0 standardised, 1 empty mask: such a sample is copied bit
    for bit), a device tensor nobody waits on."""
    B, V = _volumes(x, "histogram_standardize x")
    _chk(y, torch.float32, "histogram_standardize y", x.numel())
    _chk(stats, torch.float64, "histogram_standardize stats", B * NORMALIZE_STATS)
    if not isinstance(cutoffs, torch.Tensor) or cutoffs.dim() != 2 or tuple(cutoffs.shape) != (B, HISTSTD_KNOTS):
        raise L.GavikoHipError(f"histogram_standardize: cutoffs are [B = {B}][{HISTSTD_KNOTS}] (the volume's landmarks)")
    _chk(cutoffs, torch.float32, "histogram_standardize cutoffs")
    m = [float(t) for t in targets]
    if len(m) != HISTSTD_KNOTS or not all(np.isfinite(m)) or not float(epsilon) >= 0.0:
        raise L.GavikoHipError(f"histogram_standardize: {HISTSTD_KNOTS} finite targets and epsilon >= 0, got {targets!r}, {epsilon!r}")
    if status is None:
        status = torch.empty(B, dtype=torch.int32, device=x.device)
    if params is None:
        params = torch.empty((B, HISTSTD_PARAMS), dtype=torch.float64, device=x.device)
    _chk(status, torch.int32, "histogram_standardize status", B)
    _chk(params, torch.float64, "histogram_standardize params", HISTSTD_PARAMS * B)
    L.launch.gvk_histogram_standardize(x, y, stats, cutoffs, (C.c_double * HISTSTD_KNOTS)(*m), float(epsilon), params, status, B, V)
    return status


AXIS_CONV_MAX_N, SPIKE_MAX = 256, 4                                       # GVK_AXIS_CONV_MAX_N, GVK_SPIKE_MAX
KSPACE_COPY, KSPACE_GAMMA, KSPACE_SPIKE = 0, 1, 2                         # kind[b] of gamma_spike


def axis_circular_conv(x, out, ctab, axis, live) -> None:
    """tio.RandomGhosting's arithmetic: out[b] = the real circular convolution of x[b] along array axis axis[b] (i32 [B]: 0, 1, 2) with the row
    ctab[b] (f32 [B][AXIS_CONV_MAX_N], entries 0..N-1 used; data.ghosting_tables), on the fp32 matrix cores.  live i32 [B]: a sample with 0 is
    copied bit for bit.  The tables stay on the device and are not read here, so all of D, H, W must be in 2..AXIS_CONV_MAX_N.  out must not
    overlap x."""
    B, D, H, W = _one_channel(x, out, "axis_circular_conv")
    _chk(ctab, torch.float32, "axis_circular_conv ctab", AXIS_CONV_MAX_N * B)
    _chk(axis, torch.int32, "axis_circular_conv axis", B)
    _chk(live, torch.int32, "axis_circular_conv live", B)
    L.launch.gvk_axis_circular_conv(x, out, ctab, axis, live, B, D, H, W)


def gamma_spike(x, out, kind, gamma, amp, nspikes, tab, stats) -> None:
    """One streaming pass, kind i32 [B]: KSPACE_COPY; KSPACE_GAMMA, out = sign(x) |x|^gamma[b] (gamma f32 [B]; 1 is exactly the identity);
    KSPACE_SPIKE, out = x + amp[b] |mean(x[b])| sum over nspikes[b] (i32 [B], <= SPIKE_MAX) spikes of the cosine that the per-axis cos / sin
    tables tab f32 [B][SPIKE_MAX][2][D + H + W] (data.spike_tables) stand for; amp f32 [B]; stats = volume_stats(x)[0], whose float64 mean of
    all voxels is read on the device.  Every table must be given whatever the kinds.  out must not overlap x."""
    B, D, H, W = _one_channel(x, out, "gamma_spike")
    _chk(kind, torch.int32, "gamma_spike kind", B)
    _chk(gamma, torch.float32, "gamma_spike gamma", B)
    _chk(amp, torch.float32, "gamma_spike amp", B)
    _chk(nspikes, torch.int32, "gamma_spike nspikes", B)
    _chk(tab, torch.float32, "gamma_spike tab", B * SPIKE_MAX * 2 * (D + H + W))
    _chk(stats, torch.float64, "gamma_spike stats", B * NORMALIZE_STATS)
    L.launch.gvk_gamma_spike(x, out, kind, gamma, amp, nspikes, tab, stats, B, D, H, W)


def axis_gather2(x, out, src, w, axis, live) -> None:
    """tio.RandomAnisotropy's arithmetic: along array axis axis[b] (i32 [B]), out[..i..] = x0 if w[b][i] == 0 else fmaf(w[b][i], x1 - x0, x0) with
    x0, x1 = x[b] at the indices src[b][i][0], src[b][i][1] of that axis; src i32 [B][n_max][2], w f32 [B][n_max], n_max >= max(D, H, W)
    (data.anisotropy_tables).  live i32 [B]: a sample with 0 is copied bit for bit.  out must not overlap x."""
    B, D, H, W = _one_channel(x, out, "axis_gather2")
    _chk(src, torch.int32, "axis_gather2 src")
    _chk(w, torch.float32, "axis_gather2 w")
    if src is None or w is None or src.dim() != 3 or src.shape[0] != B or src.shape[2] != 2 or tuple(w.shape) != tuple(src.shape[:2]):
        raise L.GavikoHipError(f"axis_gather2: src [B = {B}][n_max][2] and w [B][n_max] expected")
    _chk(axis, torch.int32, "axis_gather2 axis", B)
    _chk(live, torch.int32, "axis_gather2 live", B)
    L.launch.gvk_axis_gather2(x, out, src, w, axis, live, int(src.shape[1]), B, D, H, W)


MIX_COPY, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2                                  # mode[b] of batch_mix (GVK_MIX_*)


def batch_mix(x, out, mode, lam, perm, box) -> None:
    """Mixup / CutMix of a batch in one streaming pass (data.BatchMix).  x, out: float32 volumes on the device, out must not overlap x.  The
    tables are HOST arrays (numpy or CPU tensors), checked here and then uploaded: mode [B] (MIX_COPY: out[b] = x[b] bit for bit; MIX_MIXUP:
    out[b] = lam[b] x[b] + (1 - lam[b]) x[perm[b]] in float32, two roundings; MIX_CUTMIX: out[b] = x[perm[b]] inside the half-open
    box[b] = (d0, d1, h0, h1, w0, w1) and x[b] outside, bit for bit), lam [B] in [0, 1], perm [B] in [0, B), box [B][6] inside the volume."""
    B, D, H, W = _one_channel(x, out, "batch_mix")
    mode, perm = np.ascontiguousarray(mode, dtype=np.int32).reshape(-1), np.ascontiguousarray(perm, dtype=np.int32).reshape(-1)
    lam, box = np.ascontiguousarray(lam, dtype=np.float32).reshape(-1), np.ascontiguousarray(box, dtype=np.int32).reshape(-1, 6)
    if not (len(mode) == len(perm) == len(lam) == len(box) == B):
        raise L.GavikoHipError(f"batch_mix: mode, lam, perm [B] and box [B][6] with B = {B} expected")
    if ((mode < MIX_COPY) | (mode > MIX_CUTMIX)).any():
        raise L.GavikoHipError("batch_mix: mode is MIX_COPY, MIX_MIXUP or MIX_CUTMIX")
    if ((perm < 0) | (perm >= B)).any():
        raise L.GavikoHipError(f"batch_mix: perm must lie in [0, {B})")
    if not ((lam >= 0) & (lam <= 1)).all():
        raise L.GavikoHipError("batch_mix: lam must lie in [0, 1]")
    lo, hi = box[:, 0::2], box[:, 1::2]
    if ((lo < 0) | (hi < lo) | (hi > np.array([D, H, W]))).any():
        raise L.GavikoHipError(f"batch_mix: boxes (d0, d1, h0, h1, w0, w1) must be half-open ranges inside the volume {(D, H, W)}")
    tabs = [torch.from_numpy(t).to(x.device) for t in (mode, lam, perm, box)]
    L.launch.gvk_batch_mix(x, out, *tabs, B, D, H, W)


CONFORM_MAX_TAPS, CONFORM_META = 16, 16                                    # GVK_CONFORM_MAX_TAPS, GVK_CONFORM_META
CONFORM_KEEP, CONFORM_GATHER, CONFORM_CONTRACT, CONFORM_DONE = 0, 1, 2, 3  # axis modes of a conform pass (include/gaviko_hip.h)


def _ragged(data, offsets, shapes, what):
    """The checks every ragged launch shares: data float32 [total] on the device, offsets [B] or [B + 1] and shapes [B][3] HOST arrays with
    every sample inside the buffer.  Returns (offsets int64 [B], shapes int64 [B][3], counts int64 [B])."""
    _chk(data, torch.float32, f"{what} data")
    shapes = np.ascontiguousarray(shapes, dtype=np.int64).reshape(-1, 3)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    B = len(shapes)
    if B < 1 or len(offsets) not in (B, B + 1):
        raise L.GavikoHipError(f"{what}: shapes [B][3] and offsets [B] or [B + 1] expected (host arrays)")
    offsets = offsets[:B]
    if (shapes < 1).any():
        raise L.GavikoHipError(f"{what}: every axis of every sample has at least one voxel")
    counts = shapes.prod(axis=1)
    if (offsets < 0).any() or (offsets + counts > data.numel()).any():
        raise L.GavikoHipError(f"{what}: a sample lies outside the packed buffer of {data.numel()} elements")
    return offsets, shapes, counts


def ragged_minmax(data, offsets, shapes, partials=None) -> torch.Tensor:
    """Per-sample (min, max) partials of a packed buffer of unequal volumes (data.RaggedBatch), in the layout of `minmax_partials` /
    `volume_minmax`: sample b is the prod(shapes[b]) elements at data + offsets[b], any alignment.  offsets and shapes are HOST arrays,
    checked here and then uploaded.  Returns partials (allocated unless given)."""
    offsets, shapes, counts = _ragged(data, offsets, shapes, "ragged_minmax")
    B = len(shapes)
    if partials is None:
        partials = minmax_partials(B, data.device)
    _chk(partials, torch.float32, "ragged_minmax partials", B * L.load().gvk_minmax_partials())
    L.launch.gvk_ragged_minmax(data, torch.from_numpy(offsets).to(data.device), torch.from_numpy(counts).to(data.device), partials, B)
    return partials


def conform_plan(shapes, target_shape, start, weights, inside, taps):
    """The passes of `conform_volumes` for HOST tables (data.conform_tables): an axis whose inside rows are all single taps of weight
    exactly 1 is gathered (bits moved) in the sample's first pass; every other axis is contracted in a pass of its own, the axis of largest
    reduction N / n first, so a sample takes max(1, contracted axes) passes and the batch the most any sample takes.  Returns a dict: npass,
    meta int32 [3][B][CONFORM_META], src_off / dst_off int64 [3][B] (the data offsets are added by the caller), pass_dims int32 [3][3], scratch
    (elements of intermediate storage), exact bool [B][3]."""
    shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    N = np.asarray(target_shape, dtype=np.int64)
    B, off = len(shapes), np.concatenate([[0], np.cumsum(N)])
    meta, src_off, dst_off = np.zeros((3, B, CONFORM_META), np.int32), np.zeros((3, B), np.int64), np.zeros((3, B), np.int64)
    dims, exact, scratch, npass = np.zeros((3, 3), np.int64), np.zeros((B, 3), bool), 0, 1
    for b in range(B):
        n = shapes[b]
        for a in range(3):
            rows = slice(off[a], off[a + 1])
            ins = inside[b, rows].astype(bool)
            exact[b, a] = taps[b, a] == 1 and bool((weights[b, rows, 0][ins] == 1.0).all())
        contract = sorted((a for a in range(3) if not exact[b, a]), key=lambda a: (N[a] / n[a], a))
        passes = max(1, len(contract))
        npass = max(npass, passes)
        cur = n.copy()
        for p in range(passes):
            ca = contract[p] if contract else -1
            mode = [CONFORM_CONTRACT if a == ca else
                    (CONFORM_GATHER if p == 0 else CONFORM_DONE) if exact[b, a] else
                    CONFORM_DONE if a in contract[:p] else CONFORM_KEEP for a in range(3)]
            out = np.array([cur[a] if mode[a] == CONFORM_KEEP else N[a] for a in range(3)])
            last = p == passes - 1
            meta[p, b, :14] = [1, int(p > 0), int(last), *mode, *cur, *out, ca, taps[b, ca] if ca >= 0 else 1]
            src_off[p, b] = dst_off[p - 1, b] if p else 0
            dst_off[p, b] = b * int(N.prod()) if last else scratch
            if not last:
                scratch += int(out.prod())
            dims[p] = np.maximum(dims[p], out)
            cur = out
        assert (cur == N).all()                                           # a sample's last pass leaves it on the output grid
    return dict(npass=npass, meta=meta, src_off=src_off, dst_off=dst_off, pass_dims=dims.astype(np.int32), scratch=scratch, exact=exact)


class ConformLaunch:
    """One checked and uploaded `conform_volumes` call: `run()` launches its passes and returns `out`.  It keeps the device tables alive, so
    the same conform can be launched again (tools/bench_conform.py times exactly the launches this way)."""

    def __init__(self, desc, out, keep):
        self.desc, self.out, self._keep = desc, out, keep

    def run(self) -> torch.Tensor:
        L.launch.gvk_conform_volumes(C.byref(self.desc))
        return self.out


def conform_volumes(*args, **kw) -> torch.Tensor:
    """`conform_prepare(...).run()`: a packed buffer of unequal float32 volumes onto the uniform grid, returned as out [B][D][H][W]."""
    return conform_prepare(*args, **kw).run()


def conform_prepare(data, offsets, shapes, start, weights, inside, taps, target_shape, pad_value: float = 0.0, partials=None, out=None,
                    scratch=None) -> ConformLaunch:
    """A packed buffer of unequal float32 volumes onto the uniform grid out [B][D][H][W] through the per-axis banded tables of
    `data.conform_tables` (start, inside [B][D + H + W], weights [B][D + H + W][T], taps [B][3] = each sample's own band per axis): up to three
    streaming passes planned by `conform_plan`.  offsets, shapes and all four tables are HOST arrays: every index they imply is checked here,
    then they are uploaded.  pad_value fills voxels outside a sample; with partials (ragged_minmax of the same buffer) the sample's own minimum
    does, read on the device.  out and the scratch of the intermediate passes are allocated unless given; neither may overlap data."""
    offsets, shapes, _ = _ragged(data, offsets, shapes, "conform_volumes")
    B, N = len(shapes), tuple(int(v) for v in target_shape)
    if len(N) != 3 or min(N) < 1:
        raise L.GavikoHipError(f"conform_volumes: target_shape is three positive lengths, not {target_shape!r}")
    S = sum(N)
    start, inside = np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(inside).astype(np.int32)
    weights, taps = np.ascontiguousarray(weights, dtype=np.float32), np.ascontiguousarray(taps, dtype=np.int64)
    if start.shape != (B, S) or inside.shape != (B, S) or weights.ndim != 3 or weights.shape[:2] != (B, S) or taps.shape != (B, 3):
        raise L.GavikoHipError(f"conform_volumes: start, inside [B = {B}][{S}], weights [B][{S}][T] and taps [B][3] expected")
    T = weights.shape[2]
    if not 1 <= T <= CONFORM_MAX_TAPS or (taps < 1).any() or (taps > T).any():
        raise L.GavikoHipError(f"conform_volumes: 1..{CONFORM_MAX_TAPS} taps per row and 1 <= taps <= T = {T}")
    if not np.isfinite(weights).all():
        raise L.GavikoHipError("conform_volumes: weights must be finite")
    off = np.concatenate([[0], np.cumsum(N)])
    for a in range(3):                                                  # every read an inside row implies lies inside its sample
        rows = slice(off[a], off[a + 1])
        ins = inside[:, rows] != 0
        bad = ins & ((start[:, rows] < 0) | (start[:, rows] + taps[:, a:a + 1] > shapes[:, a:a + 1]))
        if bad.any():
            b, q = np.argwhere(bad)[0]
            raise L.GavikoHipError(f"conform_volumes: sample {b}, axis {a}, row {q} reads [{start[b, off[a] + q]}, +{taps[b, a]}) of {shapes[b, a]} voxels")
    plan = conform_plan(shapes, N, start, weights, inside, taps)
    dims = plan["pass_dims"]
    for p in range(plan["npass"]):
        if (int(dims[p][0]) + 7) // 8 * B > 65535 or (int(dims[p][1]) + 3) // 4 > 65535:
            raise L.GavikoHipError(f"conform_volumes: pass {p} of {tuple(dims[p])} voxels per sample x {B} samples exceeds the launch grid")
    plan["src_off"][0] += offsets
    dev = data.device
    if out is None:
        out = torch.empty((B,) + N, dtype=torch.float32, device=dev)
    _chk(out, torch.float32, "conform_volumes out", B * N[0] * N[1] * N[2])
    if plan["scratch"] and scratch is None:
        scratch = torch.empty(plan["scratch"], dtype=torch.float32, device=dev)
    if plan["scratch"]:
        _chk(scratch, torch.float32, "conform_volumes scratch", plan["scratch"])
    if partials is not None:
        _chk(partials, torch.float32, "conform_volumes partials", B * L.load().gvk_minmax_partials())
    tabs = [torch.from_numpy(t).to(dev) for t in (plan["src_off"], plan["dst_off"], plan["meta"], start, inside, weights)]
    d = L.ConformDesc(data=L.ptr(data), scratch=L.ptr(scratch) if plan["scratch"] else None, out=L.ptr(out),
                      src_off=L.ptr(tabs[0]), dst_off=L.ptr(tabs[1]), meta=L.ptr(tabs[2]), start=L.ptr(tabs[3]), inside=L.ptr(tabs[4]),
                      weights=L.ptr(tabs[5]), partials=L.ptr(partials) if partials is not None else None,
                      B=B, D=N[0], H=N[1], W=N[2], T=T, npass=plan["npass"], pad_min=int(partials is not None),
                      pad_value=float(pad_value), **{f"p{p}d{a}": int(dims[p][a]) for p in range(3) for a in range(3)})
    return ConformLaunch(d, out, tabs + [data, scratch, partials])


def eval_rows(logits, target, proba, pred, confusion) -> None:
    _chk(logits, torch.float32, "eval_rows logits")
    N, K = logits.shape
    _chk(proba, torch.float32, "eval_rows proba", N * K)
    _chk(pred, torch.int32, "eval_rows pred", N)
    _chk(confusion, torch.int64, "eval_rows confusion", K * K)
    if target.dtype != torch.int64 or target.numel() != N or not target.is_contiguous():
        raise ValueError("eval_rows target must be a contiguous int64 [N] tensor")
    L.launch.gvk_eval_rows(logits, target, proba, pred, confusion, N, K)


def ovr_auc_counts(proba, target, counts) -> None:
    """counts[c] += {2 #{p_i > p_j} + #{p_i == p_j}, n_pos, n_neg} over positives i (target == c) and negatives j of column c of proba
    f32 [N, K].  The kernel ADDS to counts (int64 [K][3]): the caller zeroes the buffer, and a second call on it accumulates."""
    _chk(proba, torch.float32, "ovr_auc proba")
    N, K = proba.shape
    _chk(counts, torch.int64, "ovr_auc counts", 3 * K)
    if not target.is_cuda or target.dtype != torch.int64 or target.numel() != N or not target.is_contiguous():
        raise ValueError("ovr_auc_counts target must be a contiguous int64 [N] tensor on the device")
    L.launch.gvk_ovr_auc_counts(proba, target, counts, N, K)


def dropout_rows(x, drop_p, seed, seed_ptr, out32=None, out16=None, M=None, N=None, rows_in=0, rows_out=0, row_off=0):
    """out = x * mask / (1 - p) over logical rows (optionally a row range of every sample); out32 may be x itself."""
    _chk(x, torch.float32, "dropout_rows x")
    ld = x.shape[-1]
    N = ld if N is None else N
    M = x.numel() // ld if M is None else M
    if out32 is not None:
        _chk(out32, torch.float32, "dropout_rows out32")
    if out16 is not None:
        _chk(out16, torch.bfloat16, "dropout_rows out16")
    d = L.DropoutDesc(x=L.ptr(x), out32=L.ptr(out32) if out32 is not None else None, out16=L.ptr(out16) if out16 is not None else None,
                      seed_ptr=L.ptr(seed_ptr), M=M, N=N, ld=ld, rows_in=rows_in, rows_out=rows_out, row_off=row_off, drop_p=float(drop_p), seed=int(seed))
    L.launch.gvk_dropout_rows(C.byref(d))


# ---- predictive uncertainty and calibration (csrc/uncertainty.hip) ----
STATS_MAX_CLASSES = 256         # gvk_predictive_stats: 4 classes per lane of one wave, in registers
CALIBRATION_MAX_BINS = 254      # gvk_calibration_bins: one thread of the workgroup per bin (+ one each for the Brier and NLL sums)


def tta_volumes(x: torch.Tensor, src: torch.Tensor, flip: torch.Tensor, out: torch.Tensor) -> None:
    """out[o] = x[src[o]] mirrored along the axes named by the bits of flip[o] (bit 0 = D, bit 1 = H, bit 2 = W), bit for bit; flip[o] = 0 is a
    plain replica.  x f32 [S,1,D,H,W], out f32 [Bout,1,D,H,W] (not overlapping x), src / flip i32 [Bout] device tables (src within [0, S))."""
    _chk(x, torch.float32, "tta_volumes x")
    _chk(out, torch.float32, "tta_volumes out")
    if x.dim() != 5 or out.dim() != 5 or x.shape[1] != 1 or tuple(out.shape[1:]) != tuple(x.shape[1:]) or x.shape[0] < 1 or out.shape[0] < 1 \
            or min(x.shape[2:]) < 1:
        raise L.GavikoHipError(f"tta_volumes: expected x [S,1,D,H,W] and out [Bout,1,D,H,W], got {tuple(x.shape)} and {tuple(out.shape)}")
    S, _, D, H, W = x.shape
    Bout = out.shape[0]
    _tab(src, "tta_volumes src", Bout)
    _tab(flip, "tta_volumes flip", Bout)
    xe, oe = x.data_ptr() + x.numel() * 4, out.data_ptr() + out.numel() * 4
    if not (oe <= x.data_ptr() or xe <= out.data_ptr()):
        raise L.GavikoHipError("tta_volumes: out must not overlap x")
    if Bout * D * H * W >= 1 << 31:
        raise L.GavikoHipError(f"tta_volumes: {Bout} x {D * H * W} voxels per launch exceed the kernel's 32-bit index range")
    L.launch.gvk_tta_volumes(x, src, flip, out, Bout, S, D, H, W)


def predictive_stats(member_logits: torch.Tensor, B: int, S: int, out: dict = None) -> dict:
    """member_logits f32 [B, S, K] (B samples, S members each) -> dict of device tensors: probs f32 [B, K] (mean member softmax), pred i32 [B]
    (its argmax, lowest index on a tie), entropy / expected_entropy / mutual_info / variation_ratio f32 [B] (nats; mutual_info clamped at 0),
    std f32 [B, K] (population), votes i32 [B, K] (the members' own argmax counts).  `out`: the same dict, to write into existing tensors."""
    _chk(member_logits, torch.float32, "predictive_stats member_logits")
    B, S = int(B), int(S)
    if S < 1:
        raise L.GavikoHipError(f"predictive_stats: S = {S} members (at least 1)")
    if B < 1 or member_logits.numel() % (B * S) or member_logits.numel() == 0:
        raise L.GavikoHipError(f"predictive_stats: {tuple(member_logits.shape)} is not [B = {B}, S = {S}, K]")
    K = member_logits.numel() // (B * S)
    if not 2 <= K <= STATS_MAX_CLASSES:
        raise L.GavikoHipError(f"predictive_stats: K = {K} classes outside [2, {STATS_MAX_CLASSES}] (one wave keeps 4 classes per lane in registers)")
    dev = member_logits.device
    spec = {"probs": ((B, K), torch.float32), "pred": ((B,), torch.int32), "entropy": ((B,), torch.float32),
            "expected_entropy": ((B,), torch.float32), "mutual_info": ((B,), torch.float32), "variation_ratio": ((B,), torch.float32),
            "std": ((B, K), torch.float32), "votes": ((B, K), torch.int32)}
    if out is None:
        out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in spec.items()}
    for k, (shape, dt) in spec.items():
        if k not in out:
            raise L.GavikoHipError(f"predictive_stats out: {k!r} is missing")
        _chk(out[k], dt, "predictive_stats " + k)
        if tuple(out[k].shape) != shape:
            raise L.GavikoHipError(f"predictive_stats {k}: expected {shape}, got {tuple(out[k].shape)}")
    L.launch.gvk_predictive_stats(member_logits, out["probs"], out["pred"], out["entropy"], out["expected_entropy"], out["mutual_info"], out["variation_ratio"],
                                  out["std"], out["votes"], B, S, K)
    return out


def calibration_bins(proba: torch.Tensor, target: torch.Tensor, nbins: int, out: dict = None) -> dict:
    """proba f32 [N, K], target i64 [N] (within [0, K): the caller's contract) -> dict of device tensors over the equal-width confidence bins
    (i / nbins, (i + 1) / nbins]: count i64 [nbins], correct i64 [nbins], conf_sum f64 [nbins]; brier f64 [1], nll f64 [1] (sums over the rows)."""
    _chk(proba, torch.float32, "calibration_bins proba")
    if proba.dim() != 2 or proba.shape[0] < 1 or proba.shape[1] < 1:
        raise L.GavikoHipError(f"calibration_bins proba: expected [N, K], got {tuple(proba.shape)}")
    N, K = proba.shape
    _chk(target, torch.int64, "calibration_bins target")
    if target.numel() != N:
        raise L.GavikoHipError(f"calibration_bins target: expected {N} labels, got {tuple(target.shape)}")
    if isinstance(nbins, bool) or not isinstance(nbins, int) or not 1 <= nbins <= CALIBRATION_MAX_BINS:
        raise L.GavikoHipError(f"calibration_bins: nbins = {nbins!r} outside [1, {CALIBRATION_MAX_BINS}] (one thread of the workgroup per bin)")
    dev = proba.device
    spec = {"count": (nbins, torch.int64), "correct": (nbins, torch.int64), "conf_sum": (nbins, torch.float64), "brier": (1, torch.float64),
            "nll": (1, torch.float64)}
    if out is None:
        out = {k: torch.empty(n, dtype=dt, device=dev) for k, (n, dt) in spec.items()}
    for k, (n, dt) in spec.items():
        if k not in out:
            raise L.GavikoHipError(f"calibration_bins out: {k!r} is missing")
        _chk(out[k], dt, "calibration_bins " + k)
        if out[k].numel() != n:
            raise L.GavikoHipError(f"calibration_bins {k}: expected {n} entries, got {tuple(out[k].shape)}")
    L.launch.gvk_calibration_bins(proba, target, out["count"], out["correct"], out["conf_sum"], out["brier"], out["nll"], N, K, nbins)
    return out


# ---- bootstrap replicates of the evaluation metrics (csrc/bootstrap.hip) ----
BOOTSTRAP_MAX_ROWS = 8192       # gvk_bootstrap_counts: one workgroup keeps the multiplicities and the scan of a replicate in LDS
BOOTSTRAP_MAX_CLASSES = 64


def _i32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.int32).contiguous()


def _class_groups(labels: torch.Tensor, K: int):
    """labels i64 [N] -> (class_rows i32 [N]: the rows grouped by label, ascending inside a label; class_off i32 [K + 1]: where every label's rows
    start).  The stratified draw of the replicate kernels reads them, and the Mondrian segments of conformal_tables are the same groups."""
    off = torch.zeros(K + 1, dtype=torch.int64, device=labels.device)
    off[1:] = torch.cumsum(torch.bincount(labels, minlength=K)[:K], 0)
    return _i32(torch.sort(labels, stable=True).indices), _i32(off)


def _tie_groups(vals: torch.Tensor):
    """vals [..., N] sorted along the last dimension -> (gstart, gend) i64 [..., N]: per position the bounds [gstart, gend) of its run of
    equal values."""
    N = vals.shape[-1]
    pos = torch.arange(N, device=vals.device).expand(vals.shape)
    step = vals[..., 1:] != vals[..., :-1]
    edge = torch.ones(vals.shape[:-1] + (1,), dtype=torch.bool, device=vals.device)
    gstart = torch.cummax(torch.where(torch.cat([edge, step], -1), pos, torch.zeros_like(pos)), -1).values
    gend = torch.cummin(torch.where(torch.cat([step, edge], -1), pos + 1, torch.full_like(pos, N)).flip(-1), -1).values.flip(-1)
    return gstart, gend


def _replicate_rows(what: str, N: int) -> None:
    if not 1 <= N <= BOOTSTRAP_MAX_ROWS:
        raise L.GavikoHipError(f"{what}: N = {N} rows outside [1, {BOOTSTRAP_MAX_ROWS}] (one workgroup keeps a replicate in LDS)")


def _replicates(what: str, R) -> int:
    if isinstance(R, bool) or not isinstance(R, int) or R < 1:
        raise L.GavikoHipError(f"{what}: replicates = {R!r} (an integer >= 1)")
    return R


def _seed64(seed) -> int:
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def bootstrap_tables(proba: torch.Tensor, labels: torch.Tensor) -> dict:
    """The per-call tables of gvk_bootstrap_counts, built with torch on the device (plumbing: once per call, not per replicate).
    proba f32 [N, K], labels i64 [N] within [0, K) -> order / gstart / gend i32 [K, N] (the rows in ascending order of every class column,
    stable; per sorted position the bounds of its group of equal scores), class_rows i32 [N], class_off i32 [K + 1] (rows grouped by label)."""
    vals, order = torch.sort(proba.t().contiguous(), dim=1, stable=True)
    gstart, gend = _tie_groups(vals)
    class_rows, class_off = _class_groups(labels, proba.shape[1])
    return {"order": _i32(order), "gstart": _i32(gstart), "gend": _i32(gend), "class_rows": class_rows, "class_off": class_off}


def bootstrap_counts(labels: torch.Tensor, pred: torch.Tensor, tables: dict, replicates: int, seed: int, stratified: bool,
                     confusion: torch.Tensor = None, auc_counts: torch.Tensor = None):
    """R = replicates resamples of the N rows -> (confusion i64 [R, K, K], auc_counts i64 [R, K, 3]), exact integers (include/gaviko_hip.h states
    the two resampling rules).  labels i64 [N] within [0, K) and pred i32 [N] (the caller's contract, as the tables' values are: the kernel
    clamps what it reads), tables = bootstrap_tables(proba, labels).  2 <= K <= 64, N <= 8192."""
    _chk(labels, torch.int64, "bootstrap_counts labels")
    N = labels.numel()
    order = tables.get("order")
    if order is None or order.dim() != 2 or order.shape[1] != N:
        raise L.GavikoHipError(f"bootstrap_counts order: expected an int32 [K, {N}] table, got {None if order is None else tuple(order.shape)}")
    K = order.shape[0]
    _tab(order, "bootstrap_counts order", K * N)
    _replicate_rows("bootstrap_counts", N)
    if not 2 <= K <= BOOTSTRAP_MAX_CLASSES:
        raise L.GavikoHipError(f"bootstrap_counts: K = {K} classes outside [2, {BOOTSTRAP_MAX_CLASSES}]")
    R = _replicates("bootstrap_counts", replicates)
    _tab(pred, "bootstrap_counts pred", N)
    _tab(tables.get("gstart"), "bootstrap_counts gstart", K * N)
    _tab(tables.get("gend"), "bootstrap_counts gend", K * N)
    _tab(tables.get("class_rows"), "bootstrap_counts class_rows", N)
    _tab(tables.get("class_off"), "bootstrap_counts class_off", K + 1)
    dev = labels.device
    if confusion is None:
        confusion = torch.empty((R, K, K), dtype=torch.int64, device=dev)
    if auc_counts is None:
        auc_counts = torch.empty((R, K, 3), dtype=torch.int64, device=dev)
    _chk(confusion, torch.int64, "bootstrap_counts confusion")
    _chk(auc_counts, torch.int64, "bootstrap_counts auc_counts")
    if confusion.numel() != R * K * K or auc_counts.numel() != R * K * 3:
        raise L.GavikoHipError(f"bootstrap_counts: expected confusion [{R}, {K}, {K}] and auc_counts [{R}, {K}, 3], got {tuple(confusion.shape)} and "
                               f"{tuple(auc_counts.shape)}")
    L.launch.gvk_bootstrap_counts(labels, pred, tables["order"], tables["gstart"], tables["gend"], tables["class_rows"], tables["class_off"], confusion,
                                  auc_counts, N, K, R, _seed64(seed), 1 if stratified else 0)
    return confusion, auc_counts


# ---- selective prediction and temperature scaling (csrc/selective.hip) ----
RISK_COVERAGE_MAX_NEEDS = 8     # gvk_risk_coverage: accepted-row counts answered per launch
TEMPERATURE_MAX_CLASSES = 64    # gvk_temperature_fit


def selective_tables(score: torch.Tensor, labels: torch.Tensor) -> dict:
    """The per-call tables of gvk_risk_coverage, built with torch on the device (plumbing: once per call, not per replicate).
    score f32 [N] (higher = more confident, no NaN), labels i64 [N] >= 0 -> order i32 [N] (the rows by descending score, stable), gend i32 [N]
    (per sorted position, one past the end of its group of equal scores), class_rows i32 [N] / class_off i32 [K + 1] (the rows grouped by
    label, as ops.bootstrap_tables has them; K = the largest label + 1) and sorted_score f32 [N] (score[order], for the thresholds)."""
    N = score.numel()
    vals, order = torch.sort(score.reshape(N), descending=True, stable=True)
    class_rows, class_off = _class_groups(labels, int(labels.max()) + 1 if N else 1)
    return {"order": _i32(order), "gend": _i32(_tie_groups(vals)[1]), "class_rows": class_rows, "class_off": class_off,
            "sorted_score": vals.contiguous()}


def risk_coverage_counts(labels: torch.Tensor, pred: torch.Tensor, tables: dict, need=(), replicates: int = 1, seed: int = 0,
                         stratified: bool = False, resample: bool = True) -> dict:
    """The risk-coverage integers of `replicates` resamples (resample=True: the multiplicities of gvk_bootstrap_counts for the same seed and
    rule) or of the full sample (resample=False, replicates must be 1, which also writes the curve); include/gaviko_hip.h has the
    definitions.  labels i64 [N], pred i32 [N], tables = selective_tables(score, labels); need: up to 8 host integers within [1, N], ascending
    (accepted-row counts).  -> dict of device tensors: aurc f64 [R], at i32 [R, Q, 2], total i32 [R, 2] and, with resample=False, accepted /
    errors i32 [N] (per sorted position the running (accepted, wrong) counts at the end of its tie group).  N <= 8192."""
    N = labels.numel()
    _replicate_rows("risk_coverage_counts", N)
    R = _replicates("risk_coverage_counts", replicates)
    if not resample and R != 1:
        raise L.GavikoHipError(f"risk_coverage_counts: resample=False is the full sample, replicates = {R} must be 1")
    need = [n for n in need]
    Q = len(need)
    if Q > RISK_COVERAGE_MAX_NEEDS:
        raise L.GavikoHipError(f"risk_coverage_counts: Q = {Q} accepted-row counts (at most {RISK_COVERAGE_MAX_NEEDS} per launch)")
    if any(isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= N for n in need) or any(a > b for a, b in zip(need, need[1:])):
        raise L.GavikoHipError(f"risk_coverage_counts: need = {need!r} (ascending integers within [1, {N}])")
    class_off = tables.get("class_off")
    if class_off is None or class_off.numel() < 2:
        raise L.GavikoHipError("risk_coverage_counts class_off: expected an int32 [K + 1] table, K >= 1")
    K = class_off.numel() - 1
    if K > BOOTSTRAP_MAX_CLASSES:
        raise L.GavikoHipError(f"risk_coverage_counts: K = {K} classes outside [1, {BOOTSTRAP_MAX_CLASSES}]")
    _chk(labels, torch.int64, "risk_coverage_counts labels")
    _tab(pred, "risk_coverage_counts pred", N)
    _tab(tables.get("order"), "risk_coverage_counts order", N)
    _tab(tables.get("gend"), "risk_coverage_counts gend", N)
    _tab(tables.get("class_rows"), "risk_coverage_counts class_rows", N)
    _tab(class_off, "risk_coverage_counts class_off", K + 1)
    dev = labels.device
    out = {"aurc": torch.empty(R, dtype=torch.float64, device=dev), "at": torch.empty((R, Q, 2), dtype=torch.int32, device=dev),
           "total": torch.empty((R, 2), dtype=torch.int32, device=dev)}
    if not resample:
        out["accepted"] = torch.empty(N, dtype=torch.int32, device=dev)
        out["errors"] = torch.empty(N, dtype=torch.int32, device=dev)
    need_d = torch.tensor(need, dtype=torch.int32, device=dev) if Q else None
    L.launch.gvk_risk_coverage(labels, pred, tables["order"], tables["gend"], tables["class_rows"], class_off, need_d, out["aurc"], out["at"] if Q else None,
                               out["total"], out.get("accepted"), out.get("errors"), N, K, Q, R, _seed64(seed), 1 if stratified else 0,
                               1 if resample else 0)
    return out


def temperature_fit(logits: torch.Tensor, target: torch.Tensor, t_min: float = 0.05, t_max: float = 20.0, state: torch.Tensor = None) -> torch.Tensor:
    """logits f32 [N, K] (finite: the caller's contract), target i64 [N] within [0, K) -> state f64 [8] on the device = (T, beta = 1 / T,
    nll_before, nll_after, f', f'', iterations, flags: bit 0 converged, bit 1 at_bound): the temperature within [t_min, t_max] that minimises
    the mean NLL of softmax(logits / T), by one launch of gvk_temperature_fit (include/gaviko_hip.h).  2 <= K <= 64."""
    if logits.dim() != 2 or logits.shape[0] < 1:
        raise L.GavikoHipError(f"temperature_fit logits: expected [N, K], got {tuple(logits.shape)}")
    N, K = logits.shape
    if not 2 <= K <= TEMPERATURE_MAX_CLASSES:
        raise L.GavikoHipError(f"temperature_fit: K = {K} classes outside [2, {TEMPERATURE_MAX_CLASSES}]")
    if N >= 1 << 31:
        raise L.GavikoHipError(f"temperature_fit: N = {N} rows exceed the kernel's 32-bit row index")
    if target.numel() != N:
        raise L.GavikoHipError(f"temperature_fit target: expected {N} labels, got {tuple(target.shape)}")
    t_min, t_max = float(t_min), float(t_max)
    if not 0.0 < t_min < t_max < float("inf"):
        raise L.GavikoHipError(f"temperature_fit: need 0 < t_min < t_max, finite (got {t_min!r}, {t_max!r})")
    _chk(logits, torch.float32, "temperature_fit logits")
    _chk(target, torch.int64, "temperature_fit target")
    if state is None:
        state = torch.empty(8, dtype=torch.float64, device=logits.device)
    _chk(state, torch.float64, "temperature_fit state")
    if state.numel() != 8:
        raise L.GavikoHipError(f"temperature_fit state: expected 8 entries, got {tuple(state.shape)}")
    L.launch.gvk_temperature_fit(logits, target, state, N, K, t_min, t_max)
    return state


# ---- ROC operating points of a binary reading (csrc/roc.hip) ----
ROC_MAX_LEVELS = 8              # gvk_roc_replicates: entries of each of the three level lists answered per launch
ROC_BASIS_POINTS = 10000


def roc_tables(score: torch.Tensor, positive: torch.Tensor, strata: torch.Tensor = None) -> dict:
    """The per-call tables of gvk_roc_replicates, built with torch on the device (plumbing: once per call, not per replicate).
    score f32 [N] (higher = more positive, no NaN), positive [N] (bool or integers, nonzero = positive), strata i64 [N] >= 0 (the labels the
    stratified draw keeps the sizes of; default: the binary label) -> order i32 [N] (the rows by descending score, stable), gend i32 [N]
    (per sorted position, one past the end of its group of equal scores), class_rows i32 [N] / class_off i32 [K + 1] (the rows grouped by
    stratum, as ops.bootstrap_tables has them; K = the largest stratum + 1) and sorted_score f32 [N] (score[order], for the thresholds)."""
    N = score.numel()
    vals, order = torch.sort(score.reshape(N), descending=True, stable=True)
    if strata is None:
        strata = (positive.reshape(N) != 0).to(torch.int64)
    class_rows, class_off = _class_groups(strata, int(strata.max()) + 1 if N else 1)
    return {"order": _i32(order), "gend": _i32(_tie_groups(vals)[1]), "class_rows": class_rows, "class_off": class_off,
            "sorted_score": vals.contiguous()}


def _roc_levels(what: str, levels, hi: int) -> list:
    levels = [v for v in levels]
    if len(levels) > ROC_MAX_LEVELS:
        raise L.GavikoHipError(f"roc_counts: {len(levels)} {what} entries (at most {ROC_MAX_LEVELS} per launch)")
    if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= hi for v in levels):
        raise L.GavikoHipError(f"roc_counts: {what} = {levels!r} (integers within [0, {hi}])")
    return levels


def roc_counts(positive: torch.Tensor, strata: torch.Tensor, tables: dict, spec_bp=(), sens_bp=(), cut_rows=(), replicates: int = 1,
               seed: int = 0, stratified: bool = False, resample: bool = True, curve: bool = False) -> dict:
    """The ROC integers of `replicates` resamples (resample=True: the multiplicities of gvk_bootstrap_counts / gvk_risk_coverage for the same
    seed and rule) or of the full sample (resample=False, replicates must be 1; curve=True then also writes the curve); include/gaviko_hip.h has
    the definitions.  positive i32 [N] (nonzero = positive), strata i64 [N] (the labels of the stratified draw; None unless stratified),
    tables = roc_tables(score, positive, strata); spec_bp / sens_bp: up to 8 host integers each, levels in basis points within [0, 10000];
    cut_rows: up to 8 host integers within [0, N] (rows at or above a fixed threshold).  -> dict of device tensors: total i32 [R, 2] = (Pn, Nn),
    auc2 i64 [R], ap f64 [R] (average precision, NaN without a positive row), at_spec / at_sens / at_cut i32 [R, Q, 2] = (TP, FP), youden i32
    [R, 3] = (TP, FP, sorted position) and, with curve=True, tp / fp i32 [N] (per sorted position the counts at the end of its tie group).
    N <= 8192."""
    N = positive.numel()
    _replicate_rows("roc_counts", N)
    R = _replicates("roc_counts", replicates)
    if not resample and R != 1:
        raise L.GavikoHipError(f"roc_counts: resample=False is the full sample, replicates = {R} must be 1")
    if curve and resample:
        raise L.GavikoHipError("roc_counts: the curve is written with resample=False only")
    spec_bp = _roc_levels("spec_bp", spec_bp, ROC_BASIS_POINTS)
    sens_bp = _roc_levels("sens_bp", sens_bp, ROC_BASIS_POINTS)
    cut_rows = _roc_levels("cut_rows", cut_rows, N)
    class_off = tables.get("class_off")
    if class_off is None or class_off.numel() < 2:
        raise L.GavikoHipError("roc_counts class_off: expected an int32 [K + 1] table, K >= 1")
    K = class_off.numel() - 1
    if K > BOOTSTRAP_MAX_CLASSES:
        raise L.GavikoHipError(f"roc_counts: K = {K} strata outside [1, {BOOTSTRAP_MAX_CLASSES}]")
    if resample and stratified and strata is None:
        raise L.GavikoHipError("roc_counts: the stratified draw needs the strata labels")
    _tab(positive, "roc_counts positive", N)
    _chk(strata, torch.int64, "roc_counts strata")
    if strata is not None and strata.numel() != N:
        raise L.GavikoHipError(f"roc_counts strata: expected {N} labels, got {tuple(strata.shape)}")
    _tab(tables.get("order"), "roc_counts order", N)
    _tab(tables.get("gend"), "roc_counts gend", N)
    _tab(tables.get("class_rows"), "roc_counts class_rows", N)
    _tab(class_off, "roc_counts class_off", K + 1)
    dev = positive.device
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)   # noqa: E731
    Qs, Qn, Qc = len(spec_bp), len(sens_bp), len(cut_rows)
    out = {"total": i32(R, 2), "auc2": torch.empty(R, dtype=torch.int64, device=dev), "ap": torch.empty(R, dtype=torch.float64, device=dev),
           "at_spec": i32(R, Qs, 2), "at_sens": i32(R, Qn, 2), "at_cut": i32(R, Qc, 2), "youden": i32(R, 3)}
    if curve:
        out["tp"], out["fp"] = i32(N), i32(N)
    levels = torch.tensor(spec_bp + sens_bp + cut_rows, dtype=torch.int32, device=dev) if Qs + Qn + Qc else None      # one upload for the three lists
    lv = lambda a, n: levels[a:a + n] if n else None                        # noqa: E731
    L.launch.gvk_roc_replicates(strata, positive, tables["order"], tables["gend"], tables["class_rows"], class_off, lv(0, Qs), lv(Qs, Qn),
                                lv(Qs + Qn, Qc), out["total"], out["auc2"], out["ap"], out["at_spec"] if Qs else None, out["at_sens"] if Qn else None,
                                out["at_cut"] if Qc else None, out["youden"], out.get("tp"), out.get("fp"), N, K, Qs, Qn, Qc, R, _seed64(seed),
                                1 if stratified else 0, 1 if resample else 0)
    return out


# ---- split-conformal prediction sets (csrc/conformal.hip) ----
CONFORMAL_MAX_CLASSES = 64      # gvk_conformal_scores: one class per lane of a wave
CONFORMAL_MAX_LEVELS = 8        # gvk_conformal_splits: miscoverage levels answered per launch
CONFORMAL_KINDS = {"lac": 0, "aps": 1, "raps": 2}


def conformal_scores(proba: torch.Tensor, kind: str = "lac", randomized: bool = False, seed: int = 0, k_reg: int = 1, lam: float = 0.01,
                     scores: torch.Tensor = None) -> torch.Tensor:
    """proba f32 [N, K] -> scores f32 [K, N] (class-major), the nonconformity scores of include/gaviko_hip.h: kind 'lac' (1 - p), 'aps' (the
    probability mass down to and including the class, in rank order; randomized=True: u_n of the class's own mass, u_n from (seed, row)) or
    'raps' (aps + lam * max(0, rank + 1 - k_reg)).  2 <= K <= 64; NaN probabilities are the caller's contract."""
    if not isinstance(proba, torch.Tensor):
        raise L.GavikoHipError(f"conformal_scores proba: expected a tensor, got {type(proba).__name__}")
    if proba.dim() != 2 or proba.shape[0] < 1:
        raise L.GavikoHipError(f"conformal_scores proba: expected [N, K], got {tuple(proba.shape)}")
    N, K = proba.shape
    if not 2 <= K <= CONFORMAL_MAX_CLASSES:
        raise L.GavikoHipError(f"conformal_scores: K = {K} classes outside [2, {CONFORMAL_MAX_CLASSES}] (one class per lane)")
    if N * K >= 1 << 31:
        raise L.GavikoHipError(f"conformal_scores: N = {N} rows exceed the kernel's 32-bit row index")
    if kind not in CONFORMAL_KINDS:
        raise L.GavikoHipError(f"conformal_scores: kind = {kind!r} (one of {sorted(CONFORMAL_KINDS)})")
    if randomized and kind == "lac":
        raise L.GavikoHipError("conformal_scores: lac has no randomised form")
    if isinstance(k_reg, bool) or not isinstance(k_reg, int) or k_reg < 0:
        raise L.GavikoHipError(f"conformal_scores: k_reg = {k_reg!r} (an integer >= 0)")
    lam = float(lam)
    if not 0.0 <= lam < float("inf"):
        raise L.GavikoHipError(f"conformal_scores: lam = {lam!r} (a finite number >= 0)")
    _chk(proba, torch.float32, "conformal_scores proba")
    if scores is None:
        scores = torch.empty((K, N), dtype=torch.float32, device=proba.device)
    _chk(scores, torch.float32, "conformal_scores scores")
    if tuple(scores.shape) != (K, N):
        raise L.GavikoHipError(f"conformal_scores scores: expected [{K}, {N}] (class-major), got {tuple(scores.shape)}")
    L.launch.gvk_conformal_scores(proba, scores, N, K, CONFORMAL_KINDS[kind], 1 if randomized else 0, _seed64(seed), min(k_reg, K + 1),
                                  lam)
    return scores


def conformal_tables(scores: torch.Tensor, labels: torch.Tensor, mondrian: bool = False) -> dict:
    """The per-call tables of gvk_conformal_splits, built with torch (plumbing: once per call, not per replicate).  scores f32 [K, N]
    (class-major, no NaN), labels i64 [N] within [0, K) -> order i32 [N] (the rows grouped by segment -- one segment, or with mondrian=True one
    per label -- and inside a segment ascending by true-class score, stable), seg_off i32 [G + 1], and sorted_score f32 [N] (the true-class
    score of the row at every sorted position: what a qpos of the kernel stands for)."""
    K, N = scores.shape
    true = scores[labels, torch.arange(N, device=scores.device)]
    order = torch.sort(true, stable=True).indices
    if mondrian:
        order = order[torch.sort(labels[order], stable=True).indices]
        seg_off = _class_groups(labels, K)[1]
    else:
        seg_off = torch.tensor([0, N], dtype=torch.int32, device=scores.device)
    return {"order": _i32(order), "seg_off": seg_off, "sorted_score": true[order].contiguous()}


def conformal_splits(scores: torch.Tensor, labels: torch.Tensor, tables: dict, alphas, n_cal: int, replicates: int = 1, seed: int = 0) -> dict:
    """`replicates` random splits of the N rows into n_cal calibration rows and N - n_cal test rows (n_cal = N: no test rows), the conformal
    thresholds of every segment at up to 8 miscoverage levels `alphas` (host floats within (0, 1)) and the test rows' set-size and coverage
    counts; include/gaviko_hip.h has the definitions.  scores f32 [K, N] = conformal_scores(...), labels i64 [N], tables =
    conformal_tables(scores, labels, mondrian).  -> dict of int32 device tensors: qpos [R, Q, G], n_seg [R, G], size_hist / covered_by_size
    [R, Q, K + 1], class_test [R, K], class_covered [R, Q, K].  N <= 8192, 2 <= K <= 64."""
    if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
        raise L.GavikoHipError(f"conformal_splits scores: expected a class-major [K, N] tensor, got "
                               f"{tuple(scores.shape) if isinstance(scores, torch.Tensor) else type(scores).__name__}")
    K, N = scores.shape
    _replicate_rows("conformal_splits", N)
    if not 2 <= K <= CONFORMAL_MAX_CLASSES:
        raise L.GavikoHipError(f"conformal_splits: K = {K} classes outside [2, {CONFORMAL_MAX_CLASSES}]")
    R = _replicates("conformal_splits", replicates)
    if isinstance(n_cal, bool) or not isinstance(n_cal, int) or not 1 <= n_cal <= N:
        raise L.GavikoHipError(f"conformal_splits: n_cal = {n_cal!r} (an integer within [1, {N}])")
    try:
        alphas = [float(a) for a in alphas]
    except TypeError:
        raise L.GavikoHipError(f"conformal_splits: alphas = {alphas!r} (a sequence of numbers)") from None
    Q = len(alphas)
    if not 1 <= Q <= CONFORMAL_MAX_LEVELS:
        raise L.GavikoHipError(f"conformal_splits: Q = {Q} levels outside [1, {CONFORMAL_MAX_LEVELS}] per launch")
    if any(not 0.0 < a < 1.0 for a in alphas):
        raise L.GavikoHipError(f"conformal_splits: alphas = {alphas!r} (each within (0, 1))")
    seg_off = tables.get("seg_off")
    if seg_off is None or seg_off.numel() not in (2, K + 1):
        raise L.GavikoHipError(f"conformal_splits seg_off: expected an int32 [2] (marginal) or [{K + 1}] (one segment per class) table")
    G = seg_off.numel() - 1
    _chk(scores, torch.float32, "conformal_splits scores")
    _chk(labels, torch.int64, "conformal_splits labels")
    if labels.numel() != N:
        raise L.GavikoHipError(f"conformal_splits labels: expected {N} labels, got {tuple(labels.shape)}")
    _tab(tables.get("order"), "conformal_splits order", N)
    _tab(seg_off, "conformal_splits seg_off", G + 1)
    dev = scores.device
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)   # noqa: E731
    out = {"qpos": i32(R, Q, G), "n_seg": i32(R, G), "size_hist": i32(R, Q, K + 1), "covered_by_size": i32(R, Q, K + 1), "class_test": i32(R, K),
           "class_covered": i32(R, Q, K)}
    alphas_d = torch.tensor(alphas, dtype=torch.float64, device=dev)
    L.launch.gvk_conformal_splits(scores, labels, tables["order"], seg_off, alphas_d, out["qpos"], out["n_seg"], out["size_hist"], out["covered_by_size"],
                                  out["class_test"], out["class_covered"], N, K, Q, G, n_cal, R, _seed64(seed))
    return out


# ---- feature embeddings and kNN probes (csrc/features.hip) ----
FEATURE_MAX_DIM = 1024          # gvk_token_pool / gvk_feature_topk: C % 4 == 0, C <= 1024
TOPK_MAX_K = 32                 # gvk_feature_topk / gvk_knn_vote: sorted lists of at most 32 entries
VOTE_MAX_CLASSES = 256          # gvk_knn_vote: 4 classes per lane of one wave
TOPK_METRICS = {"ip": 0, "l2": 1}


def _feat_rows(t, what, C=None):
    """A contiguous f32 device matrix [N, C] with C a multiple of 4 within [4, 1024] -> (N, C)."""
    if not isinstance(t, torch.Tensor):
        raise L.GavikoHipError(f"{what}: expected a tensor, got {type(t).__name__}")
    _chk(t, torch.float32, what)
    if t.dim() != 2 or t.shape[0] < 1:
        raise L.GavikoHipError(f"{what}: expected [N, C], got {tuple(t.shape)}")
    N, Cc = t.shape
    if Cc < 4 or Cc % 4 or Cc > FEATURE_MAX_DIM:
        raise L.GavikoHipError(f"{what}: C = {Cc} (a multiple of 4 within [4, {FEATURE_MAX_DIM}])")
    if C is not None and Cc != C:
        raise L.GavikoHipError(f"{what}: C = {Cc}, expected {C}")
    return N, Cc


def token_pool(g: torch.Tensor, B: int, T: int, C: int, r0: int, R: int, out: torch.Tensor = None) -> torch.Tensor:
    """out f32 [B, C] = mean over the rows [r0, r0 + R) of the token stream g f32 [B][T][C] (the first B * T * C elements of g; row pitch
    C).  R = 1 copies row r0 bit for bit.  The summation order depends on R alone."""
    _chk(g, torch.float32, "token_pool g")
    B, T, C, r0, R = int(B), int(T), int(C), int(r0), int(R)
    if B < 1 or T < 1 or g.numel() < B * T * C:
        raise L.GavikoHipError(f"token_pool: g has {g.numel()} elements, [B = {B}, T = {T}, C = {C}] needs {B * T * C}")
    if C < 4 or C % 4 or C > FEATURE_MAX_DIM:
        raise L.GavikoHipError(f"token_pool: C = {C} (a multiple of 4 within [4, {FEATURE_MAX_DIM}])")
    if r0 < 0 or R < 1 or R > T - r0:
        raise L.GavikoHipError(f"token_pool: rows [{r0}, {r0} + {R}) outside the {T} rows of the stream")
    if out is None:
        out = torch.empty((B, C), dtype=torch.float32, device=g.device)
    _chk(out, torch.float32, "token_pool out", B * C)
    L.launch.gvk_token_pool(g, out, B, T, C, r0, R)
    return out


def l2_normalize_rows(x: torch.Tensor, out: torch.Tensor = None, norm: torch.Tensor = None, eps: float = 1e-12) -> torch.Tensor:
    """y[n] = x[n] / max(||x[n]||, eps) for x f32 [N, C]; out=x normalises in place; norm f32 [N] (optional) receives the norms."""
    if not isinstance(x, torch.Tensor):
        raise L.GavikoHipError(f"l2_normalize_rows x: expected a tensor, got {type(x).__name__}")
    _chk(x, torch.float32, "l2_normalize_rows x")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise L.GavikoHipError(f"l2_normalize_rows x: expected [N, C], got {tuple(x.shape)}")
    if not float(eps) > 0.0:
        raise L.GavikoHipError(f"l2_normalize_rows: eps = {eps!r} (must be positive)")
    N, C_ = x.shape
    if out is None:
        out = torch.empty_like(x)
    _chk(out, torch.float32, "l2_normalize_rows out")
    if tuple(out.shape) != tuple(x.shape):
        raise L.GavikoHipError(f"l2_normalize_rows out: expected {tuple(x.shape)}, got {tuple(out.shape)}")
    if out.data_ptr() != x.data_ptr():
        xe, oe = x.data_ptr() + x.numel() * 4, out.data_ptr() + out.numel() * 4
        if not (oe <= x.data_ptr() or xe <= out.data_ptr()):
            raise L.GavikoHipError("l2_normalize_rows: out must be x itself or not overlap it")
    if norm is not None:
        _chk(norm, torch.float32, "l2_normalize_rows norm")
        if norm.numel() != N:
            raise L.GavikoHipError(f"l2_normalize_rows norm: expected {N} entries, got {tuple(norm.shape)}")
    L.launch.gvk_l2_normalize_rows(x, out, norm, N, C_, float(eps))
    return out


def feature_topk(q: torch.Tensor, g: torch.Tensor, k: int, metric: str = "ip", exclude: torch.Tensor = None, slabs: int = None):
    """The k best bank rows of every query -> (idx i32 [Nq, k], score f32 [Nq, k]), best first.  q f32 [Nq, C], g f32 [Ng, C];
    metric 'ip' (score q . g, larger is better) or 'l2' (score = squared distance, smaller is better); an exact tie of the fp32 score goes to
    the lower bank index.  exclude i32 [Nq] (device): one bank index per query that is skipped (-1: none).  slabs: force the number of bank
    slabs (rounded to the nearest valid count, at most 128; None: the default split) -- the result does not depend on it."""
    Nq, C_ = _feat_rows(q, "feature_topk q")
    Ng, _ = _feat_rows(g, "feature_topk g", C_)
    if metric not in TOPK_METRICS:
        raise L.GavikoHipError(f"feature_topk: metric = {metric!r}: expected 'ip' or 'l2'")
    if g.device != q.device:
        raise L.GavikoHipError(f"feature_topk: q on {q.device}, g on {g.device}")
    if Nq * Ng >= 1 << 31:
        raise L.GavikoHipError(f"feature_topk: Nq * Ng = {Nq} * {Ng} exceeds the kernel's 32-bit range (split the queries)")
    if exclude is not None:
        _tab(exclude, "feature_topk exclude", Nq)
    avail = Ng - (1 if exclude is not None else 0)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(TOPK_MAX_K, avail):
        raise L.GavikoHipError(f"feature_topk: k = {k!r} outside [1, min({TOPK_MAX_K}, {avail})] ({Ng} bank rows"
                               + (", one excluded per query)" if exclude is not None else ")"))
    if slabs is not None and (isinstance(slabs, bool) or not isinstance(slabs, int) or slabs < 1):
        raise L.GavikoHipError(f"feature_topk: slabs = {slabs!r}: expected None or a positive int")
    nslabs = L.load().gvk_feature_topk_slabs(Nq, Ng, 0 if slabs is None else slabs)
    words = 2 * Nq * nslabs * k
    scratch = torch.empty(words, dtype=torch.int32, device=q.device)
    idx = torch.empty((Nq, k), dtype=torch.int32, device=q.device)
    score = torch.empty((Nq, k), dtype=torch.float32, device=q.device)
    d = L.FeatureTopkDesc(q=L.ptr(q), g=L.ptr(g), exclude=L.ptr(exclude) if exclude is not None else None, idx=L.ptr(idx), score=L.ptr(score),
                          scratch=L.ptr(scratch), Nq=Nq, Ng=Ng, C=C_, k=k, metric=TOPK_METRICS[metric], nslabs=nslabs, scratch_words=words)
    L.launch.gvk_feature_topk(C.byref(d))
    return idx, score


def knn_vote(idx: torch.Tensor, score: torch.Tensor, labels: torch.Tensor, num_classes: int, weights: str = "uniform", temperature: float = 0.07):
    """Neighbour lists idx i32 / score f32 [Nq, k] (what feature_topk returns; for 'l2' pass -distance) and bank labels i32 [Ng] within
    [0, num_classes) -> (probs f32 [Nq, K], pred i32 [Nq]).  weights 'uniform': votes / k; 'softmax': exp((score_j - score_0) / temperature),
    normalised, summed in rank order.  pred: the lowest class on an exact tie.  The labels' range is the caller's contract."""
    _chk(idx, torch.int32, "knn_vote idx")
    _chk(score, torch.float32, "knn_vote score")
    if idx is None or score is None or idx.dim() != 2 or tuple(idx.shape) != tuple(score.shape) or idx.shape[0] < 1:
        raise L.GavikoHipError(f"knn_vote: expected idx and score [Nq, k], got {None if idx is None else tuple(idx.shape)} and "
                               f"{None if score is None else tuple(score.shape)}")
    Nq, k = idx.shape
    if not 1 <= k <= TOPK_MAX_K:
        raise L.GavikoHipError(f"knn_vote: k = {k} outside [1, {TOPK_MAX_K}]")
    _chk(labels, torch.int32, "knn_vote labels")
    if labels is None or labels.dim() != 1 or labels.numel() < 1:
        raise L.GavikoHipError(f"knn_vote labels: expected i32 [Ng], got {None if labels is None else tuple(labels.shape)}")
    K = num_classes
    if isinstance(K, bool) or not isinstance(K, int) or not 2 <= K <= VOTE_MAX_CLASSES:
        raise L.GavikoHipError(f"knn_vote: num_classes = {K!r} outside [2, {VOTE_MAX_CLASSES}]")
    if weights not in ("uniform", "softmax"):
        raise L.GavikoHipError(f"knn_vote: weights = {weights!r}: expected 'uniform' or 'softmax'")
    if weights == "softmax" and not float(temperature) > 0.0:
        raise L.GavikoHipError(f"knn_vote: temperature = {temperature!r} (must be positive)")
    probs = torch.empty((Nq, K), dtype=torch.float32, device=idx.device)
    pred = torch.empty(Nq, dtype=torch.int32, device=idx.device)
    L.launch.gvk_knn_vote(idx, score, labels, probs, pred, Nq, labels.numel(), k, K, 1 if weights == "softmax" else 0, float(temperature))
    return probs, pred


def class_means(x: torch.Tensor, labels: torch.Tensor, num_classes: int):
    """x f32 [N, C], labels i32 [N] within [0, num_classes) -> (mean f32 [K, C], count i32 [K]); every class summed in row order; an empty
    class gives count 0 and a row of exact zeros.  The labels' range is the caller's contract (rows with other labels join no class)."""
    if not isinstance(x, torch.Tensor):
        raise L.GavikoHipError(f"class_means x: expected a tensor, got {type(x).__name__}")
    _chk(x, torch.float32, "class_means x")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise L.GavikoHipError(f"class_means x: expected [N, C], got {tuple(x.shape)}")
    N, C_ = x.shape
    _tab(labels, "class_means labels", N)
    K = num_classes
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 65535:
        raise L.GavikoHipError(f"class_means: num_classes = {K!r} outside [1, 65535]")
    mean = torch.empty((K, C_), dtype=torch.float32, device=x.device)
    count = torch.empty(K, dtype=torch.int32, device=x.device)
    L.launch.gvk_class_means(x, labels, mean, count, N, C_, K)
    return mean, count


# ---- out-of-distribution statistics (csrc/ood.hip) ----
SCATTER_TILE = 64               # gvk_scatter_matrix: S in 64 x 64 tiles, upper triangle only
SCATTER_CHUNK = 64              # rows per fp32 accumulation chunk (absolute row indices); chunk sums are added in double
SCATTER_TARGET = 512            # workgroups wanted (tile pairs x row slabs)
MAHALANOBIS_MAX_K = 32          # gvk_mahalanobis: centres per call
LOGIT_MAX_CLASSES = 256         # gvk_logit_scores: 4 classes per lane of one wave


def scatter_split(N: int, C: int):
    """-> (npairs, nchunks, chunks per slab, nslabs, scratch bytes) of gvk_scatter_matrix: the rule of include/gaviko_hip.h, a function of
    (N, C) alone."""
    nt = (C + SCATTER_TILE - 1) // SCATTER_TILE
    npairs = nt * (nt + 1) // 2
    nchunks = (N + SCATTER_CHUNK - 1) // SCATTER_CHUNK
    want = min(nchunks, (SCATTER_TARGET + npairs - 1) // npairs)
    cps = (nchunks + want - 1) // want
    nslabs = (nchunks + cps - 1) // cps
    return npairs, nchunks, cps, nslabs, (nslabs * npairs * SCATTER_TILE * SCATTER_TILE + nchunks) * 8


def scatter_matrix(x: torch.Tensor, labels: torch.Tensor, mean: torch.Tensor):
    """x f32 [N, C], labels i32 [N] (None: every row is centred on row 0 of mean), mean f32 [K, C] -> (S f64 [C, C], r4 f64 [1],
    count i32 [K]) with d_i = fl32(x_i - mean[labels_i]):  S = sum_i d_i d_i^T (not divided, S == S.T bit for bit), r4 = sum_i (||d_i||^2)^2,
    count = rows per label.  fp32 products and sums inside chunks of 64 rows, double across chunks, a fixed order: bit-reproducible.  The
    labels' range is the caller's contract (a row with a label outside [0, K) contributes nothing)."""
    N, C_ = _feat_rows(x, "scatter_matrix x")
    K, _ = _feat_rows(mean, "scatter_matrix mean", C_)
    if K > 65535:
        raise L.GavikoHipError(f"scatter_matrix: K = {K} classes outside [1, 65535]")
    if mean.device != x.device:
        raise L.GavikoHipError(f"scatter_matrix: x on {x.device}, mean on {mean.device}")
    if labels is not None:
        _tab(labels, "scatter_matrix labels", N)
    if x.data_ptr() % 16 or mean.data_ptr() % 16:
        raise L.GavikoHipError("scatter_matrix: x and mean must be 16-byte aligned")
    S = torch.empty((C_, C_), dtype=torch.float64, device=x.device)
    r4 = torch.empty(1, dtype=torch.float64, device=x.device)
    count = torch.empty(K, dtype=torch.int32, device=x.device)
    nbytes = scatter_split(N, C_)[4]
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    L.launch.gvk_scatter_matrix(x, labels, mean, S, r4, count, scratch, nbytes, N, C_, K)
    return S, r4, count


def mahalanobis(q: torch.Tensor, whiten: torch.Tensor, centres: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """q f32 [Nq, C], whiten f32 [C, C] (dense W, z = W v), centres f32 [K, C], K <= 32 -> d2 f32 [Nq, K] = ||W q_n - W m_k||^2: both sides
    whitened by the same fp32 MFMA chain, the differences of the whitened coordinates squared and added in fp32 (d2 >= 0, exactly 0 for
    q_n == m_k); a row's result does not depend on Nq."""
    Nq, C_ = _feat_rows(q, "mahalanobis q")
    _feat_rows(whiten, "mahalanobis whiten", C_)
    if whiten.shape[0] != C_:
        raise L.GavikoHipError(f"mahalanobis whiten: expected [{C_}, {C_}], got {tuple(whiten.shape)}")
    K, _ = _feat_rows(centres, "mahalanobis centres", C_)
    if K > MAHALANOBIS_MAX_K:
        raise L.GavikoHipError(f"mahalanobis: K = {K} centres outside [1, {MAHALANOBIS_MAX_K}]")
    if whiten.device != q.device or centres.device != q.device:
        raise L.GavikoHipError(f"mahalanobis: q on {q.device}, whiten on {whiten.device}, centres on {centres.device}")
    if q.data_ptr() % 16 or whiten.data_ptr() % 16 or centres.data_ptr() % 16:
        raise L.GavikoHipError("mahalanobis: q, whiten and centres must be 16-byte aligned")
    if out is None:
        out = torch.empty((Nq, K), dtype=torch.float32, device=q.device)
    _chk(out, torch.float32, "mahalanobis out")
    if tuple(out.shape) != (Nq, K):
        raise L.GavikoHipError(f"mahalanobis out: expected [{Nq}, {K}], got {tuple(out.shape)}")
    L.launch.gvk_mahalanobis(q, whiten, centres, out, Nq, C_, K)
    return out


def logit_scores(logits: torch.Tensor, temperature: float = 1.0) -> torch.Tensor:
    """logits f32 [N, K], 2 <= K <= 256 -> f32 [N, 4]: the largest softmax probability, the largest logit, T logsumexp(z / T) and the
    entropy of softmax(z) in nats; computed in double, shifted by the row maximum, one rounding at the store."""
    if not isinstance(logits, torch.Tensor):
        raise L.GavikoHipError(f"logit_scores logits: expected a tensor, got {type(logits).__name__}")
    _chk(logits, torch.float32, "logit_scores logits")
    if logits.dim() != 2 or logits.shape[0] < 1:
        raise L.GavikoHipError(f"logit_scores logits: expected [N, K], got {tuple(logits.shape)}")
    N, K = logits.shape
    if not 2 <= K <= LOGIT_MAX_CLASSES:
        raise L.GavikoHipError(f"logit_scores: K = {K} classes outside [2, {LOGIT_MAX_CLASSES}]")
    T = float(temperature)
    if not 0.0 < T < float("inf"):
        raise L.GavikoHipError(f"logit_scores: temperature = {temperature!r} (a finite positive number)")
    out = torch.empty((N, 4), dtype=torch.float32, device=logits.device)
    L.launch.gvk_logit_scores(logits, out, N, K, T)
    return out
