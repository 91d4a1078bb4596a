"""Attention maps and attention rollout: what the model attends to.

In the reference every global self-attention runs its probabilities through an `nn.Softmax` module (`Attention.attend`,
vision_transformer.py:50,67), and a forward hook there yields the attention maps.  Here the modules are parameter containers and the
flash kernels never build the probability matrix, so the maps are recomputed from the forward's own buffers: an inference forward in a
workspace of its own keeps every layer's qkv and softmax statistics (Engine.attention_forward; the engine side of this module is
engine_analysis.py), and csrc/attention_map.hip forms the row-weighted sums of P from them, as the backward recomputes P from lse.

    logits, maps = attention_maps(model, img)            # maps[i]: [B, H, T_i], the pooled query's attention in layer i
    logits, rel = attention_rollout(model, img)          # rel: [B, T], sums to 1 per sample
    grid = patch_grid(model, rel)                        # [B, D/pd, H/ph, W/pw]

These three cover the global self-attention on the bf16 path.  The parts that make the model GAViKO -- the MWSA local attention
(gaviko.py:235-238) and the two GPA prompt cross-attentions with their gates (gaviko.py:84-94,164-178) -- have functions of their own, on
BOTH precision paths (the side paths are fp32 either way): the same keep-everything forward leaves every layer's MWSA qkv / lse and GPA
latents, queries, statistics and gates, and csrc/gaviko_maps.hip turns them back into probabilities.

    logits, lmaps = local_attention_maps(model, img, rows="all")  # lmaps[i]: [B, N] = sum_r w_r P_i[b, r, :]; .view(B, *grid) is patch_grid's layout
    logits, gpa = gpa_attention_maps(model, img)                  # gpa[i]: GpaMaps(global_, local, fused [B, P, N]; importance [B, P]; global_weight [B])
    logits, rel = local_rollout(model, img, start=None, layer=None)   # rel: [B, N], sums to sum(start) per sample

gpa[i].fused[b, p, n] is exactly the coefficient with which patch position n enters enhanced prompt p of layer i.  The reference slices the
image tokens twice on the global side (gaviko.py:161,107), so gpa[i].global_ is 0 at the first P + 1 patch positions.  The image footprint of
layer i's prompts through the local path is the composition

    _, gpa = gpa_attention_maps(model, img)
    _, rel = local_rollout(model, img, start=gpa[i].local.mean(1), layer=i)      # rel.view(B, *grid)

The class-specific token-level map is the gradient-weighted attention relevance of Chefer, Gur & Wolf (2021, "Generic Attention-model
Explainability"): with A_l the attention probabilities of layer l and dA_l = d logit[b, target[b]] / d A_l,
Abar_l = mean_h max(0, A_l o dA_l) and R = (I + Abar_{L-1}) ... (I + Abar_0); the relevance is the pooled query's row of R.  In the
reference that is a hook on `attend` with retain_grad(); here dA_l = dO_l . V_l^T is recomputed tile by tile from the dO the input-only
backward sweep produces anyway (Engine.relevance_backward), layer by layer in the order the sweep visits them, so neither a T x T matrix
nor a per-layer copy of dO exists (gvk_attention_gradcolsum_bf16, gvk_relevance_step).

    logits, rel = attention_relevance(model, img, target=None)   # rel: [B, T] >= w_pool, not normalised; patch_grid(model, rel)
    logits, gmaps = attention_gradmaps(model, img)               # gmaps[i]: [B, H, T_i] = sum_r w_r max(0, A_i o dA_i)[b, h, r, :]

Gradient attributions cover every module of every method, on both precision paths: the gradient of a logit with respect to the input
volume, from a deterministic (no-dropout) forward and an input-only backward in a workspace of their own (Engine.input_backward; no
parameter gradient changes), un-patchified by csrc/input_grad.hip with the attribution arithmetic in the same pass.

    logits, g = input_gradient(model, img)                 # g: [B, 1, D, H, W], d logit[b, target[b]] / d img[b]
    logits, g = smoothgrad(model, img, samples=16)         # mean over noisy copies (Smilkov et al., 2017)
    logits, attr, delta = integrated_gradients(model, img) # (Sundararajan et al., 2017); delta: the completeness gap
    grid = patch_saliency(model, g)                        # [B, D/pd, H/ph, W/pw]: sum of |g| per patch (patch_grid's layout)

Which map is faithful, and a map without any backward pass: many inference forwards of one volume in which a chosen set of patches is
replaced by a baseline (csrc/perturb.hip builds the perturbed batch straight in the engine's input slot, Engine.perturbed_forward), for
every method on both precision paths.  Deletion / insertion curves (Petsiuk et al., 2018) rank the patches by a patch-level map
([B, N] or patch_grid / patch_saliency's [B, *grid]) and remove / restore the top k for growing k; occlusion sensitivity (Zeiler & Fergus,
2014) slides a window over the patch grid.

    res = deletion_curve(model, img, grid, target=None, steps=20)      # PerturbationCurve: logits, ks, prob, logit, auc, step_logits
    res = insertion_curve(model, img, grid, target=None, steps=20)     # small deletion auc and large insertion auc = a faithful map
    occ = occlusion_sensitivity(model, img, window=(2, 2, 2))          # OcclusionResult: logits, boxes, drops [B, Wn], map [B, *grid]
    ranks = patch_ranks(model, grid)                                   # [B, N] int32: the order the curves use (ties in patch order)
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple, Union

import torch

from . import lib as L
from . import ops
from ._checks import batch_rows, chunk_tables, volume_check

_ATTENTIONS = ("global",)


def _engine(model, img):
    eng = model._engine()
    if eng.fp32:
        raise L.GavikoHipError("attention maps are built for the bf16 path: the exact-fp32 path (set_precision('fp32')) keeps no "
                               "bf16 qkv / lse for the map kernels")
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise L.GavikoHipError("attention maps run on the HIP device: move the model and the input there (there is no CPU path)")
    return eng


def _pool_range(eng, i: int) -> Tuple[int, int]:
    """Query rows [r0, r0 + R) of layer i that the classification head pools (Engine._pool_rows, at the same indices in every layer;
    pool='mean' of the plain classes averages all T_i rows)."""
    r0, R = eng._pool_rows()
    if eng.pool == "mean" and eng.kind not in ("gaviko", "dvpt"):
        return 0, eng.Ts[i]
    return r0, R


def _forward(eng, img):
    with torch.no_grad():
        return eng.attention_forward(img)


def attention_maps(model, img: torch.Tensor, rows: Union[str, int] = "pool",
                   attention: str = "global") -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """-> (logits [B, K], maps): maps[i] is a float32 [B, H, T_i] device tensor, maps[i][b, h, j] = sum_r w_r P_i[b, h, r, j] with w
    uniform over the selected query rows -- rows='pool': the rows the head pools; an int: that one row of P."""
    if attention not in _ATTENTIONS:
        raise L.GavikoHipError(f"attention={attention!r}: only the global self-attention ('global') is covered -- the MWSA local "
                               "attention and the GPA cross-attention keep no map")
    eng = _engine(model, img)
    if isinstance(rows, bool) or not (rows == "pool" or isinstance(rows, int)):
        raise L.GavikoHipError(f"rows={rows!r}: expected 'pool' or a query row index")
    if isinstance(rows, int) and not 0 <= rows < min(eng.Ts):
        raise L.GavikoHipError(f"rows={rows}: query row outside [0, {min(eng.Ts)}) (the shortest layer's sequence)")
    logits, ws = _forward(eng, img)
    B, H, dev = ws["B"], eng.heads, img.device
    w = torch.zeros((B, eng.T), device=dev)
    maps = []
    for i in range(eng.depth):
        T = eng.Ts[i]
        if rows == "pool":
            r0, R = _pool_range(eng, i)
        else:
            r0, R = rows, 1
        w.zero_()
        w[:, r0:r0 + R] = 1.0 / R
        out = torch.empty((B, H, T), device=dev)
        ops.attention_colsum(ws["qkv"][i], ws["lse"][i], w, out, B, T, H, q0=r0, q1=r0 + R)
        maps.append(out)
    return logits, maps


def attention_rollout(model, img: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (logits [B, K], relevance [B, T] float32, summing to 1 per sample): attention rollout (Abnar & Zuidema, 2020) restricted to
    the pooled query, mean head fusion, residual weight 0.5 --  r = w_pool;  for l = L-1 .. 0:  r <- 0.5 r + 0.5 mean_h(r^T P_l[h])."""
    eng = model._engine()
    if eng.kind == "vpt" and eng.deep:
        raise L.GavikoHipError("attention rollout needs one token sequence through all layers; deep VPT rebuilds it before every layer "
                               "(vpt.py:147-153) -- use attention_maps")
    _engine(model, img)
    logits, ws = _forward(eng, img)
    B, H, T, dev = ws["B"], eng.heads, eng.T, img.device
    r0, R = _pool_range(eng, eng.depth - 1)
    r = torch.zeros((B, T), device=dev)
    r[:, r0:r0 + R] = 1.0 / R
    cs = torch.empty((B, H, T), device=dev)
    q0, q1 = r0, r0 + R                            # the first step reads the pooled rows only; r is dense from then on
    for l in range(eng.depth - 1, -1, -1):
        ops.attention_colsum(ws["qkv"][l], ws["lse"][l], r, cs, B, T, H, q0=q0, q1=q1)
        ops.rollout_step(r, cs, r, B, T, H)
        q0, q1 = 0, T
    return logits, r


def _relevance_checks(model, img, target, what):
    """Everything attention_relevance / attention_gradmaps reject, before any launch -> (engine, contiguous volume, seed)."""
    eng = model._engine()
    if eng.fp32:
        raise L.GavikoHipError(f"{what} is built for the bf16 path: the exact-fp32 path (set_precision('fp32')) keeps no bf16 qkv / lse / "
                               "dctx for the map kernels")
    want = (1,) + tuple(g * p for g, p in zip(eng.grid, eng.patch))
    if not isinstance(img, torch.Tensor) or img.dim() != 5 or tuple(img.shape[1:]) != want or img.shape[0] < 1:
        raise L.GavikoHipError(f"{what}: expected img [B, {', '.join(map(str, want))}], got {tuple(getattr(img, 'shape', ()))}")
    if img.dtype != torch.float32:
        raise L.GavikoHipError(f"{what}: expected a float32 volume, got {img.dtype}")
    B = img.shape[0]
    if target is not None:
        _targets(eng, torch.zeros((B, eng.K)), target, B)            # a bad target is rejected here (host tensors only)
    eng, x = volume_check(model, img, what)                         # (and the device)

    def seed(logits):
        return torch.nn.functional.one_hot(_targets(eng, logits, target, B), eng.K).to(logits.dtype)

    return eng, x, seed


def attention_relevance(model, img: torch.Tensor, target=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (logits [B, K], relevance [B, T] float32): the gradient-weighted attention relevance of the logit target[b] (None: the argmax
    per sample, an int, or a [B] tensor) --  r = w_pool;  for l = L-1 .. 0:  r <- r + r^T mean_h max(0, A_l o dA_l).  Not normalised;
    r >= w_pool elementwise (the identity term), so the class-specific part is r - w_pool."""
    eng = model._engine()
    if eng.kind == "vpt" and eng.deep:
        raise L.GavikoHipError("attention relevance needs one token sequence through all layers; deep VPT rebuilds it before every layer "
                               "(vpt.py:147-153) -- use attention_gradmaps")
    eng, x, seed = _relevance_checks(model, img, target, "attention_relevance")
    with torch.no_grad():
        logits, _, rv = eng.relevance_backward(x, seed, mode="relevance")
        return logits, rv["r"].clone()


def attention_gradmaps(model, img: torch.Tensor, target=None, rows: Union[str, int] = "pool") -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """-> (logits [B, K], maps): maps[i] is a float32 [B, H, T_i] device tensor, maps[i][b, h, j] = sum_r w_r max(0, A_i o dA_i)[b, h, r, j]
    with w uniform over the selected query rows (attention_maps' `rows`) and dA_i the gradient of the logit target[b] with respect to the
    probabilities of layer i: per head, not propagated -- the class-specific counterpart of attention_maps."""
    eng = model._engine()
    if isinstance(rows, bool) or not (rows == "pool" or isinstance(rows, int)):
        raise L.GavikoHipError(f"rows={rows!r}: expected 'pool' or a query row index")
    if isinstance(rows, int) and not 0 <= rows < min(eng.Ts):
        raise L.GavikoHipError(f"rows={rows}: query row outside [0, {min(eng.Ts)}) (the shortest layer's sequence)")
    eng, x, seed = _relevance_checks(model, img, target, "attention_gradmaps")
    with torch.no_grad():
        logits, _, rv = eng.relevance_backward(x, seed, mode="maps", rows=rows)
        return logits, [m.clone() for m in rv["maps"]]


def patch_grid(model, relevance: torch.Tensor) -> torch.Tensor:
    """[..., T] relevance (or a map of a layer whose sequence is the embedding's) -> [..., D/pd, H/ph, W/pw]: the patch rows (at the
    method's own row offset) in patch-grid order.  Upsampling to the volume is torch.nn.functional.interpolate's job."""
    eng = model._engine()
    if relevance.shape[-1] != eng.T:
        raise L.GavikoHipError(f"patch_grid: expected a last dimension of T = {eng.T} tokens, got {tuple(relevance.shape)}")
    patches = relevance[..., eng.row_off: eng.row_off + eng.N]
    return patches.reshape(*relevance.shape[:-1], *eng.grid)


# ---- gradient attributions ----------------------------------------------------------------------------------------------------
def _targets(eng, logits, target, B) -> torch.Tensor:
    """int64 [B] device tensor of the logit to explain per sample: None -> the argmax of `logits`, an int, or a [B] tensor."""
    dev = logits.device
    if target is None:
        return logits.argmax(dim=1)
    if isinstance(target, bool):
        raise L.GavikoHipError(f"target={target!r}: expected None, an int or a [B] tensor")
    if isinstance(target, int):
        if not 0 <= target < eng.K:
            raise L.GavikoHipError(f"target={target}: outside [0, {eng.K})")
        return torch.full((B,), target, dtype=torch.int64, device=dev)
    if isinstance(target, torch.Tensor):
        t = target.reshape(-1)
        if t.numel() != B or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise L.GavikoHipError(f"target: expected an integer tensor of {B} elements, got {tuple(target.shape)} {target.dtype}")
        t = t.to(device=dev, dtype=torch.int64)
        if bool(((t < 0) | (t >= eng.K)).any()):
            raise L.GavikoHipError(f"target: a class index outside [0, {eng.K})")
        return t
    raise L.GavikoHipError(f"target={target!r}: expected None, an int or a [B] tensor")


def _onehot(tgt, K):
    return lambda logits: torch.nn.functional.one_hot(tgt, K).to(logits.dtype)


def _accumulate(eng, rows, tgt_rows, out, S, alpha, x=None, x0=None, batch=1):
    """out[b] = sum_s alpha * g(rows[b*S + s]) (* (x[b] - x0[b])): the input gradients of the logit tgt_rows[r] at every row r, in engine
    batches of `batch` rows; each output sample's rows are summed in s order by gvk_unpatchify_f32 (one FMA per step), so the result does
    not depend on how the rows are split into batches beyond the per-row gradients themselves."""
    n = rows.shape[0]
    for c0 in range(0, n, batch):
        c1 = min(n, c0 + batch)
        _, ws = eng.input_backward(rows[c0:c1], _onehot(tgt_rows[c0:c1], eng.K))
        dcols = ws["ig"]["dcols"]
        r = c0
        while r < c1:                                   # the runs of one output sample inside this batch
            b, s = divmod(r, S)
            e = min(c1, (b + 1) * S)
            ops.unpatchify(dcols[(r - c0) * eng.N:], out[b:b + 1], eng.patch, x=None if x is None else x[b:b + 1],
                           x0=None if x0 is None else x0[b:b + 1], alpha=alpha, beta=0.0 if s == 0 else 1.0, nsum=e - r)
            r = e


def input_gradient(model, img: torch.Tensor, target=None, *, times_input: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (logits [B, K], grad [B, 1, D, H, W] float32): d logit[b, target[b]] / d img[b] (times img with times_input: gradient x input).
    target: None (the argmax per sample), an int, or a [B] tensor of class indices."""
    eng, x = volume_check(model, img, "input_gradient")
    B = x.shape[0]
    box = {}

    def seed(logits):
        box["t"] = _targets(eng, logits, target, B)
        return torch.nn.functional.one_hot(box["t"], eng.K).to(logits.dtype)

    if isinstance(target, (int, torch.Tensor)) and not isinstance(target, bool):
        _targets(eng, torch.zeros((B, eng.K), device=x.device), target, B)       # reject a bad target before any launch
    logits, ws = eng.input_backward(x, seed)
    out = torch.empty_like(x)
    ops.unpatchify(ws["ig"]["dcols"], out, eng.patch, x=x if times_input else None)
    return logits, out


def smoothgrad(model, img: torch.Tensor, target=None, *, samples: int = 16, sigma: float = 0.15, generator=None,
               batch: int = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (logits [B, K] of the clean input, grad [B, 1, D, H, W]): the mean input gradient over `samples` noisy copies x + N(0, s^2) per
    volume, s = sigma * (max - min) of that volume.  target None: the clean input's argmax.  batch: engine rows per sweep (default B)."""
    eng, x = volume_check(model, img, "smoothgrad")
    B = x.shape[0]
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
        raise L.GavikoHipError(f"samples={samples!r}: expected a positive int")
    if not sigma >= 0:
        raise L.GavikoHipError(f"sigma={sigma!r}: expected >= 0")
    if isinstance(target, (int, torch.Tensor)) and not isinstance(target, bool):
        _targets(eng, torch.zeros((B, eng.K), device=x.device), target, B)
    bs = batch_rows(batch, B)
    with torch.no_grad():
        logits = eng.eval_forward(x)
        tgt = _targets(eng, logits, target, B)
        rows = x.repeat_interleave(samples, dim=0)
        if sigma > 0:
            flat = x.reshape(B, -1)
            scale = (sigma * (flat.amax(1) - flat.amin(1))).repeat_interleave(samples).view(-1, 1, 1, 1, 1)
            noise = torch.randn(rows.shape, generator=generator, device=x.device if generator is None else generator.device)
            rows = rows + noise.to(x.device) * scale
        out = torch.empty_like(x)
        _accumulate(eng, rows.contiguous(), tgt.repeat_interleave(samples), out, samples, 1.0 / samples, batch=bs)
    return logits, out


def integrated_gradients(model, img: torch.Tensor, target=None, *, baseline: torch.Tensor = None, steps: int = 32,
                         batch: int = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (logits [B, K], attributions [B, 1, D, H, W], delta [B]): (x - x0) * mean_k grad(x0 + a_k (x - x0)), a_k = (k + 1/2) / steps
    (the midpoint rule), and the completeness gap delta = sum(attr) - (f(x) - f(x0)) of the explained logit (float64).  baseline: None
    (zeros) or a volume of img's shape.  batch: engine rows per sweep (default B)."""
    eng, x = volume_check(model, img, "integrated_gradients")
    B = x.shape[0]
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise L.GavikoHipError(f"steps={steps!r}: expected a positive int")
    if baseline is None:
        x0 = torch.zeros_like(x)
    else:
        _, x0 = volume_check(model, baseline if baseline.dim() == 5 else baseline[None], "integrated_gradients baseline")
        x0 = x0.expand_as(x).contiguous()
    if isinstance(target, (int, torch.Tensor)) and not isinstance(target, bool):
        _targets(eng, torch.zeros((B, eng.K), device=x.device), target, B)
    bs = batch_rows(batch, B)
    with torch.no_grad():
        logits = eng.eval_forward(x)
        f0 = eng.eval_forward(x0)
        tgt = _targets(eng, logits, target, B)
        a = (torch.arange(steps, device=x.device, dtype=torch.float32) + 0.5) / steps
        rows = x0.repeat_interleave(steps, dim=0) + a.repeat(B).view(-1, 1, 1, 1, 1) * (x - x0).repeat_interleave(steps, dim=0)
        out = torch.empty_like(x)
        _accumulate(eng, rows.contiguous(), tgt.repeat_interleave(steps), out, steps, 1.0 / steps, x=x, x0=x0, batch=bs)
        grid = torch.empty((B,) + tuple(eng.grid), device=x.device)
        ops.patch_reduce(out, grid, eng.patch, absval=False)
        idx = torch.arange(B, device=x.device)
        delta = grid.double().reshape(B, -1).sum(1) - (logits[idx, tgt].double() - f0[idx, tgt].double())
    return logits, out, delta


def patch_saliency(model, volume_map: torch.Tensor, reduce: str = "abs") -> torch.Tensor:
    """[B, 1, D, H, W] volume map (a gradient, an attribution) -> [B, D/pd, H/ph, W/pw]: per patch the sum of |map| (reduce='abs') or of
    the map (reduce='sum'), in the layout of patch_grid."""
    if reduce not in ("abs", "sum"):
        raise L.GavikoHipError(f"reduce={reduce!r}: expected 'abs' or 'sum'")
    eng, v = volume_check(model, volume_map, "patch_saliency")
    out = torch.empty((v.shape[0],) + tuple(eng.grid), device=v.device)
    ops.patch_reduce(v, out, eng.patch, absval=reduce == "abs")
    return out


# ---- GAViKO's own attentions: MWSA local attention and GPA prompt cross-attention ------------------------------------------------
class GpaMaps(NamedTuple):
    """One GPA layer: the prompts' cross-attention over the patch positions through the global and the local path, their gated fusion
    fused = importance * (global_weight * global_ + (1 - global_weight) * local)  [B, P, N], and the two gates as the forward kept them."""
    global_: torch.Tensor
    local: torch.Tensor
    fused: torch.Tensor
    importance: torch.Tensor
    global_weight: torch.Tensor


def _gaviko_forward(model, img, what):
    """Everything the three functions below reject, then one deterministic keep-everything forward -> (engine, logits, workspace)."""
    eng = model._engine()
    if eng.kind != "gaviko":
        raise L.GavikoHipError(f"{what}: the MWSA local attention and the GPA prompt attention exist in GAViKO models only (this engine "
                               f"is {eng.kind!r})")
    eng, x = volume_check(model, img, what)
    logits, ws = _forward(eng, x)
    return eng, logits.detach(), ws


def _window_colsum(eng, ws, i, w, out):
    m = ws["mw"][i]
    ops.window_attn_colsum(m["qkv"], m["lse"], w, out, ws["B"], eng.grid[0], eng.grid[1], eng.grid[2], eng.win[0], eng.win[1], eng.win[2],
                           eng.Lat, eng.C ** -0.5)


def local_attention_maps(model, img: torch.Tensor, rows: Union[str, int, torch.Tensor] = "all") -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """-> (logits [B, K], maps): maps[i] is a float32 [B, N] device tensor, maps[i][b, j] = sum_r w[b, r] P_i[b, r, j] with P_i the
    masked-window attention probabilities of layer i (gaviko.py:235-238) -- rows='all': w = 1 / N (how much attention each patch
    RECEIVES); an int: that query's window (zeros outside it); a float32 device tensor [B, N]: those weights."""
    eng = model._engine()
    N = getattr(eng, "N", 0)
    if isinstance(rows, bool) or not (isinstance(rows, (int, torch.Tensor)) or rows == "all"):
        raise L.GavikoHipError(f"rows={rows!r}: expected 'all', a query row index or a float32 [B, N] weight tensor")
    if isinstance(rows, int) and eng.kind == "gaviko" and not 0 <= rows < N:
        raise L.GavikoHipError(f"rows={rows}: query row outside [0, {N})")
    eng, logits, ws = _gaviko_forward(model, img, "local_attention_maps")
    B, dev = ws["B"], img.device
    if isinstance(rows, torch.Tensor):
        if tuple(rows.shape) != (B, N) or rows.dtype != torch.float32 or not rows.is_cuda:
            raise L.GavikoHipError(f"rows: expected a float32 device tensor [{B}, {N}], got {tuple(rows.shape)} {rows.dtype} on {rows.device}")
        w = rows.detach().contiguous()
    elif rows == "all":
        w = torch.full((B, N), 1.0 / N, device=dev)
    else:
        w = torch.zeros((B, N), device=dev)
        w[:, rows] = 1.0
    maps = []
    for i in range(eng.depth):
        out = torch.empty((B, N), device=dev)
        _window_colsum(eng, ws, i, w, out)
        maps.append(out)
    return logits, maps


def gpa_attention_maps(model, img: torch.Tensor) -> Tuple[torch.Tensor, List[GpaMaps]]:
    """-> (logits [B, K], one GpaMaps per LAYER (shared modules do not share activations)): float32 device tensors of their own."""
    eng, logits, ws = _gaviko_forward(model, img, "gpa_attention_maps")
    B, P, N, dev = ws["B"], eng.P, eng.N, img.device
    res = []
    for i in range(eng.depth):
        g = ws["gp"][i]
        pg, pl, fu = (torch.empty((B, P, N), device=dev) for _ in range(3))
        ops.gpa_attn_maps(g["xl"], g["ll"], g["qg"], g["ql"], g["lse_g"], g["lse_l"], g["imp"], g["gw"], B, eng.T, N, P, eng.Lat,
                          global_=pg, local=pl, fused=fu)
        res.append(GpaMaps(pg, pl, fu, g["imp"].clone(), g["gw"].clone()))
    return logits, res


def local_rollout(model, img: torch.Tensor, start: Optional[torch.Tensor] = None, layer: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (logits [B, K], relevance [B, N] float32, summing to sum(start) per sample): attention rollout on the single-head local stream
    (gaviko.py:301) with attention_rollout's residual convention --  r = start (None: 1 / N) at the output of layer `layer` (None: the
    last);  for l = layer .. 0:  r <- 0.5 r + 0.5 r^T P_l."""
    eng = model._engine()
    depth = eng.depth
    if layer is not None and (isinstance(layer, bool) or not isinstance(layer, int) or not 0 <= layer < depth):
        raise L.GavikoHipError(f"layer={layer!r}: expected None or a layer index in [0, {depth})")
    if start is not None and not isinstance(start, torch.Tensor):
        raise L.GavikoHipError(f"start={start!r}: expected None or a float32 device tensor [B, N]")
    eng, logits, ws = _gaviko_forward(model, img, "local_rollout")
    B, N, dev = ws["B"], eng.N, img.device
    if start is None:
        r = torch.full((B, N), 1.0 / N, device=dev)
    else:
        if tuple(start.shape) != (B, N) or start.dtype != torch.float32 or not start.is_cuda:
            raise L.GavikoHipError(f"start: expected a float32 device tensor [{B}, {N}], got {tuple(start.shape)} {start.dtype} on {start.device}")
        r = start.detach().clone().contiguous()
    cs = torch.empty((B, N), device=dev)
    for l in range(depth - 1 if layer is None else layer, -1, -1):
        _window_colsum(eng, ws, l, r, cs)
        ops.rollout_step(r, cs, r, B, N, 1)                   # the single head: mean head fusion over H = 1
    return logits, r


# ---- gradient-free attribution and the faithfulness of a map: occlusion sensitivity, deletion / insertion curves -----------------
class PerturbationCurve(NamedTuple):
    """deletion_curve / insertion_curve: logits [B, K] of the unperturbed volume; ks [S + 1] int64, the number of patches removed
    (restored) at every step; prob / logit [B, S + 1] of the explained class; auc [B], the trapezoid area of prob over k / N; step_logits
    [B, S + 1, K]."""
    logits: torch.Tensor
    ks: torch.Tensor
    prob: torch.Tensor
    logit: torch.Tensor
    auc: torch.Tensor
    step_logits: torch.Tensor


class OcclusionResult(NamedTuple):
    """occlusion_sensitivity: logits [B, K] of the unperturbed volume; boxes [Wn, 6] int64 (d0, d1, h0, h1, w0, w1 in patch-grid units);
    drops [B, Wn] = prob(x)[target] - prob(x with window w replaced)[target]; map [B, *grid], the mean drop of the windows covering a patch."""
    logits: torch.Tensor
    boxes: torch.Tensor
    drops: torch.Tensor
    map: torch.Tensor


def _relevance_rows(eng, relevance, B, what) -> torch.Tensor:
    """A patch-level map in one of the two layouts the package produces -- [B, N] or [B, *grid] (patch_grid / patch_saliency) -> float32
    [B, N], NaN rejected (one device check, before any step of a sweep)."""
    if not isinstance(relevance, torch.Tensor) or not relevance.is_cuda:
        raise L.GavikoHipError(f"{what}: the relevance map must be a tensor on the HIP device (there is no CPU path)")
    shape = tuple(relevance.shape)
    if shape not in ((B, eng.N), (B,) + tuple(eng.grid)) or not relevance.dtype.is_floating_point:
        raise L.GavikoHipError(f"{what}: expected a floating-point patch-level map [{B}, {eng.N}] or [{B}, {', '.join(map(str, eng.grid))}], got "
                               f"{shape} {relevance.dtype} -- token-level maps [B, T] go through patch_grid first, voxel maps through patch_saliency")
    rel = relevance.detach().reshape(B, eng.N).to(torch.float32).contiguous()
    if bool(torch.isnan(rel).any()):
        raise L.GavikoHipError(f"{what}: the relevance map holds NaN, which has no place in an order")
    return rel


def patch_ranks(model, relevance: torch.Tensor) -> torch.Tensor:
    """relevance [B, N] or [B, *grid] (the layout of patch_grid / patch_saliency) -> ranks [B, N] int32: ranks[b, n] is the position of
    patch n when the patches of sample b are sorted by descending relevance, ties in patch order -- the inverse permutation of
    torch.argsort(relevance, descending=True, stable=True)."""
    eng = model._engine()
    if not isinstance(relevance, torch.Tensor) or relevance.dim() < 1:
        raise L.GavikoHipError("patch_ranks: the relevance map must be a tensor on the HIP device (there is no CPU path)")
    return ops.patch_rank(_relevance_rows(eng, relevance, relevance.shape[0], "patch_ranks"))


def _baseline(eng, x, baseline, what):
    """-> (fill_scalar f32 [B] or None, base [1 or B,1,D,H,W] or None): 'min' (the per-sample minimum of the volume: what RescaleIntensity
    maps to 0 and RandomAffine pads with), a float, or a baseline volume."""
    B = x.shape[0]
    if isinstance(baseline, str):
        if baseline != "min":
            raise L.GavikoHipError(f"{what}: baseline={baseline!r}: expected 'min', a float or a volume [1 or B, 1, D, H, W]")
        V = x.numel() // B
        if V % 4:                                            # gvk_volume_minmax reads 16-byte words
            return x.reshape(B, V).amin(1).contiguous(), None
        part = ops.minmax_partials(B, x.device)
        ops.volume_minmax(x, part)
        return part.view(B, -1, 2)[:, :, 0].amin(1).contiguous(), None
    if isinstance(baseline, (int, float)) and not isinstance(baseline, bool):
        return torch.full((B,), float(baseline), dtype=torch.float32, device=x.device), None
    if isinstance(baseline, torch.Tensor):
        if not baseline.is_cuda:
            raise L.GavikoHipError(f"{what}: the baseline volume must be on the HIP device (there is no CPU path)")
        if baseline.dim() != 5 or tuple(baseline.shape[1:]) != tuple(x.shape[1:]) or baseline.shape[0] not in (1, B) or baseline.dtype != torch.float32:
            raise L.GavikoHipError(f"{what}: expected a float32 baseline volume [1 or {B}, {', '.join(map(str, x.shape[1:]))}], got "
                                   f"{tuple(baseline.shape)} {baseline.dtype}")
        return None, baseline.detach().contiguous()
    raise L.GavikoHipError(f"{what}: baseline={baseline!r}: expected 'min', a float or a volume [1 or B, 1, D, H, W]")


def _sweep(eng, x, target, bs, fill, base, jobs, *, rank=None):
    """The perturbed forwards of one call, in engine chunks of `bs` samples.  jobs[i] = (b, spec) asks for volume b with the patches of
    `spec` replaced: (lo, hi) = the patches of rank lo <= r < hi (with `rank`), or a box (d0, d1, h0, h1, w0, w1) in patch-grid units.
    -> (logits [B, K] of the unperturbed volumes, rows [len(jobs), K] in the order of `jobs`, prob [B + len(jobs)], logit [B + len(jobs)]:
    the B unperturbed volumes first).

    The B unperturbed volumes run first through the same chunks (an empty mask), so one workspace and one launch plan serve the whole
    call, and a job whose mask is empty (deletion at k = 0, insertion at k = N) is not run again: its row is a copy of volume b's.  The
    last chunk is padded with repeats that write nowhere.  Example, B = 2, a deletion curve with ks = [0, 500, 1000], bs = 3:
        result rows   0 1 | 2    3      4      5    6      7        (rows 0, 1: the plain volumes; 2.. : jobs in their order)
        jobs               (0,k0)(1,k0)(0,k500)(1,k500)(0,k1000)(1,k1000)
        run           src  0 1 0 | 1 0 1          (plain 0, plain 1, the four non-empty jobs)
                      slot 0 1 4 | 5 6 7          (the result row each forward's logits are gathered into; -1 for padding)
        copies        rows 2, 3 <- rows 0, 1      (the two k = 0 jobs)
    The tables go to the device once; every chunk gathers its logits rows on the device and one launch at the end scores all result
    rows (src_of_row[r] = the volume of row r picks the target), so nothing between the first and the last forward waits for the host."""
    B, K, dev = x.shape[0], eng.K, x.device
    ranked = rank is not None
    empty = (lambda sp: sp[0] >= sp[1]) if ranked else (lambda sp: sp[0] >= sp[1] or sp[2] >= sp[3] or sp[4] >= sp[5])
    blank = (0, 0) if ranked else (0, 0, 0, 0, 0, 0)
    n = B + len(jobs)                                        # result rows
    src_of_row = list(range(B)) + [b for b, _ in jobs]
    run = [(b, blank, b) for b in range(B)] + [(b, sp, B + i) for i, (b, sp) in enumerate(jobs) if not empty(sp)]   # (volume, spec, result row)
    reuse = [(B + i, b) for i, (b, sp) in enumerate(jobs) if empty(sp)]                                              # (result row, plain row)
    src, spec, slot = chunk_tables(bs, dev, [r[0] for r in run], [r[1] for r in run], slot=[r[2] for r in run])
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)       # noqa: E731
    src_row, row_id = i32(src_of_row), i32(list(range(n)))
    rows = torch.empty((n, K), device=dev)
    with torch.no_grad():
        for c in range(0, slot.numel(), bs):
            s = slice(c, c + bs)
            mask = dict(rank=rank, lo=spec[s, 0].contiguous(), hi=spec[s, 1].contiguous()) if ranked else dict(boxes=spec[s])
            eng.perturbed_forward(x, src[s], fill_scalar=fill, base=base, slot=slot[s], rows=rows, **mask)
        if reuse:
            rows[torch.tensor([r for r, _ in reuse]).to(dev)] = rows[torch.tensor([b for _, b in reuse]).to(dev)]
        logits = rows[:B].clone()
        tgt = target if target is not None else logits.argmax(dim=1)
        prob, logit = torch.empty(n, device=dev), torch.empty(n, device=dev)
        ops.perturb_scores(rows, src_row, tgt.to(torch.int32), row_id, prob, logit)
    return logits, rows[B:], prob, logit


def _perturb_checks(model, img, target, baseline, batch, what):
    eng, x = volume_check(model, img, what)
    B = x.shape[0]
    bs = batch_rows(batch, 8)
    tgt = None
    if target is not None:                                   # validated (and resolved) before any launch
        tgt = _targets(eng, torch.zeros((B, eng.K), device=x.device), target, B)
    fill, base = _baseline(eng, x, baseline, what)
    return eng, x, B, bs, tgt, fill, base


def _curve(model, img, relevance, target, steps, ks, baseline, batch, insertion, what) -> PerturbationCurve:
    eng, x, B, bs, tgt, fill, base = _perturb_checks(model, img, target, baseline, batch, what)
    N = eng.N
    if ks is None:
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise L.GavikoHipError(f"steps={steps!r}: expected a positive int")
        ks = [(s * N) // steps for s in range(steps + 1)]
    else:
        ks = [int(k) for k in (ks.tolist() if isinstance(ks, torch.Tensor) else ks)]
        if not ks or any(not 0 <= k <= N for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
            raise L.GavikoHipError(f"ks={ks!r}: expected an increasing list of patch counts within [0, {N}]")
    rank = ops.patch_rank(_relevance_rows(eng, relevance, B, what))
    P = len(ks)
    # step-major: a chunk holds the same step of consecutive samples (with batch == B, exactly the samples of img in their order)
    jobs = [(b, (k, N) if insertion else (0, k)) for k in ks for b in range(B)]
    logits, rows, prob, logit = _sweep(eng, x, tgt, bs, fill, base, jobs, rank=rank)
    by_sample = lambda t: t.view(P, B, *t.shape[1:]).transpose(0, 1).contiguous()       # noqa: E731  [P * B, ...] step-major -> [B, P, ...]
    prob, logit = by_sample(prob[B:]), by_sample(logit[B:])
    ks_dev = torch.tensor(ks, dtype=torch.int32).to(x.device)
    auc = ops.curve_auc(prob, ks_dev, N)
    return PerturbationCurve(logits, torch.tensor(ks, dtype=torch.int64), prob, logit, auc, by_sample(rows))


def deletion_curve(model, img: torch.Tensor, relevance: torch.Tensor, target=None, *, steps: int = 20, ks=None, baseline="min",
                   batch: int = 8) -> PerturbationCurve:
    """Deletion curve (Petsiuk et al., 2018): the patches of every volume are ranked by `relevance` ([B, N] or [B, *grid]: patch_grid /
    patch_saliency layout; ties in patch order) and the top k are replaced by the baseline for growing k; a faithful map makes the class
    probability fall fast, i.e. a SMALL auc.  k_s = (s N) // steps for s = 0 .. steps (k_0 = 0: the unperturbed volume), or an explicit
    increasing list `ks` within [0, N].  target: None (the argmax of the unperturbed logits per sample), an int or a [B] tensor.
    baseline: 'min' (the per-sample minimum of the volume), a float, or a float32 volume [1 or B, 1, D, H, W] (e.g. a blurred copy).
    batch: perturbed volumes per engine forward.  Runs on every method and both precision paths; the forward is the deterministic one."""
    return _curve(model, img, relevance, target, steps, ks, baseline, batch, False, "deletion_curve")


def insertion_curve(model, img: torch.Tensor, relevance: torch.Tensor, target=None, *, steps: int = 20, ks=None, baseline="min",
                    batch: int = 8) -> PerturbationCurve:
    """Insertion curve: deletion_curve's counterpart that starts from the pure baseline (k_0 = 0) and restores the top-k patches; a faithful
    map makes the class probability rise fast, i.e. a LARGE auc.  Arguments as for deletion_curve."""
    return _curve(model, img, relevance, target, steps, ks, baseline, batch, True, "insertion_curve")


def _triple(v, name):
    if isinstance(v, int) and not isinstance(v, bool):
        v = (v, v, v)
    if not isinstance(v, (tuple, list)) or len(v) != 3 or any(isinstance(a, bool) or not isinstance(a, int) or a < 1 for a in v):
        raise L.GavikoHipError(f"{name}={v!r}: expected three positive ints (patch-grid units)")
    return tuple(v)


def occlusion_sensitivity(model, img: torch.Tensor, target=None, *, window=(2, 2, 2), stride=None, baseline="min",
                          batch: int = 8) -> OcclusionResult:
    """Occlusion sensitivity (Zeiler & Fergus, 2014) at patch granularity: a window of `window` patches slides over the patch grid in steps
    of `stride` (None: the window itself, disjoint windows; windows are clipped to the grid), the patches under it are replaced by the
    baseline, and the drop of the class probability is recorded.  map[b, patch] is the mean drop over the windows that cover the patch
    (every patch must be covered).  target / baseline / batch as for deletion_curve.  No backward pass is involved."""
    eng, x, B, bs, tgt, fill, base = _perturb_checks(model, img, target, baseline, batch, "occlusion_sensitivity")
    win = _triple(window, "window")
    st = win if stride is None else _triple(stride, "stride")
    grid = tuple(eng.grid)
    axes = [[(p, min(p + w, g)) for p in range(0, g, s)] for g, w, s in zip(grid, win, st)]
    wins = [d + h + w for d in axes[0] for h in axes[1] for w in axes[2]]
    cover = torch.zeros((len(wins),) + grid)
    for i, (d0, d1, h0, h1, w0, w1) in enumerate(wins):
        cover[i, d0:d1, h0:h1, w0:w1] = 1.0
    if bool((cover.sum(0) == 0).any()):
        raise L.GavikoHipError(f"occlusion_sensitivity: window={win} with stride={st} leaves patches of the {grid} grid uncovered")
    Wn = len(wins)
    jobs = [(b, w) for w in wins for b in range(B)]                  # window-major, like the steps of a curve
    logits, _, prob, _ = _sweep(eng, x, tgt, bs, fill, base, jobs)
    drops = prob[:B, None] - prob[B:].view(Wn, B).t()
    cover = cover.view(Wn, eng.N).to(x.device)
    amap = (drops[:, :, None] * cover[None]).sum(1) / cover.sum(0)
    return OcclusionResult(logits, torch.tensor(wins, dtype=torch.int64), drops, amap.view((B,) + grid))
