"""Attention maps and attention rollout: what the model attends to.

In the reference every global self-attention runs its probabilities through an `nn.Softmax` module (`Attention.attend`,
vision_transformer.py:50,67), and a forward hook there yields the attention maps.  Here the modules are parameter containers and the
flash kernels never build the probability matrix, so the maps are recomputed from the forward's own buffers: an inference forward in a
workspace of its own keeps every layer's qkv and softmax statistics (Engine.attention_forward), and csrc/attention_map.hip forms the
row-weighted sums of P from them, as the backward recomputes P from lse.

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
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple, Union

import torch

from . import lib as L
from . import ops

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
    eng, x = _volume_check(model, img, what)                         # (and the device)

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
def _volume_check(model, img, what):
    eng = model._engine()
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise L.GavikoHipError(f"{what} runs on the HIP device: move the model and the input there (there is no CPU path)")
    want = (1,) + tuple(g * p for g, p in zip(eng.grid, eng.patch))
    if img.dim() != 5 or tuple(img.shape[1:]) != want or img.shape[0] < 1:
        raise L.GavikoHipError(f"{what}: expected img [B, {', '.join(map(str, want))}], got {tuple(img.shape)}")
    if img.dtype != torch.float32:
        raise L.GavikoHipError(f"{what}: expected a float32 volume, got {img.dtype}")
    return eng, img.detach().contiguous()


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


def _batch(batch, default):
    if batch is None:
        return default
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise L.GavikoHipError(f"batch={batch!r}: expected a positive int")
    return batch


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
    eng, x = _volume_check(model, img, "input_gradient")
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
    eng, x = _volume_check(model, img, "smoothgrad")
    B = x.shape[0]
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
        raise L.GavikoHipError(f"samples={samples!r}: expected a positive int")
    if not sigma >= 0:
        raise L.GavikoHipError(f"sigma={sigma!r}: expected >= 0")
    if isinstance(target, (int, torch.Tensor)) and not isinstance(target, bool):
        _targets(eng, torch.zeros((B, eng.K), device=x.device), target, B)
    bs = _batch(batch, B)
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
    eng, x = _volume_check(model, img, "integrated_gradients")
    B = x.shape[0]
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise L.GavikoHipError(f"steps={steps!r}: expected a positive int")
    if baseline is None:
        x0 = torch.zeros_like(x)
    else:
        _, x0 = _volume_check(model, baseline if baseline.dim() == 5 else baseline[None], "integrated_gradients baseline")
        x0 = x0.expand_as(x).contiguous()
    if isinstance(target, (int, torch.Tensor)) and not isinstance(target, bool):
        _targets(eng, torch.zeros((B, eng.K), device=x.device), target, B)
    bs = _batch(batch, B)
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
    eng, v = _volume_check(model, volume_map, "patch_saliency")
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
    eng, x = _volume_check(model, img, what)
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
