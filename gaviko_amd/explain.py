"""Attention maps and attention rollout: what the model attends to.

In the reference every global self-attention runs its probabilities through an `nn.Softmax` module (`Attention.attend`,
vision_transformer.py:50,67), and a forward hook there yields the attention maps.  Here the modules are parameter containers and the
flash kernels never build the probability matrix, so the maps are recomputed from the forward's own buffers: an inference forward in a
workspace of its own keeps every layer's qkv and softmax statistics (Engine.attention_forward), and csrc/attention_map.hip forms the
row-weighted sums of P from them, as the backward recomputes P from lse.

    logits, maps = attention_maps(model, img)            # maps[i]: [B, H, T_i], the pooled query's attention in layer i
    logits, rel = attention_rollout(model, img)          # rel: [B, T], sums to 1 per sample
    grid = patch_grid(model, rel)                        # [B, D/pd, H/ph, W/pw]

Only the bf16 path and the global self-attention are covered; the MWSA local attention and the GPA cross-attention are not.
"""
from __future__ import annotations

from typing import List, Tuple, Union

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


def patch_grid(model, relevance: torch.Tensor) -> torch.Tensor:
    """[..., T] relevance (or a map of a layer whose sequence is the embedding's) -> [..., D/pd, H/ph, W/pw]: the patch rows (at the
    method's own row offset) in patch-grid order.  Upsampling to the volume is torch.nn.functional.interpolate's job."""
    eng = model._engine()
    if relevance.shape[-1] != eng.T:
        raise L.GavikoHipError(f"patch_grid: expected a last dimension of T = {eng.T} tokens, got {tuple(relevance.shape)}")
    patches = relevance[..., eng.row_off: eng.row_off + eng.N]
    return patches.reshape(*relevance.shape[:-1], *eng.grid)
