"""Host-side argument checks and chunk tables shared by the analysis modules (explain.py, uncertainty.py, features.py)."""
from __future__ import annotations

import torch

from . import lib as L


def volume_check(model, img, what):
    """-> (engine, the detached contiguous volume): img must be a float32 [B, 1, D, H, W] device tensor of the model's geometry, B >= 1."""
    eng = model._engine()
    if not isinstance(img, torch.Tensor) or not img.is_cuda:
        raise L.GavikoHipError(f"{what} runs on the HIP device: move the model and the input there (there is no CPU path)")
    want = (1,) + tuple(g * p for g, p in zip(eng.grid, eng.patch))
    if img.dim() != 5 or tuple(img.shape[1:]) != want or img.shape[0] < 1:
        raise L.GavikoHipError(f"{what}: expected img [B, {', '.join(map(str, want))}], got {tuple(img.shape)}")
    if img.dtype != torch.float32:
        raise L.GavikoHipError(f"{what}: expected a float32 volume, got {img.dtype}")
    return eng, img.detach().contiguous()


def batch_rows(batch, default, prefix=""):
    """The rows per engine forward of a sweep: `default` for None, else `batch`, which must be a positive int (prefix: 'name: ')."""
    if batch is None:
        return default
    if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
        raise L.GavikoHipError(f"{prefix}batch={batch!r}: expected a positive int")
    return batch


def chunk_tables(bs, device, *tables, slot):
    """Per-row Python lists -> int32 device tensors (the tables in their order, then slot), each uploaded once and padded to a multiple of
    `bs` rows: the padding repeats the last row, with slot -1 (a forward of it writes nowhere)."""
    pad = (-len(slot)) % bs
    i32 = lambda rows, fill: torch.tensor(rows + [fill] * pad, dtype=torch.int32).to(device)       # noqa: E731
    return tuple(i32(t, t[-1]) for t in tables) + (i32(slot, -1),)
