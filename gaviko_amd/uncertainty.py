"""Predictive uncertainty of a trained model: Monte-Carlo dropout and flip test-time augmentation.

Both answer "how sure is this grade" the same way: S stochastic or augmented members of every volume go through the model, and the S
logit rows of a volume are reduced to the mean probability, its entropy, the part of that entropy the members agree on (the expected
entropy) and the part they do not (the mutual information), the per-class spread and the vote.

    from gaviko_amd import uncertainty
    r = uncertainty.mc_dropout(model, img, samples=32, seed=1234)      # the dropouts the method trains with, live at inference
    r = uncertainty.tta(model, img, flips="all")                       # the 8 axis flips (or "train": the RandomFlip(axis 0) of training)
    r.probs, r.pred, r.entropy, r.mutual_info, r.std, r.votes          # device tensors; r.member_logits [B, S, K] keeps every member

Every member is built on the device straight in the engine's static input slot (csrc/uncertainty.hip: gvk_tta_volumes mirrors or
replicates the source volume, one HBM pass), the chunk's forward is the engine's recorded inference plan (Engine.member_forward,
engine_analysis.py), the logits rows are gathered on the device and one launch (gvk_predictive_stats) reduces them at the end: nothing
between the first and the last forward waits for the host.  Module flags, .grad, the flat gradient buffer and the state of a pending backward are left alone.

Member order and chunking are part of the contract.  Row o = b * S + s of the sweep is member s of volume b (sample-major); the rows are
cut into chunks of `batch` rows (default: the largest multiple of S that is <= 8, else S; a last partial chunk is padded with repeats
that write nowhere).  The dropout masks are counter-based: a chunk's masks come from the workspace's seed word, which every forward
advances by 7919, and from the row index inside the chunk.  mc_dropout is therefore reproducible for a given (seed, samples, batch), and
`epochs[c]` -- the word chunk c drew from -- is all that is needed to rebuild every mask on the host.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import torch

from . import lib as L
from . import ops
from ._checks import batch_rows, chunk_tables, volume_check

_ALL_FLIPS = [(), (0,), (1,), (0, 1), (2,), (0, 2), (1, 2), (0, 1, 2)]        # flip code = sum of 1 << axis: the codes 0 .. 7 in order


class Predictive(NamedTuple):
    probs: torch.Tensor             # f32 [B, K]: mean over the members of softmax(logits)
    pred: torch.Tensor              # i32 [B]: argmax of probs, lowest index on an exact tie
    entropy: torch.Tensor           # f32 [B]: H[mean p], nats (total uncertainty)
    expected_entropy: torch.Tensor  # f32 [B]: mean over the members of H[p_s] (aleatoric part)
    mutual_info: torch.Tensor       # f32 [B]: entropy - expected_entropy, clamped at 0 (epistemic part)
    variation_ratio: torch.Tensor   # f32 [B]: 1 - (votes of the most voted class) / S
    std: torch.Tensor               # f32 [B, K]: population standard deviation of the member probabilities
    votes: torch.Tensor             # i32 [B, K]: the members' own argmax counts (lowest index on a tie)
    member_logits: torch.Tensor     # f32 [B, S, K]
    epochs: List[int]               # the dropout seed word each chunk's forward drew from ([] for tta)


def _chunk_rows(batch, S, what):
    return batch_rows(batch, (8 // S) * S if S <= 8 else S, f"{what}: ")


def training_drop_config(model) -> dict:
    """The dropout rates the method's own training mode leaves live -- model._drop_config() as model.train() would make it -- read without
    leaving any module's `training` flag changed (every flag is saved and put back one by one: Gaviko.train() is not nn.Module.train())."""
    flags = [(m, m.training) for m in model.modules()]
    try:
        model.train()
        return dict(model._drop_config())
    finally:
        for m, f in flags:
            m.training = f


def _sweep(eng, x, S, codes, bs, drop, seed):
    """B * S members in chunks of bs rows -> (member_logits [B, S, K], epochs).  codes[s]: the flip code of member s."""
    B, K, dev = x.shape[0], eng.K, x.device
    n = B * S
    src, flip, slot = chunk_tables(bs, dev, [o // S for o in range(n)], [codes[o % S] for o in range(n)], slot=list(range(n)))
    rows = torch.empty((n, K), device=dev)
    nchunks = slot.numel() // bs
    words = None
    with torch.no_grad():
        if drop is not None:
            word = eng.member_seed(bs, dev, seed)
            words = torch.empty(nchunks, dtype=torch.int64, device=dev)
        for c in range(nchunks):
            s = slice(c * bs, (c + 1) * bs)
            eng.member_forward(x, src[s], flip[s], drop, slot=slot[s], rows=rows)
            if words is not None:
                words[c:c + 1].copy_(word)                   # stream-ordered: the word this chunk's masks were drawn from
    return rows.view(B, S, K), ([] if words is None else [int(w) for w in words.tolist()])


def _result(member_logits, epochs) -> Predictive:
    B, S, _ = member_logits.shape
    st = ops.predictive_stats(member_logits, B, S)
    return Predictive(st["probs"], st["pred"], st["entropy"], st["expected_entropy"], st["mutual_info"], st["variation_ratio"], st["std"],
                      st["votes"], member_logits, epochs)


def mc_dropout(model, img: torch.Tensor, *, samples: int = 32, batch: Optional[int] = None, seed: Optional[int] = None,
               drop: Optional[dict] = None) -> Predictive:
    """Monte-Carlo dropout (Gal & Ghahramani, 2016): `samples` inference forwards of every volume with the dropouts live that the method's
    own training mode leaves live (training_drop_config; `drop`: a dict of the same keys instead).  Raises when every live rate is 0 -- all
    members would be identical.  seed: an int fixes the workspace's seed word at the start of the sweep, and the same (seed, samples,
    batch) then gives bit-identical member_logits; None continues from wherever the word stands, so two calls differ.  epochs[c] is the
    word chunk c's masks were drawn from (seed + 7919 (c + 1) with a seed).  Runs on every method and both precision paths."""
    eng, x = volume_check(model, img, "mc_dropout")
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 1:
        raise L.GavikoHipError(f"mc_dropout: samples={samples!r}: expected a positive int")
    bs = _chunk_rows(batch, samples, "mc_dropout")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 62):
        raise L.GavikoHipError(f"mc_dropout: seed={seed!r}: expected None or an int within [0, 2^62)")
    cfg = training_drop_config(model)
    if drop is not None:
        if not isinstance(drop, dict) or set(drop) - set(cfg):
            raise L.GavikoHipError(f"mc_dropout: drop={drop!r}: expected a dict with keys from {sorted(cfg)} (this method's dropouts)")
        cfg = {k: float(v) for k, v in drop.items()}
    if any(not 0.0 <= float(v) < 1.0 for v in cfg.values()):
        raise L.GavikoHipError(f"mc_dropout: dropout rates must lie in [0, 1), got {cfg}")
    if not any(float(v) > 0.0 for v in cfg.values()):
        raise L.GavikoHipError(f"mc_dropout: every live dropout rate is 0 ({cfg}): all members would be identical -- build the model with its "
                               "training dropouts, or pass drop=")
    logits, epochs = _sweep(eng, x, samples, [0] * samples, bs, cfg, seed)
    return _result(logits, epochs)


def _flip_codes(flips):
    if isinstance(flips, str):
        if flips == "all":
            flips = _ALL_FLIPS
        elif flips == "train":
            flips = [(), (0,)]
        else:
            raise L.GavikoHipError(f"tta: flips={flips!r}: expected 'all', 'train' or a list of axis tuples over (0, 1, 2) = (D, H, W)")
    try:
        flips = [tuple(f) for f in flips]
    except TypeError:
        raise L.GavikoHipError(f"tta: flips={flips!r}: expected 'all', 'train' or a list of axis tuples over (0, 1, 2) = (D, H, W)") from None
    if not flips:
        raise L.GavikoHipError("tta: flips is empty: at least one member (e.g. [()], the volume itself)")
    codes = []
    for f in flips:
        if any(isinstance(a, bool) or not isinstance(a, int) or a not in (0, 1, 2) for a in f) or len(set(f)) != len(f):
            raise L.GavikoHipError(f"tta: flip {f!r}: axes are distinct ints from (0, 1, 2) = (D, H, W)")
        codes.append(sum(1 << a for a in f))
    return codes


def tta(model, img: torch.Tensor, *, flips="all", batch: Optional[int] = None) -> Predictive:
    """Flip test-time augmentation: one deterministic inference forward per flip of every volume.  flips: 'all' (the 8 subsets of the three
    axes, in the order of their codes sum(1 << axis)), 'train' ([(), (0,)]: the RandomFlip(axis 0) the training pipeline draws) or a list
    of axis tuples over (0, 1, 2) = (D, H, W).  member_logits[b, s] belongs to flips[s].  Runs on every method and both precision paths."""
    eng, x = volume_check(model, img, "tta")
    codes = _flip_codes(flips)
    bs = _chunk_rows(batch, len(codes), "tta")
    logits, _ = _sweep(eng, x, len(codes), codes, bs, None, None)
    return _result(logits, [])
