"""Feature embeddings of a trained model and the kNN / prototype probes run on them, all on the device.

With the reference a user reads the representation with a forward pre-hook on the head's nn.Linear and a hook per block, then takes the
vectors to the host for sklearn.  Here:

    from gaviko_amd import features
    e = features.embed(model, img, layers="all")            # e.pooled [B, C]: the head Linear's input; e.logits; e.cls / e.patch_mean [n, B, C]
    bank = features.FeatureBank(e.pooled.shape[1], img.device)
    bank.add(e.pooled, labels)                               # device-resident, grows by torch.cat
    nb = features.knn(query, bank, k=20, metric="cosine")    # Neighbors(idx i32 [Nq, k], score f32 [Nq, k]), best first
    p = features.knn_classify(bank, bank, bank.labels, k=20, num_classes=5, weights="softmax", exclude_self=True)     # leave-one-out
    protos = features.prototypes(bank.features, bank.labels, 5)
    pred, score = features.nearest_prototype(query, protos)

Rows.  pooled is the mean over the rows the method's head pools of the final LayerNorm (GAViKO: prompts + CLS; DVPT: row 0, a prompt, or
rows 0..P with pool='mean'; the others: row 0 or all rows).  Layer index l names the global token stream ENTERING layer l; l = depth is the
output of the last layer, before transformer.norm.  cls[l] is the CLS row of that stream (row 0 for VPT's [cls | prompts | patches], else
the row in front of the patches), patch_mean[l] the mean over its patch rows -- for deep VPT, whose sequence shrinks layer by layer, the
rows the layer itself still has.  GAViKO's local stream is not summarised.

Ties.  Neighbours are ordered by the fp32 score (inner product: larger first; squared L2: smaller first); an exact tie goes to the lower
bank index.  'cosine' normalises both sides (gvk_l2_normalize_rows) and takes inner products.  A vote tie goes to the lower class.

The forwards are Engine.feature_forward (engine_analysis.py).  Nothing here touches module flags, .grad, the flat gradient buffer or the
state of a pending backward.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import lib as L
from . import ops
from ._checks import batch_rows, volume_check

METRICS = ("cosine", "ip", "l2")


class Embedding(NamedTuple):
    pooled: torch.Tensor                    # f32 [B, C]: the input of the head's nn.Linear
    logits: torch.Tensor                    # f32 [B, K]
    layers: Tuple[int, ...]                 # the layer indices of cls / patch_mean (() when none was asked for)
    cls: Optional[torch.Tensor]             # f32 [n, B, C]: the CLS row of the stream entering each layer
    patch_mean: Optional[torch.Tensor]      # f32 [n, B, C]: the mean over that stream's patch rows


class Neighbors(NamedTuple):
    idx: torch.Tensor                       # i32 [Nq, k]: bank rows, best first
    score: torch.Tensor                     # f32 [Nq, k]: inner product ('cosine', 'ip') or squared distance ('l2')


class KnnPrediction(NamedTuple):
    probs: torch.Tensor                     # f32 [Nq, K]
    pred: torch.Tensor                      # i32 [Nq]
    idx: torch.Tensor
    score: torch.Tensor


class Prototypes(NamedTuple):
    mean: torch.Tensor                      # f32 [K, C]
    count: torch.Tensor                     # i32 [K]


def _layers(eng, layers):
    if layers is None:
        return None
    if isinstance(layers, str):
        if layers != "all":
            raise L.GavikoHipError(f"embed: layers={layers!r}: expected None, 'all' or a sorted tuple of indices within [0, {eng.depth}]")
        return tuple(range(eng.depth + 1))
    try:
        layers = tuple(layers)
    except TypeError:
        raise L.GavikoHipError(f"embed: layers={layers!r}: expected None, 'all' or a sorted tuple of indices within [0, {eng.depth}]") from None
    if not layers or any(isinstance(l, bool) or not isinstance(l, int) or not 0 <= l <= eng.depth for l in layers) \
            or any(a >= b for a, b in zip(layers, layers[1:])):
        raise L.GavikoHipError(f"embed: layers={layers!r}: expected strictly increasing ints within [0, {eng.depth}] (l: the stream entering "
                               f"layer l; {eng.depth}: the output of the last layer)")
    return layers


def embed(model, img: torch.Tensor, *, layers=None, batch: Optional[int] = None) -> Embedding:
    """The representation of every volume: the head Linear's input, the logits and, with `layers`, the CLS row and the patch-row mean of
    the token stream entering each named layer ('all': 0 .. depth).  The volumes go through Engine.feature_forward in chunks of `batch`
    (default min(B, 8); a last partial chunk is padded with repeats that are dropped); everything stays on the device, and the result is
    bit-identical for every chunk size.  Runs on every method and both precision paths."""
    eng, x = volume_check(model, img, "embed")
    lay = _layers(eng, layers)
    B = x.shape[0]
    bs = batch_rows(batch, min(B, 8), "embed: ")
    dev, C, n = x.device, eng.C, 0 if lay is None else len(lay)
    pooled = torch.empty((B, C), device=dev)
    logits = torch.empty((B, eng.K), device=dev)
    cls = torch.empty((n, B, C), device=dev) if n else None
    patch = torch.empty((n, B, C), device=dev) if n else None
    with torch.no_grad():
        for c0 in range(0, B, bs):
            m = min(bs, B - c0)
            xc = x[c0:c0 + m]
            if m < bs:
                xc = torch.cat([xc, x[B - 1:B].expand(bs - m, -1, -1, -1, -1)])
            r = eng.feature_forward(xc, lay)
            logits[c0:c0 + m].copy_(r[0][:m])
            pooled[c0:c0 + m].copy_(r[1][:m])
            if n:
                cls[:, c0:c0 + m].copy_(r[2][:, :m])
                patch[:, c0:c0 + m].copy_(r[3][:, :m])
    return Embedding(pooled, logits, lay or (), cls, patch)


def _matrix(t, what, C=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise L.GavikoHipError(f"{what}: expected a tensor on the HIP device (there is no CPU path)")
    if t.dim() != 2 or t.shape[0] < 1:
        raise L.GavikoHipError(f"{what}: expected [N, C], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise L.GavikoHipError(f"{what}: expected float32, got {t.dtype}")
    if C is not None and t.shape[1] != C:
        raise L.GavikoHipError(f"{what}: C = {t.shape[1]}, expected {C}")
    return t.detach().contiguous()


def _labels(labels, n, num_classes, device, what):
    """-> i32 [n] device labels, checked against [0, num_classes) on the host side (one read of min and max), as metrics.calibration does."""
    if labels is None:
        raise L.GavikoHipError(f"{what}: labels are required")
    lab = torch.as_tensor(labels)
    if lab.dim() != 1 or lab.numel() != n or lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise L.GavikoHipError(f"{what}: expected {n} integer labels, got {tuple(lab.shape)} {lab.dtype}")
    lab = lab.to(device)
    if num_classes is not None:
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or num_classes < 1:
            raise L.GavikoHipError(f"{what}: num_classes = {num_classes!r}: expected a positive int")
        lo, hi = int(lab.min()), int(lab.max())
        if lo < 0 or hi >= num_classes:
            raise L.GavikoHipError(f"{what}: labels within [{lo}, {hi}] outside [0, {num_classes})")
    return lab.to(torch.int32).contiguous()


class FeatureBank:
    """Device-resident feature rows [Ng, C] with optional integer labels; add() appends by torch.cat."""

    def __init__(self, dim: int, device):
        if isinstance(dim, bool) or not isinstance(dim, int) or dim < 4 or dim % 4 or dim > ops.FEATURE_MAX_DIM:
            raise L.GavikoHipError(f"FeatureBank: dim = {dim!r} (a multiple of 4 within [4, {ops.FEATURE_MAX_DIM}])")
        self.dim, self.device = dim, torch.device(device)
        if self.device.type != "cuda":
            raise L.GavikoHipError(f"FeatureBank: device {self.device} is not the HIP device (there is no CPU path)")
        self.features = torch.empty((0, dim), device=self.device)
        self.labels: Optional[torch.Tensor] = None
        self._normalized = None

    def __len__(self):
        return self.features.shape[0]

    def add(self, features: torch.Tensor, labels=None) -> "FeatureBank":
        f = _matrix(features, "FeatureBank.add features", self.dim)
        if (labels is None) != (self.labels is None) and len(self):
            raise L.GavikoHipError("FeatureBank.add: either every row has a label or none has")
        lab = None if labels is None else _labels(labels, f.shape[0], None, self.device, "FeatureBank.add")
        if lab is not None and int(lab.min()) < 0:
            raise L.GavikoHipError(f"FeatureBank.add: negative label {int(lab.min())}")
        self.features = torch.cat([self.features, f.to(self.device)])
        if lab is not None:
            self.labels = lab if self.labels is None else torch.cat([self.labels, lab])
        self._normalized = None
        return self

    def normalized(self) -> torch.Tensor:
        """The rows divided by their L2 norms (cached until the next add)."""
        if not len(self):
            raise L.GavikoHipError("FeatureBank.normalized: the bank is empty")
        if self._normalized is None:
            self._normalized = ops.l2_normalize_rows(self.features)
        return self._normalized


def _sides(query, bank, metric, what):
    """-> (q, g, same): contiguous f32 matrices as the kernel takes them for `metric`; same: query IS the bank."""
    if metric not in METRICS:
        raise L.GavikoHipError(f"{what}: metric={metric!r}: expected one of {METRICS}")
    same = query is bank
    if isinstance(bank, FeatureBank):
        if not len(bank):
            raise L.GavikoHipError(f"{what}: the bank is empty")
        g = bank.normalized() if metric == "cosine" else bank.features
        C = bank.dim
    else:
        g = _matrix(bank, f"{what} bank")
        C = g.shape[1]
        same = same or (isinstance(query, torch.Tensor) and query.data_ptr() == g.data_ptr() and tuple(query.shape) == tuple(g.shape))
        if metric == "cosine":
            g = ops.l2_normalize_rows(g)
    if same:
        return g, g, True
    q = _matrix(query.features if isinstance(query, FeatureBank) else query, f"{what} query", C)
    if metric == "cosine":
        q = ops.l2_normalize_rows(q)
    return q, g, False


def knn(query, bank, k: int, metric: str = "cosine", exclude_self: bool = False) -> Neighbors:
    """The k nearest bank rows of every query row.  query: f32 [Nq, C] (or a FeatureBank); bank: a FeatureBank or f32 [Ng, C].  metric
    'cosine' (both sides normalised, inner product), 'ip' or 'l2' (squared distance).  exclude_self: leave-one-out on the bank itself --
    query must be the bank, and row i never returns i."""
    q, g, same = _sides(query, bank, metric, "knn")
    excl = None
    if exclude_self:
        if not same:
            raise L.GavikoHipError("knn: exclude_self=True needs the query to be the bank itself (pass the same object)")
        excl = torch.arange(g.shape[0], dtype=torch.int32, device=g.device)
    idx, score = ops.feature_topk(q, g, k, "l2" if metric == "l2" else "ip", exclude=excl)
    return Neighbors(idx, score)


def knn_classify(query, bank, labels, k: int, num_classes: int, metric: str = "cosine", weights: str = "uniform", temperature: float = 0.07,
                 exclude_self: bool = False) -> KnnPrediction:
    """kNN classification.  weights 'uniform': probs = votes / k; 'softmax' (the DINO protocol): w_j = exp((s_j - s_0) / temperature) with
    s the similarity (for 'l2' the negated distance), normalised.  labels: [Ng] integers within [0, num_classes) (checked on the host side)."""
    ng = len(bank) if isinstance(bank, FeatureBank) else (bank.shape[0] if isinstance(bank, torch.Tensor) and bank.dim() == 2 else -1)
    if weights not in ("uniform", "softmax"):
        raise L.GavikoHipError(f"knn_classify: weights={weights!r}: expected 'uniform' or 'softmax'")
    if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= ops.VOTE_MAX_CLASSES:
        raise L.GavikoHipError(f"knn_classify: num_classes = {num_classes!r} outside [2, {ops.VOTE_MAX_CLASSES}]")
    if not (isinstance(bank, FeatureBank) or (isinstance(bank, torch.Tensor) and bank.is_cuda)):
        raise L.GavikoHipError("knn_classify: the bank must be a FeatureBank or a tensor on the HIP device (there is no CPU path)")
    dev = bank.device
    lab = _labels(labels, ng, num_classes, dev, "knn_classify")
    nb = knn(query, bank, k, metric, exclude_self)
    sim = nb.score if metric != "l2" else -nb.score
    probs, pred = ops.knn_vote(nb.idx, sim, lab, num_classes, weights, temperature)
    return KnnPrediction(probs, pred, nb.idx, nb.score)


def prototypes(features: torch.Tensor, labels, num_classes: int) -> Prototypes:
    """Per-class mean rows (class prototypes) and counts; an empty class has count 0 and a row of zeros."""
    f = _matrix(features.features if isinstance(features, FeatureBank) else features, "prototypes features")
    lab = _labels(labels, f.shape[0], num_classes, f.device, "prototypes")
    return Prototypes(*ops.class_means(f, lab, num_classes))


def nearest_prototype(query: torch.Tensor, protos: Prototypes, metric: str = "cosine"):
    """Nearest-class-mean classification -> (pred i32 [Nq], score f32 [Nq, K]).  gvk_feature_topk with k = the number of non-empty classes
    over their prototypes; score[n, c] is the similarity (inner product of normalised rows, inner product, or squared distance) to class
    c, NaN for an empty class.  pred: the best class, the lower one on an exact tie."""
    if not isinstance(protos, Prototypes):
        raise L.GavikoHipError("nearest_prototype: protos must come from prototypes()")
    K = protos.mean.shape[0]
    live = torch.nonzero(protos.count > 0).flatten()
    nl = int(live.numel())
    if nl < 1:
        raise L.GavikoHipError("nearest_prototype: every class is empty")
    if nl > ops.TOPK_MAX_K:
        raise L.GavikoHipError(f"nearest_prototype: {nl} non-empty classes, at most {ops.TOPK_MAX_K}")
    bank = protos.mean if nl == K else protos.mean[live].contiguous()
    nb = knn(query, bank, nl, metric)
    cls = live.to(torch.int32)[nb.idx.long()]                           # [Nq, nl] class of every rank
    score = torch.full((nb.idx.shape[0], K), float("nan"), device=bank.device)
    score.scatter_(1, cls.long(), nb.score)
    return cls[:, 0].contiguous(), score
