"""Host restatement of gvk_bootstrap_counts (gaviko_amd/csrc/bootstrap.hip) -- test infrastructure: the two resampling rules of
include/gaviko_hip.h rebuilt from dropmask.hash_u32, and a replicate's integers counted directly from its multiplicities."""
import numpy as np

from dropmask import hash_u32


def class_lists(labels: np.ndarray, K: int):
    """rows grouped by label in ascending row order, and where each class starts"""
    off = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=K))]).astype(np.int64)
    return np.argsort(labels, kind="stable").astype(np.int64), off


def multiplicities(seed: int, R: int, labels: np.ndarray, K: int, stratified: bool) -> np.ndarray:
    """w int64 [R, N]: how often replicate b draws row j.  plain: j = (hash(seed, b N + n) * N) >> 32; stratified: the
    ((hash * n_c) >> 32)-th row of the class of row n."""
    labels = np.asarray(labels, dtype=np.int64)
    N = labels.size
    h = hash_u32(seed, np.arange(R * N, dtype=np.uint64).reshape(R, N)).astype(np.uint64)
    if stratified:
        rows, off = class_lists(labels, K)
        n_c = (off[1:] - off[:-1])[labels].astype(np.uint64)
        j = rows[off[labels][None, :] + ((h * n_c[None, :]) >> np.uint64(32)).astype(np.int64)]
    else:
        j = ((h * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
    w = np.zeros((R, N), dtype=np.int64)
    for b in range(R):
        w[b] = np.bincount(j[b], minlength=N)
    return w


def confusion_weighted(labels, pred, w, K) -> np.ndarray:
    c = np.zeros((K, K), dtype=np.int64)
    np.add.at(c, (labels, pred), w)
    return c


def auc_counts_pairs(proba, labels, w, K) -> np.ndarray:
    """int64 [K, 3] by direct O(N^2) weighted pair counting: {sum w_i w_j (2 [p_i > p_j] + [p_i == p_j]), n_pos, n_neg}"""
    out = np.zeros((K, 3), dtype=np.int64)
    for c in range(K):
        pos = labels == c
        pp, pn, wp, wn = proba[pos, c], proba[~pos, c], w[pos], w[~pos]
        score = 2 * (pp[:, None] > pn[None, :]).astype(np.int64) + (pp[:, None] == pn[None, :]).astype(np.int64)
        out[c] = [(wp[:, None] * wn[None, :] * score).sum(), wp.sum(), wn.sum()]
    return out


def auc_counts_sorted(proba, labels, w, K) -> np.ndarray:
    """the same integers through the sorted prefix sums (numpy int64), for sizes where N^2 pairs are too many"""
    out = np.zeros((K, 3), dtype=np.int64)
    for c in range(K):
        p = proba[:, c]
        order = np.argsort(p, kind="stable")
        v, pos, ws = p[order], labels[order] == c, w[order]
        P = np.concatenate([[0], np.cumsum(np.where(pos, 0, ws))])          # P[k] = negatives' weight among the first k sorted rows
        below, upto = P[np.searchsorted(v, v, "left")], P[np.searchsorted(v, v, "right")]
        out[c] = [(ws * (below + upto))[pos].sum(), ws[pos].sum(), ws[~pos].sum()]
    return out


def counts(proba, labels, pred, w, K, pairs=auc_counts_pairs):
    """(confusion int64 [R, K, K], auc_counts int64 [R, K, 3]) of the replicates with multiplicities w [R, N]"""
    conf = np.stack([confusion_weighted(labels, pred, wb, K) for wb in w])
    return conf, np.stack([pairs(proba, labels, wb, K) for wb in w])


def case(N: int, K: int, seed: int, sizes=None, quarters: bool = False, signal: float = 3.0):
    """A deterministic evaluation set: (proba f32 [N, K], labels int64 [N], pred int64 [N]).  Logits = noise + signal on the label's column
    (rounded to quarters when asked, with two rows repeated under other labels, so that probabilities tie within and across classes), probabilities = their float32 softmax, predictions
    = the first largest probability.  sizes: the class sizes (labels shuffled), else labels uniform over the classes."""
    import torch
    g = np.random.default_rng(seed)
    labels = np.repeat(np.arange(K), sizes) if sizes is not None else g.integers(0, K, N)
    labels = g.permutation(labels).astype(np.int64)
    assert labels.size == N
    logits = g.standard_normal((N, K)) + signal * np.eye(K)[labels] * (g.random((N, 1)) > 0.3)
    if quarters:
        logits = np.round(logits * 4) / 4
        logits[::4], logits[2::7] = logits[1], logits[3]                     # whole rows repeated under other labels: ties in every column
    proba = torch.softmax(torch.from_numpy(logits.astype(np.float32)), 1).numpy()
    return proba, labels, proba.argmax(1).astype(np.int64)
