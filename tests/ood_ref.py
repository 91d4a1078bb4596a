"""Float64 numpy restatements of everything gaviko_amd.ood and csrc/ood.hip compute, written from the definitions (include/gaviko_hip.h,
gaviko_amd/ood.py), not from the code.  tests/test_ood.py checks these against sklearn / scipy; tests/test_ood_gpu.py checks the device
against these."""
import math

import numpy as np


def centred(x, labels, mean):
    """d_i = fl32(x_i - mean[labels_i]) as float64 (labels None: row 0), with rows whose label is outside [0, K) dropped."""
    x = np.asarray(x, dtype=np.float32)
    mean = np.asarray(mean, dtype=np.float32)
    lab = np.zeros(len(x), dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    ok = (lab >= 0) & (lab < len(mean))
    return (x[ok] - mean[lab[ok]]).astype(np.float64), lab[ok]


def scatter(x, labels, mean):
    """-> (S f64 [C, C] = sum d d^T, r4 = sum (||d||^2)^2, count i64 [K])"""
    d, lab = centred(x, labels, mean)
    n2 = (d * d).sum(1)
    return d.T @ d, float((n2 * n2).sum()), np.bincount(lab, minlength=len(mean))[:len(mean)]


def ledoit_wolf(S, r4, n):
    """lambda = beta / delta with Sigma = S / n, mu = tr Sigma / C, delta = ||Sigma - mu I||_F^2 / C,
    beta = min((r4 / n - ||Sigma||_F^2) / (n C), delta); 0 when delta or beta is 0."""
    S = np.asarray(S, dtype=np.float64)
    C = S.shape[0]
    cov = S / n
    mu = np.trace(cov) / C
    fro2 = (cov ** 2).sum()
    delta = ((cov - mu * np.eye(C)) ** 2).sum() / C
    beta = min((r4 / n - fro2) / (n * C), delta)
    return 0.0 if beta == 0.0 or delta == 0.0 else float(beta / delta)


def shrunk(S, n, lam):
    """Sigma_l = (1 - l) S / n + l (tr (S / n) / C) I"""
    cov = np.asarray(S, dtype=np.float64) / n
    C = cov.shape[0]
    return (1.0 - lam) * cov + lam * (np.trace(cov) / C) * np.eye(C)


def whitening(cov_l):
    """W = L^-1 with L L^T = cov_l (numpy's Cholesky and a general inverse: independent of the scipy calls of ood.py)"""
    return np.linalg.inv(np.linalg.cholesky(np.asarray(cov_l, dtype=np.float64)))


def mahalanobis(q, W, m):
    """d2[n][k] = (W d) . (W d) with d = q_n - m_k, everything float64 from the given (fp32-valued) arrays"""
    q, W, m = (np.asarray(a, dtype=np.float64) for a in (q, W, m))
    out = np.empty((len(q), len(m)))
    for k in range(len(m)):
        z = (q - m[k]) @ W.T
        out[:, k] = (z * z).sum(1)
    return out


def logit_scores(z, T=1.0):
    """-> [N, 4] float64: max softmax probability, max logit, T logsumexp(z / T), entropy (0 log 0 = 0)"""
    z = np.asarray(z, dtype=np.float64)
    mx = z.max(1, keepdims=True)
    s = z - mx
    first = np.zeros(z.shape, dtype=bool)
    first[np.arange(len(z)), z.argmax(1)] = True                # its term is exp(0) = 1: kept apart so that log(1 + rest) keeps a tiny rest

    def log_sum(t):
        return np.log1p(np.where(first, 0.0, np.exp(t)).sum(1, keepdims=True))

    logS = log_sum(s)
    logp = s - logS
    p = np.exp(logp)
    plogp = np.where(p > 0, p * logp, 0.0)
    lse_t = mx[:, 0] + T * log_sum(s / T)[:, 0]
    return np.stack([p.max(1), mx[:, 0], lse_t, -plogp.sum(1)], 1)


def knn_score(q, g, k, metric="cosine", exclude_self=False):
    """the k-th smallest of 2 - 2 cos (cosine) or ||q - g||^2 (l2), float64"""
    q, g = np.asarray(q, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if metric == "cosine":
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        g = g / np.linalg.norm(g, axis=1, keepdims=True)
        d = 2.0 - 2.0 * (q @ g.T)
    else:
        d = ((q[:, None, :] - g[None, :, :]) ** 2).sum(2)
    if exclude_self:
        d = d.copy()
        d[np.arange(len(q)), np.arange(len(q))] = np.inf
    return np.sort(d, axis=1)[:, k - 1]


def threshold_rank(n, tpr):
    """m = ceil(n bp / 10000), bp = tpr in basis points, at least 1"""
    bp = int(round(tpr * 10000))
    return max(1, math.ceil(n * bp / 10000 - 1e-12)) if (n * bp) % 10000 else max(1, n * bp // 10000)


def threshold(scores, tpr):
    s = np.sort(np.asarray(scores))
    return s[threshold_rank(len(s), tpr) - 1]


def false_positives_at_tpr(score_in, score_out, bp=9500):
    """the number of in-distribution rows with score >= t at the largest threshold t (a score value) where the fraction of
    out-of-distribution rows with score >= t reaches bp / 10000, in exact integers"""
    si, so = np.asarray(score_in), np.asarray(score_out)
    for t in np.sort(np.unique(np.concatenate([si, so])))[::-1]:
        if int((so >= t).sum()) * 10000 >= bp * len(so):
            return int((si >= t).sum())
    return len(si)
