"""Host restatement of gvk_risk_coverage and gvk_temperature_fit (gaviko_amd/csrc/selective.hip) -- test infrastructure: the
risk-coverage integers and aurc straight from the definitions of include/gaviko_hip.h (a loop over the distinct scores, aurc summed with
math.fsum), the multiplicities from bootstrap_ref, and the temperature as the root of f' in float64 (scipy's brentq, taken to 1e-15)."""
import math

import numpy as np

import bootstrap_ref as br


def case_logits(N: int, K: int, seed: int, factor: float = 1.0, quarters: bool = False):
    """(logits f32 [N, K], labels int64 [N]): bootstrap_ref.case-style logits (noise + 3 on the label's column for 70 % of the rows) times
    `factor` -- 3 gives an overconfident model, 0.4 an underconfident one.  quarters: rounded to quarters, with two rows repeated under other
    labels, so that the softmax confidences tie."""
    g = np.random.default_rng(seed)
    labels = g.integers(0, K, N).astype(np.int64)
    logits = (g.standard_normal((N, K)) + 3.0 * np.eye(K)[labels] * (g.random((N, 1)) > 0.3)) * factor
    if quarters:
        logits = np.round(logits * 4) / 4
        if N > 3:
            logits[::4], logits[2::7] = logits[1], logits[3]
    return logits.astype(np.float32), labels


def case_scores(N: int, K: int, seed: int, quarters: bool = True):
    """(score f32 [N], labels int64 [N], pred int64 [N]): the max-probability confidence and the argmax of case_logits' float32 softmax"""
    import torch
    logits, labels = case_logits(N, K, seed, 1.0, quarters)
    proba = torch.softmax(torch.from_numpy(logits), 1).numpy()
    return proba.max(1), labels, proba.argmax(1).astype(np.int64), proba


def risk_coverage(score, labels, pred, w, need=()):
    """One replicate with integer multiplicities w [N], from the definitions: the distinct scores g in descending order, c_g / e_g the summed
    multiplicity of the rows / the wrong rows with that score, C_g / E_g their running sums, a group with c_g = 0 is not a threshold.
    -> dict: thresholds, accepted (C_g), errors (E_g) over ALL distinct scores; aurc = fsum(c_g E_g / C_g over c_g > 0) / N; at [Q][2] = (C_g, E_g)
    of the first threshold with C_g >= need[q]; total = (C_G, E_G)."""
    score, w = np.asarray(score), np.asarray(w, dtype=np.int64)
    wrong = np.asarray(pred, dtype=np.int64) != np.asarray(labels, dtype=np.int64)
    N = score.size
    vals = np.unique(score)[::-1]
    C = E = 0
    acc, err, terms, at = [], [], [], [None] * len(need)
    for v in vals:
        m = score == v
        c, e = int(w[m].sum()), int(w[m & wrong].sum())
        C, E = C + c, E + e
        acc.append(C)
        err.append(E)
        if c > 0:
            terms.append(c * E / C)                                       # exact integer product, one rounding in the division
            for q, n in enumerate(need):
                if at[q] is None and C >= n:
                    at[q] = (C, E)
    return {"thresholds": vals, "accepted": np.array(acc, dtype=np.int64), "errors": np.array(err, dtype=np.int64),
            "aurc": math.fsum(terms) / N, "at": np.array(at, dtype=np.int64).reshape(len(need), 2), "total": (C, E)}


def replicates(score, labels, pred, need, seed, R, K, stratified):
    """risk_coverage of the R resamples gvk_bootstrap_counts draws for (seed, stratified): K = the classes of the stratified tables"""
    w = br.multiplicities(seed, R, labels, K, stratified)
    return [risk_coverage(score, labels, pred, w[b], need) for b in range(R)], w


def _rows(logits, labels, beta):
    z = np.asarray(logits, dtype=np.float64)
    d = z - z.max(1, keepdims=True)
    e = np.exp(beta * d)
    return d, e, e.sum(1), d[np.arange(z.shape[0]), labels]


def nll(logits, labels, beta) -> float:
    """mean NLL of softmax(beta z), the row terms log sum_k exp(beta (z_k - max z)) - beta (z_y - max z) added with fsum"""
    d, e, s0, dy = _rows(logits, labels, beta)
    return math.fsum(np.log(s0) - beta * dy) / len(dy)


def fprime(logits, labels, beta) -> float:
    """f'(beta) = mean_n (sum_k p_nk z_nk - z_n,y)"""
    d, e, s0, dy = _rows(logits, labels, beta)
    return math.fsum((e * d).sum(1) / s0 - dy) / len(dy)


def fsecond(logits, labels, beta) -> float:
    """f''(beta) = mean_n Var_{p_n}(z_n)"""
    d, e, s0, dy = _rows(logits, labels, beta)
    p = e / s0[:, None]
    mean = (p * d).sum(1, keepdims=True)
    return math.fsum((p * (d - mean) ** 2).sum(1)) / len(dy)


def temperature(logits, labels, t_min=0.05, t_max=20.0):
    """(beta, at_bound): the minimiser of the mean NLL over beta = 1 / T within [1 / t_max, 1 / t_min] -- a bound where f' does not change
    sign inside, else the root of f' by brentq to 1e-15"""
    from scipy.optimize import brentq
    lo, hi = 1.0 / t_max, 1.0 / t_min
    if fprime(logits, labels, hi) <= 0.0:
        return hi, True
    if fprime(logits, labels, lo) >= 0.0:
        return lo, True
    return brentq(lambda b: fprime(logits, labels, b), lo, hi, xtol=1e-15, rtol=4 * np.finfo(np.float64).eps, maxiter=500), False
