"""Host restatement of gvk_roc_replicates (gaviko_amd/csrc/roc.hip) and of the DeLong finishing of gaviko_amd.metrics -- test
infrastructure: every output straight from the definitions of include/gaviko_hip.h (a Python loop over the distinct scores, the ap sum
with math.fsum, auc2 and the placements by brute-force O(N^2) pair counting), the multiplicities from bootstrap_ref."""
import math
from fractions import Fraction

import numpy as np

import bootstrap_ref as br

BP = 10000


def case(N: int, seed: int, scores: str = "continuous", labels: str = "mixed"):
    """(score f32 [N], positive bool [N], grades int64 [N] in 0..4): grades uniform, positive = grade >= 2 (or all / none / exactly one row),
    score = a noisy sigmoid of the grade.  scores: 'continuous'; 'quarters' (logits rounded to quarters, rows repeated under other labels:
    long tie groups, as selective_ref.case_logits(quarters=True)); 'equal' (one group)."""
    g = np.random.default_rng(seed)
    grades = g.integers(0, 5, N).astype(np.int64)
    z = g.standard_normal(N) + 0.8 * (grades - 2.0)
    if scores == "quarters":
        z = np.round(z * 4) / 4
        if N > 3:
            z[::4], z[2::7] = z[1], z[3]
    score = (1.0 / (1.0 + np.exp(-z))).astype(np.float32)
    if scores == "equal":
        score = np.full(N, 0.25, dtype=np.float32)
    positive = {"mixed": grades >= 2, "all": np.ones(N, bool), "none": np.zeros(N, bool), "one": np.arange(N) == (N // 3)}[labels]
    return score, positive.copy(), grades


def cut_rows(score, thresholds):
    """m_q: the full-sample rows with score >= the q-th threshold (float32 scores widened to float64)"""
    return [int((np.asarray(score, dtype=np.float64) >= float(t)).sum()) for t in thresholds]


def thresholds_for(score):
    """the five fixed thresholds of the tests: above the largest score, below the smallest, two values that occur, one between two scores"""
    v = np.unique(score).astype(np.float64)
    between = (v[0] + v[1]) / 2 if v.size > 1 else v[0] + 0.125
    return [float(v[-1]) + 1.0, float(v[0]) - 1.0, float(v[v.size // 2]), float(v[0]), float(between)]


def roc(score, positive, w, spec_bp=(), sens_bp=(), thresholds=()):
    """One replicate with integer multiplicities w [N], from the definitions: the distinct scores v_1 > .. > v_G, tp_g / fp_g the summed
    multiplicity of the positive / negative rows with score v_g, TP_g / FP_g their running sums, point 0 = (0, 0).
    -> dict: thresholds (the distinct scores), tp, fp (TP_g, FP_g over ALL distinct scores), total (Pn, Nn), auc2, ap (fsum / Pn, NaN when
    Pn = 0), at_spec / at_sens / at_cut [Q][2], youden (TP, FP, first sorted position of the group)."""
    score, w, positive = np.asarray(score), np.asarray(w, dtype=np.int64), np.asarray(positive, dtype=bool)
    vals, inv, cnt = np.unique(score, return_inverse=True, return_counts=True)
    G = vals.size
    tp_g = np.bincount(inv, weights=w * positive, minlength=G).astype(np.int64)[::-1].tolist()     # descending score
    fp_g = np.bincount(inv, weights=w * ~positive, minlength=G).astype(np.int64)[::-1].tolist()
    start = np.concatenate([[0], np.cumsum(cnt[::-1])]).tolist()                                    # first sorted position of every group
    Pn, Nn = sum(tp_g), sum(fp_g)
    pts, TP, FP = [(0, 0)], 0, 0                                                                    # point 0 .. point G
    auc2, terms, best = 0, [], None
    for g in range(G):
        TP, FP = TP + tp_g[g], FP + fp_g[g]
        pts.append((TP, FP))
        auc2 += tp_g[g] * (2 * (Nn - FP) + fp_g[g])
        if tp_g[g] > 0:
            terms.append(tp_g[g] * TP / (TP + FP))                          # exact integer product, one rounding in the division
        if tp_g[g] + fp_g[g] > 0:
            J = TP * Nn - FP * Pn
            if best is None or J > best[0]:                                 # on a tie the smallest g stays
                best = (J, TP, FP, start[g])
    at_spec = [[p for p in pts if (Nn - p[1]) * BP >= a * Nn][-1] for a in spec_bp]
    at_sens = [[p for p in pts if p[0] * BP >= a * Pn][0] for a in sens_bp]
    at_cut = []
    for t in thresholds:
        m = score.astype(np.float64) >= float(t)
        at_cut.append((int(w[m & positive].sum()), int(w[m & ~positive].sum())))
    i64 = lambda a, Q: np.array(a, dtype=np.int64).reshape(Q, 2)           # noqa: E731
    return {"thresholds": vals[::-1], "tp": np.array([p[0] for p in pts[1:]], dtype=np.int64), "fp": np.array([p[1] for p in pts[1:]], dtype=np.int64),
            "total": (Pn, Nn), "auc2": auc2, "ap": math.fsum(terms) / Pn if Pn else float("nan"), "at_spec": i64(at_spec, len(spec_bp)),
            "at_sens": i64(at_sens, len(sens_bp)), "at_cut": i64(at_cut, len(thresholds)), "youden": best[1:]}


def auc2_pairs(score, positive, w) -> int:
    """sum over positives i, negatives j of w_i w_j (2 [s_i > s_j] + [s_i == s_j]) by direct O(N^2) counting"""
    score, w, positive = np.asarray(score), np.asarray(w, dtype=np.int64), np.asarray(positive, dtype=bool)
    sp, sn = score[positive], score[~positive]
    k = 2 * (sp[:, None] > sn[None, :]).astype(np.int64) + (sp[:, None] == sn[None, :]).astype(np.int64)
    return int((w[positive][:, None] * w[~positive][None, :] * k).sum())


def replicates(score, positive, strata, spec_bp, sens_bp, thresholds, seed, R, stratified, resample=True):
    """roc of the R resamples gvk_bootstrap_counts draws for (seed, stratified) over the strata labels; resample=False: unit multiplicities"""
    strata = np.asarray(strata, dtype=np.int64)
    w = br.multiplicities(seed, R, strata, int(strata.max()) + 1, stratified) if resample else np.ones((1, len(score)), dtype=np.int64)
    return [roc(score, positive, w[b], spec_bp, sens_bp, thresholds) for b in range(w.shape[0])], w


def scalars(r, spec_bp, sens_bp, thresholds, score):
    """the scalars gaviko_amd.metrics.roc_scalars names, of one roc(...) result, as Python floats from the definitions: a replicate without a
    positive or without a negative row has no curve (NaN), a predictive value is NaN where its own denominator is 0"""
    nan = float("nan")
    Pn, Nn = r["total"]
    ok = Pn > 0 and Nn > 0
    out = {"auc": r["auc2"] / (2.0 * Pn * Nn) if ok else nan, "average_precision": r["ap"] if ok else nan}
    for a, (TP, FP) in zip(spec_bp, r["at_spec"]):
        out[f"sens@spec={a / BP}"] = TP / Pn if ok else nan
    for a, (TP, FP) in zip(sens_bp, r["at_sens"]):
        out[f"spec@sens={a / BP}"] = (Nn - FP) / Nn if ok else nan
    for t, (TP, FP) in zip(thresholds, r["at_cut"]):
        TN, FN = Nn - FP, Pn - TP
        out[f"sens@thr={t}"], out[f"spec@thr={t}"] = (TP / Pn if ok else nan), (TN / Nn if ok else nan)
        out[f"ppv@thr={t}"], out[f"npv@thr={t}"] = (TP / (TP + FP) if TP + FP else nan), (TN / (TN + FN) if TN + FN else nan)
    TP, FP, s = r["youden"]
    sens, spec = (TP / Pn, (Nn - FP) / Nn) if ok else (nan, nan)
    out.update(youden_threshold=float(np.sort(score)[::-1][s]) if ok else nan, youden_sensitivity=sens, youden_specificity=spec,
               youden_j=sens + spec - 1.0)
    return out


def placements(score, positive) -> np.ndarray:
    """DeLong's integer placements by O(N^2) counting, row order: a positive row's 2 #{negatives lower} + #{negatives tied}, a negative
    row's 2 #{positives higher} + #{positives tied}"""
    score, positive = np.asarray(score), np.asarray(positive, dtype=bool)
    gt = (score[:, None] > score[None, :]).astype(np.int64)
    eq = (score[:, None] == score[None, :]).astype(np.int64)
    as_pos = (2 * gt + eq)[:, ~positive].sum(1)
    as_neg = (2 * gt.T + eq)[:, positive].sum(1)
    return np.where(positive, as_pos, as_neg)


def delong_covariance_exact(psi_a, psi_b, positive) -> Fraction:
    """S10 / Pn + S01 / Nn in rational arithmetic from the placements: V10_i = psi_i / (2 Nn), V01_j = psi_j / (2 Pn), S the unbiased
    covariance of each part (DeLong et al., 1988)"""
    positive = np.asarray(positive, dtype=bool)
    Pn, Nn = int(positive.sum()), int((~positive).sum())

    def cov(x, y, scale):
        x, y = [Fraction(int(v), scale) for v in x], [Fraction(int(v), scale) for v in y]
        mx, my = sum(x) / len(x), sum(y) / len(y)
        return sum((a - mx) * (b - my) for a, b in zip(x, y)) / (len(x) - 1)

    a, b = np.asarray(psi_a), np.asarray(psi_b)
    return cov(a[positive], b[positive], 2 * Nn) / Pn + cov(a[~positive], b[~positive], 2 * Pn) / Nn
