"""CPU: the host half of gaviko_amd.metrics.roc_analysis / roc_compare -- the restatement of tests/roc_ref.py against sklearn on
materialised resamples (np.repeat(rows, w)), its invariance under permuting the rows, the DeLong integers against their O(N^2) definition
and the float64 variance against rational arithmetic on the same integers, the sort tables of ops.roc_tables (pure torch: they run on the
host too) and the argument checks of the wrappers (every limit is checked before the device is, so each rejection is reachable here)."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import roc_ref as rr
from gaviko_amd import metrics, ops
from gaviko_amd.lib import GavikoHipError

SPEC_BP, SENS_BP = (5000, 9000, 9500, 10000), (1, 5000, 9000, 10000)


def _materialised(score, positive, w):
    rows = np.repeat(np.arange(score.size), w)
    return score[rows], positive[rows]


@pytest.mark.parametrize("scores", ["continuous", "quarters"])
@pytest.mark.parametrize("N", [40, 257])
def test_restatement_equals_sklearn_on_materialised_resamples(N, scores):
    from sklearn.metrics import average_precision_score, roc_auc_score, roc_curve
    score, positive, grades = rr.case(N, N + 5, scores)
    thr = rr.thresholds_for(score)
    refs, w = rr.replicates(score, positive, grades, SPEC_BP, SENS_BP, thr, 3, 4, True)
    refs.append(rr.roc(score, positive, np.ones(N, dtype=np.int64), SPEC_BP, SENS_BP, thr))
    for r, wb in zip(refs, list(w) + [np.ones(N, dtype=np.int64)]):
        s, y = _materialised(score, positive, wb)
        Pn, Nn = r["total"]
        assert (Pn, Nn) == (int(y.sum()), int((~y).sum())) and Pn > 0 and Nn > 0
        assert r["auc2"] == rr.auc2_pairs(score, positive, wb)
        assert abs(r["auc2"] / (2.0 * Pn * Nn) - roc_auc_score(y, s)) <= 1e-12
        assert abs(r["ap"] - average_precision_score(y, s)) <= 1e-12
        fpr, tpr, th = roc_curve(y, s, drop_intermediate=False)
        reached = np.concatenate([[True], np.diff(r["tp"] + r["fp"], prepend=0) > 0])      # point 0 and the groups a draw reached
        tp, fp = np.concatenate([[0], r["tp"]])[reached], np.concatenate([[0], r["fp"]])[reached]
        assert np.array_equal(th[1:], r["thresholds"][reached[1:]]) and np.isinf(th[0])
        assert np.array_equal(tpr, tp / Pn) and np.array_equal(fpr, fp / Nn)
        for a, (TP, FP) in zip(SPEC_BP, r["at_spec"]):                                    # the best sensitivity sklearn's curve has at this specificity
            ok = np.array([(Nn - f) * rr.BP >= a * Nn for f in fp])
            assert TP / Pn == tpr[ok].max() and (Nn - FP) * rr.BP >= a * Nn
        for a, (TP, FP) in zip(SENS_BP, r["at_sens"]):
            ok = np.array([t * rr.BP >= a * Pn for t in tp])
            assert FP / Nn == fpr[ok].min() and TP * rr.BP >= a * Pn
        for t, (TP, FP) in zip(thr, r["at_cut"]):
            assert (TP, FP) == (int((y & (s >= t)).sum()), int((~y & (s >= t)).sum()))
        TPy, FPy, sy = r["youden"]
        J = tpr - fpr
        assert TPy / Pn - FPy / Nn == pytest.approx(J.max(), abs=1e-12) and TPy * Nn - FPy * Pn == max(a * Nn - b * Pn for a, b in zip(tp[1:], fp[1:]))
        assert np.sort(score)[::-1][sy] == r["thresholds"][np.flatnonzero((r["tp"] == TPy) & (r["fp"] == FPy) & reached[1:])[0]]


def test_restatement_edge_points():
    score = np.array([0.9, 0.8, 0.8, 0.7, 0.1], dtype=np.float32)
    positive = np.array([1, 0, 1, 1, 0], dtype=bool)
    r = rr.roc(score, positive, np.ones(5, dtype=np.int64), (0, 5000, 10000), (0, 1, 10000), (0.8, 2.0))
    assert r["tp"].tolist() == [1, 2, 3, 3] and r["fp"].tolist() == [0, 1, 1, 2] and r["total"] == (3, 2)
    assert r["auc2"] == 2 * 2 + (2 * 1 + 1) + 2 * 1 == rr.auc2_pairs(score, positive, np.ones(5, dtype=np.int64))
    assert r["at_spec"].tolist() == [[3, 2], [3, 1], [1, 0]]               # specificity >= 0: everything; >= 0.5: up to one false positive; 1: none
    assert r["at_sens"].tolist() == [[0, 0], [1, 0], [3, 1]]               # level 0 is met by point 0
    assert r["at_cut"].tolist() == [[2, 1], [0, 0]]
    assert r["youden"] == (3, 1, 3)                                        # TP Nn - FP Pn = 2, 1, 3, 0 over the four points: the third, at position 3
    assert r["ap"] == math.fsum([1 * 1 / 1, 1 * 2 / 3, 1 * 3 / 4]) / 3
    none = rr.roc(score, np.zeros(5, dtype=bool), np.ones(5, dtype=np.int64), (9000,), (9000,))
    assert none["total"] == (0, 5) and math.isnan(none["ap"]) and none["auc2"] == 0
    assert none["at_spec"].tolist() == [[0, 0]] and none["at_sens"].tolist() == [[0, 0]]
    w = np.array([0, 2, 0, 0, 3])                                          # groups no draw reached: 0.9 and 0.7
    r = rr.roc(score, positive, w, (10000,), (10000,))
    assert r["total"] == (0, 5) and r["youden"] == (0, 2, 1)


@pytest.mark.parametrize("scores", ["continuous", "quarters"])
def test_restatement_is_invariant_under_permuting_the_rows(scores):
    N = 130
    score, positive, _ = rr.case(N, 130, scores)
    thr = rr.thresholds_for(score)
    w = np.random.default_rng(0).integers(0, 4, N)
    perm = np.random.default_rng(1).permutation(N)
    a = rr.roc(score, positive, w, SPEC_BP, SENS_BP, thr)
    b = rr.roc(score[perm], positive[perm], w[perm], SPEC_BP, SENS_BP, thr)
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    assert (scores == "quarters") == (a["thresholds"].size < N)
    assert np.array_equal(rr.placements(score, positive)[perm], rr.placements(score[perm], positive[perm]))


def _curve(score, positive):
    """what gvk_roc_replicates writes with resample = 0, from numpy: order, gend and per sorted position the counts at or above its score"""
    order = np.argsort(-score, kind="stable")
    v = score[order]
    gend = score.size - np.searchsorted(v[::-1], v, "left")
    tp = np.array([(positive & (score >= x)).sum() for x in v])
    fp = np.array([(~positive & (score >= x)).sum() for x in v])
    return tp, fp, gend, order


@pytest.mark.parametrize("scores", ["continuous", "quarters", "equal"])
def test_delong_integers_equal_the_pairwise_definition(scores):
    N = 150
    score, positive, _ = rr.case(N, 7, scores)
    psi = metrics.delong_placements(*_curve(score, positive), positive)
    assert psi.dtype == np.int64 and np.array_equal(psi, rr.placements(score, positive))
    Pn, Nn = int(positive.sum()), int((~positive).sum())
    assert psi[positive].sum() == psi[~positive].sum() == rr.auc2_pairs(score, positive, np.ones(N, dtype=np.int64))
    assert 0 <= psi[positive].min() and psi[positive].max() <= 2 * Nn and psi[~positive].max() <= 2 * Pn


@pytest.mark.parametrize("N,scores", [(12, "quarters"), (150, "continuous"), (150, "quarters"), (1025, "quarters")])
def test_delong_variance_is_within_16_ulp_of_rational_arithmetic(N, scores):
    """the float64 finishing is two exact integer numerators and denominators, their four conversions, two divisions and one addition: fewer
    than ten roundings of relative size 2^-53 each, so 16 ulp of the exact value bounds it"""
    score, positive, _ = rr.case(N, N, scores)
    other = rr.case(N, N + 1, scores)[0]
    pa, pb = rr.placements(score, positive), rr.placements(other, positive)
    for x, y in ((pa, pa), (pb, pb), (pa, pb)):
        got, want = metrics.delong_covariance(x, y, positive), rr.delong_covariance_exact(x, y, positive)
        print(f"N={N} {scores}: {got!r} exact {float(want)!r}")
        assert abs(Fraction(got) - want) <= 16 * Fraction(math.ulp(float(want)))
    assert metrics.delong_covariance(pa, pa, positive) > 0.0
    assert math.isnan(metrics.delong_covariance(pa[:3], pa[:3], np.array([True, False, False])))      # one positive row: no variance


def test_delong_variance_matches_the_textbook_structural_components():
    """Sun & Xu's / DeLong's V10, V01 as float arrays: the integers reproduce them to rounding"""
    N = 200
    score, positive, _ = rr.case(N, 3, "quarters")
    sp, sn = score[positive], score[~positive]
    k = (sp[:, None] > sn[None, :]) + 0.5 * (sp[:, None] == sn[None, :])
    v10, v01 = k.mean(1), k.mean(0)
    want = v10.var(ddof=1) / sp.size + v01.var(ddof=1) / sn.size
    psi = rr.placements(score, positive)
    assert metrics.delong_covariance(psi, psi, positive) == pytest.approx(want, rel=1e-10)


def test_roc_tables_against_numpy():
    N = 130
    score, positive, grades = rr.case(N, 77, "quarters")
    t = {k: v.numpy() for k, v in ops.roc_tables(torch.from_numpy(score), torch.from_numpy(positive), torch.from_numpy(grades)).items()}
    order, gend, v = t["order"], t["gend"], score[t["order"]]
    assert np.array_equal(order, np.argsort(-score, kind="stable")) and np.array_equal(t["sorted_score"], v)
    assert np.array_equal(gend, N - np.searchsorted(v[::-1], v, "left")) and (gend != np.arange(1, N + 1)).any()
    import bootstrap_ref as br
    rows, off = br.class_lists(grades, 5)
    assert np.array_equal(t["class_rows"], rows) and np.array_equal(t["class_off"], off) and t["order"].dtype == np.int32
    d = {k: v.numpy() for k, v in ops.roc_tables(torch.from_numpy(score), torch.from_numpy(positive)).items()}     # default strata: the binary label
    rows, off = br.class_lists(positive.astype(np.int64), 2)
    assert np.array_equal(d["class_rows"], rows) and np.array_equal(d["class_off"], off) and np.array_equal(d["order"], order)


def test_binary_cut():
    proba = torch.softmax(torch.arange(20.0).reshape(4, 5) % 3, 1)
    labels = torch.tensor([0, 2, 4, 1])
    s, p = metrics.binary_cut(proba, labels, 2)
    assert torch.equal(s, proba[:, 2:].sum(1)) and p.tolist() == [False, True, True, False]
    for cut in (0, 5, -1, 2.0, True):
        with pytest.raises(GavikoHipError, match="cut"):
            metrics.binary_cut(proba, labels, cut)


def test_wrappers_reject_what_they_document():
    N = 40
    score, positive, grades = rr.case(N, 1)
    s, p, g = torch.from_numpy(score), torch.from_numpy(positive), torch.from_numpy(grades)
    with pytest.raises(GavikoHipError, match="HIP device"):              # no CPU path
        metrics.roc_analysis(s, p)
    bad = s.clone()
    bad[3] = float("nan")
    with pytest.raises(GavikoHipError, match="NaN"):
        metrics.roc_analysis(bad, p)
    big = ops.BOOTSTRAP_MAX_ROWS + 1
    with pytest.raises(GavikoHipError, match="8192"):
        metrics.roc_analysis(torch.zeros(big), torch.zeros(big, dtype=torch.bool))
    nine = [0.1 * i for i in range(1, 10)]
    for kw in (dict(specificities=nine), dict(sensitivities=nine), dict(thresholds=nine)):
        with pytest.raises(GavikoHipError, match="at most 8"):
            metrics.roc_analysis(s, p, **kw)
    for kw in (dict(specificities=[1.5]), dict(sensitivities=[-0.1]), dict(specificities=[float("nan")])):
        with pytest.raises(GavikoHipError, match=r"within \[0, 1\]"):
            metrics.roc_analysis(s, p, **kw)
    for R in (0, -3, 2.0, True):
        with pytest.raises(GavikoHipError, match="replicates"):
            metrics.roc_analysis(s, p, replicates=R)
    with pytest.raises(GavikoHipError, match="replicates"):
        metrics.roc_compare(s, s, p, replicates=0)
    with pytest.raises(GavikoHipError, match="one shape"):
        metrics.roc_compare(s, s[:-1], p)
    with pytest.raises(GavikoHipError, match="level"):
        metrics.roc_analysis(s, p, level=1.0)
    p32 = p.to(torch.int32)
    tables = ops.roc_tables(s, p32, g)
    with pytest.raises(GavikoHipError, match="8192"):
        ops.roc_counts(torch.zeros(big, dtype=torch.int32), None, tables)
    for kw in (dict(spec_bp=list(range(9))), dict(sens_bp=list(range(9))), dict(cut_rows=list(range(9)))):
        with pytest.raises(GavikoHipError, match="at most 8"):
            ops.roc_counts(p32, g, tables, **kw)
    for kw in (dict(spec_bp=[10001]), dict(sens_bp=[-1]), dict(spec_bp=[0.5]), dict(cut_rows=[N + 1])):
        with pytest.raises(GavikoHipError, match=r"integers within \[0, "):
            ops.roc_counts(p32, g, tables, **kw)
    with pytest.raises(GavikoHipError, match="replicates"):
        ops.roc_counts(p32, g, tables, replicates=0)
    with pytest.raises(GavikoHipError, match="must be 1"):               # resample = 0 is the full sample
        ops.roc_counts(p32, g, tables, replicates=2, resample=False)
    with pytest.raises(GavikoHipError, match="resample=False only"):
        ops.roc_counts(p32, g, tables, curve=True)
    with pytest.raises(GavikoHipError, match="needs the strata"):
        ops.roc_counts(p32, None, tables, stratified=True)
    with pytest.raises(GavikoHipError, match="HIP device"):
        ops.roc_counts(p32, g, tables, spec_bp=[9000])
