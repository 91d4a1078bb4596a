"""CPU: the host half of gaviko_amd.metrics.risk_coverage / fit_temperature -- the restatement of tests/selective_ref.py against the
textbook forms (Geifman's (1/N) sum E_n / n, scipy's scalar minimiser), the rounding of the coverages, the sort tables of
ops.selective_tables (pure torch: they run on the host too), the closed form of optimal_aurc and the argument checks of the wrappers
(every limit is checked before the device is, so each rejection is reachable here and is matched by its message)."""
import math

import numpy as np
import pytest
import torch

import selective_ref as sr
from gaviko_amd import metrics, ops
from gaviko_amd.lib import GavikoHipError


def test_reference_aurc_is_geifmans_sum_without_ties_and_weights():
    N = 200
    score, y, pred, _ = sr.case_scores(N, 5, 200, quarters=False)
    assert np.unique(score).size == N                                    # tie-free
    r = sr.risk_coverage(score, y, pred, np.ones(N, dtype=np.int64), need=[1, 100, N])
    wrong = (pred != y)[np.argsort(-score, kind="stable")]
    E = np.cumsum(wrong)
    assert 0 < E[-1] < N
    assert r["aurc"] == math.fsum(E / np.arange(1, N + 1)) / N
    assert np.array_equal(r["accepted"], np.arange(1, N + 1)) and np.array_equal(r["errors"], E)
    assert r["at"].tolist() == [[1, E[0]], [100, E[99]], [N, E[-1]]] and r["total"] == (N, E[-1])


@pytest.mark.parametrize("quarters", [False, True])
def test_reference_is_invariant_under_permuting_the_rows(quarters):
    N = 130
    score, y, pred, _ = sr.case_scores(N, 3, 130, quarters=quarters)
    w = np.random.default_rng(0).integers(0, 4, N)
    perm = np.random.default_rng(1).permutation(N)
    a = sr.risk_coverage(score, y, pred, w, need=[10, 60, 120])
    b = sr.risk_coverage(score[perm], y[perm], pred[perm], w[perm], need=[10, 60, 120])
    assert a["aurc"] == b["aurc"] and np.array_equal(a["accepted"], b["accepted"]) and np.array_equal(a["errors"], b["errors"])
    assert np.array_equal(a["at"], b["at"]) and a["total"] == b["total"]
    assert quarters == (a["thresholds"].size < N)                         # the quarter-rounded case does tie


@pytest.mark.parametrize("factor", [3.0, 0.4])
def test_reference_temperature_agrees_with_a_scalar_minimiser_of_the_nll(factor):
    """minimize_scalar sees the NLL only, whose float64 values pin the minimiser to about sqrt(2^-53) ~ 1e-8 relative: 1e-6 is asked."""
    from scipy.optimize import minimize_scalar
    logits, y = sr.case_logits(300, 5, 300, factor)
    beta, at_bound = sr.temperature(logits, y)
    assert not at_bound and abs(sr.fprime(logits, y, beta)) < 1e-14
    assert (beta < 1.0) == (factor > 1.0)                                 # an overconfident model is softened: T > 1
    m = minimize_scalar(lambda b: sr.nll(logits, y, b), bounds=(0.05, 20.0), method="bounded", options={"xatol": 1e-12})
    assert abs(m.x - beta) <= 1e-6 * beta
    assert sr.nll(logits, y, beta) <= sr.nll(logits, y, 1.0) and sr.fsecond(logits, y, beta) > 1e-2
    h = 1e-5                                                              # f' and f'' are the derivatives of the NLL they claim to be
    assert abs((sr.nll(logits, y, beta + h) - sr.nll(logits, y, beta - h)) / (2 * h) - sr.fprime(logits, y, beta)) < 1e-8
    assert abs((sr.fprime(logits, y, beta + h) - sr.fprime(logits, y, beta - h)) / (2 * h) - sr.fsecond(logits, y, beta)) < 1e-7


def test_need_rounds_up_and_keeps_integral_products():
    assert metrics.coverage_need([0.5, 0.8, 0.9, 0.95, 1.0], 10) == [5, 8, 9, 10, 10]        # 0.95 * 10 = 9.5 -> 10
    assert metrics.coverage_need([0.07, 0.29, 0.57, 0.95], 100) == [7, 29, 57, 95]           # float products 7.000000000000001, 28.999999999999996, ...
    assert metrics.coverage_need([0.5, 0.9], 1025) == [513, 923]                             # 512.5, 922.5
    assert metrics.coverage_need([1e-5, 0.001, 1.0], 7) == [1, 1, 7]                         # never below one row
    assert metrics.coverage_need([0.5, 1.0], 1) == [1, 1]


def test_optimal_aurc_is_the_curve_of_a_perfect_ranking():
    for N, E in ((1, 0), (1, 1), (10, 3), (257, 40), (64, 64)):
        wrong = np.arange(N) >= N - E                                     # the wrong rows have the lowest scores
        r = sr.risk_coverage(-np.arange(N, dtype=np.float32), wrong.astype(np.int64), np.zeros(N, dtype=np.int64), np.ones(N, dtype=np.int64))
        assert r["total"] == (N, E)
        assert abs(metrics.optimal_aurc(N, E) - r["aurc"]) <= (N + 8) * 2.0 ** -53 * r["aurc"]
    assert metrics.optimal_aurc(10, 0) == 0.0 and metrics.optimal_aurc(5, 5) == 1.0


def test_selective_tables_sort_descending_with_tie_groups():
    N = 130
    score, y, _, _ = sr.case_scores(N, 4, 77)
    t = {k: v.numpy() for k, v in ops.selective_tables(torch.from_numpy(score), torch.from_numpy(y)).items()}
    order, gend, v = t["order"], t["gend"], score[t["order"]]
    assert np.array_equal(np.sort(order), np.arange(N)) and (np.diff(v) <= 0).all() and np.array_equal(t["sorted_score"], v)
    assert np.array_equal(order, np.argsort(-score, kind="stable"))      # equal scores in row order
    assert np.array_equal(gend, N - np.searchsorted(v[::-1], v, "left")) and (gend[:-1] <= gend[1:]).all() and gend[-1] == N
    assert (gend != np.arange(1, N + 1)).any()                           # there are ties
    import bootstrap_ref as br
    rows, off = br.class_lists(y, 4)
    assert np.array_equal(t["class_rows"], rows) and np.array_equal(t["class_off"], off)
    bt = ops.bootstrap_tables(torch.rand(N, 4), torch.from_numpy(y))     # the stratified rule reads the tables bootstrap reads
    assert np.array_equal(t["class_rows"], bt["class_rows"].numpy()) and np.array_equal(t["class_off"], bt["class_off"].numpy())


def test_wrappers_reject_what_they_document():
    N = 40
    score, y, pred, _ = sr.case_scores(N, 3, 1)
    s, yt, pt = torch.from_numpy(score), torch.from_numpy(y), torch.from_numpy(pred.astype(np.int32))
    with pytest.raises(GavikoHipError, match="HIP device"):              # no CPU path
        metrics.risk_coverage(s, yt, pt)
    bad = s.clone()
    bad[3] = float("nan")
    with pytest.raises(GavikoHipError, match="NaN"):
        metrics.risk_coverage(bad, yt, pt)
    big = ops.BOOTSTRAP_MAX_ROWS + 1
    with pytest.raises(GavikoHipError, match="8192"):
        metrics.risk_coverage(torch.zeros(big), torch.zeros(big, dtype=torch.int64), torch.zeros(big, dtype=torch.int32))
    with pytest.raises(GavikoHipError, match="at most 8"):
        metrics.risk_coverage(s, yt, pt, coverages=[0.1 * i for i in range(1, 10)])
    for cov in ([0.9, 0.5], [0.0], [1.5]):
        with pytest.raises(GavikoHipError, match="ascending"):
            metrics.risk_coverage(s, yt, pt, coverages=cov)
    with pytest.raises(GavikoHipError, match="replicates"):
        metrics.risk_coverage(s, yt, pt, replicates=0)
    tables = ops.selective_tables(s, yt)
    with pytest.raises(GavikoHipError, match="8192"):
        ops.risk_coverage_counts(torch.zeros(big, dtype=torch.int64), pt, tables)
    with pytest.raises(GavikoHipError, match="at most 8"):
        ops.risk_coverage_counts(yt, pt, tables, need=list(range(1, 10)))
    with pytest.raises(GavikoHipError, match=r"within \[1, 40\]"):
        ops.risk_coverage_counts(yt, pt, tables, need=[0])
    with pytest.raises(GavikoHipError, match=r"within \[1, 40\]"):
        ops.risk_coverage_counts(yt, pt, tables, need=[5, 41])
    with pytest.raises(GavikoHipError, match="ascending"):
        ops.risk_coverage_counts(yt, pt, tables, need=[7, 5])
    with pytest.raises(GavikoHipError, match="must be 1"):               # resample = 0 is the full sample
        ops.risk_coverage_counts(yt, pt, tables, replicates=2, resample=False)
    with pytest.raises(GavikoHipError, match="HIP device"):
        ops.risk_coverage_counts(yt, pt, tables, need=[5])

    logits, yl = sr.case_logits(N, 3, 2)
    z, ylt = torch.from_numpy(logits), torch.from_numpy(yl)
    with pytest.raises(GavikoHipError, match="HIP device"):
        metrics.fit_temperature(z, ylt)
    with pytest.raises(GavikoHipError, match="HIP device"):
        ops.temperature_fit(z, ylt)
    for K in (1, ops.TEMPERATURE_MAX_CLASSES + 1):
        with pytest.raises(GavikoHipError, match=r"outside \[2, 64\]"):
            metrics.fit_temperature(torch.zeros(N, K), ylt)
        with pytest.raises(GavikoHipError, match=r"outside \[2, 64\]"):
            ops.temperature_fit(torch.zeros(N, K), ylt)
    for lo, hi in ((0.0, 20.0), (2.0, 1.0), (0.05, float("inf")), (float("nan"), 20.0)):
        with pytest.raises(GavikoHipError, match="t_min"):
            metrics.fit_temperature(z, ylt, t_min=lo, t_max=hi)
        with pytest.raises(GavikoHipError, match="t_min"):
            ops.temperature_fit(z, ylt, lo, hi)
    with pytest.raises(GavikoHipError, match="labels"):
        ops.temperature_fit(z, ylt[:-1])
