"""CPU: the host half of gaviko_amd.metrics.conformal_* -- the restatement of tests/conformal_ref.py against its naive second definition,
ops.conformal_tables (pure torch: it runs on the host too), the level expression at its edges, the argument checks of the wrappers (all
raised before anything touches the device), the finite-sample validity of the split rule on the restatement alone, and the declarations."""
import os
import re

import numpy as np
import pytest
import torch

import conformal_ref as cr
from conftest import ROOT
from gaviko_amd import lib, metrics, ops
from gaviko_amd.lib import GavikoHipError


@pytest.mark.parametrize("kind,randomized", [("lac", False), ("aps", False), ("aps", True), ("raps", False), ("raps", True)])
@pytest.mark.parametrize("ties", [False, True])
def test_scores_restatement_equals_the_row_by_row_definition(kind, randomized, ties):
    proba, _ = cr.case(41, 7, 3, ties=ties)
    for k_reg, lam in ((1, 0.01), (0, 0.25), (7, 0.5)):
        s = cr.scores(proba, kind, randomized, 11, k_reg, lam)
        u = cr.row_u(11, 41)
        for n in range(41):
            want = dict(cr.naive_row_scores(proba[n], kind, u[n] if randomized else None, k_reg, lam))
            assert all(s[n, k].tobytes() == np.float32(v).tobytes() for k, v in want.items()), (n, s[n], want)
    assert s.dtype == np.float32
    r = cr.ranks(proba)
    assert (np.sort(r, 1) == np.arange(7)).all()                           # a permutation in every row, ties included
    if ties:
        assert (r[:, 0] < r[:, 6]).all()                                    # class 6 duplicates class 0: the lower index ranks first


def test_row_u_is_a_24_bit_fraction():
    u = cr.row_u(5, 1000)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and len(np.unique(u)) > 990
    assert ((u.astype(np.float64) * 2 ** 24) % 1 == 0).all()


@pytest.mark.parametrize("mondrian", [False, True])
@pytest.mark.parametrize("kind,ties", [("lac", True), ("aps", False), ("raps", True)])
def test_split_restatement_equals_the_naive_definition(kind, ties, mondrian):
    N, K, n_cal, R, seed = 90, 4, 37, 3, 5
    proba, labels = cr.case(N, K, 8, ties=ties)
    alphas = [0.02, 0.1, 0.3, 0.9]
    S = np.ascontiguousarray(cr.scores(proba, kind, k_reg=2, lam=0.05).T)
    order, off, _ = cr.tables(S, labels, mondrian)
    got = cr.splits(S, labels, order, off, alphas, n_cal, R, seed)
    for b in range(R):
        cal = cr.calibration_rows(seed, b, N, n_cal)
        assert cal.sum() == n_cal
        want = cr.naive_split(proba, labels, cal, alphas, kind, mondrian, k_reg=2, lam=0.05)
        assert np.array_equal(got["qhat"][b], want["qhat"]), (b, got["qhat"][b], want["qhat"])
        for k in ("size_hist", "covered_by_size", "class_test", "class_covered"):
            assert np.array_equal(got[k][b], want[k]), (k, b)
        assert got["size_hist"][b].sum(1).tolist() == [N - n_cal] * len(alphas) and got["n_seg"][b].sum() == n_cal
    assert (got["qpos"] >= 0).any() and ((got["qpos"] < 0) == np.isinf(got["qhat"])).all()


def test_split_keys_are_distinct_and_a_replicate_does_not_depend_on_R():
    keys = cr.split_keys(3, 2, 8192)
    assert len(np.unique(keys)) == 8192 and ((keys & np.uint32(0x1FFF)) == np.arange(8192)).all()
    a, b = cr.calibration_rows(3, 2, 100, 40), cr.calibration_rows(3, 3, 100, 40)
    assert a.sum() == b.sum() == 40 and (a != b).any()
    assert cr.calibration_rows(3, 2, 100, 100).all()


def test_level_expression_at_its_edges():
    """m = ceil((n + 1)(1 - alpha)): m = 1, m = n, m = n + 1 (+inf: every class in every set), and a segment with no calibration row"""
    assert cr.level_m(9, 0.95) == 1 and cr.level_m(9, 0.1) == 9 and cr.level_m(9, 0.05) == 10 and cr.level_m(0, 0.5) == 1
    assert cr.level_m(99, 0.1) == 90 and cr.level_m(999, 0.1) == 900     # (n + 1)(1 - alpha) an integer up to rounding: the float64 value decides
    assert cr.level_m(19, 0.05) == int(np.ceil(20 * (1.0 - 0.05)))
    N, K, n_cal = 30, 3, 9
    g = np.random.default_rng(0)
    S = g.random((K, N)).astype(np.float32)
    labels = np.r_[np.zeros(20, np.int64), np.ones(10, np.int64)]           # class 2 absent
    order, off, true = cr.tables(S, labels, False)
    out = cr.splits(S, labels, order, off, [0.95, 0.1, 0.05], n_cal, 2, 4)
    for b in range(2):
        cal = cr.calibration_rows(4, b, N, n_cal)
        srt = np.sort(S[labels, np.arange(N)][cal])
        assert out["qhat"][b, 0, 0] == srt[0] and out["qhat"][b, 1, 0] == srt[-1] and np.isinf(out["qhat"][b, 2, 0])
        assert out["qpos"][b, 2, 0] == -1 and true[out["qpos"][b, 1, 0]] == srt[-1]
        assert out["size_hist"][b, 2].tolist() == [0] * K + [N - n_cal]     # +inf: the full set for every test row, all covered
        assert out["covered_by_size"][b, 2, K] == N - n_cal
    order, off, _ = cr.tables(S, labels, True)
    assert off.tolist() == [0, 20, 30, 30]
    out = cr.splits(S, labels, order, off, [0.5], n_cal, 2, 4)
    assert (out["n_seg"][:, 2] == 0).all() and (out["qpos"][:, 0, 2] == -1).all() and np.isinf(out["qhat"][:, 0, 2]).all()
    assert (out["size_hist"][:, 0, 0] == 0).all()                          # class 2 has no threshold: it is in every set


@pytest.mark.parametrize("alpha", [0.05, 0.1, 0.2])
def test_marginal_coverage_over_splits_has_its_exact_expectation(alpha):
    """Continuous, tie-free scores: over random splits the coverage of a test row is m / (n_cal + 1) exactly (its true-class score is
    equally likely at every rank among the n_cal + 1), so the mean over R = 2000 splits lies within 4 of its own standard errors of it."""
    N, n_cal, R, K = 400, 200, 2000, 3
    g = np.random.default_rng(20260 + int(alpha * 100))
    S = g.random((K, N)).astype(np.float32)
    assert len(np.unique(S)) == S.size
    labels = g.integers(0, K, N).astype(np.int64)
    order, off, _ = cr.tables(S, labels, False)
    out = cr.splits(S, labels, order, off, [alpha], n_cal, R, 17)
    cov = out["covered_by_size"][:, 0].sum(1) / float(N - n_cal)
    want = cr.level_m(n_cal, alpha) / (n_cal + 1.0)
    se = cov.std(ddof=1) / np.sqrt(R)
    print(f"alpha={alpha}: mean coverage {cov.mean():.6f}, expected {want:.6f}, stderr {se:.6f}, z = {(cov.mean() - want) / se:.2f}")
    assert abs(cov.mean() - want) <= 4.0 * se


@pytest.mark.parametrize("mondrian", [False, True])
def test_conformal_tables_match_the_restatement(mondrian):
    proba, labels = cr.case(70, 5, 2, ties=True, sizes=[30, 0, 25, 15, 0])
    S = np.ascontiguousarray(cr.scores(proba, "aps").T)
    order, off, true = cr.tables(S, labels, mondrian)
    t = ops.conformal_tables(torch.from_numpy(S), torch.from_numpy(labels), mondrian)
    assert t["order"].dtype == torch.int32 and t["seg_off"].dtype == torch.int32
    assert np.array_equal(t["order"].numpy(), order) and np.array_equal(t["seg_off"].numpy(), off) and np.array_equal(t["sorted_score"].numpy(), true)
    assert sorted(order.tolist()) == list(range(70))
    for g in range(len(off) - 1):
        seg = order[off[g]:off[g + 1]]
        assert (np.diff(true[off[g]:off[g + 1]]) >= 0).all() and (not mondrian or (labels[seg] == g).all())


def test_argument_checks():
    p = torch.full((40, 5), 0.2)
    y = torch.arange(40) % 5
    with pytest.raises(GavikoHipError, match=r"expected proba \[N, K\]"):
        metrics.conformal_evaluate(p[0], y)
    with pytest.raises(GavikoHipError, match="K = 1 outside"):
        metrics.conformal_evaluate(p[:, :1], y)
    with pytest.raises(GavikoHipError, match="K = 65 outside"):
        metrics.conformal_calibrate(torch.zeros(40, 65), y)
    with pytest.raises(GavikoHipError, match="N = 8193"):
        metrics.conformal_evaluate(torch.zeros(8193, 5), torch.zeros(8193, dtype=torch.int64))
    with pytest.raises(GavikoHipError, match="39 labels for 40 rows"):
        metrics.conformal_calibrate(p, y[:39])
    for bad in ((), (0.0,), (1.0,), (0.1, float("nan")), 0.1):
        with pytest.raises(GavikoHipError, match="alphas"):
            metrics.conformal_evaluate(p, y, alphas=bad)
    with pytest.raises(GavikoHipError, match="alphas"):
        metrics.conformal_calibrate(p, y, alpha=1.5)
    with pytest.raises(GavikoHipError, match="replicates"):
        metrics.conformal_evaluate(p, y, replicates=0)
    with pytest.raises(GavikoHipError, match="level"):
        metrics.conformal_evaluate(p, y, level=1.0)
    for bad in (0, 40, 2.5, True):
        with pytest.raises(GavikoHipError, match="n_cal"):
            metrics.conformal_evaluate(p, y, n_cal=bad)
    with pytest.raises(GavikoHipError, match="calibration_fraction"):
        metrics.conformal_evaluate(p, y, calibration_fraction=1.0)
    with pytest.raises(GavikoHipError, match="at least 2 rows"):
        metrics.conformal_evaluate(p[:1], y[:1])
    with pytest.raises(GavikoHipError, match="no CPU path"):
        metrics.conformal_evaluate(p, y)
    with pytest.raises(GavikoHipError, match="no CPU path"):
        metrics.conformal_calibrate(p, y)
    # the score arguments, through metrics.conformal_scores and ops.conformal_scores
    with pytest.raises(GavikoHipError, match="kind = 'top'"):
        metrics.conformal_scores(p, score="top")
    with pytest.raises(GavikoHipError, match="lac has no randomised form"):
        metrics.conformal_scores(p, score="lac", randomized=True)
    for bad in (-1, 1.0, False):
        with pytest.raises(GavikoHipError, match="k_reg"):
            metrics.conformal_scores(p, score="raps", k_reg=bad)
    for bad in (-0.1, float("inf"), float("nan")):
        with pytest.raises(GavikoHipError, match="lam"):
            metrics.conformal_scores(p, score="raps", lam=bad)
    with pytest.raises(GavikoHipError, match=r"K = 65 classes outside \[2, 64\]"):
        ops.conformal_scores(torch.zeros(3, 65))
    with pytest.raises(GavikoHipError, match=r"expected \[N, K\]"):
        ops.conformal_scores(torch.zeros(3))
    with pytest.raises(GavikoHipError, match="no CPU path"):
        ops.conformal_scores(p)
    # the split launch
    S = torch.zeros(5, 40)
    yl = y.to(torch.int64)
    tables = ops.conformal_tables(S, yl, False)
    with pytest.raises(GavikoHipError, match=r"N = 8193 rows outside \[1, 8192\]"):
        ops.conformal_splits(torch.zeros(5, 8193), yl, tables, [0.1], 1)
    with pytest.raises(GavikoHipError, match=r"K = 65 classes outside \[2, 64\]"):
        ops.conformal_splits(torch.zeros(65, 40), yl, tables, [0.1], 1)
    with pytest.raises(GavikoHipError, match="class-major"):
        ops.conformal_splits(torch.zeros(40), yl, tables, [0.1], 1)
    for bad in (0, 41, 1.0, True):
        with pytest.raises(GavikoHipError, match="n_cal"):
            ops.conformal_splits(S, yl, tables, [0.1], bad)
    with pytest.raises(GavikoHipError, match="replicates"):
        ops.conformal_splits(S, yl, tables, [0.1], 20, 0)
    with pytest.raises(GavikoHipError, match=r"Q = 9 levels outside \[1, 8\]"):
        ops.conformal_splits(S, yl, tables, [0.1] * 9, 20)
    with pytest.raises(GavikoHipError, match=r"Q = 0 levels"):
        ops.conformal_splits(S, yl, tables, [], 20)
    with pytest.raises(GavikoHipError, match=r"each within \(0, 1\)"):
        ops.conformal_splits(S, yl, tables, [0.1, 1.0], 20)
    with pytest.raises(GavikoHipError, match="seg_off"):
        ops.conformal_splits(S, yl, dict(tables, seg_off=torch.zeros(4, dtype=torch.int32)), [0.1], 20)
    with pytest.raises(GavikoHipError, match="no CPU path"):
        ops.conformal_splits(S, yl, tables, [0.1], 20)


def test_declared_bound_and_public():
    """fails on a tree without the feature: the header declares both entry points, lib.SIGNATURES binds them (tests/test_abi.py compares the
    types), the library exports them, and the public functions exist"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaviko_hip.h")).read(), flags=re.S)
    for name in ("gvk_conformal_scores", "gvk_conformal_splits"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in lib.SIGNATURES
        assert hasattr(lib.load(), name)
    assert len(lib.SIGNATURES["gvk_conformal_splits"]) == 19 and len(lib.SIGNATURES["gvk_conformal_scores"]) == 10
    assert lib.ABI_VERSION == 14
    for name in ("conformal_scores", "conformal_calibrate", "conformal_evaluate", "ConformalPredictor", "ConformalEvaluation", "PredictionSets"):
        assert hasattr(metrics, name), name
    for name in ("conformal_scores", "conformal_tables", "conformal_splits"):
        assert callable(getattr(ops, name))
    assert ops.CONFORMAL_MAX_CLASSES == 64 and ops.CONFORMAL_MAX_LEVELS == 8
    import inspect
    assert "conformal" in inspect.signature(metrics.Evaluator.compute).parameters
