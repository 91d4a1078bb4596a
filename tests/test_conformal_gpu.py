"""-m gpu: gvk_conformal_scores and gvk_conformal_splits through gaviko_amd.ops / metrics, against the host restatement of
tests/conformal_ref.py.

Scores: every float32 must have the restatement's BITS -- each score is a fixed sequence of single fp32 roundings (include/gaviko_hip.h), so
there is no tolerance to choose.  Splits: every output is an integer and must EQUAL the restatement.  Shapes: the smallest at which the
kernels take another path -- one row, two, either side of a wave, a row past the 256-thread block, either side of the 1024-entry scan tile,
the documented limit 8192 (where the dynamic LDS limit is raised); K = 2, 5 and the full wave of 64 classes; n_cal = 1, N - 1 and N."""
import numpy as np
import pytest
import torch

import conformal_ref as cr
from gaviko_amd import metrics, ops

pytestmark = pytest.mark.gpu

ALPHAS8 = [0.0001, 0.05, 0.1, 0.2, 0.5, 0.9, 0.99, 0.9999]              # for every n <= 8192: the first asks for m = n + 1 (+inf), the last for m = 1
INT_KEYS = ("qpos", "n_seg", "size_hist", "covered_by_size", "class_test", "class_covered")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("K", [2, 3, 63, 64])
@pytest.mark.parametrize("ties", [False, True])
def test_scores_have_the_restatements_bits(dev, K, ties):
    """N = 131: 33 workgroups of 4 rows, the last one short.  ties: rows quantised to sixteenths (equal probabilities inside a row), the last
    class a copy of the first (the rank tie rule decides), row 0 one-hot."""
    N = 131
    proba, _ = cr.case(N, K, 100 + K, ties=ties)
    pd = torch.from_numpy(proba).to(dev)
    runs = [("lac", False, 0, 1, 0.01), ("aps", False, 0, 1, 0.01), ("aps", True, 7, 1, 0.01), ("aps", True, (1 << 63) + 5, 1, 0.01),
            ("raps", False, 0, 0, 0.01), ("raps", False, 0, 1, 0.3), ("raps", True, 9, K, 0.125), ("raps", True, 9, 2, 0.0), ("raps", False, 0, K + 5, 1.0)]
    for kind, randomized, seed, k_reg, lam in runs:
        got = ops.conformal_scores(pd, kind, randomized, seed, k_reg, lam)
        assert got.shape == (K, N) and got.dtype == torch.float32
        want = cr.scores(proba, kind, randomized, seed, k_reg, lam)
        bad = np.argwhere(_bits(got.cpu().numpy().T) != _bits(want))
        assert bad.size == 0, (kind, randomized, k_reg, lam, bad[:4], got.cpu().numpy().T[tuple(bad[0])], want[tuple(bad[0])])
        view = metrics.conformal_scores(pd, score=kind, randomized=randomized, seed=seed, k_reg=k_reg, lam=lam)
        assert view.shape == (N, K) and np.array_equal(_bits(view.cpu().numpy()), _bits(want))
    if ties:
        s = cr.scores(proba, "aps")
        assert s[0, K // 2] == 1.0 and (s[0] == 1.0).all()                   # the one-hot row: its class first, every other adds 0
        assert (s[:, 0] <= s[:, K - 1]).all()                               # the duplicated class ranks after its original


def _n_cal(mode, N):
    return {"1": 1, "N-1": max(1, N - 1), "N": N, "half": max(1, N // 2)}[mode]


def _check_splits(dev, proba, labels, kind, alphas, n_cal, R, seed, mondrian):
    """the device's integers of R splits against the restatement (on the restatement's scores); returns both dicts"""
    N, K = proba.shape
    S = np.ascontiguousarray(cr.scores(proba, kind, k_reg=2, lam=0.05).T)
    order, off, true = cr.tables(S, labels, mondrian)
    Sd, yd = torch.from_numpy(S).to(dev), torch.from_numpy(labels).to(dev)
    tables = ops.conformal_tables(Sd, yd, mondrian)
    assert np.array_equal(tables["order"].cpu().numpy(), order) and np.array_equal(tables["seg_off"].cpu().numpy(), off)
    assert np.array_equal(_bits(tables["sorted_score"].cpu().numpy()), _bits(true))
    out = ops.conformal_splits(Sd, yd, tables, alphas, n_cal, R, seed)
    assert set(out) == set(INT_KEYS)
    ref = cr.splits(S, labels, order, off, alphas, n_cal, R, seed)
    for k in INT_KEYS:
        got = out[k].cpu().numpy()
        assert got.dtype == np.int32 and got.shape == ref[k].shape, (k, got.shape, ref[k].shape)
        assert np.array_equal(got, ref[k]), (k, np.argwhere(got != ref[k])[:4])
    return out, ref


@pytest.mark.parametrize("N,K,R,mode,Q,mondrian,ties", [
    (1, 2, 3, "N", 1, False, False), (2, 2, 4, "1", 8, False, False), (2, 5, 3, "N", 1, True, True), (63, 5, 5, "N-1", 8, True, True),
    (64, 2, 6, "1", 1, False, True), (64, 64, 3, "half", 8, False, False), (65, 64, 7, "N-1", 8, True, False), (257, 5, 3, "half", 8, False, True),
    (257, 2, 4, "half", 1, True, False), (1024, 5, 4, "N-1", 1, True, True), (1024, 64, 3, "half", 8, False, False),
    (1025, 2, 5, "1", 8, True, True), (1025, 5, 6, "N", 8, False, False), (8192, 64, 3, "half", 8, True, False)])
def test_splits_equal_the_restatement(dev, N, K, R, mode, Q, mondrian, ties):
    proba, labels = cr.case(N, K, 7 * N + K, ties=ties and N > 1)
    alphas = ALPHAS8 if Q == 8 else [0.1]
    n_cal = _n_cal(mode, N)
    kind = ("lac", "aps", "raps")[(N + K) % 3]
    out, ref = _check_splits(dev, proba, labels, kind, alphas, n_cal, R, 40 + N, mondrian)
    assert (ref["size_hist"].sum(2) == N - n_cal).all() and (ref["n_seg"].sum(1) == n_cal).all()
    if Q == 8 and not mondrian:
        m = [cr.level_m(n_cal, a) for a in alphas]
        assert m[-1] == 1 and m[0] == n_cal + 1                            # the levels reach both edges: the smallest score, and +inf
        assert (ref["qpos"][:, 0, 0] == -1).all() and (ref["qpos"][:, -1, 0] >= 0).all()
        assert (ref["size_hist"][:, 0, K] == N - n_cal).all()              # +inf: the full set for every test row


def test_splits_with_heavy_ties_in_the_true_class_score(dev):
    """lac scores of probabilities quantised to sixteenths: at most 17 distinct true-class scores over 600 rows, so every threshold falls inside
    a long run of equal scores and the compare scores <= qhat decides for many rows at once"""
    proba, labels = cr.case(600, 5, 5, ties=True)
    assert len(np.unique(1 - proba[np.arange(600), labels])) <= 17
    for mondrian in (False, True):
        _check_splits(dev, proba, labels, "lac", ALPHAS8, 300, 5, 3, mondrian)


def test_mondrian_with_absent_and_rare_classes(dev):
    """class 1 and class 4 have no row at all (empty segments: +inf, in every set); class 2 has two rows, and in some replicate both fall into
    the test half, so the class has no calibration row there"""
    proba, labels = cr.case(257, 5, 12, sizes=[120, 0, 2, 135, 0])
    out, ref = _check_splits(dev, proba, labels, "aps", [0.1, 0.5], 128, 7, 1, True)
    assert (ref["n_seg"][:, [1, 4]] == 0).all() and (ref["qpos"][:, :, [1, 4]] == -1).all() and (ref["class_test"][:, [1, 4]] == 0).all()
    lost = (ref["n_seg"][:, 2] == 0) & (ref["class_test"][:, 2] == 2)
    assert lost.any() and not lost.all(), ref["n_seg"][:, 2]
    assert (ref["qpos"][lost][:, :, 2] == -1).all() and (ref["class_covered"][lost][:, :, 2] == 2).all()    # +inf covers both test rows
    assert (ref["size_hist"][:, :, :2] == 0).all()                          # classes 1 and 4 are in every set: no set smaller than 2


def test_two_runs_are_identical_and_a_replicate_does_not_depend_on_R(dev):
    proba, labels = cr.case(700, 5, 21, ties=True)
    Sd = ops.conformal_scores(torch.from_numpy(proba).to(dev), "aps", True, 4)
    yd = torch.from_numpy(labels).to(dev)
    tables = ops.conformal_tables(Sd, yd, True)
    a = ops.conformal_splits(Sd, yd, tables, ALPHAS8, 350, 7, 9)
    b = ops.conformal_splits(Sd, yd, tables, ALPHAS8, 350, 7, 9)
    c = ops.conformal_splits(Sd, yd, tables, ALPHAS8, 350, 3, 9)
    d = ops.conformal_splits(Sd, yd, tables, ALPHAS8, 350, 3, 10)
    for k in INT_KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k][:3], c[k]), k
    assert not torch.equal(c["size_hist"], d["size_hist"])                # another seed is another split


def test_evaluate_derives_its_figures_from_the_integers(dev):
    """10 levels = two launches with the same seed; the host figures are the stated functions of the restatement's integers"""
    N, K, R, n_cal, seed = 500, 5, 6, 200, 3
    proba, labels = cr.case(N, K, 33)
    alphas = [0.004, 0.02, 0.05, 0.1, 0.15, 0.2, 0.3, 0.5, 0.8, 0.99]       # 0.004 < 1 / 201: +inf even for the marginal threshold
    pd, yd = torch.from_numpy(proba).to(dev), torch.from_numpy(labels).to(dev)
    for mondrian in (False, True):
        ev = metrics.conformal_evaluate(pd, yd, alphas=alphas, n_cal=n_cal, replicates=R, seed=seed, mondrian=mondrian, score="raps", k_reg=2, lam=0.05,
                                        level=0.9)
        S = np.ascontiguousarray(cr.scores(proba, "raps", k_reg=2, lam=0.05).T)
        order, off, _ = cr.tables(S, labels, mondrian)
        ref = cr.splits(S, labels, order, off, alphas, n_cal, R, seed)
        for k in INT_KEYS:
            assert np.array_equal(ev.counts[k], ref[k]), k
        assert np.array_equal(_bits(ev.qhat), _bits(ref["qhat"])) and ev.qhat.shape == (R, 10, K if mondrian else 1)
        nt = float(N - n_cal)
        cov = ref["covered_by_size"].sum(2) / nt
        size = (ref["size_hist"] * np.arange(K + 1)).sum(2) / nt
        assert np.array_equal(ev.coverage, cov) and np.array_equal(ev.mean_size, size) and ev.coverage.shape == (R, 10)
        assert np.allclose(ev.coverage_mean, cov.mean(0), rtol=0, atol=1e-15) and np.allclose(ev.mean_size_mean, size.mean(0), rtol=0, atol=1e-15)
        ends = [(1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0]
        assert ev.coverage_ci[3] == tuple(np.quantile(cov[:, 3], ends)) and ev.mean_size_ci[3] == tuple(np.quantile(size[:, 3], ends))
        pooled = ref["size_hist"].sum(0)
        assert np.array_equal(ev.size_hist, pooled) and np.array_equal(ev.singleton, pooled[:, 1] / (R * nt)) and np.array_equal(ev.empty, pooled[:, 0] / (R * nt))
        want = np.full((10, K + 1), np.nan)
        np.divide(ref["covered_by_size"].sum(0), pooled, out=want, where=pooled > 0)
        assert np.array_equal(ev.coverage_by_size, want, equal_nan=True) and np.isnan(ev.coverage_by_size).any()
        assert np.array_equal(ev.class_coverage, ref["class_covered"] / ref["class_test"][:, None, :].astype(np.float64))
        assert np.array_equal(ev.infinite, (ref["qpos"] < 0).mean((0, 2))) and ev.infinite[0] > 0 and ev.infinite[-1] == 0
        assert (ev.seed, ev.n_cal, ev.n_test, ev.mondrian, ev.score, ev.level, ev.alphas) == (seed, n_cal, N - n_cal, mondrian, "raps", 0.9, tuple(alphas))
    default = metrics.conformal_evaluate(pd, yd, replicates=4)
    assert default.n_cal == 250 and default.coverage.shape == (4, 1) and default.alphas == (0.1,)
    lone = cr.case(60, 3, 2, sizes=[58, 2, 0])
    ev = metrics.conformal_evaluate(torch.from_numpy(lone[0]).to(dev), torch.from_numpy(lone[1]).to(dev), n_cal=50, replicates=16, seed=1)
    assert np.isnan(ev.class_coverage[:, :, 2]).all() and ev.class_undefined[2] == 16 and 0 < ev.class_undefined[1] < 16


@pytest.mark.parametrize("mondrian", [False, True])
def test_calibrated_sets_follow_the_membership_rule_of_the_evaluation(dev, mondrian):
    """a predictor calibrated on the calibration rows of split b builds, for the test rows of split b, the sets the evaluation counted"""
    N, K, n_cal, seed, alpha = 300, 4, 120, 6, 0.1
    proba, labels = cr.case(N, K, 44, ties=True)
    pd, yd = torch.from_numpy(proba).to(dev), torch.from_numpy(labels).to(dev)
    ev = metrics.conformal_evaluate(pd, yd, alphas=(alpha,), n_cal=n_cal, replicates=3, seed=seed, mondrian=mondrian, score="aps")
    for b in range(3):
        cal = cr.calibration_rows(seed, b, N, n_cal)
        pred = metrics.conformal_calibrate(pd[torch.from_numpy(cal).to(dev)], labels[cal], alpha=alpha, mondrian=mondrian, score="aps")
        assert pred.qhat.shape == (K,) and pred.qhat.dtype == np.float32 and pred.n == n_cal and pred.alpha == alpha and pred.mondrian == mondrian
        assert np.array_equal(_bits(pred.qhat), _bits(np.broadcast_to(ev.qhat[b, 0], (K,))))
        sets = pred.sets(pd[torch.from_numpy(~cal).to(dev)])
        want = cr.scores(proba[~cal], "aps") <= pred.qhat[None, :]
        assert sets.mask.dtype == np.bool_ and np.array_equal(sets.mask, want) and np.array_equal(sets.size, want.sum(1))
        assert np.array_equal(np.bincount(sets.size, minlength=K + 1), ev.counts["size_hist"][b, 0])
        covered = sets.mask[np.arange((~cal).sum()), labels[~cal]]
        assert np.array_equal(np.bincount(sets.size[covered], minlength=K + 1), ev.counts["covered_by_size"][b, 0])
    few = metrics.conformal_calibrate(pd[:5], labels[:5], alpha=0.1, mondrian=mondrian)      # ceil(6 * 0.9) = 6 > 5 rows
    assert np.isinf(few.qhat).all() and few.sets(pd).mask.all() and (few.sets(pd).size == K).all()


def test_evaluator_compute_is_unchanged_without_conformal(dev):
    g = np.random.default_rng(3)
    logits = torch.from_numpy(g.standard_normal((200, 5)).astype(np.float32)).to(dev)
    labels = torch.from_numpy(g.integers(0, 5, 200)).to(dev)
    ev = metrics.Evaluator(5, dev)
    ev.update(logits[:90], labels[:90])
    ev.update(logits[90:], labels[90:])
    before = ev.compute()
    assert set(before) == {"accuracy", "quadratic_kappa", "auc", "confusion", "y_pred", "y_pred_proba", "y_test", "calibration"}
    after = ev.compute(conformal=None)
    with_sets = ev.compute(conformal=0.2, seed=5)
    assert set(after) == set(before) and set(with_sets) == set(before) | {"conformal"}
    for other in (after, with_sets):
        for k in before:
            if k == "calibration":
                assert all(np.array_equal(before[k][j], other[k][j], equal_nan=True) for j in before[k])
            else:
                assert np.array_equal(before[k], other[k]), k
    c = with_sets["conformal"]
    direct = metrics.conformal_evaluate(torch.from_numpy(before["y_pred_proba"]).to(dev), labels, alphas=(0.2,), seed=5)
    assert c.alphas == (0.2,) and c.coverage.shape == (1000, 1) and c.n_cal == 100 and np.array_equal(c.coverage, direct.coverage)
    both = ev.compute(conformal=[0.1, 0.3], bootstrap=8)
    assert both["conformal"].coverage.shape == (8, 2)
