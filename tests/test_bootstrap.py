"""CPU: the host half of gaviko_amd.metrics.bootstrap / compare -- the two resampling rules as tests/bootstrap_ref.py restates them, the
finishing functions (integers -> float64 metrics) against sklearn on materialised resamples, the paired p-value, classification_report,
and the sort tables of ops.bootstrap_tables (pure torch: they run on the host too) with the prefix-sum form of the pair count."""
import warnings

import numpy as np
import pytest
import torch

import bootstrap_ref as br
from gaviko_amd import metrics, ops

TOL = 1e-12                                                      # what the Evaluator's metrics are held to


@pytest.mark.parametrize("N,K,sizes", [(37, 5, [3, 5, 8, 9, 12]), (257, 3, None), (1000, 5, None)])
def test_multiplicities_sum_to_the_sample_and_to_every_class(N, K, sizes):
    _, y, _ = br.case(N, K, N, sizes=sizes)
    w = br.multiplicities(11, 16, y, K, False)
    assert w.shape == (16, N) and (w >= 0).all() and (w.sum(1) == N).all()
    assert not np.array_equal(w[0], w[1])
    ws = br.multiplicities(11, 16, y, K, True)
    assert (ws.sum(1) == N).all()
    for c in range(K):
        assert (ws[:, y == c].sum(1) == (y == c).sum()).all(), c
    assert not np.array_equal(w, ws)
    assert np.array_equal(w, br.multiplicities(11, 16, y, K, False)) and not np.array_equal(w, br.multiplicities(12, 16, y, K, False))


def _sklearn_metrics(y, pred, p, K):
    from sklearn.metrics import accuracy_score, balanced_accuracy_score, cohen_kappa_score, f1_score, roc_auc_score
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # y_pred holds classes y_true lost; kappa of one class is 0 / 0
        out = {"accuracy": accuracy_score(y, pred), "quadratic_kappa": cohen_kappa_score(y, pred, weights="quadratic"),
               "balanced_accuracy": balanced_accuracy_score(y, pred), "macro_f1": f1_score(y, pred, average="macro", zero_division=0)}
    if p is None:
        return out
    if all(0 < (y == c).sum() < y.size for c in range(K)):
        # the binary call per class: the multiclass one renormalises rows that do not sum to 1 in float32, which moves ties
        out["auc"] = float(np.mean([roc_auc_score(y == c, p[:, c]) for c in range(K)]))
    else:
        out["auc"] = float("nan")
    return out


@pytest.mark.parametrize("N,K,sizes,quarters,stratified", [(37, 5, [3, 5, 8, 9, 12], True, False), (37, 5, [3, 5, 8, 9, 12], True, True),
                                                            (130, 3, None, False, False)])
def test_finishing_functions_match_sklearn_on_materialised_resamples(N, K, sizes, quarters, stratified):
    """metrics_from_counts (accuracy, kappa_quadratic, the AUC rule of macro_ovr_auc, balanced accuracy, macro-F1) and classification_report
    on the integers of every replicate, against sklearn on np.repeat(rows, w); seed 5 loses a class in 3 of the 64 plain replicates of the
    first case (kappa's squeeze, the present-class means and the NaN rule all get exercised)."""
    R = 64
    p, y, pred = br.case(N, K, N, sizes=sizes, quarters=quarters)
    w = br.multiplicities(5, R, y, K, stratified)
    conf, cnt = br.counts(p, y, pred, w, K)
    got = metrics.metrics_from_counts(conf, cnt)
    assert set(got) == set(metrics.BOOTSTRAP_METRICS)
    lost = 0
    for b in range(R):
        rows = np.repeat(np.arange(N), w[b])
        want = _sklearn_metrics(y[rows], pred[rows], p[rows].astype(np.float64), K)
        for k, v in want.items():
            if np.isnan(v):
                assert np.isnan(got[k][b]), (b, k)
            else:
                assert abs(got[k][b] - v) < TOL, (b, k, got[k][b], v)
        if np.isnan(want["auc"]):
            lost += 1
        else:
            assert abs(metrics.macro_ovr_auc(cnt[b]) - want["auc"]) < TOL
        kq = metrics.kappa_quadratic(conf[b])                   # the batch form restates it, squeeze included
        assert np.isnan(want["quadratic_kappa"]) and np.isnan(kq) or abs(kq - want["quadratic_kappa"]) < TOL
        assert np.isnan(kq) and np.isnan(got["quadratic_kappa"][b]) or abs(kq - got["quadratic_kappa"][b]) < TOL
        rep = metrics.classification_report(conf[b])
        assert abs(rep["balanced_accuracy"] - want["balanced_accuracy"]) < TOL and abs(rep["macro_f1"] - want["macro_f1"]) < TOL
    if sizes is not None:
        assert lost == (0 if stratified else 3)


def test_sorted_prefix_form_and_device_tables_equal_pair_counting():
    """The kernel's formulation on the host: with the tables of ops.bootstrap_tables (torch, here on CPU tensors), a positive at sorted position
    s adds w (P[gstart - 1] + P[gend - 1]) over the inclusive scan P of the negatives' weights -- the integers of direct pair counting."""
    N, K, R = 130, 4, 6
    p, y, pred = br.case(N, K, 77, quarters=True)
    p[:, 2] = 0.25                                               # one column all equal
    w = br.multiplicities(3, R, y, K, False)
    _, want = br.counts(p, y, pred, w, K)
    assert np.array_equal(br.counts(p, y, pred, w, K, pairs=br.auc_counts_sorted)[1], want)
    t = {k: v.numpy() for k, v in ops.bootstrap_tables(torch.from_numpy(p), torch.from_numpy(y)).items()}
    rows, off = br.class_lists(y, K)
    assert np.array_equal(t["class_rows"], rows) and np.array_equal(t["class_off"], off)
    for c in range(K):
        order, gs, ge = t["order"][c], t["gstart"][c], t["gend"][c]
        v = p[order, c]
        assert np.array_equal(np.sort(order), np.arange(N)) and (np.diff(v) >= 0).all()
        assert np.array_equal(gs, np.searchsorted(v, v, "left")) and np.array_equal(ge, np.searchsorted(v, v, "right"))
        for b in range(R):
            ws, pos = w[b][order], y[order] == c
            P = np.concatenate([[0], np.cumsum(np.where(pos, 0, ws))])
            assert (ws * (P[gs] + P[ge]))[pos].sum() == want[b, c, 0]
    assert (want[:, 2, 0] == want[:, 2, 1] * want[:, 2, 2]).all()  # all ties: 2 * greater + ties = n_pos n_neg, AUC exactly 0.5


def test_the_three_table_builders_group_the_rows_by_label_alike():
    """class_rows / class_off of bootstrap_tables and selective_tables, and the Mondrian seg_off of conformal_tables, for labels with an
    empty class: the stratified draw and the Mondrian segments read the same groups."""
    y = torch.tensor([2, 0, 2, 2, 0, 2, 0, 2])                     # class sizes [3, 0, 5]
    p = torch.softmax(torch.from_numpy(np.random.default_rng(5).standard_normal((8, 3)).astype(np.float32)), 1)
    boot, sel = ops.bootstrap_tables(p, y), ops.selective_tables(p.max(1).values, y)
    conf = ops.conformal_tables((1.0 - p).t().contiguous(), y, mondrian=True)
    assert boot["class_rows"].tolist() == [1, 4, 6, 0, 2, 3, 5, 7] and boot["class_off"].tolist() == [0, 3, 3, 8]
    for t in (boot["class_rows"], boot["class_off"], conf["seg_off"]):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert torch.equal(sel["class_rows"], boot["class_rows"]) and torch.equal(sel["class_off"], boot["class_off"])
    assert torch.equal(conf["seg_off"], boot["class_off"])


def test_tie_groups_of_an_all_tied_row_and_of_a_row_without_ties():
    vals = torch.tensor([[0.5] * 7, [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6]])
    gstart, gend = ops._tie_groups(vals)
    assert gstart.tolist() == [[0] * 7, [0, 1, 2, 3, 4, 5, 6]]
    assert gend.tolist() == [[7] * 7, [1, 2, 3, 4, 5, 6, 7]]
    gs1, ge1 = ops._tie_groups(torch.tensor([3.0, 3.0, 2.0, 1.0, 1.0, 1.0, 0.0]))      # one dimension, descending, as selective_tables sorts
    assert gs1.tolist() == [0, 0, 2, 3, 3, 3, 6] and ge1.tolist() == [2, 2, 3, 6, 6, 6, 7]


def test_kappa_batch_restates_kappa_quadratic():
    g = np.random.default_rng(0)
    conf = g.integers(0, 6, (40, 5, 5))
    conf[:10, 2, :] = 0
    conf[:10, :, 2] = 0                                          # a class absent from labels and predictions: squeezed out
    conf[10:14, 1:, :] = 0
    conf[10:14, :, 1:] = 0                                       # one class left: 0 / 0
    conf[14] = 0                                                 # an empty matrix
    got = metrics.kappa_quadratic_batch(conf)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = np.array([metrics.kappa_quadratic(c) for c in conf])
    assert np.isnan(want[10:15]).all() and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) < TOL


def test_paired_p_value_formula():
    assert metrics.paired_p_value(np.full(9, 0.25)) == pytest.approx(2 * (0 + 1) / 10)        # all positive
    assert metrics.paired_p_value(-np.full(9, 0.25)) == pytest.approx(2 * (0 + 1) / 10)
    assert metrics.paired_p_value(np.zeros(9)) == 1.0                                          # all zero: both tails hold everything
    d = np.array([0.5, -0.25, np.nan, 0.0, 0.125, np.nan, 0.75, 1.0])                         # R_def = 6: #{<= 0} = 2, #{>= 0} = 5
    assert metrics.paired_p_value(d) == pytest.approx(min(1.0, 2 * min(3 / 7, 6 / 7)))
    assert metrics.paired_p_value(np.array([np.nan, np.nan])) == 1.0                           # nothing defined: no evidence


def test_classification_report_with_an_empty_row_and_an_empty_column():
    #          predicted 0  1  2  3
    conf = np.array([[5, 1, 0, 0],                               # class 2 is never predicted (empty column)
                     [2, 6, 0, 1],
                     [1, 3, 0, 0],
                     [0, 0, 0, 0]])                              # class 3 never occurs in the labels (empty row), but is predicted once
    r = metrics.classification_report(conf)
    assert r["support"].tolist() == [6, 9, 4, 0]
    np.testing.assert_allclose(r["recall"], [5 / 6, 6 / 9, 0.0, 0.0], rtol=0, atol=TOL)
    np.testing.assert_allclose(r["precision"], [5 / 8, 6 / 10, 0.0, 0.0], rtol=0, atol=TOL)
    np.testing.assert_allclose(r["specificity"], [10 / 13, 6 / 10, 15 / 15, 18 / 19], rtol=0, atol=TOL)
    f1 = [2 * 5 / (2 * 5 + 3 + 1), 2 * 6 / (2 * 6 + 4 + 3), 0.0, 0.0]
    np.testing.assert_allclose(r["f1"], f1, rtol=0, atol=TOL)
    assert abs(r["balanced_accuracy"] - (5 / 6 + 6 / 9 + 0.0) / 3) < TOL           # classes in the labels: 0, 1, 2
    assert abs(r["macro_f1"] - sum(f1) / 4) < TOL                                   # classes in labels or predictions: all four
    y = np.repeat(np.arange(4), conf.sum(1))
    pred = np.concatenate([np.repeat(np.arange(4), row) for row in conf])
    want = _sklearn_metrics(y, pred, None, 0)
    assert abs(r["balanced_accuracy"] - want["balanced_accuracy"]) < TOL and abs(r["macro_f1"] - want["macro_f1"]) < TOL
    from sklearn.metrics import precision_recall_fscore_support
    ps, rs, fs, _ = precision_recall_fscore_support(y, pred, labels=[0, 1, 2, 3], zero_division=0)
    for k, v in (("precision", ps), ("recall", rs), ("f1", fs)):
        np.testing.assert_allclose(r[k], v, rtol=0, atol=TOL)
    with pytest.raises(ValueError):
        metrics.classification_report(np.zeros((3, 4)))


def test_bootstrap_stderr_of_accuracy_is_the_binomial_one():
    """Statistical sanity of the resampling rule itself (host restatement only): N = 300, R = 512, accuracy 0.73 -- the bootstrap standard
    error of the accuracy within a factor 1.5 either way of sqrt(a (1 - a) / N).  Seed fixed after a look at seeds 0..7 on the host (ratios 0.93 to 1.05 over both rules)."""
    N, K, R = 300, 5, 512
    p, y, pred = br.case(N, K, 300)
    a = (pred == y).mean()
    assert 0.6 < a < 0.8
    for stratified in (False, True):
        w = br.multiplicities(3, R, y, K, stratified)
        acc = (w * (pred == y)[None, :]).sum(1) / N
        se, want = np.std(acc, ddof=1), np.sqrt(a * (1 - a) / N)
        print(f"stratified={stratified}: bootstrap stderr {se:.5f}, binomial {want:.5f}, ratio {se / want:.3f}")
        assert want / 1.5 < se < want * 1.5
        assert abs(acc.mean() - a) < 3 * want / np.sqrt(R) + 1e-3


def test_no_cpu_path_and_bad_arguments():
    from gaviko_amd.lib import GavikoHipError
    p, y, _ = br.case(40, 3, 1)
    with pytest.raises(GavikoHipError):
        metrics.bootstrap(torch.from_numpy(p), torch.from_numpy(y))
    with pytest.raises(GavikoHipError):
        metrics.compare(torch.from_numpy(p), torch.from_numpy(p[:, :2].copy()), torch.from_numpy(y))
