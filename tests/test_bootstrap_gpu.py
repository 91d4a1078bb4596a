"""-m gpu: gvk_bootstrap_counts through gaviko_amd.metrics.bootstrap / compare.  The device's integers (confusion [R, K, K], auc_counts
[R, K, 3]) must EQUAL the host restatement of tests/bootstrap_ref.py: the multiplicities rebuilt from (seed, replicate, draw) and direct
O(N^2) weighted pair counting.  Shapes: the smallest at which the kernel takes another path (a row past the 256-thread block, the scan carry
across four waves, a second 1024-entry scan tile, an all-tied column, the documented limit N = 8192)."""
import numpy as np
import pytest
import torch

import bootstrap_ref as br
from gaviko_amd import metrics, ops
from gaviko_amd.lib import GavikoHipError

pytestmark = pytest.mark.gpu

SIZES37 = [3, 5, 8, 9, 12]
SEED37 = 5            # the restatement loses a class in replicates 6, 10 and 42 of 64 with this seed (seeds 1..7 looked at on the host)


def _run(dev, p, y, R, seed, stratified, **kw):
    return metrics.bootstrap(torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev), replicates=R, seed=seed, stratified=stratified, **kw)


def _check_exact(dev, p, y, pred, K, R, seed, stratified, pairs=br.auc_counts_pairs):
    r = _run(dev, p, y, R, seed, stratified)
    w = br.multiplicities(seed, R, y, K, stratified)
    conf, cnt = br.counts(p, y, pred, w, K, pairs=pairs)
    assert r.confusion.dtype == np.int64 and r.confusion.shape == (R, K, K) and r.auc_counts.dtype == np.int64 and r.auc_counts.shape == (R, K, 3)
    assert np.array_equal(r.confusion, conf), np.argwhere(r.confusion != conf)[:5]
    assert np.array_equal(r.auc_counts, cnt), np.argwhere(r.auc_counts != cnt)[:5]
    return r, conf, cnt


def test_small_unbalanced_set_with_ties_and_lost_classes(dev):
    K, R = 5, 64
    p, y, pred = br.case(37, K, 37, sizes=SIZES37, quarters=True)
    assert min(len(np.unique(p[:, c])) for c in range(K)) < 37                       # the columns do tie
    w = br.multiplicities(SEED37, R, y, K, False)
    lost = np.array([any(w[b][y == c].sum() == 0 for c in range(K)) for b in range(R)])
    assert 0 < lost.sum() <= R // 4
    r, conf, cnt = _check_exact(dev, p, y, pred, K, R, SEED37, False)
    assert np.array_equal(np.isnan(r.replicates["auc"]), lost) and r.undefined["auc"] == int(lost.sum())
    for k in metrics.BOOTSTRAP_METRICS:
        if k != "auc":
            assert np.isfinite(r.replicates[k]).all() and r.undefined[k] == 0, k
    want = metrics.metrics_from_counts(conf, cnt)
    for k in metrics.BOOTSTRAP_METRICS:
        assert np.array_equal(r.replicates[k], want[k], equal_nan=True), k
    assert np.isfinite(r.ci["auc"]).all() and np.isfinite(r.stderr["auc"])           # the interval skips the NaN replicates
    rs, _, _ = _check_exact(dev, p, y, pred, K, R, SEED37, True)
    assert rs.undefined["auc"] == 0 and np.isfinite(rs.replicates["auc"]).all() and rs.stratified and not r.stratified
    assert (rs.confusion.sum(2) == np.array(SIZES37)[None, :]).all()                 # every class keeps its size


@pytest.mark.parametrize("N,K,R", [(257, 3, 8), (1025, 2, 4)], ids=["one_past_the_block", "second_scan_tile_k2"])
@pytest.mark.parametrize("stratified", [False, True], ids=["plain", "stratified"])
def test_counts_equal_pair_counting(dev, N, K, R, stratified):
    p, y, pred = br.case(N, K, N, quarters=True)
    _check_exact(dev, p, y, pred, K, R, 9, stratified)


def test_all_equal_column_has_auc_one_half(dev):
    N, K, R = 130, 2, 16
    p, y, pred = br.case(N, K, 130)
    p[:] = 0.5                                                                        # both columns constant: every pair is a tie
    pred = p.argmax(1).astype(np.int64)
    r, _, cnt = _check_exact(dev, p, y, pred, K, R, 2, False)
    assert (cnt[:, :, 0] == cnt[:, :, 1] * cnt[:, :, 2]).all()
    assert r.undefined["auc"] == 0 and (r.replicates["auc"] == 0.5).all() and r.point["auc"] == 0.5


def test_at_the_documented_limit_and_beyond_it(dev):
    """N = 8192 (8 scan tiles, 64 KB of LDS for the two arrays); the restatement uses the sorted prefix sums in numpy int64 here.  Over the
    limit and K = 1 are rejected by the argument checks, before any launch."""
    N, K, R = ops.BOOTSTRAP_MAX_ROWS, 2, 2
    assert N == 8192
    p, y, pred = br.case(N, K, 8192, quarters=True)
    _check_exact(dev, p, y, pred, K, R, 4, False, pairs=br.auc_counts_sorted)
    _check_exact(dev, p, y, pred, K, R, 4, True, pairs=br.auc_counts_sorted)
    big = torch.full((N + 1, K), 0.5, device=dev)
    with pytest.raises(GavikoHipError):
        metrics.bootstrap(big, torch.zeros(N + 1, dtype=torch.int64, device=dev), replicates=2)
    with pytest.raises(GavikoHipError):
        metrics.bootstrap(torch.ones((40, 1), device=dev), torch.zeros(40, dtype=torch.int64, device=dev), replicates=2)
    yb = torch.from_numpy(y[:64]).to(dev)
    pb = torch.from_numpy(p[:64]).to(dev)
    tables = ops.bootstrap_tables(pb, yb)
    with pytest.raises(GavikoHipError):                                               # the wrapper's own checks: a table of another length
        ops.bootstrap_counts(yb, torch.from_numpy(pred[:63].astype(np.int32)).to(dev), tables, 2, 0, False)
    with pytest.raises(GavikoHipError):
        ops.bootstrap_counts(yb, torch.from_numpy(pred[:64].astype(np.int32)).to(dev), tables, 0, 0, False)
    with pytest.raises(GavikoHipError):                                               # labels outside [0, K), as calibration rejects them
        metrics.bootstrap(pb, yb + 1, replicates=2)
    with pytest.raises(GavikoHipError):
        metrics.bootstrap(pb.cpu(), yb, replicates=2)


def test_many_replicates_do_not_restrict_the_launch(dev):
    """R = 65536 workgroups (past a 16-bit grid dimension) on a tiny set; the first, the last and a middle replicate against the host."""
    N, K, R = 20, 2, 65536
    p, y, pred = br.case(N, K, 20)
    r = _run(dev, p, y, R, 1, False)
    h = br.hash_u32(1, np.arange(R * N, dtype=np.uint64).reshape(R, N)).astype(np.uint64)
    j = ((h * np.uint64(N)) >> np.uint64(32)).astype(np.int64)
    for b in (0, 40000, R - 1):
        w = np.bincount(j[b], minlength=N)
        assert np.array_equal(r.confusion[b], br.confusion_weighted(y, pred, w, K)) and np.array_equal(r.auc_counts[b], br.auc_counts_pairs(p, y, w, K))
    assert (r.confusion.sum((1, 2)) == N).all()


def test_reproducible_and_seeded(dev):
    p, y, _ = br.case(257, 3, 257, quarters=True)
    a, b, c = _run(dev, p, y, 32, 7, False), _run(dev, p, y, 32, 7, False), _run(dev, p, y, 32, 8, False)
    assert np.array_equal(a.confusion, b.confusion) and np.array_equal(a.auc_counts, b.auc_counts)
    assert not np.array_equal(a.confusion, c.confusion) and not np.array_equal(a.auc_counts, c.auc_counts)
    assert a.seed == 7 and c.seed == 8 and a.level == 0.95
    pd, yd = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    same = metrics.compare(pd, pd, yd, replicates=32, seed=7)
    for k in metrics.BOOTSTRAP_METRICS:
        assert (same.delta[k] == 0).all() and same.p_value[k] == 1.0 and same.delta_point[k] == 0.0 and same.ci[k] == (0.0, 0.0), k


@pytest.mark.parametrize("stratified", [False, True], ids=["plain", "stratified"])
def test_compare_pairs_the_two_models(dev, stratified):
    K, R = 5, 64
    pa, y, _ = br.case(300, K, 300)
    pb = br.case(300, K, 301, signal=2.0)[0]                                          # another model: other scores, the labels of the first
    pad, pbd, yd = torch.from_numpy(pa).to(dev), torch.from_numpy(pb).to(dev), torch.from_numpy(y).to(dev)
    cmp_ = metrics.compare(pad, pbd, yd, replicates=R, seed=3, stratified=stratified, level=0.9)
    a = metrics.bootstrap(pad, yd, replicates=R, seed=3, stratified=stratified)
    b = metrics.bootstrap(pbd, yd, replicates=R, seed=3, stratified=stratified)
    assert np.array_equal(a.confusion.sum(2), b.confusion.sum(2))                     # the same multiplicities: the same label counts
    for k in metrics.BOOTSTRAP_METRICS:
        assert (cmp_.delta[k] == a.replicates[k] - b.replicates[k]).all(), k
        assert cmp_.delta_point[k] == a.point[k] - b.point[k]
        assert cmp_.p_value[k] == metrics.paired_p_value(cmp_.delta[k]) and 0.0 < cmp_.p_value[k] <= 1.0
        lo, hi = np.nanquantile(cmp_.delta[k], [0.05, 0.95])
        assert cmp_.ci[k] == (lo, hi)
    assert cmp_.level == 0.9 and cmp_.stratified == stratified and cmp_.seed == 3
    assert np.abs(cmp_.delta["accuracy"]).max() > 0


def test_point_estimates_intervals_and_the_evaluator(dev):
    N, K = 257, 5
    g = torch.Generator().manual_seed(5)
    y = torch.randint(0, K, (N,), generator=g)
    logits = torch.randn(N, K, generator=g) + 2.0 * torch.nn.functional.one_hot(y, K) * (torch.rand(N, 1, generator=g) > 0.4)
    logits[::9] = logits[4]
    ev = metrics.Evaluator(K, dev)
    for a in range(0, N, 64):
        ev.update(logits[a:a + 64].to(dev), y[a:a + 64].to(dev))
    plain = ev.compute()
    assert set(plain) == {"accuracy", "quadratic_kappa", "auc", "confusion", "y_pred", "y_pred_proba", "y_test", "calibration"}
    full = ev.compute(bootstrap=16, seed=2, stratified=True)
    assert set(full) == set(plain) | {"bootstrap", "report"}
    for k in ("accuracy", "quadratic_kappa", "auc"):
        assert full[k] == plain[k]
    bs = full["bootstrap"]
    assert isinstance(bs, metrics.BootstrapResult) and bs.confusion.shape == (16, K, K) and bs.seed == 2 and bs.stratified
    r = metrics.bootstrap(torch.from_numpy(plain["y_pred_proba"]).to(dev), y.to(dev), replicates=200, seed=1, level=0.9)
    for k in ("accuracy", "quadratic_kappa", "auc"):
        assert r.point[k] == plain[k] == bs.point[k], k
    rep = metrics.classification_report(plain["confusion"])
    assert r.point["balanced_accuracy"] == rep["balanced_accuracy"] and r.point["macro_f1"] == rep["macro_f1"]
    assert full["report"]["balanced_accuracy"] == rep["balanced_accuracy"] and np.array_equal(full["report"]["support"], plain["confusion"].sum(1))
    for k in metrics.BOOTSTRAP_METRICS:
        lo, hi = np.nanquantile(r.replicates[k], [0.05, 0.95])
        assert r.ci[k] == (lo, hi) and lo <= hi, k
        assert r.stderr[k] == np.nanstd(r.replicates[k], ddof=1) and r.stderr[k] > 0
        assert r.replicates[k].dtype == np.float64 and r.replicates[k].shape == (200,)
        assert lo - 3 * r.stderr[k] < r.point[k] < hi + 3 * r.stderr[k]                # the point estimate sits with its own resamples
