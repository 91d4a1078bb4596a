"""GPU: the evaluation kernels of csrc/metrics.hip (gvk_eval_rows, gvk_ovr_auc_counts) through ops.eval_rows / ops.ovr_auc_counts, and
metrics.Evaluator on top of them, against numpy in int64 and float64.

The reference is the definition: the float64 softmax of the float32 logits, the first-maximum argmax, np.bincount for the confusion matrix and,
per class, the brute-force pair count 2 #{p_i > p_j} + #{p_i == p_j} over positives i and negatives j on the float32 scores.  Every integer
output is compared with ==; the probabilities are held to 1e-6, the bound of test_eval_metrics_match_sklearn.

The inputs are built, not drawn: scores come from a set of four values so that most pairs tie, row j and row j + 1024 carry the same scores so
that ties straddle the kernel's 1024-row LDS tiles, and N walks over the 256-thread block and the 1024-row tile boundaries."""
import numpy as np
import pytest
import torch

from gaviko_amd import ops
from gaviko_amd.metrics import Evaluator, kappa_quadratic, macro_ovr_auc

pytestmark = pytest.mark.gpu

NS = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 3000]
KS = [1, 2, 5, 64]
PAD = 64                                                                   # sentinel elements on either side of an output view
VALS = np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32)


# ---- references ------------------------------------------------------------------------------------------------------------------------
def _ref_auc_counts(p, y):
    """int64 [K, 3]: {2 #{p_i > p_j} + #{p_i == p_j}, n_pos, n_neg} per class c over positives i (y_i == c) and negatives j, on float32"""
    N, K = p.shape
    out = np.zeros((K, 3), dtype=np.int64)
    for c in range(K):
        pos, neg = p[y == c, c], p[y != c, c]
        gt = int((pos[:, None] > neg[None, :]).sum())
        eq = int((pos[:, None] == neg[None, :]).sum())
        out[c] = (2 * gt + eq, pos.size, neg.size)
    return out


def _ref_rows(x, y):
    """(float64 softmax [N, K], first-maximum argmax [N], int64 confusion [K, K] over the rows whose label is a class)"""
    N, K = x.shape
    x64 = x.astype(np.float64)
    m = x64.max(1, keepdims=True)
    e = np.exp(x64 - m)
    pred = np.argmax(x, axis=1)                                            # numpy: the first maximum
    ok = (y >= 0) & (y < K)
    conf = np.bincount(y[ok] * K + pred[ok], minlength=K * K).astype(np.int64).reshape(K, K)
    return e / e.sum(1, keepdims=True), pred, conf


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def _auc_case(N, K):
    """scores from VALS with period 1024 in the row index (row j and row j + 1024 tie in every column), labels that differ between the two,
    and the last column constant when K >= 2"""
    j = np.arange(N)
    r = j % 1024
    k = np.arange(K)
    p = VALS[(r[:, None] * 7 + r[:, None] // 5 + 3 * k[None, :]) % 4]
    if K >= 2:
        p[:, K - 1] = 0.5
    y = ((j * 5 + j // 1024 + j // 7) % K).astype(np.int64)
    return np.ascontiguousarray(p), y


def _rows_case(N, K):
    """logits whose rows cycle through: random, duplicated maximum, all equal, shifted by +1e4 and by -1e4, a spread of 200, some -inf, random;
    labels mostly classes, with -100, -1, K and 2^32 + 1 among them"""
    rng = np.random.default_rng(1000 * N + K)
    x = (rng.standard_normal((N, K)) * 3).astype(np.float32)
    i = np.arange(N)
    kind = i % 8
    if K >= 2:
        for r in i[kind == 1]:                                             # the maximum twice: positions a < b, the prediction is a
            a, b = sorted(rng.choice(K, 2, replace=False))
            x[r, a] = x[r, b] = np.float32(x[r].max() + 1)
    x[kind == 2] = x[kind == 2][:, :1]                                     # all equal: the prediction is 0
    x[kind == 3] += np.float32(1e4)
    x[kind == 4] -= np.float32(1e4)
    for r in i[kind == 5]:                                                 # exp(-200) is 0 in float32
        x[r] = np.float32(-100) + x[r] / 8
        x[r, r % K] += np.float32(200)
    if K >= 2:
        for r in i[kind == 6]:                                             # some, not all: even or odd columns
            x[r, (r // 8) % 2::2] = -np.inf
    y = ((i * 3 + i // 5) % K).astype(np.int64)
    y[i % 11 == 3], y[i % 11 == 5], y[i % 11 == 7], y[i % 11 == 9] = -100, -1, K, 2 ** 32 + 1
    return x, y


def _view(dev, n, dtype, fill):
    """an n-element view into the middle of a larger buffer filled with `fill`"""
    big = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
    return big, big[PAD:PAD + n]


def _sentinels_intact(big, fill):
    return bool((big[:PAD] == fill).all()) and bool((big[-PAD:] == fill).all())


# ---- gvk_ovr_auc_counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_auc_counts_with_ties_across_the_lds_tiles(dev, N, K):
    p, y = _auc_case(N, K)
    want = _ref_auc_counts(p, y)
    if N > 1024:                                                           # the case is what it claims: equal scores 1024 rows apart
        assert np.array_equal(p[:N - 1024], p[1024:])
        assert K == 1 or (y[:N - 1024] != y[1024:]).any()
    big, counts = _view(dev, 3 * K, torch.int64, -7)
    counts.zero_()
    ops.ovr_auc_counts(torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev), counts)
    got = counts.cpu().numpy().reshape(K, 3)
    assert np.array_equal(got, want), f"N={N} K={K}\n{got}\n{want}"
    assert _sentinels_intact(big, -7)
    assert (got[:, 1] + got[:, 2] == N).all()
    if K >= 2 and want[K - 1, 1] > 0 and want[K - 1, 2] > 0:               # the constant column: every pair ties, the AUC is exactly 1/2
        assert got[K - 1, 0] == got[K - 1, 1] * got[K - 1, 2]
        assert got[K - 1, 0] / (2.0 * got[K - 1, 1] * got[K - 1, 2]) == 0.5
    if (want[:, 1] > 0).all() and (want[:, 2] > 0).all():
        assert macro_ovr_auc(got) == float((want[:, 0] / (2.0 * want[:, 1] * want[:, 2])).mean())


def test_auc_counts_add_to_the_buffer(dev):
    """the kernel adds: a second call on the same buffer doubles it, and whatever the buffer held before stays in it -- the caller zeroes it"""
    p, y = _auc_case(1025, 5)
    want = _ref_auc_counts(p, y).reshape(-1)
    pd, yd = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    counts = torch.zeros(15, dtype=torch.int64, device=dev)
    ops.ovr_auc_counts(pd, yd, counts)
    ops.ovr_auc_counts(pd, yd, counts)
    assert np.array_equal(counts.cpu().numpy(), 2 * want)
    start = torch.arange(15, dtype=torch.int64, device=dev) * 1000
    counts = start.clone()
    ops.ovr_auc_counts(pd, yd, counts)
    assert np.array_equal(counts.cpu().numpy(), start.cpu().numpy() + want)


def test_auc_counts_reject_a_wrong_target(dev):
    p = torch.zeros(8, 3, device=dev)
    counts = torch.zeros(9, dtype=torch.int64, device=dev)
    for bad in (torch.zeros(8, dtype=torch.int32, device=dev), torch.zeros(7, dtype=torch.int64, device=dev),
                torch.zeros(16, dtype=torch.int64, device=dev)[::2]):
        with pytest.raises(ValueError):
            ops.ovr_auc_counts(p, bad, counts)
    assert not counts.any()


@pytest.mark.parametrize("name", ["no_positive", "one_class", "all_one_label"])
def test_auc_of_a_class_without_positives_or_negatives(dev, name):
    """the counts are the reference's; macro_ovr_auc raises for them as sklearn does, and Evaluator reports auc = None"""
    N = 300
    j = np.arange(N)
    K, y = {"no_positive": (5, np.array([0, 1, 2, 4])[j % 4]),            # class 3 has no positive row
            "one_class": (1, np.zeros(N, dtype=np.int64)),                 # K = 1: the class has no negative row
            "all_one_label": (2, np.zeros(N, dtype=np.int64))}[name]      # class 0 has no negative row, class 1 no positive one
    y = y.astype(np.int64)
    p = VALS[(j[:, None] * 3 + j[:, None] // 4 + np.arange(K)[None, :]) % 4]
    want = _ref_auc_counts(p, y)
    assert (want[:, 1] == 0).any() or (want[:, 2] == 0).any()
    counts = torch.zeros(3 * K, dtype=torch.int64, device=dev)
    ops.ovr_auc_counts(torch.from_numpy(np.ascontiguousarray(p)).to(dev), torch.from_numpy(y).to(dev), counts)
    got = counts.cpu().numpy().reshape(K, 3)
    assert np.array_equal(got, want)
    assert (got[(got[:, 1] == 0) | (got[:, 2] == 0), 0] == 0).all()        # no pair, no count
    with pytest.raises(ValueError):
        macro_ovr_auc(got)
    if K >= 2:
        ev = Evaluator(K, dev)
        ev.update(torch.from_numpy(np.ascontiguousarray(p)).to(dev), torch.from_numpy(y).to(dev))
        r = ev.compute()
        assert r["auc"] is None
        assert np.array_equal(r["confusion"], _ref_rows(p, y)[2])


# ---- gvk_eval_rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_eval_rows_against_numpy(dev, N, K):
    x, y = _rows_case(N, K)
    proba, pred, conf = _ref_rows(x, y)
    kind = np.arange(N) % 8
    if K >= 2 and N >= 8:                                                  # the case is what it claims
        assert ((x[kind == 1] == x[kind == 1].max(1, keepdims=True)).sum(1) == 2).all()
        assert (pred[kind == 2] == 0).all() and (proba[kind == 2] == 1.0 / K).all()
        assert np.isinf(x[kind == 6]).any(1).all() and not np.isinf(x[kind == 6]).all(1).any()
    bp, vp = _view(dev, N * K, torch.float32, 7.0)
    bi, vi = _view(dev, N, torch.int32, -7)
    bc, vc = _view(dev, K * K, torch.int64, -7)
    vc.zero_()
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    ops.eval_rows(xd, yd, vp.view(N, K), vi, vc)
    got_p, got_i = vp.cpu().numpy().reshape(N, K), vi.cpu().numpy()
    assert np.array_equal(got_i, pred)
    assert np.array_equal(vc.cpu().numpy().reshape(K, K), conf)
    assert conf.sum() == int(((y >= 0) & (y < K)).sum())
    err = np.abs(got_p.astype(np.float64) - proba).max()
    print(f"eval_rows N={N} K={K}: proba err {err:.2e} (bound 1e-06)")
    assert err < 1e-6
    assert (got_p[np.isinf(x)] == 0).all()                                 # -inf: probability exactly 0
    assert np.isfinite(got_p).all()
    ops.eval_rows(xd, yd, vp.view(N, K), vi, vc)                           # the confusion matrix accumulates, the rest is written again
    assert np.array_equal(vc.cpu().numpy().reshape(K, K), 2 * conf)
    assert np.array_equal(vp.cpu().numpy().reshape(N, K), got_p) and np.array_equal(vi.cpu().numpy(), got_i)
    assert _sentinels_intact(bp, 7.0) and _sentinels_intact(bi, -7) and _sentinels_intact(bc, -7)


# ---- Evaluator -------------------------------------------------------------------------------------------------------------------------
def test_evaluator_does_not_depend_on_the_batching(dev):
    N, K = 1100, 5
    x, y = _rows_case(N, K)
    y = np.where((y >= 0) & (y < K), y, (np.arange(N) * 3) % K).astype(np.int64)      # labels that are classes: calibration takes them
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    results = []
    for step in (N, 1, 64, 1000):
        ev = Evaluator(K, dev)
        for a in range(0, N, step):
            ev.update(xd[a:a + step], yd[a:a + step])
        results.append(ev.compute())
    proba, pred, conf = _ref_rows(x, y)
    first = results[0]
    assert np.array_equal(first["confusion"], conf) and np.array_equal(first["y_pred"], pred)
    assert first["accuracy"] == float(np.trace(conf)) / N
    want_auc = _ref_auc_counts(first["y_pred_proba"], y)
    assert first["auc"] == float((want_auc[:, 0] / (2.0 * want_auc[:, 1] * want_auc[:, 2])).mean())
    for r in results[1:]:
        assert np.array_equal(r["confusion"], first["confusion"]) and np.array_equal(r["y_pred"], first["y_pred"])
        assert np.array_equal(r["y_test"], first["y_test"])
        assert np.array_equal(r["y_pred_proba"].view(np.uint32), first["y_pred_proba"].view(np.uint32))
        for key in ("accuracy", "quadratic_kappa", "auc"):
            assert r[key] == first[key]


def test_kappa_with_a_class_absent_from_labels_and_predictions(dev):
    from sklearn.metrics import cohen_kappa_score
    N, K = 500, 5
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((N, K)) * 2).astype(np.float32)
    x[:, 3] = -50.0                                                        # never predicted ...
    y = np.array([0, 1, 2, 4])[rng.integers(0, 4, N)].astype(np.int64)     # ... and never a label
    x[np.arange(N), y] += (rng.random(N) > 0.5) * 2.0
    ev = Evaluator(K, dev)
    ev.update(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    r = ev.compute()
    pred = np.argmax(x, 1)
    assert np.array_equal(r["y_pred"], pred) and not (pred == 3).any()
    assert r["confusion"][3].sum() == 0 and r["confusion"][:, 3].sum() == 0
    want = cohen_kappa_score(y, pred, weights="quadratic")
    assert abs(r["quadratic_kappa"] - want) < 1e-12
    assert abs(kappa_quadratic(_ref_rows(x, y)[2]) - want) < 1e-12
    assert r["auc"] is None                                                # class 3 has no positive row
