"""-m gpu: the kernels of csrc/features.hip (gvk_token_pool, gvk_l2_normalize_rows, gvk_feature_topk, gvk_knn_vote, gvk_class_means)
through their ops wrappers, against the float64 restatements of tests/test_features_golden.py.  Bounds are worst cases of the fp32
arithmetic at the shapes used, derived, not measured."""
import numpy as np
import pytest
import torch

from gaviko_amd import features, ops
from gaviko_amd.lib import GavikoHipError

U = 2.0 ** -24                                  # fp32 unit round-off


def integer_case(Nq, Ng, C, seed):
    """Values in -3..3: every product, partial sum and norm is an exact fp32 integer."""
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, (Nq, C)).astype(np.float32), rng.integers(-3, 4, (Ng, C)).astype(np.float32)


def dev_t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


# ------------------------------------------------------------------ token_pool
POOL_SHAPES = [(2, 41, 192, 9, 32), (1, 1001, 768, 1, 1000), (3, 7, 64, 0, 1), (2, 10, 1024, 3, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,C,r0,R", POOL_SHAPES)
def test_token_pool_against_float64(dev, B, T, C, r0, R):
    """|error| <= R * 2^-24 * mean_r |x| per element: (R - 1) u sum|x| / R for the sum in any order plus one rounding of the division."""
    rng = np.random.default_rng(B * 1000 + T)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    g = dev_t(x, dev)
    out = ops.token_pool(g, B, T, C, r0, R)
    rows = x[:, r0:r0 + R].astype(np.float64)
    err = np.abs(out.double().cpu().numpy() - rows.mean(1))
    bound = R * U * np.abs(rows).mean(1)
    print(f"token_pool {B, T, C, r0, R}: worst error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    if R == 1:
        assert torch.equal(out, g[:, r0])
    assert torch.equal(ops.token_pool(g, B, T, C, r0, R), out)
    into = torch.full((B, C), 7.0, device=dev)
    assert ops.token_pool(g, B, T, C, r0, R, out=into) is into and torch.equal(into, out)


@pytest.mark.gpu
def test_token_pool_does_not_depend_on_the_batch(dev):
    x = torch.randn((3, 41, 192), device=dev)
    full = ops.token_pool(x, 3, 41, 192, 9, 32)
    for b in range(3):
        assert torch.equal(ops.token_pool(x[b].contiguous(), 1, 41, 192, 9, 32)[0], full[b])


# ------------------------------------------------------------------ feature_topk
TOPK_SHAPES = [(37, 533, 1024, 10), (1, 33, 64, 32), (16, 1000, 192, 1), (5, 70, 768, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("Nq,Ng,C,k", TOPK_SHAPES)
def test_feature_topk_integer_inputs_exact(dev, Nq, Ng, C, k, metric):
    from test_features_golden import topk64
    q, g = integer_case(Nq, Ng, C, 0)
    idx, score = ops.feature_topk(dev_t(q, dev), dev_t(g, dev), k, metric)
    want_i, want_s = topk64(q, g, k, metric)
    assert idx.dtype == torch.int32 and score.dtype == torch.float32 and tuple(idx.shape) == (Nq, k)
    assert np.array_equal(idx.cpu().numpy(), want_i), (metric, np.argwhere(idx.cpu().numpy() != want_i)[:5])
    assert np.array_equal(score.double().cpu().numpy(), want_s)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_feature_topk_exclude_and_slab_count(dev, metric):
    from test_features_golden import topk64
    _, g = integer_case(1, 97, 64, 3)
    gd = dev_t(g, dev)
    ar = torch.arange(97, dtype=torch.int32, device=dev)
    idx, score = ops.feature_topk(gd, gd, 9, metric, exclude=ar)
    want_i, want_s = topk64(g, g, 9, metric, exclude=np.arange(97))
    got = idx.cpu().numpy()
    assert not (got == np.arange(97)[:, None]).any()
    assert np.array_equal(got, want_i) and np.array_equal(score.double().cpu().numpy(), want_s)
    none = torch.full((97,), -1, dtype=torch.int32, device=dev)
    a, b = ops.feature_topk(gd, gd, 9, metric, exclude=none), ops.feature_topk(gd, gd, 9, metric)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    q, g = integer_case(37, 533, 1024, 0)
    qd, gd = dev_t(q, dev), dev_t(g, dev)
    one = ops.feature_topk(qd, gd, 10, metric, slabs=1)
    dflt = ops.feature_topk(qd, gd, 10, metric)
    many = ops.feature_topk(qd, gd, 10, metric, slabs=34)
    from gaviko_amd import lib
    assert lib.load().gvk_feature_topk_slabs(37, 533, 0) > 1 and lib.load().gvk_feature_topk_slabs(37, 533, 1) == 1
    for r in (dflt, many):
        assert torch.equal(r[0], one[0]) and torch.equal(r[1], one[1])


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_feature_topk_gaussian_inputs(dev, metric):
    """Every returned score within C * 2^-24 * (|q| . |g|) of the float64 score of the returned index (the worst case of a C-term fp32 dot
    product; three times that for 'l2', which adds the two norms and doubles the product), and the index at rank j equal to topk64's
    wherever the float64 gaps to ranks j - 1 and j + 1 both exceed twice the bound.  At least 95 % of the entries must be compared."""
    from test_features_golden import scores64, topk64
    Nq, Ng, C, k = 37, 533, 192, 10
    rng = np.random.default_rng(0)
    q32, g32 = rng.standard_normal((Nq, C)).astype(np.float32), rng.standard_normal((Ng, C)).astype(np.float32)
    qd, gd = dev_t(q32, dev), dev_t(g32, dev)
    if metric == "ip":
        qd, gd = ops.l2_normalize_rows(qd), ops.l2_normalize_rows(gd)
    q, g = qd.cpu().numpy(), gd.cpu().numpy()
    idx, score = ops.feature_topk(qd, gd, k, metric)
    idx, score = idx.cpu().numpy().astype(np.int64), score.double().cpu().numpy()
    s64 = scores64(q, g, metric)
    bound = C * U * (np.abs(q).astype(np.float64) @ np.abs(g).astype(np.float64).T) * (3.0 if metric == "l2" else 1.0)
    b_at = np.take_along_axis(bound, idx, 1)
    err = np.abs(score - np.take_along_axis(s64, idx, 1))
    print(f"feature_topk gaussian {metric}: worst score error {err.max():.3e}, bound {b_at.max():.3e}, worst error / bound {(err / b_at).max():.3f}")
    assert (err <= b_at).all()
    want_i, want_s = topk64(q, g, k + 1, metric)
    gap_hi = np.abs(np.diff(want_s, axis=1))                                      # [Nq, k]: rank j to j + 1
    gap_lo = np.concatenate([np.full((Nq, 1), np.inf), gap_hi[:, :-1]], 1)        # rank j - 1 to j
    clear = (gap_hi > 2 * bound.max()) & (gap_lo > 2 * bound.max())
    frac = clear.mean()
    print(f"feature_topk gaussian {metric}: {frac * 100:.1f} % of the {Nq * k} entries are clear of twice the bound")
    assert frac >= 0.95
    assert np.array_equal(idx[clear], want_i[:, :k][clear])


# ------------------------------------------------------------------ l2_normalize_rows
@pytest.mark.gpu
@pytest.mark.parametrize("N,C", [(37, 192), (5, 768), (3, 70)])
def test_l2_normalize_rows(dev, N, C):
    x = np.random.default_rng(N).standard_normal((N, C)).astype(np.float32)
    x[1] = 0.0
    xd = dev_t(x, dev)
    norm = torch.empty(N, device=dev)
    y = ops.l2_normalize_rows(xd, norm=norm)
    n64 = np.linalg.norm(x.astype(np.float64), axis=1)
    assert (np.abs(norm.double().cpu().numpy() - n64) <= C * U * n64).all()
    assert torch.equal(y[1], torch.zeros(C, device=dev)) and float(norm[1]) == 0.0
    live = n64 > 0
    want = x[live].astype(np.float64) / n64[live, None]
    assert np.abs(y.double().cpu().numpy()[live] - want).max() <= (C + 2) * U
    z = xd.clone()
    assert ops.l2_normalize_rows(z, out=z) is z and torch.equal(z, y)


# ------------------------------------------------------------------ knn_vote
@pytest.mark.gpu
def test_knn_vote_uniform_exact(dev):
    from test_features_golden import vote64
    rng = np.random.default_rng(5)
    Nq, Ng, k, K = 41, 200, 5, 7
    labels = rng.integers(0, K, Ng)
    idx = np.stack([rng.permutation(Ng)[:k] for _ in range(Nq)])
    labels[[10, 11]], labels[[12, 13]], labels[14] = 4, 2, 0                      # a 2-2-1 vote: the lower class wins
    idx[0] = [10, 12, 11, 13, 14]
    score = -np.sort(rng.random((Nq, k)), axis=1).astype(np.float32)
    probs, pred = ops.knn_vote(dev_t(idx, dev, torch.int32), dev_t(score, dev), dev_t(labels, dev, torch.int32), K, "uniform")
    want_p, want_c = vote64(idx, score, labels, K, "uniform")
    assert np.array_equal(probs.cpu().numpy(), want_p.astype(np.float32))
    assert np.array_equal(pred.cpu().numpy(), want_c) and int(pred[0]) == 2 and probs[0].tolist() == pytest.approx([0.2, 0, 0.4, 0, 0.4, 0, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("k,T", [(5, 0.07), (20, 0.07), (32, 1.0)])
def test_knn_vote_softmax_weights(dev, k, T):
    """Within k * 2^-23 relative of float64, element by element; pred equal wherever float64's two best classes differ by more than that."""
    from test_features_golden import vote64
    rng = np.random.default_rng(k)
    Nq, Ng, K = 53, 300, 5
    labels = rng.integers(0, K, Ng)
    idx = np.stack([rng.permutation(Ng)[:k] for _ in range(Nq)])
    score = (-np.sort(rng.random((Nq, k)), axis=1)).astype(np.float32)            # similarities, best first
    probs, pred = ops.knn_vote(dev_t(idx, dev, torch.int32), dev_t(score, dev), dev_t(labels, dev, torch.int32), K, "softmax", T)
    want_p, want_c = vote64(idx, score, labels, K, "softmax", T)
    got = probs.double().cpu().numpy()
    tol = k * 2.0 ** -23
    rel = np.abs(got - want_p) / np.where(want_p > 0, want_p, 1.0)
    print(f"knn_vote softmax k={k} T={T}: worst relative error {rel.max():.3e} (bound {tol:.3e})")
    assert (rel <= tol).all() and (got[want_p == 0] == 0).all()
    top2 = np.sort(want_p, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > tol
    assert clear.mean() > 0.9 and np.array_equal(pred.cpu().numpy()[clear], want_c[clear])


# ------------------------------------------------------------------ class_means
@pytest.mark.gpu
@pytest.mark.parametrize("N,K,C", [(257, 5, 64), (257, 5, 768), (40, 3, 64), (40, 3, 768)])
def test_class_means(dev, N, K, C):
    from test_features_golden import class_means64
    rng = np.random.default_rng(N + C)
    x = rng.standard_normal((N, C)).astype(np.float32)
    labels = rng.integers(0, K, N)
    if N == 40:
        labels[labels == 1] = 2                                                   # class 1 is empty
    xd, ld = dev_t(x, dev), dev_t(labels, dev, torch.int32)
    mean, count = ops.class_means(xd, ld, K)
    want_m, want_c = class_means64(x, labels, K)
    assert np.array_equal(count.cpu().numpy(), want_c)
    for c in range(K):
        if want_c[c] == 0:
            assert torch.equal(mean[c], torch.zeros(C, device=dev))
        else:
            bound = want_c[c] * U * np.abs(x[labels == c].astype(np.float64)).mean(0)
            assert (np.abs(mean[c].double().cpu().numpy() - want_m[c]) <= bound).all(), c
    again = ops.class_means(xd, ld, K)
    assert torch.equal(again[0], mean) and torch.equal(again[1], count)
    p = features.prototypes(xd, labels, K)
    assert torch.equal(p.mean, mean) and torch.equal(p.count, count)


# ------------------------------------------------------------------ rejections
@pytest.mark.gpu
def test_rejections_leave_the_wrappers_usable(dev):
    q, g = torch.randn((4, 64), device=dev), torch.randn((33, 64), device=dev)

    def ok():
        idx, score = ops.feature_topk(q, g, 3)
        assert tuple(idx.shape) == (4, 3) and bool((score[:, :-1] >= score[:, 1:]).all())

    bad = [lambda: ops.feature_topk(q, g, 0), lambda: ops.feature_topk(q, g, 33), lambda: ops.feature_topk(q, g[:20], 21),
           lambda: ops.feature_topk(q, g, 33, exclude=torch.zeros(4, dtype=torch.int32, device=dev)),
           lambda: ops.feature_topk(torch.randn((4, 190), device=dev), torch.randn((33, 190), device=dev), 3),
           lambda: ops.feature_topk(torch.randn((4, 1028), device=dev), torch.randn((33, 1028), device=dev), 3),
           lambda: ops.feature_topk(q.cpu(), g, 3), lambda: ops.feature_topk(q, g.cpu(), 3),
           lambda: ops.feature_topk(torch.randn((4, 128), device=dev)[:, ::2], g, 3),
           lambda: ops.feature_topk(q, g, 3, metric="cosine"), lambda: ops.feature_topk(q, g, 3, slabs=0),
           # Nq * Ng = 2^31 by shape arithmetic alone: 2^16 x 2^15 rows of 4 columns, 1.5 MB in all
           lambda: ops.feature_topk(torch.zeros((1 << 16, 4), device=dev), torch.zeros((1 << 15, 4), device=dev), 1)]
    for i, f in enumerate(bad):
        with pytest.raises(GavikoHipError):
            f()
        ok()
    x = torch.randn((2, 9, 64), device=dev)
    for f in (lambda: ops.token_pool(x, 2, 9, 64, 3, 7), lambda: ops.token_pool(x, 2, 9, 64, 0, 0), lambda: ops.token_pool(x, 2, 9, 62, 0, 1),
              lambda: ops.token_pool(x.cpu(), 2, 9, 64, 0, 1), lambda: ops.token_pool(x, 3, 9, 64, 0, 1)):
        with pytest.raises(GavikoHipError):
            f()
        assert torch.equal(ops.token_pool(x, 2, 9, 64, 8, 1), x[:, 8])
    for f in (lambda: ops.l2_normalize_rows(q.cpu()), lambda: ops.l2_normalize_rows(q, eps=0.0), lambda: ops.l2_normalize_rows(q[:, ::2])):
        with pytest.raises(GavikoHipError):
            f()
        ops.l2_normalize_rows(q)
    labels = torch.arange(33, dtype=torch.int32, device=dev) % 3
    for f in (lambda: features.prototypes(g, labels + 1, 3),                      # a label = K
              lambda: features.prototypes(g, labels - 1, 3), lambda: features.prototypes(g.cpu(), labels, 3),
              lambda: features.knn_classify(q, g, labels + 1, 3, 3), lambda: features.knn_classify(q, g, labels, 3, 1),
              lambda: features.knn_classify(q, g, labels[:5], 3, 3), lambda: features.knn(q, g, 3, exclude_self=True),
              lambda: features.knn(q, g, 3, metric="cos"), lambda: ops.class_means(g, labels.long(), 3),
              lambda: ops.knn_vote(torch.zeros((4, 33), dtype=torch.int32, device=dev), torch.zeros((4, 33), device=dev), labels, 3)):
        with pytest.raises(GavikoHipError):
            f()
        assert int(features.prototypes(g, labels, 3).count.sum()) == 33
        assert tuple(features.knn_classify(q, g, labels, 3, 3).probs.shape) == (4, 3)
