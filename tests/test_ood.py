"""CPU: the float64 reference of the out-of-distribution scores (tests/ood_ref.py) and the host side of gaviko_amd.ood against independent
code (sklearn.covariance, scipy), and the argument validation of every public function, which raises before anything touches a device."""
import numpy as np
import pytest
import torch

import ood_ref
from gaviko_amd import ood, ops
from gaviko_amd.lib import GavikoHipError


def class_rows(N, C, K, seed):
    """Gaussian rows with a per-class offset of 10 and correlated columns, labels, class means (fp32), class-centred rows (float64)."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, K, N)
    mix = rng.standard_normal((C, C)) / np.sqrt(C) + np.eye(C)
    x = (rng.standard_normal((N, C)) @ mix + 10.0 * lab[:, None]).astype(np.float32)
    mean = np.stack([x[lab == k].astype(np.float64).mean(0) if (lab == k).any() else np.zeros(C) for k in range(K)]).astype(np.float32)
    d, _ = ood_ref.centred(x, lab, mean)
    return x, lab, mean, d


@pytest.mark.parametrize("N,C", [(24, 40), (40, 40), (200, 40)])
def test_ledoit_wolf_matches_sklearn(N, C):
    from sklearn.covariance import ledoit_wolf_shrinkage
    x, lab, mean, d = class_rows(N, C, 3, N)
    S, r4, count = ood_ref.scatter(x, lab, mean)
    assert count.sum() == N and np.array_equal(S, S.T)
    want = ledoit_wolf_shrinkage(d, assume_centered=True)
    assert 0.0 < want < 1.0
    for got in (ood_ref.ledoit_wolf(S, r4, N), ood.ledoit_wolf_shrinkage(S, r4, N)):
        assert abs(got - want) <= 1e-10 * want, (got, want)


def test_ledoit_wolf_degenerate_inputs():
    S = 3.0 * np.eye(8) * 10                                    # Sigma = mu I: delta = 0
    assert ood_ref.ledoit_wolf(S, 1.0, 10) == 0.0 and ood.ledoit_wolf_shrinkage(S, 1.0, 10) == 0.0


@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0, "ledoit_wolf"])
def test_shrunk_covariance_and_whitening(lam):
    from sklearn.covariance import shrunk_covariance
    N, C = 90, 32
    x, lab, mean, d = class_rows(N, C, 3, 5)
    S, r4, _ = ood_ref.scatter(x, lab, mean)
    l = ood_ref.ledoit_wolf(S, r4, N) if lam == "ledoit_wolf" else lam
    cov_l = ood_ref.shrunk(S, N, l)
    np.testing.assert_allclose(cov_l, shrunk_covariance(d.T @ d / N, shrinkage=l), rtol=1e-12, atol=1e-12)
    W_ref = ood_ref.whitening(cov_l)
    W, got_l = ood.whitening_from_scatter(S, r4, N, lam)
    assert abs(got_l - l) <= 1e-12 * max(l, 1e-300) and np.allclose(np.triu(W, 1), 0.0)
    for w in (W_ref, W):
        assert np.abs(w @ cov_l @ w.T - np.eye(C)).max() <= 1e-9
    np.testing.assert_allclose(W, W_ref, rtol=1e-8, atol=1e-10)


def test_mahalanobis_reference_matches_scipy():
    from scipy.spatial.distance import mahalanobis
    N, C, K = 90, 32, 3
    x, lab, mean, _ = class_rows(N, C, K, 6)
    S, r4, _ = ood_ref.scatter(x, lab, mean)
    cov_l = ood_ref.shrunk(S, N, ood_ref.ledoit_wolf(S, r4, N))
    W = ood_ref.whitening(cov_l)
    VI = np.linalg.inv(cov_l)
    q = x[:7]
    got = ood_ref.mahalanobis(q, W, mean)
    want = np.array([[mahalanobis(q[n].astype(np.float64), mean[k].astype(np.float64), VI) ** 2 for k in range(K)] for n in range(7)])
    np.testing.assert_allclose(got, want, rtol=1e-9)
    assert (got >= 0).all() and ood_ref.mahalanobis(mean[1:2], W, mean)[0, 1] == 0.0


@pytest.mark.parametrize("T", [0.5, 1.0, 1000.0])
def test_logit_reference_matches_scipy(T):
    from scipy.special import logsumexp, softmax
    rng = np.random.default_rng(1)
    z = rng.standard_normal((9, 5)) * 4
    z[0] = 2.5                                                  # all equal
    z[1] = [80.0, -80.0, 0.0, -80.0, -80.0]                    # dominant
    got = ood_ref.logit_scores(z, T)
    p = softmax(z, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(p > 0, p * np.log(p), 0.0).sum(1)
    np.testing.assert_allclose(got[:, 0], p.max(1), rtol=1e-13)
    assert np.array_equal(got[:, 1], z.max(1))
    np.testing.assert_allclose(got[:, 2], T * logsumexp(z / T, axis=1), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(got[:, 3], ent, rtol=1e-12, atol=1e-15)
    assert abs(got[0, 3] - np.log(5)) < 1e-14 and abs(got[0, 0] - 0.2) < 1e-15 and got[1, 3] >= 0.0


def test_cholesky_failure_names_the_problem_and_ledoit_wolf_repairs_it():
    N, C = 10, 24                                               # N < C: the scatter has rank <= N
    x, lab, mean, _ = class_rows(N, C, 2, 7)
    S, r4, _ = ood_ref.scatter(x, lab, mean)
    with pytest.raises(ValueError, match=r"N = 10 rows in C = 24 dimensions with shrinkage lambda = 0.*ledoit_wolf"):
        ood.whitening_from_scatter(S, r4, N, 0.0)
    W, lam = ood.whitening_from_scatter(S, r4, N, "ledoit_wolf")
    assert 0.0 < lam <= 1.0
    assert np.abs(W @ ood_ref.shrunk(S, N, lam) @ W.T - np.eye(C)).max() <= 1e-9


def test_knn_and_threshold_references():
    rng = np.random.default_rng(2)
    g = rng.standard_normal((20, 8))
    d = ood_ref.knn_score(g, g, 1, "l2")
    assert np.allclose(d, 0.0)                                  # every row is its own nearest neighbour
    assert (ood_ref.knn_score(g, g, 1, "l2", exclude_self=True) > 0).all()
    c = ood_ref.knn_score(g[:3], g, 20, "cosine")
    assert (c <= 4.0 + 1e-12).all() and (c >= 0).all()
    for n, tpr, m in [(100, 0.95, 95), (101, 0.95, 96), (7, 0.95, 7), (40, 0.5, 20), (3, 0.0001, 1), (10, 1.0, 10)]:
        assert ood_ref.threshold_rank(n, tpr) == m == ood.threshold_rank(n, tpr)
    s = rng.standard_normal(101)
    assert (s > ood_ref.threshold(s, 0.95)).sum() == 5
    assert ood_ref.false_positives_at_tpr(np.array([0.0, 1.0, 2.0, 3.0]), np.array([2.5, 3.5])) == 1


def test_scatter_split_is_a_function_of_the_shape_alone():
    npairs, nchunks, cps, nslabs, nbytes = ops.scatter_split(4096, 768)
    assert (npairs, nchunks) == (78, 64) and nslabs * cps >= nchunks > (nslabs - 1) * cps and npairs * nslabs >= 256
    assert nbytes == (nslabs * npairs * 4096 + nchunks) * 8
    assert ops.scatter_split(1, 4) == (1, 1, 1, 1, 4097 * 8)


# ---- validation: everything below raises on a machine without a device, before any launch

def test_logit_scores_validation():
    z = torch.zeros((4, 5))
    for T in (0.0, -1.0, float("inf"), float("nan"), "x"):
        with pytest.raises(GavikoHipError, match="temperature"):
            ood.logit_scores(z, T)
    with pytest.raises(GavikoHipError, match="HIP device"):
        ood.logit_scores(z)
    with pytest.raises(GavikoHipError, match="HIP device"):
        ood.logit_scores([[0.0, 1.0]])


def test_fit_gaussian_validation():
    x, lab = torch.zeros((8, 16)), torch.zeros(8, dtype=torch.int64)
    for s in (-0.1, 1.5, "oas", None, True):
        with pytest.raises(GavikoHipError, match="shrinkage"):
            ood.fit_gaussian(x, lab, 3, shrinkage=s)
    for K in (0, 33, 2.0, True):
        with pytest.raises(GavikoHipError, match="num_classes"):
            ood.fit_gaussian(x, lab, K)
    with pytest.raises(GavikoHipError, match="HIP device"):
        ood.fit_gaussian(x, lab, 3)
    with pytest.raises(GavikoHipError, match="shrinkage"):
        ood.whitening_from_scatter(np.eye(4), 1.0, 4, 2.0)


def test_knn_score_validation():
    x = torch.zeros((8, 16))
    for k in (0, 33, 1.5, True):
        with pytest.raises(GavikoHipError, match="k = "):
            ood.knn_score(x, x, k)
    with pytest.raises(GavikoHipError, match="metric"):
        ood.knn_score(x, x, 3, metric="ip")
    with pytest.raises(GavikoHipError, match="HIP device"):
        ood.knn_score(x, x, 3)


def test_threshold_and_evaluate_validation():
    s = torch.zeros(10)
    for tpr in (0.0, 1.01, -1, "a"):
        with pytest.raises(GavikoHipError, match="tpr"):
            ood.threshold(s, tpr)
    with pytest.raises(GavikoHipError, match="HIP device"):
        ood.threshold(s)
    with pytest.raises(GavikoHipError, match="replicates"):
        ood.evaluate(s, s, replicates=0)
    with pytest.raises(GavikoHipError, match="level"):
        ood.evaluate(s, s, level=1.0)
    with pytest.raises(GavikoHipError, match="HIP device"):
        ood.evaluate(s, s)


def test_ops_wrappers_validation():
    x = torch.zeros((8, 16))
    with pytest.raises(GavikoHipError, match="scatter_matrix x: tensor must live on the HIP device"):
        ops.scatter_matrix(x, None, x[:2])
    with pytest.raises(GavikoHipError, match="mahalanobis q: tensor must live on the HIP device"):
        ops.mahalanobis(x, torch.zeros((16, 16)), x[:2])
    with pytest.raises(GavikoHipError, match="logit_scores logits: tensor must live on the HIP device"):
        ops.logit_scores(x)
    for bad in ([[0.0]], None):
        with pytest.raises(GavikoHipError, match="expected a tensor"):
            ops.scatter_matrix(bad, None, x)
        with pytest.raises(GavikoHipError, match="expected a tensor"):
            ops.mahalanobis(bad, x, x)
        with pytest.raises(GavikoHipError, match="expected a tensor"):
            ops.logit_scores(bad)
