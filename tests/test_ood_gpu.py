"""-m gpu: the kernels of csrc/ood.hip (gvk_scatter_matrix, gvk_mahalanobis, gvk_logit_scores) through their ops wrappers and the
gaviko_amd.ood API, against the float64 restatements of tests/ood_ref.py.  Integer-valued inputs make every fp32 partial an exact
integer, so those cases are compared bit for bit; the bounds of the random cases are worst cases of the fp32 arithmetic at the shapes
used, derived in each docstring, not measured."""
import numpy as np
import pytest
import torch

import ood_ref
from gaviko_amd import features, ood, ops
from gaviko_amd.lib import GavikoHipError

U = 2.0 ** -24                                  # fp32 unit round-off
CHUNK = ops.SCATTER_CHUNK


def gamma(n):
    return n * U / (1.0 - n * U)


def dev_t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


# ------------------------------------------------------------------ scatter_matrix
def scatter_case(N, C, K, seed, labels="random"):
    """x integer in -3..3, means integer in -2..2: d in -5..5, a chunk sum <= 64 * 25, ||d||^2 <= 25 * 1024: exact fp32 integers."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (N, C)).astype(np.float32)
    mean = rng.integers(-2, 3, (K, C)).astype(np.float32)
    if labels == "random":
        lab = rng.integers(0, K, N).astype(np.int32)
    elif labels == "one_empty":
        lab = rng.integers(0, K - 1, N).astype(np.int32)
        lab[lab >= 1] += 1                                      # class 1 stays empty
    elif labels == "one_class":
        lab = np.full(N, K - 1, dtype=np.int32)
    else:
        lab = None
    return x, lab, mean


def run_scatter(dev, x, lab, mean):
    S, r4, count = ops.scatter_matrix(dev_t(x, dev), None if lab is None else dev_t(lab, dev), dev_t(mean, dev))
    assert S.dtype == torch.float64 and r4.dtype == torch.float64 and count.dtype == torch.int32
    return S, r4, count


def assert_scatter_exact(S, r4, count, x, lab, mean):
    wS, wr4, wcount = ood_ref.scatter(x, lab, mean)
    assert np.array_equal(S.cpu().numpy(), wS), np.argwhere(S.cpu().numpy() != wS)[:5]
    assert float(r4.item()) == wr4
    assert np.array_equal(count.cpu().numpy(), wcount)
    assert torch.equal(S, S.T.contiguous())


# the last two: more than 64 chunks (every level of the r4 fold holds a live value; at C = 768 seven slabs of ten chunks) and more than 256
# chunks (a thread of the r4 fold adds two chunks).  Still exact: a chunk sum <= 1600, r4 <= 16500 * (25 * 768)^2 < 2^53.
SCATTER_SHAPES = [(1, 4, 1), (65, 68, 3), (257, 192, 5), (1000, 768, 5), (130, 1024, 2), (CHUNK - 1, 68, 3), (CHUNK, 68, 3),
                  (4200, 768, 3), (16500, 68, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("N,C,K", SCATTER_SHAPES)
def test_scatter_matrix_integer_inputs_exact(dev, N, C, K):
    x, lab, mean = scatter_case(N, C, K, N + C)
    S, r4, count = run_scatter(dev, x, lab, mean)
    assert_scatter_exact(S, r4, count, x, lab, mean)
    again = run_scatter(dev, x, lab, mean)
    assert torch.equal(again[0], S) and torch.equal(again[1], r4) and torch.equal(again[2], count)


@pytest.mark.gpu
@pytest.mark.parametrize("labels", ["one_empty", "one_class", "none"])
def test_scatter_matrix_label_cases(dev, labels):
    N, C, K = 257, 192, 4
    x, lab, mean = scatter_case(N, C, K, 11, labels)
    S, r4, count = run_scatter(dev, x, lab, mean)
    assert_scatter_exact(S, r4, count, x, lab, mean)
    c = count.cpu().numpy()
    if labels == "one_empty":
        assert c[1] == 0 and c.sum() == N
    elif labels == "one_class":
        assert list(c) == [0, 0, 0, N]
    else:
        assert list(c) == [N, 0, 0, 0]


@pytest.mark.gpu
def test_scatter_matrix_ignores_rows_past_n_and_labels_out_of_range(dev):
    N, C, K = 130, 192, 3
    x, lab, mean = scatter_case(N, C, K, 12)
    big = torch.full((N + 70, C), float("nan"), device=dev)
    big[:N] = dev_t(x, dev)
    S, r4, count = ops.scatter_matrix(big[:N], dev_t(lab, dev), dev_t(mean, dev))
    assert bool(torch.isfinite(S).all()) and bool(torch.isfinite(r4).all())
    assert_scatter_exact(S, r4, count, x, lab, mean)
    bad = lab.copy()
    bad[::7] = K                                                # the kernel's own contract: such rows contribute nothing
    bad[3] = -1
    S, r4, count = run_scatter(dev, x, bad, mean)
    assert_scatter_exact(S, r4, count, x, bad, mean)
    assert int(count.sum()) == int(((bad >= 0) & (bad < K)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("N,C,K", [(300, 192, 5), (1000, 768, 5)])
def test_scatter_matrix_gaussian_inputs(dev, N, C, K):
    """Gaussian rows plus a per-class offset of 10; the class means are the device's own (ops.class_means), so d = fl32(x - mean) is the same
    fp32 number on both sides and only products and sums differ.  Inside a chunk of 64 rows an entry is a chain of 64 fmas, one rounding
    each: |error| <= gamma_64 sum |d_a d_b| over the chunk; the chunk sums are added in double (N 2^-53, far below).  Per entry:
    |S - S64| <= 65 u (|D|^T |D|).  ||d||^2 is a sum of C rounded products in some order: relative error <= gamma_(C+1); squared: twice
    that, so |r4 - r4_64| <= 2.1 (C + 1) u r4_64."""
    rng = np.random.default_rng(N)
    lab = rng.integers(0, K, N).astype(np.int32)
    x = (rng.standard_normal((N, C)) + 10.0 * lab[:, None]).astype(np.float32)
    xd, ld = dev_t(x, dev), dev_t(lab, dev)
    mean, _ = ops.class_means(xd, ld, K)
    S, r4, count = ops.scatter_matrix(xd, ld, mean)
    m = mean.cpu().numpy()
    wS, wr4, wcount = ood_ref.scatter(x, lab, m)
    d, _ = ood_ref.centred(x, lab, m)
    assert np.abs(d).max() < 8.0                                # the centring mattered: the raw rows reach 10 K
    bound = 65 * U * (np.abs(d).T @ np.abs(d))
    err = np.abs(S.cpu().numpy() - wS)
    r4_err, r4_bound = abs(float(r4.item()) - wr4), 2.1 * (C + 1) * U * wr4
    print(f"scatter_matrix {N, C, K}: worst S error / bound = {(err / bound).max():.3f}, r4 error / bound = {r4_err / r4_bound:.3f}")
    assert (err <= bound).all() and r4_err <= r4_bound
    assert np.array_equal(count.cpu().numpy(), wcount) and torch.equal(S, S.T.contiguous())


# ------------------------------------------------------------------ mahalanobis
def sparse_w(C, seed):
    """+-1 at the columns j, (j + 1) mod C and (j + 5) mod C of row j (added where two of them coincide, C = 4): not symmetric."""
    rng = np.random.default_rng(seed)
    W = np.zeros((C, C), dtype=np.float32)
    for j in range(C):
        for col in (j, (j + 1) % C, (j + 5) % C):
            W[j, col] += rng.choice([-1.0, 1.0])
    assert not np.array_equal(W, W.T) or C == 4
    return W


def maha_case(Nq, K, C, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, (Nq, C)).astype(np.float32), rng.integers(-3, 4, (K, C)).astype(np.float32)


MAHA_SHAPES = [(1, 1, 4), (15, 5, 68), (16, 32, 768), (17, 5, 1024), (37, 32, 68), (37, 1, 768), (16, 16, 192), (17, 17, 192)]


@pytest.mark.gpu
@pytest.mark.parametrize("Nq,K,C", MAHA_SHAPES)
def test_mahalanobis_integer_inputs_exact(dev, Nq, K, C):
    """|W v| <= 12 for v in -3..3 and three +-1 per row, a squared difference <= 576, a sum over C <= 1024 of them < 2^24: exact."""
    q, m = maha_case(Nq, K, C, Nq * 100 + K)
    W = sparse_w(C, C)
    qd, Wd, md = dev_t(q, dev), dev_t(W, dev), dev_t(m, dev)
    d2 = ops.mahalanobis(qd, Wd, md)
    assert d2.dtype == torch.float32 and tuple(d2.shape) == (Nq, K)
    want = ood_ref.mahalanobis(q, W, m)
    assert want.max() < 2 ** 24
    assert np.array_equal(d2.double().cpu().numpy(), want), np.argwhere(d2.double().cpu().numpy() != want)[:5]
    if C > 4:
        assert not np.array_equal(want, ood_ref.mahalanobis(q, W.T, m))      # a transposed read of W would show
    eye = ops.mahalanobis(qd, torch.eye(C, device=dev), md)
    assert np.array_equal(eye.double().cpu().numpy(), ((q[:, None, :].astype(np.float64) - m[None]) ** 2).sum(2))
    assert torch.equal(ops.mahalanobis(qd, Wd, md), d2)
    into = torch.full((Nq, K), -1.0, device=dev)
    assert ops.mahalanobis(qd, Wd, md, out=into) is into and torch.equal(into, d2)


@pytest.mark.gpu
@pytest.mark.parametrize("Nq,K,C", [(37, 5, 68), (17, 32, 768)])
def test_mahalanobis_row_does_not_depend_on_the_batch(dev, Nq, K, C):
    rng = np.random.default_rng(3)
    q = rng.standard_normal((Nq, C)).astype(np.float32)
    W = (rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    m = rng.standard_normal((K, C)).astype(np.float32)
    big = torch.full((Nq + 20, C), float("nan"), device=dev)
    big[:Nq] = dev_t(q, dev)
    Wd, md = dev_t(W, dev), dev_t(m, dev)
    full = ops.mahalanobis(dev_t(q, dev), Wd, md)
    assert bool(torch.isfinite(full).all())
    assert torch.equal(ops.mahalanobis(big[:Nq], Wd, md), full)              # NaN rows past Nq change nothing
    for n in range(Nq):
        assert torch.equal(ops.mahalanobis(big[n:n + 1], Wd, md)[0], full[n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("C", [192, 768])
def test_mahalanobis_gaussian_inputs(dev, C):
    """W: a real inverse Cholesky factor (ood_ref, Ledoit-Wolf) rounded to fp32; the float64 side uses the same fp32 W, so conditioning
    does not enter.  The device whitens q and m_k separately: with A(v)_j = sum_c |W_jc| |v_c| each whitened coordinate is a chain of C
    fmas, |error| <= gamma_C A(v)_j, so the computed difference is (delta_j + eps_j)(1 + theta), delta = W (q - m_k),
    |eps_j| <= E_j = gamma_C (A(q)_j + A(m_k)_j), |theta| <= u.  Squaring (one rounding) and adding C terms in some order multiplies every
    term by at most 1 + rho, rho = gamma_(C + 3).  So |d2 - d2_64| <= (1 + rho) sum_j (2 |delta_j| E_j + E_j^2) + rho d2_64.
    d2 >= 0 everywhere and exactly 0 for a query that is a centre."""
    rng = np.random.default_rng(C)
    N, K, Nq = 2 * C + 40, 5, 37
    lab = rng.integers(0, K, N)
    mix = rng.standard_normal((C, C)) / np.sqrt(C) + np.eye(C)
    x = (rng.standard_normal((N, C)) @ mix + 10.0 * lab[:, None]).astype(np.float32)
    m = np.stack([x[lab == k].mean(0) for k in range(K)]).astype(np.float32)
    S, r4, _ = ood_ref.scatter(x, lab, m)
    W = ood_ref.whitening(ood_ref.shrunk(S, N, ood_ref.ledoit_wolf(S, r4, N))).astype(np.float32)
    q = (rng.standard_normal((Nq, C)) @ mix + 10.0 * rng.integers(0, K, Nq)[:, None]).astype(np.float32)
    q[5] = m[2]
    d2 = ops.mahalanobis(dev_t(q, dev), dev_t(W, dev), dev_t(m, dev)).double().cpu().numpy()
    want = ood_ref.mahalanobis(q, W, m)
    aW = np.abs(W).astype(np.float64)
    Aq, Am = np.abs(q).astype(np.float64) @ aW.T, np.abs(m).astype(np.float64) @ aW.T
    rho, worst = gamma(C + 3), 0.0
    for k in range(K):
        delta = (q.astype(np.float64) - m[k].astype(np.float64)) @ W.astype(np.float64).T
        E = gamma(C) * (Aq + Am[k])
        bound = (1 + rho) * (2 * np.abs(delta) * E + E * E).sum(1) + rho * want[:, k]
        err = np.abs(d2[:, k] - want[:, k])
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (k, (err / bound).max())
    print(f"mahalanobis C = {C}: worst error / bound = {worst:.4f}; d2 within [{d2.min():.3g}, {d2.max():.3g}]")
    assert (d2 >= 0).all() and d2[5, 2] == 0.0 and want[5, 2] == 0.0


# ------------------------------------------------------------------ logit_scores
def logit_case(K):
    rng = np.random.default_rng(K)
    z = (rng.standard_normal((41, K)) * 5).astype(np.float32)
    z[0] = 2.5                                                  # all equal: entropy log K, msp 1 / K
    z[1] = -80.0
    z[1, K // 2] = 80.0                                         # dominant: nothing overflows, entropy >= 0
    z[2] = 80.0
    z[2, 0] = -80.0
    z[3] = 0.0
    z[3, K - 1] = 1e-3                                          # a maximum barely above the rest
    z[4, :] = z[5, :]
    z[4, 0] = z[4, K - 1] = z[4].max() + 1.0                    # a tied maximum
    return z


@pytest.mark.gpu
@pytest.mark.parametrize("T", [0.5, 1.0, 1000.0])
@pytest.mark.parametrize("K", [2, 5, 256])
def test_logit_scores_against_float64(dev, K, T):
    """The kernel computes in double from the fp32 logits and rounds once at the store: |error| <= 1 ulp of fp32 at the float64 value
    (half an ulp of rounding, the rest for the double arithmetic); T is exact in fp32 for the three values, the logits are fp32 on both
    sides, so no input rounding enters."""
    z = logit_case(K)
    out = ops.logit_scores(dev_t(z, dev), T)
    assert out.dtype == torch.float32 and tuple(out.shape) == (41, 4)
    got, want = out.double().cpu().numpy(), ood_ref.logit_scores(z, T)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want)
    print(f"logit_scores K = {K}, T = {T}: worst error / ulp = {(err / ulp).max():.3f}")
    assert np.isfinite(got).all() and (err <= ulp).all(), np.argwhere(err > ulp)[:5]
    assert abs(got[0, 3] - np.log(K)) <= np.spacing(np.float32(np.log(K))) and abs(got[0, 0] - 1.0 / K) <= np.spacing(np.float32(1.0 / K))
    assert (got[:, 3] >= 0).all() and got[1, 0] == 1.0 and got[1, 1] == 80.0
    s = ood.logit_scores(dev_t(z, dev), T)
    assert torch.equal(s.msp, -out[:, 0]) and torch.equal(s.max_logit, -out[:, 1]) and torch.equal(s.energy, -out[:, 2])
    assert torch.equal(s.entropy, out[:, 3])


# ------------------------------------------------------------------ end to end
def paired_classes(sizes, C, centres, seed):
    """Integer features whose class means and grand mean are integers: every class is made of pairs centre + e, centre - e with e in
    -3..3, and sum_k size_k centre_k = 0.  Then d is an integer for both Gaussians and S, r4 are exact."""
    rng = np.random.default_rng(seed)
    assert sum(s * c for s, c in zip(sizes, centres)) == 0 and all(s % 2 == 0 for s in sizes)
    xs, ls = [], []
    for k, (s, c) in enumerate(zip(sizes, centres)):
        e = rng.integers(-3, 4, (s // 2, C)).astype(np.float32)
        xs += [c + e, c - e]
        ls += [np.full(s, k, dtype=np.int64)]
    x, lab = np.concatenate(xs), np.concatenate(ls)
    p = rng.permutation(len(x))
    return x[p], lab[p]


@pytest.mark.gpu
@pytest.mark.parametrize("sizes,centres", [((14, 14, 12), (-6, 6, 0)), ((100, 100, 100), (-10, 0, 10))])
def test_fit_gaussian_end_to_end(dev, sizes, centres):
    C, K, N = 64, 3, sum(sizes)
    x, lab = paired_classes(sizes, C, centres, N)
    xd = dev_t(x, dev)
    fit = ood.fit_gaussian(xd, dev_t(lab, dev), K)
    means, mean0 = fit.means.cpu().numpy(), fit.mean0.cpu().numpy()
    assert np.array_equal(means, np.repeat(np.array(centres, dtype=np.float32)[:, None], C, 1)) and not mean0.any()
    assert list(fit.count.cpu().numpy()) == list(sizes)
    S, r4, _ = ood_ref.scatter(x, lab, means)
    S0, r40, _ = ood_ref.scatter(x, None, mean0)
    lam, lam0 = ood_ref.ledoit_wolf(S, r4, N), ood_ref.ledoit_wolf(S0, r40, N)
    print(f"fit_gaussian N = {N}: shrinkage {fit.shrinkage:.15g} (reference {lam:.15g}), shrinkage0 {fit.shrinkage0:.15g} (reference {lam0:.15g})")
    assert 0.0 < lam < 1.0 and 0.0 < lam0 < 1.0
    assert abs(fit.shrinkage - lam) <= 1e-12 * lam and abs(fit.shrinkage0 - lam0) <= 1e-12 * lam0
    for W, SS, l in ((fit.whiten, S, lam), (fit.whiten0, S0, lam0)):
        w = W.double().cpu().numpy()
        cov = ood_ref.shrunk(SS, N, l)                           # W = W64 (1 + e), |e| <= u: W cov W^T - I = 2 e-terms + O(u^2), float64 part 1e-9
        assert W.dtype == torch.float32 and (np.abs(w @ cov @ w.T - np.eye(C)) <= 2.1 * U * (np.abs(w) @ np.abs(cov) @ np.abs(w).T) + 1e-9).all()
    q = dev_t(np.random.default_rng(1).integers(-12, 13, (21, C)).astype(np.float32), dev)
    by_hand = ops.mahalanobis(q, fit.whiten, fit.means)
    score, dist = fit.mahalanobis(q)
    assert torch.equal(dist, by_hand) and torch.equal(score, by_hand.min(1).values)
    rel_hand = by_hand - ops.mahalanobis(q, fit.whiten0, fit.mean0)
    rscore, rel = fit.relative(q)
    assert torch.equal(rel, rel_hand) and torch.equal(rscore, rel_hand.min(1).values)
    fixed = ood.fit_gaussian(xd, dev_t(lab, dev), K, shrinkage=0.25)
    assert fixed.shrinkage == 0.25 == fixed.shrinkage0 and torch.equal(fixed.means, fit.means)
    if N < C:
        with pytest.raises(ValueError, match=rf"N = {N} rows in C = {C} dimensions"):
            ood.fit_gaussian(xd, dev_t(lab, dev), K, shrinkage=0.0)
    with pytest.raises(GavikoHipError, match="labels within"):
        ood.fit_gaussian(xd, dev_t(lab + 1, dev), K)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_knn_score_is_the_kth_neighbour(dev, metric):
    """Equal to column k - 1 of features.knn bit for bit.  Against float64 (an order statistic moves by at most the largest error of a
    distance): 'l2' is (|q|^2 + |g|^2) - 2 q.g, three C-term fp32 sums and two combinations: <= 2 (C + 2) u (|q| + |g|)^2; 'cosine' divides
    both rows by their fp32 norms (relative error (C / 2 + 2) u per element), takes a C-term inner product of unit rows and forms
    2 - 2 s: <= (4 C + 16) u."""
    rng = np.random.default_rng(4)
    g = dev_t(rng.standard_normal((150, 64)).astype(np.float32), dev)
    q = dev_t(rng.standard_normal((23, 64)).astype(np.float32), dev)
    bank = features.FeatureBank(64, dev).add(g)
    k = 7
    nb = features.knn(q, bank, k, metric)
    col = nb.score[:, k - 1]
    got = ood.knn_score(q, bank, k, metric)
    assert torch.equal(got, 2.0 - 2.0 * col if metric == "cosine" else col)
    qn, gn = q.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    gmax = np.linalg.norm(gn, axis=1).max()

    def bound(rows):
        return np.full(len(rows), (4 * 64 + 16) * U) if metric == "cosine" else 2 * (64 + 2) * U * (np.linalg.norm(rows, axis=1) + gmax) ** 2

    err = np.abs(got.double().cpu().numpy() - ood_ref.knn_score(qn, gn, k, metric))
    own = ood.knn_score(bank, bank, k, metric, exclude_self=True)
    err_own = np.abs(own.double().cpu().numpy() - ood_ref.knn_score(gn, gn, k, metric, exclude_self=True))
    print(f"knn_score {metric}: worst error / bound = {max((err / bound(qn)).max(), (err_own / bound(gn)).max()):.3f}")
    assert (err <= bound(qn)).all() and (err_own <= bound(gn)).all() and bool((own > 0).all())


@pytest.mark.gpu
def test_evaluate_and_threshold(dev):
    from sklearn.metrics import average_precision_score, roc_auc_score
    rng = np.random.default_rng(5)
    C, Ni, No = 16, 301, 207
    cloud_in = rng.standard_normal((Ni, C)).astype(np.float32)
    cloud_out = (rng.standard_normal((No, C)) + 0.9).astype(np.float32)
    fit = ood.fit_gaussian(dev_t(cloud_in, dev), torch.zeros(Ni, dtype=torch.int64), 1)
    s_in, _ = fit.mahalanobis(dev_t(cloud_in, dev))
    s_out, _ = fit.mahalanobis(dev_t(cloud_out, dev))
    ev = ood.evaluate(s_in, s_out, replicates=50, seed=3)
    a, b = s_in.cpu().numpy(), s_out.cpu().numpy()
    y, s = np.concatenate([np.zeros(Ni, dtype=bool), np.ones(No, dtype=bool)]), np.concatenate([a, b])
    pairs2 = 2 * int((b[:, None] > a[None, :]).sum()) + int((b[:, None] == a[None, :]).sum())
    assert ev.auroc == pairs2 / (2.0 * Ni * No) and abs(ev.auroc - roc_auc_score(y, s)) <= 1e-12
    assert abs(ev.aupr - average_precision_score(y, s)) <= 1e-12
    fp = ood_ref.false_positives_at_tpr(a, b)
    assert ev.fpr95 == 1.0 - (Ni - fp) / Ni and 0 < fp < Ni and 0.6 < ev.auroc < 1.0
    assert (ev.n_in, ev.n_out) == (Ni, No)
    assert ev.auroc_ci[0] <= ev.auroc <= ev.auroc_ci[1] and ev.fpr95_ci[0] <= ev.fpr95_ci[1] and ev.aupr_ci[0] <= ev.aupr_ci[1]
    assert ood.evaluate(s_in, s_out, replicates=None).auroc_ci is None
    for tpr in (0.95, 0.5, 1.0):
        thr = ood.threshold(s_in, tpr)
        m = ood_ref.threshold_rank(Ni, tpr)
        assert len(np.unique(a)) == Ni and float(thr) == ood_ref.threshold(a, tpr)
        assert int((s_in > thr).sum()) == Ni - m                 # exactly the documented number of in-distribution rows is flagged


# ------------------------------------------------------------------ validation on the device, the example
@pytest.mark.gpu
def test_validation_on_the_device_names_the_argument(dev):
    """What the CPU file cannot reach: the checks behind the device check, each before any launch."""
    x = torch.zeros((8, 16), device=dev)
    lab = torch.zeros(8, dtype=torch.int64, device=dev)
    with pytest.raises(GavikoHipError, match=r"N = 1 rows \(at least 2\)"):
        ood.fit_gaussian(x[:1], lab[:1], 1)
    with pytest.raises(GavikoHipError, match=r"C = 6 \(a multiple of 4"):
        ood.fit_gaussian(torch.zeros((8, 6), device=dev), lab, 1)
    with pytest.raises(GavikoHipError, match=r"C = 1028 \(a multiple of 4"):
        ood.fit_gaussian(torch.zeros((8, 1028), device=dev), lab, 1)
    with pytest.raises(GavikoHipError, match="expected float32"):
        ood.fit_gaussian(x.double(), lab, 1)
    with pytest.raises(GavikoHipError, match=r"expected \[N, C\]"):
        ood.fit_gaussian(x[0], lab, 1)
    with pytest.raises(GavikoHipError, match="expected 8 integer labels"):
        ood.fit_gaussian(x, lab[:7], 1)
    with pytest.raises(GavikoHipError, match="expected 8 integer labels"):
        ood.fit_gaussian(x, lab.float(), 1)
    with pytest.raises(GavikoHipError, match="num_classes = 0 outside"):
        ood.fit_gaussian(x, lab, 0)
    with pytest.raises(GavikoHipError, match=r"labels within \[-1, 0\]"):
        ood.fit_gaussian(x, torch.tensor([-1] + [0] * 7, device=dev), 2)
    fit = ood.fit_gaussian(torch.randn((40, 16), device=dev), torch.zeros(40, dtype=torch.int64), 1)
    for call in (fit.mahalanobis, fit.relative):
        with pytest.raises(GavikoHipError, match="C = 8, expected 16"):
            call(torch.zeros((3, 8), device=dev))
        with pytest.raises(GavikoHipError, match="expected float32"):
            call(torch.zeros((3, 16), device=dev, dtype=torch.float64))
    z = torch.zeros((4, 5), device=dev)
    with pytest.raises(GavikoHipError, match="expected float32 logits"):
        ood.logit_scores(z.half())
    for bad in (z[0], z[:, :1], torch.zeros((4, 257), device=dev), z[:0]):
        with pytest.raises(GavikoHipError, match=r"expected logits \[N, K\] with 2 <= K <= 256"):
            ood.logit_scores(bad)
    with pytest.raises(GavikoHipError, match="temperature"):
        ood.logit_scores(z, 0.0)
    with pytest.raises(GavikoHipError, match=r"K = 257 classes outside \[2, 256\]"):
        ops.logit_scores(torch.zeros((4, 257), device=dev))
    with pytest.raises(GavikoHipError, match="temperature"):
        ops.logit_scores(z, -1.0)
    with pytest.raises(GavikoHipError, match=r"K = 33 centres outside \[1, 32\]"):
        ops.mahalanobis(x, torch.eye(16, device=dev), torch.zeros((33, 16), device=dev))
    with pytest.raises(GavikoHipError, match=r"whiten: expected \[16, 16\]"):
        ops.mahalanobis(x, torch.zeros((8, 16), device=dev), x)
    with pytest.raises(GavikoHipError, match="mahalanobis centres: C = 8, expected 16"):
        ops.mahalanobis(x, torch.eye(16, device=dev), torch.zeros((2, 8), device=dev))
    with pytest.raises(GavikoHipError, match="must be contiguous"):
        ops.mahalanobis(x.T.contiguous().T, torch.eye(16, device=dev), x)
    with pytest.raises(GavikoHipError, match="scatter_matrix mean: C = 8, expected 16"):
        ops.scatter_matrix(x, None, torch.zeros((2, 8), device=dev))
    with pytest.raises(GavikoHipError, match="scatter_matrix labels: expected 8 int32 entries"):
        ops.scatter_matrix(x, torch.zeros(7, dtype=torch.int32, device=dev), x[:2])
    with pytest.raises(GavikoHipError, match="scatter_matrix labels: expected torch.int32"):
        ops.scatter_matrix(x, lab, x[:2])
    s = torch.zeros(10, device=dev)
    for fn in (ood.threshold, lambda t: ood.evaluate(t, s), lambda t: ood.evaluate(s, t)):
        with pytest.raises(GavikoHipError, match=r"expected (scores|score_in|score_out) \[N\]"):
            fn(torch.zeros((2, 5), device=dev))
        with pytest.raises(GavikoHipError, match=r"expected (scores|score_in|score_out) \[N\]"):
            fn(s[:0])
        with pytest.raises(GavikoHipError, match="expected float32"):
            fn(s.double())
    with pytest.raises(GavikoHipError, match="k = 33"):
        ood.knn_score(x, x, 33)
    with pytest.raises(GavikoHipError, match="exclude_self=True needs the query to be the bank"):
        ood.knn_score(x[:4], x, 2, exclude_self=True)


@pytest.mark.gpu
def test_example_ood_option_runs(dev, tmp_path):
    """examples/train_synthetic.py --ood on its smallest run: 8 volumes, 5 classes (so several classes are empty: distance +inf, never the
    nearest) and a handful of validation scores through roc_analysis: it runs, logs its line and every figure is finite."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic as ts
    lines = []
    res = ts.run(method="gaviko", backbone="vit-t16", epochs=1, samples=8, out=str(tmp_path), batch_size=4, log=lines.append, ood_scores=True)
    ev = res["ood"]
    assert isinstance(ev, ood.OodEvaluation) and ev.n_in == ev.n_out >= 1
    assert np.isfinite([ev.auroc, ev.fpr95, ev.aupr]).all() and 0.0 <= ev.auroc <= 1.0 and 0.0 <= ev.fpr95 <= 1.0 and 0.0 < ev.aupr <= 1.0
    assert np.isfinite(ev.roc.thresholds[1:]).all()             # no score is +inf or NaN although several classes are empty
    assert any(l.startswith("ood (relative Mahalanobis") for l in lines)
    assert ts.run.__defaults__[-1] is False                     # the default run does none of this
