"""Out-of-distribution detection on the device: is this scan the kind of scan the model was trained on?

Every score is an ANOMALY score: larger means more out-of-distribution.  Inputs are device tensors; features come from
features.embed(...).pooled or a features.FeatureBank.

    from gaviko_amd import features, ood
    e = features.embed(model, train_img)
    fit = ood.fit_gaussian(e.pooled, train_labels, num_classes=5)         # class means, tied covariance, Ledoit-Wolf shrinkage
    q = features.embed(model, img)
    score, dist = fit.mahalanobis(q.pooled)                                # Lee et al. 2018: min_k d2_k
    rel, _ = fit.relative(q.pooled)                                        # Ren et al. 2021: min_k (d2_k - d2_0)
    s = ood.logit_scores(q.logits)                                         # s.msp, s.max_logit, s.energy, s.entropy
    knn = ood.knn_score(q.pooled, bank, k=10)                              # Sun et al. 2022: distance to the k-th neighbour
    thr = ood.threshold(fit.mahalanobis(val.pooled)[0], tpr=0.95)          # flag a scan when score > thr
    ev = ood.evaluate(score_in, score_out)                                 # AUROC, FPR at 95 % TPR, AUPR with bootstrap intervals

Scores.
  msp        -max softmax probability (Hendrycks & Gimpel 2017)           max_logit  -max logit (Hendrycks et al. 2022)
  energy     -T logsumexp(z / T) (Liu et al. 2020)                         entropy    the entropy of softmax(z), nats
  mahalanobis, relative, knn: above.  'cosine' kNN is 2 - 2 cos (the squared distance of the normalised rows), 'l2' the squared distance.

This module's own definitions.  The covariance is the maximum-likelihood one, divided by N (not N - 1, not N - K): Sigma = S / N with S the
scatter about the class means (tied) or about the grand mean (the background Gaussian of `relative`).  Shrinkage is toward the scaled
identity: Sigma_l = (1 - l) Sigma + l (tr Sigma / C) I; 'ledoit_wolf' is the closed form of Ledoit & Wolf (2004) on the centred rows, which
needs nothing from the device but S and r4 = sum_i (||d_i||^2)^2 (it reproduces sklearn.covariance.ledoit_wolf_shrinkage(d,
assume_centered=True)).  W = L^-1 with L L^T = Sigma_l (float64 on the host, rounded to fp32 once), so d2 = ||W (q - m)||^2.

Host traffic.  fit_gaussian checks the labels' range (one read of min and max, as features.prototypes does) and reads S and r4 of both
Gaussians in ONE copy (the class counts stay on the device); the factorisation runs on the host in float64 (scipy) and W goes back as
fp32.  Scoring reads nothing.

Limits.  C % 4 == 0, C <= 1024; num_classes <= 32 for fit_gaussian (gvk_mahalanobis); logits with 2..256 classes; k <= 32; evaluate takes at
most 8192 scores (metrics.roc_analysis).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import features as F
from . import lib as L
from . import metrics, ops

KNN_METRICS = ("cosine", "l2")


class LogitScores(NamedTuple):
    msp: torch.Tensor                       # f32 [N]: -max softmax probability
    max_logit: torch.Tensor                 # f32 [N]: -max logit
    energy: torch.Tensor                    # f32 [N]: -T logsumexp(z / T)
    entropy: torch.Tensor                   # f32 [N]: entropy of softmax(z), nats


class GaussianFit(NamedTuple):
    means: torch.Tensor                     # f32 [K, C] class means (an empty class: zeros, never the nearest)
    mean0: torch.Tensor                     # f32 [1, C] grand mean
    whiten: torch.Tensor                    # f32 [C, C] W of the tied within-class covariance
    whiten0: torch.Tensor                   # f32 [C, C] W of the total covariance
    shrinkage: float                        # lambda of the tied covariance
    shrinkage0: float                       # lambda of the total covariance
    count: torch.Tensor                     # i32 [K] rows per class

    def _query(self, q, what):
        return F._matrix(q, f"{what} query", self.means.shape[1])

    def _class_dist(self, q):
        d = ops.mahalanobis(q, self.whiten, self.means)
        return torch.where(self.count > 0, d, torch.full_like(d, float("inf")))

    def mahalanobis(self, q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (score f32 [Nq] = min_k d2_k, dist f32 [Nq, K]): the squared Mahalanobis distance to every class mean under the tied
        covariance (+inf for an empty class)."""
        dist = self._class_dist(self._query(q, "GaussianFit.mahalanobis"))
        return dist.min(1).values, dist

    def relative(self, q: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (score f32 [Nq] = min_k (d2_k - d2_0), rel f32 [Nq, K]): d2_0 is the distance to the grand mean under the total covariance."""
        q = self._query(q, "GaussianFit.relative")
        rel = self._class_dist(q) - ops.mahalanobis(q, self.whiten0, self.mean0)
        return rel.min(1).values, rel


class OodEvaluation(NamedTuple):
    auroc: float                            # P(score_out > score_in) + P(tie) / 2
    fpr95: float                            # the fraction of in-distribution rows flagged at the first threshold that flags >= 95 % of the others
    aupr: float                             # average precision, out-of-distribution = positive
    auroc_ci: Optional[Tuple[float, float]]     # percentile bootstrap intervals (None without replicates)
    fpr95_ci: Optional[Tuple[float, float]]
    aupr_ci: Optional[Tuple[float, float]]
    n_in: int
    n_out: int
    roc: metrics.RocAnalysis                # everything else (curve, DeLong standard error, replicates)


def logit_scores(logits: torch.Tensor, temperature: float = 1.0) -> LogitScores:
    """The four logit-based scores of logits f32 [N, K] (2 <= K <= 256), each negated where needed so that larger = more anomalous."""
    try:
        T = float(temperature)
    except (TypeError, ValueError):
        T = float("nan")
    if not 0.0 < T < float("inf"):
        raise L.GavikoHipError(f"logit_scores: temperature = {temperature!r} (a finite positive number)")
    metrics._device_tensor("logit_scores", logits, "logits")
    if logits.dim() != 2 or logits.shape[0] < 1 or not 2 <= logits.shape[1] <= ops.LOGIT_MAX_CLASSES:
        raise L.GavikoHipError(f"logit_scores: expected logits [N, K] with 2 <= K <= {ops.LOGIT_MAX_CLASSES}, got {tuple(logits.shape)}")
    if logits.dtype != torch.float32:
        raise L.GavikoHipError(f"logit_scores: expected float32 logits, got {logits.dtype}")
    out = ops.logit_scores(logits.detach().contiguous(), T)
    return LogitScores(-out[:, 0], -out[:, 1], -out[:, 2], out[:, 3].contiguous())


def _shrinkage_arg(shrinkage):
    if isinstance(shrinkage, str):
        if shrinkage != "ledoit_wolf":
            raise L.GavikoHipError(f"fit_gaussian: shrinkage = {shrinkage!r}: expected 'ledoit_wolf' or a number within [0, 1]")
        return shrinkage
    if isinstance(shrinkage, bool) or not isinstance(shrinkage, (int, float)) or not 0.0 <= float(shrinkage) <= 1.0:
        raise L.GavikoHipError(f"fit_gaussian: shrinkage = {shrinkage!r}: expected 'ledoit_wolf' or a number within [0, 1]")
    return float(shrinkage)


def ledoit_wolf_shrinkage(S: np.ndarray, r4: float, n: int) -> float:
    """The Ledoit-Wolf shrinkage of n centred rows d_i toward (tr Sigma / C) I from S = sum_i d_i d_i^T and r4 = sum_i (||d_i||^2)^2, float64:
      Sigma = S / n,  mu = tr Sigma / C,  delta = (||Sigma||_F^2 - 2 mu tr Sigma + C mu^2) / C  (= ||Sigma - mu I||_F^2 / C),
      beta = min((r4 / n - ||Sigma||_F^2) / (n C), delta),  lambda = beta / delta, and 0 when delta or beta is 0."""
    S = np.asarray(S, dtype=np.float64)
    C = S.shape[0]
    cov = S / n
    trace = float(np.trace(cov))
    mu = trace / C
    fro2 = float((cov * cov).sum())
    delta = (fro2 - 2.0 * mu * trace + C * mu * mu) / C
    beta = min((float(r4) / n - fro2) / (n * C), delta)
    return 0.0 if beta == 0.0 or delta == 0.0 else beta / delta


def whitening_from_scatter(S: np.ndarray, r4: float, n: int, shrinkage="ledoit_wolf") -> Tuple[np.ndarray, float]:
    """Host, float64: S [C, C] = sum of d d^T over n rows -> (W [C, C] with W Sigma_l W^T = I, lambda).  Sigma = S / n, Sigma_l =
    (1 - lambda) Sigma + lambda (tr Sigma / C) I, L = cholesky(Sigma_l) (lower), W = L^-1 by a triangular solve.  A Sigma_l that is not
    positive definite raises ValueError."""
    import scipy.linalg
    shrinkage = _shrinkage_arg(shrinkage)
    S = np.asarray(S, dtype=np.float64)
    C = S.shape[0]
    lam = ledoit_wolf_shrinkage(S, r4, n) if shrinkage == "ledoit_wolf" else shrinkage
    cov = S / n
    cov_l = (1.0 - lam) * cov
    cov_l[np.diag_indices(C)] += lam * (float(np.trace(cov)) / C)
    try:
        low = scipy.linalg.cholesky(cov_l, lower=True, check_finite=True)
    except (scipy.linalg.LinAlgError, ValueError) as e:
        raise ValueError(f"fit_gaussian: the covariance of N = {n} rows in C = {C} dimensions with shrinkage lambda = {lam:.6g} is not positive "
                         f"definite ({e}); use shrinkage='ledoit_wolf' or a larger shrinkage") from None
    W = scipy.linalg.solve_triangular(low, np.eye(C), lower=True, check_finite=False)
    return W, float(lam)


def fit_gaussian(features, labels, num_classes: int, shrinkage="ledoit_wolf") -> GaussianFit:
    """Class-conditional Gaussians with a tied covariance (Lee et al. 2018) and the background Gaussian of the relative distance (Ren et al.
    2021).  features f32 [N, C] on the device (or a FeatureBank), labels [N] integers within [0, num_classes), num_classes <= 32;
    shrinkage: 'ledoit_wolf' or a number within [0, 1].  Class and grand means by gvk_class_means, the two scatters by gvk_scatter_matrix,
    then whitening_from_scatter on the host after ONE read of both scatters and both r4 (the counts stay on the device)."""
    shrinkage = _shrinkage_arg(shrinkage)
    K = num_classes
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= ops.MAHALANOBIS_MAX_K:
        raise L.GavikoHipError(f"fit_gaussian: num_classes = {K!r} outside [1, {ops.MAHALANOBIS_MAX_K}]")
    if isinstance(features, F.FeatureBank):
        if labels is None:
            labels = features.labels
        features = features.features
    f = F._matrix(features, "fit_gaussian features")
    N, C = f.shape
    if N < 2:
        raise L.GavikoHipError(f"fit_gaussian: N = {N} rows (at least 2)")
    if C < 4 or C % 4 or C > ops.FEATURE_MAX_DIM:
        raise L.GavikoHipError(f"fit_gaussian: C = {C} (a multiple of 4 within [4, {ops.FEATURE_MAX_DIM}])")
    lab = F._labels(labels, N, K, f.device, "fit_gaussian")
    means, count = ops.class_means(f, lab, K)
    mean0, _ = ops.class_means(f, torch.zeros_like(lab), 1)
    S, r4, _ = ops.scatter_matrix(f, lab, means)
    S0, r40, _ = ops.scatter_matrix(f, None, mean0)
    host = torch.cat([S.flatten(), r4, S0.flatten(), r40]).cpu().numpy()       # the one read
    cc = C * C
    W, lam = whitening_from_scatter(host[:cc].reshape(C, C), host[cc], N, shrinkage)
    W0, lam0 = whitening_from_scatter(host[cc + 1:2 * cc + 1].reshape(C, C), host[2 * cc + 1], N, shrinkage)
    up = lambda w: torch.from_numpy(w.astype(np.float32)).to(f.device).contiguous()       # noqa: E731
    return GaussianFit(means, mean0, up(W), up(W0), lam, lam0, count)


def knn_score(query, bank, k: int = 10, metric: str = "cosine", exclude_self: bool = False) -> torch.Tensor:
    """The distance to the k-th nearest bank row (Sun et al. 2022) -> f32 [Nq].  metric 'cosine': 2 - 2 cos, the squared distance of the
    normalised rows; 'l2': the squared distance.  exclude_self=True scores the bank itself (pass the same object as query and bank)."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= ops.TOPK_MAX_K:
        raise L.GavikoHipError(f"knn_score: k = {k!r} outside [1, {ops.TOPK_MAX_K}]")
    if metric not in KNN_METRICS:
        raise L.GavikoHipError(f"knn_score: metric = {metric!r}: expected one of {KNN_METRICS}")
    if not isinstance(bank, F.FeatureBank):
        metrics._device_tensor("knn_score", bank, "bank")
    nb = F.knn(query, bank, k, metric, exclude_self)
    kth = nb.score[:, k - 1]
    return 2.0 - 2.0 * kth if metric == "cosine" else kth.contiguous()


def _scores(what, t, noun):
    metrics._device_tensor(what, t, noun)
    if t.dim() != 1 or t.numel() < 1:
        raise L.GavikoHipError(f"{what}: expected {noun} [N], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise L.GavikoHipError(f"{what}: expected float32 {noun}, got {t.dtype}")
    return t.detach()


def threshold_rank(n: int, tpr: float) -> int:
    """The rank of `threshold`: tpr is rounded to basis points bp = round(10000 tpr) and m = ceil(n bp / 10000), at least 1: the smallest
    rank with m / n >= tpr."""
    bp = int(round(float(tpr) * ops.ROC_BASIS_POINTS))
    return max(1, -((-n * bp) // ops.ROC_BASIS_POINTS))


def threshold(scores_in: torch.Tensor, tpr: float = 0.95) -> torch.Tensor:
    """The score below which a fraction `tpr` of the in-distribution scores fall -> a 0-dim device tensor: the m-th smallest score
    (torch.kthvalue, an order statistic, no interpolation) with m = threshold_rank(N, tpr).  Flag a scan when score > threshold: at most
    N - m of the N in-distribution rows are flagged, exactly N - m when the scores are distinct."""
    try:
        ok = 0.0 < float(tpr) <= 1.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise L.GavikoHipError(f"threshold: tpr = {tpr!r} outside (0, 1]")
    s = _scores("threshold", scores_in, "scores")
    return torch.kthvalue(s, threshold_rank(s.numel(), tpr)).values


def evaluate(score_in: torch.Tensor, score_out: torch.Tensor, *, replicates: Optional[int] = 2000, seed: int = 0, level: float = 0.95) -> OodEvaluation:
    """How well a score separates in-distribution rows (score_in f32 [Ni]) from out-of-distribution rows (score_out f32 [No]):
    metrics.roc_analysis of the concatenated scores with out-of-distribution = positive, sensitivities = (0.95,).  fpr95 = 1 - the
    specificity at sensitivity 0.95.  No statistics of its own: the intervals are roc_analysis's percentile bootstrap intervals."""
    metrics._check_replicates("evaluate", replicates, optional=True)
    metrics._check_level("evaluate", level)
    a, b = _scores("evaluate", score_in, "score_in"), _scores("evaluate", score_out, "score_out")
    if a.device != b.device:
        raise L.GavikoHipError(f"evaluate: score_in on {a.device}, score_out on {b.device}")
    score = torch.cat([a, b])
    is_out = torch.cat([torch.zeros(a.numel(), dtype=torch.bool, device=a.device), torch.ones(b.numel(), dtype=torch.bool, device=a.device)])
    r = metrics.roc_analysis(score, is_out, sensitivities=(0.95,), replicates=replicates, seed=seed, level=level)
    ci = r.ci
    fpr_ci = None
    if ci is not None:
        lo, hi = ci["spec@sens=0.95"]
        fpr_ci = (1.0 - hi, 1.0 - lo)
    return OodEvaluation(auroc=r.auc, fpr95=1.0 - r.specificity_at[0.95], aupr=r.average_precision,
                         auroc_ci=None if ci is None else ci["auc"], fpr95_ci=fpr_ci, aupr_ci=None if ci is None else ci["average_precision"],
                         n_in=a.numel(), n_out=b.numel(), roc=r)
