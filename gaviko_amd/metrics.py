"""Evaluation side of eval.py:97-153 with the per-sample work on the device.

`Evaluator` accumulates logits/labels of the validation loop without host reads; `compute()` runs `gvk_eval_rows` (softmax,
argmax, K x K confusion counts) and `gvk_ovr_auc_counts` (exact one-vs-rest pair counts) and finishes the three numbers the
reference logs -- accuracy, quadratic-weighted Cohen kappa, macro one-vs-rest ROC AUC (`sklearn.metrics` calls of eval.py:120-122)
-- in float64 on the host from K*K + 3K integers.  `write_eval_outputs` reproduces the files of eval.py:127-153.
"""
from __future__ import annotations

import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import ops
from .lib import GavikoHipError


def kappa_quadratic(confusion: np.ndarray) -> float:
    """sklearn.metrics.cohen_kappa_score(weights='quadratic') from a confusion matrix.  sklearn builds its label set from the labels
    that OCCUR (in y_true or y_pred), so absent classes are squeezed out before the (i - j)^2 weights are laid down."""
    c = np.asarray(confusion, dtype=np.float64)
    present = (c.sum(0) + c.sum(1)) > 0
    c = c[present][:, present]
    n = c.shape[0]
    if n < 2:
        return float("nan")                              # sklearn: 0/0 with a RuntimeWarning
    expected = np.outer(c.sum(1), c.sum(0)) / c.sum()
    idx = np.arange(n)
    w = (idx[:, None] - idx[None, :]).astype(np.float64) ** 2
    return float(1.0 - (w * c).sum() / (w * expected).sum())


def macro_ovr_auc(counts: np.ndarray) -> float:
    """roc_auc_score(multi_class='ovr', average='macro') from per-class {2*greater + ties, n_pos, n_neg}; sklearn raises when a class
    has no positive (or no negative) sample, and so does this."""
    counts = np.asarray(counts, dtype=np.float64).reshape(-1, 3)
    if (counts[:, 1] == 0).any() or (counts[:, 2] == 0).any():
        raise ValueError("Only one class present in y_true for at least one one-vs-rest problem. ROC AUC score is not defined in that case.")
    return float((counts[:, 0] / (2.0 * counts[:, 1] * counts[:, 2])).mean())


def _device_tensor(what: str, t, noun: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise GavikoHipError(f"{what}: the {noun} must be a tensor on the HIP device (there is no CPU path)")


def _check_replicates(what: str, replicates, optional: bool = False) -> None:
    if optional and replicates is None:
        return
    if isinstance(replicates, bool) or not isinstance(replicates, int) or replicates < 1:
        raise GavikoHipError(f"{what}: replicates = {replicates!r} ({'None or ' if optional else ''}an integer >= 1)")


def _check_level(what: str, level) -> None:
    if not 0.0 < float(level) < 1.0:
        raise GavikoHipError(f"{what}: level = {level!r} outside (0, 1)")


def calibration(proba: torch.Tensor, labels: torch.Tensor, bins: int = 15) -> Dict[str, object]:
    """Calibration of top-1 confidences (Guo et al., 2017) from the device probabilities gvk_eval_rows wrote: proba f32 [N, K], labels [N]
    within [0, K).  gvk_calibration_bins counts, per equal-width confidence bin (i / bins, (i + 1) / bins], the rows, the correct top-1
    predictions and the confidence sum, and sums the Brier and NLL terms, every sum in row order; the rest is float64 on the host:
      ece  = sum_i (n_i / N) |acc_i - conf_i|        mce = max_i |acc_i - conf_i| over the non-empty bins
      brier = (1 / N) sum_n sum_k (p_nk - 1[y_n = k])^2        nll = (1 / N) sum_n -log max(p_n,y_n, FLT_MIN)
      bin_count int64 [bins], bin_accuracy / bin_confidence f64 [bins] (NaN for an empty bin): the reliability diagram."""
    _device_tensor("calibration", proba, "probabilities")
    if proba.dim() != 2:
        raise GavikoHipError(f"calibration: expected proba [N, K], got {tuple(proba.shape)}")
    N, K = proba.shape
    labels = torch.as_tensor(labels).to(proba.device).to(torch.int64).contiguous()
    if labels.numel() != N or N < 1:
        raise GavikoHipError(f"calibration: {labels.numel()} labels for {N} rows of probabilities")
    if int(labels.min()) < 0 or int(labels.max()) >= K:
        raise GavikoHipError(f"calibration: labels outside [0, {K})")
    r = ops.calibration_bins(proba.detach().float().contiguous(), labels, bins)
    count = r["count"].cpu().numpy()
    correct = r["correct"].cpu().numpy().astype(np.float64)
    conf_sum = r["conf_sum"].cpu().numpy()
    some = count > 0
    acc = np.full(bins, np.nan)
    conf = np.full(bins, np.nan)
    acc[some] = correct[some] / count[some]
    conf[some] = conf_sum[some] / count[some]
    gap = np.abs(acc[some] - conf[some])
    return {"ece": float((count[some] / float(N) * gap).sum()), "mce": float(gap.max()), "brier": float(r["brier"].item()) / float(N),
            "nll": float(r["nll"].item()) / float(N), "bin_count": count, "bin_accuracy": acc, "bin_confidence": conf}


def _ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """num / den in float64 with 0 where den == 0 (sklearn's zero_division=0)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.zeros(np.broadcast(num, den).shape), where=den != 0)


def _class_stats(confusion: np.ndarray) -> Dict[str, np.ndarray]:
    """Per-class figures of confusion matrices [..., K, K] (rows = labels, columns = predictions), float64, empty denominators -> 0:
    support, recall, specificity, precision, f1 = 2 tp / (2 tp + fp + fn) (sklearn's form of 2 P R / (P + R)), each [..., K]; and
    balanced_accuracy (mean recall over the classes with support), macro_f1 (mean F1 over the classes in labels or predictions), each [...]."""
    c = np.asarray(confusion, dtype=np.int64)
    tp = np.diagonal(c, axis1=-2, axis2=-1)
    support, predicted = c.sum(-1), c.sum(-2)
    fn, fp = support - tp, predicted - tp
    tn = c.sum((-2, -1))[..., None] - support - fp
    has_label, present = support > 0, (support + predicted) > 0
    recall, f1 = _ratio(tp, support), _ratio(2 * tp, 2 * tp + fp + fn)
    return {"support": support, "recall": recall, "specificity": _ratio(tn, tn + fp), "precision": _ratio(tp, predicted), "f1": f1,
            "balanced_accuracy": _ratio((recall * has_label).sum(-1), has_label.sum(-1)), "macro_f1": _ratio((f1 * present).sum(-1), present.sum(-1))}


def classification_report(confusion) -> Dict[str, object]:
    """Host only, float64, from one K x K confusion matrix (rows = labels): per-class `support` (int64), `recall` (sensitivity), `specificity`,
    `precision` and `f1` as [K] arrays, with sklearn's zero_division=0 for an empty denominator; `balanced_accuracy` = mean recall over the
    classes that occur in the labels (balanced_accuracy_score), `macro_f1` = mean F1 over the classes that occur in the labels or the
    predictions (f1_score(average='macro', zero_division=0))."""
    c = np.asarray(confusion)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] < 1:
        raise ValueError(f"classification_report: expected a K x K confusion matrix, got {c.shape}")
    s = _class_stats(c)
    return dict(s, balanced_accuracy=float(s["balanced_accuracy"]), macro_f1=float(s["macro_f1"]))


def kappa_quadratic_batch(confusion: np.ndarray) -> np.ndarray:
    """kappa_quadratic of R confusion matrices [R, K, K] at once, float64 [R], its absent-class squeeze included: a class that occurs in neither
    the labels nor the predictions of a replicate has an empty row and column there, so it adds nothing to either sum and only has to be left
    out of the numbering behind the (i - j)^2 weights -- the weights use each class's rank among the classes present in that replicate."""
    c = np.asarray(confusion, dtype=np.float64)
    rows, cols = c.sum(2), c.sum(1)
    present = (rows + cols) > 0
    rank = np.cumsum(present, 1) - 1
    w = (rank[:, :, None] - rank[:, None, :]).astype(np.float64) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        expected = rows[:, :, None] * cols[:, None, :] / c.sum((1, 2))[:, None, None]
        k = 1.0 - (w * c).sum((1, 2)) / (w * expected).sum((1, 2))
    return np.where(present.sum(1) < 2, np.nan, k)


BOOTSTRAP_METRICS = ("accuracy", "quadratic_kappa", "auc", "balanced_accuracy", "macro_f1")


def metrics_from_counts(confusion: np.ndarray, auc_counts: np.ndarray) -> Dict[str, np.ndarray]:
    """BOOTSTRAP_METRICS of R replicates, float64 [R] each, from confusion int64 [R, K, K] and auc_counts int64 [R, K, 3].  A replicate in
    which some class has no positive or no negative row has no one-vs-rest AUC: its `auc` is NaN (where macro_ovr_auc raises)."""
    conf = np.asarray(confusion, dtype=np.int64)
    cnt = np.asarray(auc_counts, dtype=np.float64)
    s = _class_stats(conf)
    defined = ((cnt[:, :, 1] > 0) & (cnt[:, :, 2] > 0)).all(1)
    auc = np.full(conf.shape[0], np.nan)
    d = cnt[defined]
    auc[defined] = (d[:, :, 0] / (2.0 * d[:, :, 1] * d[:, :, 2])).mean(1)
    return {"accuracy": _ratio(np.trace(conf, axis1=1, axis2=2), conf.sum((1, 2))), "quadratic_kappa": kappa_quadratic_batch(conf),
            "auc": auc, "balanced_accuracy": s["balanced_accuracy"], "macro_f1": s["macro_f1"]}


class BootstrapResult(NamedTuple):
    point: Dict[str, float]                # BOOTSTRAP_METRICS on the full sample (auc NaN where it is undefined)
    replicates: Dict[str, np.ndarray]      # float64 [R] per metric
    ci: Dict[str, Tuple[float, float]]     # percentile interval: np.nanquantile(rep, [(1 - level) / 2, (1 + level) / 2])
    stderr: Dict[str, float]               # np.nanstd(rep, ddof=1)
    undefined: Dict[str, int]              # NaN replicates per metric
    confusion: np.ndarray                  # int64 [R, K, K]
    auc_counts: np.ndarray                 # int64 [R, K, 3]
    seed: int
    stratified: bool
    level: float


class Comparison(NamedTuple):
    delta_point: Dict[str, float]          # a - b on the full sample
    delta: Dict[str, np.ndarray]           # float64 [R], a - b per replicate (the same multiplicities on both sides)
    ci: Dict[str, Tuple[float, float]]     # percentile interval of delta
    p_value: Dict[str, float]              # two-sided, paired_p_value(delta)
    a: BootstrapResult
    b: BootstrapResult
    seed: int
    stratified: bool
    level: float


def _interval(rep: np.ndarray, level: float) -> Tuple[float, float]:
    if np.isnan(rep).all():
        return (float("nan"), float("nan"))
    lo, hi = np.nanquantile(rep, [(1.0 - level) / 2.0, (1.0 + level) / 2.0])
    return (float(lo), float(hi))


def _stderr(rep: np.ndarray) -> float:
    return float(np.nanstd(rep, ddof=1)) if (~np.isnan(rep)).sum() > 1 else float("nan")


def paired_p_value(delta) -> float:
    """Two-sided bootstrap p-value of 'no difference' from paired replicate differences, over the R_def replicates that are not NaN:
    min(1, 2 min((#{delta <= 0} + 1) / (R_def + 1), (#{delta >= 0} + 1) / (R_def + 1)))."""
    d = np.asarray(delta, dtype=np.float64)
    d = d[~np.isnan(d)]
    n = d.size + 1.0
    return float(min(1.0, 2.0 * min(((d <= 0).sum() + 1.0) / n, ((d >= 0).sum() + 1.0) / n)))


def bootstrap(proba: torch.Tensor, labels: torch.Tensor, *, replicates: int = 2000, seed: int = 0, stratified: bool = False, level: float = 0.95,
              pred: Optional[torch.Tensor] = None) -> BootstrapResult:
    """Bootstrap confidence intervals of the evaluation metrics: proba f32 [N, K] on the device (what gvk_eval_rows wrote), labels [N] within
    [0, K).  gvk_bootstrap_counts resamples the N rows `replicates` times and leaves every replicate's confusion matrix and one-vs-rest AUC
    pair counts as exact integers; BOOTSTRAP_METRICS are finished from them in float64 on the host.
      plain:       draw n of replicate b takes row  (hash_u32(seed, b N + n) * N) >> 32
      stratified:  draw n takes the  ((hash_u32(seed, b N + n) * n_c) >> 32)-th row (ascending) of the class c of row n, which has n_c rows:
                   every class keeps its size, so the AUC is always defined
    A replicate that lost a class (no positive, or no negative row for it) has auc = NaN and counts in undefined["auc"]; the interval and the
    standard error skip NaN.  `pred` i32 [N] (optional): the predictions, where they are not the argmax of proba (lowest index on a tie).
    N <= 8192, 2 <= K <= 64."""
    _device_tensor("bootstrap", proba, "probabilities")
    if proba.dim() != 2:
        raise GavikoHipError(f"bootstrap: expected proba [N, K], got {tuple(proba.shape)}")
    N, K = proba.shape
    labels = torch.as_tensor(labels).to(proba.device).to(torch.int64).contiguous()
    if labels.numel() != N or N < 1:
        raise GavikoHipError(f"bootstrap: {labels.numel()} labels for {N} rows of probabilities")
    if N > ops.BOOTSTRAP_MAX_ROWS or not 2 <= K <= ops.BOOTSTRAP_MAX_CLASSES:
        raise GavikoHipError(f"bootstrap: N = {N}, K = {K} outside N <= {ops.BOOTSTRAP_MAX_ROWS}, 2 <= K <= {ops.BOOTSTRAP_MAX_CLASSES}")
    if int(labels.min()) < 0 or int(labels.max()) >= K:
        raise GavikoHipError(f"bootstrap: labels outside [0, {K})")
    _check_replicates("bootstrap", replicates)
    _check_level("bootstrap", level)
    proba = proba.detach().float().contiguous()
    if bool(torch.isnan(proba).any()):
        raise GavikoHipError("bootstrap: NaN probabilities have no rank")
    if pred is None:
        pred = torch.argmax(proba, dim=1)
    pred = pred.to(proba.device).to(torch.int32).contiguous()
    if pred.numel() != N:
        raise GavikoHipError(f"bootstrap: {pred.numel()} predictions for {N} rows")
    conf_d, cnt_d = ops.bootstrap_counts(labels, pred, ops.bootstrap_tables(proba, labels), replicates, seed, bool(stratified))
    full = torch.zeros(3 * K, dtype=torch.int64, device=proba.device)
    ops.ovr_auc_counts(proba, labels, full)
    conf0 = torch.bincount(labels * K + pred.clamp(0, K - 1).to(torch.int64), minlength=K * K).view(1, K, K)
    conf, cnt = conf_d.cpu().numpy(), cnt_d.cpu().numpy()
    point = {k: float(v[0]) for k, v in metrics_from_counts(conf0.cpu().numpy(), full.cpu().numpy().reshape(1, K, 3)).items()}
    conf0 = conf0.cpu().numpy()[0]
    point["accuracy"], point["quadratic_kappa"] = float(np.trace(conf0)) / float(N), kappa_quadratic(conf0)    # as Evaluator.compute takes them
    if not np.isnan(point["auc"]):
        point["auc"] = macro_ovr_auc(full.cpu().numpy())
    rep = metrics_from_counts(conf, cnt)
    return BootstrapResult(point=point, replicates=rep, ci={k: _interval(v, float(level)) for k, v in rep.items()},
                           stderr={k: _stderr(v) for k, v in rep.items()}, undefined={k: int(np.isnan(v).sum()) for k, v in rep.items()},
                           confusion=conf, auc_counts=cnt, seed=int(seed), stratified=bool(stratified), level=float(level))


def compare(proba_a: torch.Tensor, proba_b: torch.Tensor, labels: torch.Tensor, *, replicates: int = 2000, seed: int = 0, stratified: bool = False,
            level: float = 0.95) -> Comparison:
    """Paired bootstrap comparison of two models on the same rows: both are resampled with the same multiplicities (the rule depends on
    (seed, replicate, draw, labels) alone), so delta = a - b per replicate is the paired difference.  Per metric: delta_point, delta [R], its
    percentile interval, and paired_p_value(delta) over the replicates where both sides are defined."""
    if not isinstance(proba_a, torch.Tensor) or not isinstance(proba_b, torch.Tensor) or tuple(proba_a.shape) != tuple(proba_b.shape):
        raise GavikoHipError("compare: the two models' probabilities must be device tensors of one shape [N, K]")
    a = bootstrap(proba_a, labels, replicates=replicates, seed=seed, stratified=stratified, level=level)
    b = bootstrap(proba_b, labels, replicates=replicates, seed=seed, stratified=stratified, level=level)
    delta = {k: a.replicates[k] - b.replicates[k] for k in BOOTSTRAP_METRICS}
    return Comparison(delta_point={k: a.point[k] - b.point[k] for k in BOOTSTRAP_METRICS}, delta=delta,
                      ci={k: _interval(v, float(level)) for k, v in delta.items()}, p_value={k: paired_p_value(v) for k, v in delta.items()},
                      a=a, b=b, seed=int(seed), stratified=bool(stratified), level=float(level))


class TemperatureFit(NamedTuple):
    T: float                               # the fitted temperature, within [t_min, t_max]
    nll_before: float                      # mean NLL of softmax(logits)
    nll_after: float                       # mean NLL of softmax(logits / T)
    ece_before: float                      # calibration(...)["ece"] of softmax(logits)
    ece_after: float                       # ... of softmax(logits / T)
    iterations: int                        # Newton / bisection steps taken (0 at a bound)
    converged: bool
    at_bound: bool                         # T is t_min or t_max: the NLL still falls (or already rises) at that end of the bracket

    def apply(self, logits: torch.Tensor) -> torch.Tensor:
        """logits / T: the calibrated logits (softmax of them = the calibrated probabilities; the argmax is the one of `logits`)."""
        return logits / self.T


class RiskCoverage(NamedTuple):
    thresholds: np.ndarray                 # float32 [G]: the distinct scores, descending -- accept a row when its score >= threshold
    coverage: np.ndarray                   # float64 [G]: accepted / N at every threshold (ascending, the last is 1)
    risk: np.ndarray                       # float64 [G]: errors / accepted
    accepted: np.ndarray                   # int64 [G]
    errors: np.ndarray                     # int64 [G]
    aurc: float                            # (1 / N) sum over the thresholds of (rows at the threshold) * risk
    optimal_aurc: float                    # the aurc of a score that ranks every wrong row below every right one
    eaurc: float                           # aurc - optimal_aurc
    at: Dict[float, Tuple[float, float, float]]   # coverage asked for -> (threshold, achieved coverage, risk)
    replicates: Optional[Dict[str, np.ndarray]]   # "aurc", "risk@<q>": float64 [R] (None without replicates, as ci and stderr are)
    ci: Optional[Dict[str, Tuple[float, float]]]
    stderr: Optional[Dict[str, float]]
    seed: int
    stratified: bool
    level: float


def optimal_aurc(N: int, E: int) -> float:
    """The smallest aurc a set of N rows with E wrong ones can have (every wrong row ranked last, no ties): the first N - E thresholds have
    risk 0, the j-th wrong row is accepted at risk j / (N - E + j):  (1 / N) sum_{j = 1..E} j / (N - E + j), in float64."""
    j = np.arange(1, int(E) + 1, dtype=np.float64)
    return float(np.sum(j / (float(N - E) + j)) / float(N))


def coverage_need(coverages, N: int) -> List[int]:
    """Accepted-row counts of the coverages asked for: min(N, max(1, ceil(q N))) with q read as the decimal it prints as, in exact rational
    arithmetic -- 0.07 * 100 is 7 rows (the float product 7.000000000000001 would round up to 8)."""
    from fractions import Fraction
    return [min(int(N), max(1, -((-Fraction(repr(float(q))) * int(N)).__floor__()))) for q in coverages]


def fit_temperature(logits: torch.Tensor, labels: torch.Tensor, *, t_min: float = 0.05, t_max: float = 20.0) -> TemperatureFit:
    """Temperature scaling (Guo et al., 2017): the single T within [t_min, t_max] that minimises the mean NLL of softmax(logits / T), fitted
    on the device by one launch of gvk_temperature_fit (safeguarded Newton on beta = 1 / T in float64; the NLL is convex in beta).  logits
    f32 [N, K] on the device, all finite, 2 <= K <= 64; labels [N] within [0, K).  ece_before / ece_after are calibration(...)["ece"] of the
    probabilities gvk_eval_rows writes for logits and logits / T.
    Fit on VALIDATION rows and apply to test rows:  fit = fit_temperature(val_logits, val_labels);  test_proba = softmax(fit.apply(test_logits))
    (or Evaluator.compute(temperature=fit.T)).  A T fitted on the rows it is judged on flatters its own ece_after.  T > 1 softens an
    overconfident model, T < 1 sharpens an underconfident one; the argmax, and so the accuracy, does not change."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[0] < 1:
        raise GavikoHipError(f"fit_temperature: expected logits [N, K], got {tuple(logits.shape) if isinstance(logits, torch.Tensor) else type(logits).__name__}")
    N, K = logits.shape
    if not 2 <= K <= ops.TEMPERATURE_MAX_CLASSES:
        raise GavikoHipError(f"fit_temperature: K = {K} classes outside [2, {ops.TEMPERATURE_MAX_CLASSES}]")
    if not 0.0 < float(t_min) < float(t_max) < float("inf"):
        raise GavikoHipError(f"fit_temperature: need 0 < t_min < t_max, finite (got {t_min!r}, {t_max!r})")
    _device_tensor("fit_temperature", logits, "logits")
    logits = logits.detach().float().contiguous()
    labels = torch.as_tensor(labels).to(logits.device).to(torch.int64).contiguous()
    if labels.numel() != N:
        raise GavikoHipError(f"fit_temperature: {labels.numel()} labels for {N} rows of logits")
    if int(labels.min()) < 0 or int(labels.max()) >= K:
        raise GavikoHipError(f"fit_temperature: labels outside [0, {K})")
    if not bool(torch.isfinite(logits).all()):
        raise GavikoHipError("fit_temperature: non-finite logits have no likelihood")
    st = ops.temperature_fit(logits, labels, t_min, t_max).cpu().numpy()
    T, flags = float(st[0]), int(st[7])

    def ece(z):
        proba, pred = torch.empty_like(z), torch.empty(N, dtype=torch.int32, device=z.device)
        ops.eval_rows(z, labels, proba, pred, torch.zeros(K * K, dtype=torch.int64, device=z.device))
        return calibration(proba, labels)["ece"]

    return TemperatureFit(T=T, nll_before=float(st[2]), nll_after=float(st[3]), ece_before=ece(logits), ece_after=ece((logits / T).contiguous()),
                          iterations=int(st[6]), converged=bool(flags & 1), at_bound=bool(flags & 2))


def risk_coverage(score: torch.Tensor, labels: torch.Tensor, pred: torch.Tensor, *, coverages=(0.5, 0.8, 0.9, 0.95, 1.0),
                  replicates: Optional[int] = None, seed: int = 0, stratified: bool = False, level: float = 0.95) -> RiskCoverage:
    """Selective prediction (Geifman & El-Yaniv, 2017): if the model abstains on its least confident rows, what error is left on the rest?
    score f32 [N] on the device, HIGHER = MORE CONFIDENT, no NaN -- e.g. proba.max(1).values, -predictive.entropy or -predictive.mutual_info
    (uncertainty.py); labels [N] >= 0 and pred [N]: a row is wrong when pred != label.  Rows are accepted from the highest score down, rows
    with EQUAL scores together (nothing depends on the order inside a tie).  Per distinct score (threshold) g: accepted C_g, errors E_g,
    coverage C_g / N, risk E_g / C_g.
      aurc = (1 / N) sum_g c_g E_g / C_g  (c_g rows at threshold g: every row is charged the risk at its own threshold; without ties the
      (1 / N) sum_n E_n / n of the paper),  optimal_aurc(N, E_G) the best any score could do with this many errors,  eaurc their difference
      at[q] = (threshold, achieved coverage, risk) of the first threshold that accepts at least min(N, max(1, ceil(q N))) rows
    replicates = R adds bootstrap replicates of aurc and of every risk@q, drawn by the rule of `bootstrap` (same seed and rule = the same
    resamples, replicate for replicate: they pair with its accuracy / kappa / AUC replicates), with percentile intervals and standard errors.
    gvk_risk_coverage computes all integers exactly on the device.  N <= 8192, labels < 64, at most 8 coverages, each in (0, 1], ascending."""
    if not isinstance(score, torch.Tensor) or score.dim() != 1 or score.numel() < 1:
        raise GavikoHipError(f"risk_coverage: expected score [N], got {tuple(score.shape) if isinstance(score, torch.Tensor) else type(score).__name__}")
    N = score.numel()
    if N > ops.BOOTSTRAP_MAX_ROWS:
        raise GavikoHipError(f"risk_coverage: N = {N} outside N <= {ops.BOOTSTRAP_MAX_ROWS}")
    cov = [float(q) for q in coverages]
    if len(cov) > ops.RISK_COVERAGE_MAX_NEEDS:
        raise GavikoHipError(f"risk_coverage: {len(cov)} coverages (at most {ops.RISK_COVERAGE_MAX_NEEDS})")
    if any(not 0.0 < q <= 1.0 for q in cov) or any(a > b for a, b in zip(cov, cov[1:])):
        raise GavikoHipError(f"risk_coverage: coverages = {coverages!r} (ascending, each within (0, 1])")
    _check_replicates("risk_coverage", replicates, optional=True)
    _check_level("risk_coverage", level)
    if bool(torch.isnan(score).any()):
        raise GavikoHipError("risk_coverage: NaN scores have no rank")
    _device_tensor("risk_coverage", score, "scores")
    score = score.detach().float().contiguous()
    labels = torch.as_tensor(labels).to(score.device).to(torch.int64).contiguous()
    pred = torch.as_tensor(pred).to(score.device).to(torch.int32).contiguous()
    if labels.numel() != N or pred.numel() != N:
        raise GavikoHipError(f"risk_coverage: {labels.numel()} labels and {pred.numel()} predictions for {N} scores")
    if int(labels.min()) < 0 or int(labels.max()) >= ops.BOOTSTRAP_MAX_CLASSES:
        raise GavikoHipError(f"risk_coverage: labels outside [0, {ops.BOOTSTRAP_MAX_CLASSES})")
    need = coverage_need(cov, N)
    tables = ops.selective_tables(score, labels)
    full = ops.risk_coverage_counts(labels, pred, tables, need, resample=False)
    rep_d = ops.risk_coverage_counts(labels, pred, tables, need, replicates, seed, bool(stratified)) if replicates is not None else None
    sorted_score, gend = tables["sorted_score"].cpu().numpy(), tables["gend"].cpu().numpy()
    acc_all, err_all = full["accepted"].cpu().numpy().astype(np.int64), full["errors"].cpu().numpy().astype(np.int64)
    last = gend == np.arange(1, N + 1)                                    # the last position of every tie group: one entry per distinct score
    accepted, errors = acc_all[last], err_all[last]
    at0, E = full["at"].cpu().numpy()[0], int(full["total"].cpu().numpy()[0, 1])
    aurc = float(full["aurc"].item())
    opt = optimal_aurc(N, E)
    # unit multiplicities: the group that first reaches need[q] ends at sorted position C_g - 1
    at = {q: (float(sorted_score[int(c) - 1]), float(c) / float(N), float(e) / float(c)) for q, (c, e) in zip(cov, at0)}
    rep = ci = se = None
    if rep_d is not None:
        at_r = rep_d["at"].cpu().numpy().astype(np.float64)
        rep = {"aurc": rep_d["aurc"].cpu().numpy()}
        for i, q in enumerate(cov):
            rep[f"risk@{q}"] = at_r[:, i, 1] / at_r[:, i, 0]
        ci = {k: _interval(v, float(level)) for k, v in rep.items()}
        se = {k: _stderr(v) for k, v in rep.items()}
    return RiskCoverage(thresholds=sorted_score[last], coverage=accepted / float(N), risk=errors / accepted.astype(np.float64), accepted=accepted,
                        errors=errors, aurc=aurc, optimal_aurc=opt, eaurc=aurc - opt, at=at, replicates=rep, ci=ci, stderr=se, seed=int(seed),
                        stratified=bool(stratified), level=float(level))


class PredictionSets(NamedTuple):
    mask: np.ndarray                       # bool [N, K]: class k is in the set of row n
    size: np.ndarray                       # int64 [N]


class ConformalPredictor(NamedTuple):
    qhat: np.ndarray                       # float32 [K]: class k is in a row's set when its score <= qhat[k] (one value repeated when not mondrian); may be +inf
    alpha: float                           # the miscoverage asked for
    level: float                           # 1 - alpha, the coverage the sets are built for
    n: int                                 # calibration rows
    score: str                             # 'lac', 'aps' or 'raps'
    params: Dict[str, object]              # randomized, seed, k_reg, lam: what conformal_scores was called with
    mondrian: bool

    def sets(self, proba: torch.Tensor) -> PredictionSets:
        """The prediction sets of new rows: proba f32 [N, K] on the device -> mask[n, k] = score[n, k] <= qhat[k], the rule
        gvk_conformal_splits counts the test rows by.  An infinite qhat[k] (too few calibration rows for this alpha) puts k in every set."""
        s = conformal_scores(proba, score=self.score, **self.params)
        if s.shape[1] != self.qhat.size:
            raise GavikoHipError(f"ConformalPredictor.sets: {s.shape[1]} classes, calibrated on {self.qhat.size}")
        mask = (s <= torch.from_numpy(self.qhat).to(s.device)[None, :]).cpu().numpy()
        return PredictionSets(mask=mask, size=mask.sum(1).astype(np.int64))


class ConformalEvaluation(NamedTuple):
    alphas: Tuple[float, ...]              # the Q miscoverage levels
    coverage: np.ndarray                   # float64 [R, Q]: covered test rows / test rows of every split
    mean_size: np.ndarray                  # float64 [R, Q]: mean set size over the test rows of every split
    coverage_mean: np.ndarray              # float64 [Q]: mean over the splits
    coverage_ci: List[Tuple[float, float]]     # per level, the percentile interval of coverage over the splits
    mean_size_mean: np.ndarray             # float64 [Q]
    mean_size_ci: List[Tuple[float, float]]
    singleton: np.ndarray                  # float64 [Q]: share of test rows (all splits pooled) whose set has exactly one class
    empty: np.ndarray                      # float64 [Q]: ... whose set is empty
    size_hist: np.ndarray                  # int64 [Q, K + 1]: test rows by set size, all splits pooled
    coverage_by_size: np.ndarray           # float64 [Q, K + 1]: size-stratified coverage, all splits pooled; NaN where no test row had the size
    class_coverage: np.ndarray             # float64 [R, Q, K]: coverage among the test rows of every label; NaN where a split has none
    class_undefined: np.ndarray            # int64 [K]: splits whose test half has no row of the label
    infinite: np.ndarray                   # float64 [Q]: share of the (split, segment) thresholds that are +inf
    qhat: np.ndarray                       # float32 [R, Q, G]: the thresholds as scores (+inf where a segment has too few calibration rows)
    seed: int
    n_cal: int
    n_test: int
    mondrian: bool
    score: str
    level: float
    counts: Dict[str, np.ndarray]          # the device's integers: qpos [R, Q, G], n_seg [R, G], size_hist / covered_by_size [R, Q, K + 1],
                                           # class_test [R, K], class_covered [R, Q, K]


def _conformal_shape(what: str, proba, labels) -> Tuple[int, int]:
    if not isinstance(proba, torch.Tensor) or proba.dim() != 2 or proba.shape[0] < 1:
        raise GavikoHipError(f"{what}: expected proba [N, K], got {tuple(proba.shape) if isinstance(proba, torch.Tensor) else type(proba).__name__}")
    N, K = proba.shape
    if N > ops.BOOTSTRAP_MAX_ROWS or not 2 <= K <= ops.CONFORMAL_MAX_CLASSES:
        raise GavikoHipError(f"{what}: N = {N}, K = {K} outside N <= {ops.BOOTSTRAP_MAX_ROWS}, 2 <= K <= {ops.CONFORMAL_MAX_CLASSES}")
    if torch.as_tensor(labels).numel() != N:
        raise GavikoHipError(f"{what}: {torch.as_tensor(labels).numel()} labels for {N} rows of probabilities")
    return N, K


def _conformal_labels(what: str, proba, labels) -> torch.Tensor:
    _device_tensor(what, proba, "probabilities")
    labels = torch.as_tensor(labels).to(proba.device).to(torch.int64).contiguous().reshape(proba.shape[0])
    if int(labels.min()) < 0 or int(labels.max()) >= proba.shape[1]:
        raise GavikoHipError(f"{what}: labels outside [0, {proba.shape[1]})")
    return labels


def _conformal_alphas(what: str, alphas) -> List[float]:
    try:
        a = [float(x) for x in alphas]
    except TypeError:
        raise GavikoHipError(f"{what}: alphas = {alphas!r} (a sequence of numbers within (0, 1))") from None
    if not a or any(not 0.0 < x < 1.0 for x in a):
        raise GavikoHipError(f"{what}: alphas = {alphas!r} (at least one, each within (0, 1))")
    return a


def conformal_scores(proba: torch.Tensor, *, score: str = "lac", randomized: bool = False, seed: int = 0, k_reg: int = 1,
                     lam: float = 0.01) -> torch.Tensor:
    """Nonconformity scores for split conformal prediction, f32 [N, K] on the device (a row-major VIEW of the class-major [K, N] buffer
    gvk_conformal_scores writes): low = the class conforms.  proba f32 [N, K] on the device, 2 <= K <= 64, no NaN.  With the classes of a
    row ranked by descending probability (ties: the lower class index first):
      'lac'  (Sadinle et al., 2019)       1 - p_k: the smallest sets on average
      'aps'  (Romano et al., 2020)        the probability mass of the classes ranked at or above k, added in rank order: adaptive sets.
                                          randomized=True counts the class's own mass only u_n times, u_n in [0, 1) from (seed, row)
      'raps' (Angelopoulos et al., 2021)  aps + lam * max(0, rank_k + 1 - k_reg), rank_k 0-based: a penalty that keeps the tail out
    Every operation is one float32 rounding (tests/conformal_ref.py restates the bits in numpy)."""
    if not isinstance(proba, torch.Tensor):
        raise GavikoHipError(f"conformal_scores: expected proba [N, K], got {type(proba).__name__}")
    if proba.is_cuda:
        proba = proba.detach().float().contiguous()
    return ops.conformal_scores(proba, score, bool(randomized), seed, k_reg, lam).t()


def conformal_calibrate(proba: torch.Tensor, labels: torch.Tensor, *, alpha: float = 0.1, mondrian: bool = False, score: str = "lac",
                        randomized: bool = False, seed: int = 0, k_reg: int = 1, lam: float = 0.01) -> ConformalPredictor:
    """Split conformal calibration (Angelopoulos & Bates, 2021) on held-out rows: proba f32 [N, K] on the device, labels [N] within [0, K).
    The threshold is the m-th smallest true-class score of the n calibration rows, m = ceil((n + 1)(1 - alpha)) in float64; the sets
    {k : score_k <= qhat} of exchangeable new rows then contain the label with probability >= 1 - alpha.  m > n (too few rows for this alpha)
    gives qhat = +inf: every class in every set.  mondrian=True calibrates every class on its own rows (class-conditional coverage; a class with
    fewer than ceil(1 / alpha) - 1 calibration rows gets +inf).  gvk_conformal_splits computes the thresholds (n_cal = N, one replicate)."""
    N, K = _conformal_shape("conformal_calibrate", proba, labels)
    a = _conformal_alphas("conformal_calibrate", [alpha])
    labels = _conformal_labels("conformal_calibrate", proba, labels)
    params = {"randomized": bool(randomized), "seed": int(seed), "k_reg": k_reg, "lam": float(lam)}
    s = conformal_scores(proba, score=score, **params).t()
    tables = ops.conformal_tables(s, labels, bool(mondrian))
    qpos = ops.conformal_splits(s, labels, tables, a, N, 1, 0)["qpos"].cpu().numpy()[0, 0]
    sorted_score = tables["sorted_score"].cpu().numpy()
    qhat = np.where(qpos >= 0, sorted_score[np.maximum(qpos, 0)], np.float32(np.inf)).astype(np.float32)
    return ConformalPredictor(qhat=np.broadcast_to(qhat, (K,)).copy(), alpha=a[0], level=1.0 - a[0], n=N, score=score, params=params,
                              mondrian=bool(mondrian))


def conformal_evaluate(proba: torch.Tensor, labels: torch.Tensor, *, alphas=(0.1,), n_cal: Optional[int] = None, calibration_fraction: float = 0.5,
                       replicates: int = 1000, seed: int = 0, mondrian: bool = False, score: str = "lac", randomized: bool = False,
                       k_reg: int = 1, lam: float = 0.01, level: float = 0.95) -> ConformalEvaluation:
    """How a conformal method behaves on this evaluation set, over `replicates` random calibration/test splits (Angelopoulos & Bates, 2021,
    section 3): every split calibrates on n_cal rows (default floor(calibration_fraction N), within [1, N - 1]) and builds the sets of the
    other N - n_cal.  proba f32 [N, K] on the device, labels [N] within [0, K); any number of `alphas` (8 per launch, the same seed and so
    the same splits in every launch).  Split b: the n_cal rows with the smallest keys (hash_u32(seed, b N + i) & ~0x1FFF) | i.
    Reported per level: coverage and mean set size of every split, their means and percentile intervals at `level`, singleton / empty rates,
    the set-size histogram, coverage by set size and per class, and how often a threshold was +inf (a segment with too few calibration rows:
    under mondrian=True a class needs at least ceil(1 / alpha) - 1 of them).  Marginal coverage of a split has expectation
    ceil((n_cal + 1)(1 - alpha)) / (n_cal + 1) when scores do not tie.  gvk_conformal_splits counts everything in exact integers on the device.
    N <= 8192, 2 <= K <= 64."""
    N, K = _conformal_shape("conformal_evaluate", proba, labels)
    a = _conformal_alphas("conformal_evaluate", alphas)
    _check_replicates("conformal_evaluate", replicates)
    _check_level("conformal_evaluate", level)
    if N < 2:
        raise GavikoHipError("conformal_evaluate: a split needs at least 2 rows")
    if n_cal is None:
        if not 0.0 < float(calibration_fraction) < 1.0:
            raise GavikoHipError(f"conformal_evaluate: calibration_fraction = {calibration_fraction!r} outside (0, 1)")
        n_cal = min(N - 1, max(1, int(float(calibration_fraction) * N)))
    if isinstance(n_cal, bool) or not isinstance(n_cal, int) or not 1 <= n_cal <= N - 1:
        raise GavikoHipError(f"conformal_evaluate: n_cal = {n_cal!r} (an integer within [1, {N - 1}]: every split needs test rows)")
    labels = _conformal_labels("conformal_evaluate", proba, labels)
    R, Q, n_test = replicates, len(a), N - n_cal
    s = conformal_scores(proba, score=score, randomized=randomized, seed=seed, k_reg=k_reg, lam=lam).t()
    tables = ops.conformal_tables(s, labels, bool(mondrian))
    parts = [ops.conformal_splits(s, labels, tables, a[i:i + ops.CONFORMAL_MAX_LEVELS], n_cal, R, seed) for i in range(0, Q, ops.CONFORMAL_MAX_LEVELS)]
    counts = {k: np.concatenate([p[k].cpu().numpy() for p in parts], 1) if parts[0][k].dim() == 3 else parts[0][k].cpu().numpy() for k in parts[0]}
    sorted_score = tables["sorted_score"].cpu().numpy()
    qpos = counts["qpos"]
    qhat = np.where(qpos >= 0, sorted_score[np.maximum(qpos, 0)], np.float32(np.inf)).astype(np.float32)
    hist, cov_hist = counts["size_hist"].astype(np.int64), counts["covered_by_size"].astype(np.int64)
    sizes = np.arange(K + 1, dtype=np.float64)
    coverage = cov_hist.sum(2) / float(n_test)
    mean_size = (hist * sizes).sum(2) / float(n_test)
    pooled, pooled_cov = hist.sum(0), cov_hist.sum(0)
    cls_test = counts["class_test"].astype(np.float64)[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        by_size = np.where(pooled > 0, pooled_cov / pooled.astype(np.float64), np.nan)
        by_class = np.where(cls_test > 0, counts["class_covered"] / cls_test, np.nan)
    return ConformalEvaluation(alphas=tuple(a), coverage=coverage, mean_size=mean_size, coverage_mean=coverage.mean(0),
                               coverage_ci=[_interval(coverage[:, q], float(level)) for q in range(Q)], mean_size_mean=mean_size.mean(0),
                               mean_size_ci=[_interval(mean_size[:, q], float(level)) for q in range(Q)],
                               singleton=pooled[:, 1] / float(R * n_test), empty=pooled[:, 0] / float(R * n_test), size_hist=pooled,
                               coverage_by_size=by_size, class_coverage=by_class, class_undefined=(counts["class_test"] == 0).sum(0).astype(np.int64),
                               infinite=(qpos < 0).mean((0, 2)), qhat=qhat, seed=int(seed), n_cal=int(n_cal), n_test=int(n_test),
                               mondrian=bool(mondrian), score=score, level=float(level), counts=counts)


class RocAnalysis(NamedTuple):
    thresholds: np.ndarray                 # float32 [G + 1]: +inf (point 0: call nothing positive), then the distinct scores, descending
    tp: np.ndarray                         # int64 [G + 1]: positives with score >= threshold
    fp: np.ndarray                         # int64 [G + 1]: negatives with score >= threshold
    tpr: np.ndarray                        # float64 [G + 1]: tp / positives (NaN without a positive row)
    fpr: np.ndarray                        # float64 [G + 1]: fp / negatives (NaN without a negative row)
    positives: int
    negatives: int
    auc: float                             # (2 #{positive above negative} + #{tied pairs}) / (2 positives negatives); NaN when undefined
    auc_se: float                          # DeLong's standard error of auc (NaN with fewer than 2 positives or 2 negatives)
    average_precision: float               # sum_g (tp_g / positives) * precision_g: sklearn's step definition
    sensitivity_at: Dict[float, float]     # specificity level -> the largest sensitivity of a point with specificity >= level
    specificity_at: Dict[float, float]     # sensitivity level -> the largest specificity of a point with sensitivity >= level
    at_threshold: Dict[float, Dict[str, float]]   # fixed threshold -> sensitivity, specificity, ppv, npv of "score >= threshold" (NaN: empty denominator)
    youden: Tuple[float, float, float, float]     # (threshold, sensitivity, specificity, J) of the point with the largest J = sens + spec - 1
    replicates: Optional[Dict[str, np.ndarray]]   # float64 [R] per scalar, see roc_analysis (None without replicates, as the five below are)
    ci: Optional[Dict[str, Tuple[float, float]]]
    stderr: Optional[Dict[str, float]]
    undefined: Optional[Dict[str, int]]    # NaN replicates per scalar
    counts: Optional[Dict[str, np.ndarray]]       # the device's integers per replicate: total, auc2, at_spec, at_sens, at_cut, youden
    placements: np.ndarray                 # int64 [N], row order: DeLong's integer placement of every row (delong_placements)
    seed: int
    stratified: bool
    level: float


class RocComparison(NamedTuple):
    delta_point: Dict[str, float]          # a - b on the full sample, per scalar of RocAnalysis.replicates
    delta: Dict[str, np.ndarray]           # float64 [R], a - b per replicate (the same multiplicities on both sides)
    ci: Dict[str, Tuple[float, float]]     # percentile interval of delta
    p_value: Dict[str, float]              # two-sided, paired_p_value(delta)
    delong_z: float                        # (auc_a - auc_b) / sqrt(DeLong's variance of the difference of two correlated curves)
    delong_p: float                        # two-sided normal p-value of delong_z
    a: RocAnalysis
    b: RocAnalysis
    seed: int
    stratified: bool
    level: float


def binary_cut(proba: torch.Tensor, labels: torch.Tensor, cut: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The binary reading "grade >= cut" of K ordered classes (radiographic OA is KL >= 2): proba [N, K], labels [N] ->
    (score = proba[:, cut:].sum(1), positive = labels >= cut).  1 <= cut < K."""
    if not isinstance(proba, torch.Tensor) or proba.dim() != 2:
        raise GavikoHipError(f"binary_cut: expected proba [N, K], got {tuple(proba.shape) if isinstance(proba, torch.Tensor) else type(proba).__name__}")
    K = proba.shape[1]
    if isinstance(cut, bool) or not isinstance(cut, int) or not 1 <= cut < K:
        raise GavikoHipError(f"binary_cut: cut = {cut!r} outside [1, {K})")
    return proba[:, cut:].sum(1), torch.as_tensor(labels).to(proba.device) >= cut


def delong_placements(tp, fp, gend, order, positive) -> np.ndarray:
    """DeLong's placements as integers, host only.  tp, fp [N]: per sorted position (descending score) the positives / negatives at or above
    its score (the curve gvk_roc_replicates writes); gend [N]: one past the end of its tie group; order [N]: the row at every sorted position;
    positive bool [N] in row order.  -> psi int64 [N] in row order:
      positive row:  2 #{negatives scoring lower} + #{negatives tied}  in [0, 2 Nn]
      negative row:  2 #{positives scoring higher} + #{positives tied}  in [0, 2 Pn]
    so that AUC = sum(psi over the positives) / (2 Pn Nn) = sum(psi over the negatives) / (2 Pn Nn)."""
    tp, fp, gend = np.asarray(tp, dtype=np.int64), np.asarray(fp, dtype=np.int64), np.asarray(gend, dtype=np.int64)
    order, positive = np.asarray(order, dtype=np.int64), np.asarray(positive, dtype=bool)
    N = tp.size
    last = gend == np.arange(1, N + 1)
    group = np.concatenate([[0], np.cumsum(last)[:-1]])                    # the tie group of every sorted position
    TP, FP = np.concatenate([[0], tp[last]]), np.concatenate([[0], fp[last]])
    tp_g, fp_g = np.diff(TP)[group], np.diff(FP)[group]
    pos_s = positive[order]
    psi_s = np.where(pos_s, 2 * (FP[-1] - FP[group + 1]) + fp_g, 2 * TP[group] + tp_g)
    psi = np.empty(N, dtype=np.int64)
    psi[order] = psi_s
    return psi


def delong_covariance(psi_a, psi_b, positive) -> float:
    """DeLong, DeLong & Clarke-Pearson (1988): the covariance S10 / Pn + S01 / Nn of the AUCs of two scores on the same rows, from their
    integer placements (delong_placements; psi_a is psi_b: the variance of one AUC).  The sums sum psi, sum psi_a psi_b are exact integers
    (psi <= 2^14, N <= 2^13); each part is (n sum ab - sum a sum b) / (4 m^2 n^2 (n - 1)), n the rows of the part's own class and m those of
    the other, formed in float64 from the exact numerator and denominator.  NaN with fewer than 2 positive or 2 negative rows."""
    a, b, positive = np.asarray(psi_a, dtype=np.int64), np.asarray(psi_b, dtype=np.int64), np.asarray(positive, dtype=bool)
    Pn, Nn = int(positive.sum()), int((~positive).sum())
    if Pn < 2 or Nn < 2:
        return float("nan")

    def part(x, y, n, m):
        num = n * int((x * y).sum()) - int(x.sum()) * int(y.sum())
        return float(num) / float(4 * m * m * n * n * (n - 1))

    return part(a[positive], b[positive], Pn, Nn) + part(a[~positive], b[~positive], Nn, Pn)


def _roc_bp(what: str, levels) -> List[int]:
    try:
        lv = [float(q) for q in levels]
    except TypeError:
        raise GavikoHipError(f"roc_analysis: {what} = {levels!r} (a sequence of numbers within [0, 1])") from None
    if len(lv) > ops.ROC_MAX_LEVELS:
        raise GavikoHipError(f"roc_analysis: {len(lv)} {what} (at most {ops.ROC_MAX_LEVELS})")
    if any(not 0.0 <= q <= 1.0 for q in lv):
        raise GavikoHipError(f"roc_analysis: {what} = {levels!r} (each within [0, 1])")
    return [int(round(q * ops.ROC_BASIS_POINTS)) for q in lv]


def _div(num, den) -> np.ndarray:
    """num / den in float64, NaN where den == 0"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.full(np.broadcast(num, den).shape, np.nan), where=den != 0)


def roc_scalars(counts: Dict[str, np.ndarray], spec_bp, sens_bp, thresholds, sorted_score: np.ndarray) -> Dict[str, np.ndarray]:
    """The scalars of R replicates, float64 [R] each, from the integers of gvk_roc_replicates (host arrays).  With (Pn, Nn) = total:
      auc = auc2 / (2 Pn Nn);  average_precision = ap;  youden_*: of the kernel's point, J = sensitivity + specificity - 1
      sens@spec=<q>: TP / Pn of at_spec;  spec@sens=<q>: (Nn - FP) / Nn of at_sens  (q = level in basis points / 10000)
      sens@thr=<t>, spec@thr=<t>, ppv@thr=<t> = TP / (TP + FP), npv@thr=<t> = TN / (TN + FN) of at_cut
    A replicate with Pn = 0 or Nn = 0 has no curve: every scalar but the predictive values is NaN there; a predictive value is NaN where its
    own denominator is 0."""
    total = np.asarray(counts["total"], dtype=np.int64)
    Pn, Nn = total[:, 0], total[:, 1]
    both = (Pn > 0) & (Nn > 0)
    nan = lambda v: np.where(both, v, np.nan)                              # noqa: E731
    out = {"auc": nan(_div(counts["auc2"], 2.0 * Pn * Nn)), "average_precision": nan(np.asarray(counts["ap"], dtype=np.float64))}
    for i, a in enumerate(spec_bp):
        out[f"sens@spec={a / ops.ROC_BASIS_POINTS}"] = nan(_div(counts["at_spec"][:, i, 0], Pn))
    for i, a in enumerate(sens_bp):
        out[f"spec@sens={a / ops.ROC_BASIS_POINTS}"] = nan(_div(Nn - counts["at_sens"][:, i, 1], Nn))
    for i, t in enumerate(thresholds):
        TP, FP = counts["at_cut"][:, i, 0].astype(np.int64), counts["at_cut"][:, i, 1].astype(np.int64)
        out[f"sens@thr={t}"], out[f"spec@thr={t}"] = nan(_div(TP, Pn)), nan(_div(Nn - FP, Nn))
        out[f"ppv@thr={t}"], out[f"npv@thr={t}"] = _div(TP, TP + FP), _div(Nn - FP, (Nn - FP) + (Pn - TP))
    y = np.asarray(counts["youden"], dtype=np.int64)
    sens, spec = nan(_div(y[:, 0], Pn)), nan(_div(Nn - y[:, 1], Nn))
    out.update(youden_threshold=nan(np.asarray(sorted_score, dtype=np.float64)[y[:, 2]]), youden_sensitivity=sens, youden_specificity=spec,
               youden_j=sens + spec - 1.0)
    return out


def roc_analysis(score: torch.Tensor, positive: torch.Tensor, *, specificities=(0.9, 0.95), sensitivities=(0.9,), thresholds=(),
                 replicates: Optional[int] = None, seed: int = 0, stratified: bool = False, strata: Optional[torch.Tensor] = None,
                 level: float = 0.95) -> RocAnalysis:
    """The ROC analysis of a binary reading (binary_cut gives the one of ordered grades): score f32 [N] on the device, HIGHER = MORE
    POSITIVE, no NaN; positive [N] (bool, or integers with nonzero = positive).  Rows with EQUAL scores are one point of the curve (nothing
    depends on the order inside a tie).  Point g calls a row positive when score >= thresholds[g]; point 0 calls nothing positive.
      specificities: sensitivity_at[q] = the sensitivity of the last point whose specificity is still >= q
      sensitivities: specificity_at[q] = the specificity of the first point whose sensitivity is already >= q
      thresholds:    at_threshold[t] = sensitivity, specificity, ppv, npv of the rule score >= t (t compared with the float32 scores in float64)
    Levels are rounded to BASIS POINTS (0.0001) and compared in exact integers, each within [0, 1], at most 8 per list.
    auc_se is DeLong's (delong_covariance of the rows' placements).  replicates = R adds bootstrap replicates of every scalar -- roc_scalars
    names them -- drawn by the rule of `bootstrap` (same seed and rule = the same resamples, replicate for replicate), with percentile
    intervals, standard errors and the number of undefined (NaN) replicates: a replicate without a positive or without a negative row is
    counted there, not raised.  stratified = True keeps the size of every stratum in every replicate; `strata` [N] are the strata's integer
    labels, by default the binary label itself (pass the K grades to repeat the resamples of bootstrap(..., stratified=True)).
    gvk_roc_replicates computes all integers exactly on the device.  N <= 8192, strata < 64."""
    if not isinstance(score, torch.Tensor) or score.dim() != 1 or score.numel() < 1:
        raise GavikoHipError(f"roc_analysis: expected score [N], got {tuple(score.shape) if isinstance(score, torch.Tensor) else type(score).__name__}")
    N = score.numel()
    if N > ops.BOOTSTRAP_MAX_ROWS:
        raise GavikoHipError(f"roc_analysis: N = {N} outside N <= {ops.BOOTSTRAP_MAX_ROWS}")
    spec_bp, sens_bp = _roc_bp("specificities", specificities), _roc_bp("sensitivities", sensitivities)
    try:
        thr = [float(t) for t in thresholds]
    except TypeError:
        raise GavikoHipError(f"roc_analysis: thresholds = {thresholds!r} (a sequence of numbers)") from None
    if len(thr) > ops.ROC_MAX_LEVELS or any(t != t for t in thr):
        raise GavikoHipError(f"roc_analysis: thresholds = {thresholds!r} (at most {ops.ROC_MAX_LEVELS}, none NaN)")
    _check_replicates("roc_analysis", replicates, optional=True)
    _check_level("roc_analysis", level)
    if bool(torch.isnan(score).any()):
        raise GavikoHipError("roc_analysis: NaN scores have no rank")
    _device_tensor("roc_analysis", score, "scores")
    score = score.detach().float().contiguous()
    positive = torch.as_tensor(positive).to(score.device).reshape(-1) != 0
    if positive.numel() != N:
        raise GavikoHipError(f"roc_analysis: {positive.numel()} labels for {N} scores")
    strata = positive.to(torch.int64) if strata is None else torch.as_tensor(strata).to(score.device).to(torch.int64).contiguous().reshape(-1)
    if strata.numel() != N:
        raise GavikoHipError(f"roc_analysis: {strata.numel()} strata labels for {N} scores")
    if int(strata.min()) < 0 or int(strata.max()) >= ops.BOOTSTRAP_MAX_CLASSES:
        raise GavikoHipError(f"roc_analysis: strata outside [0, {ops.BOOTSTRAP_MAX_CLASSES})")
    pos32 = positive.to(torch.int32)
    tables = ops.roc_tables(score, pos32, strata)
    sorted_score = tables["sorted_score"].cpu().numpy()
    wide = sorted_score.astype(np.float64)
    cut_rows = [int((wide >= t).sum()) for t in thr]
    full_d = ops.roc_counts(pos32, strata, tables, spec_bp, sens_bp, cut_rows, resample=False, curve=True)
    rep_d = ops.roc_counts(pos32, strata, tables, spec_bp, sens_bp, cut_rows, replicates, seed, bool(stratified)) if replicates is not None else None
    full = {k: v.cpu().numpy() for k, v in full_d.items()}
    gend, order = tables["gend"].cpu().numpy(), tables["order"].cpu().numpy()
    last = gend == np.arange(1, N + 1)                                    # the last position of every tie group: one entry per distinct score
    tp = np.concatenate([[0], full["tp"][last]]).astype(np.int64)
    fp = np.concatenate([[0], full["fp"][last]]).astype(np.int64)
    Pn, Nn = int(full["total"][0, 0]), int(full["total"][0, 1])
    point = {k: float(v[0]) for k, v in roc_scalars(full, spec_bp, sens_bp, thr, sorted_score).items()}
    psi = delong_placements(full["tp"], full["fp"], gend, order, positive.cpu().numpy())
    var = delong_covariance(psi, psi, positive.cpu().numpy())
    rep = ci = se = undefined = counts = None
    if rep_d is not None:
        counts = {k: v.cpu().numpy() for k, v in rep_d.items()}
        rep = roc_scalars(counts, spec_bp, sens_bp, thr, sorted_score)
        ci = {k: _interval(v, float(level)) for k, v in rep.items()}
        se = {k: _stderr(v) for k, v in rep.items()}
        undefined = {k: int(np.isnan(v).sum()) for k, v in rep.items()}
    B = float(ops.ROC_BASIS_POINTS)
    return RocAnalysis(thresholds=np.concatenate([[np.float32(np.inf)], sorted_score[last]]).astype(np.float32), tp=tp, fp=fp, tpr=_div(tp, Pn),
                       fpr=_div(fp, Nn), positives=Pn, negatives=Nn, auc=point["auc"], auc_se=float(np.sqrt(var)),
                       average_precision=point["average_precision"],
                       sensitivity_at={a / B: point[f"sens@spec={a / B}"] for a in spec_bp},
                       specificity_at={a / B: point[f"spec@sens={a / B}"] for a in sens_bp},
                       at_threshold={t: {"sensitivity": point[f"sens@thr={t}"], "specificity": point[f"spec@thr={t}"], "ppv": point[f"ppv@thr={t}"],
                                         "npv": point[f"npv@thr={t}"]} for t in thr},
                       youden=(point["youden_threshold"], point["youden_sensitivity"], point["youden_specificity"], point["youden_j"]),
                       replicates=rep, ci=ci, stderr=se, undefined=undefined, counts=counts, placements=psi, seed=int(seed),
                       stratified=bool(stratified), level=float(level))


def roc_compare(score_a: torch.Tensor, score_b: torch.Tensor, positive: torch.Tensor, *, specificities=(0.9, 0.95), sensitivities=(0.9,),
                thresholds=(), replicates: int = 2000, seed: int = 0, stratified: bool = False, strata: Optional[torch.Tensor] = None,
                level: float = 0.95) -> RocComparison:
    """Paired comparison of two scores on the same rows: both are resampled with the same multiplicities (the rule depends on (seed,
    replicate, draw, strata) alone), so delta = a - b per replicate is the paired difference.  Per scalar of roc_analysis: delta_point, delta
    [R], its percentile interval, and paired_p_value(delta) over the replicates where both sides are defined.  For the AUC also DeLong's test
    of two correlated curves: z = (auc_a - auc_b) / sqrt(var_a + var_b - 2 cov_ab) from delong_covariance, p two-sided normal; both NaN when
    the variance of the difference is 0 or undefined."""
    import math
    if not isinstance(score_a, torch.Tensor) or not isinstance(score_b, torch.Tensor) or tuple(score_a.shape) != tuple(score_b.shape):
        raise GavikoHipError("roc_compare: the two models' scores must be device tensors of one shape [N]")
    _check_replicates("roc_compare", replicates)
    kw = dict(specificities=specificities, sensitivities=sensitivities, thresholds=thresholds, replicates=replicates, seed=seed,
              stratified=stratified, strata=strata, level=level)
    a, b = roc_analysis(score_a, positive, **kw), roc_analysis(score_b, positive, **kw)
    delta = {k: a.replicates[k] - b.replicates[k] for k in a.replicates}
    point_a, point_b = _roc_point(a), _roc_point(b)
    pos = (torch.as_tensor(positive).reshape(-1) != 0).cpu().numpy()
    var = delong_covariance(a.placements, a.placements, pos) + delong_covariance(b.placements, b.placements, pos) \
        - 2.0 * delong_covariance(a.placements, b.placements, pos)
    z = (a.auc - b.auc) / math.sqrt(var) if var > 0.0 else float("nan")
    return RocComparison(delta_point={k: point_a[k] - point_b[k] for k in delta}, delta=delta,
                         ci={k: _interval(v, float(level)) for k, v in delta.items()}, p_value={k: paired_p_value(v) for k, v in delta.items()},
                         delong_z=z, delong_p=math.erfc(abs(z) / math.sqrt(2.0)) if z == z else float("nan"), a=a, b=b, seed=int(seed),
                         stratified=bool(stratified), level=float(level))


def _roc_point(r: RocAnalysis) -> Dict[str, float]:
    """the full-sample scalars of a RocAnalysis under the names of its replicates"""
    out = {"auc": r.auc, "average_precision": r.average_precision, "youden_threshold": r.youden[0], "youden_sensitivity": r.youden[1],
           "youden_specificity": r.youden[2], "youden_j": r.youden[3]}
    out.update({f"sens@spec={q}": v for q, v in r.sensitivity_at.items()})
    out.update({f"spec@sens={q}": v for q, v in r.specificity_at.items()})
    for t, d in r.at_threshold.items():
        out.update({f"sens@thr={t}": d["sensitivity"], f"spec@thr={t}": d["specificity"], f"ppv@thr={t}": d["ppv"], f"npv@thr={t}": d["npv"]})
    return out


_bootstrap = bootstrap                                     # Evaluator.compute has a parameter of that name


class Evaluator:
    def __init__(self, num_classes: int, device):
        self.K, self.device = num_classes, device
        self._logits: List[torch.Tensor] = []
        self._labels: List[torch.Tensor] = []

    def update(self, outputs: torch.Tensor, labels: torch.Tensor) -> None:      # eval.py:112-116 without the three .cpu() copies
        self._logits.append(outputs.detach().float())
        self._labels.append(labels.detach().to(torch.int64))

    def compute(self, bootstrap: Optional[int] = None, seed: int = 0, stratified: bool = False, *, selective: bool = False,
                temperature: Optional[float] = None, conformal=None, roc: Optional[int] = None) -> Dict[str, object]:
        """bootstrap = R adds "bootstrap" (the BootstrapResult of R replicates with this seed and rule, on the probabilities and predictions
        computed here) and "report" (classification_report of the confusion matrix); None returns the keys eval.py needs and "calibration".
        selective = True adds "selective": the RiskCoverage of the max-probability confidence, with R replicates of the same seed and rule
        when bootstrap = R.  temperature = T > 0 (fit_temperature on validation rows) takes the probabilities, and with them "auc",
        "calibration", "bootstrap" and "selective", from logits / T; the predictions and the confusion matrix stay those of the logits.
        conformal = alpha (or a sequence of them) adds "conformal": the ConformalEvaluation of the lac score over random halves of these rows
        (conformal_evaluate with this seed; `bootstrap` replicates when given, else 1000), on the probabilities computed here.
        roc = cut adds "roc": the RocAnalysis of the binary reading "class >= cut" (binary_cut of the probabilities computed here), with R
        replicates of the same seed and rule when bootstrap = R; the stratified draw keeps the sizes of the K classes, as "bootstrap" does."""
        logits = torch.cat(self._logits).contiguous()
        labels = torch.cat(self._labels).contiguous().to(self.device)
        N, K = logits.shape
        proba = torch.empty_like(logits)
        pred = torch.empty(N, dtype=torch.int32, device=self.device)
        confusion = torch.zeros(K * K, dtype=torch.int64, device=self.device)
        counts = torch.zeros(3 * K, dtype=torch.int64, device=self.device)
        ops.eval_rows(logits, labels, proba, pred, confusion)
        if temperature is not None:
            T = float(temperature)
            if not 0.0 < T < float("inf"):
                raise GavikoHipError(f"Evaluator.compute: temperature = {temperature!r} (a positive, finite number)")
            ops.eval_rows((logits / T).contiguous(), labels, proba, torch.empty_like(pred), torch.zeros_like(confusion))
        ops.ovr_auc_counts(proba, labels, counts)
        conf = confusion.cpu().numpy().reshape(K, K)
        try:
            auc: Optional[float] = macro_ovr_auc(counts.cpu().numpy())
        except ValueError:
            auc = None
        try:
            cal: Optional[dict] = calibration(proba, labels)
        except GavikoHipError:                               # labels outside [0, K): the confusion counts skip them, calibration has no term for them
            cal = None
        out = {"accuracy": float(np.trace(conf)) / float(N), "quadratic_kappa": kappa_quadratic(conf), "auc": auc, "confusion": conf,
               "y_pred": pred.cpu().numpy(), "y_pred_proba": proba.cpu().numpy(), "y_test": labels.cpu().numpy(),
               "calibration": cal}
        if bootstrap is not None:
            out["bootstrap"] = _bootstrap(proba, labels, replicates=bootstrap, seed=seed, stratified=stratified, pred=pred)
            out["report"] = classification_report(conf)
        if selective:
            out["selective"] = risk_coverage(proba.max(1).values, labels, pred, replicates=bootstrap, seed=seed, stratified=stratified)
        if conformal is not None:
            out["conformal"] = conformal_evaluate(proba, labels, alphas=conformal if isinstance(conformal, (list, tuple)) else (conformal,),
                                                  replicates=1000 if bootstrap is None else bootstrap, seed=seed)
        if roc is not None:
            out["roc"] = roc_analysis(*binary_cut(proba, labels, roc), replicates=bootstrap, seed=seed, stratified=stratified, strata=labels)
        return out


def _versioned_csv(results_dir: str, method: str, backbone: str, kind: str, mri_paths, y_pred):
    os.makedirs(results_dir, exist_ok=True)
    version = 1
    bb = backbone.replace("-", "_")
    while True:
        name = f"{method}_{bb}_{kind}_results_v{version}.csv"
        path = os.path.join(results_dir, name)
        if not os.path.exists(path):
            break
        version += 1
    with open(path, "w") as f:
        f.write("mri_path,outputs\n")
        for p, y in zip(mri_paths, y_pred):
            f.write(f"{os.path.basename(str(p))},{int(y)}\n")
    return path, name


def write_inference_outputs(results_dir: str, method: str, backbone: str, mri_paths, y_pred) -> str:
    """inference.py:117-139: '<method>_<backbone>_inference_results_v<n>.csv' (first free n), columns mri_path (basename), outputs."""
    return _versioned_csv(results_dir, method, backbone, "inference", mri_paths, y_pred)[0]


@torch.no_grad()
def predict(model, loader, transforms=None, device=None) -> np.ndarray:
    """The loop of inference.py:100-113: argmax class of every volume a CustomDatasetPrediction loader yields (one host copy at the end)."""
    device = device or next(model.parameters()).device
    model.eval()
    preds = []
    for inputs in loader:
        x = inputs.to(device)
        preds.append(torch.argmax(model(transforms(x) if transforms is not None else x), dim=1))
    return torch.cat(preds).cpu().numpy()


def write_eval_outputs(results_dir: str, method: str, backbone: str, mri_paths, y_pred, acc, qwk, auc) -> str:
    """eval.py:127-153: '<method>_<backbone>_eval_results_v<n>.csv' (first free n) with columns mri_path (basename), outputs; and the
    '_metrics.txt' next to it."""
    path, name = _versioned_csv(results_dir, method, backbone, "eval", mri_paths, y_pred)
    with open(os.path.join(results_dir, name.replace(".csv", "") + "_metrics.txt"), "w") as f:
        f.write(f"Test Accuracy: {acc}\n")
        f.write(f"Test Quadratic Kappa: {qwk}\n")
        f.write(f"Test AUC: {auc}\n")
    return path
