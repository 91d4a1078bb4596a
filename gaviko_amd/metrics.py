"""Evaluation side of eval.py:97-153 with the per-sample work on the device.

`Evaluator` accumulates logits/labels of the validation loop without host reads; `compute()` runs `gvk_eval_rows` (softmax,
argmax, K x K confusion counts) and `gvk_ovr_auc_counts` (exact one-vs-rest pair counts) and finishes the three numbers the
reference logs -- accuracy, quadratic-weighted Cohen kappa, macro one-vs-rest ROC AUC (`sklearn.metrics` calls of eval.py:120-122)
-- in float64 on the host from K*K + 3K integers.  `write_eval_outputs` reproduces the files of eval.py:127-153.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

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


def calibration(proba: torch.Tensor, labels: torch.Tensor, bins: int = 15) -> Dict[str, object]:
    """Calibration of top-1 confidences (Guo et al., 2017) from the device probabilities gvk_eval_rows wrote: proba f32 [N, K], labels [N]
    within [0, K).  gvk_calibration_bins counts, per equal-width confidence bin (i / bins, (i + 1) / bins], the rows, the correct top-1
    predictions and the confidence sum, and sums the Brier and NLL terms, every sum in row order; the rest is float64 on the host:
      ece  = sum_i (n_i / N) |acc_i - conf_i|        mce = max_i |acc_i - conf_i| over the non-empty bins
      brier = (1 / N) sum_n sum_k (p_nk - 1[y_n = k])^2        nll = (1 / N) sum_n -log max(p_n,y_n, FLT_MIN)
      bin_count int64 [bins], bin_accuracy / bin_confidence f64 [bins] (NaN for an empty bin): the reliability diagram."""
    if not isinstance(proba, torch.Tensor) or not proba.is_cuda:
        raise GavikoHipError("calibration: the probabilities must be a tensor on the HIP device (there is no CPU path)")
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


class Evaluator:
    def __init__(self, num_classes: int, device):
        self.K, self.device = num_classes, device
        self._logits: List[torch.Tensor] = []
        self._labels: List[torch.Tensor] = []

    def update(self, outputs: torch.Tensor, labels: torch.Tensor) -> None:      # eval.py:112-116 without the three .cpu() copies
        self._logits.append(outputs.detach().float())
        self._labels.append(labels.detach().to(torch.int64))

    def compute(self) -> Dict[str, object]:
        logits = torch.cat(self._logits).contiguous()
        labels = torch.cat(self._labels).contiguous().to(self.device)
        N, K = logits.shape
        proba = torch.empty_like(logits)
        pred = torch.empty(N, dtype=torch.int32, device=self.device)
        confusion = torch.zeros(K * K, dtype=torch.int64, device=self.device)
        counts = torch.zeros(3 * K, dtype=torch.int64, device=self.device)
        ops.eval_rows(logits, labels, proba, pred, confusion)
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
        return {"accuracy": float(np.trace(conf)) / float(N), "quadratic_kappa": kappa_quadratic(conf), "auc": auc, "confusion": conf,
                "y_pred": pred.cpu().numpy(), "y_pred_proba": proba.cpu().numpy(), "y_test": labels.cpu().numpy(),
                "calibration": cal}


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
