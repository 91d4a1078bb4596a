"""Bootstrap timings at N = 1000 rows, K = 5 classes, R = 2000 replicates (a validation set of KL grades), plain and stratified:

  a. metrics.bootstrap: the whole call as a user makes it -- sort tables (torch), gvk_bootstrap_counts, the device-to-host copy of the
     integers, the float64 finishing on the host; wall time, the device drained before and after;
  b. the gvk_bootstrap_counts launch alone (device events, tables prepared once);
  c. the host loop it replaces, timed in the same run on this machine's CPU: numpy resampling (rng.integers, or per class for the
     stratified form) and accuracy_score, cohen_kappa_score(weights='quadratic'), roc_auc_score(multi_class='ovr') per replicate,
     a replicate that lost a class caught and counted as the loop has to.

    python tools/bench_bootstrap.py [--iters 5] [--host-replicates 2000] [--out profiles/bootstrap_timing.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gaviko_amd import metrics, ops  # noqa: E402


def host_loop(proba, y, R, stratified, seed=0):
    from sklearn.metrics import accuracy_score, cohen_kappa_score, roc_auc_score
    rng = np.random.default_rng(seed)
    N, K = proba.shape
    pred = proba.argmax(1)
    p64 = proba.astype(np.float64)
    p64 /= p64.sum(1, keepdims=True)                                # the multiclass call checks the row sums
    lists = [np.flatnonzero(y == c) for c in range(K)]
    acc, qwk, auc, lost = np.empty(R), np.empty(R), np.full(R, np.nan), 0
    for b in range(R):
        rows = np.concatenate([rng.choice(rows_c, rows_c.size) for rows_c in lists]) if stratified else rng.integers(0, N, N)
        yb, pb = y[rows], pred[rows]
        acc[b] = accuracy_score(yb, pb)
        qwk[b] = cohen_kappa_score(yb, pb, weights="quadratic")
        try:
            auc[b] = roc_auc_score(yb, p64[rows], multi_class="ovr", average="macro", labels=np.arange(K))
        except ValueError:
            lost += 1
    return acc, qwk, auc, lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-replicates", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, K, R = 1000, 5, 2000
    g = np.random.default_rng(0)
    y = g.choice(K, N, p=[0.38, 0.18, 0.26, 0.13, 0.05]).astype(np.int64)      # unbalanced, as KL grades are
    logits = g.standard_normal((N, K)) + 2.0 * np.eye(K)[y] * (g.random((N, 1)) > 0.3)
    proba = torch.softmax(torch.from_numpy(logits.astype(np.float32)), 1)
    pd, yd = proba.to(dev), torch.from_numpy(y).to(dev)
    res = {"N": N, "K": K, "R": R}
    for stratified in (False, True):
        key = "stratified" if stratified else "plain"
        for _ in range(2):
            r = metrics.bootstrap(pd, yd, replicates=R, seed=0, stratified=stratified)
        wall = []
        for i in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = metrics.bootstrap(pd, yd, replicates=R, seed=i, stratified=stratified)
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        tables = ops.bootstrap_tables(pd, yd)
        pred = torch.argmax(pd, 1).to(torch.int32)
        conf = torch.empty((R, K, K), dtype=torch.int64, device=dev)
        cnt = torch.empty((R, K, 3), dtype=torch.int64, device=dev)
        kern = []
        for i in range(a.iters + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.bootstrap_counts(yd, pred, tables, R, i, stratified, conf, cnt)
            e1.record()
            torch.cuda.synchronize()
            kern.append(e0.elapsed_time(e1))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            host_loop(proba.numpy(), y, 5, stratified)              # sklearn's import and first-call costs stay out of the timing
            t0 = time.perf_counter()
            acc, qwk, auc, lost = host_loop(proba.numpy(), y, a.host_replicates, stratified)
            host_ms = 1e3 * (time.perf_counter() - t0) * R / a.host_replicates
        res[key] = dict(bootstrap_call_ms=dict(median=statistics.median(wall), min=min(wall), max=max(wall)),
                        kernel_launch_ms=dict(median=statistics.median(kern[2:]), min=min(kern[2:]), max=max(kern[2:])),
                        host_loop_ms=host_ms, host_loop_replicates_timed=a.host_replicates, host_loop_undefined_auc=lost,
                        ratio_host_loop_over_bootstrap_call=host_ms / statistics.median(wall),
                        device=dict(accuracy_ci=r.ci["accuracy"], kappa_ci=r.ci["quadratic_kappa"], auc_ci=r.ci["auc"], undefined_auc=r.undefined["auc"]),
                        host=dict(accuracy_ci=[float(v) for v in np.quantile(acc, [0.025, 0.975])],
                                  kappa_ci=[float(v) for v in np.nanquantile(qwk, [0.025, 0.975])],
                                  auc_ci=[float(v) for v in np.nanquantile(auc, [0.025, 0.975])]))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/bench_bootstrap.py --iters %d --host-replicates %d --out %s\n" % (a.iters, a.host_replicates, a.out))
            f.write("# N = 1000 rows, K = 5 classes (unbalanced), R = 2000 replicates, one MI355X and its host CPU (one thread of Python for the host loop).\n")
            f.write("# bootstrap_call_ms: wall time of metrics.bootstrap (tables, kernel, copy back, float64 finishing), device drained before and after;\n")
            f.write("# kernel_launch_ms: gvk_bootstrap_counts alone between device events; host_loop_ms: numpy resampling + accuracy_score,\n")
            f.write("# cohen_kappa_score(weights='quadratic'), roc_auc_score(multi_class='ovr') per replicate, scaled to R if fewer were timed.\n")
            f.write("# The two sides draw different resamples (another generator): the intervals agree statistically, not bit for bit.\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
