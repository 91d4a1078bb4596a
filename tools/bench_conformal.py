"""Split-conformal timings at N = 1000 rows, K = 5 classes, R = 1000 splits, one level (alpha = 0.1), aps scores:

  a. metrics.conformal_evaluate: the whole call as a user makes it -- gvk_conformal_scores, the sort tables (torch), gvk_conformal_splits,
     the device-to-host copies, the float64 finishing; wall time, the device drained before and after;
  b. the gvk_conformal_splits launch alone (device events, scores and tables prepared once);
  c. the host loop it replaces, timed in the same run on this machine's CPU: per split a numpy permutation, np.partition of the calibration
     rows' true-class scores for the order statistic, the N_test x K compare, set sizes and coverage (scores computed once, outside);
  d. the same by hand with torch on the device: per split torch.randperm, torch.kthvalue, the compare and two reductions, the R results
     read back once at the end.

Report only: medians with their spread over --iters runs after two warm-up runs each.

    python tools/bench_conformal.py [--iters 7] [--host-replicates 1000] [--out profiles/conformal_timing.txt]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gaviko_amd import metrics, ops  # noqa: E402


def aps_host(p):
    """aps scores [N, K] in numpy (float32 cumulative sums in descending order of probability)"""
    order = np.argsort(-p, axis=1, kind="stable")
    c = np.cumsum(np.take_along_axis(p, order, 1), axis=1, dtype=np.float32)
    s = np.empty_like(p)
    np.put_along_axis(s, order, c, 1)
    return s


def host_loop(s, y, n_cal, m, R, seed=0):
    rng = np.random.default_rng(seed)
    N = y.size
    true = s[np.arange(N), y]
    cov, size = np.empty(R), np.empty(R)
    for b in range(R):
        perm = rng.permutation(N)
        cal, test = perm[:n_cal], perm[n_cal:]
        qhat = np.partition(true[cal], m - 1)[m - 1]
        inset = s[test] <= qhat
        cov[b] = (true[test] <= qhat).mean()
        size[b] = inset.sum(1).mean()
    return cov, size


def torch_loop(s, y, n_cal, m, R):
    N = y.numel()
    true = s[torch.arange(N, device=s.device), y]
    cov, size = torch.empty(R, device=s.device), torch.empty(R, device=s.device)
    for b in range(R):
        perm = torch.randperm(N, device=s.device)
        cal, test = perm[:n_cal], perm[n_cal:]
        qhat = torch.kthvalue(true[cal], m).values
        cov[b] = (true[test] <= qhat).float().mean()
        size[b] = (s[test] <= qhat).sum(1).float().mean()
    return cov.cpu().numpy(), size.cpu().numpy()


def timed(fn, iters, warm=2):
    for _ in range(warm):
        out = fn(0)
    ms = []
    for i in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(i)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--host-replicates", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, K, R, alpha = 1000, 5, 1000, 0.1
    n_cal = N // 2
    m = int(math.ceil((n_cal + 1) * (1.0 - alpha)))
    g = np.random.default_rng(0)
    y = g.choice(K, N, p=[0.38, 0.18, 0.26, 0.13, 0.05]).astype(np.int64)      # unbalanced, as KL grades are
    logits = (g.standard_normal((N, K)) + 2.0 * np.eye(K)[y] * (g.random((N, 1)) > 0.3)).astype(np.float32)
    yd = torch.from_numpy(y).to(dev)
    proba = torch.softmax(torch.from_numpy(logits).to(dev), 1).contiguous()
    res = {"N": N, "K": K, "R": R, "alpha": alpha, "n_cal": n_cal, "score": "aps"}

    ev, call = timed(lambda i: metrics.conformal_evaluate(proba, yd, alphas=(alpha,), replicates=R, seed=i, score="aps"), a.iters)
    s = ops.conformal_scores(proba, "aps")
    tables = ops.conformal_tables(s, yd, False)
    kern = []
    for i in range(a.iters + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.conformal_splits(s, yd, tables, [alpha], n_cal, R, i)
        e1.record()
        torch.cuda.synchronize()
        kern.append(e0.elapsed_time(e1))
    p_h = proba.cpu().numpy()
    s_h = aps_host(p_h)
    host_loop(s_h, y, n_cal, m, 5)
    host = []
    for i in range(3):
        t0 = time.perf_counter()
        cov_h, size_h = host_loop(s_h, y, n_cal, m, a.host_replicates, i)
        host.append(1e3 * (time.perf_counter() - t0) * R / a.host_replicates)
    s_rows = s.t().contiguous()
    (cov_t, size_t), by_hand = timed(lambda i: torch_loop(s_rows, yd, n_cal, m, R), a.iters)
    res["conformal_evaluate"] = dict(
        call_ms=call, split_launch_ms=dict(median=statistics.median(kern[2:]), min=min(kern[2:]), max=max(kern[2:])),
        host_loop_ms=dict(median=statistics.median(host), min=min(host), max=max(host)), host_loop_replicates_timed=a.host_replicates,
        torch_loop_ms=by_hand, ratio_host_loop_over_call=statistics.median(host) / call["median"],
        ratio_torch_loop_over_call=by_hand["median"] / call["median"],
        device=dict(coverage_mean=float(ev.coverage_mean[0]), coverage_ci=ev.coverage_ci[0], mean_size=float(ev.mean_size_mean[0])),
        host=dict(coverage_mean=float(cov_h.mean()), coverage_ci=[float(v) for v in np.quantile(cov_h, [0.025, 0.975])], mean_size=float(size_h.mean())),
        torch=dict(coverage_mean=float(cov_t.mean()), mean_size=float(size_t.mean())), expected_coverage=m / (n_cal + 1.0))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/bench_conformal.py --iters %d --host-replicates %d --out %s\n" % (a.iters, a.host_replicates, a.out))
            f.write("# N = 1000 rows, K = 5 classes (unbalanced), R = 1000 random halves, alpha = 0.1, aps scores; one MI355X and its host CPU (one thread\n")
            f.write("# of Python for the host loop).  call_ms: wall time of metrics.conformal_evaluate (scores, sort tables, the split launch, copies back,\n")
            f.write("# float64 finishing), device drained before and after, median / min / max of --iters runs after 2 warm-up runs; split_launch_ms:\n")
            f.write("# gvk_conformal_splits (R = 1000) alone between device events; host_loop_ms: per split numpy permutation + np.partition + the\n")
            f.write("# N_test x K compare, 3 runs, scaled to R if fewer were timed; torch_loop_ms: the same per split with torch.randperm / kthvalue on the\n")
            f.write("# device, results read back once.  The three sides draw different splits (other generators): the figures agree statistically.\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
