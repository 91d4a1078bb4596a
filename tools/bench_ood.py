"""Out-of-distribution timings for a bank of N = 4096 rows, C = 768, K = 5 classes and Nq = 1024 queries:

  1. gvk_scatter_matrix alone (device events), next to (x - mu).T @ (x - mu) in torch fp32 in the same run, and its byte and flop time;
  2. gvk_mahalanobis alone, next to the torch formulation that materialises Z = (q - m_k) @ W.T for every class;
  3. a whole ood.fit_gaussian (wall time, device drained before and after), with the host factorisation (two whitening_from_scatter calls)
     and the one device-to-host copy timed separately;
  4. a whole GaussianFit.mahalanobis call.

Report only: no ratio is asked for.  Kernel and torch launches alternate inside every round; every timing is min / median / max over the
rounds.

    python tools/bench_ood.py [--rounds 9] [--launches 20] [--out profiles/ood_timing.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gaviko_amd import ood, ops  # noqa: E402

HBM_TBS, F32_TFLOPS = 6.3, 155.0               # achievable HBM rate and fp32 matrix rate of one MI355X


def spread(ms):
    return dict(min=min(ms), median=statistics.median(ms), max=max(ms))


def event_ms(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, C, K, Nq = 4096, 768, 5, 1024
    g = np.random.default_rng(0)
    lab_h = g.integers(0, K, N)
    mix = g.standard_normal((C, C)) / np.sqrt(C) + np.eye(C)
    x = torch.from_numpy((g.standard_normal((N, C)) @ mix + 2.0 * lab_h[:, None]).astype(np.float32)).to(dev)
    q = torch.from_numpy((g.standard_normal((Nq, C)) @ mix + 2.0 * g.integers(0, K, Nq)[:, None]).astype(np.float32)).to(dev)
    lab = torch.from_numpy(lab_h).to(dev)
    lab32 = lab.to(torch.int32)
    means, _ = ops.class_means(x, lab32, K)
    fit = ood.fit_gaussian(x, lab, K)
    W = fit.whiten

    def torch_scatter():
        d = x - means[lab]
        return d.T @ d

    def torch_maha():
        return torch.stack([(((q - means[k]) @ W.T) ** 2).sum(1) for k in range(K)], 1)

    kern_scatter = lambda: ops.scatter_matrix(x, lab32, means)            # noqa: E731
    kern_maha = lambda: ops.mahalanobis(q, W, means)                      # noqa: E731
    S_k, S_t = kern_scatter()[0], torch_scatter().double()
    d_k, d_t = kern_maha(), torch_maha()
    agree = dict(scatter_rel=float((S_k - S_t).abs().max() / S_t.abs().max()), mahalanobis_rel=float(((d_k - d_t).abs() / d_t.clamp_min(1e-6)).max()))
    for f in (kern_scatter, torch_scatter, kern_maha, torch_maha):
        event_ms(f, 3)
    t = {k: [] for k in ("scatter_kernel", "scatter_torch", "maha_kernel", "maha_torch", "fit_call", "fit_copy", "fit_host", "maha_call")}
    for _ in range(a.rounds):
        t["scatter_kernel"].append(event_ms(kern_scatter, a.launches))
        t["scatter_torch"].append(event_ms(torch_scatter, a.launches))
        t["maha_kernel"].append(event_ms(kern_maha, a.launches))
        t["maha_torch"].append(event_ms(torch_maha, a.launches))
        t["fit_call"].append(wall_ms(lambda: ood.fit_gaussian(x, lab, K))[0])
        S, r4, _ = ops.scatter_matrix(x, lab32, means)
        ms, host = wall_ms(lambda: torch.cat([S.flatten(), r4, S.flatten(), r4]).cpu().numpy())
        t["fit_copy"].append(ms)
        t0 = time.perf_counter()
        for _ in range(2):
            ood.whitening_from_scatter(host[:C * C].reshape(C, C), host[C * C], N)
        t["fit_host"].append(1e3 * (time.perf_counter() - t0))
        t["maha_call"].append(wall_ms(lambda: fit.mahalanobis(q))[0])
    npairs, nchunks, cps, nslabs, scratch = ops.scatter_split(N, C)
    scatter_bytes = 4 * N * C + 8 * C * C + 2 * (scratch - 8 * nchunks)           # x once, S once, slab partials written and read
    res = dict(N=N, C=C, K=K, Nq=Nq, rounds=a.rounds, launches_per_window=a.launches,
               scatter=dict(kernel_ms=spread(t["scatter_kernel"]), torch_fp32_ms=spread(t["scatter_torch"]), split=dict(pairs=npairs, slabs=nslabs, chunks_per_slab=cps),
                            byte_time_ms=1e3 * scatter_bytes / (HBM_TBS * 1e12), flop_time_ms=1e3 * 2.0 * N * C * (C + 64) / 2 / (F32_TFLOPS * 1e12)),
               mahalanobis=dict(kernel_ms=spread(t["maha_kernel"]), torch_fp32_ms=spread(t["maha_torch"]),
                                flop_time_ms=1e3 * 2.0 * (Nq + 16 * (Nq // 16)) * C * C / (F32_TFLOPS * 1e12)),
               fit_gaussian=dict(call_ms=spread(t["fit_call"]), copy_ms=spread(t["fit_copy"]), host_factorisation_ms=spread(t["fit_host"]),
                                 shrinkage=fit.shrinkage, shrinkage0=fit.shrinkage0),
               mahalanobis_call_ms=spread(t["maha_call"]), kernel_vs_torch=agree)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/bench_ood.py --rounds %d --launches %d --out %s\n" % (a.rounds, a.launches, a.out))
            f.write("# one MI355X and its host CPU.  kernel_ms / torch_fp32_ms: per launch between device events over a window of back-to-back launches\n")
            f.write("# (the wrapper's allocations included), kernel and torch windows in turn inside every round; call_ms: wall time, device drained\n")
            f.write("# before and after; min / median / max over the rounds.  byte_time / flop_time: the bytes (x, S, slab partials written and read) at\n")
            f.write("# 6.3 TB/s and the upper-triangle flops at 155 TFLOP/s; for gvk_mahalanobis the flops of whitening the queries and, per tile, 16 centres.\n")
            f.write("# torch: d = x - mu[labels]; d.T @ d  and  stack_k (((q - m_k) @ W.T) ** 2).sum(1), fp32, no fixed order.\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
