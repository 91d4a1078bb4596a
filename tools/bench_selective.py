"""Selective-prediction and temperature-scaling timings at N = 1000 rows, K = 5 classes (a validation set of KL grades):

  a. metrics.risk_coverage with R = 2000 replicates: the whole call as a user makes it -- sort tables (torch), the two gvk_risk_coverage
     launches (full sample and replicates), the device-to-host copies, the float64 finishing; wall time, the device drained before and after;
  b. the gvk_risk_coverage replicate launch alone (device events, tables prepared once);
  c. the host loop it replaces, timed in the same run on this machine's CPU: per replicate numpy resampling (rng.integers), a stable argsort
     of the resampled scores, the cumulative error count, the tie-aware aurc and the risk at the five coverages;
  d. metrics.fit_temperature: the whole call (checks, gvk_temperature_fit, the copy of its 8 doubles, the two ECE evaluations), and
     ops.temperature_fit + the copy back alone;
  e. what d replaces: Guo et al.'s temperature fit with torch.optim.LBFGS (lr 0.01, max_iter 50) on the device, float32, its result read back.

    python tools/bench_selective.py [--iters 7] [--host-replicates 2000] [--out profiles/selective_timing.txt]
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

from gaviko_amd import metrics, ops  # noqa: E402

COVERAGES = (0.5, 0.8, 0.9, 0.95, 1.0)


def host_loop(score, wrong, R, need, seed=0):
    rng = np.random.default_rng(seed)
    N = score.size
    aurc, risk = np.empty(R), np.empty((R, len(need)))
    for b in range(R):
        rows = rng.integers(0, N, N)
        s, w = score[rows], wrong[rows]
        order = np.argsort(-s, kind="stable")
        s, E = s[order], np.cumsum(w[order])
        last = np.flatnonzero(np.append(s[1:] != s[:-1], True))            # the end of every tie group
        C, Eg = last + 1, E[last]
        aurc[b] = (np.diff(C, prepend=0) * Eg / C).sum() / N
        i = np.searchsorted(C, need)
        risk[b] = Eg[i] / C[i]
    return aurc, risk


def lbfgs_temperature(logits, labels):
    """temperature_scaling.py of Guo et al. (2017): one LBFGS.step over the NLL of logits / T, T initialised to 1.5"""
    T = torch.nn.Parameter(torch.ones(1, device=logits.device) * 1.5)
    opt = torch.optim.LBFGS([T], lr=0.01, max_iter=50)
    nll = torch.nn.CrossEntropyLoss()

    def closure():
        opt.zero_grad()
        loss = nll(logits / T, labels)
        loss.backward()
        return loss

    opt.step(closure)
    return float(T.item())


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
    ap.add_argument("--host-replicates", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, K, R = 1000, 5, 2000
    g = np.random.default_rng(0)
    y = g.choice(K, N, p=[0.38, 0.18, 0.26, 0.13, 0.05]).astype(np.int64)      # unbalanced, as KL grades are
    logits = (3.0 * (g.standard_normal((N, K)) + 2.0 * np.eye(K)[y] * (g.random((N, 1)) > 0.3))).astype(np.float32)    # overconfident
    zd, yd = torch.from_numpy(logits).to(dev), torch.from_numpy(y).to(dev)
    proba = torch.softmax(zd, 1)
    score, pred = proba.max(1).values.contiguous(), proba.argmax(1).to(torch.int32)
    res = {"N": N, "K": K, "R": R}

    rc, call = timed(lambda i: metrics.risk_coverage(score, yd, pred, coverages=COVERAGES, replicates=R, seed=i), a.iters)
    tables = ops.selective_tables(score, yd)
    need = metrics.coverage_need(COVERAGES, N)
    kern = []
    for i in range(a.iters + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.risk_coverage_counts(yd, pred, tables, need, R, i, False)
        e1.record()
        torch.cuda.synchronize()
        kern.append(e0.elapsed_time(e1))
    s_h, wrong_h = score.cpu().numpy(), (pred.cpu().numpy() != y)
    host_loop(s_h, wrong_h, 5, need)
    t0 = time.perf_counter()
    aurc_h, risk_h = host_loop(s_h, wrong_h, a.host_replicates, need)
    host_ms = 1e3 * (time.perf_counter() - t0) * R / a.host_replicates
    res["risk_coverage"] = dict(call_ms=call, replicate_launch_ms=dict(median=statistics.median(kern[2:]), min=min(kern[2:]), max=max(kern[2:])),
                                host_loop_ms=host_ms, host_loop_replicates_timed=a.host_replicates, ratio_host_loop_over_call=host_ms / call["median"],
                                device=dict(aurc=rc.aurc, eaurc=rc.eaurc, aurc_ci=rc.ci["aurc"], risk_at_0_8_ci=rc.ci["risk@0.8"]),
                                host=dict(aurc_ci=[float(v) for v in np.quantile(aurc_h, [0.025, 0.975])],
                                          risk_at_0_8_ci=[float(v) for v in np.quantile(risk_h[:, 1], [0.025, 0.975])]))

    fit, fit_call = timed(lambda i: metrics.fit_temperature(zd, yd), a.iters)
    _, fit_kernel = timed(lambda i: ops.temperature_fit(zd, yd).cpu(), a.iters)
    T_lbfgs, lbfgs = timed(lambda i: lbfgs_temperature(zd, yd), a.iters)
    res["temperature"] = dict(fit_temperature_call_ms=fit_call, temperature_fit_and_copy_ms=fit_kernel, lbfgs_ms=lbfgs,
                              ratio_lbfgs_over_call=lbfgs["median"] / fit_call["median"],
                              ratio_lbfgs_over_fit_and_copy=lbfgs["median"] / fit_kernel["median"],
                              device=dict(T=fit.T, iterations=fit.iterations, converged=fit.converged, nll_before=fit.nll_before, nll_after=fit.nll_after,
                                          ece_before=fit.ece_before, ece_after=fit.ece_after),
                              lbfgs=dict(T=T_lbfgs))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/bench_selective.py --iters %d --host-replicates %d --out %s\n" % (a.iters, a.host_replicates, a.out))
            f.write("# N = 1000 rows, K = 5 classes (unbalanced, overconfident logits), one MI355X and its host CPU (one thread of Python for the host loop).\n")
            f.write("# risk_coverage.call_ms: wall time of metrics.risk_coverage with R = 2000 replicates (tables, both launches, copies back, float64\n")
            f.write("# finishing), device drained before and after; replicate_launch_ms: gvk_risk_coverage (R = 2000) alone between device events;\n")
            f.write("# host_loop_ms: numpy resampling + stable argsort + cumsum + tie-aware aurc and five risks per replicate, scaled to R if fewer were timed.\n")
            f.write("# The two sides draw different resamples (another generator): the intervals agree statistically, not bit for bit.\n")
            f.write("# temperature.fit_temperature_call_ms: wall time of metrics.fit_temperature (checks, gvk_temperature_fit, copy back, two ECE\n")
            f.write("# evaluations); temperature_fit_and_copy_ms: ops.temperature_fit and the copy of its 8 doubles; lbfgs_ms: torch.optim.LBFGS(lr=0.01,\n")
            f.write("# max_iter=50) on the device over CrossEntropyLoss(logits / T), float32, T read back (Guo et al.'s reference code; it stops at\n")
            f.write("# max_iter, short of the optimum the Newton fit reaches -- compare the two T).\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
