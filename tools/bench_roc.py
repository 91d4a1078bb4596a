"""ROC operating-point timings at N = 1000 rows (a validation set of KL grades read as "grade >= 2"), R = 2000 replicates:

  a. metrics.roc_analysis with R = 2000 replicates: the whole call as a user makes it -- sort tables (torch), the two gvk_roc_replicates
     launches (full sample with the curve, and the replicates), the device-to-host copies, the float64 finishing and DeLong's variance; wall
     time, the device drained before and after;
  b. the gvk_roc_replicates replicate launch alone (device events, tables prepared once);
  c. the gvk_risk_coverage replicate launch at the same N, R and seed, in the same run, for comparison: the kernel on the same skeleton
     (csrc/replicate.hpp), one packed scan each.  b and c alternate, launch by launch, inside every round;
  d. the host loop a replaces, timed in the same run on this machine's CPU: per replicate numpy resampling (rng.integers),
     sklearn.metrics.roc_curve(drop_intermediate=False), the trapezoid AUC, the sensitivity at two specificities, the specificity at one
     sensitivity and the Youden point.

Report only: no ratio is asked for.  Every timing is min / median / max over the rounds.

    python tools/bench_roc.py [--rounds 9] [--launches 20] [--host-replicates 2000] [--out profiles/roc_timing.txt]
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

SPECIFICITIES, SENSITIVITIES = (0.9, 0.95), (0.9,)


def host_loop(score, positive, R, seed=0):
    from sklearn.metrics import roc_curve
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    rng = np.random.default_rng(seed)
    N = score.size
    out = np.full((R, 5), np.nan)
    for b in range(R):
        rows = rng.integers(0, N, N)
        y, s = positive[rows], score[rows]
        if y.all() or not y.any():
            continue
        fpr, tpr, _ = roc_curve(y, s, drop_intermediate=False)
        out[b] = (trapezoid(tpr, fpr), tpr[1.0 - fpr >= 0.9].max(), tpr[1.0 - fpr >= 0.95].max(), 1.0 - fpr[tpr >= 0.9].min(), (tpr - fpr).max())
    return out


def spread(ms):
    return dict(min=min(ms), median=statistics.median(ms), max=max(ms))


def event_ms(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(launches):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20, help="launches per timed window of b and c")
    ap.add_argument("--host-replicates", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, K, R = 1000, 5, 2000
    g = np.random.default_rng(0)
    y = g.choice(K, N, p=[0.38, 0.18, 0.26, 0.13, 0.05]).astype(np.int64)      # unbalanced, as KL grades are
    logits = (g.standard_normal((N, K)) + 1.5 * np.eye(K)[y] * (g.random((N, 1)) > 0.3)).astype(np.float32)
    yd = torch.from_numpy(y).to(dev)
    proba = torch.softmax(torch.from_numpy(logits).to(dev), 1)
    score, positive = metrics.binary_cut(proba, yd, 2)
    score = score.contiguous()
    res = {"N": N, "K": K, "R": R, "rounds": a.rounds, "launches_per_window": a.launches}

    pos32 = positive.to(torch.int32)
    tables = ops.roc_tables(score, pos32, yd)
    spec_bp, sens_bp = [9000, 9500], [9000]
    conf, pred = proba.max(1).values.contiguous(), proba.argmax(1).to(torch.int32)
    sel_tables = ops.selective_tables(conf, yd)
    need = metrics.coverage_need((0.5, 0.8, 0.9, 0.95, 1.0), N)
    roc_launch = lambda i: ops.roc_counts(pos32, yd, tables, spec_bp, sens_bp, (), R, i, False)          # noqa: E731
    sel_launch = lambda i: ops.risk_coverage_counts(yd, pred, sel_tables, need, R, i, False)             # noqa: E731
    for warm in range(2):
        r = metrics.roc_analysis(score, positive, specificities=SPECIFICITIES, sensitivities=SENSITIVITIES, replicates=R, seed=warm, strata=yd)
        event_ms(roc_launch, 3)
        event_ms(sel_launch, 3)
    call, roc_ms, sel_ms = [], [], []
    for rnd in range(a.rounds):                                            # the three alternate inside every round
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = metrics.roc_analysis(score, positive, specificities=SPECIFICITIES, sensitivities=SENSITIVITIES, replicates=R, seed=rnd, strata=yd)
        torch.cuda.synchronize()
        call.append(1e3 * (time.perf_counter() - t0))
        roc_ms.append(event_ms(roc_launch, a.launches))
        sel_ms.append(event_ms(sel_launch, a.launches))
    s_h, p_h = score.cpu().numpy(), positive.cpu().numpy()
    host_loop(s_h, p_h, 5)
    t0 = time.perf_counter()
    host = host_loop(s_h, p_h, a.host_replicates)
    host_ms = 1e3 * (time.perf_counter() - t0) * R / a.host_replicates
    q = lambda v: [float(x) for x in np.nanquantile(v, [0.025, 0.975])]    # noqa: E731
    res["roc"] = dict(call_ms=spread(call), roc_replicate_launch_ms=spread(roc_ms), risk_coverage_replicate_launch_ms=spread(sel_ms),
                      host_loop_ms=host_ms, host_loop_replicates_timed=a.host_replicates,
                      device=dict(auc=r.auc, auc_se_delong=r.auc_se, auc_ci=r.ci["auc"], sens_at_spec_0_9=r.sensitivity_at[0.9],
                                  sens_at_spec_0_9_ci=r.ci["sens@spec=0.9"], spec_at_sens_0_9_ci=r.ci["spec@sens=0.9"], youden_j_ci=r.ci["youden_j"]),
                      host=dict(auc_ci=q(host[:, 0]), sens_at_spec_0_9_ci=q(host[:, 1]), spec_at_sens_0_9_ci=q(host[:, 3]), youden_j_ci=q(host[:, 4])))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/bench_roc.py --rounds %d --launches %d --host-replicates %d --out %s\n" % (a.rounds, a.launches, a.host_replicates, a.out))
            f.write("# N = 1000 rows, K = 5 grades (unbalanced) read as grade >= 2, R = 2000 replicates, one MI355X and its host CPU (one thread of Python\n")
            f.write("# for the host loop).  call_ms: wall time of metrics.roc_analysis (tables, both launches, copies back, float64 finishing, DeLong),\n")
            f.write("# device drained before and after; roc_replicate_launch_ms / risk_coverage_replicate_launch_ms: gvk_roc_replicates and\n")
            f.write("# gvk_risk_coverage (R = 2000, same N and seeds) alone between device events, per launch over a window of back-to-back launches\n")
            f.write("# (the wrapper's allocations and level upload included), the three measured in turn inside every round; min / median / max\n")
            f.write("# over the rounds.  host_loop_ms: numpy resampling + sklearn roc_curve + five read-offs per replicate, scaled to R if fewer were\n")
            f.write("# timed.  The two sides draw different resamples (another generator): the intervals agree statistically, not bit for bit.\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
