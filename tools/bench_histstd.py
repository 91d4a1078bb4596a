"""GPU box: histogram standardisation (gvk_volume_landmarks, gvk_histogram_standardize) on a batch of 4 raw (120,160,160) volumes
resident in HBM, an all-distinct batch and a batch with 60 % exact zeros.  Three rows, every one against its counterpart in the same run:

(a) ONE gvk_volume_landmarks launch at the 13 training percentiles (4 sweeps over the batch) against the way the same 13 numbers were
    got before it existed: four gvk_volume_order_stats calls of 4 + 4 + 4 + 1 percentiles (3 passes each, a pass sweeping twice when its
    ranks fall under more than 4 prefixes).  The outputs are compared bit for bit first.
(b) the apply pass of gvk_histogram_standardize (1 read, 1 write) over its byte time, the bytes at the rate gvk_rescale_intensity -- the
    same two streams -- reaches in the same run.
(c) the whole transform (gvk_volume_stats + landmarks at 11 percentiles + apply) against a by-hand device build: torch.quantile per
    volume, torch.bucketize on the interior knots, gathered slopes and intercepts.

Library paths are 20 recorded launches replayed between two device events, the by-hand build is device events around queued torch calls;
all rows are timed in interleaved rounds and reported as the median and the range over the rounds.  Writes profiles/histstd_timing.txt
(or --out)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gaviko_amd import data, lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "histstd_timing.txt"))
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()
lib.require_device()
dev = torch.device("cuda:0")
B, shape = 4, (120, 160, 160)
V = int(np.prod(shape))
MB = B * V * 4 / 1e6                                                      # one pass over the batch
REPLAYS = 20
lines, plans = [], []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say(f"# tools/bench_histstd.py on {torch.cuda.get_device_name(0)}: B = {B} volumes of {shape}, {MB:.1f} MB per pass over the batch.")
say(f"# Library rows: {REPLAYS} recorded launches replayed between two device events; by hand: device events around queued torch calls.")
say(f"# {args.rounds} interleaved rounds per batch; every figure is the median [minimum .. maximum] over the rounds, in us per call.")
torch.manual_seed(0)
batches = {"all distinct": (torch.randn(B, 1, *shape, device=dev) * 300 + 1000).contiguous()}
z = torch.randn(B, 1, *shape, device=dev).abs() * 500 + 1
batches["60 % zeros"] = torch.where(torch.rand(B, 1, *shape, device=dev) < 0.6, torch.zeros_like(z), z).contiguous()
del z
out = torch.empty(B, 1, *shape, device=dev)
part = ops.minmax_partials(B, dev)
stats = torch.empty(B, ops.NORMALIZE_STATS, dtype=torch.float64, device=dev)
count = torch.empty(B, dtype=torch.int64, device=dev)
spart = torch.empty(B * ops.NORMALIZE_SLABS * 4, dtype=torch.float64, device=dev)
ws_old = torch.empty(B * ops.NORMALIZE_ORDER_WS_WORDS, dtype=torch.int32, device=dev)
ws_new = torch.empty(B * ops.LANDMARKS_WS_WORDS, dtype=torch.int32, device=dev)
Q13 = data.landmark_percentiles().tolist()
Q11 = [Q13[i] for i in data.LANDMARK_APPLY_INDEX]
GROUPS = [Q13[i:i + 4] for i in range(0, 13, 4)]
pairs13, cut13 = torch.empty(B, 13, 2, device=dev), torch.empty(B, 13, device=dev)
pairs11, cut11 = torch.empty(B, 11, 2, device=dev), torch.empty(B, 11, device=dev)
old_out = [(torch.empty(B, len(g), 2, device=dev), torch.empty(B, len(g), device=dev)) for g in GROUPS]
status, params = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, ops.HISTSTD_PARAMS, dtype=torch.float64, device=dev)
TARGETS = np.linspace(0.0, 100.0, 13)[list(data.LANDMARK_APPLY_INDEX)]


def plan(fn):
    for _ in range(3):
        fn()
    l = lib.load()
    lib.check(l.gvk_plan_begin(), "begin")
    for _ in range(REPLAYS):
        fn()
    pid = l.gvk_plan_end()
    plans.append(pid)
    torch.cuda.synchronize()
    l.gvk_plan_replay(pid)
    torch.cuda.synchronize()

    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); l.gvk_plan_replay(pid); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / REPLAYS
    return run


def events(fn, calls=3):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()

    def run():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls
    return run


def fmt(v):
    return f"{statistics.median(v):8.1f} us [{min(v):7.1f} .. {max(v):7.1f}]"


failed = False
for label, x in batches.items():
    def landmarks13():
        ops.volume_landmarks(x, stats, Q13, pairs=pairs13, cutoffs=cut13, workspace=ws_new)

    def four_calls():
        for g, (p, c) in zip(GROUPS, old_out):
            ops.volume_order_stats(x, stats, g, pairs=p, cutoffs=c, workspace=ws_old)

    def rescale_only():
        ops.rescale_intensity(x, part, out, 0.0, 1.0)

    def apply_only():
        ops.histogram_standardize(x, out, stats, cut11, TARGETS, 1e-5, status=status, params=params)

    def whole():
        ops.volume_stats(x, None, want_std=False, stats=stats, count=count, partials=spart)
        ops.volume_landmarks(x, stats, Q11, pairs=pairs11, cutoffs=cut11, workspace=ws_new)
        ops.histogram_standardize(x, out, stats, cut11, TARGETS, 1e-5, status=status, params=params)

    qd, md = torch.tensor(Q11, device=dev, dtype=torch.float32) / 100, torch.tensor(TARGETS, device=dev, dtype=torch.float64)

    def by_hand():
        flat = x.reshape(B, -1)
        ys = []
        for b in range(B):
            k = torch.quantile(flat[b], qd)
            d = (k[1:] - k[:-1]).double()
            d = torch.where(d < 1e-5, torch.full_like(d, float("inf")), d)
            slope = (md[1:] - md[:-1]) / d
            icpt = md[:-1] - slope * k[:-1].double()
            j = torch.bucketize(flat[b], k[1:-1], right=True)
            ys.append((slope[j] * flat[b].double() + icpt[j]).float())
        return torch.stack(ys)

    say()
    say(f"## {label}")
    ops.volume_minmax(x, part)
    ops.volume_stats(x, None, want_std=False, stats=stats, count=count, partials=spart)
    landmarks13(); four_calls()
    same = torch.equal(pairs13.view(torch.int32), torch.cat([p for p, _ in old_out], 1).view(torch.int32)) and \
        torch.equal(cut13.view(torch.int32), torch.cat([c for _, c in old_out], 1).view(torch.int32))
    say(f"# the 13 landmarks of one launch and of the four calls are bit-identical: {same}")
    whole()
    ref = by_hand()
    say(f"# max |whole transform - by hand| = {(out.reshape(B, -1) - ref).abs().max().item():.3e} (torch.quantile interpolates in float32), "
        f"status {status.tolist()}")
    del ref
    rows = dict(new=plan(landmarks13), old=plan(four_calls), rescale=plan(rescale_only), apply=plan(apply_only), whole=plan(whole), hand=events(by_hand))
    t = {k: [] for k in rows}
    for _ in range(args.rounds):
        for k, run in rows.items():
            t[k].append(run())
    ratio_a = [n / o for n, o in zip(t["new"], t["old"])]
    ratio_b = [a / r for a, r in zip(t["apply"], t["rescale"])]                 # both move 2 passes: the ratio of times is the ratio to the byte time
    ratio_c = [h / w for h, w in zip(t["hand"], t["whole"])]
    say(f"(a) gvk_volume_landmarks, 13 percentiles, one launch (4 sweeps)      {fmt(t['new'])}  {4 * MB / statistics.median(t['new']):5.2f} TB/s algorithmic")
    say(f"(a) four gvk_volume_order_stats calls, 4 + 4 + 4 + 1 percentiles     {fmt(t['old'])}")
    say(f"    one launch / four calls, round by round: median {statistics.median(ratio_a):.3f} [{min(ratio_a):.3f} .. {max(ratio_a):.3f}]"
        f" -- {'not slower in any round' if max(ratio_a) <= 1.0 else 'SLOWER in at least one round'}")
    say(f"(b) gvk_histogram_standardize, apply (1 read, 1 write)               {fmt(t['apply'])}  {2 * MB / statistics.median(t['apply']):5.2f} TB/s")
    say(f"(b) gvk_rescale_intensity, the same two streams (the byte rate)      {fmt(t['rescale'])}  {2 * MB / statistics.median(t['rescale']):5.2f} TB/s")
    say(f"    apply / byte time, round by round: median {statistics.median(ratio_b):.2f} [{min(ratio_b):.2f} .. {max(ratio_b):.2f}]")
    say(f"(c) whole transform: statistics + 11 landmarks + apply (6 passes)    {fmt(t['whole'])}")
    say(f"(c) by hand: torch.quantile + torch.bucketize + gather per volume    {fmt(t['hand'])}")
    say(f"    by hand / library, round by round: median {statistics.median(ratio_c):.1f} [{min(ratio_c):.1f} .. {max(ratio_c):.1f}]")
    while plans:
        lib.load().gvk_plan_free(plans.pop())
    failed = failed or not same or statistics.median(ratio_a) > 1.0
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
sys.exit(1 if failed else 0)
