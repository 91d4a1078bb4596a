"""GPU box: the normalisers of csrc/normalize.hip on a batch of 4 raw (120,160,160) volumes -- the percentile rescale
(RescaleIntensity((0, 1), percentiles=(0.5, 99.5))) and the z-normalisation above the mean (ZNormalization('mean')) -- on an all-distinct
batch and on a batch with 60 % exact zeros, next to today's min-max pair (gvk_volume_minmax + gvk_rescale_intensity) and next to the
by-hand device build (torch.quantile per volume + clamp + arithmetic; x[mask].mean() / .std()).  The builds alternate in one process,
twice: the spread between the repeats is the noise of the comparison.  Each library path is also split into its calls.  The byte time
is the bytes each path has to move (every pass reads the batch once, the apply pass also writes it) at the rate the min-max pair's
rescale kernel reaches in the same run.  Writes profiles/normalize_timing.txt (or --out)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gaviko_amd import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize_timing.txt"))
args = ap.parse_args()
lib.require_device()
dev = torch.device("cuda:0")
B, shape = 4, (120, 160, 160)
V = int(np.prod(shape))
MB = B * V * 4 / 1e6                                                      # one pass over the batch
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say(f"# tools/bench_normalize.py on {torch.cuda.get_device_name(0)}: B = {B} volumes of {shape}, {MB:.1f} MB per pass over the batch.")
say("# Library paths: 50 recorded launches replayed between two device events.  By hand: device events around queued torch calls.")
torch.manual_seed(0)
batches = {"all distinct": (torch.randn(B, 1, *shape, device=dev) * 300 + 1000).contiguous()}
z = torch.randn(B, 1, *shape, device=dev).abs() * 500 + 1
batches["60 % zeros"] = torch.where(torch.rand(B, 1, *shape, device=dev) < 0.6, torch.zeros_like(z), z).contiguous()
out = torch.empty(B, 1, *shape, device=dev)
part = ops.minmax_partials(B, dev)
stats = torch.empty(B, ops.NORMALIZE_STATS, dtype=torch.float64, device=dev)
count = torch.empty(B, dtype=torch.int64, device=dev)
spart = torch.empty(B * ops.NORMALIZE_SLABS * 4, dtype=torch.float64, device=dev)
ws = torch.empty(B * ops.NORMALIZE_ORDER_WS_WORDS, dtype=torch.int32, device=dev)
pairs, cutoffs = torch.empty(B, 2, 2, device=dev), torch.empty(B, 2, device=dev)
status, params = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, 8, dtype=torch.float64, device=dev)
Q = (0.5, 99.5)


def t_plan(name, fn, passes):
    for _ in range(3):
        fn()
    l = lib.load()
    lib.check(l.gvk_plan_begin(), "begin")
    for _ in range(50):
        fn()
    pid = l.gvk_plan_end()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    l.gvk_plan_replay(pid)
    e0.record(); l.gvk_plan_replay(pid); e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 50
    say(f"{name:60s} {us:8.1f} us  {passes * MB / us:6.2f} TB/s algorithmic ({passes} passes, {passes * MB:.0f} MB)")
    l.gvk_plan_free(pid)
    return us


def t_events(name, fn, seconds=0.3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        fn()
    e1.record(); torch.cuda.synchronize()
    iters = max(10, int(seconds * 1e3 / max(e0.elapsed_time(e1) / 3, 1e-3)))
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    say(f"{name:60s} {us:8.1f} us  ({iters} calls)")
    return us


for label, x in batches.items():
    def minmax_only():
        ops.volume_minmax(x, part)

    def rescale_only():
        ops.rescale_intensity(x, part, out, 0.0, 1.0)

    def minmax_pair():
        ops.volume_minmax(x, part)
        ops.rescale_intensity(x, part, out, 0.0, 1.0)

    def stats_plain():
        ops.volume_stats(x, None, want_std=False, stats=stats, count=count, partials=spart)

    def order():
        ops.volume_order_stats(x, stats, Q, pairs=pairs, cutoffs=cutoffs, workspace=ws)

    def apply_rescale():
        ops.normalize_intensity(x, out, stats, ops.NORMALIZE_RESCALE, cutoffs, 0.0, 1.0, status=status, params=params)

    def percentile():
        stats_plain(); order(); apply_rescale()

    def stats_mean():
        ops.volume_stats(x, "mean", want_std=True, stats=stats, count=count, partials=spart)

    def apply_znorm():
        ops.normalize_intensity(x, out, stats, ops.NORMALIZE_ZNORM, status=status, params=params)

    def znorm():
        stats_mean(); apply_znorm()

    def hand_percentile():
        flat = x.reshape(B, -1)
        ys = []
        for b in range(B):
            c = torch.quantile(flat[b], torch.tensor([0.005, 0.995], device=dev))
            t = flat[b].clamp(c[0], c[1])
            ys.append((t - c[0]) / (c[1] - c[0]))
        return torch.stack(ys)

    def hand_znorm():
        flat = x.reshape(B, -1)
        ys = []
        for b in range(B):
            v = flat[b][flat[b] > flat[b].mean()]
            ys.append((flat[b] - v.mean()) / v.std())
        return torch.stack(ys)

    say()
    say(f"## {label}")
    percentile()
    ref = hand_percentile()
    say(f"# max |percentile path - by hand| = {(out.reshape(B, -1) - ref).abs().max().item():.3e} (torch.quantile interpolates in float32), status {status.tolist()}")
    znorm()
    ref = hand_znorm()
    say(f"# max |znorm path - by hand| = {(out.reshape(B, -1) - ref).abs().max().item():.3e}, status {status.tolist()}")
    del ref
    for rep in (1, 2):
        say(f"# repeat {rep}")
        t_plan("gvk_volume_minmax", minmax_only, 1)
        r = t_plan("gvk_rescale_intensity", rescale_only, 2)
        rate = 2 * MB / r                                                 # MB per us of the streaming rescale, this run
        m = t_plan("min-max pair", minmax_pair, 3)
        stats_plain()
        a = t_plan("  gvk_volume_stats, no mask, no std (1 read)", stats_plain, 1)
        o = t_plan("  gvk_volume_order_stats, 2 percentiles (3 reads)", order, 3)
        w = t_plan("  gvk_normalize_intensity, rescale (1 read, 1 write)", apply_rescale, 2)
        p = t_plan("percentile rescale (0.5, 99.5): the three calls", percentile, 6)
        say(f"{'':60s} byte time at the rescale kernel's rate {6 * MB / rate:.1f} us: measured / byte time = {p / (6 * MB / rate):.2f}; "
            f"calls {a / (MB / rate):.2f} / {o / (3 * MB / rate):.2f} / {w / (2 * MB / rate):.2f}; percentile / min-max pair = {p / m:.2f}")
        stats_mean()
        s3 = t_plan("  gvk_volume_stats, 'mean' mask, std (3 reads)", stats_mean, 3)
        wz = t_plan("  gvk_normalize_intensity, znorm (1 read, 1 write)", apply_znorm, 2)
        zt = t_plan("z-normalisation above the mean: the two calls", znorm, 5)
        say(f"{'':60s} byte time {5 * MB / rate:.1f} us: measured / byte time = {zt / (5 * MB / rate):.2f}; calls {s3 / (3 * MB / rate):.2f} / "
            f"{wz / (2 * MB / rate):.2f}; znorm / min-max pair = {zt / m:.2f}")
        hp = t_events("by hand: torch.quantile per volume + clamp + arithmetic", hand_percentile)
        hz = t_events("by hand: x[x > x.mean()].mean() / .std() per volume", hand_znorm)
        say(f"{'':60s} by hand / library: percentile {hp / p:.1f}, znorm {hz / zt:.1f}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
