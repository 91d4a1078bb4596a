"""GPU box: gvk_batch_mix (csrc/batchmix.hip) on a batch of 4 normalised (120,160,160) volumes -- every sample a copy, every sample Mixup,
every sample CutMix (a box of half the volume, its w-range off the 16-byte grid) -- each next to its byte time (2 V floats per copy or
CutMix sample, 3 V per Mixup sample, at the HBM rate below) and next to the by-hand device build of the same result: x.clone(),
lam * x + (1 - lam) * x[perm], and a clone with the slice-assigned box paste per sample.  The builds alternate in one process, twice: the
spread between the repeats is the noise of the comparison.  Every build rotates through 8 input / output pairs (786 MB), more than the
256 MB Infinity Cache holds, so that a repeated launch reads HBM and not the cache.  Writes profiles/batchmix_timing.txt (or --out)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gaviko_amd import lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batchmix_timing.txt"))
args = ap.parse_args()
lib.require_device()
dev = torch.device("cuda:0")
B, shape = 4, (120, 160, 160)
D, H, W = shape
V = int(np.prod(shape))
HBM_TBS = 8.0                                                             # MI355X peak HBM3E bandwidth
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say(f"# tools/bench_batchmix.py on {torch.cuda.get_device_name(0)}: B = {B} volumes of {shape}, every sample in the named mode.")
say("# Library launches: 50 recorded launches replayed between two device events.  By hand: device events around queued torch calls.")
say("# Every build rotates through 8 input / output pairs (786 MB > the 256 MB Infinity Cache): the reads come from HBM.")
say(f"# byte time at {HBM_TBS} TB/s: 2 V floats per copy / CutMix sample = {2 * B * V * 4 / 1e6:.1f} MB, 3 V per Mixup sample = {3 * B * V * 4 / 1e6:.1f} MB.")
torch.manual_seed(0)
ROT = 8                                                                   # input / output pairs in rotation: 8 x 98 MB > the 256 MB Infinity Cache
xs = [torch.rand(B, 1, *shape, device=dev).contiguous() for _ in range(ROT)]
outs = [torch.empty_like(xs[0]) for _ in range(ROT)]
x, out = xs[0], outs[0]
turn = [0]


def nxt():
    turn[0] = (turn[0] + 1) % ROT
    return xs[turn[0]], outs[turn[0]]


perm_h = np.array([1, 2, 3, 0], np.int32)
lam_h = np.array([0.3, 0.5, 0.7, 0.9], np.float32)
box_h = np.tile(np.array([30, 90, 20, 140, 13, 147], np.int32), (B, 1))   # (60, 120, 134): 49 % of the volume; w0, w1 odd
perm, lam, box = [torch.from_numpy(t).to(dev) for t in (perm_h, lam_h, box_h)]
perm64, lam5 = perm.long(), lam.view(B, 1, 1, 1, 1)
modes = {name: torch.full((B,), m, dtype=torch.int32, device=dev) for name, m in (("copy", ops.MIX_COPY), ("Mixup", ops.MIX_MIXUP),
                                                                                   ("CutMix", ops.MIX_CUTMIX))}


def lib_call(mode, rotate=True):
    def run():
        xi, oi = nxt() if rotate else (x, out)
        lib.check(lib.load().gvk_batch_mix(lib.ptr(xi), lib.ptr(oi), lib.ptr(mode), lib.ptr(lam), lib.ptr(perm), lib.ptr(box), B, D, H, W,
                                           lib.stream_ptr()), "gvk_batch_mix")
    return run


def hand_copy(x=None):
    x = nxt()[0] if x is None else x
    return x.clone()


def hand_mixup(x=None):
    x = nxt()[0] if x is None else x
    return lam5 * x + (1 - lam5) * x[perm64]


def hand_cutmix(x=None):
    x = nxt()[0] if x is None else x
    y = x.clone()
    for b in range(B):
        d0, d1, h0, h1, w0, w1 = box_h[b]
        y[b, :, d0:d1, h0:h1, w0:w1] = x[perm_h[b], :, d0:d1, h0:h1, w0:w1]
    return y


def t_plan(name, fn, byte_us):
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
    meds = []
    for _ in range(5):                                                    # the median of five replays of 50 launches
        e0.record(); l.gvk_plan_replay(pid); e1.record(); torch.cuda.synchronize()
        meds.append(e0.elapsed_time(e1) * 1e3 / 50)
    us = float(np.median(meds))
    say(f"{name:44s} {us:8.1f} us  (five replays {min(meds):.1f}..{max(meds):.1f})  byte time {byte_us:5.1f} us ({us / byte_us:4.2f}x)")
    l.gvk_plan_free(pid)
    return us


def t_events(name, fn, seconds=0.3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        fn()
    e1.record(); torch.cuda.synchronize()
    iters = max(20, int(seconds * 1e3 / max(e0.elapsed_time(e1) / 5, 1e-3)))
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    say(f"{name:44s} {us:8.1f} us  ({iters} calls)")
    return us


# ---- agreement of the two builds ----
for name, hand in (("copy", hand_copy), ("Mixup", hand_mixup), ("CutMix", hand_cutmix)):
    out.fill_(float("nan"))
    lib_call(modes[name], rotate=False)()
    say(f"# {name}: max |library - by hand| = {(out - hand(x)).abs().max().item():.3e}")

cases = (("copy", hand_copy, "by hand: x.clone()", 2), ("Mixup", hand_mixup, "by hand: lam * x + (1 - lam) * x[perm]", 3),
         ("CutMix", hand_cutmix, "by hand: clone + slice-assigned paste", 2))
for rep in (1, 2):
    say(f"# repeat {rep}")
    for name, hand, label, floats in cases:
        us = t_plan(f"gvk_batch_mix, all {name}", lib_call(modes[name]), floats * B * V * 4 / (HBM_TBS * 1e6))
        h = t_events(label, hand)
        say(f"{'':44s} by hand / library = {h / us:.2f}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
