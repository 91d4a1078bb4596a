"""GPU box: data.Conform (csrc/conform.hip) on a ragged batch of 4 volumes of unequal shape near (144, 384, 384) at about 0.7 x 0.37 x 0.37 mm,
onto (120, 160, 160): crop / pad only, linear resampling to 0.84 x 0.888 x 0.888 mm, and the same with antialiasing.  Each row is set
against two yardsticks: the byte time of reading the packed input once and writing the output once at the HBM peak, and the same result
built by hand on the device per sample -- a conv3d Gaussian per shrinking axis (edge replicated), F.interpolate(trilinear,
align_corners=False) at the given scale, slicing / F.pad to the target -- then torch.stack.  Three timings per row: the launches
alone (tables uploaded once, `ops.conform_prepare(...).run()`), the whole `Conform.__call__` (host tables, uploads, launches) and the
by-hand build; device events around queued calls after a warm-up, the median of five windows.  The packed input alone is 341 MB, more than
the 256 MB Infinity Cache, so every launch reads HBM.  Writes profiles/conform_timing.txt (or --out).  Without a GPU it says so and exits 0."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conform_timing.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    print("tools/bench_conform.py: no GPU visible; nothing measured (the timings need an MI355X)")
    sys.exit(0)

from gaviko_amd import lib, ops  # noqa: E402
from gaviko_amd.data import Conform, CropOrPad, Resample, collate_ragged, conform_tables  # noqa: E402

lib.require_device()
dev = torch.device("cuda:0")
N = (120, 160, 160)
SHAPES = [(144, 384, 384), (140, 376, 380), (150, 390, 372), (136, 384, 400)]
SPACING = [(0.7, 0.37, 0.37), (0.72, 0.38, 0.37), (0.68, 0.36, 0.38), (0.74, 0.37, 0.36)]
TARGET = (0.84, 0.888, 0.888)
HBM_TBS = 8.0                                                             # MI355X peak HBM3E bandwidth
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


rng = np.random.default_rng(0)
vols = [torch.from_numpy((100.0 + 30.0 * rng.standard_normal(s, dtype=np.float32))) for s in SHAPES]
ragged = collate_ragged([(v, s) for v, s in zip(vols, SPACING)]).to(dev)
dvols = [ragged.volume(b) for b in range(len(vols))]
v_in, v_out = sum(int(np.prod(s)) for s in SHAPES), len(SHAPES) * int(np.prod(N))
byte_us = (v_in + v_out) * 4 / (HBM_TBS * 1e6)
say(f"# tools/bench_conform.py on {torch.cuda.get_device_name(0)}: {len(SHAPES)} volumes {SHAPES} at {SPACING} mm onto {N}.")
say(f"# byte time at {HBM_TBS} TB/s: the packed input read once ({v_in * 4 / 1e6:.1f} MB) + the output written once ({v_out * 4 / 1e6:.1f} MB) = {byte_us:.1f} us.")
say("# Device events around queued calls after a warm-up; the median of five windows (min..max).")


def timed(fn, calls=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    meds = []
    for _ in range(5):
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        meds.append(e0.elapsed_time(e1) * 1e3 / calls)
    return float(np.median(meds)), min(meds), max(meds)


def gauss1d(r):
    sigma = math.sqrt((r * r - 1.0) / (8.0 * math.log(2.0)))
    radius = int(4.0 * sigma + 0.5)
    k = torch.arange(-radius, radius + 1, dtype=torch.float64)
    w = torch.exp(-0.5 * (k / sigma) ** 2)
    return (w / w.sum()).float().to(dev), radius


def by_hand(resample, antialias):
    outs = []
    for v, shape, spacing in zip(dvols, SHAPES, SPACING):
        x = v[None, None]
        if resample:
            r = [t / s for t, s in zip(TARGET, spacing)]
            m = [max(1, int(math.floor(n / f + 1e-9))) for n, f in zip(shape, r)]
            if antialias:
                for a in range(3):
                    if r[a] > 1.0:
                        w, radius = gauss1d(r[a])
                        pad, kshape = [0] * 6, [1, 1, 1, 1, 1]
                        pad[2 * (2 - a)] = pad[2 * (2 - a) + 1] = radius
                        kshape[2 + a] = 2 * radius + 1
                        x = F.conv3d(F.pad(x, pad, mode="replicate"), w.view(kshape))
            # the positions are (u + 0.5) r - 0.5 with r = target / spacing (not n / m): the scale is given, not recomputed from the sizes
            x = F.interpolate(x, scale_factor=[1.0 / f for f in r], mode="trilinear", align_corners=False, recompute_scale_factor=False)
            assert list(x.shape[2:]) == m, (list(x.shape[2:]), m)
        x = x[0, 0]
        for a in range(3):                                                # CropOrPad: ceil in front, floor behind
            d = N[a] - x.shape[a]
            if d < 0:
                x = x.narrow(a, (1 - d) // 2, N[a])
            elif d > 0:
                pad = [0] * 6
                pad[2 * (2 - a)], pad[2 * (2 - a) + 1] = -(-d // 2), d // 2
                x = F.pad(x, pad)
        outs.append(x)
    return torch.stack(outs).unsqueeze(1)


cases = (("crop / pad only", [CropOrPad(N)], False, False),
         ("linear", [Resample(TARGET, "linear", antialias=False), CropOrPad(N)], True, False),
         ("linear + antialias", [Resample(TARGET, "linear", antialias=True), CropOrPad(N)], True, True))
shapes_h, offsets_h = ragged.shapes.numpy(), ragged.offsets.numpy()
for rep in (1, 2):
    say(f"# repeat {rep}")
    for name, stages, resample, antialias in cases:
        conform = Conform(stages)
        t = conform_tables(shapes_h, ragged.spacing.numpy(), stages, N)
        launch = ops.conform_prepare(ragged.data, offsets_h, shapes_h, t.start, t.weights, t.inside, t.taps, N)
        plan = ops.conform_plan(shapes_h, N, t.start, t.weights, t.inside.astype(np.int32), t.taps)
        if rep == 1:
            diff = (launch.run() - by_hand(resample, antialias)[:, 0]).abs().max().item()
            say(f"# {name}: {plan['npass']} passes, {int(t.taps.max())} taps at most, {plan['scratch'] * 4 / 1e6:.1f} MB of intermediates; "
                f"max |library - by hand| = {diff:.3e}")
        k = timed(launch.run)
        c = timed(lambda: conform(ragged))
        h = timed(lambda: by_hand(resample, antialias), calls=3)
        say(f"{name:20s} launches alone {k[0]:8.1f} us ({k[1]:.1f}..{k[2]:.1f})  = {k[0] / byte_us:5.2f} x byte time")
        say(f"{'':20s} Conform call   {c[0]:8.1f} us ({c[1]:.1f}..{c[2]:.1f})  host tables, uploads and launches")
        say(f"{'':20s} by hand        {h[0]:8.1f} us ({h[1]:.1f}..{h[2]:.1f})  by hand / launches = {h[0] / k[0]:.2f}, by hand / Conform call = {h[0] / c[0]:.2f}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
