"""GPU box: gvk_elastic_deform (csrc/elastic.hip) on a batch of 4 raw (120,160,160) volumes with torchio's default 7 control points per axis,
every sample live -- with and without the field output -- next to gvk_spatial_transform with the affine live on the same batch (the same
8-neighbour gather without the spline) and next to the by-hand device build (three basis contractions with torch.einsum, then
F.grid_sample).  The builds alternate in one process, twice: the spread between the repeats is the noise of the comparison.
Writes profiles/elastic_timing.txt (or --out)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from gaviko_amd import data, lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elastic_timing.txt"))
args = ap.parse_args()
lib.require_device()
dev = torch.device("cuda:0")
B, shape, n = 4, (120, 160, 160), (7, 7, 7)
V = int(np.prod(shape))
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say(f"# tools/bench_elastic.py on {torch.cuda.get_device_name(0)}: B = {B} volumes of {shape}, {n} control points, every sample live.")
say("# Library launches: 50 recorded launches replayed between two device events.  By hand: device events around queued torch calls.")
torch.manual_seed(0)
x = (torch.randn(B, 1, *shape, device=dev) * 300 + 1000).contiguous()
out, field = torch.empty_like(x), torch.empty(B, 3, *shape, device=dev)
part = ops.minmax_partials(B, dev)
ops.volume_minmax(x, part)
el = data.RandomElasticDeformation()                                      # tio's defaults: 7 points, 7.5 voxels, locked borders 2
rng = np.random.default_rng(0)
coarse = np.stack([el.sample(rng) for _ in range(B)]).astype(np.float32)
ctrl = torch.from_numpy(coarse).to(dev)
live = torch.ones(B, dtype=torch.int32, device=dev)
mats = np.stack([data.affine_matrix((1.05, 0.95, 1.02), (10, -12, 14), (0, 0, 0), shape).astype(np.float32)] * B)
mats_d, fl_aff = torch.from_numpy(mats).to(dev), torch.full((B,), 8, dtype=torch.int32, device=dev)


def t_plan(name, fn, nbytes):
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
    say(f"{name:52s} {us:8.1f} us  {nbytes / us / 1e6:6.2f} TB/s algorithmic ({nbytes / 1e6:.1f} MB)")
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
    say(f"{name:52s} {us:8.1f} us  ({iters} calls)")
    return us


# ---- the by-hand device build: dense field by three basis contractions, then grid_sample (zero padding of x - min = padding with min) ----
def basis(S, k):
    """float32 [S][k], the 1-D cubic B-spline weights of csrc/elastic.hip's header comment"""
    M = k - 3
    u = (np.arange(S) + 0.5) * M / S
    i = np.minimum(np.floor(u).astype(int), M - 1)
    t = u - i
    m = np.zeros((S, k))
    for j, p in enumerate([(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6]):
        m[np.arange(S), i + j] = p
    return torch.from_numpy(m.astype(np.float32)).to(dev)


B0, B1, B2 = (basis(S, k) for S, k in zip(shape, n))
q = torch.stack(torch.meshgrid(*(torch.arange(S, device=dev, dtype=torch.float32) for S in shape), indexing="ij"), dim=-1)     # [D][H][W][3]
scale = torch.tensor([2.0 / (S - 1) for S in shape], device=dev)
mn = x.amin(dim=(1, 2, 3, 4), keepdim=True)


def by_hand():
    d = torch.einsum("zi,yj,xk,bijkc->bzyxc", B0, B1, B2, ctrl)
    g = ((q + d) * scale - 1.0).flip(-1)                                  # grid_sample wants (x, y, z) = (W, H, D) in [-1, 1]
    return F.grid_sample(x - mn, g, mode="bilinear", padding_mode="zeros", align_corners=True) + mn


def fused():
    ops.elastic_deform(x, out, ctrl, live, part)


def fused_field():
    ops.elastic_deform(x, out, ctrl, live, part, field)


def affine():
    ops.spatial_transform(x, out, mats_d, fl_aff, part)


have_hand = False
try:
    ref = by_hand()
    torch.cuda.synchronize()
except Exception as e:                                                    # the fused rows then stand alone
    say(f"by hand: does not run here ({type(e).__name__}: {e})")
else:
    fused()
    say(f"# max |fused - by hand| = {(out - ref).abs().max().item():.3e} on intensities ~1e3 (grid_sample normalises the positions to [-1, 1] in fp32)")
    del ref
    have_hand = True

ratios = []
for rep in (1, 2):
    say(f"# repeat {rep}")
    a = t_plan("gvk_spatial_transform, affine live", affine, 2 * B * V * 4)
    e = t_plan("gvk_elastic_deform", fused, 2 * B * V * 4)
    f = t_plan("gvk_elastic_deform with field", fused_field, 5 * B * V * 4)
    say(f"{'':52s} elastic / spatial = {e / a:.2f}, with field {f / a:.2f}")
    ratios.append(e / a)
    if have_hand:
        h = t_events("by hand: 3 einsum contractions + F.grid_sample", by_hand)
        t_events("gvk_elastic_deform, events", fused)
        say(f"{'':52s} by hand / fused = {h / e:.1f}")
say(f"# ratio gvk_elastic_deform / gvk_spatial_transform: {min(ratios):.2f} .. {max(ratios):.2f}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
