"""GPU box: the kernels of csrc/kspace.hip on a batch of 4 raw (120,160,160) volumes, every sample live -- gvk_axis_circular_conv once per
axis (RandomGhosting), gvk_gamma_spike as gamma and as four spikes (with and without the gvk_volume_stats launch the spikes need),
gvk_axis_gather2 once per axis (RandomAnisotropy) -- each next to its byte time (one read and one write of the batch at the HBM rate
below), the convolution also next to its matrix-pipe time at 2 N flops per voxel, and next to the by-hand device build of the same result:
torch.fft.fftn / mask / ifftn for ghosting and spikes, torch.pow for gamma.  The builds alternate in one process, twice: the spread between
the repeats is the noise of the comparison.  Also measures powf's largest error in ulps, the figure tests/test_kspace_augment_gpu.py derives
its gamma bound from.  Writes profiles/kspace_timing.txt (or --out)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gaviko_amd import data, lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kspace_timing.txt"))
args = ap.parse_args()
lib.require_device()
dev = torch.device("cuda:0")
B, shape = 4, (120, 160, 160)
V = int(np.prod(shape))
HBM_TBS, MATRIX_TFLOPS = 8.0, 157.3                                       # MI355X peaks: HBM3E bandwidth, f32-input matrix cores
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say(f"# tools/bench_kspace.py on {torch.cuda.get_device_name(0)}: B = {B} volumes of {shape}, every sample live.")
say("# Library launches: 50 recorded launches replayed between two device events.  By hand: device events around queued torch calls.")
say(f"# byte time = {2 * B * V * 4 / 1e6:.1f} MB at {HBM_TBS} TB/s; matrix-pipe time = 2 N flops per voxel at {MATRIX_TFLOPS} TFLOP/s.")
torch.manual_seed(0)
x = (torch.randn(B, 1, *shape, device=dev) * 300 + 1000).contiguous()
out = torch.empty_like(x)
live = torch.ones(B, dtype=torch.int32, device=dev)
byte_us = 2 * B * V * 4 / (HBM_TBS * 1e6)


def t_plan(name, fn, flops=0):
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
    pipe = f", matrix-pipe time {flops / (MATRIX_TFLOPS * 1e6):6.1f} us ({us * MATRIX_TFLOPS * 1e6 / flops:4.1f}x)" if flops else ""
    say(f"{name:52s} {us:8.1f} us  byte time {byte_us:5.1f} us ({us / byte_us:4.1f}x){pipe}")
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


# ---- tables ----
n_ghosts, g = 6, 0.8
ghost = {}
for a in range(3):
    N = shape[a]
    ctab = torch.from_numpy(data.ghosting_tables([n_ghosts] * B, [g] * B, [N] * B)).to(dev)
    mask = torch.ones(N, device=dev)
    mask[::n_ghosts] = 1 - g
    mask[N // 2] = 1
    ghost[a] = (ctab, torch.full((B,), a, dtype=torch.int32, device=dev), mask.reshape([-1 if i == a else 1 for i in range(3)]))
positions = np.random.default_rng(0).random((B, ops.SPIKE_MAX, 3))
tab = torch.from_numpy(np.stack([data.spike_tables(p, shape) for p in positions])).to(dev)
amp, nsp = torch.full((B,), 2.0, device=dev), torch.full((B,), ops.SPIKE_MAX, dtype=torch.int32, device=dev)
gam = torch.full((B,), float(np.exp(0.3)), device=dev)
k_gamma = torch.full((B,), ops.KSPACE_GAMMA, dtype=torch.int32, device=dev)
k_spike = torch.full((B,), ops.KSPACE_SPIKE, dtype=torch.int32, device=dev)
stats, count = ops.volume_stats(x, None, want_std=False)
stat_part = torch.empty(B * ops.NORMALIZE_SLABS * 4, dtype=torch.float64, device=dev)
aniso = {}
for a in range(3):
    s, w = data.anisotropy_tables(3.0, shape[a], max(shape))
    aniso[a] = (torch.from_numpy(np.stack([s] * B)).to(dev), torch.from_numpy(np.stack([w] * B)).to(dev),
                torch.full((B,), a, dtype=torch.int32, device=dev))
spike_idx = [[[min(int(p * n), n - 1) for p, n in zip(row, shape)] for row in positions[b]] for b in range(B)]
xs = x[:, 0]


def ghost_lib(a):
    return lambda: ops.axis_circular_conv(x, out, ghost[a][0], ghost[a][1], live)


def ghost_hand(a):
    def run():
        spec = torch.fft.fftshift(torch.fft.fftn(xs, dim=(1, 2, 3)), dim=(1, 2, 3)) * ghost[a][2]
        return torch.fft.ifftn(torch.fft.ifftshift(spec, dim=(1, 2, 3)), dim=(1, 2, 3)).real
    return run


def spike_lib():
    ops.gamma_spike(x, out, k_spike, gam, amp, nsp, tab, stats)


def spike_lib_with_stats():
    ops.volume_stats(x, None, want_std=False, stats=stats, count=count, partials=stat_part)
    ops.gamma_spike(x, out, k_spike, gam, amp, nsp, tab, stats)


def spike_hand():
    spec = torch.fft.fftshift(torch.fft.fftn(xs, dim=(1, 2, 3)), dim=(1, 2, 3))
    a = 2.0 * xs.mean(dim=(1, 2, 3)).abs() * V
    for b in range(B):
        for k in spike_idx[b]:
            spec[b, k[0], k[1], k[2]] += a[b]
    return torch.fft.ifftn(torch.fft.ifftshift(spec, dim=(1, 2, 3)), dim=(1, 2, 3)).real


def gamma_lib():
    ops.gamma_spike(x, out, k_gamma, gam, amp, nsp, tab, stats)


def gamma_hand():
    return torch.sign(x) * torch.pow(x.abs(), gam.view(B, 1, 1, 1, 1))


def aniso_lib(a):
    return lambda: ops.axis_gather2(x, out, aniso[a][0], aniso[a][1], aniso[a][2], live)


# ---- agreement of the two builds (fp32 FFT on intensities ~1e3 against an exact-operand product) ----
for a in range(3):
    ghost_lib(a)()
    say(f"# ghosting axis {a}: max |library - by hand| = {(out[:, 0] - ghost_hand(a)()).abs().max().item():.3e}")
spike_lib()
say(f"# spikes: max |library - by hand| = {(out[:, 0] - spike_hand()).abs().max().item():.3e}")
gamma_lib()
say(f"# gamma: max |library - by hand| = {(out - gamma_hand()).abs().max().item():.3e}")

# ---- powf against float64: the figure the test bound derives from ----
xg = np.exp(np.random.default_rng(60).uniform(np.log(1e-6), np.log(4e3), (2, 1, 8, 64, 256))).astype(np.float32)
gg = np.array([np.exp(-0.3), np.exp(0.3)], np.float32)
xt, og = torch.from_numpy(xg).to(dev), torch.empty(2, 1, 8, 64, 256, device=dev)
ops.gamma_spike(xt, og, k_gamma[:2].contiguous(), torch.from_numpy(gg).to(dev), amp[:2].contiguous(), nsp[:2].contiguous(),
                torch.zeros(2, ops.SPIKE_MAX, 2, 8 + 64 + 256, device=dev), stats[:2].contiguous())
ref = np.power(xg.astype(np.float64), gg.astype(np.float64).reshape(2, 1, 1, 1, 1))
ulps = np.abs(og.cpu().numpy().astype(np.float64) - ref) / np.spacing(ref.astype(np.float32)).astype(np.float64)
say(f"# gamma: largest error of powf against float64 np.power over x in [1e-6, 4e3], gamma = exp(-0.3), exp(0.3): {ulps.max():.3f} ulp "
    f"of the float32 result ({ulps.size} values)")

for rep in (1, 2):
    say(f"# repeat {rep}")
    for a in range(3):
        lib_us = t_plan(f"gvk_axis_circular_conv, axis {a} (N = {shape[a]})", ghost_lib(a), flops=2.0 * shape[a] * B * V)
        hand = t_events(f"by hand: fftn / mask / ifftn, axis {a}", ghost_hand(a))
        say(f"{'':52s} by hand / library = {hand / lib_us:.1f}")
    sp = t_plan("gvk_gamma_spike, 4 spikes", spike_lib)
    t_plan("gvk_volume_stats + gvk_gamma_spike, 4 spikes", spike_lib_with_stats)
    hand = t_events("by hand: fftn / 4 adds / ifftn", spike_hand)
    say(f"{'':52s} by hand / library = {hand / sp:.1f}")
    ga = t_plan("gvk_gamma_spike, gamma", gamma_lib)
    hand = t_events("by hand: sign(x) * pow(|x|, gamma)", gamma_hand)
    say(f"{'':52s} by hand / library = {hand / ga:.1f}")
    for a in range(3):
        t_plan(f"gvk_axis_gather2, axis {a}, f = 3", aniso_lib(a))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
