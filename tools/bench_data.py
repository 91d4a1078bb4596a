"""GPU box: the data-side kernels (csrc/augment.hip, csrc/intensity.hip, csrc/motion.hip) on a batch of 4 raw (120,160,160) volumes, timed by replaying 50 recorded launches."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from gaviko_amd import data, lib, ops
lib.require_device()
dev = torch.device("cuda:0")
B, shape = 4, (120, 160, 160)
V = int(np.prod(shape))
x = (torch.randn(B, 1, *shape, device=dev) * 300 + 1000).contiguous()
out = torch.empty_like(x)
part = ops.minmax_partials(B, dev)
mats = np.stack([data.affine_matrix((1.05, 0.95, 1.02), (10, -12, 14), (0, 0, 0), shape).astype(np.float32)] * B)
mats_d = torch.from_numpy(mats).to(dev)
fl_aff = torch.full((B,), 9, dtype=torch.int32, device=dev)
fl_flip = torch.full((B,), 1, dtype=torch.int32, device=dev)


def t(name, fn, nbytes):
    for _ in range(3): fn()
    l = lib.load()
    lib.check(l.gvk_plan_begin(), "begin")
    for _ in range(50): fn()
    pid = l.gvk_plan_end()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    l.gvk_plan_replay(pid)
    e0.record(); l.gvk_plan_replay(pid); e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / 50
    print(f"{name:34s} {us:7.1f} us  {nbytes / us / 1e6:6.2f} TB/s algorithmic ({nbytes / 1e6:.1f} MB)")
    l.gvk_plan_free(pid)


t("volume_minmax", lambda: ops.volume_minmax(x, part), B * V * 4)
t("rescale_intensity", lambda: ops.rescale_intensity(x, part, out), 2 * B * V * 4)
t("spatial: flip axis 0", lambda: ops.spatial_transform(x, out, mats_d, fl_flip, part), 2 * B * V * 4)
t("spatial: affine + flip (trilinear)", lambda: ops.spatial_transform(x, out, mats_d, fl_aff, part), 2 * B * V * 4)

# ---- intensity augmentation (csrc/intensity.hip): per-sample tables, every sample drawing the transform that the row names ----------
scratch, tmp = torch.empty_like(x), torch.empty_like(x)
w_np, r_np = data.blur_tables(np.full((B, 3), 1.5))
w_d, r_d = torch.from_numpy(w_np).to(dev), torch.from_numpy(r_np).to(dev)
rng = np.random.default_rng(0)
noise_d = torch.tensor([[0.2, 0.0]] * B, dtype=torch.float32, device=dev)
seeds_d = torch.from_numpy(rng.integers(0, 2 ** 64, B, dtype=np.uint64).view(np.int64)).to(dev)
coeff_d = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, ops.BIAS_COEFFS)).astype(np.float32)).to(dev)
kinds = lambda k: torch.full((B,), k, dtype=torch.int32, device=dev)  # noqa: E731
k_copy, k_noise, k_bias = kinds(0), kinds(1), kinds(2)
t("blur sigma 1.5 (H/W + D pass)", lambda: ops.gaussian_blur3d(x, out, scratch, w_d, r_d, int(r_np.max())), 4 * B * V * 4)
t("intensity_pointwise: copy", lambda: ops.intensity_pointwise(x, out, k_copy, noise_d, seeds_d, coeff_d, 3), 2 * B * V * 4)
t("intensity_pointwise: noise", lambda: ops.intensity_pointwise(x, out, k_noise, noise_d, seeds_d, coeff_d, 3), 2 * B * V * 4)
t("intensity_pointwise: bias order 3", lambda: ops.intensity_pointwise(x, out, k_bias, noise_d, seeds_d, coeff_d, 3), 2 * B * V * 4)

# the kernel sequence DeviceCompose issues for train_transforms(intensity=...) on one batch: affine + flip on every sample, then (intensity)
# a batch whose four samples drew none / noise / bias field / blur -- both intensity launches -- then min/max + rescale
k_mix = torch.tensor([0, 1, 2, 0], dtype=torch.int32, device=dev)
w_mix, r_mix = data.blur_tables([[0, 0, 0], [0, 0, 0], [0, 0, 0], [1.5, 1.5, 1.5]])
w_mix_d, r_mix_d = torch.from_numpy(w_mix).to(dev), torch.from_numpy(r_mix).to(dev)


def pipeline(intensity):
    ops.volume_minmax(x, part)
    ops.spatial_transform(x, out, mats_d, fl_aff, part)
    cur = out
    if intensity:
        ops.intensity_pointwise(cur, tmp, k_mix, noise_d, seeds_d, coeff_d, 3)
        ops.gaussian_blur3d(tmp, out, scratch, w_mix_d, r_mix_d, int(r_mix.max()))
    ops.volume_minmax(cur, part)
    ops.rescale_intensity(cur, part, tmp)


t("pipeline intensity=False", lambda: pipeline(False), (1 + 2 + 1 + 2) * B * V * 4)
t("pipeline intensity=True (mixed)", lambda: pipeline(True), (1 + 2 + 2 + 4 + 1 + 2) * B * V * 4)

# ---- RandomMotion (csrc/motion.hip): K = 2 movements on every sample, fused, next to the by-hand build torchio's algorithm asks for ----------
K, W = 2, shape[-1]
mo_deg, mo_tr, mo_times = rng.uniform(-10, 10, (B, K, 3)), rng.uniform(-10, 10, (B, K, 3)), np.tile([0.3, 0.7], (B, 1))
mo_mats = np.stack([np.stack([data.affine_matrix((1, 1, 1), mo_deg[b, k], mo_tr[b, k], shape).astype(np.float32) for k in range(K)]) for b in range(B)])
ctab, src = data.motion_tables(mo_times, W)
mo_mats_d, ctab_d = torch.from_numpy(mo_mats).to(dev), torch.from_numpy(ctab).to(dev)
live_d = torch.ones(B, dtype=torch.int32, device=dev)
ops.volume_minmax(x, part)
flops = 2.0 * (K + 1) * W * B * V
t("motion_artifact K=2 (fused)", lambda: ops.motion_artifact(x, out, mo_mats_d, ctab_d, live_d, part, K), 2 * B * V * 4)


def t_events(name, fn, seconds=0.3):
    """device events around enough calls issued from Python to fill `seconds`: for work that the library's launch plans cannot record
    (torch.fft).  The calls are queued ahead of the device, so host dispatch hides behind device work as long as the device is the slower."""
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5): fn()
    e1.record(); torch.cuda.synchronize()
    iters = max(20, int(seconds * 1e3 / max(e0.elapsed_time(e1) / 5, 1e-3)))
    e0.record()
    for _ in range(iters): fn()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    print(f"{name:40s} {us:8.1f} us  ({iters} calls)")
    return us


def fused():
    ops.motion_artifact(x, out, mo_mats_d, ctab_d, live_d, part, K)


moved = [torch.empty_like(x) for _ in range(K)]
mats_k = [torch.from_numpy(np.ascontiguousarray(mo_mats[:, k])).to(dev) for k in range(K)]
fl_live = torch.full((B,), 8, dtype=torch.int32, device=dev)
edges = [0] + [int(W * v) for v in mo_times[0]] + [W]
dims = (-3, -2, -1)


def by_hand():
    """K resampling launches into scratch volumes, then torchio's compositing as written: shifted 3-D spectra, slab copies, inverse, real part"""
    for k in range(K):
        ops.spatial_transform(x, moved[k], mats_k[k], fl_live, part)
    spec = [torch.fft.fftshift(torch.fft.fftn(torch.fft.ifftshift(v, dim=dims), dim=dims), dim=dims) for v in [x] + moved]
    res = torch.empty_like(spec[0])
    for j in range(K + 1):
        res[..., edges[j]:edges[j + 1]] = spec[int(src[0, j])][..., edges[j]:edges[j + 1]]
    return torch.fft.fftshift(torch.fft.ifftn(torch.fft.ifftshift(res, dim=dims), dim=dims), dim=dims).real


have_fft = False
try:
    ref = by_hand()
    torch.cuda.synchronize()
except Exception as e:                                    # no working FFT library on this box: the fused kernel's rows stand alone
    print(f"motion by hand: torch.fft does not work here ({type(e).__name__}: {e}); only the fused kernel is recorded")
else:
    fused()
    print(f"max |fused - by hand| = {(out - ref).abs().max().item():.3e} on intensities ~1e3 (the by-hand FFTs are complex64)")
    del ref
    have_fft = True
# same process, the two builds alternating, twice: the spread between the repeats is the noise of the comparison
for rep in (1, 2):
    us = t_events(f"motion fused, events (repeat {rep})", fused)
    print(f"{'':40s} {flops / us / 1e6:8.1f} TFLOP/s fp32 of {flops / 1e9:.1f} GFLOP (matrix-pipe bound: 157.3 peak)")
    if have_fft:
        t_events(f"motion by hand: 2 resamples + FFTs (repeat {rep})", by_hand)
