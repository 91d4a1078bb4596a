"""GPU box: the data-side kernels (csrc/augment.hip, csrc/intensity.hip) on a batch of 4 raw (120,160,160) volumes, timed by replaying 50 recorded launches."""
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
