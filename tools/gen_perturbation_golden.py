#!/usr/bin/env python3
"""Generate tests/golden/perturb_<case>.npz by RUNNING THE REFERENCE classes (imported as tools/gen_golden.py does) on perturbed volumes.

The perturbed volumes are built here with plain numpy indexing -- an independent construction of what gaviko_amd.explain's deletion /
insertion curves and occlusion sweeps feed the model: the patches of a volume ranked by a synthetic relevance (counter hash, quantised
so that ties are frequent, with a block of exact zeros), the top k replaced by a baseline (deletion) or all but the top k (insertion),
and the eight disjoint 5x5x5 windows of the 10x10x10 patch grid.  Volumes are not stored (synth regenerates them): each file holds the
relevance, the ks, the reference's logits of every step and the largest deviation of the oracle on the same volumes.

Only runs where the reference is present.  Usage:  python tools/gen_perturbation_golden.py [case ...]
"""
from __future__ import annotations

import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from gaviko_amd.utils import synth  # noqa: E402
from gen_golden import BASE, GAVIKO, build_reference, import_reference  # noqa: E402

CASES = {
    "gaviko_t16_b2": ("gaviko", "vit-t16", 2, dict(GAVIKO)),
    "linear_t16_b2": ("linear", "vit-t16", 2, {}),
    "evp_t16_b2": ("evp", "vit-t16", 2, dict(freeze_vit=True)),
}
STEPS = 4
WINDOW = (5, 5, 5)


def relevance(B, N):
    """Counter-hash values quantised to 1/64 (ties are frequent), the first N // 8 patches of every sample an exact 0."""
    r = np.floor(synth.uniform01(synth.name_seed("perturb.relevance"), B * N).reshape(B, N) * 64.0).astype(np.float32) / np.float32(64.0)
    r[:, : N // 8] = 0.0
    return r


def ranks(rel):
    """rank[b, n] = #{m : rel[m] > rel[n]} + #{m < n : rel[m] == rel[n]}, counted directly (O(N^2), no sort)."""
    gt = (rel[:, None, :] > rel[:, :, None]).sum(2)
    idx = np.arange(rel.shape[1])
    eq = ((rel[:, None, :] == rel[:, :, None]) & (idx[None, None, :] < idx[None, :, None])).sum(2)
    return (gt + eq).astype(np.int64)


def upsample(mask, grid, patch):
    """[B, N] patch mask -> [B, 1, D, H, W] voxel mask."""
    m = mask.reshape((mask.shape[0],) + tuple(grid))
    for ax, p in enumerate(patch):
        m = np.repeat(m, p, axis=ax + 1)
    return m[:, None]


def windows(grid, win):
    return [(d, min(d + win[0], grid[0]), h, min(h + win[1], grid[1]), w, min(w + win[2], grid[2]))
            for d in range(0, grid[0], win[0]) for h in range(0, grid[1], win[1]) for w in range(0, grid[2], win[2])]


def run_case(mods, name, outdir):
    import oracle

    method, backbone, B, extra = CASES[name]
    cfg = dict(BASE, backbone=backbone, method=method, **extra)
    t0 = time.time()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            model = build_reference(mods, method, cfg)
        finally:
            os.chdir(cwd)
    sd = model.state_dict()
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in sd.items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    model.eval()
    osd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    dev = [0.0]

    def both(vol):
        """reference logits of a batch of volumes; the oracle's deviation on the same batch is tracked."""
        xt = torch.from_numpy(np.ascontiguousarray(vol))
        with torch.no_grad():
            ref = model(xt)
            orc = oracle.FORWARD[method](osd, xt, cfg, None)
        dev[0] = max(dev[0], (orc - ref).abs().max().item())
        return ref.numpy().copy()

    patch = (cfg["frame_patch_size"], cfg["image_patch_size"], cfg["image_patch_size"])
    x = synth.volumes(0, B)
    grid = tuple(s // p for s, p in zip(x.shape[2:], patch))
    N = int(np.prod(grid))
    rel = relevance(B, N)
    rk = ranks(rel)
    ks = np.array([(s * N) // STEPS for s in range(STEPS + 1)], dtype=np.int64)
    out = {"meta/method": method, "meta/backbone": backbone, "meta/batch": B, "meta/cfg": repr(dict(cfg)), "relevance": rel, "ks": ks,
           "meta/window": np.array(WINDOW, dtype=np.int64)}
    out["logits"] = both(x)
    fills = {"min": x.reshape(B, -1).min(1).reshape(B, 1, 1, 1, 1).astype(np.float32) * np.ones_like(x),
             "vol": np.broadcast_to(synth.volumes(100, 1), x.shape)}
    for tag, fill in fills.items():
        dele, ins = [], []
        for k in ks:
            top = upsample(rk < k, grid, patch)                                   # the k most relevant patches
            dele.append(both(np.where(top, fill, x)))
            ins.append(both(np.where(top, x, fill)))
        out[f"deletion_{tag}"] = np.stack(dele, 1)                                # [B, steps + 1, K]
        out[f"insertion_{tag}"] = np.stack(ins, 1)
    wins = windows(grid, WINDOW)
    occ = []
    for (d0, d1, h0, h1, w0, w1) in wins:
        m = np.zeros((B,) + grid, dtype=bool)
        m[:, d0:d1, h0:h1, w0:w1] = True
        occ.append(both(np.where(upsample(m.reshape(B, N), grid, patch), fills["min"], x)))
    out["occlusion_boxes"] = np.array(wins, dtype=np.int64)
    out["occlusion_min"] = np.stack(occ, 1)                                       # [B, 8, K]
    out["meta/oracle_dev"] = np.float64(dev[0])
    assert dev[0] < 2e-5, dev[0]
    path = os.path.join(outdir, f"perturb_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"perturb_{name}: oracle vs reference {dev[0]:.3e}, deletion prob-free logits[0,:,0]={out['deletion_min'][0, :, 0]}, "
          f"{os.path.getsize(path) / 1024:.0f} KiB, {time.time() - t0:.1f}s")


def main():
    outdir = os.path.join(ROOT, "tests", "golden")
    mods = import_reference()
    for n in sys.argv[1:] or list(CASES):
        run_case(mods, n, outdir)


if __name__ == "__main__":
    main()
