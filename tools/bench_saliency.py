"""Input-gradient timings at cfg2 (ViT-B GAViKO, B = 4, bf16): a training step, the input-only sweep of gaviko_amd.explain (a
deterministic training forward + the backward down to the voxels, no parameter gradient kept), one integrated_gradients call at
steps = 32, and the un-patchify kernel alone (B*N*Kp*4 bytes in, a volume out).  Each is timed in isolation after warm-up (the launch
plans are recorded by then), with events around `--iters` repetitions.

    python tools/bench_saliency.py [--iters 20] [--batch 4] [--backbone vit-b16]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gaviko_amd import explain, ops  # noqa: E402
from gaviko_amd.registry import build_model  # noqa: E402
from gaviko_amd.utils import synth  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--backbone", default="vit-b16")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dict(image_size=160, image_patch_size=16, frames=120, frame_patch_size=12, num_classes=5, channels=1, pool="cls", dim_head=64,
               dropout=0.0, emb_dropout=0.0, backbone=a.backbone, method="gaviko", num_prompts=32, prompt_latent_dim=20, local_dim=20,
               local_k=(6, 6, 6), DHW=(10, 10, 10), attn_drop=0.0, proj_drop=0.0, freeze_vit=True, share_factor=1)
    m = build_model(cfg)
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev).train()
    B = a.batch
    x = torch.from_numpy(synth.volumes(0, B)).to(dev)
    y = torch.from_numpy(synth.labels(0, B)).to(dev)
    eng = m._engine()

    def train_step():
        torch.nn.functional.cross_entropy(m(x), y).backward()

    onehot = torch.nn.functional.one_hot(torch.zeros(B, dtype=torch.int64, device=dev), eng.K).float()
    res = {"backbone": a.backbone, "B": B}
    res["train_step_ms"] = timed(train_step, a.iters)
    res["input_only_sweep_ms"] = timed(lambda: eng.input_backward(x, lambda lg: onehot), a.iters)
    res["integrated_gradients_steps32_ms"] = timed(lambda: explain.integrated_gradients(m, x[:1], 0, steps=32, batch=B), max(2, a.iters // 5))
    ws = eng._wss[(B, True, str(dev), "igrad")]
    out = torch.empty_like(x)
    us = 1e3 * timed(lambda: ops.unpatchify(ws["ig"]["dcols"], out, eng.patch), 200)
    nbytes = B * eng.N * eng.Kp * 4 + out.numel() * 4
    res["unpatchify_us"] = us
    res["unpatchify_GBps"] = nbytes / (us * 1e-6) / 1e9
    res["unpatchify_bytes"] = nbytes
    print(json.dumps(res))


if __name__ == "__main__":
    main()
