#!/usr/bin/env python3
"""Timings of gaviko_amd.features on one MI355X -> profiles/features_timing.txt (report only, nothing is asserted).

  embed            cfg2 (ViT-B GAViKO, bf16, B = 4): embed(layers=None), embed(layers="all") and Engine.eval_forward, interleaved rounds
  token_pool       the (cls, patch mean) pair of one layer at cfg2 against the bytes it reads (B * R * C * 4)
  feature_topk     Nq = 8, 256 x Ng = 1e3, 1e5 at C = 768, k = 20, inner product, against torch.topk(q @ g.T) on the device

Usage:  python tools/bench_features.py [--iters 20] [--out profiles/features_timing.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gaviko_amd import features, ops  # noqa: E402
from gaviko_amd.registry import build_model  # noqa: E402
from gaviko_amd.utils import synth  # noqa: E402

CFG2 = dict(image_size=160, image_patch_size=16, frames=120, frame_patch_size=12, num_classes=5, channels=1, pool="cls", dim_head=64,
            dropout=0.0, emb_dropout=0.0, backbone="vit-b16", method="gaviko", num_prompts=32, prompt_latent_dim=20, local_dim=20,
            local_k=(6, 6, 6), DHW=(10, 10, 10), attn_drop=0.0, proj_drop=0.0, freeze_vit=True, share_factor=1)


def timed(fn, iters):
    """Median and extremes of `iters` single calls, each between two device synchronisations (microseconds)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(t), 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_timing.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    res = {}
    m = build_model(dict(CFG2))
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev).eval()
    x = torch.from_numpy(synth.volumes(0, 4)).to(dev)
    eng = m._engine()
    with torch.no_grad():
        runs = {"eval_forward": lambda: eng.eval_forward(x), "embed": lambda: features.embed(m, x),
                "embed_all_layers": lambda: features.embed(m, x, layers="all")}
        acc = {k: [] for k in runs}
        for _ in range(3):                                  # interleaved rounds: drift hits every variant alike
            for k, f in runs.items():
                acc[k].append(timed(f, a.iters)["median_us"])
        res["embed_cfg2_b4"] = {k: {"median_us": statistics.median(v), "rounds": v} for k, v in acc.items()}
    B, T, C, off = 4, eng.T, eng.C, eng.row_off
    g = torch.randn((B, T, C), device=dev)
    out = torch.empty((2, B, C), device=dev)

    def pair():
        ops.token_pool(g, B, T, C, off - 1, 1, out=out[0])
        ops.token_pool(g, B, T, C, off, T - off, out=out[1])

    r = timed(pair, a.iters)
    nbytes = B * (T - off + 1) * C * 4
    res["token_pool_pair_cfg2"] = dict(r, bytes_read=nbytes, gb_per_s=round(nbytes / r["median_us"] / 1e3, 1))
    for Nq in (8, 256):
        for Ng in (1000, 100000):
            q = torch.nn.functional.normalize(torch.randn((Nq, 768), device=dev))
            bank = torch.nn.functional.normalize(torch.randn((Ng, 768), device=dev))
            ours = timed(lambda: ops.feature_topk(q, bank, 20), a.iters)
            ref = timed(lambda: torch.topk(q @ bank.T, 20, dim=1), a.iters)
            i1, _ = ops.feature_topk(q, bank, 20)
            i2 = torch.topk(q @ bank.T, 20, dim=1).indices
            res[f"feature_topk_Nq{Nq}_Ng{Ng}_C768_k20"] = {"feature_topk": ours, "torch_topk_of_matmul": ref,
                                                        "slabs": L_slabs(Nq, Ng), "index_agreement": round(float((i1 == i2).float().mean()), 4),
                                                        "gflop": round(2.0 * Nq * Ng * 768 / 1e9, 3)}
    lines = ["# python tools/bench_features.py --iters %d" % a.iters,
             "# one MI355X; single calls between device synchronisations, median of --iters (embed: median of 3 interleaved rounds)"]
    lines += [json.dumps({k: v}) for k, v in res.items()]
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def L_slabs(Nq, Ng):
    from gaviko_amd import lib
    return lib.load().gvk_feature_topk_slabs(Nq, Ng, 0)


if __name__ == "__main__":
    main()
