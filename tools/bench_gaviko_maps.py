"""Cost of the MWSA / GPA map functions of gaviko_amd.explain at cfg2 (ViT-B GAViKO, B = 4): per-call time of local_attention_maps,
gpa_attention_maps and local_rollout next to the keep-everything forward they all start with (Engine.attention_forward) and the plain
no-grad forward, on both precision paths, plus the two kernels alone with the bytes they move.  Report only, no threshold.

Each function is warmed up (its launch plan is recorded by then) and timed with device events around `--iters` calls; the whole list is
measured `--rounds` times, alternating the functions, and the median and the spread (min .. max) of the rounds are printed.

    python tools/bench_gaviko_maps.py [--iters 20] [--rounds 5] [--batch 4] [--backbone vit-b16]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gaviko_amd import explain, ops  # noqa: E402
from gaviko_amd.registry import build_model  # noqa: E402
from gaviko_amd.utils import synth  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rounds(fns, iters, n):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(n):
        for k, fn in fns.items():
            got[k].append(timed(fn, iters))
    return {k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
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
    m.to(dev).eval()
    B = a.batch
    x = torch.from_numpy(synth.volumes(0, B)).to(dev)
    eng = m._engine()
    res = {"backbone": a.backbone, "B": B, "iters": a.iters, "rounds": a.rounds, "unit": "ms per call"}

    def plain():
        with torch.no_grad():
            m(x)

    def keep():
        with torch.no_grad():
            eng.attention_forward(x)

    for prec in ("bf16", "fp32"):
        m.set_precision(prec)
        eng = m._engine()
        res[prec] = rounds({"no_grad_forward": plain, "keep_attn_forward": keep,
                            "local_attention_maps": lambda: explain.local_attention_maps(m, x),
                            "gpa_attention_maps": lambda: explain.gpa_attention_maps(m, x),
                            "local_rollout": lambda: explain.local_rollout(m, x)}, a.iters, a.rounds)
    # the kernels alone, on the buffers of the last keep-everything forward
    with torch.no_grad():
        _, ws = eng.attention_forward(x)
    N, P, T, Lt = eng.N, eng.P, eng.T, eng.Lat
    mw, g = ws["mw"][0], ws["gp"][0]
    w = torch.full((B, N), 1.0 / N, device=dev)
    out = torch.empty((B, N), device=dev)
    blocks = [torch.empty((B, P, N), device=dev) for _ in range(3)]
    k = rounds({"window_attn_colsum": lambda: ops.window_attn_colsum(mw["qkv"], mw["lse"], w, out, B, *eng.grid, *eng.win, Lt, eng.C ** -0.5),
                "gpa_attn_maps": lambda: ops.gpa_attn_maps(g["xl"], g["ll"], g["qg"], g["ql"], g["lse_g"], g["lse_l"], g["imp"], g["gw"], B, T, N, P, Lt,
                                                           global_=blocks[0], local=blocks[1], fused=blocks[2])}, 200, a.rounds)
    # bytes the algorithm needs (each operand once): qkv's q and k blocks + lse + w in, out; latents + queries + statistics in, three blocks out
    k["window_attn_colsum"]["bytes"] = B * N * (2 * Lt + 3) * 4
    k["gpa_attn_maps"]["bytes"] = (2 * B * N * Lt + 2 * B * P * Lt + 3 * B * P + B + 3 * B * P * N) * 4
    for v in k.values():
        v["GBps_at_median"] = round(v["bytes"] / (v["median"] * 1e-3) / 1e9, 2)
    res["kernels"] = k
    print(json.dumps(res))


if __name__ == "__main__":
    main()
