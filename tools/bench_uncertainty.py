"""Uncertainty timings at cfg2 (ViT-B GAViKO, bf16, 4 volumes of 120x160x160, attn_drop = proj_drop = 0.2 as shipped), after warm-up (the
launch plans are recorded by then), device events around every repetition, the two sides of a comparison interleaved:

  a. gvk_tta_volumes per member for the flip codes 0 (replica), 1 (D mirror) and 4 (W mirror: the mirrored float4, lanes reversed), 8
     members per launch, beside out.copy_(x) of the same bytes timed in the same run (2 * Bout * V * 4 bytes either way);
  b. mc_dropout(samples=32) and tta(flips='all') on the 4 volumes against the same work assembled by hand from what the package offered
     before: repeat_interleave / torch.flip, model.train() under no_grad (model.eval() for tta), one model call per chunk of the same
     size, torch softmax / entropy / vote arithmetic; and against the bare chunk forwards alone;
  c. the gvk_predictive_stats launch alone.

    python tools/bench_uncertainty.py [--iters 10] [--out profiles/uncertainty_timing.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from gaviko_amd import ops, uncertainty  # noqa: E402
from gaviko_amd.registry import build_model  # noqa: E402
from gaviko_amd.utils import synth  # noqa: E402


def interleaved(fns, iters, warm=3):
    """median ms of every fn, one repetition of each in turn per round (so that clocks and cache state are shared)."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def repeated(fn, reps):
    def run():
        for _ in range(reps):
            fn()
    return run


def torch_stats(z):
    """The statistics in torch, as a user would write them.  z [B, S, K]."""
    p = torch.softmax(z, 2)
    mean = p.mean(1)
    ent = -(mean * torch.log(mean.clamp_min(1e-38))).sum(1)
    exp = -(p * torch.log(p.clamp_min(1e-38))).sum(2).mean(1)
    votes = torch.nn.functional.one_hot(z.argmax(2), z.shape[2]).sum(1)
    return mean, mean.argmax(1), ent, exp, (ent - exp).clamp_min(0), 1 - votes.max(1).values.float() / z.shape[1], p.std(1, unbiased=False), votes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dict(image_size=160, image_patch_size=16, frames=120, frame_patch_size=12, num_classes=5, channels=1, pool="cls", dim_head=64,
               dropout=0.0, emb_dropout=0.0, backbone="vit-b16", method="gaviko", num_prompts=32, prompt_latent_dim=20, local_dim=20,
               local_k=(6, 6, 6), DHW=(10, 10, 10), attn_drop=0.2, proj_drop=0.2, freeze_vit=True, share_factor=1)
    m = build_model(cfg)
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev).train()
    eng = m._engine()
    B, S = 4, 32
    x = torch.from_numpy(synth.volumes(0, B)).to(dev)
    V = x.numel() // B
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)       # noqa: E731
    res = {}

    # a. the member kernel against a plain copy of the same bytes
    Bc = 8
    out = torch.empty((Bc,) + tuple(x.shape[1:]), device=dev)
    xs = x.repeat(2, 1, 1, 1, 1).contiguous()                       # 8 volumes: the copy's source
    src = i32([o % B for o in range(Bc)])
    fns = {"copy_": repeated(lambda: out.copy_(xs), 20)}
    for code in (0, 1, 4):
        flip = i32([code] * Bc)
        fns[f"tta_volumes_code{code}"] = repeated(lambda flip=flip: ops.tta_volumes(x, src, flip, out), 20)
    nbytes = 2 * Bc * V * 4
    for k, v in interleaved(fns, a.iters).items():
        us = 1e3 * v["median_ms"] / 20
        res["a_" + k] = dict(us_per_launch=us, us_per_member=us / Bc, bytes=nbytes, TBps=nbytes / (us * 1e-6) / 1e12, hbm_ceiling_TBps=6.3)

    # b. the sweeps against the hand-built loops and the bare forwards
    drop = uncertainty.training_drop_config(m)
    bs_mc, bs_tta = S, 8

    def hand_mc():
        with torch.no_grad():                                       # the model is in train mode: its dropouts are live
            rows = x.repeat_interleave(S, 0)
            z = torch.cat([m(rows[c:c + bs_mc]).clone() for c in range(0, B * S, bs_mc)]).view(B, S, -1)
            return torch_stats(z)

    def hand_tta():
        m.eval()
        with torch.no_grad():
            dims = [[a_ + 2 for a_ in range(3) if c >> a_ & 1] for c in range(8)]
            z = torch.cat([m(torch.cat([torch.flip(x[b:b + 1], d) if d else x[b:b + 1] for d in dims])).clone() for b in range(B)]).view(B, 8, -1)
            r = torch_stats(z)
        m.train()
        return r

    xb_mc, xb_tta = x.repeat_interleave(S, 0)[:bs_mc].contiguous(), x.repeat(2, 1, 1, 1, 1).contiguous()

    def bare_mc():
        with torch.no_grad():
            for _ in range(B * S // bs_mc):
                eng.forward(xb_mc, train=False, drop=drop)

    def bare_tta():
        for _ in range(B * 8 // bs_tta):
            eng.eval_forward(xb_tta)

    r = interleaved({"mc_dropout": lambda: uncertainty.mc_dropout(m, x, samples=S), "by_hand": hand_mc, "bare_forwards": bare_mc}, a.iters)
    res["b_mc_dropout_samples32_B4_batch32"] = dict(r, chunks=B * S // bs_mc, ratio_vs_by_hand=r["mc_dropout"]["median_ms"] / r["by_hand"]["median_ms"],
                                                    overhead_vs_bare_forwards=r["mc_dropout"]["median_ms"] / r["bare_forwards"]["median_ms"] - 1)
    r = interleaved({"tta": lambda: uncertainty.tta(m, x, flips="all"), "by_hand": hand_tta, "bare_forwards": bare_tta}, a.iters)
    res["b_tta_all_B4_batch8"] = dict(r, chunks=B * 8 // bs_tta, ratio_vs_by_hand=r["tta"]["median_ms"] / r["by_hand"]["median_ms"],
                                      overhead_vs_bare_forwards=r["tta"]["median_ms"] / r["bare_forwards"]["median_ms"] - 1)

    # c. the statistics launch alone, beside the torch arithmetic it replaces
    z = torch.randn((B, S, eng.K), device=dev)
    r = interleaved({"predictive_stats": repeated(lambda: ops.predictive_stats(z, B, S), 50), "torch_stats": repeated(lambda: torch_stats(z), 50)}, a.iters)
    res["c_stats_B4_S32_K5"] = {k: dict(us_per_call=1e3 * v["median_ms"] / 50) for k, v in r.items()}

    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/bench_uncertainty.py --iters %d --out %s\n" % (a.iters, a.out))
            f.write("# cfg2: ViT-B GAViKO, bf16, 4 volumes of 120x160x160, attn_drop = proj_drop = 0.2, one MI355X; device events around every repetition after\n")
            f.write("# warm-up, the sides of a comparison interleaved; medians.  a: 8 members per launch, 20 launches per repetition, bytes = 2 Bout V 4;\n")
            f.write("# b: wall time of one whole call on the device timeline (host work between launches included); c: 50 calls per repetition.\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
