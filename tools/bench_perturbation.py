"""Perturbation timings at cfg2 (ViT-B GAViKO, bf16, 120x160x160 volumes), each in isolation after warm-up (the launch plans are
recorded by then), with events around the repetitions:

  1. gvk_perturb_volume alone at chunk 4 and 8 (Bout*V*4 bytes written, (S + 1)*V*4 read with a baseline volume, S*V*4 with a scalar
     fill), beside its sibling gvk_unpatchify_f32 re-measured in the same run;
  2. deletion_curve(steps=20) on one volume at batch 8 (21 samples: step k = 0 is the unperturbed volume; 3 chunks) against 3 plain
     eval_forward calls at the same chunk size, and the mask / perturb / gather launches of one chunk on their own;
  3. the same sweep built by hand: torch.where on volumes, a copy into the model per chunk of 8, softmax and .cpu() per step;
  4. occlusion_sensitivity(window=(2, 2, 2)): 125 windows.

    python tools/bench_perturbation.py [--iters 20] [--out profiles/perturbation_timing.txt]
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


def timed(fn, iters, warm=3):
    for _ in range(warm):
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = dict(image_size=160, image_patch_size=16, frames=120, frame_patch_size=12, num_classes=5, channels=1, pool="cls", dim_head=64,
               dropout=0.0, emb_dropout=0.0, backbone="vit-b16", method="gaviko", num_prompts=32, prompt_latent_dim=20, local_dim=20,
               local_k=(6, 6, 6), DHW=(10, 10, 10), attn_drop=0.0, proj_drop=0.0, freeze_vit=True, share_factor=1)
    m = build_model(cfg)
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    m.to(dev).train()
    eng = m._engine()
    x = torch.from_numpy(synth.volumes(0, 1)).to(dev)
    N, V = eng.N, x.numel()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)       # noqa: E731
    g = torch.Generator().manual_seed(0)
    rel = torch.rand((1, N), generator=g).to(dev)
    res = {}

    # 1. the volume kernel alone, and its sibling
    base = torch.from_numpy(synth.volumes(100, 1)).to(dev)
    fill = torch.zeros(1, device=dev)
    for Bc in (4, 8):
        out = torch.empty((Bc,) + tuple(x.shape[1:]), device=dev)
        mask = (torch.rand((Bc, N), generator=g) < 0.5).to(torch.uint8).to(dev)
        src = i32([0] * Bc)
        for tag, kw, nread in (("scalar", dict(fill_scalar=fill), 1), ("volume", dict(base=base), 2)):
            us = 1e3 * timed(lambda: ops.perturb_volume(x, mask, src, out, eng.patch, **kw), 200)
            nbytes = (Bc + nread) * V * 4
            res[f"perturb_volume_{tag}_chunk{Bc}"] = dict(us=us, bytes=nbytes, TBps=nbytes / (us * 1e-6) / 1e12)
        dcols = torch.randn((Bc * N, eng.Kp), generator=g).to(dev)
        us = 1e3 * timed(lambda: ops.unpatchify(dcols, out, eng.patch), 200)
        nbytes = 2 * Bc * V * 4
        res[f"unpatchify_chunk{Bc}"] = dict(us=us, bytes=nbytes, TBps=nbytes / (us * 1e-6) / 1e12)

    # 2. a deletion curve against the same number of plain forwards at the same chunk size
    Bc = 8
    xb = x.expand(Bc, -1, -1, -1, -1).contiguous()
    fwd_ms = timed(lambda: eng.eval_forward(xb), a.iters, warm=5)
    curve_ms = timed(lambda: explain.deletion_curve(m, x, rel, 0, steps=20, batch=Bc), a.iters, warm=5)
    rank = ops.patch_rank(rel)
    src, lo, hi, slot = i32([0] * Bc), i32([0] * Bc), i32(list(range(0, 400, 50))), i32(list(range(Bc)))
    mask = torch.empty((Bc, N), dtype=torch.uint8, device=dev)
    out = torch.empty_like(xb)
    rows = torch.empty((Bc, eng.K), device=dev)
    logits = torch.randn((Bc, eng.K), device=dev)
    res["deletion_curve_steps20_B1_batch8"] = dict(
        curve_ms=curve_ms, plain_forward_chunk8_ms=fwd_ms, chunks=3, three_plain_forwards_ms=3 * fwd_ms, ratio=curve_ms / (3 * fwd_ms),
        per_chunk_us=dict(patch_mask_rank=1e3 * timed(lambda: ops.patch_mask_rank(rank, src, lo, hi, mask), 200),
                          perturb_volume=1e3 * timed(lambda: ops.perturb_volume(x, mask, src, out, eng.patch, fill_scalar=fill), 200),
                          gather_rows=1e3 * timed(lambda: ops.perturb_scores(logits, None, None, slot, None, None, rows), 200)),
        per_call_us=dict(patch_rank=1e3 * timed(lambda: ops.patch_rank(rel), 200)))

    # 3. the sweep a user had to write before: torch.where on volumes, a copy into the model per chunk, softmax and .cpu() per step
    order = torch.argsort(rel, dim=1, descending=True, stable=True)
    ks = [(s * N) // 20 for s in range(21)]
    fillv = x.min()

    def by_hand():
        probs = []
        with torch.no_grad():
            for c in range(0, len(ks), Bc):
                vols = []
                for k in ks[c:c + Bc]:
                    pm = torch.zeros(N, dtype=torch.bool, device=dev)
                    pm[order[0, :k]] = True
                    vm = pm.view(1, 1, *eng.grid).repeat_interleave(eng.patch[0], 2).repeat_interleave(eng.patch[1], 3).repeat_interleave(eng.patch[2], 4)
                    vols.append(torch.where(vm, fillv, x))
                while len(vols) < Bc:
                    vols.append(vols[-1])
                logits = eng.eval_forward(torch.cat(vols))
                for i in range(len(ks[c:c + Bc])):
                    probs.append(logits[i].softmax(0)[0].cpu())                  # one probability to the host per step
        return probs

    res["deletion_curve_by_hand_ms"] = timed(by_hand, max(2, a.iters // 2), warm=2)

    # 4. occlusion sensitivity with 2x2x2 windows: 125 windows + the plain volume = 126 samples, 16 chunks of 8
    res["occlusion_window222_ms"] = timed(lambda: explain.occlusion_sensitivity(m, x, 0, window=(2, 2, 2), batch=Bc), max(2, a.iters // 4), warm=2)

    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# python tools/bench_perturbation.py --iters %d --out %s\n" % (a.iters, a.out))
            f.write("# cfg2: ViT-B GAViKO, bf16, 120x160x160, one MI355X; device events around the repetitions after warm-up (plans recorded by then);\n")
            f.write("# bytes = algorithmic bytes of the launch ((Bout + S [+ 1 with a baseline volume]) V 4 for perturb_volume, 2 Bout V 4 for unpatchify)\n")
            f.write(text + "\n")


if __name__ == "__main__":
    main()
