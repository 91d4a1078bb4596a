"""GPU box: cost of the explanation kernels (csrc/attention_map.hip) and of a whole attention_rollout.  Report only, no assertion.
  * the column-sum kernel alone at cfg2 (B=4, T=1033, H=12) and cfg5 (ViT-L: B=2, T=1033, H=16), pooled (the 33 prompt + CLS rows of
    GAViKO) and dense (all rows: every rollout step after the first); flops = 2 B H (q1 - q0) T 64 (the score product);
  * the rollout step kernel alone (the separate form: DESIGN kernel table);
  * the gradient column-sum kernel (gradient x attention: a second MFMA chain for dP = dO . V^T) and the relevance step, same shapes;
  * attention_rollout against one no-grad forward of the cfg2 model (ViT-B GAViKO, B=4);
  * attention_relevance and attention_gradmaps against input_gradient (the same forward + input-only sweep without the 12 launches).
Every kernel figure is the median of 7 rounds of 50 launches recorded into one launch plan.
usage: python tools/bench_explain.py [--out FILE.jsonl]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaviko_amd import explain, lib, ops  # noqa: E402

lib.require_device()
dev = torch.device("cuda:0")
l = lib.load()
NL, ROUNDS = 50, 7


def plan_time_us(fn):
    for _ in range(3):
        fn()
    lib.check(l.gvk_plan_begin(), "gvk_plan_begin")
    for _ in range(NL):
        fn()
    pid = l.gvk_plan_end()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lib.check(l.gvk_plan_replay(pid), "gvk_plan_replay")
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / NL)
    l.gvk_plan_free(pid)
    return statistics.median(ts)


def kernels(name, B, T, H, pooled_rows):
    inner = H * 64
    qkv = ops.act_zeros(B * T, 3 * inner, torch.bfloat16, dev)
    qkv[: B * T] = (torch.randn(B * T, 3 * inner, device=dev) * 0.7).bfloat16()
    ops.qkv_prescale(qkv, B * T, H, 0.125)
    o = ops.act_zeros(B * T, inner, torch.bfloat16, dev)
    lse = torch.empty((B, H, T), device=dev)
    ops.attention_fwd(qkv, o, lse, B, T, H, 0.125, q_prescaled=True)
    w = torch.rand((B, T), device=dev)
    out = torch.empty((B, H, T), device=dev)
    r = torch.rand((B, T), device=dev)
    res = []
    for form, q1 in (("pooled", pooled_rows), ("dense", T)):
        us = plan_time_us(lambda: ops.attention_colsum(qkv, lse, w, out, B, T, H, q0=0, q1=q1))
        fl = 2.0 * B * H * q1 * T * 64
        res.append(dict(shape=name, kernel="colsum", form=form, B=B, T=T, H=H, rows=q1, us=round(us, 2), tflops=round(fl / us * 1e-6, 1)))
    us = plan_time_us(lambda: ops.rollout_step(r, out, r, B, T, H))
    res.append(dict(shape=name, kernel="rollout_step", B=B, T=T, H=H, us=round(us, 2)))
    dctx = ops.act_zeros(B * T, inner, torch.bfloat16, dev)
    dctx[: B * T] = (torch.randn(B * T, inner, device=dev) * 1e-3).bfloat16()
    for form, q1 in (("pooled", pooled_rows), ("dense", T)):
        us = plan_time_us(lambda: ops.attention_gradcolsum(qkv, lse, dctx, w, out, B, T, H, q0=0, q1=q1))
        fl = 4.0 * B * H * q1 * T * 64
        res.append(dict(shape=name, kernel="gradcolsum", form=form, B=B, T=T, H=H, rows=q1, us=round(us, 2), tflops=round(fl / us * 1e-6, 1)))
    us = plan_time_us(lambda: ops.relevance_step(r, out, r, B, T, H))
    res.append(dict(shape=name, kernel="relevance_step", B=B, T=T, H=H, us=round(us, 2)))
    fa = plan_time_us(lambda: ops.attention_fwd(qkv, o, lse, B, T, H, 0.125, q_prescaled=True))
    res.append(dict(shape=name, kernel="attention_fwd (for scale)", B=B, T=T, H=H, us=round(fa, 2)))
    return res


def whole_rollout():
    from gaviko_amd.registry import build_model
    from gaviko_amd.utils import synth
    cfg = dict(image_size=160, image_patch_size=16, frames=120, frame_patch_size=12, num_classes=5, channels=1, pool="cls", dim_head=64,
               dropout=0.0, emb_dropout=0.0, backbone="vit-b16", method="gaviko", num_prompts=32, prompt_latent_dim=20, local_dim=20,
               local_k=(6, 6, 6), DHW=(10, 10, 10), attn_drop=0.0, proj_drop=0.0, freeze_vit=True, share_factor=1, fp16=False)
    m = build_model(cfg)
    sd = m.state_dict()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.fill_state_dict({k: tuple(v.shape) for k, v in sd.items()}).items()})
    m.to(dev).eval()
    x = torch.from_numpy(synth.volumes(0, 4)).to(dev)

    def timed(fn, n=20):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    with torch.no_grad():
        fwd = timed(lambda: m(x))
    # the explanation's own forward (inference forward into the workspace that keeps every layer's qkv / lse), then the 12 map steps
    eng = m._engine()
    efwd = timed(lambda: eng.attention_forward(x))
    roll = timed(lambda: explain.attention_rollout(m, x))
    igrad = timed(lambda: explain.input_gradient(m, x))
    relv = timed(lambda: explain.attention_relevance(m, x))
    gmaps = timed(lambda: explain.attention_gradmaps(m, x))
    more = [dict(shape="cfg2 model", what="input_gradient (forward + input-only sweep + un-patchify)", ms=round(igrad, 3)),
            dict(shape="cfg2 model", what="attention_relevance (the same sweep + 12 gradient column sums + 12 steps)", ms=round(relv, 3)),
            dict(shape="cfg2 model", what="attention_gradmaps (the same sweep + 12 pooled gradient column sums)", ms=round(gmaps, 3)),
            dict(shape="cfg2 model", what="relevance beyond input_gradient", ms=round(relv - igrad, 3)),
            dict(shape="cfg2 model", what="input_gradient + 2 x rollout-beyond-forward (the expected ceiling)", ms=round(igrad + 2 * (roll - efwd), 3))]
    return more + [dict(shape="cfg2 model", what="no-grad forward", ms=round(fwd, 3)),
            dict(shape="cfg2 model", what="explanation forward (keeps qkv / lse)", ms=round(efwd, 3)),
            dict(shape="cfg2 model", what="attention_rollout (forward + 12 column sums + 12 steps)", ms=round(roll, 3)),
            dict(shape="cfg2 model", what="rollout beyond its forward", ms=round(roll - efwd, 3))]


if __name__ == "__main__":
    t0 = time.time()
    rows = kernels("cfg2", 4, 1033, 12, 33) + kernels("cfg5", 2, 1033, 16, 33) + whole_rollout()
    for r in rows:
        print(json.dumps(r))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    print(f"({time.time() - t0:.0f} s)")
