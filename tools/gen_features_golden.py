#!/usr/bin/env python3
"""Generate tests/golden/features_<method>_t16_b2.npz by RUNNING THE REFERENCE classes (imported as tools/gen_golden.py does) in eval mode
on ViT-T/16 with the formula-seeded weights and synth.volumes(0, 2).

Each file holds
  pooled            [B, C] f32   the input of the head's nn.Linear, from a forward pre-hook on it (what a user of the reference reads)
  logits            [B, K] f32   the reference's logits
  cls, patch_mean   [depth + 1, B, C] f64   per layer l, of the global token stream ENTERING layer l (l = depth: the output of the last
                    layer, before transformer.norm): the CLS row and the mean over the patch rows.  From the oracle's embedding output and its
                    layer{i}.post_mlp taps, reduced in float64.  Deep VPT cuts the sequence in front of every layer (vpt.py:147-153): the
                    patch rows of layer l are the ones that layer still has.
  meta/oracle_dev   the oracle's largest deviation from the reference (logits and head input), asserted < 2e-5
  floor/<key>       max|x_bf16 - x| / max|x| of pooled / logits / cls / patch_mean from the oracle under BF16_OPERANDS: the bf16 floor
Volumes are not stored (synth regenerates them).

Only runs where the reference is present (the build container).  Usage:  python tools/gen_features_golden.py [method ...]
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
    "gaviko": dict(GAVIKO),
    "linear": {},
    "deep_vpt": dict(num_prompts=8, prompt_dim=64, prompt_dropout=0.0, freeze_vit=True, deep_prompt=True),     # the sequence shrinks per layer
    "dvpt": dict(num_prompts=8, freeze_vit=True),                                                             # pool='cls' reads row 0: a prompt
}
B = 2


def head_linear(model, K):
    """The nn.Linear that produces the logits (mlp_head.head of Gaviko, the head Linear of the other classes)."""
    found = [(n, m) for n, m in model.named_modules() if isinstance(m, torch.nn.Linear) and "head" in n and m.out_features == K]
    assert len(found) == 1, [n for n, _ in found]
    return found[0]


def layer_rows(method, cfg, sd, x, taps):
    """[(cls [B, C], patches [B, n_l, C])] for l = 0 .. depth from the oracle's embedding output and post_mlp taps."""
    from oracle import vit_ref
    depth = vit_ref.mapping_vit(cfg["backbone"])[0]
    patch = (cfg["frame_patch_size"], cfg["image_patch_size"], cfg["image_patch_size"])
    P = cfg.get("num_prompts", 0)
    out = []
    if method == "gaviko":
        e = taps["embed.global"]                                   # [P prompts | cls | patches]
        out.append((e[:, P], e[:, P + 1:]))
    elif method == "dvpt":
        pe = vit_ref.patch_embed(sd, "conv_proj.0", x, patch)
        pos = sd["pos_embedding"]
        out.append(((sd["cls_token"] + pos[:, :1]).expand(x.shape[0], -1, -1)[:, 0], pe + pos[:, 1:]))
    else:
        e = vit_ref.embed_tokens(sd, x, patch, "vision_transformer." if method == "deep_vpt" else "")     # [cls | patches]; VPT's prompts go between
        out.append((e[:, 0], e[:, 1:]))
    for l in range(1, depth + 1):
        t = taps[f"layer{l - 1}.post_mlp"]
        if method in ("gaviko", "dvpt"):
            out.append((t[:, P], t[:, P + 1:]))
        elif method == "deep_vpt":
            # the stream entering layer l < depth is [cls | new prompts | t[:, 1 + prompt_dim:]] (vpt.py:147-153); the last output is not cut
            skip = cfg["prompt_dim"] if l < depth else P
            out.append((t[:, 0], t[:, 1 + skip:]))
        else:
            out.append((t[:, 0], t[:, 1:]))
    return out


def oracle_run(method, cfg, osd, x, bf16):
    import oracle
    from oracle import vit_ref
    old = vit_ref.BF16_OPERANDS
    vit_ref.BF16_OPERANDS = bf16
    try:
        taps = {}
        with torch.no_grad():
            logits = oracle.FORWARD[method](osd, x, cfg, taps)
            rows = layer_rows(method, cfg, osd, x, taps)
    finally:
        vit_ref.BF16_OPERANDS = old
    fn = taps["final_norm"].double()
    P = cfg.get("num_prompts", 0)
    if method == "gaviko":
        pooled = fn[:, : P + 1].mean(1)
    elif cfg.get("pool", "cls") == "mean":
        pooled = fn.mean(1)
    else:
        pooled = fn[:, 0]
    return {"logits": logits.double().numpy(), "pooled": pooled.numpy(),
            "cls": np.stack([c.double().numpy() for c, _ in rows]), "patch_mean": np.stack([p.double().mean(1).numpy() for _, p in rows]),
            "patch_rows": np.array([p.shape[1] for _, p in rows], dtype=np.int64)}


def run_case(mods, method, outdir):
    cfg = dict(BASE, backbone="vit-t16", method=method, **CASES[method])
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
    x = torch.from_numpy(synth.volumes(0, B))
    got = {}
    name, head = head_linear(model, cfg["num_classes"])
    h = head.register_forward_pre_hook(lambda m, inp: got.__setitem__("in", inp[0].detach().clone()))
    with torch.no_grad():
        ref = model(x)
    h.remove()
    hi = oracle_run(method, cfg, osd, x, False)
    lo = oracle_run(method, cfg, osd, x, True)
    dev = max(float(np.abs(hi["logits"] - ref.double().numpy()).max()), float(np.abs(hi["pooled"] - got["in"].double().numpy()).max()))
    assert dev < 2e-5, dev
    out = {"meta/method": method, "meta/backbone": "vit-t16", "meta/batch": B, "meta/cfg": repr(dict(cfg)), "meta/oracle_dev": np.float64(dev),
           "meta/head": name, "meta/patch_rows": hi["patch_rows"],
           "pooled": got["in"].numpy().astype(np.float32), "logits": ref.numpy().astype(np.float32),
           "cls": hi["cls"], "patch_mean": hi["patch_mean"]}
    for k in ("pooled", "logits", "cls", "patch_mean"):
        out["floor/" + k] = np.float64(np.abs(lo[k] - hi[k]).max() / np.abs(hi[k]).max())
    path = os.path.join(outdir, f"features_{method}_t16_b2.npz")
    np.savez_compressed(path, **out)
    print(f"features_{method}_t16_b2: head {name}, oracle vs reference {dev:.3e}, patch rows {hi['patch_rows'].tolist()}, floors "
          + ", ".join(f"{k} {float(out['floor/' + k]):.2e}" for k in ("pooled", "logits", "cls", "patch_mean"))
          + f", {os.path.getsize(path) / 1024:.1f} KiB, {time.time() - t0:.1f}s")


def main():
    outdir = os.path.join(ROOT, "tests", "golden")
    mods = import_reference()
    for n in sys.argv[1:] or list(CASES):
        run_case(mods, n, outdir)


if __name__ == "__main__":
    main()
