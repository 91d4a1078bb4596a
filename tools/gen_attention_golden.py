#!/usr/bin/env python3
"""Generate tests/golden/attn_<case>.npz -- attention maps and attention rollout of THE REFERENCE (imported as tools/gen_golden.py does).

Only runs in the build container (the reference never travels).  For each case it
  1. builds the reference model with the synth weights of gaviko_amd.utils.synth, puts it in eval(), runs synth.volumes(0, B),
  2. hooks every global self-attention: the `attend` softmax output (what a user's hook sees) and the `to_qkv` output,
  3. recomputes P = softmax(scale q.k^T) in float64 from the hooked q, k (checked against the hooked softmax: meta/attend_dev) and stores
       pool/layer{i}  [B, H, T_i]  maps of the rows the REFERENCE's head pools (gaviko.py:316, vision_transformer.py:161, dvpt.py:80-83,205,
                                   vpt.py:159) -- uniform weights over those rows,
       cls/layer{i}   [B, H, T_i]  the CLS row's map of the first and the last layer,
       rollout        [B, T]       r = w_pool; for l = L-1 .. 0: r <- 0.5 r + 0.5 mean_h(r^T P_l[h])   (one token sequence only),
       floor/<key>                 max|x_bf16 - x| / max|x| of the same quantity recomputed from q * scale * log2(e) and k rounded to bf16
                                   (the operands the bf16 kernels read): the precision floor of any bf16 implementation.
Everything is stored as float32.

Usage:  python tools/gen_attention_golden.py [case ...]      (no args = all cases)
"""
from __future__ import annotations

import math
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from gaviko_amd.utils import synth  # noqa: E402
from gen_golden import BASE, CASES, build_reference, import_reference  # noqa: E402

# case -> which layers' pooled maps are stored (None = all), whether the rollout is stored
ATTN_CASES = {
    "gaviko_t16_b2": (None, True),
    "cfg1_linear_t16_b1": (None, True),
    "dvpt_t16_b2_mean_p8": (None, True),
    "deep_vpt_t16_b2": (None, False),            # the sequence changes per layer (vpt.py:147-153): maps only
    "cfg2_gaviko_b16_b4": ("ends", True),        # rollout plus layers 0 and L-1 (file size)
}


def attention_modules(model, method):
    """The global self-attention of every layer, in layer order (each has .attend and .to_qkv)."""
    if method == "gaviko":
        return list(model.transformer.attns)
    if method in ("linear", "fft", "bitfit"):
        return [layer[0] for layer in model.transformer.layers]
    if method == "dvpt":
        return [layer[0].attn for layer in model.transformer.layers]
    if method in ("deep_vpt", "shallow_vpt"):
        return [layer[0] for layer in model.vision_transformer.transformer.layers]
    raise ValueError(method)


def pooled_rows(model, method, T_last):
    """Query rows the reference's classification head averages over."""
    if method == "gaviko":                                      # gaviko.py:316  x[:, 0:num_prompts+1].mean(dim=1)
        return list(range(model.num_prompts + 1)), "prompts+cls"
    if method == "dvpt":                                        # dvpt.py:80-83 (mean: norm(x[:, 0:num+1])), 205
        pool = model.pool
        return (list(range(model.transformer.num + 1)), "rows 0..P") if pool == "mean" else ([0], "row 0")
    vt = model.vision_transformer if method in ("deep_vpt", "shallow_vpt") else model
    return (None, "all rows") if vt.pool == "mean" else ([0], "row 0")      # vision_transformer.py:161, vpt.py:138,159


def cls_row(model, method):
    if method in ("gaviko", "dvpt"):                            # [prompts | cls | patches]
        return int(model.num_prompts if method == "gaviko" else model.transformer.num)
    return 0


def probs(q, k, heads, bf16):
    """P [B, H, T, T] float64 from the to_qkv output's q, k blocks [B, T, inner]; bf16=True: from the bf16 operands of the kernels
    (q * scale * log2 e and k, each rounded to bf16), exponent base 2."""
    B, T, inner = q.shape
    d = inner // heads
    q = q.reshape(B, T, heads, d).transpose(1, 2)
    k = k.reshape(B, T, heads, d).transpose(1, 2)
    scale = d ** -0.5
    if bf16:
        qs = (q.float() * (scale * math.log2(math.e))).bfloat16().double()
        kk = k.float().bfloat16().double()
        s = torch.matmul(qs, kk.transpose(-1, -2)) * math.log(2.0)
    else:
        s = torch.matmul(q.double(), k.double().transpose(-1, -2)) * scale
    return torch.softmax(s, dim=-1)


def weights(rows, B, T):
    w = torch.zeros((B, T), dtype=torch.float64)
    if rows is None:
        w[:] = 1.0 / T
    else:
        w[:, rows] = 1.0 / len(rows)
    return w


def rel_err(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def run_case(mods, name, outdir):
    method, backbone, B, extra = CASES[name]
    extra = dict(extra)
    shards = extra.pop("shards", 1)
    cfg = dict(BASE, backbone=backbone, method=method, **extra)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)  # vpt.py:54-55 appends to ./deep_prompt.txt
        try:
            model = build_reference(mods, method, cfg)
        finally:
            os.chdir(cwd)
    sd = model.state_dict()
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in sd.items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    model.eval()
    trainable = [k for k, p in model.named_parameters() if p.requires_grad]
    attns = attention_modules(model, method)
    L = len(attns)
    heads = attns[0].heads
    got_p, got_qkv = {}, {}
    hooks = []
    for i, a in enumerate(attns):
        hooks.append(a.attend.register_forward_hook(lambda m, inp, out, i=i: got_p.__setitem__(i, out.detach().clone())))
        hooks.append(a.to_qkv.register_forward_hook(lambda m, inp, out, i=i: got_qkv.__setitem__(i, out.detach().clone())))
    x = torch.from_numpy(synth.volumes(0, B))
    with torch.no_grad():
        logits = model(x)
    for h in hooks:
        h.remove()
    assert len(got_p) == L and len(got_qkv) == L, f"{name}: hooks fired for {len(got_p)} / {len(got_qkv)} of {L} layers"
    Ts = [got_qkv[i].shape[1] for i in range(L)]
    rows, rows_desc = pooled_rows(model, method, Ts[-1])
    crow = cls_row(model, method)
    which, want_rollout = ATTN_CASES[name]
    layers = list(range(L)) if which is None else [0, L - 1]

    out = {"meta/method": method, "meta/backbone": backbone, "meta/batch": B, "meta/shards": shards,
           "meta/cfg": repr({k: v for k, v in cfg.items()}), "meta/trainable": np.array(trainable),
           "meta/pool_rows": np.array(rows if rows is not None else [-1], dtype=np.int64), "meta/pool_desc": rows_desc,
           "meta/cls_row": np.int64(crow), "meta/Ts": np.array(Ts, dtype=np.int64), "meta/heads": np.int64(heads),
           "meta/layers": np.array(layers, dtype=np.int64), "logits": logits.numpy().astype(np.float32)}
    attend_dev = 0.0
    one_seq = len(set(Ts)) == 1
    r = r16 = None
    if want_rollout:
        assert one_seq, name
        r = weights(rows, B, Ts[0])
        r16 = r.clone()
    for i in range(L - 1, -1, -1):
        inner = got_qkv[i].shape[-1] // 3
        q, k = got_qkv[i][..., :inner], got_qkv[i][..., inner:2 * inner]
        P = probs(q, k, heads, bf16=False)
        attend_dev = max(attend_dev, float((P - got_p[i].double()).abs().max()))
        P16 = None
        if i in layers or want_rollout:
            P16 = probs(q, k, heads, bf16=True)
        if i in layers:
            w = weights(rows, B, Ts[i])
            m = torch.einsum("bi,bhij->bhj", w, P)
            m16 = torch.einsum("bi,bhij->bhj", w, P16)
            out[f"pool/layer{i}"] = m.numpy().astype(np.float32)
            out[f"floor/pool/layer{i}"] = np.float32(rel_err(m16, m))
            if i in (0, L - 1):
                c, c16 = P[:, :, crow, :], P16[:, :, crow, :]
                out[f"cls/layer{i}"] = c.numpy().astype(np.float32)
                out[f"floor/cls/layer{i}"] = np.float32(rel_err(c16, c))
        if want_rollout:
            r = 0.5 * r + 0.5 * torch.einsum("bi,bhij->bhj", r, P).mean(dim=1)
            r16 = 0.5 * r16 + 0.5 * torch.einsum("bi,bhij->bhj", r16, P16).mean(dim=1)
        del P, P16
    if want_rollout:
        out["rollout"] = r.numpy().astype(np.float32)
        out["floor/rollout"] = np.float32(rel_err(r16, r))
    out["meta/attend_dev"] = np.float64(attend_dev)
    path = os.path.join(outdir, f"attn_{name}.npz")
    np.savez_compressed(path, **out)
    floors = {k: float(v) for k, v in out.items() if k.startswith("floor/")}
    print(f"{name}: T={Ts[0]}..{Ts[-1]} H={heads} rows={rows_desc} attend_dev={attend_dev:.2e} max floor={max(floors.values()):.2e} "
          f"-> {path} ({os.path.getsize(path)} bytes)")


def main():
    torch.set_num_threads(8)
    mods = import_reference()
    outdir = os.path.join(ROOT, "tests", "golden")
    names = sys.argv[1:] or list(ATTN_CASES)
    for n in names:
        run_case(mods, n, outdir)


if __name__ == "__main__":
    main()
