#!/usr/bin/env python3
"""Generate tests/golden/relv_<case>.npz -- the class-specific attention relevance (gradient x attention; Chefer, Gur & Wolf 2021,
"Generic Attention-model Explainability") of THE REFERENCE, imported as tools/gen_attention_golden.py does.

Only runs in the build container (the reference never travels).  For each case it
  1. builds the reference model with the synth weights of gaviko_amd.utils.synth, puts it in eval(), runs synth.volumes(0, B) with
     requires_grad (the `linear` case has no trainable tensor below the head),
  2. hooks every global self-attention: the `attend` softmax output and its gradient, the `to_qkv` output, and the input of `to_out`
     with its gradient (dO), and backpropagates logits[b, target[b]].sum(),
  3. folds layer by layer, in the order the backward visits the layers, in float64 (no [L, B, H, T, T] stack ever exists):
       Abar_l = mean_h max(0, A_l * dA_l);   r = w_pool;  for l = L-1 .. 0:  r <- r + r^T Abar_l
       relevance/{argmax,alt}       [B, T]      r for the argmax class and for another class (meta/target_*)
       gradmaps/argmax/layer{0,L-1} [B, H, T]   sum_i w_pool[i] max(0, A * dA)[b, h, i, :]
       meta/dA_dev                              max over layers of  max|dO . V^T - attend.grad| / max|attend.grad|
       floor/operand/<key>                      the same quantity from q * scale * log2(e), k, v and dO rounded to bf16 (the operands of
                                                the bf16 kernels), relative to the largest element
       floor/weights/<key>                      the same quantity from a second run of the reference whose tensors of two or more dimensions
                                                are rounded to bf16
     Both floors of the relevance are taken over the part added to w_pool (r - w_pool): the identity term dominates r itself.
Everything is stored as float32.

Usage:  python tools/gen_relevance_golden.py [case ...]      (no args = all cases)
"""
from __future__ import annotations

import copy
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from gaviko_amd.utils import synth  # noqa: E402
from gen_attention_golden import attention_modules, pooled_rows, probs, rel_err, weights  # noqa: E402
from gen_golden import BASE, CASES, build_reference, import_reference  # noqa: E402

RELV_CASES = ["gaviko_t16_b2", "cfg1_linear_t16_b1", "dvpt_t16_b2_mean_p8", "cfg2_gaviko_b16_b4"]


def heads_of(t, heads):
    B, T, inner = t.shape
    return t.reshape(B, T, heads, inner // heads).transpose(1, 2)


def explain_run(model, method, x, targets, rows):
    """One forward + backward of logits[b, targets[b]] (targets None: the argmax) -> dict(logits, targets, r, r16, gm, gm16, dA_dev)."""
    attns = attention_modules(model, method)
    L, heads = len(attns), attns[0].heads
    st = dict(P={}, qkv={}, dO={}, next=L - 1, dA_dev=0.0, gm={}, gm16={}, r=None, r16=None, w=None)

    def fold(i, dA):
        assert st["next"] == i, f"backward visited layer {i}, expected {st['next']}"
        st["next"] = i - 1
        P, qkv, dO = st["P"].pop(i), st["qkv"].pop(i), st["dO"].pop(i)
        B, T = qkv.shape[:2]
        inner = qkv.shape[-1] // 3
        q, k, v = qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:]
        if st["r"] is None:
            st["w"] = weights(rows, B, T)
            st["r"], st["r16"] = st["w"].clone(), st["w"].clone()
        w = st["w"]
        dA = dA.double()
        dA2 = torch.matmul(heads_of(dO, heads).double(), heads_of(v, heads).double().transpose(-1, -2))
        st["dA_dev"] = max(st["dA_dev"], rel_err(dA2, dA))
        del dA2
        G = torch.relu(P.double() * dA)
        del dA
        P16 = probs(q, k, heads, bf16=True)
        dA16 = torch.matmul(heads_of(dO, heads).float().bfloat16().double(), heads_of(v, heads).float().bfloat16().double().transpose(-1, -2))
        G16 = torch.relu(P16 * dA16)
        del P16, dA16
        if i in (0, L - 1):
            st["gm"][i] = torch.einsum("bi,bhij->bhj", w, G)
            st["gm16"][i] = torch.einsum("bi,bhij->bhj", w, G16)
        st["r"] = st["r"] + torch.einsum("bi,bij->bj", st["r"], G.mean(dim=1))
        st["r16"] = st["r16"] + torch.einsum("bi,bij->bj", st["r16"], G16.mean(dim=1))

    def on_attend(i, out):
        st["P"][i] = out.detach()
        out.register_hook(lambda g, i=i: fold(i, g))

    def on_out_input(i, inp):
        inp[0].register_hook(lambda g, i=i: st["dO"].__setitem__(i, g.detach()))

    hooks = []
    for i, a in enumerate(attns):
        hooks.append(a.attend.register_forward_hook(lambda m, inp, out, i=i: on_attend(i, out)))
        hooks.append(a.to_qkv.register_forward_hook(lambda m, inp, out, i=i: st["qkv"].__setitem__(i, out.detach())))
        hooks.append(a.to_out.register_forward_pre_hook(lambda m, inp, i=i: on_out_input(i, inp)))
    x = x.clone().requires_grad_(True)
    logits = model(x)
    for h in hooks:
        h.remove()
    Ts = [st["qkv"][i].shape[1] for i in range(L)]
    assert len(set(Ts)) == 1, "the relevance needs one token sequence through all layers"
    if targets is None:
        targets = logits.detach().argmax(dim=1)
    logits[torch.arange(logits.shape[0]), targets].sum().backward()
    assert st["next"] == -1, "not every layer's attend gradient arrived"
    return dict(logits=logits.detach(), targets=targets, Ts=Ts, heads=heads, L=L, w=st["w"], r=st["r"], r16=st["r16"], gm=st["gm"],
                gm16=st["gm16"], dA_dev=st["dA_dev"])


def round_weights(model):
    m = copy.deepcopy(model)
    with torch.no_grad():
        for t in list(m.parameters()) + list(m.buffers()):
            if t.dim() >= 2 and t.is_floating_point():
                t.copy_(t.bfloat16().float())
    return m


def run_case(mods, name, outdir):
    method, backbone, B, extra = CASES[name]
    extra = dict(extra)
    extra.pop("shards", 1)
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
    model16 = round_weights(model)
    x = torch.from_numpy(synth.volumes(0, B))
    K = cfg["num_classes"]

    def both(targets):
        a = explain_run(model, method, x, targets, rows)
        b = explain_run(model16, method, x, a["targets"], rows)
        return a, b

    rows, rows_desc = pooled_rows(model, method, None)
    base, base16 = both(None)
    L, w = base["L"], base["w"]
    out = {"meta/method": method, "meta/backbone": backbone, "meta/batch": B, "meta/cfg": repr({k: v for k, v in cfg.items()}),
           "meta/pool_rows": np.array(rows if rows is not None else [-1], dtype=np.int64), "meta/pool_desc": rows_desc,
           "meta/Ts": np.array(base["Ts"], dtype=np.int64), "meta/heads": np.int64(base["heads"]),
           "meta/layers": np.array([0, L - 1], dtype=np.int64), "logits": base["logits"].numpy().astype(np.float32),
           "meta/target_argmax": base["targets"].numpy().astype(np.int64)}

    def put(tag, a, a16, with_maps):
        out[f"relevance/{tag}"] = a["r"].numpy().astype(np.float32)
        out[f"floor/operand/relevance/{tag}"] = np.float32(rel_err(a["r16"] - w, a["r"] - w))
        out[f"floor/weights/relevance/{tag}"] = np.float32(rel_err(a16["r"] - w, a["r"] - w))
        if with_maps:
            for i in sorted(a["gm"]):
                out[f"gradmaps/{tag}/layer{i}"] = a["gm"][i].numpy().astype(np.float32)
                out[f"floor/operand/gradmaps/{tag}/layer{i}"] = np.float32(rel_err(a["gm16"][i], a["gm"][i]))
                out[f"floor/weights/gradmaps/{tag}/layer{i}"] = np.float32(rel_err(a16["gm"][i], a["gm"][i]))

    put("argmax", base, base16, True)
    dA_dev = max(base["dA_dev"], base16["dA_dev"])
    alt = None
    for shift in (2, 1, 3, 4):                      # another class whose relevance differs by more than 10 x the larger floor
        tgt = (base["targets"] + shift) % K
        alt, alt16 = both(tgt)
        put("alt", alt, alt16, False)
        diff = rel_err(alt["r"] - w, base["r"] - w)
        floor = max(float(v) for k, v in out.items() if k.startswith("floor/") and "/relevance/" in k)
        print(f"{name}: alt shift {shift}: relative difference of the added parts {diff:.3e}, larger floor {floor:.3e}")
        if diff > 10 * floor:
            break
    else:
        raise SystemExit(f"{name}: no alt class differs by more than 10 x the floor")
    out["meta/target_alt"] = alt["targets"].numpy().astype(np.int64)
    out["meta/alt_diff"] = np.float64(diff)
    out["meta/dA_dev"] = np.float64(max(dA_dev, alt["dA_dev"]))
    path = os.path.join(outdir, f"relv_{name}.npz")
    np.savez_compressed(path, **out)
    added = float((base["r"] - w).max())
    print(f"{name}: T={base['Ts'][0]} H={base['heads']} rows={rows_desc} max r={float(base['r'].max()):.3e} largest added {added:.3e} "
          f"dA_dev={float(out['meta/dA_dev']):.2e} targets {base['targets'].tolist()} / {alt['targets'].tolist()}")
    for k in sorted(out):
        if k.startswith("floor/"):
            print(f"    {k} {float(out[k]):.3e}")
    print(f"    -> {path} ({os.path.getsize(path)} bytes)")


def main():
    torch.set_num_threads(8)
    mods = import_reference()
    outdir = os.path.join(ROOT, "tests", "golden")
    names = sys.argv[1:] or list(RELV_CASES)
    for n in names:
        run_case(mods, n, outdir)


if __name__ == "__main__":
    main()
