#!/usr/bin/env python3
"""Every static fact of the launch-plan engine, per method, as one JSON record per case -> tests/golden/engine_manifest.json.

For each case below the model is built with registry.build_model on the CPU, its Engine is taken, and the record holds
  * the geometry attributes and feature flags Engine.__init__ sets (an attribute the engine does not have is left out of the record),
  * the name queries (Names, _backbone_weight_names, _fold_deps, trainable_names, flat_names) and, over every parameter name,
    where _own_grad_kernels / _grad_supported answer True,
  * four workspaces (eval, train, keep_attn, feat): the ordered keys, the nesting / shape / dtype of every slot, the number of non-zero
    elements of every tensor and their float64 sum (the `act` bias columns, the seed word), and the count of distinct data_ptr() values.
The file stores a dictionary that occurs more than once (a workspace two methods share, a name list) a single time: pack() / unpack().
No kernel is launched; only gaviko's training workspace needs the built library (gvk_gpa_gate_param_count).
tests/test_engine_manifest.py regenerates the records and compares them with the committed file: a change to a method's geometry, flags,
names or buffers shows up there as the case and key that moved.

Usage:  python tools/engine_manifest.py [out.json]        (default: tests/golden/engine_manifest.json)
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "engine_manifest.json")
SEED = 20261004                        # torch.manual_seed before every workspace: the seed word starts from torch.initial_seed()
# environment switches the engine's flags read: a record describes the defaults
ENV_SWITCHES = ("GAVIKO_HIP_PRECISION", "GAVIKO_HIP_PRUNE", "GAVIKO_HIP_DIAG")

BASE = dict(image_size=160, image_patch_size=16, frames=120, frame_patch_size=12, num_classes=5, channels=1, pool="cls", dim_head=64,
            dropout=0.0, emb_dropout=0.0, backbone="vit-t16")
GAVIKO = dict(num_prompts=32, prompt_latent_dim=20, local_dim=20, local_k=(6, 6, 6), DHW=(10, 10, 10), attn_drop=0.2, proj_drop=0.2,
              freeze_vit=True, share_factor=1, fp16=False)
VPT = dict(num_prompts=8, prompt_dim=64, prompt_dropout=0.0, freeze_vit=True)
EXTRA = {"gaviko": GAVIKO, "linear": {}, "fft": {}, "bitfit": {}, "adaptformer": dict(freeze_vit=True), "dvpt": dict(num_prompts=50, freeze_vit=True),
         "evp": dict(freeze_vit=True), "ssf": dict(freeze_vit=True), "melo": dict(r=4, alpha=4), "deep_vpt": VPT, "shallow_vpt": VPT}

# (case name, method, overrides, B): all eleven registry methods at vit-t16, then the configurations that move a static fact
CASES = [(m, m, {}, 2) for m in ("gaviko", "linear", "fft", "bitfit", "adaptformer", "dvpt", "evp", "ssf", "melo", "deep_vpt", "shallow_vpt")]
CASES += [("gaviko_b16", "gaviko", dict(backbone="vit-b16"), 1),          # _fold_ln1 and the side-tile fusions are live
          ("gaviko_no_dhw", "gaviko", dict(DHW=None), 2),
          ("gaviko_unfrozen", "gaviko", dict(freeze_vit=False), 2),
          ("gaviko_share2", "gaviko", dict(share_factor=2), 2),
          ("gaviko_fp32", "gaviko", dict(precision="fp32"), 2),
          ("dvpt_mean", "dvpt", dict(pool="mean"), 2),
          ("deep_vpt_mean", "deep_vpt", dict(pool="mean"), 2),            # pools Ts[-1] rows of the shrunk sequence
          ("melo_layers", "melo", dict(alpha=8, lora_layer=[0, 5, 11]), 2),
          ("linear_fp32", "linear", dict(precision="fp32"), 2)]
CASE_NAMES = [c[0] for c in CASES]

ATTRS = ("kind", "depth", "heads", "C", "mlp", "patch", "grid", "N", "Kp", "K", "fp32", "q_scale", "adt", "pool", "P", "T", "Ts", "row_off", "Lat",
         "share", "win", "r", "Lp", "freq", "pd", "deep", "adim", "lora_s", "lora_layers", "ldx", "prune_dead_rows", "_fuse_proj", "_dy16",
         "_gelu_grad", "_fuse_local", "_fuse_bnd", "_fuse_next", "_pgrad", "_fuse_up", "_fold_ln1", "_fold_names", "_shadowed")


def _plain(v):
    if isinstance(v, (frozenset, set)):
        v = sorted(v)
        return compact(v) if v and isinstance(v[0], str) else v
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, torch.dtype):
        return str(v)
    return v


def _runs(idx):
    """[0, 1, 2, 5] -> '0-2,5' (in the order given)."""
    out, k = [], 0
    while k < len(idx):
        j = k
        while j + 1 < len(idx) and idx[j + 1] == idx[j] + 1:
            j += 1
        out.append(str(idx[k]) if j == k else f"{idx[k]}-{idx[j]}")
        k = j + 1
    return ",".join(out)


def compact(names):
    """An ordered list of tensor names in a small exact form: its length, the hash of the ordered list, and the names grouped as
    {text before the first layer index: {text after it: the indices that occur, in order of occurrence}} (names without one: under '')."""
    groups = {}
    for n in names:
        m = re.search(r"\.(\d+)(\.|$)", n)
        if m:
            groups.setdefault(n[:m.start(1)], {}).setdefault(n[m.end(1):], []).append(int(m.group(1)))
        else:
            groups.setdefault("", {})[n] = []
    return {"n": len(names), "sha256": hashlib.sha256("\n".join(names).encode()).hexdigest()[:16],
            "groups": {pre: {k: _runs(v) for k, v in g.items()} for pre, g in groups.items()}}


DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.int64: "i64"}


def describe(v, ptrs):
    """Nesting, shape and dtype of one workspace slot.  A tensor is 'f32[rows,cols]', followed by ' nnz=<non-zero elements> sum=<their
    float64 sum>' where it is not all zero; a dict keeps its key order in 'keys'; a list is its runs of identical entries."""
    if isinstance(v, torch.Tensor):
        ptrs.append(v.data_ptr())
        nnz = int(torch.count_nonzero(v))
        return DT[v.dtype] + json.dumps(list(v.shape), separators=(",", ":")) + (f" nnz={nnz} sum={float(v.sum(dtype=torch.float64))!r}" if nnz else "")
    if isinstance(v, dict):
        return {"keys": ",".join(v), "dict": {k: describe(x, ptrs) for k, x in v.items()}}
    if isinstance(v, (list, tuple)):
        out = []
        for d in (describe(x, ptrs) for x in v):              # runs of identical entries -> [count, entry]
            if out and out[-1][1] == d:
                out[-1][0] += 1
            else:
                out.append([1, d])
        return {"list": out}
    return _plain(v)


def tensor_fields(desc):
    """'f32[2,3] nnz=2 sum=2.0' -> ('f32', [2, 3], 2, 2.0)."""
    m = re.fullmatch(r"([a-z0-9]+)(\[[0-9,]*\])(?: nnz=(\d+) sum=(\S+))?", desc)
    return m.group(1), json.loads(m.group(2)), int(m.group(3) or 0), float(m.group(4) or 0.0)


def workspace_record(eng, B, **kw):
    torch.manual_seed(SEED)
    eng._wss.clear()                                         # one workspace alive at a time
    ws = eng.workspace(B, torch.device("cpu"), **kw)
    ptrs = []
    slots = {k: describe(v, ptrs) for k, v in ws.items()}
    return {"keys": ",".join(ws), "slots": slots, "tensors": len(ptrs), "distinct_ptrs": len(set(ptrs))}


def record(method, over, B):
    from gaviko_amd.registry import build_model
    model = build_model(dict(BASE, method=method, **dict(EXTRA[method], **over)))
    eng = model._engine()
    nm, depth = eng.names, eng.depth
    rec = {"B": B, "attrs": {a: _plain(getattr(eng, a)) for a in ATTRS if hasattr(eng, a)}}
    rec["pool_rows"] = list(eng._pool_rows())
    rec["backbone_weight_names"] = compact(eng._backbone_weight_names())
    if eng._fold_ln1:
        rec["fold_deps"] = compact(eng._fold_deps())
    rec["trainable_names"] = compact(eng.trainable_names())
    rec["flat_names"] = compact(eng.flat_names())
    rec["own_grad_kernels"] = compact([n for n in eng.p if eng._own_grad_kernels(n)])
    rec["grad_supported"] = compact([n for n in eng.p if eng._grad_supported(n)])
    rec["names"] = {"root": nm.root, "conv": nm.conv(), "head": nm.head()}
    for i in sorted({0, depth - 1}):
        rec["names"][f"layer{i}"] = {"attn": nm.attn(i), "mlp": nm.mlp(i), "qkv_weight": nm.qkv_weight(i)}
    rec["workspaces"] = {"eval": workspace_record(eng, B, train=False), "train": workspace_record(eng, B, train=True),
                         "keep_attn": workspace_record(eng, B, train=False, keep_attn=True),
                         "feat": workspace_record(eng, B, train=False, feat=(0, depth))}
    eng._wss.clear()
    return rec


def generate():
    """{case name: record} for every case, with the engine's environment switches at their defaults."""
    saved = {k: os.environ.pop(k) for k in ENV_SWITCHES if k in os.environ}
    try:
        return {name: record(method, over, B) for name, method, over, B in CASES}
    finally:
        os.environ.update(saved)


def _dump(v):
    return json.dumps(v, separators=(",", ":"))


def pack(records):
    """The file form of generate()'s records.  The train / keep_attn / feat workspaces of a case hold only the slots that differ from its
    eval workspace ('keys' keeps the whole order); then every dictionary or string of 100 characters or more that occurs more than once
    (a workspace two methods share, a name list, a per-layer slot, a key order) is stored once under 'shared' and referred to as '@<n>'."""
    records = json.loads(_dump(records))
    for rec in records.values():
        base = rec["workspaces"]["eval"]["slots"]
        for tag in ("train", "keep_attn", "feat"):
            w = rec["workspaces"][tag]
            w["unlike_eval"] = {k: v for k, v in w.pop("slots").items() if base.get(k) != v}
    seen = {}

    def big(v):
        return isinstance(v, (dict, str)) and len(_dump(v)) >= 100

    def count(v):
        for x in (v.values() if isinstance(v, dict) else v if isinstance(v, list) else ()):
            count(x)
        if big(v):
            seen[_dump(v)] = seen.get(_dump(v), 0) + 1

    count(records)
    shared, ids = {}, {}

    def fold(v):
        if isinstance(v, list):
            return [fold(x) for x in v]
        folded = {k: fold(x) for k, x in v.items()} if isinstance(v, dict) else v      # children first: they get the lower numbers
        if not big(v) or seen[_dump(v)] < 2:
            return folded
        if _dump(v) not in ids:
            ids[_dump(v)] = f"@{len(ids)}"
            shared[ids[_dump(v)]] = folded
        return ids[_dump(v)]

    return {"shared": shared, "cases": {name: fold(rec) for name, rec in records.items()}}


def unpack(packed):
    """pack() undone: {case name: record}."""
    shared = packed["shared"]

    def un(v):
        if isinstance(v, str) and v in shared:
            return un(shared[v])
        if isinstance(v, list):
            return [un(x) for x in v]
        return {k: un(x) for k, x in v.items()} if isinstance(v, dict) else v

    records = {name: un(rec) for name, rec in packed["cases"].items()}
    for rec in records.values():
        base = rec["workspaces"]["eval"]["slots"]
        for tag in ("train", "keep_attn", "feat"):
            w = rec["workspaces"][tag]
            unlike = w.pop("unlike_eval")
            slots = {k: unlike[k] if k in unlike else base[k] for k in w["keys"].split(",")}
            rec["workspaces"][tag] = {"keys": w["keys"], "slots": slots, "tensors": w["tensors"], "distinct_ptrs": w["distinct_ptrs"]}
    return records


def write(packed, path):
    """One line per shared entry and per case."""
    with open(path, "w") as f:
        f.write('{"shared":{\n' + ",\n".join(f"{_dump(k)}:{_dump(v)}" for k, v in packed["shared"].items()) + '\n},\n"cases":{\n')
        f.write(",\n".join(f"{_dump(k)}:{_dump(v)}" for k, v in packed["cases"].items()) + "\n}}\n")


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    write(pack(generate()), out)
    print(f"wrote {out} ({os.path.getsize(out)} bytes, {len(CASES)} cases)")
