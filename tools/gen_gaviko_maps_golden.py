#!/usr/bin/env python3
"""Generate tests/golden/gmaps_<case>.npz -- the MWSA local-attention and GPA prompt-attention probabilities of THE REFERENCE (imported as
tools/gen_golden.py does).

Only runs in the build container (the reference never travels).  For each case it
  1. builds the reference model with the synth weights of gaviko_amd.utils.synth, puts it in eval(), runs synth.volumes(0, B),
  2. records the probabilities the reference's own forward computed: torch.nn.functional.softmax is wrapped for the duration of the
     forward and every call is tagged by the module that is running -- LocalSelfAttention (gaviko.py:238) through a forward pre-hook,
     the two BaseFusionAttention.forward (gaviko.py:91) through a hook on their inner query_proj (Awakening_Prompt calls .forward(...) of
     global_attention / local_attention / cls_analyzer / gl_balancer directly, so hooks on those never fire); shared modules
     (share_factor > 1) fire once per layer and are indexed by call order,
  3. recomputes each block in float64 from the hooked operands (qkv, query_proj and proj_down outputs); the largest deviation from the
     recorded softmax is meta/softmax_dev,
  4. stores, as float32, reductions of the float64 blocks (N = patches, P = prompts; global blocks are padded with the P + 1 leading
     zeros of the reference's double slice, gaviko.py:161,107, so index n is the patch position in all three):
       local/all/layer{i}          [B, N]  mean over the query rows of the MWSA probabilities (uniform weights 1 / N)
       local/row{q}/layer{i}       [B, N]  row q of P, q = 0 (a grid corner) and the centre query, first and last layer
       gpa/global_mean|local_mean|fused_mean/layer{i}   [B, N]  mean over the prompts
       gpa/importance/layer{i} [B, P], gpa/global_weight/layer{i} [B]   (outputs of the hooked cls_analyzer_ / gl_balancer_)
       gpa/global|local|fused/layer{i}   [B, len(meta/block_prompts), N]  whole rows of the blocks, first and last layer
                                          (every prompt when B * P <= 12, else an evenly spaced subset: file size)
       local_rollout               [B, N]  r = 1 / N; for l = L-1 .. 0: r <- 0.5 r + 0.5 r^T P_l
     for the layers in meta/layers (all of them; the first and the last for the ViT-B case),
  5. floor/<key>: max|x_bf16 - x| / max|x| of the same quantity computed the same way from the local / global streams of the oracle
     (oracle.gaviko_ref) run once in fp32 and once in its BF16_OPERANDS mode, as tools/noise_floor.py does: the precision floor of any
     bf16 backbone feeding these maps (the side paths themselves stay fp32 in both runs).

Usage:  python tools/gen_gaviko_maps_golden.py [case ...]      (no args = all cases)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gaviko_amd.utils import synth  # noqa: E402
from gen_golden import BASE, CASES, build_reference, import_reference  # noqa: E402
from oracle import gaviko_ref, vit_ref  # noqa: E402

# case -> which layers are stored (None = all)
GMAPS_CASES = {
    "gaviko_t16_b2": None,
    "gaviko_t16_b2_k366_p8": None,
    "gaviko_t16_b2_lat16": None,
    "gaviko_t16_b1_share2": None,
    "cfg2_gaviko_b16_b4": "ends",
}


def rel_err(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def block_prompts(B, P):
    n = max(1, min(P, 12 // B))
    return sorted({int(round(v)) for v in np.linspace(0, P - 1, n)})


def record_reference(model, x):
    """One forward of the reference -> per layer (call order) the recorded softmax outputs and the hooked operands."""
    tr = model.transformer
    rec = {k: [] for k in ("p_local", "p_global", "p_gpalocal", "qkv", "qg", "ql", "down", "imp", "gw")}
    cur = {"tag": None}
    hooks = []
    orig = F.softmax

    def tagged_softmax(*a, **kw):
        out = orig(*a, **kw)
        if cur["tag"] is not None:                    # (the backbone's nn.Softmax comes through here too, untagged)
            rec[cur["tag"]].append(out.detach().clone())
            cur["tag"] = None
        return out

    def tag(name):
        return lambda *_: cur.__setitem__("tag", name)

    def keep(name):
        return lambda m, inp, out: rec[name].append(out.detach().clone())

    for la in tr.local_attns:
        hooks.append(la.register_forward_pre_hook(tag("p_local")))
        hooks.append(la.qkv.register_forward_hook(keep("qkv")))
    for pp in tr.prompt_projs:
        hooks.append(pp.proj_down.register_forward_hook(keep("down")))                       # fires twice per layer: global, local
        hooks.append(pp.global_attention.query_proj.register_forward_hook(keep("qg")))
        hooks.append(pp.global_attention.query_proj.register_forward_hook(tag("p_global")))
        hooks.append(pp.local_attention.query_proj.register_forward_hook(keep("ql")))
        hooks.append(pp.local_attention.query_proj.register_forward_hook(tag("p_gpalocal")))
        hooks.append(pp.cls_analyzer.cls_analyzer_.register_forward_hook(keep("imp")))
        hooks.append(pp.gl_balancer.gl_balancer_.register_forward_hook(keep("gw")))
    F.softmax = tagged_softmax
    try:
        with torch.no_grad():
            logits = model(x)
    finally:
        F.softmax = orig
        for h in hooks:
            h.remove()
    L = tr.depth
    assert all(len(rec[k]) == L for k in rec if k != "down") and len(rec["down"]) == 2 * L, {k: len(v) for k, v in rec.items()}
    return logits, rec


def local_probs(qkv, mask, scale):
    """MWSA probabilities [B, N, N] float64 from the qkv projection's output (gaviko.py:233-238)."""
    q, k, _ = qkv.double().chunk(3, dim=-1)
    return torch.softmax(q @ k.transpose(-2, -1) * scale + mask.double().unsqueeze(0), dim=-1)


def cross_probs(q, tokens):
    """BaseFusionAttention's probabilities [B, P, n] float64 (gaviko.py:90-91)."""
    return torch.softmax(torch.einsum("bpd,bnd->bpn", q.double(), tokens.double()) * (q.shape[-1] ** -0.5), dim=-1)


def gpa_blocks(qg, ql, x_lat, l_lat, imp, gw, P):
    """-> global (padded to the N patch positions), local, fused [B, P, N] float64 (gaviko.py:161,107,170-178)."""
    pl = cross_probs(ql, l_lat)
    pg_live = cross_probs(qg, x_lat[:, 2 * P + 2:])
    pg = torch.zeros_like(pl)
    pg[:, :, P + 1:] = pg_live
    imp, gw = imp.double().reshape(imp.shape[0], P, 1), gw.double().reshape(-1, 1, 1)
    return pg, pl, imp * (gw * pg + (1 - gw) * pl), pg_live


def quantities(layers_data, layers, rows, prompts):
    """layers_data[i] = (P_local, pg, pl, fused, imp, gw) float64 for EVERY layer -> {key: float64 tensor} of what is stored."""
    out = {}
    L = len(layers_data)
    r = None
    for i in range(L - 1, -1, -1):
        P_loc, pg, pl, fu, imp, gw = layers_data[i]
        if r is None:
            r = torch.full(P_loc.shape[:2], 1.0 / P_loc.shape[1], dtype=torch.float64)
        r = 0.5 * r + 0.5 * torch.einsum("bi,bij->bj", r, P_loc)
        if i not in layers:
            continue
        out[f"local/all/layer{i}"] = P_loc.mean(dim=1)
        out[f"gpa/global_mean/layer{i}"], out[f"gpa/local_mean/layer{i}"], out[f"gpa/fused_mean/layer{i}"] = pg.mean(1), pl.mean(1), fu.mean(1)
        out[f"gpa/importance/layer{i}"], out[f"gpa/global_weight/layer{i}"] = imp.double().reshape(imp.shape[0], -1), gw.double().reshape(-1)
        if i in (0, L - 1):
            for q in rows:
                out[f"local/row{q}/layer{i}"] = P_loc[:, q, :]
            out[f"gpa/global/layer{i}"], out[f"gpa/local/layer{i}"], out[f"gpa/fused/layer{i}"] = pg[:, prompts], pl[:, prompts], fu[:, prompts]
    out["local_rollout"] = r
    return out


def oracle_layers(sd, x, cfg, bf16):
    """The same blocks from the oracle's streams (taps), in fp32 or BF16_OPERANDS mode -> layers_data."""
    depth = vit_ref.mapping_vit(cfg["backbone"])[0]
    P, share = cfg["num_prompts"], cfg.get("share_factor", 1)
    taps = {}
    old = vit_ref.BF16_OPERANDS
    vit_ref.BF16_OPERANDS = bf16
    try:
        with torch.no_grad():
            gaviko_ref.gaviko_forward(sd, x, cfg, taps)
    finally:
        vit_ref.BF16_OPERANDS = old
    mask = gaviko_ref.window_mask(tuple(cfg["DHW"]), tuple(cfg["local_k"]))
    data = []
    for i in range(depth):
        s = i // share
        la, gp = f"transformer.local_attns.{s}", f"transformer.prompt_projs.{s}"
        lin = taps["embed.local"] if i == 0 else taps[f"layer{i - 1}.local"]
        lat = F.linear(vit_ref.layer_norm(sd, la + ".norm", lin), sd[la + ".proj_down.weight"], sd[la + ".proj_down.bias"])
        P_loc = local_probs(F.linear(lat, sd[la + ".qkv.weight"]), mask, lin.shape[-1] ** -0.5)
        wd, bd = sd[gp + ".proj_down.0.weight"], sd[gp + ".proj_down.0.bias"]
        qgelu = lambda t: t * torch.sigmoid(1.702 * t)
        x_lat, l_lat = qgelu(F.linear(taps[f"layer{i}.post_attn"], wd, bd)), qgelu(F.linear(taps[f"layer{i}.local"], wd, bd))
        cls = x_lat[:, P:P + 1]
        a, g = gp + ".cls_analyzer.cls_analyzer_", gp + ".gl_balancer.gl_balancer_"
        h = F.gelu(F.linear(F.layer_norm(cls, (cls.shape[-1],), sd[a + ".0.weight"], sd[a + ".0.bias"]), sd[a + ".1.weight"], sd[a + ".1.bias"]))
        imp = torch.sigmoid(F.linear(h, sd[a + ".3.weight"], sd[a + ".3.bias"]))
        gw = torch.sigmoid(F.linear(F.layer_norm(cls, (cls.shape[-1],), sd[g + ".0.weight"], sd[g + ".0.bias"]), sd[g + ".1.weight"], sd[g + ".1.bias"]))
        qg = F.linear(x_lat[:, :P], sd[gp + ".global_attention.query_proj.weight"], sd[gp + ".global_attention.query_proj.bias"])
        ql = F.linear(x_lat[:, :P], sd[gp + ".local_attention.query_proj.weight"], sd[gp + ".local_attention.query_proj.bias"])
        pg, pl, fu, _ = gpa_blocks(qg, ql, x_lat, l_lat, imp, gw, P)
        data.append((P_loc, pg, pl, fu, imp, gw))
    return data


def run_case(mods, name, outdir):
    method, backbone, B, extra = CASES[name]
    assert method == "gaviko", name
    cfg = dict(BASE, backbone=backbone, method=method, **dict(extra))
    model = build_reference(mods, method, cfg)
    sd = model.state_dict()
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in sd.items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    model.eval()
    x = torch.from_numpy(synth.volumes(0, B))
    logits, rec = record_reference(model, x)
    tr = model.transformer
    L, P, share = tr.depth, model.num_prompts, tr.share_factor
    grid, win = tuple(cfg["DHW"]), tuple(cfg["local_k"])
    N = grid[0] * grid[1] * grid[2]
    rows = [0, ((grid[0] // 2) * grid[1] + grid[1] // 2) * grid[2] + grid[2] // 2]
    prompts = block_prompts(B, P)
    layers = list(range(L)) if GMAPS_CASES[name] is None else [0, L - 1]

    dev = 0.0
    data = []
    for i in range(L):
        la = tr.local_attns[i // share]
        P_loc = local_probs(rec["qkv"][i], la.mask[0], la.scale)
        dev = max(dev, float((P_loc - rec["p_local"][i].double()).abs().max()))
        x_lat, l_lat = rec["down"][2 * i], rec["down"][2 * i + 1]
        pg, pl, fu, pg_live = gpa_blocks(rec["qg"][i], rec["ql"][i], x_lat, l_lat, rec["imp"][i], rec["gw"][i], P)
        assert rec["p_global"][i].shape == pg_live.shape and rec["p_gpalocal"][i].shape == pl.shape, name
        dev = max(dev, float((pg_live - rec["p_global"][i].double()).abs().max()), float((pl - rec["p_gpalocal"][i].double()).abs().max()))
        data.append((P_loc, pg, pl, fu, rec["imp"][i], rec["gw"][i]))
    ref = quantities(data, layers, rows, prompts)
    del data

    osd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ocfg = {k: v for k, v in cfg.items()}
    q32 = quantities(oracle_layers(osd, x, ocfg, False), layers, rows, prompts)
    q16 = quantities(oracle_layers(osd, x, ocfg, True), layers, rows, prompts)
    oracle_dev = max(rel_err(q32[k], ref[k]) for k in ref)          # the oracle's fp32 run against the reference's own blocks

    out = {"meta/method": method, "meta/backbone": backbone, "meta/batch": B, "meta/cfg": repr(cfg), "meta/layers": np.array(layers, dtype=np.int64),
           "meta/rows": np.array(rows, dtype=np.int64), "meta/block_prompts": np.array(prompts, dtype=np.int64),
           "meta/grid": np.array(grid, dtype=np.int64), "meta/window": np.array(win, dtype=np.int64), "meta/num_prompts": np.int64(P),
           "meta/depth": np.int64(L), "meta/softmax_dev": np.float64(dev), "meta/oracle_dev": np.float64(oracle_dev),
           "logits": logits.numpy().astype(np.float32)}
    for k, v in ref.items():
        out[k] = v.numpy().astype(np.float32)
        out["floor/" + k] = np.float32(rel_err(q16[k], q32[k]))
    path = os.path.join(outdir, f"gmaps_{name}.npz")
    np.savez_compressed(path, **out)
    floors = {k: float(v) for k, v in out.items() if k.startswith("floor/")}
    print(f"{name}: L={L} P={P} N={N} window={win} softmax_dev={dev:.2e} oracle_dev={oracle_dev:.2e} max floor={max(floors.values()):.2e} "
          f"({max(floors, key=floors.get)}) -> {path} ({os.path.getsize(path)} bytes)")


def main():
    torch.set_num_threads(8)
    mods = import_reference()
    outdir = os.path.join(ROOT, "tests", "golden")
    for n in sys.argv[1:] or list(GMAPS_CASES):
        run_case(mods, n, outdir)


if __name__ == "__main__":
    main()
