"""The static facts of every engine kind, one stateless spec per kind (METHOD_SPECS): token geometry, feature flags, the method's own
workspace slots, which tensors its own gradient kernels cover, the rows the head pools, and the state_dict name patterns of its reference
class.  Engine.__init__ looks its kind up once (`self.method`) and engine_common.Names reads the patterns; the sweeps of engine.py and its
mixins still choose their LAUNCHES by `self.kind` -- nothing here launches anything.  The plain ViT is the base class: a method overrides
only where it differs."""
from __future__ import annotations

import os

import torch

from . import lib as L
from . import ops


def _mk(device):
    return lambda *s: torch.zeros(s, device=device)


class VitSpec:
    """Plain ViT (`linear` / `bitfit` / `fft`): [cls | patches], no tensors of its own."""
    # state_dict names of the reference class below `root` (%d = the layer), read by engine_common.Names
    root = ""
    attn_name = "transformer.layers.%d.0"
    mlp_name = "transformer.layers.%d.1"
    conv_name = "conv_proj.0"
    head_name = "mlp_head"
    wraps_qkv = False               # MeLO: to_qkv of the listed layers is a wrapper module around the frozen projection
    # backbone tensors can train (engine_peft.py `_bb_*`): the plain ViT (`fft` / `bitfit`); every class that freezes by default, with freeze_vit=False
    backbone_trainable = True
    supports_prune = False          # Engine.set_prune: dead-row pruning exists on the frozen GAViKO path only

    def share_factor(self, cfg) -> int:
        """Layers that share one side-path module (distributed.flat_order groups their gradients)."""
        return 1

    def geometry(self, eng, cfg) -> None:
        """Token layout: P prompts, T tokens per sample, the first patch row, and Ts[i] = tokens entering layer i."""
        eng.lora_layers = frozenset()
        eng.P, eng.T, eng.row_off = 0, 1 + eng.N, 1
        eng.Ts = [eng.T] * eng.depth

    def flags(self, eng, cfg) -> None:
        """The fusions and shortcuts of the frozen GAViKO path (GavikoSpec.flags explains each): off everywhere else."""
        eng._fuse_proj = eng.prune_dead_rows = eng._dy16 = eng._gelu_grad = False
        eng._fuse_local = eng._fuse_bnd = eng._fuse_next = False
        eng._pgrad = eng._fuse_up = eng._fold_ln1 = False

    def forward_buffers(self, eng, ws, B, device, train, nsave) -> None:
        """The method's own workspace slots, after the shared forward slots (nsave = per-layer copies the forward keeps)."""

    def scratch_lat(self, eng) -> int:
        """Latent width the generic wgrad scratch is sized for."""
        return 1

    def backward_buffers(self, eng, ws, B, device) -> None:
        """The method's own training-only slots, after the shared backward slots."""
        ws["scratch"] = torch.zeros(max(128 * eng.C, ops.outer_scratch_elems(self.scratch_lat(eng), eng.C)), device=device)

    def owns(self, name: str) -> bool:
        """The method's OWN trainable tensors (prompts, adapters, LoRA factors, ...): gradients from the method-specific kernels."""
        return False

    def pool_rows(self, eng):
        """(first row, row count) of the final stream the classification head averages."""
        return (0, eng.Ts[-1]) if eng.pool == "mean" else (0, 1)

    def final_stream(self, eng, ws, train):
        return ws["G"][eng.depth] if train else ws["G"][eng.depth & 1]


class GavikoSpec(VitSpec):
    """GAViKO: [P prompts | cls | patches], the MWSA local stream and the GPA prompt attention beside every layer."""
    attn_name = "transformer.attns.%d"
    mlp_name = "transformer.mlps.%d"
    head_name = "mlp_head.head"
    supports_prune = True

    def share_factor(self, cfg) -> int:
        return cfg.get("share_factor", 1)

    def geometry(self, eng, cfg) -> None:
        eng.lora_layers = frozenset()
        eng.P = cfg["num_prompts"]
        eng.Lat = cfg.get("prompt_latent_dim", 20)
        if cfg.get("local_dim", 20) != eng.Lat:
            raise L.GavikoHipError("local_dim and prompt_latent_dim must match (one latent width per build)")
        eng.share = cfg.get("share_factor", 1)
        eng.T = eng.P + 1 + eng.N
        eng.row_off = eng.P + 1
        dhw = cfg.get("DHW", (10, 10, 10))
        if dhw is None:
            eng.win = tuple(2 * g + 1 for g in eng.grid)     # no mask == a window that always covers the grid
        else:
            if tuple(dhw) != eng.grid:
                raise L.GavikoHipError(f"DHW={tuple(dhw)} does not match the patch grid {eng.grid}")
            eng.win = tuple(cfg.get("local_k", (3, 6, 6)))
        eng.Ts = [eng.T] * eng.depth

    def flags(self, eng, cfg) -> None:
        dim = eng.C
        # GPA projections of backbone rows ride along in the backbone's LayerNorm kernels (gvk_layernorm_fwd_proj, gvk_ln_bwd_desc.proj)
        eng._fuse_proj = (not eng.fp32 and ops.rowproj_supported(eng.Lat, dim) and L.diag_env("GAVIKO_HIP_FUSE_PROJ", "1") != "0")
        # In the backward, the LayerNorm-1 backward of layer i > 0 also leaves dcomb = dG . W_up for the GPA core of layer i - 1 (computing it
        # on the GPA stream instead was measured slower and removed: DESIGN.md 7e).
        # Rows nobody consumes are not computed (round 5).  With a frozen backbone the loss reads the LAST layer's output only at the rows
        # the head pools (prompts + CLS, gaviko.py:316), so that layer's MLP -- a row-wise function -- runs on those rows in the forward, and
        # its backward (fc2 / fc1 dgrad, LayerNorm 2) on the same rows: every other row of the incoming gradient is an exact zero.  At the
        # other end only the P prompt rows of the FIRST layer's input carry a trainable tensor (patch embedding, cls token and position
        # embedding are frozen: gaviko.py:540-548), so its qkv dgrad and LayerNorm-1 backward run on those rows.  Logits and every gradient
        # are bit-identical to the full computation (tests/test_model_gpu.py::test_pruned_rows_are_dead); GAVIKO_HIP_PRUNE=0 computes
        # everything (the golden taps of the last layer's far rows need that).
        eng.prune_dead_rows = not eng.fp32 and os.environ.get("GAVIKO_HIP_PRUNE", "1") != "0"
        # frozen backbone: the fc1 / qkv dgrad GEMMs hand the LayerNorm backward its input gradient in bf16 (half the bytes on both sides; the other
        # operands of that chain -- dpre, dqkv, the dgrad operands -- are bf16 already)
        eng._dy16 = not eng.fp32 and L.diag_env("GAVIKO_HIP_DY16", "1") != "0"
        # ... and fc1's forward epilogue leaves GELU'(pre) instead of pre (it has the exponential in hand and VALU to spare behind its two output
        # streams); the fc2 dgrad epilogue then multiplies instead of evaluating the derivative (isolated: 33.7 -> 30.3 us with a free derivative)
        eng._gelu_grad = not eng.fp32 and L.diag_env("GAVIKO_HIP_GELU_GRAD", "1") != "0"
        eng._fuse_local = ops.side_tile_supported(eng.Lat, dim)
        eng._fuse_bnd = eng._fuse_local and L.diag_env("GAVIKO_HIP_FUSE_BOUNDARY", "1") != "0"
        eng._fuse_next = eng._fuse_local and L.diag_env("GAVIKO_HIP_FUSE_NEXT", "1") != "0"
        # every parameter gradient of a side-path module of one layer in ONE launch per stream (csrc/paramgrad.hip; round 4)
        eng._pgrad = (ops.param_grads_supported(cfg.get("prompt_latent_dim", 20), dim) and L.diag_env("GAVIKO_HIP_PGRAD", "1") != "0")
        # GPA up-projection as K-concatenation of the MLP's second Linear: 64 spare K columns carry the rank-L product in split-bf16 form,
        # A' = [act | lat_hi | lat_lo | lat_hi | 1 | 1], W' = [W_fc2 | Wup_hi | Wup_hi | Wup_lo | b_hi | b_lo] (fp32-grade: the dropped
        # lo.lo term is 2^-16 relative), so x + ff(x) + proj_up(.) (gaviko.py:187 after vision_transformer.py:34) is ONE GEMM and the
        # main stream loses a full read-modify-write pass over the token stream per layer
        eng._fuse_up = (not eng.fp32 and 3 * eng.Lat + 2 <= 64 and L.diag_env("GAVIKO_HIP_FUSE_UP", "1") != "0")
        # First LayerNorm of layers 1.. folded into their qkv projection (vision_transformer.py:49,61-62): the fc2 GEMM of the layer below
        # leaves the bf16 copy of its output rows and per-row (sum, sum of squares) partials, the prompt-fix kernel turns them into mean /
        # rstd, and the qkv GEMM runs on the RAW rows against gamma o W with  rstd * (acc - mean * c1) + c2  in its epilogue -- one launch
        # (and its dependency gap) less per layer on the main stream.  128-column tiles only (C % 128 == 0: ViT-B / ViT-L).
        eng._fold_ln1 = (eng._fuse_up and eng._fuse_proj and dim % 128 == 0 and L.diag_env("GAVIKO_HIP_FOLD_LN1", "1") != "0")

    def forward_buffers(self, eng, ws, B, device, train, nsave) -> None:
        Lt, P, BN, M, C, mk = eng.Lat, eng.P, B * eng.N, B * eng.T, eng.C, _mk(device)
        ws["Lc"] = [torch.zeros((BN, C), device=device) for _ in range((eng.depth + 1) if train else 2)]
        ws["mw"] = [dict(mean=mk(BN), rstd=mk(BN), lat=mk(BN, Lt), qkv=mk(BN, 3 * Lt), ctx=mk(BN, Lt), lse=mk(BN)) for _ in range(nsave)]
        ws["gp"] = [dict(zx=mk(M, Lt), xl=mk(M, Lt), zl=mk(BN, Lt), ll=mk(BN, Lt), imp=mk(B, P), gw=mk(B), enh=mk(B, P, Lt),
                         prm=mk(B, P, Lt), qg=mk(B, P, Lt), ql=mk(B, P, Lt), cg=mk(B, P, Lt), cl=mk(B, P, Lt), lse_g=mk(B, P),
                         lse_l=mk(B, P)) for _ in range(nsave)]

    def backward_buffers(self, eng, ws, B, device) -> None:
        Lt, P, BN, M, C, mk = eng.Lat, eng.P, B * eng.N, B * eng.T, eng.C, _mk(device)
        ng = ops.gpa_gate_param_count(Lt, P)
        ws["dL"] = [mk(BN, C), mk(BN, C)]
        ws["dGb"] = ops.act_zeros(M, C, torch.float32, device)       # second layer-boundary gradient buffer (parity ping-pong)
        ws["bw"] = dict(dcomb=mk(M, Lt), dimp=mk(B, P), dgw_part=mk(B, P), dqg=mk(B, P, Lt), dql=mk(B, P, Lt), dcg=mk(B, P, Lt),
                        dcl=mk(B, P, Lt), delta_g=mk(B, P), delta_l=mk(B, P), dprm=mk(B, P, Lt), dcls=mk(B, Lt),
                        gate_partials=mk(B, ng), dzx=mk(M, Lt), dzl=[mk(BN, Lt), mk(BN, Lt)],
                        dctx=mk(BN, Lt), dqkv=mk(BN, 3 * Lt), wdelta=mk(BN), dlat=mk(BN, Lt), Q=mk(Lt, C), S=mk(Lt))
        ws["scratch"] = mk(max(ops.outer_scratch_elems(Lt, C), 128 * C, 64 * 3 * Lt * Lt, 64 * ng))
        ws["rscratch"] = mk(32 * (ng + 2 * Lt * Lt + 3 * Lt + 3 * Lt * Lt + 64))
        ws["scratch_l"] = mk(max(ops.outer_scratch_elems(Lt, C), 128 * C))      # the MWSA chain runs on its own stream
        ws["rscratch_l"] = mk(32 * (3 * Lt * Lt + Lt + 64))
        if eng._pgrad:                                                           # one scratch + ticket block per stream (gvk_param_grads)
            nct = (C + 63) // 64
            ws["pscratch"] = mk(ops.param_grads_scratch_elems(Lt, [nct, nct], [ng, Lt * Lt, Lt, Lt * Lt, Lt, Lt]))
            ws["pscratch_l"] = mk(ops.param_grads_scratch_elems(Lt, [nct, nct, (3 * Lt + 63) // 64], []))   # third job: the qkv weight, 3 Lat columns (two tiles from Lat = 24)
            ws["ptick"] = torch.zeros(ops.PGRAD_TICKETS, dtype=torch.int32, device=device)
            ws["ptick_l"] = torch.zeros(ops.PGRAD_TICKETS, dtype=torch.int32, device=device)

    def owns(self, name: str) -> bool:
        return "local_attns" in name or "prompt_projs" in name or name in ("prompt_embeddings", "prompt_positional_embedding")

    def pool_rows(self, eng):
        return 0, eng.P + 1                       # gaviko.py:316 prompts + CLS


class DvptSpec(VitSpec):
    """DVPT: [P prompts | cls | patches], the prompts re-weighted by a shared rank-20 MLP before every layer."""
    attn_name = "transformer.layers.%d.0.attn"
    mlp_name = "transformer.layers.%d.0.mlp"

    def geometry(self, eng, cfg) -> None:
        eng.lora_layers = frozenset()
        eng.P = cfg.get("num_prompts", 50)
        eng.Lat = 20                                                                  # share_MLP.latent_dim (dvpt.py:27)
        eng.T, eng.row_off = eng.P + 1 + eng.N, eng.P + 1
        eng.Ts = [eng.T] * eng.depth

    def forward_buffers(self, eng, ws, B, device, train, nsave) -> None:
        mk = _mk(device)
        ws["dv"] = [dict(z=mk(B * eng.T, eng.Lat), enh=mk(B, eng.P, eng.Lat), lse=mk(B, eng.P)) for _ in range(nsave)]

    def backward_buffers(self, eng, ws, B, device) -> None:
        Lt, P, M, mk = eng.Lat, eng.P, B * eng.T, _mk(device)
        ws["dvb"] = dict(dcomb=mk(M, Lt), dz=mk(M, Lt), delta=mk(B, P))
        ws["scratch"] = mk(max(ops.outer_scratch_elems(Lt, eng.C), 128 * eng.C))
        ws["rscratch"] = mk(32 * (Lt + 64))

    def owns(self, name: str) -> bool:
        return "prompt" in name

    def pool_rows(self, eng):
        return (0, eng.P + 1) if eng.pool == "mean" else (0, 1)      # dvpt.py:80-83,205: 'cls' reads row 0 -- the FIRST PROMPT; 'mean' = prompts + cls


class VptSpec(VitSpec):
    """VPT, shallow and deep: [cls | P prompts | patches]."""
    root = "vision_transformer."

    def geometry(self, eng, cfg) -> None:
        eng.lora_layers = frozenset()
        eng.P = cfg.get("num_prompts", 8)
        eng.pd = cfg.get("prompt_dim", 64)
        eng.deep = bool(cfg.get("deep_prompt", True))
        eng.T, eng.row_off = 1 + eng.P + eng.N, 1 + eng.P
        # tokens entering layer i.  Deep VPT rebuilds the sequence before every layer > 0 as [cls | P prompts | x[:, 1+prompt_dim:]]
        # (vpt.py:147-153: the slice uses deep_prompt_embeddings[i].shape[1] == prompt_dim), so it shrinks by prompt_dim - P per layer.
        eng.Ts = [eng.T] * eng.depth
        if eng.deep:
            for i in range(1, eng.depth):
                eng.Ts[i] = eng.Ts[i - 1] - eng.pd + eng.P
            if eng.Ts[-1] <= 1 + eng.pd:
                raise L.GavikoHipError("deep VPT: the shrinking sequence runs out of tokens for this depth / prompt_dim")

    def forward_buffers(self, eng, ws, B, device, train, nsave) -> None:
        R, M, C = (eng.depth if eng.deep else 1) * eng.P, B * eng.T, eng.C
        ws["vproj"] = torch.zeros((R, C), device=device)
        ws["Go"] = ops.act_zeros(M, C, torch.float32, device)      # layer output before the deep-VPT re-pack
        if train:
            ws["dvproj"] = torch.zeros((R, C), device=device)
            ws["dGv"] = ops.act_zeros(M, C, torch.float32, device)

    def owns(self, name: str) -> bool:
        return name in ("prompt_proj.weight", "prompt_proj.bias", "deep_prompt_embeddings", "prompt_embeddings")

    def final_stream(self, eng, ws, train):
        return ws["Go"] if eng.deep else super().final_stream(eng, ws, train)


class EvpSpec(VitSpec):
    """EVP: [cls | patches], a rank-r prompt from the patch embedding and the high-pass filtered volume added before every layer."""
    conv_name = "conv_proj.proj"                 # evp.py:292: a PatchEmbed, not a Sequential

    def geometry(self, eng, cfg) -> None:
        super().geometry(eng, cfg)
        eng.r = eng.C // int(cfg.get("scale_factor", 32))                             # rank of the prompt latents (evp.py:41-42)
        widths = [w_ for w_ in (4, 8, 16, 20, 24, 32) if w_ >= eng.r]
        if not widths or eng.r < 1:
            raise L.GavikoHipError(f"EVP: prompt rank dim/scale_factor = {eng.r} is outside the rank-L kernels' range (1..32)")
        eng.Lp = widths[0]                                                            # latents are zero-padded to this width
        eng.freq = float(cfg.get("freq_nums", 0.25))

    def forward_buffers(self, eng, ws, B, device, train, nsave) -> None:
        BN, Lp, C, mk = B * eng.N, eng.Lp, eng.C, _mk(device)
        z = lambda r, c: ops.act_zeros(r, c, torch.float32, device)
        ws["xc"] = z(BN, C)
        ws["hp"] = torch.zeros_like(ws["img"])
        ws["hcols"] = z(BN, eng.Kp)
        ws["hc"] = z(BN, 64)
        ws["ev"] = dict(e=mk(BN, Lp), s=mk(BN, Lp), pre=[mk(BN, Lp) for _ in range(nsave)], u=[mk(BN, Lp) for _ in range(nsave)],
                        tmp=z(BN, C))
        if train:                                # (its scratch sits here, ahead of the shared backward slots)
            ws["evb"] = dict(du=mk(BN, Lp), dpre=mk(BN, Lp), ds_tmp=mk(BN, Lp), ds=mk(BN, Lp))
            ws["scratch"] = mk(max(ops.outer_scratch_elems(Lp, eng.Kp), 128 * C))
            ws["rscratch"] = mk(32 * (Lp * Lp + Lp + 64))

    def backward_buffers(self, eng, ws, B, device) -> None:
        """Nothing more: scratch / rscratch are sized with the EVP buffers of forward_buffers."""

    def owns(self, name: str) -> bool:
        return "prompt_generator" in name


class AdaptFormerSpec(VitSpec):
    """AdaptFormer: a rank-64 adapter beside every MLP; layers are (attention, adapter, feed-forward) triples."""
    mlp_name = "transformer.layers.%d.2"

    def geometry(self, eng, cfg) -> None:
        super().geometry(eng, cfg)
        eng.adim = 64                                                                 # Adapter(down_dim=64), adaptformer.py:25

    def forward_buffers(self, eng, ws, B, device, train, nsave) -> None:
        M, C = B * eng.T, eng.C
        ws["xa"] = ops.act_zeros(M, C, eng.adt, device)
        ws["ad"] = [dict(mean=torch.zeros(M, device=device), rstd=torch.zeros(M, device=device), h16=ops.act_zeros(M, eng.adim, eng.adt, device))
                    for _ in range(nsave)]
        if train:
            ws["dh16"] = ops.act_zeros(M, eng.adim, eng.adt, device)
            ws["h32"] = torch.zeros((M, eng.adim), device=device)
            ws["dh32"] = torch.zeros((M, eng.adim), device=device)

    def scratch_lat(self, eng) -> int:
        return 64

    def owns(self, name: str) -> bool:
        return "adapter" in name


class MeloSpec(VitSpec):
    """MeLO: LoRA factors on the q and v blocks of the wrapped layers' qkv projection; everything else stays frozen."""
    root = "lora_vit."
    wraps_qkv = True
    backbone_trainable = False

    def geometry(self, eng, cfg) -> None:
        super().geometry(eng, cfg)
        eng.lora_layers = frozenset(cfg.get("lora_layer") or range(eng.depth))
        eng.r, eng.lora_s = int(cfg["r"]), int(cfg["alpha"]) // int(cfg["r"])       # integer alpha // r (melo.py:45-46)

    def forward_buffers(self, eng, ws, B, device, train, nsave) -> None:
        M, C, mk = B * eng.T, eng.C, _mk(device)
        ws["merge32"] = mk(3 * C, C)
        if train:
            ws["dq32"], ws["dv32"] = mk(M, C), mk(M, C)
            ws["lu"] = dict(uq=mk(M, eng.r), uv=mk(M, eng.r), duq=mk(M, eng.r), duv=mk(M, eng.r))

    def scratch_lat(self, eng) -> int:
        return eng.r

    def owns(self, name: str) -> bool:
        return ".linear_a_" in name or ".linear_b_" in name


class SsfSpec(VitSpec):
    """SSF: a scale and a shift after every Linear / LayerNorm, folded into the operands inside the recorded step."""

    def backward_buffers(self, eng, ws, B, device) -> None:
        M = B * eng.T
        ws["ssf_scratch"] = torch.zeros(64 * 2 * max(eng.mlp, 3 * eng.C), device=device)
        ws["ssf_tmp"] = torch.zeros(2 * eng.C, device=device)
        ws["ssf_stat"] = [torch.zeros(M, device=device), torch.zeros(M, device=device)]
        super().backward_buffers(eng, ws, B, device)

    def owns(self, name: str) -> bool:
        return "ssf_scale_" in name or "ssf_shift_" in name


METHOD_SPECS = {"vit": VitSpec(), "gaviko": GavikoSpec(), "dvpt": DvptSpec(), "vpt": VptSpec(), "evp": EvpSpec(),
                "adaptformer": AdaptFormerSpec(), "melo": MeloSpec(), "ssf": SsfSpec()}
