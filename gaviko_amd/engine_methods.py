"""Everything that is a PEFT method's own, one stateless spec per engine kind (METHOD_SPECS).

The static facts: token geometry, feature flags, the method's own workspace slots, which tensors its own gradient kernels cover, the rows
the head pools, and the state_dict name patterns of its reference class (engine_common.Names reads those).
The launches: the sweeps of engine.py are the backbone plus GAViKO's stream choreography; wherever another method does something of its own
they call a hook of `self.method` with the engine as `eng` -- fwd_* in the forward, bwd_* in the backward, in the order of the sweep -- and
the hook enqueues the method's C-ABI launches there.  In the base class (the plain ViT) every hook launches nothing, or the plain form
(patch_embed, embed_rows); a method overrides only where it differs, so what e.g. SSF does in a step reads top to bottom in SsfSpec.
GAViKO's side streams share local state with the sweeps and stay inline there (engine.py, engine_gaviko.py): beside its facts GavikoSpec
launches only what it shares with DVPT, the two ends of the leading prompt rows (_LeadingPrompts.embed_rows / bwd_tail).
Specs hold no state: what a method caches (EvpSpec.state) lives on the engine or in the workspace."""
from __future__ import annotations

import os

import torch

from . import lib as L
from . import ops
from .engine_common import SEED_PROMPT, evp_highpass_operator


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
    folds_in_step = False           # SSF: every GEMM operand is folded inside the recorded step, Engine.refresh_weights has nothing to do
    reads_masked_grad = False       # SSF: its sites read the fp32 dropout-masked gradient (the need32 of Engine._masked_grad)
    ln2_leaves_operand = True       # the LayerNorm-2 backward leaves the bf16 operand copy of dG1; False where a later launch of the block writes it

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

    def cls_row(self, eng) -> int:
        """Row of the cls token: right in front of the patch rows, which start at eng.row_off."""
        return eng.row_off - 1

    def shrinking_rows(self, eng) -> bool:
        """Deep VPT: the sequence shrinks layer by layer while the wgrad operand buffers are shared (Engine._bb_wgrad clears their tails)."""
        return False

    # ---- forward hooks, in the order Engine._forward_impl calls them
    def fwd_begin(self, eng, ws, train) -> None:
        """Before the embedding."""

    def patch_embed(self, eng, ws, B, G0, pos, out1=None) -> None:
        """The patch-embedding GEMM: + bias + pos, scattered to the patch rows of G0 (out1: GAViKO's local stream gets the same rows)."""
        ops.gemm_nt(ws["cols"], eng._w16["conv"], B * eng.N, G0, epilogue=ops.EPI_PATCH_F32, out1=out1, bias=eng._d(eng.names.conv() + ".bias"),
                    pos=pos[1:], rows_in=eng.N, rows_out=eng.T, row_off=eng.row_off)

    def embed_rows(self, eng, G0, cls, pos, B) -> None:
        """The rows every sample shares: the cls token."""
        ops.rows_broadcast(G0, cls, pos[0:1], B, eng.T, self.cls_row(eng), 1, eng.C)

    def fwd_embedded(self, eng, ws, sv, G0, train) -> None:
        """After embedding dropout, before the first layer."""

    def fwd_layer_begin(self, eng, ws, i, si, g, B) -> None:
        """Layer i, before its attention block; g = the layer input."""

    def fwd_after_attn(self, eng, ws, i, si, g1, M, B) -> None:
        """Layer i, after its attention block, before LayerNorm 2; g1 = the mid-layer stream."""

    def fwd_after_mlp(self, eng, ws, i, si, gout, M) -> None:
        """Layer i, after its MLP block wrote gout."""

    def layer_out(self, eng, ws, go):
        """The buffer a layer's MLP block writes."""
        return ws["G"][go]

    def fwd_layer_end(self, eng, ws, sv, i, gout, go, B) -> None:
        """Layer i, after everything else of the layer."""

    # ---- backward hooks, in the order of Engine._backward_head / _backward_segment / _mlp_block_bwd / _attn_block_bwd
    def bwd_head(self, eng, ws, sv, gv, bb, B) -> None:
        """After the head's own gradients, when the sweep goes on into the backbone."""

    def bwd_first_boundary(self, eng, ws, hi):
        """The buffer that holds the boundary gradient entering layer `hi`, the first of a segment."""
        return ws["dG"][0]

    def bwd_linear_site(self, eng, ws, gv, prefix, idx, dy, y0, M, N, y1=None, **kw) -> None:
        """One Linear of the backbone (`prefix`: the block's name, idx: 1 = its first, 2 = its second): dy = the gradient of its output,
        y0 (- y1) = that output."""

    def bwd_ln_site(self, eng, ws, gv, prefix, ln, dy, x, mean, rstd, M) -> None:
        """One LayerNorm of the backbone (`prefix + ln`): dy = the gradient of its output, x / mean / rstd = its input and statistics."""

    def bwd_mlp_begin(self, eng, ws, gv, i, dGout, M, B) -> None:
        """MLP block of layer i, before the fc2 dgrad."""

    def bwd_mlp_end(self, eng, ws, gv, i, dGout, dGin, M, bdrop) -> None:
        """MLP block of layer i, after its LayerNorm backward wrote dGin (bdrop: the backbone's dropout rate)."""

    def bwd_after_attention(self, eng, ws, gv, i, M) -> None:
        """Attention block of layer i, after the attention backward wrote ws['dqkv']."""

    def bwd_layer(self, eng, ws, gv, bb, i, dG, B) -> None:
        """Layer i, after its attention block wrote dG, the gradient of the layer input: what is left of the layer's own gradients."""

    def bwd_layer_boundary(self, eng, ws, sv, i, dG, B):
        """Layer i, after its gradients are final; -> the buffer that holds the boundary gradient for layer i - 1."""
        return dG

    def bwd_embed_dlocal(self, eng, ws, dG, B):
        """A second gradient of the raw patch embedding [B*N][C] for Engine._bb_embed_grads, or None."""
        return None

    def bwd_tail(self, eng, ws, sv, gv, dG, B) -> None:
        """After layer 0 and the embedding's backbone gradients; dG = the gradient of the layer-0 input."""


class _LeadingPrompts:
    """[P prompts | cls | patches] (gaviko.py:536-548, dvpt.py:196-199): the two ends of the prompt rows."""

    def embed_rows(self, eng, G0, cls, pos, B) -> None:
        d = eng._d
        ops.rows_broadcast(G0, d("prompt_embeddings")[0], d("prompt_positional_embedding")[0], B, eng.T, 0, eng.P, eng.C)
        ops.rows_broadcast(G0, cls, pos[0:1], B, eng.T, eng.P, 1, eng.C)

    def bwd_tail(self, eng, ws, sv, gv, dG, B) -> None:
        ops.rows_batch_sum(dG, gv["prompt_embeddings"].view(eng.P, eng.C), gv["prompt_positional_embedding"].view(eng.P, eng.C), B, eng.T, 0,
                           eng.P, eng.C)


class GavikoSpec(_LeadingPrompts, VitSpec):
    """GAViKO: [P prompts | cls | patches], the MWSA local stream and the GPA prompt attention beside every layer."""
    attn_name = "transformer.attns.%d"
    mlp_name = "transformer.mlps.%d"
    head_name = "mlp_head.head"
    supports_prune = True
    ln2_leaves_operand = False      # the GPA scatter behind it adds into dG1 and writes the operand copy

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


class DvptSpec(_LeadingPrompts, VitSpec):
    """DVPT: [P prompts | cls | patches], the prompts re-weighted by a shared rank-20 MLP before every layer."""
    attn_name = "transformer.layers.%d.0.attn"
    mlp_name = "transformer.layers.%d.0.mlp"
    ln2_leaves_operand = False      # bwd_mlp_end adds into dG1 and writes the operand copy

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

    # ---- share_MLP beside the MLP block (dvpt.py:24-63)

    @staticmethod
    def _names(i):
        p = f"transformer.layers.{i}.0.prompt_proj"
        return p + ".prompt_key_proj_d", p + ".prompt_key_proj_u", p + ".prompt_gate"

    def fwd_after_attn(self, eng, ws, i, si, g1, M, B) -> None:
        pd, pu, pg = self._names(i)
        d, v = eng._d, ws["dv"][si]
        ops.skinny_down(x=g1, w=d(pd + ".weight"), bias=d(pd + ".bias"), y=v["z"], M=M, C=eng.C, L=eng.Lat, act=0, w_layout=0, act_in=1)
        ops.dvpt_fwd(z=v["z"], enh=v["enh"], lse=v["lse"], B=B, T=eng.T, P=eng.P, L=eng.Lat, C=eng.C, scale=eng.C ** -0.5)

    def fwd_after_mlp(self, eng, ws, i, si, gout, M) -> None:
        pd, pu, pg = self._names(i)
        d, v = eng._d, ws["dv"][si]
        ops.skinny_up(lat=v["z"], lat_override=v["enh"], w=d(pu + ".weight"), bias=d(pu + ".bias"), alpha_ptr=d(pg), out=gout, M=M, C=eng.C,
                      L=eng.Lat, T=eng.T, P=eng.P, w_layout=0, accumulate=1)

    def bwd_mlp_begin(self, eng, ws, gv, i, dGout, M, B) -> None:
        """dcomb = dGout . W_u;  dW_u, db_u (gate applied afterwards), dgate;  latent backward -> dz;  db_d, dW_d."""
        pd, pu, pg = self._names(i)
        d, v, bw, C, Lt = eng._d, ws["dv"][i], ws["dvb"], eng.C, eng.Lat
        ops.skinny_down(x=dGout, w=d(pu + ".weight"), y=bw["dcomb"], M=M, C=C, L=Lt, act=0, w_layout=1)
        ops.outer_reduce(narrow=v["z"], lat_override=v["enh"], wide=dGout, scratch=ws["scratch"], out=gv[pu + ".weight"], colsum=gv[pu + ".bias"],
                         M=M, C=C, L=Lt, T=eng.T, P=eng.P, transposed=1, accumulate=0)
        ops.dvpt_bwd(z=v["z"], enh=v["enh"], lse=v["lse"], dcomb=bw["dcomb"], gate=d(pg), bu=d(pu + ".bias"), colsum_dy=gv[pu + ".bias"],
                     delta=bw["delta"], dz=bw["dz"], dgate=gv[pg], B=B, T=eng.T, P=eng.P, L=Lt, C=C, scale=C ** -0.5)
        ops.scale_dev_(gv[pu + ".weight"], d(pg))
        ops.scale_dev_(gv[pu + ".bias"], d(pg))
        ops.reduce_batch([(bw["dz"], None, gv[pd + ".bias"], 0)], ws["rscratch"])
        ops.outer_reduce(narrow=bw["dz"], wide=ws["G1"][i], scratch=ws["scratch"], out=gv[pd + ".weight"], M=M, C=C, L=Lt, transposed=0,
                         accumulate=0, wide_act=1)

    def bwd_mlp_end(self, eng, ws, gv, i, dGout, dGin, M, bdrop) -> None:
        """dG1 += (dz . Wd) * QuickGELU'(G1)  (+ operand copy)."""
        pd, pu, pg = self._names(i)
        ops.skinny_up(lat=ws["dvb"]["dz"], w=eng._d(pd + ".weight"), out=dGin, out_bf16=None if eng.fp32 else ws["dG16"], gg_x=ws["G1"][i],
                      M=M, C=eng.C, L=eng.Lat, w_layout=1, accumulate=1)
        if eng.fp32:
            ops.copy_(ws["dG16"], dGin)


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

    def cls_row(self, eng) -> int:
        return 0                                   # [cls | prompts | patches] (vpt.py:127-131)

    def shrinking_rows(self, eng) -> bool:
        return eng.deep

    @staticmethod
    def _prompt_dropout(eng, ws, sv, i, g, T):
        """prompt_dropout on the projected prompts of layer i, rows 1..P of every sample (vpt.py:129,148,152: applied after .expand(B),
        so every sample draws its own mask)."""
        if sv["pdrop"] > 0:
            ops.dropout_rows(g, sv["pdrop"], SEED_PROMPT + i, ws["seed"], out32=g, M=sv["B"] * eng.P, N=eng.C, rows_in=eng.P, rows_out=T, row_off=1)

    def fwd_embedded(self, eng, ws, sv, G0, train) -> None:
        """prompt_proj on every layer's prompts at once (vpt.py:56,127-153); layer 0's go into rows 1..P."""
        d, B, C = eng._d, sv["B"], eng.C
        emb = d("deep_prompt_embeddings" if eng.deep else "prompt_embeddings").reshape(-1, eng.pd)
        ops.small_linear_fwd(emb, d("prompt_proj.weight"), d("prompt_proj.bias"), ws["vproj"], emb.shape[0], eng.pd, C)
        ops.rows_broadcast(G0, ws["vproj"][: eng.P], None, B, eng.T, 1, eng.P, C)
        self._prompt_dropout(eng, ws, sv, 0, G0, eng.Ts[0])

    def layer_out(self, eng, ws, go):
        return ws["Go"] if eng.deep else ws["G"][go]           # deep: the layer output before the re-pack

    def fwd_layer_end(self, eng, ws, sv, i, gout, go, B) -> None:
        if eng.deep and i + 1 < eng.depth:
            ops.vpt_repack_fwd(gout, ws["vproj"][(i + 1) * eng.P: (i + 2) * eng.P], ws["G"][go], B, eng.Ts[i], eng.Ts[i + 1], eng.P, eng.pd, eng.C)
            self._prompt_dropout(eng, ws, sv, i + 1, ws["G"][go], eng.Ts[i + 1])

    def bwd_first_boundary(self, eng, ws, hi):
        return ws["dGv"] if eng.deep and ((eng.depth - 1 - hi) & 1) else ws["dG"][0]      # the un-repack alternates two buffers with the layer parity

    def bwd_layer_boundary(self, eng, ws, sv, i, dG, B):
        P, C, T = eng.P, eng.C, eng.Ts[i]
        if i == 0 or eng.deep:
            # prompt rows 1..P of this layer's input are this layer's projected prompts (vpt.py:127-131,147-153)
            if sv.get("pdrop", 0.0) > 0:                                 # through prompt_dropout: same mask, in place (these rows end here)
                ops.dropout_rows(dG, sv["pdrop"], SEED_PROMPT + i, ws["seed"], out32=dG, M=B * P, N=C, rows_in=P, rows_out=T, row_off=1)
            ops.rows_batch_sum(dG, ws["dvproj"][i * P: (i + 1) * P], None, B, T, 1, P, C)
        if eng.deep and i > 0:
            other = ws["dGv"] if dG is ws["dG"][0] else ws["dG"][0]
            ops.vpt_repack_bwd(dG, other, B, eng.Ts[i - 1], T, P, eng.pd, C)
            dG = other
            ops.to_operand(dG, ws["dG16"], eng.adt)
        return dG

    def bwd_tail(self, eng, ws, sv, gv, dG, B) -> None:
        d = eng._d
        emb_name = "deep_prompt_embeddings" if eng.deep else "prompt_embeddings"
        emb = d(emb_name).reshape(-1, eng.pd)
        ops.small_linear_bwd(emb, d("prompt_proj.weight"), ws["dvproj"], gv["prompt_proj.weight"], gv["prompt_proj.bias"],
                             gv[emb_name].view(-1, eng.pd), emb.shape[0], eng.pd, eng.C)


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

    # ---- prompts from a high-pass copy of the volume + the patch embeddings, added in front of every layer (evp.py)
    def state(self, eng, device):
        """Static per-engine buffers, kept on the engine: the high-pass operator, zero-padded copies of the trainable prompt-generator weights
        and of their gradients (the latents have rank r = dim/32 = 6 / 24 / 32; the rank-L kernels run at the padded width Lp)."""
        st = eng.__dict__.get("_evp")
        if st is not None:
            return st
        C, Lp, Kp = eng.C, eng.Lp, eng.Kp
        mk = _mk(device)
        D, H, W = (g * p_ for g, p_ in zip(eng.grid, eng.patch))
        hp, dm = evp_highpass_operator(D, H, W, eng.freq)
        st = dict(hp=torch.from_numpy(hp).to(device), dmask=torch.from_numpy(dm).to(device),
                  Wp=mk(64, Kp), bp=mk(64), We=mk(Lp, C), be=mk(Lp), Ws=mk(C, Lp),
                  Wi=[mk(Lp, Lp) for _ in range(eng.depth)], WiT=[mk(Lp, Lp) for _ in range(eng.depth)], bi=[mk(Lp) for _ in range(eng.depth)],
                  dWs=mk(C, Lp), dWe=mk(Lp, C), dWp=mk(Lp, Kp), dvec=mk(Lp), dWi=mk(Lp, Lp))
        eng.__dict__["_evp"] = st
        return st

    def patch_embed(self, eng, ws, B, G0, pos, out1=None) -> None:
        """The raw patch embedding is needed on its own (embedding_generator reads it, evp.py:347-348): conv -> xc, tokens = xc + pos; then the
        latents s = proj(highpass(img)) + embedding_generator(conv(img))  (evp.py:76-84, 347-349), at the padded width."""
        d, N, C, Kp, r, Lp, BN = eng._d, eng.N, eng.C, eng.Kp, eng.r, eng.Lp, B * eng.N
        ops.gemm_nt(ws["cols"], eng._w16["conv"], BN, ws["xc"], epilogue=ops.EPI_STORE_F32, bias=d(eng.names.conv() + ".bias"))
        ops.rows_patch(G0, ws["xc"], pos[1:], B, eng.T, N, C, 1, False)
        st, ev = self.state(eng, ws["img"].device), ws["ev"]
        pg = "prompt_generator."
        ops.pad2d(d(pg + "prompt_generator.proj.weight").reshape(r, Kp), r, Kp, st["Wp"], 64, Kp)
        ops.pad2d(d(pg + "prompt_generator.proj.bias"), 1, r, st["bp"], 1, 64)
        ops.pad2d(d(pg + "embedding_generator.weight"), r, C, st["We"], Lp, C)
        ops.pad2d(d(pg + "embedding_generator.bias"), 1, r, st["be"], 1, Lp)
        ops.pad2d(d(pg + "shared_mlp.weight"), C, r, st["Ws"], C, Lp)
        for i in range(eng.depth):
            wi = d(pg + f"lightweight_mlp_{i}.0.weight")
            ops.pad2d(wi, r, r, st["Wi"][i], Lp, Lp)
            ops.pad2d(wi, r, r, st["WiT"][i], Lp, Lp, transpose=True)
            ops.pad2d(d(pg + f"lightweight_mlp_{i}.0.bias"), 1, r, st["bi"][i], 1, Lp)
        ops.skinny_down(x=ws["xc"], w=st["We"], bias=st["be"], y=ev["e"], M=BN, C=C, L=Lp, act=0, w_layout=0)
        ops.evp_highpass(ws["img"], st["hp"], st["dmask"], ws["hp"])
        ops.patchify(ws["hp"], ws["hcols"], eng.patch)
        ops.gemm_nt(ws["hcols"], st["Wp"], BN, ws["hc"], epilogue=ops.EPI_STORE_F32, bias=st["bp"])      # fp32 GEMM in both precisions (1.6 GF)
        ops.add2d(ws["hc"], 64, ev["e"], Lp, ev["s"], Lp, BN, Lp)

    def fwd_layer_begin(self, eng, ws, i, si, g, B) -> None:
        """x[:, 1:] += prompt_i = shared_mlp(GELU(lightweight_mlp_i(s)))  (evp.py:86-95, 235-238)."""
        st, ev = self.state(eng, g.device), ws["ev"]
        Lp, C, BN = eng.Lp, eng.C, B * eng.N
        ops.small_linear_fwd(ev["s"], st["Wi"][i], st["bi"][i], ev["pre"][si], BN, Lp, Lp)
        ops.gelu_fwd(ev["pre"][si], ev["u"][si])
        ops.skinny_up(lat=ev["u"][si], w=st["Ws"], bias=eng._d("prompt_generator.shared_mlp.bias"), out=ev["tmp"], M=BN, C=C, L=Lp, w_layout=0)
        ops.rows_patch(g, ev["tmp"], None, B, eng.T, eng.N, C, 1, True)

    def bwd_layer(self, eng, ws, gv, bb, i, dG, B) -> None:
        """d prompt_i = the patch rows of the gradient of layer i's input; accumulates d shared_mlp over the layers and d s."""
        st, ev, bw = self.state(eng, dG.device), ws["ev"], ws["evb"]
        Lp, C, BN, r = eng.Lp, eng.C, B * eng.N, eng.r
        pg = "prompt_generator."
        top = i == eng.depth - 1
        ops.rows_gather(dG, ev["tmp"], B, eng.T, eng.N, C, 1)
        ops.outer_reduce(narrow=ev["u"][i], wide=ev["tmp"], scratch=ws["scratch"], out=st["dWs"], colsum=gv[pg + "shared_mlp.bias"], M=BN, C=C, L=Lp,
                         transposed=1, accumulate=0 if top else 1)
        ops.skinny_down(x=ev["tmp"], w=st["Ws"], y=bw["du"], M=BN, C=C, L=Lp, act=0, w_layout=1)
        ops.gelu_bwd(bw["du"], ev["pre"][i], bw["dpre"])
        ops.reduce_batch([(bw["dpre"], ev["s"], st["dWi"], 0), (bw["dpre"], None, st["dvec"], 0)], ws["rscratch"])
        ops.pad2d(st["dWi"], r, r, gv[pg + f"lightweight_mlp_{i}.0.weight"], r, r, ld_src=Lp)
        ops.pad2d(st["dvec"], 1, r, gv[pg + f"lightweight_mlp_{i}.0.bias"], 1, r, ld_src=Lp)
        ops.small_linear_fwd(bw["dpre"], st["WiT"][i], None, bw["ds"] if top else bw["ds_tmp"], BN, Lp, Lp)       # d s = dpre . W_i
        if not top:
            ops.add2d(bw["ds"], Lp, bw["ds_tmp"], Lp, bw["ds"], Lp, BN, Lp)

    def bwd_embed_dlocal(self, eng, ws, dG, B):
        """The raw conv output also feeds embedding_generator (evp.py:347-348): d xc += d s . W_e  (d s is complete once layer 0 is through).
        It reaches the conv tensors but not pos_embedding."""
        dlocal = ws["ev"]["tmp"]
        ops.skinny_up(lat=ws["evb"]["ds"], w=self.state(eng, dG.device)["We"], out=dlocal, M=B * eng.N, C=eng.C, L=eng.Lp, w_layout=1, accumulate=0)
        return dlocal

    def bwd_tail(self, eng, ws, sv, gv, dG, B) -> None:
        st, bw = self.state(eng, ws["img"].device), ws["evb"]
        Lp, C, BN, r, Kp = eng.Lp, eng.C, B * eng.N, eng.r, eng.Kp
        pg = "prompt_generator."
        ops.pad2d(st["dWs"], C, r, gv[pg + "shared_mlp.weight"], C, r, ld_src=Lp)
        ops.outer_reduce(narrow=bw["ds"], wide=ws["xc"], scratch=ws["scratch"], out=st["dWe"], M=BN, C=C, L=Lp, transposed=0, accumulate=0)
        ops.pad2d(st["dWe"], r, C, gv[pg + "embedding_generator.weight"], r, C)
        ops.reduce_batch([(bw["ds"], None, st["dvec"], 0)], ws["rscratch"])
        ops.pad2d(st["dvec"], 1, r, gv[pg + "embedding_generator.bias"], 1, r, ld_src=Lp)
        ops.pad2d(st["dvec"], 1, r, gv[pg + "prompt_generator.proj.bias"], 1, r, ld_src=Lp)
        ops.outer_reduce(narrow=bw["ds"], wide=ws["hcols"], scratch=ws["scratch"], out=st["dWp"], M=BN, C=Kp, L=Lp, transposed=0, accumulate=0)
        ops.pad2d(st["dWp"], r, Kp, gv[pg + "prompt_generator.proj.weight"].view(r, Kp), r, Kp)


class AdaptFormerSpec(VitSpec):
    """AdaptFormer: a rank-64 adapter beside every MLP; layers are (attention, adapter, feed-forward) triples."""
    mlp_name = "transformer.layers.%d.2"
    ln2_leaves_operand = False      # bwd_mlp_end adds LN_a'(...) into dG1 and writes the operand copy

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

    # ---- r = up(ReLU(down(LN_a(x)))), x_out = ff(x) + x + r  (adaptformer.py:58-78, 93-97)

    @staticmethod
    def _prefix(i):
        return f"transformer.layers.{i}.1"

    def fwd_embedded(self, eng, ws, sv, G0, train) -> None:
        """bf16 MFMA operands of the TRAINABLE adapter weights, refreshed in place every step (inside the captured graph)."""
        w = eng._w16
        for i in range(eng.depth):
            p = self._prefix(i)
            wd, wu = eng._d(p + ".down_adapter_proj.weight"), eng._d(p + ".up_adapter_proj.weight")
            w[f"ad_d{i}"] = ops.to_operand(wd, None if eng.fp32 else w.get(f"ad_d{i}"), eng.adt)
            w[f"ad_u{i}"] = ops.to_operand(wu, None if eng.fp32 else w.get(f"ad_u{i}"), eng.adt)
            if train:
                w[f"ad_dT{i}"] = ops.transpose_operand(wd, w.get(f"ad_dT{i}"), eng.adt)
                w[f"ad_uT{i}"] = ops.transpose_operand(wu, w.get(f"ad_uT{i}"), eng.adt)

    def fwd_after_attn(self, eng, ws, i, si, g1, M, B) -> None:
        p, d, ad = self._prefix(i), eng._d, ws["ad"][si]
        ops.layernorm_fwd(g1, d(p + ".adapter_layer_norm_before.weight"), d(p + ".adapter_layer_norm_before.bias"), M, eng.C, y16=ws["xa"],
                          mean=ad["mean"], rstd=ad["rstd"])
        eng._gemm(ws["xa"], eng._w16[f"ad_d{i}"], M, ad["h16"], epilogue=ops.EPI_BIAS_RELU_BF16, bias=d(p + ".down_adapter_proj.bias"))

    def fwd_after_mlp(self, eng, ws, i, si, gout, M) -> None:
        p = self._prefix(i)
        eng._gemm(ws["ad"][si]["h16"], eng._w16[f"ad_u{i}"], M, gout, epilogue=ops.EPI_BIAS_RES_F32, bias=eng._d(p + ".up_adapter_proj.bias"),
                  res=gout)

    def bwd_mlp_end(self, eng, ws, gv, i, dGout, dG1, M, bdrop) -> None:
        p, d, C, A = self._prefix(i), eng._d, eng.C, eng.adim
        ad, w, sc = ws["ad"][i], eng._w16, ws["scratch"]
        g, b = d(p + ".adapter_layer_norm_before.weight"), d(p + ".adapter_layer_norm_before.bias")
        if bdrop > 0:
            # backbone dropout live (freeze_vit=False): the operand buffer holds dGout * mask(fc2's dropout) for the FFN branch; the adapter
            # branch joins the stream unmasked (adaptformer.py:96-98: x = ff(x) + x + adapter(x)), so it needs the plain gradient again
            ops.to_operand(dGout, ws["dG16"], eng.adt)
        # up-projection: dh = (dGout . Wu) * [h > 0]; dWu = dGout^T . h; dbu = colsum(dGout)
        eng._gemm(ws["dG16"], w[f"ad_uT{i}"], M, ws["dh16"], epilogue=ops.EPI_RELU_BWD_BF16, aux=ad["h16"])
        ops.cast_bf16_f32_strided(ad["h16"], ws["h32"], M, A, A)
        ops.cast_bf16_f32_strided(ws["dh16"], ws["dh32"], M, A, A)
        ops.outer_reduce(narrow=ws["h32"], wide=dGout, scratch=sc, out=gv[p + ".up_adapter_proj.weight"], colsum=gv[p + ".up_adapter_proj.bias"],
                         M=M, C=C, L=A, transposed=1, accumulate=0)
        # down-projection: dxa = dh . Wd; dWd = dh^T . LN_a(G1); dbd = colsum(dh)
        eng._gemm(ws["dh16"], w[f"ad_dT{i}"], M, ws["dx32"], epilogue=ops.EPI_STORE_F32)
        ops.outer_reduce(narrow=ws["dh32"], wide=ws["G1"][i], mean=ad["mean"], rstd=ad["rstd"], ln_gamma=g, ln_beta=b, scratch=sc,
                         out=gv[p + ".down_adapter_proj.weight"], M=M, C=C, L=A, transposed=0, accumulate=0)
        ops.colsum(ws["dh32"], gv[p + ".down_adapter_proj.bias"], sc, M, A)
        # trainable LayerNorm in front of the adapter: input gradient accumulates into dG1 (+ the operand copy), affine gradients
        ops.layernorm_bwd(ws["dx32"], ws["G1"][i], ad["mean"], ad["rstd"], g, M, C, dx=dG1, dres=dG1, dx16=ws["dG16"])
        ops.layernorm_bwd_affine(ws["dx32"], ws["G1"][i], ad["mean"], ad["rstd"], gv[p + ".adapter_layer_norm_before.weight"],
                                 gv[p + ".adapter_layer_norm_before.bias"], sc, M, C)


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

    # ---- qkv = W x + s B_q A_q x (q columns) + s B_v A_v x (v columns)  (melo.py:41-47)
    @staticmethod
    def _names(eng, i):
        q = eng.names.attn(i) + ".to_qkv"
        return q + ".linear_a_q.weight", q + ".linear_b_q.weight", q + ".linear_a_v.weight", q + ".linear_b_v.weight"

    def fwd_embedded(self, eng, ws, sv, G0, train) -> None:
        """Fold the rank-r update into the bf16 QKV operand (and its transpose) every step: the forward is then the plain GEMM."""
        w, C = eng._w16, eng.C
        for i in range(eng.depth):
            if i not in eng.lora_layers:                    # a layer outside lora_layer (melo.py:67-68) keeps the plain frozen shadows
                continue                                    # refresh_weights() built for it
            aq, bq, av, bv = (eng._d(n) for n in self._names(eng, i))
            ops.lora_merge(eng._d(eng.names.qkv_weight(i)), aq, bq, av, bv, ws["merge32"], C, eng.r, eng.lora_s)
            if eng.fp32 and not isinstance(w.get(f"qkv{i}_own"), torch.Tensor):
                w[f"qkv{i}_own"] = torch.empty_like(ws["merge32"])     # the merged weight needs its own buffer per layer
            w[f"qkv{i}"] = ops.to_operand(ws["merge32"], w[f"qkv{i}_own"] if eng.fp32 else w.get(f"qkv{i}"), eng.adt)
            if train:
                w[f"qkv{i}_t"] = ops.transpose_operand(ws["merge32"], w.get(f"qkv{i}_t"), eng.adt)

    def bwd_after_attention(self, eng, ws, gv, i, M) -> None:
        """dB = s dq^T u, dA = s (dq B)^T LN(x), u = LN(x) A^T -- all rank-r fp32 kernels over the bf16 dq / dv blocks."""
        if i not in eng.lora_layers:
            return
        C, r, d, sc = eng.C, eng.r, eng._d, ws["scratch"]
        na_q, nb_q, na_v, nb_v = self._names(eng, i)
        a = eng.names.attn(i)
        g1, b1, st, x = d(a + ".norm.weight"), d(a + ".norm.bias"), ws["stat"][i], ws["G"][i]
        lu = ws["lu"]
        ops.cast_bf16_f32_strided(ws["dqkv"], ws["dq32"], M, C, 3 * C, col0=0)
        ops.cast_bf16_f32_strided(ws["dqkv"], ws["dv32"], M, C, 3 * C, col0=2 * C)
        for na, nb, dblk, u, du in ((na_q, nb_q, ws["dq32"], lu["uq"], lu["duq"]), (na_v, nb_v, ws["dv32"], lu["uv"], lu["duv"])):
            ops.skinny_down(x=x, w=d(na), ln_gamma=g1, ln_beta=b1, y=u, M=M, C=C, L=r, act=0, w_layout=0, eps=1e-5)
            ops.outer_reduce(narrow=u, wide=dblk, scratch=sc, out=gv[nb], M=M, C=C, L=r, transposed=1, accumulate=0)
            ops.skinny_down(x=dblk, w=d(nb), y=du, M=M, C=C, L=r, act=0, w_layout=1)
            ops.outer_reduce(narrow=du, wide=x, mean=st[0], rstd=st[1], ln_gamma=g1, ln_beta=b1, scratch=sc, out=gv[na], M=M, C=C, L=r,
                             transposed=0, accumulate=0)
            if eng.lora_s != 1:
                ops.scale_(gv[na], float(eng.lora_s))
                ops.scale_(gv[nb], float(eng.lora_s))


class SsfSpec(VitSpec):
    """SSF: a scale and a shift after every Linear / LayerNorm, folded into the operands inside the recorded step."""
    folds_in_step = True
    reads_masked_grad = True

    def backward_buffers(self, eng, ws, B, device) -> None:
        M = B * eng.T
        ws["ssf_scratch"] = torch.zeros(64 * 2 * max(eng.mlp, 3 * eng.C), device=device)
        ws["ssf_tmp"] = torch.zeros(2 * eng.C, device=device)
        ws["ssf_stat"] = [torch.zeros(M, device=device), torch.zeros(M, device=device)]
        super().backward_buffers(eng, ws, B, device)

    def owns(self, name: str) -> bool:
        return "ssf_scale_" in name or "ssf_shift_" in name

    # ---- effective parameters per step, scale / shift gradients per site (ssf.py)

    @staticmethod
    def _sites(eng):
        """(scale name, shift name, kind, target) for every ssf_ada of the model, in forward order: the patch embedding, six per layer, the
        final norm."""
        nm = eng.names
        sites = [("ssf_scale_1", "ssf_shift_1", "linear", ("conv", "conv_proj.0.weight", "conv_proj.0.bias"))]
        for i in range(eng.depth):
            a, m = nm.attn(i), nm.mlp(i)
            sites += [(a + ".ssf_scale_0", a + ".ssf_shift_0", "ln", (a + ".norm.weight", a + ".norm.bias")),
                      (a + ".ssf_scale_1", a + ".ssf_shift_1", "linear", (f"qkv{i}", a + ".to_qkv.weight", a + ".to_qkv.bias")),
                      (a + ".ssf_scale_2", a + ".ssf_shift_2", "linear", (f"out{i}", a + ".to_out.0.weight", a + ".to_out.0.bias")),
                      (m + ".ssf_scale_0", m + ".ssf_shift_0", "ln", (m + ".net.0.weight", m + ".net.0.bias")),
                      (m + ".ssf_scale_1", m + ".ssf_shift_1", "linear", (f"fc1{i}", m + ".net.1.weight", m + ".net.1.bias")),
                      (m + ".ssf_scale_2", m + ".ssf_shift_2", "linear", (f"fc2{i}", m + ".net.4.weight", m + ".net.4.bias"))]
        sites.append(("transformer.ssf_scale_1", "transformer.ssf_shift_1", "ln", ("transformer.norm.weight", "transformer.norm.bias")))
        return sites

    def fwd_begin(self, eng, ws, train) -> None:
        """gamma' = gamma*s, beta' = beta*s + t;  W' = s[:,None]*W (operand dtype, + transpose for the dgrad), b' = b*s + t.
        Runs inside the recorded step: the scales and shifts are what the optimiser updates."""
        w, eff, raw = eng._w16, eng._eff, (lambda n: eng.p[n].detach())
        for sn, tn, kind, tgt in self._sites(eng):
            s_, t_ = raw(sn), raw(tn)
            if kind == "ln":
                gname, bname = tgt
                if gname not in eff:
                    eff[gname], eff[bname] = torch.empty_like(s_), torch.empty_like(s_)
                ops.ssf_fold_vec(raw(gname), s_, None, eff[gname])
                ops.ssf_fold_vec(raw(bname), s_, t_, eff[bname])
            else:
                key, wname, bname = tgt
                W = raw(wname)
                W2 = W.reshape(W.shape[0], -1)
                if key not in w:
                    w[key] = torch.empty(W2.shape, dtype=eng.adt, device=W.device)
                    eff[bname] = torch.empty_like(s_)
                need_t = train and key != "conv"
                if need_t and key + "_t" not in w:
                    w[key + "_t"] = torch.empty((W2.shape[1], W2.shape[0]), dtype=eng.adt, device=W.device)
                ops.ssf_fold_weight(W2, s_, w[key], w[key + "_t"] if need_t else None)
                ops.ssf_fold_vec(eng.p[bname].detach() if bname in eng.p else None, s_, t_, eff[bname])

    @staticmethod
    def _unfold(eng, gv, bb, sites):
        """ScalingShiftingFeatures(freeze_vit=False): the backbone-gradient hooks see the EFFECTIVE tensors (W' = s o W, b' = b o s + t,
        gamma' = gamma o s, beta' = beta o s + t), so what they left in gv is dW', db', dgamma', dbeta'; the chain rule to the raw
        tensors is one multiplication by the site's scale (in place)."""
        if not bb:
            return
        for sn, tn, kind, tgt in sites:
            s_ = eng.p[sn].detach()
            if kind == "ln":
                for n in tgt:
                    if n in bb:
                        ops.ssf_fold_vec(gv[n], s_, None, gv[n])
            else:
                _, wname, bname = tgt
                if wname in bb:
                    ops.ssf_fold_weight(gv[wname], s_, gv[wname], None)
                if bname in bb:
                    ops.ssf_fold_vec(gv[bname], s_, None, gv[bname])

    def bwd_head(self, eng, ws, sv, gv, bb, B) -> None:
        """final norm + ssf (ssf.py:138): statistics of the final stream, then the pooled rows' scale / shift gradients."""
        C, T, raw = eng.C, eng.T, (lambda n: eng.p[n].detach())
        r0, R = eng._pool_rows()
        g, st = eng._final_stream(ws, True), ws["ssf_stat"]
        ops.layernorm_fwd(g, raw("transformer.norm.weight"), raw("transformer.norm.bias"), B * T, C, y16=ws["xn"], mean=st[0], rstd=st[1])
        ops.ssf_head_grad(g, st[0], st[1], eng._d(eng.names.head() + ".weight"), ws["dlogits"], raw("transformer.norm.weight"),
                          raw("transformer.norm.bias"), gv["transformer.ssf_scale_1"], gv["transformer.ssf_shift_1"], B, T, C, eng.K, r0, R)
        self._unfold(eng, gv, bb, self._sites(eng)[-1:])                              # the final norm's affine

    def bwd_linear_site(self, eng, ws, gv, prefix, idx, dy, y0, M, N, y1=None, **kw) -> None:
        sn, tn = f"{prefix}.ssf_scale_{idx}", f"{prefix}.ssf_shift_{idx}"
        ops.ssf_colgrad(dy, y0, eng.p[sn].detach(), eng.p[tn].detach(), gv[sn], gv[tn], ws["ssf_scratch"], M, N, y1=y1, **kw)

    def bwd_ln_site(self, eng, ws, gv, prefix, ln, dy, x, mean, rstd, M) -> None:
        C, tmp = eng.C, ws["ssf_tmp"]
        ops.layernorm_bwd_affine(dy, x, mean, rstd, tmp[:C], tmp[C:], ws["scratch"], M, C)
        ops.ssf_ln_grad(tmp[:C], tmp[C:], eng.p[prefix + ln + ".weight"].detach(), eng.p[prefix + ln + ".bias"].detach(),
                        gv[prefix + ".ssf_scale_0"], gv[prefix + ".ssf_shift_0"])

    def bwd_layer(self, eng, ws, gv, bb, i, dG, B) -> None:
        self._unfold(eng, gv, bb, self._sites(eng)[1 + 6 * i: 7 + 6 * i])             # this layer's six sites, before its bucket is final

    def bwd_tail(self, eng, ws, sv, gv, dG, B) -> None:
        """patch embedding + ssf (ssf.py:229-232): dy = the patch rows of the input gradient, y = G[0] patch rows - pos[1:]."""
        pos = eng.p["pos_embedding"].detach()[0]
        ops.ssf_colgrad(dG, ws["G"][0], eng.p["ssf_scale_1"].detach(), eng.p["ssf_shift_1"].detach(), gv["ssf_scale_1"], gv["ssf_shift_1"],
                        ws["ssf_scratch"], B * eng.N, eng.C, pos=pos[1:], rows_in=eng.N, rows_out=eng.T, row_off=1,
                        y_mul=1.0 - sv.get("edrop", 0.0))              # (dG is already masked by emb_dropout when that is live)
        self._unfold(eng, gv, sv.get("bb") or (), self._sites(eng)[:1])               # the patch embedding's conv tensors


METHOD_SPECS = {"vit": VitSpec(), "gaviko": GavikoSpec(), "dvpt": DvptSpec(), "vpt": VptSpec(), "evp": EvpSpec(),
                "adaptformer": AdaptFormerSpec(), "melo": MeloSpec(), "ssf": SsfSpec()}
