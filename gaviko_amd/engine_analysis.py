"""Analysis half of the launch-plan engine: the entry points of gaviko_amd.explain / uncertainty / features (attention, feature, perturbed and
member forwards, the input-only backward with its attention-relevance launches) and the hooks the sweep calls for them (_feat_pool, _relv_layer,
_ig_buffers, _ig_scratch_views, _input_grad_tail).  Mixed into engine.Engine; every method only enqueues C-ABI launches.  Every public entry
point runs under _undisturbed(), so a call between a training forward and its backward leaves that backward's gradients bit-identical."""
from __future__ import annotations

from contextlib import contextmanager
from typing import Dict, List, Optional

import torch

from . import lib as L
from . import ops
from .engine_common import SEED_EMB, flat_views

# what a pending backward reads besides its workspace: the saved activations and the per-step decisions of forward()
_PENDING = ("_ws", "_saved", "_saved_key", "_keep_inputs", "_pre_is_grad", "_fold_on", "_last_run", "_fwd_gen")


class AnalysisPaths:
    @contextmanager
    def _undisturbed(self):
        """Puts the state of a pending backward (_PENDING, each if present) back on the way out, whether the body returns or raises."""
        keep = {k: getattr(self, k) for k in _PENDING if hasattr(self, k)}
        try:
            yield
        finally:
            for k, v in keep.items():
                setattr(self, k, v)

    # ------------------------------------------------------------------ inference forwards
    def attention_forward(self, img: torch.Tensor):
        """The deterministic inference forward (no dropout) in a workspace of its own that keeps every layer's qkv / lse -> (logits, ws)."""
        with self._undisturbed():
            logits = self.forward(img, train=False, drop=None, keep_attn=True)
            return logits, self._ws

    def eval_forward(self, img: torch.Tensor) -> torch.Tensor:
        """A deterministic inference forward (no dropout) that leaves the state of a pending backward as it was."""
        with self._undisturbed():
            return self.forward(img, train=False, drop=None)

    def feature_forward(self, img: torch.Tensor, layers: Optional[tuple] = None):
        """The deterministic inference forward (no dropout) that also hands out the representation, for gaviko_amd.features.
        layers=None: eval_forward's own recorded plan and workspace -> (logits, pooled); pooled [B, C] is a clone of the vector the head's
        nn.Linear consumes (the mean over _pool_rows() of the final LayerNorm).
        layers = a sorted tuple of indices in 0..depth (l: the global token stream entering layer l; depth: the output of the last layer,
        before transformer.norm): a workspace and a plan of their own, in which two gvk_token_pool launches per requested layer run on the
        main stream while that layer's stream is still live -> (logits, pooled, cls, patch_mean), the last two [len(layers), B, C]:
        cls[j] = row r_cls (0 for VPT's [cls | prompts | patches], else row_off - 1), patch_mean[j] = the mean over the rows
        row_off .. Ts[l] - 1 of that layer's own sequence (deep VPT's shrinks).  The launches write fixed workspace slots, so they are
        recorded and replay.  With `depth` requested the last layer's MLP computes every row in this plan (dead-row pruning would leave the
        patch rows unwritten); the logits are bit-identical either way.  GAViKO's local stream is not summarised.  The state of a
        pending backward is put back, as for eval_forward."""
        if layers is not None:
            try:
                layers = tuple(int(l) for l in layers)
            except (TypeError, ValueError):
                raise L.GavikoHipError(f"feature_forward: layers={layers!r}: expected None or a sorted tuple of ints") from None
            if not layers or any(not 0 <= l <= self.depth for l in layers) or any(a >= b for a, b in zip(layers, layers[1:])):
                raise L.GavikoHipError(f"feature_forward: layers={layers!r}: expected strictly increasing indices within [0, {self.depth}] "
                                       f"(l: the stream entering layer l; {self.depth}: the output of the last layer)")
        with self._undisturbed():
            logits = self.forward(img, train=False, drop=None, feat=layers)
            ws = self._ws
            if layers is None:
                return logits, ws["pooled"].clone()
            return logits, ws["pooled"].clone(), ws["feat_cls"].clone(), ws["feat_patch"].clone()

    def _feat_pool(self, ws, sv, l, g, T):
        """feature_forward: the CLS row and the patch-row mean of the stream g [B][T][C] entering layer l (l = depth: the last output)."""
        if l in sv["feat"]:
            j = sv["feat"].index(l)
            r_cls = self.method.cls_row(self)
            ops.token_pool(g, sv["B"], T, self.C, r_cls, 1, out=ws["feat_cls"][j])
            ops.token_pool(g, sv["B"], T, self.C, self.row_off, T - self.row_off, out=ws["feat_patch"][j])

    # ------------------------------------------------------------------ chunks of a sweep (perturbation, members)
    def _chunk_forward(self, Bc, device, build, drop, gather_src, slot, rows) -> torch.Tensor:
        """One chunk of a sweep: `build(ws)` launches the Bc inputs into the static input slot of the (Bc, inference) workspace, the recorded
        inference forward of `drop` runs on them -> logits [Bc, K], and with `rows` the logits row of sample o is also written to
        rows.view(-1, K)[slot[o]] (slot[o] < 0: nowhere).  The build and gather launches are issued eagerly on the forward's stream: their
        arguments are slices of the sweep's device tables, which a recorded plan would freeze."""
        with self._undisturbed():
            ws = self.workspace(Bc, device, False)
            build(ws)
            logits = self.forward(ws["img"], train=False, drop=drop)
            if rows is not None:
                ops.perturb_scores(ws["logits"], gather_src, None, slot, None, None, rows)
        return logits

    def perturbed_forward(self, x: torch.Tensor, src: torch.Tensor, *, rank=None, lo=None, hi=None, boxes=None, fill_scalar=None, base=None,
                          slot=None, rows=None) -> torch.Tensor:
        """One chunk of a perturbation sweep, for gaviko_amd.explain: Bc = len(src) perturbed copies of the volumes x [S,1,D,H,W] are built
        straight in the static input slot of the (Bc, inference) workspace -- output sample o is x[src[o]] with the patches of its mask
        replaced by fill_scalar[src[o]] or by the baseline volume `base` -- and eval_forward's deterministic forward runs on them -> logits
        [Bc, K].  The mask is a rank interval (rank i32 [S, N], lo / hi i32 [Bc]: lo <= rank < hi) or a box per sample (boxes i32 [Bc, 6],
        patch-grid units).  slot / rows: the logits row of sample o is also written to rows.view(-1, K)[slot[o]] (slot[o] < 0: nowhere).
        Every table is a device tensor, so a sweep uploads them once and no step waits for the host.  The forward is the recorded plan of
        eval_forward at this batch size (one workspace, one plan key for a whole sweep); the mask, perturb and gather launches around it
        are issued eagerly (_chunk_forward).  The state of a pending backward is put back, as for eval_forward."""
        if (boxes is None) == (rank is None):
            raise L.GavikoHipError("perturbed_forward: exactly one of rank (with lo, hi) and boxes")
        if (slot is None) != (rows is None):
            raise L.GavikoHipError("perturbed_forward: slot and rows go together")
        Bc = src.numel()

        def build(ws):
            mask = ws.get("pmask")
            if mask is None:
                mask = ws["pmask"] = torch.zeros((Bc, self.N), dtype=torch.uint8, device=x.device)
            if boxes is not None:
                ops.patch_mask_box(boxes, mask, self.grid)
            else:
                ops.patch_mask_rank(rank, src, lo, hi, mask)
            ops.perturb_volume(x, mask, src, ws["img"], self.patch, fill_scalar=fill_scalar, base=base)

        return self._chunk_forward(Bc, x.device, build, None, src, slot, rows)

    def member_seed(self, Bc: int, device, seed: Optional[int] = None) -> torch.Tensor:
        """The dropout seed word (one int64 device word) of the (Bc, inference) workspace that member_forward runs in; seed: set it first
        (one fill_), so that the draws of a sweep are reproducible.  Every forward advances the word by 7919 and draws its masks from the
        advanced value.  The state of a pending backward is put back."""
        with self._undisturbed():
            word = self.workspace(Bc, device, False)["seed"]
        if seed is not None:
            word.fill_(int(seed))
        return word

    def member_forward(self, x: torch.Tensor, src: torch.Tensor, flip: torch.Tensor, drop: Optional[dict], *, slot=None, rows=None) -> torch.Tensor:
        """One chunk of a member sweep, for gaviko_amd.uncertainty: Bc = len(src) members of the volumes x [S,1,D,H,W] are built straight in
        the static input slot of the (Bc, inference) workspace -- member o is x[src[o]] mirrored along the axes in the bits of flip[o] (0: a
        plain replica) -- and an inference forward runs on them -> logits [Bc, K].  drop=None: eval_forward's deterministic plan; a dict with
        live rates: the recorded plan of that drop configuration, the masks drawn from the workspace's seed word (member_seed) by the row
        index inside the chunk.  slot / rows: the logits row of member o is also written to rows.view(-1, K)[slot[o]] (slot[o] < 0:
        nowhere).  src / flip / slot are device tensors, so a sweep uploads them once and no step waits for the host; the build and gather
        launches are issued eagerly around the replayed forward (_chunk_forward; the gather takes the rows in chunk order: no src table).
        The state of a pending backward is put back, as for eval_forward."""
        if (slot is None) != (rows is None):
            raise L.GavikoHipError("member_forward: slot and rows go together")
        return self._chunk_forward(src.numel(), x.device, lambda ws: ops.tta_volumes(x, src, flip, ws["img"]), drop, None, slot, rows)

    # ------------------------------------------------------------------ input-only backward (gaviko_amd.explain)
    def _input_only_backward(self, img, seed, relv=None):
        """A deterministic training forward (no dropout) and an input-only backward from seed(logits), both in the 'igrad' workspace ->
        (logits, ws, rv).  relv = (mode, rows, keep_dctx): the sweep also feeds the relevance buffers rv (self._relv, set around the backward
        only and cleared whether seed, the backward or neither raises)."""
        with self._undisturbed():
            logits = self.forward(img, train=True, drop=None, ws_tag="igrad")
            ws = self._ws
            rv = None if relv is None else self._relv_buffers(ws, *relv, img.device)
            self._relv = rv
            try:
                self.backward(seed(logits), input_grad="only")
            finally:
                self._relv = None
        return logits, ws, rv

    def input_backward(self, img: torch.Tensor, seed):
        """Gradient of the logits with respect to the input volume, for gaviko_amd.explain: a deterministic training forward (no dropout)
        and an input-only backward, both in the 'igrad' workspace -> (logits, ws).  `seed(logits)` returns dlogits [B, K] (the logit
        gradient to start from).  ws['ig']['dcols'] holds the gradient in the patch-embedding's im2col layout, ws['dimg'] the volume.  No
        parameter gradient is written (the sweep writes into a scratch buffer of its own) and the state of a pending backward is put back."""
        return self._input_only_backward(img, seed)[:2]

    def relevance_backward(self, img: torch.Tensor, seed, mode: str = "relevance", rows="pool", keep_dctx: bool = False):
        """Gradient x attention of every global self-attention layer, for gaviko_amd.explain: input_backward's deterministic forward and
        input-only sweep in the 'igrad' workspace, and after the out-projection dgrad of layer i has written ws['dctx'] (= dO of that
        layer) one gvk_attention_gradcolsum_bf16 on ws['qkv'][i], ws['lse'][i] and ws['dctx'] -> (logits, ws, rv).  No [T, T] matrix and no
        per-layer copy of dO exists; the launches are part of the sweep's plan (a plan key of its own).
          mode='relevance': rv['r'] [B, T] = w_pool propagated from the last layer to the first, r <- r + (1 / H) sum_h r^T max(0, P o dP)
                            (the order the sweep visits the layers); rv['added'] = r - w_pool, accumulated on its own.  The first step reads the pooled rows only: with dead-row pruning
                            the other rows of the top layer's dctx are not written.
          mode='maps':      rv['maps'][i] [B, H, T_i] = sum_r w_r max(0, P o dP)[r, :], w uniform over `rows` ('pool' or one row index).
        keep_dctx (tests on tiny models): rv['keep'][i] is a copy of layer i's dctx.
        No parameter gradient is written and the state of a pending backward is put back, as for input_backward."""
        if self.fp32:
            raise L.GavikoHipError("relevance_backward is built for the bf16 path (the exact-fp32 path keeps no bf16 qkv / dctx)")
        if mode not in ("relevance", "maps"):
            raise L.GavikoHipError(f"mode={mode!r}: expected 'relevance' or 'maps'")
        if mode == "relevance" and len(set(self.Ts)) != 1:
            raise L.GavikoHipError("the attention relevance needs one token sequence through all layers (deep VPT rebuilds it before every layer)")
        return self._input_only_backward(img, seed, (mode, rows, bool(keep_dctx)))

    def _relv_buffers(self, ws, mode, rows, keep_dctx, device) -> dict:
        """The relevance buffers of one (mode, rows, keep_dctx), in the workspace: a recorded plan keeps their addresses."""
        key = (mode, rows, keep_dctx)
        rv = ws.setdefault("relv", {}).get(key)
        if rv is not None:
            return rv
        B, H, L_ = ws["B"], self.heads, self.depth
        r0, R = self._pool_rows()
        rng = [((0, self.Ts[i]) if (self.pool == "mean" and self.kind not in ("gaviko", "dvpt")) else (r0, r0 + R)) if rows == "pool"
               else (rows, rows + 1) for i in range(L_)]
        rv = dict(key=key, mode=mode, rows=rng, keep=[torch.zeros_like(ws["dctx"]) for _ in range(L_)] if keep_dctx else None,
                  allrows=rows != "pool")
        def uniform(q0, q1, T):
            w = torch.zeros((B, T), device=device)
            w[:, q0:q1] = 1.0 / (q1 - q0)
            return w
        if mode == "relevance":
            rv["w0"] = uniform(*rng[-1], self.T)
            rv["r"] = torch.zeros((B, self.T), device=device)
            rv["added"] = torch.zeros((B, self.T), device=device)        # r - w_pool, accumulated on its own
            rv["cs"] = torch.zeros((B, H, self.T), device=device)
        else:
            rv["w"] = [uniform(*rng[i], self.Ts[i]) for i in range(L_)]
            rv["maps"] = [torch.zeros((B, H, self.Ts[i]), device=device) for i in range(L_)]
        ws["relv"][key] = rv
        return rv

    def _relv_layer(self, ws, i, B, T):
        """Main stream, right after the out-projection dgrad of layer i: ws['dctx'] holds dO of this layer."""
        rv, H = self._relv, self.heads
        if rv["keep"] is not None:
            ops.copy_(rv["keep"][i], ws["dctx"])
        if rv["mode"] == "relevance":
            q0, q1 = 0, T
            if i == self.depth - 1:                         # r = w_pool: zero outside the pooled rows, which are all the first step reads
                ops.copy_(rv["r"], rv["w0"])
                ops.memset_zero(rv["added"])
                q0, q1 = rv["rows"][i]
            ops.attention_gradcolsum(ws["qkv"][i], ws["lse"][i], ws["dctx"], rv["r"], rv["cs"], B, T, H, q0=q0, q1=q1)
            # The added part is 1e-3 .. 1e-5 of w_pool on the pooled rows: summed into r itself it would lose its low bits to w_pool's
            # exponent at every layer.  It is accumulated on its own and r = w_pool + added is rounded once per layer.
            ops.relevance_step(rv["added"], rv["cs"], rv["added"], B, T, H)
            ops.add2d(rv["w0"], T, rv["added"], T, rv["r"], T, B, T)
        else:
            q0, q1 = rv["rows"][i]
            ops.attention_gradcolsum(ws["qkv"][i], ws["lse"][i], ws["dctx"], rv["w"][i], rv["maps"][i], B, T, H, q0=q0, q1=q1)

    # ------------------------------------------------------------------ input gradient (gaviko_amd.explain, img.requires_grad)
    def _ig_names(self) -> List[str]:
        """Every tensor whose gradient kernel the sweep may reach: the trainable ones, the method's own and the head.  An input-gradient
        sweep runs the full backward whatever trains, so the kernels of the tensors that do not train get scratch targets."""
        head = self.names.head()
        return [n for n, p in self.p.items() if p.requires_grad or n.startswith(head) or self._own_grad_kernels(n)]

    def _ig_scratch_views(self, device, real) -> Dict[str, torch.Tensor]:
        """Scratch gradient targets for the names of _ig_names that `real` (the flat buffer's views) lacks: all of them in "only" mode,
        where the scratch buffer takes the flat buffer's layout (distributed.flat_order: GAViKO's GPA gate tensors are one contiguous slice
        that one kernel writes) and stands in for it during the sweep (_backward)."""
        names = [n for n in self._ig_names() if n not in real]
        if not real:
            from .distributed import flat_order
            names = flat_order(tuple(names), self.cfg.get("share_factor", 1) if self.kind == "gaviko" else 1, self.bucket_layers)
        sig = (tuple((n, tuple(self.p[n].shape)) for n in names), str(device))
        sc = self._ig_scratch.get(self._igrad)
        if sc is None or sc["sig"] != sig:
            if sc is not None:                            # recorded plans hold the old buffer's addresses
                self._graphs.clear()
                self._calls.clear()
            buf, views = flat_views(self.p, names, device, min_elems=1)
            sc = self._ig_scratch[self._igrad] = {"sig": sig, "buf": buf, "views": views}
        return sc["views"]

    def _ig_buffers(self, ws, B, device) -> None:
        """Buffers of the input-gradient tail (in the workspace: a recorded plan keeps their addresses) and the transposed patch-embedding
        operand conv^T [Kp][C] (the dgrad GEMM's W), rebuilt in place when the conv weight changed.  SSF folds its scale into the operand
        inside the step (_input_grad_tail)."""
        C, BN, Kp = self.C, B * self.N, self.Kp
        if "ig" not in ws:
            ig = ws["ig"] = dict(dxc=ops.act_zeros(BN, C, torch.float32, device), dcols=ops.act_zeros(BN, Kp, torch.float32, device))
            if not self.fp32:
                ig["dxc16"] = ops.act_zeros(BN, C, self.adt, device)
            if self.kind == "evp":
                ig["dhc"] = ops.act_zeros(BN, 64, torch.float32, device)
                ig["dhcols"] = ops.act_zeros(BN, Kp, torch.float32, device)
                ig["dhp"] = torch.zeros_like(ws["img"])
                ig["dhp2"] = torch.zeros_like(ws["img"])
            ws["dimg"] = torch.zeros_like(ws["img"])
        w = self._w16
        if "conv_t" not in w:
            w["conv_t"] = torch.zeros((Kp, C), dtype=self.adt, device=device)
        if self.kind == "evp":
            st = self.method.state(self, device)
            if "hpT" not in st:
                st["hpT"] = st["hp"].t().contiguous()                   # the adjoint operator of the high-pass's linear part
                st["WpT"] = torch.zeros((Kp, 64), device=device)
        if self.kind == "ssf":
            return
        cw = self.p[self.names.conv() + ".weight"]
        version = (cw._version, cw.data_ptr())
        if version != self._conv_t_version:
            ops.transpose_operand(self._d(self.names.conv() + ".weight").reshape(C, Kp).contiguous(), w["conv_t"], self.adt)
            self._conv_t_version = version

    def _input_grad_tail(self, ws, sv, dG0, B, lo):
        """dG0 (the gradient of the layer-0 input) -> the gradient of the input volume.  The patch rows of dG0 (through emb_dropout) plus
        whatever else read the raw patch embedding -- GAViKO's local stream (the MWSA chain's input gradient, dL), EVP's
        embedding_generator (ds . W_e) -- make d xc [B*N][C]; d cols = d xc . W_conv (the dgrad GEMM against conv^T); the stride-equals-
        kernel convolution makes the volume a permutation of d cols (gvk_unpatchify_f32).  EVP adds its high-pass branch:
        d hcols = ds . W_p, un-patchified, through the modulus and the adjoint high-pass, back to the im2col layout and into d cols."""
        C, T, N, Kp, BN = self.C, self.T, self.N, self.Kp, B * self.N
        ig, w = ws["ig"], self._w16
        edrop = sv.get("edrop", 0.0)
        premasked = bool(sv.get("bb"))                    # the trainable-embedding tail above has applied the emb_dropout masks in place
        src = dG0
        if edrop > 0 and not premasked:
            ops.dropout_rows(dG0, edrop, SEED_EMB, ws["seed"], out32=ws["dx32"], M=B * T, N=C)
            src = ws["dx32"]
        ops.rows_gather(src, ig["dxc"], B, T, N, C, self.row_off)
        if self.kind == "gaviko":                          # local stream = conv(img) + pos[1:] (gaviko.py:545-546): its input gradient
            dlocal = ws["dL"][(self.depth - lo) & 1]        # (what _mwsa_final of the lowest layer wrote)
            if edrop > 0 and not premasked:
                ops.dropout_rows(dlocal, edrop, SEED_EMB + 1, ws["seed"], out32=dlocal, M=BN, N=C)
            ops.add2d(ig["dxc"], C, dlocal, C, ig["dxc"], C, BN, C)
        if self.kind == "evp":                             # embedding_generator reads the raw conv output (evp.py:347-348)
            ops.skinny_up(lat=ws["evb"]["ds"], w=self.method.state(self, dG0.device)["We"], out=ig["dxc"], M=BN, C=C, L=self.Lp, w_layout=1, accumulate=1)
        if self.kind == "ssf":                             # y = s o conv(img) + t (ssf.py:229-232): the operand is s o W, as the forward's
            ops.ssf_fold_weight(self.p[self.names.conv() + ".weight"].detach().reshape(C, Kp), self.p["ssf_scale_1"].detach(), w["conv"], w["conv_t"])
        a = ig["dxc"] if self.fp32 else ops.to_operand(ig["dxc"], ig["dxc16"], self.adt)
        ops.gemm_nt(a, w["conv_t"], BN, ig["dcols"], epilogue=ops.EPI_STORE_F32)
        if self.kind == "evp":
            st = self.method.state(self, dG0.device)
            # hc = hcols . Wp^T + bp, s = hc[:, :Lp] + e  ->  d hcols = ds . Wp (rows >= r of Wp are zero); fp32 as the forward's GEMM
            ops.pad2d(ws["evb"]["ds"], BN, self.Lp, ig["dhc"], BN, 64)
            ops.transpose_any(st["Wp"], st["WpT"], 64, Kp)
            ops.gemm_nt(ig["dhc"], st["WpT"], BN, ig["dhcols"], epilogue=ops.EPI_STORE_F32)
            ops.unpatchify(ig["dhcols"], ig["dhp"], self.patch)
            ops.evp_highpass_sign(ws["img"], st["hp"], st["dmask"], ig["dhp"], ig["dhp2"])
            ops.evp_highpass_linear(ig["dhp2"], st["hpT"], st["dmask"], ig["dhp"])
            ops.patchify(ig["dhp"], ig["dhcols"], self.patch)
            ops.add2d(ig["dcols"], Kp, ig["dhcols"], Kp, ig["dcols"], Kp, BN, Kp)
        ops.unpatchify(ig["dcols"], ws["dimg"], self.patch)
