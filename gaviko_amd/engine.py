"""Launch plans (forward + backward) of the 3D-ViT hot path on MI355X.

One `Engine` per model instance.  It owns
  * bf16 MFMA-operand shadows of the frozen fp32 weights, W and W^T (the dgrad of a frozen Linear is an NT GEMM against
    the pre-transposed weight; frozen weights need no wgrad and their GEMM inputs are never saved),
  * the per-batch-size workspace (fp32 residual streams per layer, bf16 GEMM operands, saved statistics),
  * the ordered list of C-ABI launches that make up forward() and backward().
GAViKO's side paths and the unfrozen-backbone gradients are mixins (engine_gaviko.py, engine_peft.py), and so are the analysis entry points
of gaviko_amd.explain / uncertainty / features (engine_analysis.py).  Everything else that is a method's own -- token geometry, feature
flags, workspace slots, name patterns AND its launches -- is one spec per kind in engine_methods.py (`self.method`): the sweeps here are the
backbone plus GAViKO's stream choreography, call `self.method.<hook>(self, ...)` wherever another method launches something, and compare
`self.kind` with "gaviko" only.
Everything is enqueued on torch's current HIP stream; nothing synchronises, so a whole step can be captured in a HIP
graph.  There is no CPU / eager fallback.

Data layout in HBM (B samples, T tokens, C channels, M = B*T):
  G[i], G1[i]   fp32 [pad128(M)][C]   global residual stream entering layer i / after its attention block
  Lc[i]         fp32 [B*N][C]         GAViKO local stream entering layer i
  xn / act / dpre ... bf16 [pad128(M)][*]  MFMA operands (transient, reused by every layer)
  qkv[i], ctx[i], pre[i]  bf16        saved for the backward (flash attention recompute, GELU')
Reference call structure mirrored here: gaviko.py:291-306 (layer loop), 531-552 (embedding + head).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import torch

from . import lib as L
from . import ops
from .engine_analysis import AnalysisPaths
from .engine_common import GRAPH_WARMUP, PLAN_TIMING, SEED_EMB, SEED_LAYER, USE_GRAPHS, _ABLATE, _EPI_NAMES, _SIDE_STREAMS, Names, _on, flat_views
from .engine_common import SEED_PROMPT, evp_highpass_operator  # noqa: F401  (re-exported: tests read them from here)
from .engine_gaviko import GavikoPaths
from .engine_methods import METHOD_SPECS
from .engine_peft import BackboneGrads

# bench.py instrumentation: when set to a dict, plans recorded from then on bracket every GEMM launch (and the patch-embed
# stage) with timestamped plan events, so the kernels are timed inside the real three-stream schedule of a replayed step.
GEMM_MARKS = None


class Engine(GavikoPaths, BackboneGrads, AnalysisPaths):
    def __init__(self, kind: str, cfg: dict, params: Dict[str, torch.nn.Parameter], depth, heads, dim, mlp_dim):
        self.kind, self.cfg, self.p = kind, cfg, params
        self.method = METHOD_SPECS.get(kind)           # everything that is the kind's own: geometry, flags, buffers, names, launches (engine_methods.py)
        if self.method is None:
            raise L.GavikoHipError(f"unknown engine kind {kind!r}: expected one of {tuple(METHOD_SPECS)}")
        self.depth, self.heads, self.C, self.mlp = depth, heads, dim, mlp_dim
        fp, ip = cfg["frame_patch_size"], cfg["image_patch_size"]
        self.patch = (fp, ip, ip)
        self.grid = (cfg["frames"] // fp, cfg["image_size"] // ip, cfg["image_size"] // ip)
        self.N = self.grid[0] * self.grid[1] * self.grid[2]
        self.Kp = fp * ip * ip
        self.K = cfg["num_classes"]
        # Operand precision of the backbone GEMMs / attention: "bf16" = MFMA bf16 operands with fp32 accumulation (the headline
        # path); "fp32" = exact fp32 arithmetic (gemm_f32.hip / attention_f32.hip) for the reference's fp32 configurations
        # (train.py:157 keeps the model in float32 unless config['train']['fp16']; BASELINE cfg4 is pinned at 1e-5).
        prec = str(cfg.get("precision") or os.environ.get("GAVIKO_HIP_PRECISION", "bf16")).lower()
        if prec not in ("bf16", "fp32", "float32"):
            raise L.GavikoHipError(f"precision={prec!r}: expected 'bf16' or 'fp32'")
        self.fp32 = prec != "bf16"
        self.q_scale = 64 ** -0.5 * ops.LOG2E     # what the saved q block carries on the bf16 path (attention kernels' operand form)
        self.adt = torch.float32 if self.fp32 else torch.bfloat16
        if cfg.get("dim_head", 64) != 64:
            raise L.GavikoHipError("the attention kernels are built for dim_head = 64")
        if cfg.get("channels", 1) != 1:
            raise L.GavikoHipError("patch embedding is built for single-channel volumes (channels = 1)")
        self.pool = cfg.get("pool", "cls")
        self.method.geometry(self, cfg)                # P, T, Ts, row_off and the method's own widths
        self.names = Names(self.method, self.lora_layers if self.method.wraps_qkv else None)
        self._w16: Dict[str, torch.Tensor] = {}
        self._w16_version = None
        self._shadowed = frozenset(self._backbone_weight_names())
        self._fwd_gen = 0                       # counts training-mode forwards: the autograd node checks it owns the saved state
        # static_io = True: forward() returns the workspace's logits buffer itself (valid until the next forward) instead of a copy
        self.static_io = False
        self._have_dgrad = False
        self._graphs = {}
        self._calls = {}
        self._wss = {}
        self._streams = {}
        self._recording = False
        self._keep_inputs = False               # unfrozen backbone weights: the forward keeps the GEMM inputs for their wgrads
        self._eff: Dict[str, torch.Tensor] = {}
        self._mwsa_pending = None
        self.method.flags(self, cfg)                   # the fusions of the frozen GAViKO path; all off for every other kind
        self.ldx = self.mlp + 64 if self._fuse_up else self.mlp      # row stride of the MLP hidden buffers
        self._fold: Dict[str, torch.Tensor] = {}
        self._fold_version = None
        self._fold_names = frozenset(self._fold_deps()) if self._fold_ln1 else frozenset()
        self._fold_on = False
        self._marks = []
        self.plan_marks = {}                # plan id -> [(name, event id)]
        self._bucket_marks = {}             # (stream kind, layer) -> event of the pass being issued / recorded: gradients of that layer final
        self.plan_bucket_marks = {}         # plan id -> that dict, for replays
        self._want_bucket_marks = False
        self._gemm_marks = []
        self.plan_gemm_marks = {}           # plan id -> [(class, flops, shape, bytes, e0, e1)]
        self._ws = None
        self._step = 0
        self._flat_grad = None
        self._flat_names = None
        self.bucket_layers = 4              # layout of the flat gradient buffer: completion groups of this many layers (set_bucket_layers)
        self._saved = None
        self._pre_is_grad = False
        self._relv = None                   # the input-only sweep being issued also feeds the attention-relevance kernels (relevance_backward)
        self._igrad = None                  # the backward being issued also carries the gradient to the input volume: None | "params" | "only"
        self._ig_scratch = {}               # input-gradient mode -> scratch gradient targets (a recorded plan keeps their addresses)
        self._conv_t_version = None

    def _gemm(self, a, w, M, out0, alg_k=None, **kw):
        """One NT GEMM launch.  alg_k: the ALGORITHMIC contraction length when the operand carries padding columns (fc2 with the
        K-concatenated GPA up-projection: 3072 + 20 of 3136 columns are products the reference computes, the split-bf16 copies and the
        zero padding are not) -- only the bench instrumentation reads it, for flop_per_launch."""
        if GEMM_MARKS is None or not self._recording:
            return ops.gemm_nt(a, w, M, out0, **kw)
        N, K = w.shape[0], int(kw.get("K") or w.shape[1])
        ka = int(alg_k) if alg_k is not None else K
        key = f"gemm_nt_{'f32' if self.fp32 else 'bf16'}[{_EPI_NAMES[kw['epilogue']]}] M={M} N={N} K={K}"
        mrows = M
        if kw.get("m_panels"):                               # strided row panels: 64-row tiles at the first rows of every sample
            mrows = 64 * kw["m_panels"]
            key += f" panels={kw['m_panels']}x64"
        cur = torch.cuda.current_stream()
        e0 = self._ev_record(cur)
        ops.gemm_nt(a, w, M, out0, **kw)
        e1 = self._ev_record(cur)
        self._gemm_marks.append((key, 2.0 * mrows * N * ka, [mrows, N, K], None, e0, e1))

    def collect_gemm_marks(self, acc=None):
        """After a sync: add the event-pair durations of the last replay of every instrumented plan to `acc`
        ({class: {"ms": [...], "flops", "shape", "bytes", "overhead_ms"}}).  Durations are RAW event-pair times (they agree with the
        rocprofv3 kernel durations of the same launches, profiles/r02_bench_kernel_stats.csv); the empty event pair recorded at the head
        of each plan is reported beside them as `overhead_ms`, never subtracted."""
        import ctypes
        acc = {} if acc is None else acc
        lib, ms = L.load(), ctypes.c_float()
        for pid, marks in self.plan_gemm_marks.items():
            overhead = 0.0
            for key, flops, shape, nbytes, e0, e1 in marks:
                L.check(lib.gvk_plan_event_elapsed(pid, e0, e1, ctypes.byref(ms)), "gvk_plan_event_elapsed")
                if key == "__empty__":
                    overhead = ms.value
                    continue
                rec = acc.setdefault(key, {"ms": [], "flops": flops, "shape": shape, "bytes": nbytes, "overhead_ms": overhead})
                rec["ms"].append(ms.value)
        return acc

    # ------------------------------------------------------------------ weights
    def _d(self, name) -> torch.Tensor:
        eff = self._eff.get(name)                 # SSF: LayerNorm affines and biases are read in their effective (folded) form
        return self.p[name].detach() if eff is None else eff

    def _backbone_weight_names(self) -> List[str]:
        n = [self.names.conv() + ".weight"]
        for i in range(self.depth):
            n += [self.names.qkv_weight(i), self.names.attn(i) + ".to_out.0.weight", self.names.mlp(i) + ".net.1.weight",
                  self.names.mlp(i) + ".net.4.weight"]
        return n

    def refresh_weights(self, need_dgrad: bool) -> None:
        """(Re)build the bf16 shadows when a source weight changed (load_state_dict, optimizer step on an unfrozen tensor).
        Shadows are rewritten IN PLACE so that captured HIP graphs keep pointing at valid operands."""
        if self.method.folds_in_step:
            return                                  # SSF: every operand is re-folded from (W, scale) inside the recorded step
        names = self._backbone_weight_names()
        version = tuple(self.p[n]._version for n in names) + tuple(self.p[n].data_ptr() for n in names)
        stale = version != self._w16_version
        w = self._w16
        if stale:
            conv = self._d(names[0]).reshape(self.C, self.Kp).contiguous()
            w["conv"] = ops.to_operand(conv, None if self.fp32 else w.get("conv"), self.adt)
        if not stale and (not need_dgrad or self._have_dgrad):
            return
        for i in range(self.depth):
            for tag, nm in (("qkv", self.names.qkv_weight(i)), ("out", self.names.attn(i) + ".to_out.0.weight"),
                            ("fc1", self.names.mlp(i) + ".net.1.weight"), ("fc2", self.names.mlp(i) + ".net.4.weight")):
                src = self._d(nm).contiguous()
                if stale and tag == "fc2" and self._fuse_up:
                    buf = w.get(f"fc2{i}")
                    if buf is None:
                        buf = w[f"fc2{i}"] = torch.zeros((self.C, self.ldx), dtype=self.adt, device=src.device)
                    buf[:, :self.mlp].copy_(src)                 # columns mlp.. are packed from the trainable proj_up inside every step
                elif stale:
                    w[f"{tag}{i}"] = ops.to_operand(src, None if self.fp32 else w.get(f"{tag}{i}"), self.adt)   # fp32: the parameter itself
                if need_dgrad and (stale or not self._have_dgrad):
                    w[f"{tag}{i}_t"] = ops.transpose_operand(src, w.get(f"{tag}{i}_t"), self.adt)
        self._have_dgrad = self._have_dgrad and not stale or need_dgrad
        self._w16_version = version

    def _fold_deps(self) -> List[str]:
        """Every tensor the folded qkv operands of layers 1.. are built from: the projection weight AND the LayerNorm affine."""
        n = []
        for i in range(1, self.depth):
            a = self.names.attn(i)
            n += [self.names.qkv_weight(i), a + ".norm.weight", a + ".norm.bias"]
        return n

    def _ensure_fold(self) -> bool:
        """Folded operands (gamma o W in bf16, c1 = its row sums, c2 = beta . W^T) of every layer > 0, rebuilt IN PLACE (recorded plans keep
        their pointers) whenever one of their sources changed -- whichever tensors train.  Called by every forward that may take the
        folded path (the ones that keep no GEMM inputs: a frozen backbone, or any eval / no-grad forward), so the path never meets a
        missing or stale operand (a Gaviko(freeze_vit=False) eval forward at ViT-B used to raise KeyError 'w1' here)."""
        if not self._fold_ln1:
            return False
        names = self._fold_deps()
        version = tuple(self.p[n]._version for n in names) + tuple(self.p[n].data_ptr() for n in names)
        if version == self._fold_version and self._fold:
            return True
        for i in range(1, self.depth):
            a = self.names.attn(i)
            Wq, g, b = self._d(self.names.qkv_weight(i)), self._d(a + ".norm.weight"), self._d(a + ".norm.bias")
            w16 = ops.to_operand((Wq * g[None, :]).contiguous(), self._fold.get(f"w{i}"), self.adt)
            self._fold[f"w{i}"] = w16
            for key, val in ((f"c1_{i}", w16.float().sum(1)),                # row sums of the bf16 operand the MFMAs actually multiply
                             (f"c2_{i}", (Wq * b[None, :]).sum(1))):          # beta . W^T
                if key in self._fold:
                    self._fold[key].copy_(val)
                else:
                    self._fold[key] = val.contiguous()
        self._fold_version = version
        return True

    # ------------------------------------------------------------------ workspace
    def _seed_base(self, train: bool) -> int:
        """Initial value of the device-side dropout epoch word.  Mixes torch's base seed (torch.manual_seed = the user's knob), the
        data-parallel rank and the mode, so that ranks -- and the train / eval workspaces of one rank -- draw independent masks, as
        the reference's per-process torch RNG streams do (train.py has no seeding; every process draws its own)."""
        rank = 0
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                rank = dist.get_rank()
        except Exception:
            rank = 0
        x = (torch.initial_seed() & 0xFFFFFFFFFFFF) * 0x9E3779B97F4A7C15 + (rank + 1) * 0xBF58476D1CE4E5B9 + (0x94D049BB133111EB if train else 0)
        x &= (1 << 64) - 1
        x ^= x >> 31
        return 0x5EED0000 ^ (x & 0x3FFFFFFFFFFF0000)          # stays positive in int64; the low 16 bits are left to the per-site offsets

    def invalidate_weights(self, names=None) -> None:
        """Tell the engine that parameters were written behind torch's back (a raw-pointer optimizer step: `p._version` does not move).
        With `names`, only if one of them is a backbone weight the engine keeps operand shadows of."""
        if names is None or any(n in self._shadowed for n in names):
            self._w16_version = None
        if names is None or any(n in self._fold_names for n in names):
            self._fold_version = None

    def workspace(self, B: int, device, train: bool, keep_attn: bool = False, tag: Optional[str] = None, feat: Optional[tuple] = None):
        """keep_attn (inference only, gaviko_amd.explain): a workspace of its own whose forward keeps every layer's qkv / lse (and every
        other per-layer slot) as a training forward does, for the attention-map kernels.  tag: another workspace of its own for the same
        (B, mode) -- 'igrad', the input-gradient sweeps of gaviko_amd.explain.  feat (inference only, gaviko_amd.features): a workspace of
        its own with the per-layer summary slots feat_cls / feat_patch [len(feat)][B][C] of feature_forward."""
        key = (B, train, str(device)) + (("attn",) if keep_attn else ()) + ((tag,) if tag else ()) + (("feat", feat) if feat else ())
        if key in self._wss:
            self._ws = self._wss[key]
            return self._ws
        C, T, N, M = self.C, self.T, self.N, B * self.T
        z = lambda r, c, dt: ops.act_zeros(r, c, dt, device)
        f32, bf16 = torch.float32, self.adt                # "bf16" below = the GEMM-operand dtype (fp32 on the fp32 path)
        nsave = self.depth if (train or keep_attn) else 1
        ws = {"key": key, "B": B, "M": M}
        ws["img"] = torch.zeros((B, 1) + tuple(g * p for g, p in zip(self.grid, self.patch)), device=device)
        ws["logits"] = torch.zeros((B, self.K), device=device)
        ws["dlogits"] = torch.zeros((B, self.K), device=device)
        ws["seed"] = torch.full((1,), self._seed_base(train), dtype=torch.int64, device=device)
        ws["cols"] = z(B * N, self.Kp, bf16)
        ws["G"] = [z(M, C, f32) for _ in range(self.depth + 1)] if train else [z(M, C, f32), z(M, C, f32)]
        ws["G1"] = [z(M, C, f32) for _ in range(nsave)]
        ws["xn"] = z(M, C, bf16)
        ws["qkv"] = [z(M, 3 * C, bf16) for _ in range(nsave)]
        ws["ctx"] = [z(M, C, bf16) for _ in range(nsave)]
        ws["lse"] = [torch.zeros((B, self.heads, T), device=device) for _ in range(nsave)]
        ws["pre"] = [z(M, self.ldx, bf16) for _ in range(nsave)] if train else [None]
        ws["act"] = z(M, self.ldx, bf16)
        if self._fuse_up:
            ws["act"][:, self.mlp + 3 * self.Lat: self.mlp + 3 * self.Lat + 2] = 1.0     # the two bias columns (b_hi, b_lo); the rest of the slot stays 0
        ws["stat"] = [[torch.zeros(M, device=device) for _ in range(4)] for _ in range(nsave)]   # mean1, rstd1, mean2, rstd2
        ws["pooled"] = torch.zeros((B, C), device=device)
        if feat:
            ws["feat_cls"] = torch.zeros((len(feat), B, C), device=device)
            ws["feat_patch"] = torch.zeros((len(feat), B, C), device=device)
        if self._fold_ln1:
            ws["xg16"] = z(M, C, bf16)                                          # bf16 copy of the global stream entering a folded layer
            ws["spart"] = torch.zeros((C // 64) * M * 2, device=device)         # per-row (sum, sum of squares) over 64-column groups
        self.method.forward_buffers(self, ws, B, device, train, nsave)      # the method's own slots (engine_methods.py)
        if train:
            ws["dG"] = [z(M, C, f32), z(M, C, f32)]          # ping-pong gradient of the global stream
            ws["dG16"] = z(M, C, bf16)
            ws["dpre"] = z(M, self.mlp, bf16)
            ws["dx32"] = z(M, C, f32)
            if self._dy16:
                ws["dx16b"] = z(M, C, bf16)
            ws["dctx"] = z(M, C, bf16)
            ws["dqkv"] = z(M, 3 * C, bf16)
            ws["delta"] = torch.zeros((B, self.heads, T), device=device)
            self.method.backward_buffers(self, ws, B, device)
        self._ws = self._wss[key] = ws       # one workspace (and one set of captured graphs) per (batch, mode)
        return ws

    # ------------------------------------------------------------------ two-stream fork / join
    # GAViKO's local branch (MWSA) and the latent-space GPA core are independent of the backbone's attention / MLP GEMMs within
    # a layer; they run on a side stream and meet the main stream only where the dataflow does (gaviko.py:301-304).  Inside
    # a HIP-graph capture these waits become graph edges, so the replayed graph has two parallel branches.
    def _stream(self, name):
        st = self._streams.get(name)
        if st is None:
            # One side stream of each kind per DEVICE, shared by every engine of the process (train + eval models, a test suite's many
            # models): engines run their steps one after another, and every stream of their own would eventually alias hardware queues
            # (tools/bench_reducer.py: the 5th model of a process ran 14.8 ms steps instead of 5.9).
            key = (torch.cuda.current_device(), name)
            st = _SIDE_STREAMS.get(key)
            if st is not None:
                self._streams[name] = st
                return st
            # (confining the side streams to a CU subset with hipExtStreamCreateWithCUMask was measured: 676 -> 170-260 volumes/s for
            #  every mask shape tried -- masked queues are far slower to dispatch on this runtime)
            st = self._streams[name] = _SIDE_STREAMS[key] = torch.cuda.Stream()
            if "sidenop" in _ABLATE or f"{name}nop" in _ABLATE:
                L.load().gvk_plan_nop_stream(st.cuda_stream)
        return st

    def _ev_record(self, stream):
        """Record an event on `stream`; while a launch plan is being recorded the event belongs to the plan."""
        if "noevents" in _ABLATE:
            return None
        if self._recording:
            rc = L.load().gvk_plan_event_record(stream.cuda_stream)
            if rc < 0:
                L.check(rc, "gvk_plan_event_record")
            return rc
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev

    def _bucket_mark(self, kind, layer):
        """Data parallelism (distributed.GradReducer, mode 'events'): an event on the CURRENT stream after the last kernel that writes
        a gradient of (`kind`, `layer`); the collective stream waits for it.  Recorded with the system-scope fence: peers read the data."""
        if not self._want_bucket_marks:
            return
        cur = torch.cuda.current_stream()
        if self._recording:
            rc = L.load().gvk_plan_event_record_fenced(cur.cuda_stream)
            if rc < 0:
                L.check(rc, "gvk_plan_event_record_fenced")
            self._bucket_marks[(kind, layer)] = rc
        else:
            ev = torch.cuda.Event()
            ev.record(cur)
            self._bucket_marks[(kind, layer)] = ev

    def _mark(self, name):
        """Diagnostics (GAVIKO_HIP_PLAN_TIMING=1): a timestamped plan event on the current stream, read by tools/plan_marks.py."""
        if self._recording and PLAN_TIMING:
            self._marks.append((name, self._ev_record(torch.cuda.current_stream())))

    def _ev_wait(self, stream, ev):
        if "noevents" in _ABLATE or ("nowait" in _ABLATE and stream.cuda_stream == torch.cuda.current_stream().cuda_stream):
            return
        if self._recording:
            L.check(L.load().gvk_plan_event_wait(stream.cuda_stream, ev), "gvk_plan_event_wait")
        else:
            stream.wait_event(ev)

    def _wait(self, waiter, on):
        """stream `waiter` waits for everything enqueued so far on stream `on` (None = the current/main stream)."""
        cur = torch.cuda.current_stream()
        src = cur if on is None else self._stream(on)
        dst = cur if waiter is None else self._stream(waiter)
        self._ev_wait(dst, self._ev_record(src))

    # ------------------------------------------------------------------ graphs
    def _run(self, tag, key, fn):
        """Run `fn` eagerly the first GRAPH_WARMUP times, then record it into a launch plan (csrc/runtime.hip) and replay that.
        Everything `fn` launches reads/writes workspace buffers only, so a replay is exactly one more step."""
        k = (tag,) + key + (torch.cuda.current_stream().cuda_stream,)
        g = self._graphs.get(k)
        self._last_run = ("eager", None)
        if g is not None:
            L.check(L.load().gvk_plan_replay(g), "gvk_plan_replay")
            self._last_run = ("replayed", g)
            return
        n = self._calls.get(k, 0)
        self._calls[k] = n + 1
        if not USE_GRAPHS or n < GRAPH_WARMUP:
            fn()
            return
        # this pass both executes and records; every launch inside fn goes through the library (no torch kernels)
        lib = L.load()
        L.check(lib.gvk_plan_begin(), "gvk_plan_begin")
        self._recording = True
        self._marks, self._gemm_marks = [], []
        self._bucket_marks = {}
        try:
            if GEMM_MARKS is not None:               # calibration: an empty event pair on the launch stream
                cur = torch.cuda.current_stream()
                self._gemm_marks.append(("__empty__", 0.0, None, None, self._ev_record(cur), self._ev_record(cur)))
            fn()
        except BaseException:
            lib.gvk_plan_abort()
            raise
        finally:
            self._recording = False
        pid = lib.gvk_plan_end()
        if pid < 0:
            L.check(pid, "gvk_plan_end")
        self._graphs[k] = pid
        self.plan_marks[pid] = (tag, self._marks)
        self.plan_bucket_marks[pid] = dict(self._bucket_marks)
        self._last_run = ("recorded", pid)
        if self._gemm_marks:
            self.plan_gemm_marks[pid] = self._gemm_marks
        return

    # ------------------------------------------------------------------ forward
    def forward(self, img: torch.Tensor, train: bool, drop: Optional[dict] = None, keep_attn: bool = False, ws_tag: Optional[str] = None,
                feat: Optional[tuple] = None) -> torch.Tensor:
        L.require_device()
        if not img.is_cuda:
            raise L.GavikoHipError("input volume must be on the HIP device: gaviko_amd has no CPU path")
        if img.dim() != 5 or img.shape[1] != 1 or tuple(img.shape[2:]) != tuple(g * p for g, p in zip(self.grid, self.patch)):
            raise L.GavikoHipError(f"expected img [B,1,{self.grid[0] * self.patch[0]},{self.grid[1] * self.patch[1]},"
                                   f"{self.grid[2] * self.patch[2]}], got {tuple(img.shape)}")
        B = img.shape[0]
        drop = drop or {}
        sv = {"B": B, "train": train, "keep": train or keep_attn, "attn_drop": float(drop.get("attn_drop", 0.0)), "proj_drop": float(drop.get("proj_drop", 0.0))}
        # nn.Dropout of the backbone itself (vision_transformer.py:33-34,52-54,157; vpt.py:129,148): live for the classes without a
        # train() override (linear / bitfit / fft, melo) and for VPT's prompt_dropout.  bf16 path only.
        sv["bdrop"], sv["edrop"], sv["pdrop"] = (float(drop.get(k, 0.0)) for k in ("dropout", "emb_dropout", "prompt_dropout"))
        sv["feat"] = tuple(feat) if (feat and not train) else ()     # feature_forward: the layers whose entering stream is summarised
        self.refresh_weights(need_dgrad=train)
        ws = self.workspace(B, img.device, train, keep_attn=keep_attn and not train, tag=ws_tag, feat=sv["feat"] or None)
        if img.data_ptr() != ws["img"].data_ptr():           # a caller that fills input_buffer() itself skips the copy-in launch
            ws["img"].copy_(img.detach())                   # static input buffer (the only per-step host-visible copy-in)
        # unfrozen backbone tensors (`fft` / `bitfit`, train.py:123-137): which ones train, and whether GEMM inputs must be kept
        # (`fft` / `bitfit` of the plain ViT; AdaptFormer(freeze_vit=False): adapters keep their own kernels, everything else is backbone)
        # Gaviko(freeze_vit=False): prompts / MWSA / GPA keep their own kernels, everything else is backbone)
        bb = frozenset()
        if train and self.method.backbone_trainable:
            head, own = self.names.head(), self.method.owns
            bb = frozenset(n for n in self.trainable_names() if not n.startswith(head) and not own(n))
        sv["bb"] = bb
        sv["wgrad"] = any(self.p[n].dim() >= 2 and n.endswith("weight") for n in bb)
        if bb:
            self._bb_buffers(ws, B, img.device, sv["wgrad"])
        key = (B, train, sv["attn_drop"], sv["proj_drop"], len(bb), sv["wgrad"], sv["bdrop"], sv["edrop"], sv["pdrop"])
        if keep_attn and not train:
            key += ("attn",)                                 # its own workspace: its own launch plan
        if ws_tag:
            key += (ws_tag,)
        if sv["feat"]:
            key += ("feat", sv["feat"])                     # its own workspace and two token_pool launches per layer: its own plan
        self._keep_inputs = bool(sv["wgrad"])
        sv["pre_is_grad"] = self._pre_is_grad = bool(train and self._gelu_grad and not self._keep_inputs and sv["bdrop"] <= 0 and not bb)
        self._fold_on = (not self._keep_inputs) and self._ensure_fold()      # ONE place decides: operands are current whenever the fold is taken
        self._run("fwd", key, lambda: self._forward_impl(ws, sv))
        self._saved = sv if train else None
        self._saved_key = key
        if train:
            self._fwd_gen += 1
        return ws["logits"] if self.static_io else ws["logits"].clone()

    def input_buffer(self, B: int, device, train: bool = True) -> torch.Tensor:
        """The static [B,1,D,H,W] input slot of the (B, train) workspace: a data pipeline that writes its batch here (and passes this very
        tensor to the model) saves the per-step device copy."""
        return self.workspace(B, device, train)["img"]

    def _forward_impl(self, ws, sv):
        B, C, T, N, train = sv["B"], self.C, self.T, self.N, sv["train"]
        M = B * T
        nm, d = self.names, self._d
        self._mark("f:begin")
        ops.seed_advance(ws["seed"], 7919)                  # device-side dropout epoch (replay safe)
        gaviko = self.kind == "gaviko"
        self.method.fwd_begin(self, ws, train)
        # ---- embedding: patch GEMM (+bias +pos, scattered to rows row_off..) and the broadcast rows
        marking = GEMM_MARKS is not None and self._recording  # bench.py: time the whole patch-embed stage (im2col + GEMM + scatter)
        cur = torch.cuda.current_stream()
        pe0 = self._ev_record(cur) if marking else None
        pos = d(nm.root + "pos_embedding")[0]
        G0 = ws["G"][0]
        # im2col -> bf16, then the MFMA GEMM scatters the token rows (a fused gather-GEMM was built in round 2 and measured slower: DESIGN.md 7b.5)
        ops.patchify(ws["img"], ws["cols"], self.patch)
        self.method.patch_embed(self, ws, B, G0, pos, out1=ws["Lc"][0] if gaviko else None)     # (EVP: + its latents)
        if marking:
            nout = 2 if gaviko else 1
            self._gemm_marks.append(("__patch_embed__", 2.0 * B * N * self.Kp * C, [B * N, C, self.Kp],
                                     B * (self.Kp * N * 4 + nout * N * C * 4), pe0, self._ev_record(cur)))
        self.method.embed_rows(self, G0, d(nm.root + "cls_token")[0], pos, B)           # cls, behind the prompts where they lead
        if sv["edrop"] > 0:                                   # x = dropout(x + pos) over [cls | patches] (vision_transformer.py:157)
            ops.dropout_rows(G0, sv["edrop"], SEED_EMB, ws["seed"], out32=G0, M=B * T, N=C)
            if gaviko:                                        # ... and, with its own draw, over the local tokens (gaviko.py:544,548)
                ops.dropout_rows(ws["Lc"][0], sv["edrop"], SEED_EMB + 1, ws["seed"], out32=ws["Lc"][0], M=B * N, N=C)
        self.method.fwd_embedded(self, ws, sv, G0, train)     # VPT's projected prompts, the MeLO merge, AdaptFormer's operand shadows
        # ---- layers.  main stream: attention block -> MLP block;  side stream: MWSA -> GPA latents / gates / cross-attention
        if gaviko:
            loc, gpa = self._stream("loc"), self._stream("gpa")
            self._wait("loc", None)                                  # Lc[0] written by the patch GEMM
            self._wait("gpa", None)
            fuse_up = self._fuse_up and sv["bdrop"] <= 0             # (dropout behind fc2 must not touch the up-projection)
            # The trainable half of W'_fc2 (gvk_pack_split_bf16) is written on the GPA stream, layer i+1's in the idle time behind layer i's GPA:
            # all twelve at the head of the step made layer 0's GPA -- and with it the main stream's prompt fix -- wait for them.
            def side_weights(i):
                if fuse_up and "noside" not in _ABLATE and i + 1 < self.depth:
                    with torch.cuda.stream(gpa):
                        pre, _ = self._gpa_names(i + 1)
                        ops.pack_split_bf16(d(pre + ".proj_up.weight"), self._w16[f"fc2{i + 1}"], self.mlp, C, b=d(pre + ".proj_up.bias"), weight_side=True)
            side_weights(-1)                                         # (layer 0's operand)
        folded_in = False                                            # this layer's first LayerNorm rides its qkv GEMM (self._fold_ln1)
        for i in range(self.depth):
            si = i if sv["keep"] else 0
            gi, go = (i, i + 1) if train else (i & 1, (i + 1) & 1)
            Mi = B * self.Ts[i]
            gout = self.method.layer_out(self, ws, go)               # (deep VPT: the layer output before its re-pack)
            if sv["feat"]:
                self._feat_pool(ws, sv, i, ws["G"][gi], self.Ts[i])       # before anything of layer i touches its input (EVP adds its prompt in place)
            if gaviko:
                if not train and i > 0:
                    self._wait("loc", "gpa")                         # eval ping-pongs Lc: the GPA of layer i-1 must be done with it
                with torch.cuda.stream(loc):
                    # with the 16-row-tile kernels the MWSA up-projection also emits GPA's proj_down of the rows it writes
                    fuse_local = self._fuse_proj and self._fuse_local
                    self._mwsa_fwd(ws, sv, i, si, ws["Lc"][gi], ws["Lc"][go], gpa_local=fuse_local)
                    if self._fuse_proj and not fuse_local:
                        self._gpa_down_local(ws, i, si, ws["Lc"][go], B)
            self._mark(f"f{i}:start")
            self.method.fwd_layer_begin(self, ws, i, si, ws["G"][gi], B)      # EVP: x[:, 1:] += prompt_i
            self._attn_block_fwd(ws, i, si, ws["G"][gi], ws["G1"][si], Mi, sv["bdrop"], folded=folded_in)
            self._mark(f"f{i}:attn")
            fused = gaviko and self._fuse_proj
            if gaviko and not fused:
                self._wait("gpa", None)                              # G1 ready
                self._wait("gpa", "loc")                             # L' ready
                with torch.cuda.stream(gpa):
                    self._gpa_fwd_latents(ws, i, si, ws["G1"][si], ws["Lc"][go], M, B, True)
                side_weights(i)
            self.method.fwd_after_attn(self, ws, i, si, ws["G1"][si], Mi, B)  # AdaptFormer's down-projection, DVPT's latents
            self._mlp_ln_fwd(ws, i, si, ws["G1"][si], Mi, fused)     # fused: also zx / xl = GPA proj_down(G1), same pass
            if fused:
                self._wait("gpa", None)                              # xl ready
                self._wait("gpa", "loc")                             # ll ready (the MWSA chain projects its own L')
                with torch.cuda.stream(gpa):
                    self._gpa_fwd_latents(ws, i, si, ws["G1"][si], ws["Lc"][go], M, B, False)
                side_weights(i)
            up_in_fc2 = gaviko and fused and fuse_up
            fold_next = bool(up_in_fc2 and self._fold_on and i + 1 < self.depth and _on("noside"))
            # fc2 carries proj_up of the PLAIN latents of every row (ready right behind the LayerNorm); the GPA has the two GEMMs' time
            # to finish, and only the P prompt rows it replaces are fixed up afterwards
            # the last layer's output is read at the pooled rows only (frozen backbone, no dropout behind fc2): its MLP runs on those rows
            # (feature_forward with `depth` requested reads every row of that output: no pruning in that plan)
            last_rows = (self._panels(B, self._pool_rows()[0] + self._pool_rows()[1])
                         if (gaviko and i + 1 == self.depth and up_in_fc2 and not self._keep_inputs and sv["bdrop"] <= 0
                             and self.depth not in sv["feat"]) else None)
            self._mlp_block_fwd(ws, i, si, ws["G1"][si], gout, Mi, train, sv["bdrop"],
                                up_in_fc2=up_in_fc2, stats_out=fold_next, panels=last_rows)
            self.method.fwd_after_mlp(self, ws, i, si, gout, Mi)     # ... and their up-projections into gout
            self._mark(f"f{i}:mlp")
            if gaviko and up_in_fc2:
                # the P prompt rows still lack (enh - xl) . Wup^T; when the next layer's first LayerNorm is folded into its qkv GEMM, the
                # fix also turns the fc2 GEMM's row partials into that LayerNorm's mean / rstd
                pre, _ = self._gpa_names(i)
                g = ws["gp"][si]
                self._wait(None, "gpa")                              # enh ready
                if fold_next:
                    sn = ws["stat"][si + 1 if sv["keep"] else 0]
                    ops.prompt_up_fix_stats(g["enh"], g["xl"], d(pre + ".proj_up.weight"), ws["G"][go], ws["xg16"], ws["spart"],
                                            sn[0], sn[1], B, self.T, self.P, C, self.Lat, pivot=ws["stat"][si][2])
                elif _on("noside"):
                    ops.prompt_up_fix(g["enh"], g["xl"], d(pre + ".proj_up.weight"), ws["G"][go], B, self.T, self.P, C, self.Lat)
                folded_in = fold_next
            elif gaviko:
                self._wait(None, "gpa")                              # enh ready
                self._gpa_fwd_up(ws, i, si, ws["G"][go], M)
            self._mark(f"f{i}:end")
            self.method.fwd_layer_end(self, ws, sv, i, gout, go, B)  # deep VPT: re-pack into G[go], prompt dropout
        if gaviko:
            self._wait(None, "loc")                                  # join the local chain (capture needs every fork joined)
        gfin = self._final_stream(ws, train)
        if sv["feat"]:
            self._feat_pool(ws, sv, self.depth, gfin, self.Ts[-1])
        r0, R = self._pool_rows()
        ops.head_fwd(g=gfin, ln_gamma=d(nm.root + "transformer.norm.weight"), ln_beta=d(nm.root + "transformer.norm.bias"),
                     wh=d(nm.head() + ".weight"), bh=d(nm.head() + ".bias"), logits=ws["logits"], pooled=ws["pooled"],
                     B=B, T=self.Ts[-1], C=C, K=self.K, r0=r0, R=R)
        self._mark("f:head")

    def _final_stream(self, ws, train):
        return self.method.final_stream(self, ws, train)

    def _pool_rows(self):
        return self.method.pool_rows(self)

    def _masked_grad(self, ws, dy, p, seed, need32, M):
        """ws['dG16'] (the dgrad GEMM operand) = dy * mask; also returns the fp32 masked gradient when bias / weight gradients need it."""
        if self.fp32:                                        # the operand IS fp32 on this path
            ops.dropout_rows(dy, p, seed, ws["seed"], out32=ws["dG16"], M=M, N=self.C)
            return ws["dG16"]
        out32 = ws["dyd"] if need32 else None
        ops.dropout_rows(dy, p, seed, ws["seed"], out32=out32, out16=ws["dG16"], M=M, N=self.C)
        return out32

    def _attn_block_fwd(self, ws, i, si, gin, g1, M, pdrop=0.0, folded=False):
        nm, w, d, C = self.names, self._w16, self._d, self.C
        a = nm.attn(i)
        st = ws["stat"][si]
        if folded:
            # LayerNorm folded into the projection: A = the raw rows (bf16 copy left by the fc2 GEMM below + the prompt fix), W = gamma o W,
            # mean / rstd of the rows already in st[0], st[1] (gvk_prompt_up_fix_stats)
            fo = self._fold
            self._gemm(ws["xg16"], fo[f"w{i}"], M, ws["qkv"][si], epilogue=ops.EPI_STORE_BF16, bias=fo[f"c2_{i}"], ln_mean=st[0], ln_rstd=st[1],
                       ln_c1=fo[f"c1_{i}"], scale_cols=self.heads * 64, col_scale=self.q_scale)
            ops.attention_fwd(ws["qkv"][si], ws["ctx"][si], ws["lse"][si], ws["B"], self.Ts[i], self.heads, 64 ** -0.5,
                              drop_p=pdrop, seed=SEED_LAYER + 8 * i, seed_ptr=ws["seed"], q_prescaled=True)
            self._gemm(ws["ctx"][si], w[f"out{i}"], M, g1, epilogue=ops.EPI_BIAS_RES_F32, bias=d(a + ".to_out.0.bias"), res=gin,
                       drop_p=pdrop, seed=SEED_LAYER + 8 * i + 1, seed_ptr=ws["seed"])
            return
        ops.layernorm_fwd(gin, d(a + ".norm.weight"), d(a + ".norm.bias"), M, C, y16=ws["xn"], mean=st[0], rstd=st[1])
        if self._keep_inputs:
            ops.copy_(ws["sav"]["xn1"][si], ws["xn"])
        # bf16 path: the q block leaves the projection as q * scale * log2(e) (one rounding, in the GEMM epilogue) -- the form the flash
        # kernels take, forward and backward alike; the fp32 kernels take the raw block
        qs = {} if self.fp32 else dict(scale_cols=self.heads * 64, col_scale=self.q_scale)
        self._gemm(ws["xn"], w[f"qkv{i}"], M, ws["qkv"][si], epilogue=ops.EPI_STORE_BF16, bias=self._eff.get(a + ".to_qkv.bias"), **qs)
        ops.attention_fwd(ws["qkv"][si], ws["ctx"][si], ws["lse"][si], ws["B"], self.Ts[i], self.heads, 64 ** -0.5,
                          drop_p=pdrop, seed=SEED_LAYER + 8 * i, seed_ptr=ws["seed"], q_prescaled=True)
        self._gemm(ws["ctx"][si], w[f"out{i}"], M, g1, epilogue=ops.EPI_BIAS_RES_F32, bias=d(a + ".to_out.0.bias"), res=gin,
                   drop_p=pdrop, seed=SEED_LAYER + 8 * i + 1, seed_ptr=ws["seed"])

    def _mlp_ln_fwd(self, ws, i, si, g1, M, fused):
        nm, d, C = self.names, self._d, self.C
        m = nm.mlp(i)
        st = ws["stat"][si]
        if fused:
            pre, _ = self._gpa_names(i)
            g = ws["gp"][si]
            split = dict(y_split=ws["act"], col_split=self.mlp) if self._fuse_up else {}      # the plain latents ride fc2 (self._fuse_up)
            ops.layernorm_fwd_proj(g1, d(m + ".net.0.weight"), d(m + ".net.0.bias"), M, C, y16=ws["xn"], mean=st[2], rstd=st[3],
                                   w=d(pre + ".proj_down.0.weight"), bias=d(pre + ".proj_down.0.bias"), z=g["zx"], y=g["xl"], act=1, w_layout=0,
                                   L_=self.Lat, **split)
        else:
            ops.layernorm_fwd(g1, d(m + ".net.0.weight"), d(m + ".net.0.bias"), M, C, y16=ws["xn"], mean=st[2], rstd=st[3])

    def _panels(self, B, rows):
        """gemm_nt kwargs that restrict a launch to the first `rows` rows of every sample (64-row tiles at stride T), or {}."""
        if not self.prune_dead_rows or rows > 64 or self.T < 64:
            return {}
        return dict(m_panels=B, m_stride=self.T)

    def _mlp_block_fwd(self, ws, i, si, g1, gout, M, train, pdrop=0.0, up_in_fc2=False, stats_out=False, panels=None):
        nm, w, d, C = self.names, self._w16, self._d, self.C
        m = nm.mlp(i)
        pk = panels or {}
        if self._keep_inputs:
            ops.copy_(ws["sav"]["xn2"][si], ws["xn"])
        gg = bool(train and self._pre_is_grad)               # decided once per step in forward(); the backward reads ws["pre"] accordingly
        self._gemm(ws["xn"], w[f"fc1{i}"], M, ws["pre"][si] if train else None, epilogue=ops.EPI_BIAS_GELU_BF16, out1=ws["act"],
                    bias=d(m + ".net.1.bias"),           # inference keeps no pre-activation (out0 = NULL)
                    ldo=self.ldx, drop_p=pdrop, seed=SEED_LAYER + 8 * i + 2, seed_ptr=ws["seed"], aux_is_grad=int(gg), **pk)
        if self._keep_inputs:
            ops.copy_(ws["sav"]["act"][si], ws["act"])
        so = (dict(epilogue=ops.EPI_BIAS_RES_F32_BF16, out1=ws["xg16"], stat_part=ws["spart"], stat_pivot=ws["stat"][si][2]) if stats_out     # pivot = mean of the residual row (LN2)
              else dict(epilogue=ops.EPI_BIAS_RES_F32))
        self._gemm(ws["act"], w[f"fc2{i}"], M, gout, bias=d(m + ".net.4.bias"), res=g1,
                   K=self.ldx if up_in_fc2 else self.mlp,      # the GPA latents ride this GEMM as 64 extra K columns (self._fuse_up)
                   alg_k=self.mlp + self.Lat if up_in_fc2 else None,
                   drop_p=pdrop, seed=SEED_LAYER + 8 * i + 3, seed_ptr=ws["seed"], **so, **pk)

    # ------------------------------------------------------------------ backward
    def trainable_names(self) -> List[str]:
        return [k for k, p in self.p.items() if p.requires_grad]

    def flat_names(self) -> List[str]:
        """Trainable tensors in the order of the flat gradient buffer: grouped by the bucket of the backward sweep that completes them
        (distributed.flat_order), so that what the data-parallel reducer sends together is one contiguous slice."""
        from .distributed import flat_order
        key = (tuple(self.trainable_names()), self.bucket_layers)
        if self._flat_names is None or self._flat_names[0] != key:
            self._flat_names = (key, flat_order(key[0], self.method.share_factor(self.cfg), self.bucket_layers))
        return self._flat_names[1]

    def set_bucket_layers(self, k: int) -> None:
        """Layers per gradient bucket of the flat layout (model.make_reducer passes its own).  Changing it moves gradient views: recorded
        plans hold their addresses, so they are dropped."""
        k = int(k)
        if k != self.bucket_layers:
            self.bucket_layers = k
            self._flat_grad = None
            self._graphs.clear()
            self._calls.clear()

    def set_prune(self, on: bool) -> None:
        """Dead-row pruning on / off (see prune_dead_rows in __init__).  Recorded plans hold the launch lists, so they are dropped."""
        on = bool(on) and self.method.supports_prune and not self.fp32
        if on != self.prune_dead_rows:
            self.prune_dead_rows = on
            self._graphs.clear()
            self._calls.clear()

    def _grad_views(self, device) -> Dict[str, torch.Tensor]:
        names = self.flat_names()
        sig = tuple((n, tuple(self.p[n].shape)) for n in names)
        if self._flat_grad is None or self._flat_grad["sig"] != sig or self._flat_grad["buf"].device != device:
            buf, views = flat_views(self.p, names, device)
            self._flat_grad = {"sig": sig, "buf": buf, "views": views}
        return self._flat_grad["views"]

    @property
    def flat_grad(self) -> Optional[torch.Tensor]:
        return None if self._flat_grad is None else self._flat_grad["buf"]

    def backward(self, dlogits: torch.Tensor, reducer=None, input_grad: Optional[str] = None) -> Dict[str, torch.Tensor]:
        """Fills and returns {param name: gradient view into the flat fp32 gradient buffer} for every trainable tensor.
        The sweep is cut into segments at the reducer's bucket boundaries (one segment without a reducer); each segment is a
        HIP graph after warm-up.  `reducer` (distributed.GradReducer) is told after every segment which layers are done, so
        finished buckets of the flat buffer are all-reduced on its side stream while the next segment runs.
        input_grad: the sweep also carries the gradient down to the input volume (ws['dimg'], ws['ig']['dcols']) -- "params": and the
        parameter gradients as without it (bit-identical); "only": no parameter gradient is written (the kernels that produce them write
        into a scratch buffer of its own; the flat buffer and every .grad stay untouched) and {} is returned."""
        if input_grad not in (None, "params", "only"):
            raise L.GavikoHipError(f"input_grad={input_grad!r}: expected None, 'params' or 'only'")
        if input_grad is None:
            return self._backward(dlogits, reducer)
        self._igrad = input_grad
        try:
            return self._backward(dlogits, reducer if input_grad == "params" else None)
        finally:
            self._igrad = None

    def _backward(self, dlogits, reducer):
        sv = self._saved
        if sv is None:
            raise L.GavikoHipError("backward() without a preceding training-mode forward()")
        ws = self._ws
        ig = self._igrad
        gv = self._grad_views(dlogits.device) if ig != "only" else {}
        unsupported = [n for n in gv if not self._grad_supported(n)]
        if unsupported:
            raise NotImplementedError(f"gradients for backbone tensors are not built yet (frozen-backbone PEFT only): {unsupported[:3]}...")
        real = gv
        if ig:
            self._ig_buffers(ws, sv["B"], dlogits.device)
            gv = dict(real, **self._ig_scratch_views(dlogits.device, real))
        if dlogits.data_ptr() != ws["dlogits"].data_ptr():
            ws["dlogits"].copy_(dlogits.detach())
        flat = self._flat_grad["buf"] if ig != "only" else None
        saved_key = self._saved_key + (("ig", ig),) if ig else self._saved_key
        if self._relv is not None:
            saved_key += (("relv",) + self._relv["key"],)
        if ig == "only":
            keep = self._flat_grad
            self._flat_grad = self._ig_scratch["only"]        # the kernels that address the flat buffer directly write the scratch
            try:
                return self._backward_sweep(ws, sv, gv, real, flat, saved_key, reducer)
            finally:
                self._flat_grad = keep
        return self._backward_sweep(ws, sv, gv, real, flat, saved_key, reducer)

    def _backward_sweep(self, ws, sv, gv, real, flat, saved_key, reducer):
        ig = self._igrad
        if reducer is not None:
            reducer.begin()
        if not self._needs_backbone_backward() and not ig:
            self._run("bwd_head", saved_key, lambda: self._backward_head(ws, sv, gv, False))
            if reducer is not None:
                reducer.finish(flat)
            return gv
        if reducer is not None and getattr(reducer, "mode", "segments") == "events":
            # ONE plan; every bucket is reduced behind the event recorded on the stream that finalises it (no cut, no join)
            self._want_bucket_marks = True
            self._bucket_marks = {}
            try:
                self._run("bwd0", saved_key + ("events",),
                          lambda: self._backward_segment(ws, sv, gv, self.depth - 1, 0, True, True))
            finally:
                self._want_bucket_marks = False
            how, pid = self._last_run
            if how in ("replayed", "recorded"):
                marks, lib = self.plan_bucket_marks[pid], L.load()
                waiter = lambda stream, ev: L.check(lib.gvk_plan_event_stream_wait(pid, ev, stream.cuda_stream), "gvk_plan_event_stream_wait")
            else:
                marks = self._bucket_marks
                waiter = lambda stream, ev: stream.wait_event(ev)
            reducer.reduce_marked(flat, marks, waiter)
            return real
        cuts = sorted({r for r, _, _ in reducer.ranges if r >= 0}, reverse=True) if reducer is not None else []
        cuts = [c for c in cuts if 0 < c < self.depth]          # segment k ends (inclusive) at layer cuts[k]
        hi = self.depth - 1
        for seg, lo in enumerate(cuts + [0]):
            first, last = seg == 0, lo == 0
            self._run(f"bwd{seg}", saved_key + (tuple(cuts),),
                      lambda hi=hi, lo=lo, first=first, last=last: self._backward_segment(ws, sv, gv, hi, lo, first, last))
            if reducer is not None:
                reducer.layer_done(flat, lo)
            hi = lo - 1
        if reducer is not None:
            reducer.finish(flat)
        return real

    def _backward_head(self, ws, sv, gv, backbone_bwd):
        nm, d = self.names, self._d
        B, C = sv["B"], self.C
        r0, R = self._pool_rows()
        dG = ws["dG"][0] if backbone_bwd else None
        if backbone_bwd:
            ops.memset_zero(dG)
        ops.head_bwd(g=self._final_stream(ws, True), ln_gamma=d(nm.root + "transformer.norm.weight"),
                     ln_beta=d(nm.root + "transformer.norm.bias"), wh=d(nm.head() + ".weight"), bh=d(nm.head() + ".bias"), pooled=ws["pooled"],
                     dlogits=ws["dlogits"], dg=dG, dwh=gv[nm.head() + ".weight"], dbh=gv[nm.head() + ".bias"], B=B, T=self.Ts[-1], C=C,
                     K=self.K, r0=r0, R=R, accumulate=0)
        bb = sv.get("bb") or ()
        nw, nb = nm.root + "transformer.norm.weight", nm.root + "transformer.norm.bias"
        if backbone_bwd and (nw in bb or nb in bb):
            g, bw, Tl = self._final_stream(ws, True), ws["bbw"], self.Ts[-1]
            ops.layernorm_fwd(g, d(nw), d(nb), B * Tl, C, y16=ws["xn"], mean=bw["stat"][0], rstd=bw["stat"][1])
            ops.ssf_head_grad(g, bw["stat"][0], bw["stat"][1], d(nm.head() + ".weight"), ws["dlogits"], bw["ones"][:C], bw["zeros"][:C],
                              gv[nw] if nw in bb else bw["junk"][:C], gv[nb] if nb in bb else bw["junk"][C: 2 * C], B, Tl, C, self.K, r0, R)
        if backbone_bwd:
            self.method.bwd_head(self, ws, sv, gv, bb, B)            # SSF: the final norm's scale / shift
            ops.to_operand(dG, ws["dG16"], self.adt)
            if self.kind == "gaviko":
                ops.memset_zero(ws["dL"][0])

    def _backward_segment(self, ws, sv, gv, hi, lo, first, last):
        """Layers hi, hi-1, ..., lo of the backward sweep (+ the head when `first`, + the embedding rows when `last`).
        ws['dG'][0] always holds the gradient of the global stream at a layer boundary, ws['dG'][1] the mid-layer one;
        the local-stream gradient ping-pongs with the layer parity."""
        if first:
            self._mwsa_pending = None
        B, C = sv["B"], self.C
        gaviko = self.kind == "gaviko"
        if first:
            self._mark("b:begin")
            self._backward_head(ws, sv, gv, True)
        dGout, dGin = self.method.bwd_first_boundary(self, ws, hi), ws["dG"][1]      # (dG[0]; deep VPT's un-repack alternates two buffers)
        if gaviko and ((self.depth - 1 - hi) & 1):
            dGout = ws["dGb"]                                  # the boundary gradient ping-pongs with the layer parity (see below)
        if gaviko:
            loc, gpa = self._stream("loc"), self._stream("gpa")
            self._wait("gpa", None)
            self._wait("loc", None)
        bb = sv.get("bb") or ()
        # frozen backbone: the fc1 / qkv dgrad GEMMs hand the LayerNorm backward its input gradient in bf16 (self._dy16)
        dy16 = bool(self._dy16 and not bb and not sv["wgrad"])
        # Dead rows of a frozen backbone (prune_dead_rows).  Top layer (the first of the sweep): the incoming gradient is an exact zero outside
        # the rows the head pools, so its MLP backward (row-wise) runs on those rows.  Bottom layer (the last of the sweep): of its INPUT gradient
        # only the P prompt rows of every sample are read (prompt_embeddings and their position embedding; patch embedding, cls token and
        # pos_embedding carry none), so its qkv dgrad and LayerNorm-1 backward run on those rows.
        frozen = gaviko and not bb and sv.get("bdrop", 0.0) <= 0 and not sv["wgrad"]
        top = self._panels(B, sum(self._pool_rows())) if (frozen and first) else {}
        if self._relv is not None and self._relv["allrows"]:
            top = {}                                           # a map of a row the head does not pool reads that row of the top layer's dctx
        bot = self._panels(B, self.P) if (frozen and last and self.P > 0 and not self._igrad) else {}     # (the input gradient reads every row)
        prev_scl = None
        for i in range(hi, lo - 1, -1):
            M = B * self.Ts[i]
            par = (self.depth - 1 - i) & 1
            # GPA stream: the critical kernels (-> dzx, dzl) first, then the parameter gradients; the other streams wait only
            # for the event between the two
            if gaviko:
                with torch.cuda.stream(gpa):
                    # dcomb = dGout . W_up was produced by the LayerNorm backward that wrote dGout, except for the top layer
                    self._gpa_bwd_core(ws, sv, gv, i, dGout, M, B, par, project=not self._fuse_proj or i == self.depth - 1)
                    dz_ready = self._ev_record(gpa)
                    self._gpa_bwd_params(ws, sv, gv, i, dGout, M, B, par)
                    self._bucket_mark("gpa", i)                              # prompt_projs.{i // share} gradients final once the lowest layer using it is done
            self._mark(f"b{i}:start")
            self._mlp_block_bwd(ws, sv, gv, i, dGout, dGin, dy16, top if i == self.depth - 1 else {})
            self._mark(f"b{i}:ln2")
            if gaviko:
                self._ev_wait(torch.cuda.current_stream(), dz_ready)
                self._gpa_bwd_scatter_g(ws, i, dGin, M)                      # dG1 += dzx.Wd (+ bf16 copy)
                self._mark(f"b{i}:scatter")
                # The MWSA chain of this layer (~170 us of kernels against ~290 us of backbone work per layer) runs beside the attention
                # backward, which it slows by 21 % (tools/plan_marks.py, locnop ablation); holding it back until that is through was
                # measured slower and removed
                self._mwsa_chain_bwd(ws, sv, gv, i, par, B, loc, dz_ready)
            # The new boundary gradient of GAViKO goes to the OTHER parity buffer: the GPA parameter kernels of this layer keep reading
            # dGout off the critical path.  The buffer being overwritten was last read by layer i+1's parameter kernels, which precede this
            # layer's dz_ready in the GPA stream -- and the main stream has already waited for that above.
            if gaviko:
                dGout = ws["dGb"] if dGout is ws["dG"][0] else ws["dG"][0]
            self._attn_block_bwd(ws, sv, gv, i, dGin, dGout, dy16, bot if i == 0 else {})
            if gaviko:
                # The MWSA chain never feeds the global stream in the backward, so the main stream does not join it per layer: dzl
                # is double-buffered by layer parity and the only cross-stream hazard left is layer i-1's GPA rewriting the buffer
                # layer i+1's scatter read -- ordered by making the GPA stream (not the main one) wait for THAT long finished kernel.
                if prev_scl is not None:
                    self._ev_wait(gpa, prev_scl)
                prev_scl = self._scl_done
                self._wait("gpa", None)                                      # the next layer's GPA backward needs this dG[i]
            self.method.bwd_layer(self, ws, gv, bb, i, dGout, B)              # EVP's layer step, the SSF unfold: before the layer's bucket is final
            self._mark(f"b{i}:end")
            if not gaviko:
                self._bucket_mark("main", i)                                 # transformer.layers.{i}.* gradients (adapters, LoRA, ...) are final
            dGout = self.method.bwd_layer_boundary(self, ws, sv, i, dGout, B)   # VPT: its prompt rows end here; deep VPT un-repacks into the other buffer
        if gaviko:
            if last:                                                         # (the deferred step crosses segment boundaries like layer boundaries)
                # frozen embedding: the local stream's INPUT gradient (layer 0's deferred last step) has no reader -- conv / pos_embedding carry none
                self._mwsa_flush(ws, B, loc, dead=self.prune_dead_rows and lo == 0 and not sv.get("bb") and not self._igrad)
            self._wait(None, "gpa")
            self._wait(None, "loc")
        if last and sv.get("bb"):
            if sv.get("edrop", 0.0) > 0:                                     # through emb_dropout
                ops.dropout_rows(dGout, sv["edrop"], SEED_EMB, ws["seed"], out32=dGout, M=B * self.T, N=C)
            # a second gradient of the raw patch embedding: what _mwsa_final of GAViKO's lowest layer wrote; EVP's embedding_generator share
            dlocal = ws["dL"][(self.depth - 1 - lo + 1) & 1] if gaviko else self.method.bwd_embed_dlocal(self, ws, dGout, B)
            if gaviko and sv.get("edrop", 0.0) > 0:
                ops.dropout_rows(dlocal, sv["edrop"], SEED_EMB + 1, ws["seed"], out32=dlocal, M=B * self.N, N=C)
            self._bb_embed_grads(ws, gv, sv["bb"], dGout, B, dlocal=dlocal, dlocal_to_pos=gaviko)
        if last:
            # what the method's own tensors still lack: EVP's generators, SSF's patch-embedding site, VPT's prompt_proj, the leading prompt rows
            self.method.bwd_tail(self, ws, sv, gv, dGout, B)
        if last and self._igrad:
            self._input_grad_tail(ws, sv, dGout, B, lo)
        if last:
            self._bucket_mark("main", -1)                                    # everything else (prompts, head, unindexed tensors): end of the sweep
        self._mark("b:tail")                                                 # side streams joined, embedding-side gradients issued

    def _mlp_block_bwd(self, ws, sv, gv, i, dGout, dGin, dy16, top):
        """Main stream, MLP block of layer i: dGin = dGout + LN2'(fc1^T(GELU'(pre) * fc2^T(dGout))), with the method's own gradients of the
        block in launch order.  top: _panels kwargs that restrict the block to the rows the head pools (frozen top layer), or {}."""
        w, d, C = self._w16, self._d, self.C
        B, T = sv["B"], self.Ts[i]
        M, m, st = B * T, self.names.mlp(i), ws["stat"][i]
        bb, pd_ = sv.get("bb") or (), sv.get("bdrop", 0.0)
        site, ln_site = self.method.bwd_linear_site, self.method.bwd_ln_site      # SSF's scale / shift gradients; no-ops elsewhere
        dy_ff = dGout
        if pd_ > 0:                                                          # gradient of dropout(fc2(.)): the forward's mask on dGout
            dy_ff = self._masked_grad(ws, dGout, pd_, SEED_LAYER + 8 * i + 3, bool(bb) or self.method.reads_masked_grad, M)
        if bb:                                                               # fc2: db = colsum(dGout), dW = dGout^T . act
            self._bb_linear_grads(ws, gv, bb, m + ".net.4", dy_ff, ws["dG16"], ws["sav"]["act"][i] if sv["wgrad"] else None, M, C, self.mlp,
                                  ldx=self.ldx if self.ldx != self.mlp else None)
        self.method.bwd_mlp_begin(self, ws, gv, i, dGout, M, B)              # DVPT: its latents' backward
        # fc2: dy = dGout, y = G[i+1] - G1[i] (behind a live dropout the stored difference is kept / (1 - p): masked gradient, y_mul = 1 - p)
        site(self, ws, gv, m, 2, dy_ff, ws["G"][i + 1], M, C, y1=ws["G1"][i], y_mul=1.0 - pd_)
        self._gemm(ws["dG16"], w[f"fc2{i}_t"], M, ws["dpre"], epilogue=ops.EPI_GELU_BWD_BF16, aux=ws["pre"][i], ldaux=self.ldx,
                   drop_p=pd_, seed=SEED_LAYER + 8 * i + 2, seed_ptr=ws["seed"], aux_is_grad=int(sv.get("pre_is_grad", False)), **top)
        site(self, ws, gv, m, 1, ws["dpre"], ws["pre"][i], M, self.mlp)      # fc1: dy = d(pre-activation), y = saved pre-activation
        if bb:                                                               # fc1: db = colsum(dpre), dW = dpre^T . LN2(G1)
            self._bb_linear_grads(ws, gv, bb, m + ".net.1", ws["dpre"], ws["dpre"], ws["sav"]["xn2"][i] if sv["wgrad"] else None, M, self.mlp, C)
        self._gemm(ws["dpre"], w[f"fc1{i}_t"], M, ws["dx16b"] if dy16 else ws["dx32"], epilogue=ops.EPI_STORE_BF16 if dy16 else ops.EPI_STORE_F32,
                   **top)
        self._mark(f"b{i}:fc1d")
        if bb:
            self._bb_ln_grads(ws, gv, bb, m + ".net.0", ws["dx32"], ws["G1"][i], st[2], st[3], M)
        ln_site(self, ws, gv, m, ".net.0", ws["dx32"], ws["G1"][i], st[2], st[3], M)
        if top:                                                              # the other rows of dG1 are dGout: zero, in one memset
            ops.memset_zero(dGin)
        ops.layernorm_bwd(ws["dx16b"] if dy16 else ws["dx32"], ws["G1"][i], st[2], st[3], d(m + ".net.0.weight"), M, C, dx=dGin, dres=dGout,
                          dx16=ws["dG16"] if self.method.ln2_leaves_operand else None,
                          rows=(B, sum(self._pool_rows()), T) if top else None)
        self.method.bwd_mlp_end(self, ws, gv, i, dGout, dGin, M, pd_)        # DVPT's scatter, AdaptFormer's backward: += dG1, refresh dG16

    def _attn_block_bwd(self, ws, sv, gv, i, dGin, dx, dy16, bot):
        """Main stream, attention block of layer i: dx = dGin + LN1'(qkv^T(attn'(out^T(dGin)))), with the method's own gradients of the block
        in launch order.  bot: _panels kwargs that restrict the qkv dgrad and LayerNorm 1 to the prompt rows (frozen bottom layer), or {}."""
        w, d, C = self._w16, self._d, self.C
        B, T = sv["B"], self.Ts[i]
        M, a, st = B * T, self.names.attn(i), ws["stat"][i]
        bb, pd_ = sv.get("bb") or (), sv.get("bdrop", 0.0)
        site, ln_site = self.method.bwd_linear_site, self.method.bwd_ln_site
        dy_at = dGin
        if pd_ > 0:                                                          # gradient of dropout(to_out(.))
            dy_at = self._masked_grad(ws, dGin, pd_, SEED_LAYER + 8 * i + 1, bool(bb) or self.method.reads_masked_grad, M)
        site(self, ws, gv, a, 2, dy_at, ws["G1"][i], M, C, y1=ws["G"][i], y_mul=1.0 - pd_)      # to_out: dy = dG1, y = G1[i] - G[i]
        if bb:                                                               # to_out: db = colsum(dG1), dW = dG1^T . ctx
            self._bb_linear_grads(ws, gv, bb, a + ".to_out.0", dy_at, ws["dG16"], ws["ctx"][i], M, C, C)
        self._gemm(ws["dG16"], w[f"out{i}_t"], M, ws["dctx"], epilogue=ops.EPI_STORE_BF16)
        self._mark(f"b{i}:outd")
        if self._relv is not None:
            self._relv_layer(ws, i, B, T)
        # (bottom layer of a frozen backbone: only dq / dk / dv of the prompt rows are read -- by the row-panel qkv dgrad below)
        ops.attention_bwd(ws["qkv"][i], ws["ctx"][i], ws["dctx"], ws["lse"][i], ws["delta"], ws["dqkv"], B, T, self.heads, 64 ** -0.5,
                          drop_p=pd_, seed=SEED_LAYER + 8 * i, seed_ptr=ws["seed"], q_prescaled=True, need_rows=self.P if bot else None)
        self._mark(f"b{i}:attnb")
        self.method.bwd_after_attention(self, ws, gv, i, M)                  # MeLO: the LoRA factors of a wrapped layer
        uq = {} if self.fp32 else dict(y0_cols=self.heads * 64, y0_mul=1.0 / self.q_scale)         # the saved q block is pre-scaled
        site(self, ws, gv, a, 1, ws["dqkv"], ws["qkv"][i], M, 3 * C, **uq)   # to_qkv: dy = dqkv, y = saved qkv
        if bb:                                                               # to_qkv (bias-free): dW = dqkv^T . LN1(G)
            self._bb_linear_grads(ws, gv, bb, a + ".to_qkv", None, ws["dqkv"], ws["sav"]["xn1"][i] if sv["wgrad"] else None, M, 3 * C, C)
        self._gemm(ws["dqkv"], w[f"qkv{i}_t"], M, ws["dx16b"] if dy16 else ws["dx32"], epilogue=ops.EPI_STORE_BF16 if dy16 else ops.EPI_STORE_F32,
                   **bot)
        if bb:
            self._bb_ln_grads(ws, gv, bb, a + ".norm", ws["dx32"], ws["G"][i], st[0], st[1], M)
        ln_site(self, ws, gv, a, ".norm", ws["dx32"], ws["G"][i], st[0], st[1], M)
        self._mark(f"b{i}:qkvd")
        proj = None
        if self._fuse_proj and i > 0:                                        # + dcomb = dx . W_up for the GPA core of layer i - 1
            pre_lo, _ = self._gpa_names(i - 1)
            proj = dict(w=d(pre_lo + ".proj_up.weight"), y=ws["bw"]["dcomb"], w_layout=1, L_=self.Lat)
        ops.layernorm_bwd(ws["dx16b"] if dy16 else ws["dx32"], ws["G"][i], st[0], st[1], d(a + ".norm.weight"), M, C, dx=dx, dres=dGin,
                          dx16=None if bot else ws["dG16"], rows=(B, self.P, T) if bot else None, proj=proj)

    def _grad_supported(self, name: str) -> bool:
        # head: always; backbone tensors: the classes whose backbone can train (plain ViT `linear` / `bitfit` / `fft`, AdaptFormer and Gaviko
        # with freeze_vit=False, ...: every kind but MeLO); everything else: the method's own tensors
        return name.startswith(self.names.head()) or self.method.backbone_trainable or self._own_grad_kernels(name)

    def _own_grad_kernels(self, name: str) -> bool:
        """The method's OWN trainable tensors (prompts, adapters, LoRA factors, ...): gradients from the method-specific kernels."""
        return self.method.owns(name)

    def _needs_backbone_backward(self) -> bool:
        return any(not n.startswith(self.names.head()) for n in self.trainable_names())
