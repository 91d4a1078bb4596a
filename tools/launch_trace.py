#!/usr/bin/env python3
"""What one step LAUNCHES, per method, as one record list per case -> tests/golden/launch_trace.json.

tools/engine_manifest.py pins the static facts of the engine; this pins the dynamic ones.  For each case below the model is built with
registry.build_model, moved to the device, and runs ONE eager training step (forward + backward) and ONE eval forward while
  * every call through gaviko_amd.lib.launch is recorded: the entry point, the ordinal of the stream it went to (order of first use in
    the case, 0 = the stream the step was issued on), every scalar argument and every pointer -- a tensor argument, or a pointer field
    of a descriptor passed with ctypes.byref / as a ctypes array, whose scalar fields are recorded beside it;
  * every cross-stream edge is recorded: Engine._ev_record / Engine._ev_wait, the only two places that issue one, with the stream and the
    ordinal of the event.
A pointer is named by what it points into: the path of the workspace slot, parameter, operand shadow, folded operand, EVP state entry or
flat gradient buffer whose storage holds the address, plus the byte offset; an address outside all of them by the ordinal of its first
appearance in the case.  Which argument is a pointer is read from lib.SIGNATURES and the descriptors' field types (a raw address such as
`x.data_ptr() + column offset` is one), and the naming is done when the case is over: every buffer the step allocated on its way then hangs
on the engine, and every tensor that reached a launch has been kept alive, so no address was used twice.  Addresses themselves never enter
a record, so two runs on one tree give identical records.
The tool wraps lib.launch, lib.ptr and the two engine methods from outside for the duration of a case; the product path is untouched.

The committed file holds, per case, the ordered (entry point, stream) list -- tandem repeats (the layers) folded to [count, block], blocks and
names stored once -- the SHA-256 of the full canonical record, and a 16-bit digest of every WINDOW consecutive records, which is how
tests/test_launch_trace_gpu.py names the first launch that differs without the file holding every argument.

Usage:  python tools/launch_trace.py [out.json]            (default: tests/golden/launch_trace.json)
        python tools/launch_trace.py --full out.json [case ...]   every record in full, for diffing two trees (keep it out of git)
"""
from __future__ import annotations

import bisect
import ctypes
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "launch_trace.json")
SEED = 20261021
WINDOW = 8                             # records per argument digest of the committed file


def _manifest_tool():
    spec = importlib.util.spec_from_file_location("engine_manifest", os.path.join(ROOT, "tools", "engine_manifest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_MT = _manifest_tool()
BASE, EXTRA, ENV_SWITCHES = _MT.BASE, _MT.EXTRA, _MT.ENV_SWITCHES

# (case name, method, overrides, B): the manifest tool's BASE configuration (vit-t16, 160x160x120, B = 2) -- every hook of every method runs
METHODS = ("gaviko", "linear", "fft", "bitfit", "adaptformer", "dvpt", "evp", "ssf", "melo", "deep_vpt", "shallow_vpt")
DROPOUT_METHODS = ("ssf", "adaptformer", "dvpt", "gaviko")
CASES = [(m, m, {}, 2) for m in METHODS]
# with the backbone frozen these four classes keep every nn.Dropout of it in eval (their train() overrides), so a step launches exactly what
# the plain case launches: the cases pin that the rates then reach no launch ...
CASES += [(m + "_dropout", m, dict(dropout=0.2, emb_dropout=0.1), 2) for m in DROPOUT_METHODS]
CASES += [(m + "_prompt_dropout", m, dict(prompt_dropout=0.1), 2) for m in ("deep_vpt", "shallow_vpt")]
# the backbone-gradient branches, EVP's dlocal, the SSF unfold
CASES += [(m + "_unfrozen", m, dict(freeze_vit=False), 2) for m in ("adaptformer", "evp", "ssf", "dvpt", "gaviko")]
# ... and unfrozen the same rates are LIVE: the masked gradients, AdaptFormer's operand refresh, SSF's y_mul = 1 - p, the embedding dropout
CASES += [(m + "_unfrozen_dropout", m, dict(freeze_vit=False, dropout=0.2, emb_dropout=0.1), 2) for m in DROPOUT_METHODS]
CASES += [("melo_layers", "melo", dict(alpha=8, lora_layer=[0, 5, 11]), 2),        # (alpha // r = 2: the gradient scaling launches too)
          ("gaviko_b16", "gaviko", dict(backbone="vit-b16"), 1)]                  # the folded first LayerNorm and the side-tile fusions
CASE_NAMES = [c[0] for c in CASES]

# descriptor fields that point at another HOST descriptor: followed, never named as an address
NESTED = {("gvk_ln_bwd_desc", "proj"): "gvk_rowproj_desc"}


class _Addr:
    """A device address inside a record, until Tracer.resolve names it."""
    __slots__ = ("addr",)

    def __init__(self, addr):
        self.addr = addr


class Tracer:
    """Records the launches and edges of one engine between start() and stop()."""

    def __init__(self, eng):
        from gaviko_amd import lib
        self.eng, self.lib = eng, lib
        self.records = []
        self.streams, self.events, self.unknown = {}, {}, {}
        self.alive = []                                      # tensors and events seen: their addresses / ids stay theirs
        self.starts, self.regions = [], []
        self.struct_names = {cls: name for name, cls in lib.STRUCTS.items()}

    # ---- naming
    def _roots(self):
        eng = self.eng
        yield "p", eng.p
        for key, ws in eng._wss.items():
            yield "ws(" + ",".join(str(k) for k in key[1:2] + key[3:]) + ")", ws
        yield "w16", eng._w16
        yield "fold", eng._fold
        yield "eff", eng._eff
        yield "evp", eng.__dict__.get("_evp")
        if eng._flat_grad is not None:
            yield "grad", eng._flat_grad["buf"]
        yield "ig", eng._ig_scratch

    def _walk(self, path, v, out):
        if isinstance(v, torch.Tensor):
            if v.is_cuda and v.numel():
                out.append((v.data_ptr(), v.data_ptr() + v.numel() * v.element_size(), path))
        elif isinstance(v, dict):
            for k, x in v.items():
                self._walk(f"{path}.{k}", x, out)
        elif isinstance(v, (list, tuple)):
            for k, x in enumerate(v):
                self._walk(f"{path}[{k}]", x, out)

    def rescan(self):
        """Disjoint address ranges of everything the engine holds, first root first (a parameter that is also its own fp32 operand, a
        gradient view of the flat buffer: the earlier name wins)."""
        found = []
        for name, root in self._roots():
            self._walk(name, root, found)
        self.starts, self.regions = [], []
        for lo, hi, path in found:
            k = bisect.bisect_right(self.starts, lo)
            if (k and self.regions[k - 1][1] > lo) or (k < len(self.starts) and self.starts[k] < hi):
                continue
            self.starts.insert(k, lo)
            self.regions.insert(k, (lo, hi, path))

    def _find(self, addr):
        k = bisect.bisect_right(self.starts, addr)
        if k and self.regions[k - 1][1] > addr:
            lo, _, path = self.regions[k - 1]
            return f"{path}+{addr - lo}"
        return None

    def resolve(self, v):
        """The records with every address replaced by its name: done once, when the case is over -- by then everything the step allocated
        on its way (operand shadows, the flat gradient buffer) hangs on the engine, and everything that reached a launch is still alive."""
        if isinstance(v, _Addr):
            got = self._find(v.addr)
            if got is None:
                got = self.unknown.setdefault(v.addr, f"#{len(self.unknown)}")
            return got
        if isinstance(v, dict):
            return {k: self.resolve(x) for k, x in v.items()}
        return [self.resolve(x) for x in v] if isinstance(v, list) else v

    def _stream(self, handle):
        return self.streams.setdefault(handle, len(self.streams))

    # ---- arguments
    def _struct(self, s):
        cname = self.struct_names.get(type(s), type(s).__name__)
        out = {"struct": cname}
        for f, ct in s._fields_:
            v = getattr(s, f)
            if ct is ctypes.c_void_p:
                nested = NESTED.get((cname, f))
                out[f] = self._struct(self.lib.STRUCTS[nested].from_address(v)) if (nested and v) else _Addr(v) if v else None
            else:
                out[f] = v
        return out

    def _arg(self, a, ctype):
        """One argument of an entry point whose declared type (lib.SIGNATURES) is `ctype`."""
        if ctype is ctypes.c_void_p:                          # a tensor, None, or a raw address (a column offset into a tensor)
            if isinstance(a, torch.Tensor):
                self.alive.append(a)
                a = a.data_ptr()
            return _Addr(a) if a else None
        if isinstance(a, ctypes.Array):
            return [self._struct(x) for x in a]
        obj = getattr(a, "_obj", None)                        # ctypes.byref(descriptor)
        if isinstance(obj, ctypes.Structure):
            return self._struct(obj)
        if a is None or isinstance(a, (bool, int, float)):
            return a
        raise TypeError(f"launch_trace: an argument of type {type(a).__name__} reached lib.launch")

    # ---- the wrappers
    def start(self):
        from gaviko_amd.engine import Engine
        tr, lib, real = self, self.lib, self.lib.launch
        self._saved = (real, lib.ptr, Engine._ev_record, Engine._ev_wait)
        self._stream(torch.cuda.current_stream().cuda_stream)

        class Launch:
            def __getattr__(self, fn):
                call = getattr(real, fn)

                def traced(*args):
                    tr.records.append({"fn": fn, "stream": tr._stream(torch.cuda.current_stream().cuda_stream),
                                       "args": [tr._arg(a, t) for a, t in zip(args, lib.SIGNATURES[fn])]})
                    return call(*args)
                return traced

        def ptr(t):
            if t is not None:
                tr.alive.append(t)
            return tr._saved[1](t)

        def ev_record(eng, stream):
            ev = tr._saved[2](eng, stream)
            if ev is not None:
                tr.alive.append(ev)
                tr.records.append({"fn": "ev_record", "stream": tr._stream(stream.cuda_stream), "event": tr.events.setdefault(id(ev), len(tr.events))})
            return ev

        def ev_wait(eng, stream, ev):
            if ev is not None:
                tr.records.append({"fn": "ev_wait", "stream": tr._stream(stream.cuda_stream), "event": tr.events.setdefault(id(ev), len(tr.events))})
            return tr._saved[3](eng, stream, ev)

        lib.launch, lib.ptr, Engine._ev_record, Engine._ev_wait = Launch(), ptr, ev_record, ev_wait

    def mark(self, what):
        self.records.append({"fn": "phase:" + what, "stream": 0})

    def stop(self):
        """Unwraps; -> the records, addresses named."""
        from gaviko_amd.engine import Engine
        self.lib.launch, self.lib.ptr, Engine._ev_record, Engine._ev_wait = self._saved
        self.rescan()
        records = self.resolve(self.records)
        self.alive = []
        return records


def trace_case(method, over, B, device="cuda:0"):
    """The records of one eager training step and one eval forward of a fresh model."""
    from gaviko_amd.registry import build_model
    from gaviko_amd.utils import synth
    torch.manual_seed(SEED)
    dev = torch.device(device)
    model = build_model(dict(BASE, method=method, **dict(EXTRA[method], **over)))
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    model.to(dev)
    x = torch.from_numpy(synth.volumes(0, B)).to(dev)
    y = torch.from_numpy(synth.labels(0, B)).to(dev)
    tr = Tracer(model._engine())
    tr.start()
    try:
        model.train()
        tr.mark("train")
        torch.nn.functional.cross_entropy(model(x), y).backward()
        model.eval()
        tr.mark("eval")
        with torch.no_grad():
            model(x)
        torch.cuda.synchronize()
    finally:
        records = tr.stop()
    return records


def generate(names=None):
    """{case name: [record]} with the engine's environment switches at their defaults."""
    saved = {k: os.environ.pop(k) for k in ENV_SWITCHES if k in os.environ}
    try:
        return {name: trace_case(method, over, B) for name, method, over, B in CASES if names is None or name in names}
    finally:
        os.environ.update(saved)


# ---- the committed form
def _dump(v):
    return json.dumps(v, separators=(",", ":"))


def canonical(records):
    return _dump(records).encode()


def order(records):
    """The ordered (entry point, stream) list as 'entry@stream' strings."""
    return [f"{r['fn']}@{r['stream']}" for r in records]


def digests(records):
    return "".join(hashlib.sha256(canonical(records[k: k + WINDOW])).hexdigest()[:4] for k in range(0, len(records), WINDOW))


def fold_repeats(seq, max_period=600):
    """[a, b, c, b, c, d] -> [a, [2, [b, c]], d]: at every position the tandem repeat that covers the most items is folded."""
    out, i, n = [], 0, len(seq)
    while i < n:
        best = (0, 0, 0)                                     # (items covered, period, count)
        for p in range(1, min(max_period, (n - i) // 2) + 1):
            if seq[i] != seq[i + p]:
                continue
            c = 1
            while seq[i + c * p: i + (c + 1) * p] == seq[i: i + p]:
                c += 1
            if c >= 2 and c * p > best[0]:
                best = (c * p, p, c)
        if best[0] >= 4:
            out.append([best[2], fold_repeats(seq[i: i + best[1]], max_period)])
            i += best[0]
        else:
            out.append(seq[i])
            i += 1
    return out


def unfold_repeats(folded):
    out = []
    for x in folded:
        if isinstance(x, list):
            out += unfold_repeats(x[1]) * x[0]
        else:
            out.append(x)
    return out


def summary(records):
    return {"n": len(records), "order": order(records), "sha256": hashlib.sha256(canonical(records)).hexdigest(), "digests": digests(records)}


def pack(summaries):
    """File form of {case: summary(records)}: names once ('names', referred to by index), repeats folded, and every folded block of
    20 characters or more that occurs more than once stored once under 'blocks' and referred to as '@<n>'."""
    names = sorted({s for c in summaries.values() for s in c["order"]})
    idx = {s: k for k, s in enumerate(names)}
    cases = {name: dict(c, order=fold_repeats([idx[s] for s in c["order"]])) for name, c in summaries.items()}
    seen = {}

    def count(v):
        for x in v:
            if isinstance(x, list):
                count(x[1])
                seen[_dump(x[1])] = seen.get(_dump(x[1]), 0) + 1

    for c in cases.values():
        count(c["order"])
    blocks, ids = {}, {}

    def fold(v):
        out = []
        for x in v:
            if isinstance(x, list):
                key, inner = _dump(x[1]), fold(x[1])
                if len(key) >= 20 and seen[key] > 1:
                    if key not in ids:
                        ids[key] = f"@{len(ids)}"
                        blocks[ids[key]] = inner
                    inner = ids[key]
                out.append([x[0], inner])
            else:
                out.append(x)
        return out

    return {"window": WINDOW, "names": names, "blocks": blocks, "cases": {name: dict(c, order=fold(c["order"])) for name, c in cases.items()}}


def unpack(packed):
    """pack() undone: {case: summary}."""
    names, blocks = packed["names"], packed["blocks"]

    def un(v):
        return [[x[0], un(blocks[x[1]] if isinstance(x[1], str) else x[1])] if isinstance(x, list) else x for x in v]

    return {name: dict(c, order=[names[k] for k in unfold_repeats(un(c["order"]))]) for name, c in packed["cases"].items()}


def first_difference(got, want):
    """None, or a sentence naming the first launch at which summary `got` departs from the committed summary `want`."""
    for k, (a, b) in enumerate(zip(got["order"], want["order"])):
        if a != b:
            return f"launch {k}: {a} where the committed trace has {b} (after {got['order'][max(0, k - 3): k]})"
    if got["n"] != want["n"]:
        k = min(got["n"], want["n"])
        return f"{got['n']} launches, the committed trace has {want['n']}; the first one without a partner is {(got['order'] + want['order'])[k]} at {k}"
    for k in range(0, len(want["digests"]), 4):
        if got["digests"][k: k + 4] != want["digests"][k: k + 4]:
            lo = k // 4 * WINDOW
            return (f"same entry points and streams, but the arguments of launches {lo}..{lo + WINDOW - 1} differ "
                    f"({got['order'][lo: lo + WINDOW]}); `tools/launch_trace.py --full` on both trees shows the argument")
    return None if got["sha256"] == want["sha256"] else "the full records differ in a way the window digests do not show"


def write(packed, path):
    with open(path, "w") as f:
        f.write('{"window":%d,\n"names":%s,\n"blocks":{\n' % (packed["window"], _dump(packed["names"])))
        f.write(",\n".join(f"{_dump(k)}:{_dump(v)}" for k, v in packed["blocks"].items()) + '\n},\n"cases":{\n')
        f.write(",\n".join(f"{_dump(k)}:{_dump(v)}" for k, v in packed["cases"].items()) + "\n}}\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv and argv[0] == "--full":
        recs = generate(set(argv[2:]) or None)
        with open(argv[1], "w") as f:
            f.write("{\n" + ",\n".join(_dump(k) + ":[\n" + ",\n".join(_dump(r) for r in v) + "\n]" for k, v in recs.items()) + "\n}\n")
        print(f"wrote {argv[1]} ({os.path.getsize(argv[1])} bytes, {len(recs)} cases)")
    else:
        out = argv[0] if argv else OUT
        write(pack({k: summary(v) for k, v in generate().items()}), out)
        print(f"wrote {out} ({os.path.getsize(out)} bytes, {len(CASES)} cases)")
