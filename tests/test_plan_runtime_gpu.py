"""-m gpu: the launch-plan runtime (csrc/runtime.hip) and the fill / copy kernels, called directly through the library.

Every hot-path step runs twice eagerly and then as a replayed plan, so what is checked here is the contract the engine relies on:
a recording pass executes, a replay is exactly one more eager pass through the same pointers, calls that return early record
nothing, every misuse is refused with -2 and a message naming the entry point, and the event edges order streams at replay time.

Every expected value is an integer, a byte pattern or a power-of-two multiple of a float in [1, 2): all comparisons are torch.equal,
there are no tolerances.  The reference of a recorded sequence is the same Python function issued eagerly, the same number of
times, on clones of the buffers.  Every recording is ended or aborted in a `finally`; only plans created here are freed.
"""
import ctypes
import math
import os
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64                       # guard bytes on each side of a fill / copy region (keeps the region 16-byte aligned)
FILL = 0xA5                      # what guards and destinations are prefilled with
CAP = 2048 * 256 * 16            # bytes one pass of the capped grid covers: 2048 blocks x 256 threads x 16 bytes
SIZES = [4, 8, 12, 16, 20, 28, 4096, 4096 + 12, 256 * 16 + 4, CAP, CAP + 16, CAP + 3 * 256 * 16 + 12]
FAR = 1 << 30                    # a plan / event id far beyond any that exists


@pytest.fixture(scope="module")
def lib(dev):
    from gaviko_amd import lib as L
    return L.load()


def _err(lib):
    return lib.gvk_last_error().decode()


def _refused(lib, rc, name, text=None):
    assert rc == -2, f"{name}: expected a refusal (-2), got {rc}"
    msg = _err(lib)
    assert name + ":" in msg, f"the message does not name {name}: {msg!r}"
    if text is not None:
        assert text in msg, msg


def _guarded(dev, n):
    """A byte buffer of GUARD + n + GUARD bytes, all FILL; returns (buffer, pointer to the region)."""
    buf = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + GUARD


def _guards_intact(buf, n):
    g = torch.full((GUARD,), FILL, dtype=torch.uint8, device=buf.device)
    return torch.equal(buf[:GUARD], g) and torch.equal(buf[GUARD + n:], g)


def _all_fill(buf):
    return torch.equal(buf, torch.full_like(buf, FILL))


def _ramp(dev, n, seed):
    """n floats in [1, 2): any power-of-two multiple of them (within range) is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    return (1.0 + torch.rand(n, generator=g)).to(dev)


def _cur():
    return torch.cuda.current_stream().cuda_stream


class _Recording:
    """`with _Recording(lib) as r:` begins a plan; leaving the block ends it (r.pid) or, after an exception, aborts it."""

    def __init__(self, lib):
        self.lib, self.pid = lib, None

    def __enter__(self):
        assert self.lib.gvk_plan_begin() == 0, _err(self.lib)
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:
            self.lib.gvk_plan_abort()
            return False
        self.pid = self.lib.gvk_plan_end()
        assert self.pid >= 0, _err(self.lib)
        return False


# ---------------------------------------------------------------------------------------------------------------------
# fill and copy kernels: a 16-byte vector body, a tail of up to 3 words, a grid capped at 2048 blocks with a stride loop
@pytest.mark.parametrize("n", SIZES)
def test_fill_is_bit_exact_and_stays_inside(dev, lib, n):
    for value in (0, 0x5A, 0xFF, 0x1FF, 0x100, -1):
        buf, p = _guarded(dev, n)
        assert lib.gvk_memset_async(p, value, n, _cur()) == 0, _err(lib)
        torch.cuda.synchronize()
        want = torch.full((n,), value & 0xFF, dtype=torch.uint8, device=dev)      # only the low byte counts
        got = buf[GUARD:GUARD + n]
        if not torch.equal(got, want):
            bad = (got != want).nonzero().flatten()
            raise AssertionError(f"fill of {n} bytes with {value:#x}: {bad.numel()} wrong bytes, first at {int(bad[0])}, last at {int(bad[-1])}")
        assert _guards_intact(buf, n), f"fill of {n} bytes with {value:#x} wrote outside the region"


@pytest.mark.parametrize("n", SIZES)
def test_copy_is_bit_exact_and_stays_inside(dev, lib, n):
    g = torch.Generator().manual_seed(n)
    src = torch.randint(-2 ** 31, 2 ** 31, (n // 4,), generator=g, dtype=torch.int64).to(torch.int32).to(dev)
    src0 = src.clone()
    buf, p = _guarded(dev, n)
    assert lib.gvk_copy_async(p, src.data_ptr(), n, _cur()) == 0, _err(lib)
    torch.cuda.synchronize()
    got = buf[GUARD:GUARD + n].view(torch.int32)
    if not torch.equal(got, src0):
        bad = (got != src0).nonzero().flatten()
        raise AssertionError(f"copy of {n} bytes: {bad.numel()} wrong words, first at {int(bad[0])}, last at {int(bad[-1])}")
    assert _guards_intact(buf, n), f"copy of {n} bytes wrote outside the region"
    assert torch.equal(src, src0), "the copy changed its source"


def test_ops_copy_into_a_larger_destination(dev):
    from gaviko_amd import ops
    n = 4 * 256 * 3 + 3                                     # whole vectors for more than one block, then a 3-word tail
    src = _ramp(dev, n, 11)
    src0 = src.clone()
    dst = torch.full((n + 37,), -3.0, device=dev)
    ops.copy_(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst[:n], src0)
    assert torch.equal(dst[n:], torch.full((37,), -3.0, device=dev)), "copy_ wrote past src.numel() elements"
    assert torch.equal(src, src0)


def test_fill_and_copy_refusals(dev, lib):
    from gaviko_amd import ops
    from gaviko_amd.lib import GavikoHipError
    buf, p = _guarded(dev, 64)
    src = torch.arange(16, dtype=torch.int32, device=dev)
    s = src.data_ptr()
    _refused(lib, lib.gvk_memset_async(p + 4, 0, 16, _cur()), "gvk_memset_async")       # pointer off by one word
    _refused(lib, lib.gvk_memset_async(p, 0, 6, _cur()), "gvk_memset_async")            # size no multiple of 4
    _refused(lib, lib.gvk_memset_async(None, 0, 16, _cur()), "gvk_memset_async")        # null pointer, bytes > 0
    _refused(lib, lib.gvk_copy_async(p + 4, s, 16, _cur()), "gvk_copy_async")
    _refused(lib, lib.gvk_copy_async(p, s + 4, 16, _cur()), "gvk_copy_async")
    _refused(lib, lib.gvk_copy_async(p, s, 6, _cur()), "gvk_copy_async")
    _refused(lib, lib.gvk_copy_async(None, s, 16, _cur()), "gvk_copy_async")
    _refused(lib, lib.gvk_copy_async(p, None, 16, _cur()), "gvk_copy_async")
    assert lib.gvk_memset_async(None, 0, 0, _cur()) == 0                               # nothing to do: fine even with null pointers
    assert lib.gvk_copy_async(None, None, 0, _cur()) == 0
    assert lib.gvk_memset_async(p + 4, 0, 0, _cur()) == 0
    odd = torch.full((7,), 1.5, dtype=torch.bfloat16, device=dev)                      # 14 bytes
    with pytest.raises(GavikoHipError, match="gvk_memset_async"):
        ops.memset_zero(odd)
    torch.cuda.synchronize()
    assert _all_fill(buf), "a refused call wrote to its destination"
    assert torch.equal(odd, torch.full_like(odd, 1.5))
    assert torch.equal(src, torch.arange(16, dtype=torch.int32, device=dev))


# ---------------------------------------------------------------------------------------------------------------------
# record and replay
N = 1000                         # floats of the recorded step's vector: four blocks of the scale kernel, the last one partial


class _Step:
    """The buffers of one small step and the step itself: x *= 2; word += 7919; y = 0; z = x."""

    def __init__(self, dev, seed=1):
        self.x = _ramp(dev, N, seed)
        self.word = torch.full((1,), 20261004, dtype=torch.int64, device=dev)
        self.y = torch.full((24,), 9, dtype=torch.int32, device=dev)
        self.z = torch.full((N,), -1.0, device=dev)

    def clone(self):
        c = object.__new__(_Step)
        c.x, c.word, c.y, c.z = self.x.clone(), self.word.clone(), self.y.clone(), self.z.clone()
        return c

    def run(self, lib):
        st = _cur()
        assert lib.gvk_scale_f32(self.x.data_ptr(), 2.0, N, st) == 0, _err(lib)
        assert lib.gvk_seed_advance(self.word.data_ptr(), 7919, st) == 0, _err(lib)
        assert lib.gvk_memset_async(self.y.data_ptr(), 0, self.y.numel() * 4, st) == 0, _err(lib)
        assert lib.gvk_copy_async(self.z.data_ptr(), self.x.data_ptr(), N * 4, st) == 0, _err(lib)

    def same(self, other):
        torch.cuda.synchronize()
        return [k for k in ("x", "word", "y", "z") if not torch.equal(getattr(self, k), getattr(other, k))]


def test_recording_executes_and_a_replay_is_one_more_eager_pass(dev, lib):
    s = _Step(dev)
    ref = s.clone()
    torch.cuda.synchronize()
    with _Recording(lib) as r:
        s.run(lib)
    ref.run(lib)
    assert s.same(ref) == [], "the recording pass did not do what one eager pass does"
    assert int(s.word) == 20261004 + 7919 and torch.equal(s.y, torch.zeros_like(s.y))      # (the eager reference is not vacuous)
    assert lib.gvk_plan_size(r.pid) == 4
    k = 3
    for _ in range(k):
        assert lib.gvk_plan_replay(r.pid) == 0, _err(lib)
        ref.run(lib)
    assert s.same(ref) == [], f"{k} replays after the recording differ from {k + 1} eager passes"
    assert int(s.word) == 20261004 + (k + 1) * 7919
    torch.cuda.synchronize()
    assert lib.gvk_plan_free(r.pid) == 0


def test_arguments_are_frozen_and_memory_is_live(dev, lib):
    s = _Step(dev)
    torch.cuda.synchronize()
    with _Recording(lib) as r:
        s.run(lib)
    assert lib.gvk_plan_replay(r.pid) == 0, _err(lib)
    fresh = _ramp(dev, N, 77)
    s.x.copy_(fresh)                                         # new contents, same pointers
    s.y.fill_(5)
    s.z.fill_(-2.0)
    s.word.fill_(100)
    ref = s.clone()
    torch.cuda.synchronize()
    assert lib.gvk_plan_replay(r.pid) == 0, _err(lib)
    ref.run(lib)
    assert s.same(ref) == [], "a replay did not act on the current contents of its buffers"
    assert torch.equal(s.x, fresh * 2) and torch.equal(s.z, fresh * 2) and int(s.word) == 100 + 7919
    assert torch.equal(s.y, torch.zeros_like(s.y))
    assert lib.gvk_plan_free(r.pid) == 0


def test_calls_that_return_early_record_nothing(dev, lib):
    x = _ramp(dev, N, 3)
    x0 = x.clone()
    buf, p = _guarded(dev, 64)
    src = torch.arange(16, dtype=torch.int32, device=dev)
    sp = src.data_ptr()
    torch.cuda.synchronize()
    st = _cur()
    with _Recording(lib) as r:
        assert lib.gvk_scale_f32(x.data_ptr(), 2.0, N, st) == 0, _err(lib)                # the one real launch
        assert lib.gvk_scale_f32(x.data_ptr(), 2.0, 0, st) == 0
        assert lib.gvk_memset_async(p, 0, 0, st) == 0
        assert lib.gvk_copy_async(p, sp, 0, st) == 0
        assert lib.gvk_memset_async(p + 4, 0, 16, st) == -2
        assert lib.gvk_memset_async(p, 0, 6, st) == -2
        assert lib.gvk_memset_async(None, 0, 16, st) == -2
        assert lib.gvk_copy_async(p + 4, sp, 16, st) == -2
        assert lib.gvk_copy_async(p, sp + 4, 16, st) == -2
        assert lib.gvk_copy_async(p, sp, 6, st) == -2
        assert lib.gvk_copy_async(None, sp, 16, st) == -2
        assert lib.gvk_copy_async(p, None, 16, st) == -2
    assert lib.gvk_plan_size(r.pid) == 1
    torch.cuda.synchronize()
    assert torch.equal(x, x0 * 2) and _all_fill(buf)
    assert lib.gvk_plan_replay(r.pid) == 0, _err(lib)
    torch.cuda.synchronize()
    assert torch.equal(x, x0 * 4) and _all_fill(buf)
    assert torch.equal(src, torch.arange(16, dtype=torch.int32, device=dev))
    assert lib.gvk_plan_free(r.pid) == 0


def test_abort_keeps_what_ran_and_consumes_no_id(dev, lib):
    x = _ramp(dev, N, 4)
    x0 = x.clone()
    torch.cuda.synchronize()
    st = _cur()
    with _Recording(lib) as first:
        assert lib.gvk_scale_f32(x.data_ptr(), 2.0, N, st) == 0, _err(lib)
    assert lib.gvk_plan_begin() == 0, _err(lib)
    try:
        assert lib.gvk_scale_f32(x.data_ptr(), 2.0, N, st) == 0, _err(lib)
    finally:
        assert lib.gvk_plan_abort() == 0
    torch.cuda.synchronize()
    assert torch.equal(x, x0 * 4), "the launches made before the abort did not run"
    _refused(lib, lib.gvk_plan_end(), "gvk_plan_end")                                     # the aborted recording is gone
    with _Recording(lib) as second:                                                       # ... and a new one can begin
        assert lib.gvk_scale_f32(x.data_ptr(), 2.0, N, st) == 0, _err(lib)
    assert second.pid == first.pid + 1, "the aborted recording consumed a plan id"
    assert lib.gvk_plan_size(second.pid) == 1
    assert lib.gvk_plan_abort() == 0                                                      # nothing recording: still 0
    assert lib.gvk_plan_replay(first.pid) == 0 and lib.gvk_plan_replay(second.pid) == 0, _err(lib)
    torch.cuda.synchronize()
    assert torch.equal(x, x0 * 32)
    assert lib.gvk_plan_free(first.pid) == 0 and lib.gvk_plan_free(second.pid) == 0


def test_free_retires_one_plan_and_its_id(dev, lib):
    xa, xb = _ramp(dev, N, 5), _ramp(dev, N, 6)
    a0, b0 = xa.clone(), xb.clone()
    torch.cuda.synchronize()
    st = _cur()
    with _Recording(lib) as a:
        assert lib.gvk_plan_event_record(st) == 0, _err(lib)
        assert lib.gvk_scale_f32(xa.data_ptr(), 2.0, N, st) == 0, _err(lib)
    with _Recording(lib) as b:
        assert lib.gvk_scale_f32(xb.data_ptr(), 0.5, N, st) == 0, _err(lib)
    assert lib.gvk_plan_event_stream_wait(a.pid, 0, st) == 0, _err(lib)                   # valid while the plan exists
    torch.cuda.synchronize()
    assert lib.gvk_plan_free(a.pid) == 0, _err(lib)
    ms = ctypes.c_float(-1.0)
    gone = "no such plan"
    _refused(lib, lib.gvk_plan_size(a.pid), "gvk_plan_size", gone)
    _refused(lib, lib.gvk_plan_replay(a.pid), "gvk_plan_replay", gone)
    _refused(lib, lib.gvk_plan_free(a.pid), "gvk_plan_free", gone)
    _refused(lib, lib.gvk_plan_event_stream_wait(a.pid, 0, st), "gvk_plan_event_stream_wait", gone)
    _refused(lib, lib.gvk_plan_event_elapsed(a.pid, 0, 0, ctypes.byref(ms)), "gvk_plan_event_elapsed", gone)
    assert lib.gvk_plan_size(b.pid) == 1
    assert lib.gvk_plan_replay(b.pid) == 0, _err(lib)
    with _Recording(lib) as c:
        assert lib.gvk_scale_f32(xb.data_ptr(), 0.5, N, st) == 0, _err(lib)
    assert c.pid == b.pid + 1 and c.pid != a.pid, "a freed plan's id was handed out again"
    _refused(lib, lib.gvk_plan_size(a.pid), "gvk_plan_size", gone)
    torch.cuda.synchronize()
    assert torch.equal(xa, a0 * 2), "a refused replay of a freed plan launched something"
    assert torch.equal(xb, b0 * 0.125)
    assert lib.gvk_plan_free(b.pid) == 0 and lib.gvk_plan_free(c.pid) == 0


def test_refusal_table(dev, lib):
    x = _ramp(dev, N, 7)
    x0 = x.clone()
    torch.cuda.synchronize()
    st = _cur()
    ms = ctypes.c_float(-1.0)
    with _Recording(lib) as good:
        assert lib.gvk_plan_event_record(st) == 0, _err(lib)
        assert lib.gvk_scale_f32(x.data_ptr(), 2.0, N, st) == 0, _err(lib)
    # outside a recording
    _refused(lib, lib.gvk_plan_end(), "gvk_plan_end")
    _refused(lib, lib.gvk_plan_event_record(st), "gvk_plan_event_record")
    _refused(lib, lib.gvk_plan_event_record_fenced(st), "gvk_plan_event_record_fenced")
    _refused(lib, lib.gvk_plan_event_wait(st, 0), "gvk_plan_event_wait")
    for bad in (-1, FAR):
        _refused(lib, lib.gvk_plan_replay(bad), "gvk_plan_replay", "no such plan")
        _refused(lib, lib.gvk_plan_size(bad), "gvk_plan_size", "no such plan")
        _refused(lib, lib.gvk_plan_free(bad), "gvk_plan_free", "no such plan")
        _refused(lib, lib.gvk_plan_event_stream_wait(bad, 0, st), "gvk_plan_event_stream_wait", "no such plan")
        _refused(lib, lib.gvk_plan_event_elapsed(bad, 0, 0, ctypes.byref(ms)), "gvk_plan_event_elapsed", "no such plan")
    for bad in (-1, 1, FAR):                                                              # the plan has exactly one event, id 0
        _refused(lib, lib.gvk_plan_event_stream_wait(good.pid, bad, st), "gvk_plan_event_stream_wait", "no such event")
        _refused(lib, lib.gvk_plan_event_elapsed(good.pid, bad, 0, ctypes.byref(ms)), "gvk_plan_event_elapsed")
        _refused(lib, lib.gvk_plan_event_elapsed(good.pid, 0, bad, ctypes.byref(ms)), "gvk_plan_event_elapsed")
    _refused(lib, lib.gvk_plan_event_elapsed(good.pid, 0, 0, None), "gvk_plan_event_elapsed")
    assert ms.value == -1.0
    # inside a recording
    with _Recording(lib) as r:
        _refused(lib, lib.gvk_plan_begin(), "gvk_plan_begin")
        _refused(lib, lib.gvk_plan_replay(good.pid), "gvk_plan_replay")
        _refused(lib, lib.gvk_plan_event_wait(st, 0), "gvk_plan_event_wait", "no such event")     # no event exists yet
        assert lib.gvk_plan_event_record(st) == 0, _err(lib)
        _refused(lib, lib.gvk_plan_event_wait(st, -1), "gvk_plan_event_wait", "no such event")
        _refused(lib, lib.gvk_plan_event_wait(st, 1), "gvk_plan_event_wait", "no such event")
    assert lib.gvk_plan_size(r.pid) == 1, "a refused call was recorded"
    assert lib.gvk_plan_size(good.pid) == 2
    torch.cuda.synchronize()
    assert torch.equal(x, x0 * 2), "a refused call launched something"
    assert lib.gvk_plan_free(good.pid) == 0 and lib.gvk_plan_free(r.pid) == 0


# ---------------------------------------------------------------------------------------------------------------------
# cross-stream ordering: a fork-join over two streams, replayed back to back
CHAIN = 32                       # producer launches alternating x2 / x0.5 (plus one more x2: the net of a pass is x2)
BIG = 4 << 20                    # floats of the producer's buffer: 16 MiB
TAIL = 1024                      # floats the consumer copies: the last 4 KiB


@pytest.mark.parametrize("which", ["record", "record_fenced"])
def test_event_edges_order_the_streams_at_replay(dev, lib, which):
    record = {"record": lib.gvk_plan_event_record, "record_fenced": lib.gvk_plan_event_record_fenced}[which]
    s0, s1, s2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    p0, p1, p2 = s0.cuda_stream, s1.cuda_stream, s2.cuda_stream
    a = _ramp(dev, BIG, 8)
    a0 = a.clone()
    b = torch.full((TAIL,), -1.0, device=dev)
    c = torch.full((BIG,), -1.0, device=dev)
    tail_ptr = a.data_ptr() + (BIG - TAIL) * 4
    torch.cuda.synchronize()
    with _Recording(lib) as r:
        e0 = record(p0)
        assert lib.gvk_plan_event_wait(p1, e0) == 0, _err(lib)
        for i in range(CHAIN + 1):
            assert lib.gvk_scale_f32(a.data_ptr(), 2.0 if i % 2 == 0 else 0.5, BIG, p1) == 0, _err(lib)
        e1 = record(p1)
        assert lib.gvk_plan_event_wait(p0, e1) == 0, _err(lib)
        assert lib.gvk_copy_async(b.data_ptr(), tail_ptr, TAIL * 4, p0) == 0, _err(lib)
    assert (e0, e1) == (0, 1), _err(lib)
    assert lib.gvk_plan_size(r.pid) == (CHAIN + 1) + 1 + 2 + 2                            # launches + 2 records + 2 waits
    # no host synchronisation from here to the end of the replays: e1 keeps each consumer behind its producer, and e0 keeps the
    # producer of replay n+1 behind the consumer of replay n
    for _ in range(5):
        assert lib.gvk_plan_replay(r.pid) == 0, _err(lib)
    # a stream that is no part of the plan waits for e1 of the last replay
    assert lib.gvk_plan_event_stream_wait(r.pid, e1, p2) == 0, _err(lib)
    assert lib.gvk_copy_async(c.data_ptr(), a.data_ptr(), BIG * 4, p2) == 0, _err(lib)
    torch.cuda.synchronize()
    want = a0 * 64.0                                                                      # the recording pass and five replays
    assert torch.equal(a, want)
    assert torch.equal(b, want[BIG - TAIL:]), "the consumer did not wait for its producer (stale tail)"
    assert torch.equal(c, want), "gvk_plan_event_stream_wait did not order the outside stream behind the last replay"
    with _Recording(lib) as nxt:                                                          # event ids restart in every plan
        assert record(p0) == 0, _err(lib)
    assert lib.gvk_plan_free(r.pid) == 0 and lib.gvk_plan_free(nxt.pid) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the timing pair
def _timed_chain(dev, lib, x):
    st = _cur()
    with _Recording(lib) as r:
        assert lib.gvk_plan_event_record(st) == 0, _err(lib)
        for alpha in (2.0, 0.5, 2.0, 0.5):
            assert lib.gvk_scale_f32(x.data_ptr(), alpha, N, st) == 0, _err(lib)
        assert lib.gvk_plan_event_record(st) == 1, _err(lib)
    assert lib.gvk_plan_replay(r.pid) == 0, _err(lib)
    torch.cuda.synchronize()
    return r.pid


def test_timed_plan_reports_an_elapsed_time(dev, lib):
    x = _ramp(dev, N, 9)
    x0 = x.clone()
    torch.cuda.synchronize()
    try:
        assert lib.gvk_plan_set_timing(1) == 0
        pid = _timed_chain(dev, lib, x)
    finally:
        assert lib.gvk_plan_set_timing(0) == 0
    ms = ctypes.c_float(float("nan"))
    assert lib.gvk_plan_event_elapsed(pid, 0, 1, ctypes.byref(ms)) == 0, _err(lib)
    assert math.isfinite(ms.value) and ms.value >= 0.0, ms.value
    assert torch.equal(x, x0)
    assert lib.gvk_plan_free(pid) == 0


def test_untimed_plan_refuses_the_query_and_leaves_no_stale_error(dev, lib):
    """The refusal is a host-side API error (hipEventElapsedTime on events without timestamps); the HIP runtime keeps such an error
    until somebody reads it, and check_launch reads it after every kernel launch: the library has to drain it on the refusing path,
    or the next, perfectly good, call reports 'launch failed'."""
    if os.environ.get("GAVIKO_HIP_PLAN_TIMING") is not None:
        pytest.skip("GAVIKO_HIP_PLAN_TIMING is set: every plan event carries timestamps")
    x = _ramp(dev, N, 10)
    x0 = x.clone()
    torch.cuda.synchronize()
    assert lib.gvk_plan_set_timing(0) == 0
    pid = _timed_chain(dev, lib, x)
    ms = ctypes.c_float(-1.0)
    assert lib.gvk_plan_event_elapsed(pid, 0, 1, ctypes.byref(ms)) == -1
    assert "GAVIKO_HIP_PLAN_TIMING" in _err(lib), _err(lib)
    rc = lib.gvk_scale_f32(x.data_ptr(), 2.0, N, _cur())
    assert rc == 0, f"the call after a refused timing query failed (rc={rc}): {_err(lib)}"
    torch.cuda.synchronize()
    assert torch.equal(x, x0 * 2)
    assert lib.gvk_plan_free(pid) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the recording state belongs to the thread that called gvk_plan_begin
def test_recording_is_per_thread(dev, lib):
    x = _ramp(dev, N, 12)
    x0 = x.clone()
    y = _ramp(dev, N, 13)
    y0 = y.clone()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    go, launched, ended, done = (threading.Event() for _ in range(4))
    out = {}

    def other():
        try:
            if not go.wait(60):
                return
            out["end"] = lib.gvk_plan_end()                  # this thread is not recording
            out["end_msg"] = _err(lib)
            out["launch"] = [lib.gvk_scale_f32(y.data_ptr(), 2.0, N, side.cuda_stream) for _ in range(3)]
            side.synchronize()
            launched.set()
            if not ended.wait(60):
                return
            out["replay"] = lib.gvk_plan_replay(out["pid"])
            out["replay_msg"] = _err(lib)
            torch.cuda.synchronize()
        except BaseException as e:                           # reported by the main thread
            out["error"] = e
        finally:
            launched.set()
            done.set()

    t = threading.Thread(target=other)
    t.start()
    st = _cur()
    try:
        with _Recording(lib) as r:
            assert lib.gvk_scale_f32(x.data_ptr(), 2.0, N, st) == 0, _err(lib)
            go.set()
            assert launched.wait(60), "the second thread did not answer"
            assert lib.gvk_scale_f32(x.data_ptr(), 2.0, N, st) == 0, _err(lib)
        out["pid"] = r.pid
        torch.cuda.synchronize()
    finally:
        go.set()
        ended.set()
        done.wait(60)
        t.join(60)
    assert not t.is_alive()
    assert "error" not in out, out.get("error")
    assert out["end"] == -2 and "gvk_plan_end:" in out["end_msg"], "the second thread saw the main thread's recording"
    assert out["launch"] == [0, 0, 0]
    assert lib.gvk_plan_size(r.pid) == 2, "launches of another thread were recorded into this thread's plan"
    assert out["replay"] == 0, out["replay_msg"]
    assert torch.equal(x, x0 * 16), "a plan replayed from another thread is not one more pass"
    assert torch.equal(y, y0 * 8), "the second thread's own launches did not run exactly once each"
    assert lib.gvk_plan_free(r.pid) == 0
