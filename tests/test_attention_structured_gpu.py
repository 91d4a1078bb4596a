"""-m gpu: every form of the attention kernels on the structured inputs of tests/attention_ref.py, compared per element with the float64
reference (|got - want| <= r 2^-9 |want| + floor; the roundings r, the measured floors and the fp32 bounds are listed there).  The selector
inputs turn any key, query, head, batch or 16-byte chunk read from the wrong place into an error of 1/(g+1) of a value; the offset inputs
put the scores hundreds to thousands of log2 units away from zero.  tests/test_attention_structured.py shows on the CPU that the comparison
refuses each such fault.  Every line printed ends in the worst err / tolerance of the case and the largest error on the elements whose
reference is below the floor, so a later change of the kernels can see how much room it has."""
import functools

import pytest
import torch

import attention_ref as ar

pytestmark = pytest.mark.gpu

CASES = [(B, T, H, kind) for B, T, H in ar.SHAPES for kind in ar.SELECTOR_KINDS + ar.OFFSET_KINDS]
F32_CASES = [(B, T, H, kind) for B, T, H in ar.SHAPES for kind in ar.SELECTOR_KINDS + ar.F32_OFFSET_KINDS]
GRADS = ("dq", "dk", "dv")
case_params = pytest.mark.parametrize("B,T,H,kind", CASES, ids=lambda v: str(v))


@functools.lru_cache(maxsize=None)
def _case(kind, B, T, H):
    """one input set and its float64 reference per (kind, B, T, H) and module; nothing changes it afterwards"""
    cs = ar.make_case(kind, B, T, H)
    cs.ref = ar.autograd_reference(cs)
    q, k, v = cs.qkv()
    full = ar.attend(q, k, v, cs.d_o())
    cs.P, cs.dP, cs.s = full["P"], full["dP"], cs.smax()
    return cs


def _heads(x, cs):
    """[pad(B*T), n*inner] -> n tensors [B,H,T,64]"""
    x = x[: cs.B * cs.T].double().cpu().reshape(cs.B, cs.T, -1, cs.H, 64)
    return [x[:, :, i].permute(0, 2, 1, 3) for i in range(x.shape[2])]


def _guarded(cs, dev):
    """f32 [B,H,T] as the head of a NaN-filled buffer: entries past the sequence must stay NaN"""
    n = cs.B * cs.H * cs.T
    buf = torch.full((n + 4096,), float("nan"), device=dev)
    return buf, buf[:n].view(cs.B, cs.H, cs.T)


def _forward(cs, dev):
    from gaviko_amd import ops
    Q = cs.op.to(dev)
    O = torch.full((cs.rows, cs.inner), ar.SENTINEL, dtype=torch.bfloat16, device=dev)
    buf, lse = _guarded(cs, dev)
    ops.attention_fwd(Q, O, lse, cs.B, cs.T, cs.H, 0.125, q_prescaled=True)
    torch.cuda.synchronize()
    assert bool((O[cs.B * cs.T:] == ar.SENTINEL).all()), "forward stored a row past the sequence"
    assert bool(torch.isnan(buf[lse.numel():]).all()), "forward stored an lse past the sequence"
    return Q, O, lse


def _check(tag, pairs):
    """pairs: (name, got, want, ratio); prints (in brackets the least floor that would pass), then asserts every ratio <= 1"""
    line = ", ".join(f"{n} {r:.3f}" + (f" [{ar.excess(g, w, ar.R[n]):.2e}]" if n in ar.R else "") for n, g, w, r in pairs)
    print(f"{tag}: err/tol {line}")
    for n, _, _, r in pairs:
        assert r <= 1.0, f"{tag} {n}: worst err / tolerance {r:.3f}"


@case_params
def test_forward_every_key_tile(dev, monkeypatch, B, T, H, kind):
    """launcher's choice, 96-key and 128-key tiles.  On the selector inputs lse is also held against its closed form, 128 ln 2 + ln(size)."""
    cs = _case(kind, B, T, H)
    for kb in (None, 96, 128):
        if kb is None:
            monkeypatch.delenv("GAVIKO_HIP_ATTN_KB", raising=False)
        else:
            monkeypatch.setenv("GAVIKO_HIP_ATTN_KB", str(kb))
        _, O, lse = _forward(cs, dev)
        got = _heads(O, cs)[0]
        pairs = [("O", got, cs.ref["O"], ar.ratio(got, cs.ref["O"], ar.R["O"], ar.floors(kind)["O"])),
                 ("lse", lse, cs.ref["lse"], ar.ratio_lse(lse.cpu(), cs.ref["lse"], T))]
        if kind in ar.SELECTOR_KINDS:
            closed = 128 * ar.LN2 + torch.log(cs.size.double())
            pairs.append(("lse-closed", lse, closed, ar.ratio_lse(lse.cpu(), closed, T)))
        _check(f"fwd {kind} B={B} T={T} H={H} kb={kb}", pairs)


def _backward(cs, dev, Q, O, lse, ws=None, need_rows=None):
    from gaviko_amd import ops
    DO = cs.dout.to(dev)
    DQ = torch.full((cs.rows, 3 * cs.inner), ar.SENTINEL, dtype=torch.bfloat16, device=dev)
    buf, delta = _guarded(cs, dev)
    ops.attention_bwd(Q, O, DO, lse, delta, DQ, cs.B, cs.T, cs.H, 0.125, q_prescaled=True, ws=ws, need_rows=need_rows)
    torch.cuda.synchronize()
    assert bool((DQ[cs.B * cs.T:] == ar.SENTINEL).all()), "backward stored a row past the sequence"
    assert bool(torch.isnan(buf[delta.numel():]).all()), "backward stored a delta past the sequence"
    return DQ, delta


def _grad_pairs(cs, DQ, delta, rows=None):
    rows = cs.T if rows is None else rows
    fl = ar.floors(cs.kind)
    pairs = [("delta", delta, cs.ref["delta"], ar.ratio(delta.cpu(), cs.ref["delta"], ar.R["delta"], fl["delta"]))]
    for name, got in zip(GRADS, _heads(DQ, cs)):
        got, want = got[:, :, :rows], cs.ref[name][:, :, :rows]
        pairs.append((name, got, want, ar.ratio(got, want, ar.R[name], fl[name])))
    return pairs


def _forward_for_backward(cs, dev, monkeypatch):
    monkeypatch.delenv("GAVIKO_HIP_ATTN_KB", raising=False)
    Q, O, lse = _forward(cs, dev)
    O[cs.B * cs.T:] = cs.out_pad[cs.B * cs.T:].to(dev)                 # the padding rows of the backward's inputs hold values, not zeros
    return Q, O, lse


@case_params
def test_backward_two_pass_and_one_pass(dev, monkeypatch, B, T, H, kind):
    """two-pass kernels at the launcher's tile, 96 and 128; the one-pass kernel with its workspace: no bounded wait hit, every progress word
    back at zero, bit-equal on repetition"""
    from gaviko_amd import ops
    cs = _case(kind, B, T, H)
    Q, O, lse = _forward_for_backward(cs, dev, monkeypatch)
    for kb in (0, 96, 128):
        if kb:
            monkeypatch.setenv("GAVIKO_HIP_ATTN_KB", str(kb))
        DQ, delta = _backward(cs, dev, Q, O, lse)
        _check(f"bwd {kind} B={B} T={T} H={H} kb={kb}", _grad_pairs(cs, DQ, delta))
    monkeypatch.delenv("GAVIKO_HIP_ATTN_KB", raising=False)
    ws = ops.attention_bwd_workspace(B, T, H, dev)
    st = int(ops.L.load().gvk_attention_bwd_status_offset(ws.numel() * 4)) // 4
    DQ, delta = _backward(cs, dev, Q, O, lse, ws=ws)
    assert ops.attention_bwd_timeouts(ws) == 0 and int(ws[:st].abs().max()) == 0
    _check(f"bwd {kind} B={B} T={T} H={H} one-pass", _grad_pairs(cs, DQ, delta))
    again, delta2 = _backward(cs, dev, Q, O, lse, ws=ws)
    assert torch.equal(again.view(torch.int16), DQ.view(torch.int16)) and torch.equal(delta2, delta)
    assert ops.attention_bwd_timeouts(ws) == 0 and int(ws[:st].abs().max()) == 0


@case_params
def test_backward_first_rows(dev, monkeypatch, B, T, H, kind):
    """gvk_attention_desc.need_rows on the two-pass kernels.  The contract (gaviko_hip.h; both kernels leave by whole 128-row workgroups):
    dq, dk, dv of every row below need_rows rounded up to 128 carry the full call's values -- all of them are compared per element, not
    only the rows below need_rows -- every row from there on is left alone, delta is complete."""
    cs = _case(kind, B, T, H)
    Q, O, lse = _forward_for_backward(cs, dev, monkeypatch)
    for need in sorted({min(n, T) for n in (1, 8, 33, T)}):
        DQ, delta = _backward(cs, dev, Q, O, lse, need_rows=need)
        keep = (need + 127) // 128 * 128
        _check(f"bwd {kind} B={B} T={T} H={H} need_rows={need}", _grad_pairs(cs, DQ, delta, rows=min(keep, T)))
        assert bool((DQ[: B * T].view(B, T, -1)[:, keep:] == ar.SENTINEL).all())


@case_params
def test_colsum_and_gradcolsum_windows(dev, B, T, H, kind):
    """integer weights 1..4 (7 outside the window: never read), windows that start and end on, and one off, every 32-row edge.  On the
    selector inputs colsum is a sum of w over a group divided by its size."""
    from gaviko_amd import ops
    cs = _case(kind, B, T, H)
    Q, DO = cs.op.to(dev), cs.dout.to(dev)
    lse32 = cs.ref["lse"].float().to(dev).contiguous()
    g = torch.Generator().manual_seed(300 + T)
    wint = torch.randint(1, 5, (B, T), generator=g).double()
    worst, over = [0.0, 0.0], [-1.0, -1.0]
    for q0, q1 in ar.windows(T):
        w = torch.full((B, T), 7.0)
        w[:, q0:q1] = wint[:, q0:q1].float()
        w = w.to(dev)
        bufc, outc = _guarded(cs, dev)
        bufg, outg = _guarded(cs, dev)
        ops.attention_colsum(Q, lse32, w, outc, B, T, H, q0=q0, q1=q1)
        ops.attention_gradcolsum(Q, lse32, DO, w, outg, B, T, H, q0=q0, q1=q1)
        torch.cuda.synchronize()
        assert bool(torch.isnan(bufc[outc.numel():]).all()) and bool(torch.isnan(bufg[outg.numel():]).all())
        wantc, wantg = ar.colsum_ref(cs.P, wint, q0, q1), ar.gradcolsum_ref(cs.P, cs.dP, wint, q0, q1)
        rc, rg = ar.ratio32(outc.cpu(), wantc, cs.s, T), ar.ratio32(outg.cpu(), wantg, cs.s, T)
        worst = [max(worst[0], rc), max(worst[1], rg)]
        over = [max(over[0], ar.excess32(outc, wantc, cs.s, T)), max(over[1], ar.excess32(outg, wantg, cs.s, T))]
        if rc > 1.0 or rg > 1.0:
            print(f"maps {kind} B={B} T={T} H={H} rows [{q0}, {q1}): colsum {rc:.3f} [{over[0]:.2e}], gradcolsum {rg:.3f} [{over[1]:.2e}]")
        assert rc <= 1.0 and rg <= 1.0, f"maps {kind} B={B} T={T} H={H} rows [{q0}, {q1}): colsum {rc:.3f}, gradcolsum {rg:.3f}"
    print(f"maps {kind} B={B} T={T} H={H}: err/tol colsum {worst[0]:.3f} [{over[0]:.2e}], gradcolsum {worst[1]:.3f} [{over[1]:.2e}] "
          f"over {len(ar.windows(T))} windows")


@pytest.mark.parametrize("B,T,H,kind", F32_CASES, ids=lambda v: str(v))
def test_fp32_path(dev, B, T, H, kind):
    """attention_f32.hip on the same inputs as fp32 operands with the raw q (the reference attends over those fp32 values)"""
    from gaviko_amd import ops
    cs = _case(kind, B, T, H)
    flat32 = cs.exact_flat().float()
    ref = ar.autograd_reference(cs, flat32.double())
    Q = flat32[: B * T].to(dev).contiguous()
    DO = cs.dout[: B * T].float().to(dev).contiguous()
    O = torch.full((B * T, cs.inner), ar.SENTINEL, device=dev)
    DQ = torch.full((B * T, 3 * cs.inner), ar.SENTINEL, device=dev)
    buf, lse = _guarded(cs, dev)
    bufd, delta = _guarded(cs, dev)
    ops.attention_fwd(Q, O, lse, B, T, H, 0.125)
    ops.attention_bwd(Q, O, DO, lse, delta, DQ, B, T, H, 0.125)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[lse.numel():]).all()) and bool(torch.isnan(bufd[delta.numel():]).all())
    got = _heads(O, cs)[0]
    fl = ar.floors_f32(kind)
    pairs = [("O", got, ref["O"], ar.ratio32(got, ref["O"], cs.s, T, fl["O"])), ("lse", lse, ref["lse"], ar.ratio_lse(lse.cpu(), ref["lse"], T))]
    for name, got in zip(GRADS, _heads(DQ, cs)):
        pairs.append((name, got, ref[name], ar.ratio32(got, ref[name], cs.s, T, fl[name])))
    line = ", ".join(f"{n} {r:.3f}" + (f" [{ar.excess32(g, w, cs.s, T):.2e}]" if n in fl else "") for n, g, w, r in pairs)
    print(f"f32 {kind} B={B} T={T} H={H}: err/tol {line}")
    for n, _, _, r in pairs:
        assert r <= 1.0, f"f32 {kind} B={B} T={T} H={H} {n}: worst err / tolerance {r:.3f}"
