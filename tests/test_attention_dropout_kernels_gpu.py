"""-m gpu: the dropout instantiations of the attention kernels, element by element, in both precisions.

bf16: attn_fwd_kernel<96|128, true>, attn_bwd_dq_kernel<96, true>, attn_bwd_dkdv_kernel<96, true>; fp32: attn_f32_fwd_kernel<true>,
attn_f32_bwd_dq_kernel<true>, attn_f32_bwd_kv_kernel<true>.  Each of them recomputes the mask word hash(key(seed, b*H + head), query*T + key)
on its own, so each gets a read-out of its own.

1. Mask read-out (drop_p = 0.5).  With the q block at 0 every score is 0, P = 1/T exactly and lse = ln T, whatever K holds.  One-hot
   operands then turn 64 columns of the mask per launch into the output itself:
     forward  v[k, :] = e_(k-64j) in key block j                        ->  out[q, d] = M[q, 64j+d] / T
     dV       dO[q, :] = e_(q-64j) in query block j                     ->  dV[k, d]  = M[64j+d, k] / T
     dQ       v[:, 0] = 1, dO[:, 0] = 1, k[k, :] = e_(k-64j) in block j ->  dQ[q, d]  = (scale/T) (M[q, 64j+d] - delta_q),
              delta_q = inv_keep * (kept fraction of row q): kept elements are positive, dropped ones negative; with every row's kept
              fraction in [0.2, 0.8] (asserted on the host mask) both signs stay 0.4 scale/T away from zero.
   A dropped position is exactly 0, a kept one inv_keep/T within 2 % (bf16: one rounding of P.M and one of the result, 2^-9 each) or
   1e-5 (fp32); the recovered mask equals tests/dropmask.py's for every (b, head, query, key), and the two precisions recover the same.
   Shapes: the tile edges (T = 1, 31, 97, 129, 200, 257) and (2,97,12), where B*H = 24 puts a second sample behind twelve heads.

2. Peaked operands (test_attention_bwd's: uniform +-2, seeds 61 / 62; drop_p = 0.1) against float64 autograd over exactly the values the
   device operands represent, with the host mask.  Bounds relative to the reference's own maximum, the non-dropout tests' numbers:
   bf16 out 1.5e-2, lse 2e-3, dq / dk / dv 2.5e-2 each; fp32 those of test_attention_f32_fwd_bwd.  The seed pair is (0, 2^40 + 5):
   measured on the float64 reference alone, before any launch.  Relative errors measured on the MI355X (max |err| / |ref|max):

     bf16 (B,T,H)   out      lse      dq       dk       dv       | the non-dropout kernels, same operands: out, dq, dk, dv
     (2,97,2)       4.26e-03 6.99e-07 4.45e-03 3.84e-03 3.54e-03 | 2.51e-03 3.80e-03 3.24e-03 3.36e-03
     (1,200,3)      3.44e-03 7.94e-07 3.72e-03 3.51e-03 3.47e-03 | 3.38e-03 3.79e-03 3.64e-03 3.49e-03
     (1,31,1)       3.25e-03 5.29e-07 3.71e-03 2.62e-03 3.22e-03 | 2.53e-03 3.31e-03 2.55e-03 3.45e-03
     (2,129,12)     3.48e-03 8.72e-07 3.95e-03 4.20e-03 2.79e-03 | 4.15e-03 4.26e-03 3.62e-03 2.80e-03
     fp32
     (2,97,2)       7.06e-07 6.66e-07 8.59e-07 7.07e-07 6.68e-07 | 7.67e-07 8.08e-07 9.09e-07 6.26e-07
     (1,200,3)      7.77e-07 7.72e-07 1.11e-06 8.02e-07 6.41e-07 | 7.23e-07 8.85e-07 6.95e-07 6.37e-07
     (1,31,1)       6.85e-07 6.60e-07 5.63e-07 4.84e-07 6.53e-07 | 6.30e-07 5.40e-07 5.16e-07 6.89e-07
     (2,129,12)     6.56e-07 7.93e-07 6.32e-07 6.40e-07 6.14e-07 | 7.43e-07 7.76e-07 6.45e-07 6.80e-07
   (the dropout kernels are as exact as the plain ones: every bound holds with a factor of 3 or more to spare.)  The dQ read-out's
   magnitudes came out within 7.7e-3 of the float64 value in bf16 (bound 5 %) and within 6e-7 in fp32 (bound 1e-5).

   test_bounds_discriminate (CPU, no launch) recomputes the reference under three corrupted masks -- (a) keys, (b) queries from
   96 floor((T-1)/96) on and (c) the last (b, head) drawn from seed + 1 -- and asserts that each moves the output and every gradient
   block by at least 3x the bf16 bound.  Ratios difference / bound, smallest over out, dq, dk, dv:
     (2,97,2): a 7.9 b 8.8 c 21.4    (1,200,3): a 11.5 b 8.0 c 21.8    (1,31,1): 14.5 (a = b = c)    (2,129,12): a 21.6 b 20.9 c 9.8
   (With the seed pair (31, 2024) corruption (b) moves dv at (2,97,2) by 2.8x only, which is why that pair is not the one used here.)

3. ops.attention_bwd's precedence (drop_p > 0 wins over need_rows and ws), drop_p = 0 with a seed supplied, and repeatability.
"""
import math

import pytest
import torch

import dropmask

pytestmark = pytest.mark.gpu

SCALE = 0.125
ATTN_C = SCALE * 1.4426950408889634      # what the q block of the bf16 operand carries: q * scale * log2(e)
SEEDS = [(31, 2024), (0, 2 ** 40 + 5), (7, -3)]          # (descriptor seed, device word); the last two: high-half fold, wraparound of seed + word
SEED_IDS = ["31+2024", "0+2^40+5", "7-3"]
# the tile edges, and (2, 97, 12): B*H = 24, a second sample at H = 12 (b*H + head for b >= 1, bh = 12..23)
READ_SHAPES = [(1, 1, 1), (1, 31, 1), (2, 97, 2), (1, 129, 12), (2, 200, 3), (1, 257, 2), (2, 97, 12)]
READ_P = 0.5
PEAK_SHAPES = [(2, 97, 2), (1, 200, 3), (1, 31, 1), (2, 129, 12)]
PEAK_P = 0.1
# test_bounds_discriminate's 3x margin depends on this pair ((31, 2024) reaches 2.8x only): re-run that test, which needs no device, when
# changing it
PEAK_SEED = (0, 2 ** 40 + 5)
BF16_OUT_TOL, BF16_GRAD_TOL, LSE_TOL = 1.5e-2, 2.5e-2, 2e-3      # test_attention_fwd / test_attention_bwd


@pytest.fixture(scope="module")
def dev():
    from gaviko_amd import lib
    lib.require_device()
    return torch.device("cuda:0")


def _word(dev, value):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _dtype(prec):
    return torch.bfloat16 if prec == "bf16" else torch.float32


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


def _bf(x):
    return x.float().to(torch.bfloat16).double()


def _to_dev(dev, prec, x, rows):
    """float64 [.., cols] -> padded device matrix of the precision's type (the values are representable: no rounding happens here)"""
    from gaviko_amd import ops
    x = x.reshape(rows, -1)
    buf = ops.act_zeros(rows, x.shape[1], _dtype(prec), dev)
    buf[:rows] = x.to(dev).to(_dtype(prec))
    return buf


def _fwd(dev, prec, Q, B, T, H, p, seed, word):
    from gaviko_amd import ops
    O = ops.act_zeros(B * T, H * 64, _dtype(prec), dev)
    lse = torch.full((B, H, T), float("nan"), device=dev)
    ops.attention_fwd(Q, O, lse, B, T, H, SCALE, drop_p=p, seed=seed, seed_ptr=word, q_prescaled=True)
    return O, lse


def _bwd(dev, prec, Q, O, DO, lse, B, T, H, p, seed, word, **kw):
    from gaviko_amd import ops
    DQ = ops.act_zeros(B * T, 3 * H * 64, _dtype(prec), dev)
    delta = torch.full((B, H, T), float("nan"), device=dev)
    ops.attention_bwd(Q, O, DO, lse, delta, DQ, B, T, H, SCALE, drop_p=p, seed=seed, seed_ptr=word, q_prescaled=True, **kw)
    return DQ, delta


def _heads(x, B, T, H):
    """device [pad(B*T), H*64] -> float64 [B, H, T, 64] on the host"""
    return x[: B * T].cpu().double().view(B, T, H, 64).permute(0, 2, 1, 3)


def _grads(DQ, B, T, H):
    """device dqkv -> (dq, dk, dv), each float64 [B, H, T, 64]"""
    g = DQ[: B * T].cpu().double().view(B, T, 3, H, 64)
    return tuple(g[:, :, i].permute(0, 2, 1, 3) for i in range(3))


# ---------------------------------------------------------------------------------------------------------------- 1. mask read-out
def _host_mask(seed, word, B, T, H, p):
    return torch.from_numpy(dropmask.attn_mask(seed + word, B, H, T, p))          # [B, H, T, T], 0 or inv_keep


def _one_hot_block(B, T, H, j):
    """[B, T, H*64]: row 64j + i of every (b, head) is e_i (i < 64, 64j + i < T), every other row 0; and the number of such rows"""
    n = min(64, T - 64 * j)
    x = torch.zeros(B, T, H, 64, dtype=torch.float64)
    i = torch.arange(n)
    x[:, 64 * j + i, :, i] = 1.0
    return x.reshape(B, T, H * 64), n


def _kept(vals, want, rtol, what):
    """every value is exactly 0 (dropped) or `want` within rtol (kept); returns the kept flags"""
    zero = vals == 0
    near = (vals - want).abs() <= rtol * want
    bad = ~(zero | near)
    assert not bad.any(), f"{what}: {int(bad.sum())} values are neither 0 nor {want:.6g} within {rtol}: e.g. {vals[bad][:4].tolist()}"
    return ~zero


def _readout_qkv(B, T, H, k=None, v=None):
    """q block 0; k, v float64 [B, T, H*64] (default: bf16-representable noise -- with q = 0 the scores do not see K)"""
    inner = H * 64
    qkv = torch.zeros(B, T, 3 * inner, dtype=torch.float64)
    qkv[..., inner:2 * inner] = _bf(_rand((B, T, inner), 71)) if k is None else k
    qkv[..., 2 * inner:] = _bf(_rand((B, T, inner), 72)) if v is None else v
    return qkv


_RTOL = {"bf16": 2e-2, "f32": 1e-5}


def _read_fwd(dev, monkeypatch, prec, kb, B, T, H, seed, word):
    """the mask the forward applied, [B, H, T, T] bool (kb: the key tile forced on the bf16 kernel; fp32 has one form, kb = 0)"""
    if kb:
        monkeypatch.setenv("GAVIKO_HIP_ATTN_KB", str(kb))
    w = _word(dev, word)
    rec = torch.zeros(B, H, T, T, dtype=torch.bool)
    keep = float(dropmask.inv_keep(READ_P)) / T
    for j in range((T + 63) // 64):
        v, n = _one_hot_block(B, T, H, j)
        O, lse = _fwd(dev, prec, _to_dev(dev, prec, _readout_qkv(B, T, H, v=v), B * T), B, T, H, READ_P, seed, w)
        o = _heads(O, B, T, H)
        assert (o[..., n:] == 0).all(), f"forward {prec} pass {j}: columns past the last key are not 0"
        rec[..., 64 * j:64 * j + n] = _kept(o[..., :n], keep, _RTOL[prec], f"forward {prec} kb={kb} pass {j}")
        lse_err = (lse.cpu().double() - math.log(T)).abs().max().item()          # (NaN where the kernel wrote nothing)
        assert lse_err < LSE_TOL, f"forward {prec} pass {j}: |lse - ln T| = {lse_err:.2e} (the statistics are those of the undropped scores)"
    return rec


def _bwd_inputs(dev, prec, B, T, H, seed, w):
    """forward at q = 0 with v[:, 0] = 1 (the other columns noise): out[q, 0] = inv_keep * kept fraction of row q, lse = ln T -- for any K"""
    v = _bf(_rand((B, T, H * 64), 72)).view(B, T, H, 64)
    v[..., 0] = 1.0
    v = v.reshape(B, T, H * 64)
    O, lse = _fwd(dev, prec, _to_dev(dev, prec, _readout_qkv(B, T, H, v=v), B * T), B, T, H, READ_P, seed, w)
    return v, O, lse


def _read_dv(dev, prec, B, T, H, seed, word):
    """the mask as the dK/dV pass indexes it, [B, H, T(query), T(key)] bool"""
    w = _word(dev, word)
    rec = torch.zeros(B, H, T, T, dtype=torch.bool)
    keep = float(dropmask.inv_keep(READ_P)) / T
    v, O, lse = _bwd_inputs(dev, prec, B, T, H, seed, w)
    Q = _to_dev(dev, prec, _readout_qkv(B, T, H, v=v), B * T)
    for j in range((T + 63) // 64):
        dO, n = _one_hot_block(B, T, H, j)
        DQ, _ = _bwd(dev, prec, Q, O, _to_dev(dev, prec, dO, B * T), lse, B, T, H, READ_P, seed, w)
        _, dk, dv = _grads(DQ, B, T, H)
        assert (dk == 0).all(), f"dK {prec} pass {j}: not 0 although q = 0"
        assert (dv[..., n:] == 0).all(), f"dV {prec} pass {j}: columns past the last query are not 0"
        rec[:, :, 64 * j:64 * j + n, :] = _kept(dv[..., :n], keep, _RTOL[prec], f"dV {prec} pass {j}").transpose(-1, -2)
    return rec


def _read_dq(dev, prec, B, T, H, seed, word):
    """dQ / (scale/T) = M[q, key] - delta_q as the dQ pass computed it, float64 [B, H, T, T] (T = 1: nothing to read, dK = 0 is asserted)"""
    w = _word(dev, word)
    val = torch.zeros(B, H, T, T, dtype=torch.float64)
    v, O, lse = _bwd_inputs(dev, prec, B, T, H, seed, w)
    dO = torch.zeros(B, T, H, 64, dtype=torch.float64)
    dO[..., 0] = 1.0
    DO = _to_dev(dev, prec, dO, B * T)
    for j in range((T + 63) // 64):
        k, n = _one_hot_block(B, T, H, j)
        DQ, _ = _bwd(dev, prec, _to_dev(dev, prec, _readout_qkv(B, T, H, k=k, v=v), B * T), O, DO, lse, B, T, H, READ_P, seed, w)
        dq, dk, _ = _grads(DQ, B, T, H)
        assert (dk == 0).all(), f"dK {prec} pass {j}: not 0 although q = 0"
        assert (dq[..., n:] == 0).all(), f"dQ {prec} pass {j}: columns past the last key are not 0"
        val[..., 64 * j:64 * j + n] = dq[..., :n] * (T / SCALE)
    return val


def _assert_mask(rec, host, what):
    diff = rec != (host > 0)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.numel()} mask elements differ from the host mask, first at (b, head, q, k) = " \
                           f"{diff.nonzero()[0].tolist()}"


@pytest.mark.parametrize("seed,word", SEEDS, ids=SEED_IDS)
@pytest.mark.parametrize("B,T,H", READ_SHAPES)
@pytest.mark.parametrize("prec,kb", [("bf16", 96), ("bf16", 128), ("f32", 0)])
def test_mask_readout_forward(dev, monkeypatch, prec, kb, B, T, H, seed, word):
    _assert_mask(_read_fwd(dev, monkeypatch, prec, kb, B, T, H, seed, word), _host_mask(seed, word, B, T, H, READ_P), f"forward {prec} kb={kb}")


@pytest.mark.parametrize("seed,word", SEEDS, ids=SEED_IDS)
@pytest.mark.parametrize("B,T,H", READ_SHAPES)
@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_mask_readout_dv(dev, prec, B, T, H, seed, word):
    _assert_mask(_read_dv(dev, prec, B, T, H, seed, word), _host_mask(seed, word, B, T, H, READ_P), f"dK/dV pass {prec}")


@pytest.mark.parametrize("seed,word", SEEDS, ids=SEED_IDS)
@pytest.mark.parametrize("B,T,H", READ_SHAPES)
@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_mask_readout_dq(dev, prec, B, T, H, seed, word):
    host = _host_mask(seed, word, B, T, H, READ_P).double()
    frac = (host > 0).double().mean(-1)
    if T > 1:           # the condition of the read-out, on the host mask, before anything is launched
        assert 0.2 <= frac.min().item() and frac.max().item() <= 0.8, "a row's kept fraction leaves [0.2, 0.8]: choose another seed"
    val = _read_dq(dev, prec, B, T, H, seed, word)
    if T == 1:          # M - delta = M - M: nothing to read (dK = 0 was asserted inside)
        return
    assert (val != 0).all()
    _assert_mask(val > 0, host, f"dQ pass {prec}")
    want = host - float(dropmask.inv_keep(READ_P)) * frac[..., None]
    rel = ((val - want).abs() / want.abs()).max().item()
    print(f"attention_dropout dq read-out {prec} B={B} T={T} H={H}: magnitude rel err {rel:.2e}")
    assert rel <= (5e-2 if prec == "bf16" else 1e-5)


@pytest.mark.parametrize("seed,word", SEEDS, ids=SEED_IDS)
@pytest.mark.parametrize("B,T,H", READ_SHAPES)
def test_both_precisions_drop_the_same_elements(dev, monkeypatch, B, T, H, seed, word):
    """attention_desc.hpp: "both precisions take the same constants, so they drop the same elements" -- the same seed, seed_ptr and drop_p"""
    assert torch.equal(_read_fwd(dev, monkeypatch, "bf16", 96, B, T, H, seed, word), _read_fwd(dev, monkeypatch, "f32", 0, B, T, H, seed, word))
    assert torch.equal(_read_dv(dev, "bf16", B, T, H, seed, word), _read_dv(dev, "f32", B, T, H, seed, word))
    if T > 1:
        assert torch.equal(_read_dq(dev, "bf16", B, T, H, seed, word) > 0, _read_dq(dev, "f32", B, T, H, seed, word) > 0)


# ------------------------------------------------------------------------------------------------- 2. peaked operands against float64
def _reference(exact, dO, mask, B, T, H):
    """float64: out [B, T, inner], lse [B, H, T], d(out . dO) / d qkv [B, T, 3*inner] of attention with the scale mask on the probabilities"""
    qkv = exact.clone().requires_grad_(True)
    q, k, v = (t.reshape(B, T, H, 64).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
    s = q @ k.transpose(-1, -2) * SCALE
    o = ((s.softmax(-1) * mask) @ v).permute(0, 2, 1, 3).reshape(B, T, H * 64)
    o.backward(dO)
    return o.detach(), torch.logsumexp(s.detach(), -1), qkv.grad


_peaked_refs = {}       # operands and float64 reference per (precision, shape): a pure function of the key, read-only


def _peaked(prec, B, T, H):
    """test_attention_bwd's operands.  bf16: q block pre-scaled with ONE rounding, the reference over exactly the q, k, v those values
    represent; fp32: the same values rounded to fp32, q unscaled.  Computed once per (precision, shape), never modified."""
    key = (prec, B, T, H)
    if key not in _peaked_refs:
        inner = H * 64
        op = _rand((B, T, 3 * inner), 61, 2.0)
        op[..., :inner] *= ATTN_C
        op = op.bfloat16().double()
        exact = op.clone()
        exact[..., :inner] /= ATTN_C
        if prec == "f32":
            op = exact = exact.float().double()
        dO = _bf(_rand((B, T, inner), 62, 1.0))
        mask = _host_mask(*PEAK_SEED, B, T, H, PEAK_P).double()
        out, lse, grad = _reference(exact, dO, mask, B, T, H)
        _peaked_refs[key] = dict(op=op, exact=exact, dO=dO, mask=mask, out=out, lse=lse, grad=grad)
    return _peaked_refs[key]


def _blocks(g, inner):
    return (("dq", g[..., :inner]), ("dk", g[..., inner:2 * inner]), ("dv", g[..., 2 * inner:]))


def _run_peaked(dev, prec, B, T, H, p=PEAK_P, seed=PEAK_SEED[0], **kw):
    """forward and backward of the peaked operands on the device: (out, lse, dqkv, delta) device tensors"""
    r = _peaked(prec, B, T, H)
    w = _word(dev, PEAK_SEED[1])
    Q, DO = _to_dev(dev, prec, r["op"], B * T), _to_dev(dev, prec, r["dO"], B * T)
    O, lse = _fwd(dev, prec, Q, B, T, H, p, seed, w)
    DQ, delta = _bwd(dev, prec, Q, O, DO, lse, B, T, H, p, seed, w, **kw)
    return O, lse, DQ, delta


def _rel(got, want):
    return (got - want).abs().max().item() / want.abs().max().item()


@pytest.mark.parametrize("B,T,H", PEAK_SHAPES)
def test_peaked_bf16(dev, B, T, H):
    r, inner = _peaked("bf16", B, T, H), H * 64
    O, lse, DQ, _ = _run_peaked(dev, "bf16", B, T, H)
    errs = {"out": _rel(O[: B * T].cpu().double().view(B, T, inner), r["out"]), "lse": (lse.cpu().double() - r["lse"]).abs().max().item()}
    got = DQ[: B * T].cpu().double().view(B, T, 3 * inner)
    for (name, g), (_, w) in zip(_blocks(got, inner), _blocks(r["grad"], inner)):
        errs[name] = _rel(g, w)
    print(f"attention_dropout bf16 B={B} T={T} H={H}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["out"] <= BF16_OUT_TOL and errs["lse"] < LSE_TOL, errs
    for name in ("dq", "dk", "dv"):
        assert errs[name] <= BF16_GRAD_TOL, errs


@pytest.mark.parametrize("B,T,H", PEAK_SHAPES)
def test_peaked_f32(dev, B, T, H):
    """the bounds of test_attention_f32_fwd_bwd"""
    r, inner = _peaked("f32", B, T, H), H * 64
    O, lse, DQ, _ = _run_peaked(dev, "f32", B, T, H)
    out, l, got = O[: B * T].cpu().double().view(B, T, inner), lse.cpu().double(), DQ[: B * T].cpu().double().view(B, T, 3 * inner)
    print(f"attention_dropout f32 B={B} T={T} H={H}: out {_rel(out, r['out']):.2e}, lse {(l - r['lse']).abs().max().item():.2e}, " +
          ", ".join(f"{n} {_rel(g, w):.2e}" for (n, g), (_, w) in zip(_blocks(got, inner), _blocks(r["grad"], inner))))
    assert torch.allclose(out, r["out"], atol=2e-6, rtol=1e-5)
    assert torch.allclose(l, r["lse"], atol=1e-5, rtol=1e-6)
    assert (got - r["grad"]).abs().max() <= 1e-5 * r["grad"].abs().max()


@pytest.mark.parametrize("B,T,H", PEAK_SHAPES)
def test_bounds_discriminate(B, T, H):
    """CPU only: a mask that is wrong in the last partial tile's keys (a), its queries (b) or for one (b, head) (c) moves the float64
    reference by at least 3x the bf16 bounds (the fp32 ones are three orders tighter), in the output and in every gradient block --
    a kernel that applied such a mask cannot pass test_peaked_*."""
    r, inner = _peaked("bf16", B, T, H), H * 64
    other = _host_mask(PEAK_SEED[0] + 1, PEAK_SEED[1], B, T, H, PEAK_P).double()
    edge = 96 * ((T - 1) // 96)
    a, b, c = r["mask"].clone(), r["mask"].clone(), r["mask"].clone()
    a[..., :, edge:] = other[..., :, edge:]
    b[..., edge:, :] = other[..., edge:, :]
    c[-1, -1] = other[-1, -1]
    for name, m in (("a", a), ("b", b), ("c", c)):
        out, _, grad = _reference(r["exact"], r["dO"], m, B, T, H)
        ratios = {"out": _rel(out, r["out"]) / BF16_OUT_TOL}
        for (n, g), (_, w) in zip(_blocks(grad, inner), _blocks(r["grad"], inner)):
            ratios[n] = (g - w).abs().max().item() / w.abs().max().item() / BF16_GRAD_TOL
        print(f"attention_dropout discrimination B={B} T={T} H={H} ({name}): " + ", ".join(f"{k} {v:.1f}x" for k, v in ratios.items()))
        assert min(ratios.values()) >= 3.0, (name, ratios)


# ------------------------------------------------------------------------------------------------------------------ 3. small things
@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_bwd_precedence_dropout_over_rows_and_workspace(dev, prec):
    """ops.attention_bwd: drop_p > 0 wins over need_rows and ws (the engine's _attn_block_bwd passes drop_p and need_rows together) -- the
    full dropout result, bit for bit, and a workspace the one-pass kernel never touched"""
    from gaviko_amd import ops
    B, T, H = 2, 200, 3
    _, _, want, want_delta = _run_peaked(dev, prec, B, T, H)
    ws = ops.attention_bwd_workspace(B, T, H, dev)
    _, _, got, delta = _run_peaked(dev, prec, B, T, H, need_rows=5, ws=ws)
    assert torch.equal(got, want) and torch.equal(delta, want_delta)
    assert want[: B * T].float().abs().max().item() > 0 and torch.isfinite(want_delta).all()
    assert int(ws.abs().max()) == 0


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_drop_p_zero_with_a_seed_is_the_plain_kernel(dev, prec):
    """forward and backward, bit for bit (test_dropout_gpu.py covers the bf16 forward alone)"""
    from gaviko_amd import ops
    B, T, H = 2, 200, 3
    r = _peaked(prec, B, T, H)
    Q, DO = _to_dev(dev, prec, r["op"], B * T), _to_dev(dev, prec, r["dO"], B * T)
    O0, lse0 = ops.act_zeros(B * T, H * 64, _dtype(prec), dev), torch.zeros(B, H, T, device=dev)
    ops.attention_fwd(Q, O0, lse0, B, T, H, SCALE, q_prescaled=True)
    DQ0, delta0 = ops.act_zeros(B * T, 3 * H * 64, _dtype(prec), dev), torch.zeros(B, H, T, device=dev)
    ops.attention_bwd(Q, O0, DO, lse0, delta0, DQ0, B, T, H, SCALE, q_prescaled=True)
    O1, lse1, DQ1, delta1 = _run_peaked(dev, prec, B, T, H, p=0.0, seed=31)         # a seed and a seed word, both unused at p = 0
    assert torch.equal(O0, O1) and torch.equal(lse0, lse1)
    assert torch.equal(DQ0, DQ1) and torch.equal(delta0, delta1)
    assert DQ0[: B * T].float().abs().max().item() > 0


@pytest.mark.parametrize("prec", ["bf16", "f32"])
@pytest.mark.parametrize("B,T,H", [(2, 200, 3), (1, 129, 12)])
def test_dropout_is_repeatable(dev, prec, B, T, H):
    """no atomics in the dropout kernels: a second run of the same descriptor that differs in one bit read something uninitialised"""
    first = _run_peaked(dev, prec, B, T, H)
    again = _run_peaked(dev, prec, B, T, H)
    for name, x, y in zip(("out", "lse", "dqkv", "delta"), first, again):
        assert torch.equal(x, y), name
