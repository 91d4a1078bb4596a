"""Structured inputs, float64 reference, planted faults and the per-element comparison for the flash-attention kernels (attention_fwd.hip,
attention_bwd.hip, attention_map.hip, attention_f32.hip) -- test infrastructure in the style of tests/elastic_ref.py, not collected by pytest.

Inputs.  Every operand is exact in bf16; the device operand carries the q block pre-scaled by scale*log2(e) (test_kernels_gpu._attn_operands'
convention) and the float64 reference divides that factor back out, so both sides attend over the same numbers.

  selector:  one book of +-1 vectors c_0 .. c_{n-1} in 64 dimensions (torch seed 0, largest off-diagonal |c_a.c_b| <= 40).  In every (batch,
             head) key row j holds the code of its GROUP, groups being runs of g in {1, 2, 4} rows of a (b, h)-dependent permutation of the
             rows (a last short run is split into sizes 2 and 1, so every weight stays a power of two); query row i holds 2 * c (pre-scaled
             amplitude exactly 2.0, i.e. A = 2 / (scale*log2 e) = 11.09) of the group of key tau_{b,h}(i), tau another permutation.  Matched
             score 128 log2 units, every other one <= 80 (84 with unequal keys): the matched keys carry 1/size each, all others < 2^-40.
             Every row is a matched query AND a matched key, so every loop boundary of every kernel form holds both.  "pm" cases make the
             keys of a pair UNEQUAL at equal score (c + e, c - e with e sparse, e.c = 0), which gives dq a value; with equal keys dq = 0.
             V and dO are integers in [-4, 4] drawn per (b, h, row, column); the padding rows of qkv / out / dout continue book and draw.
  offset:    k_j = r_j + gamma_j u, q'_i = s_i + beta_i u with u = 4 on the last 8 coordinates and r, s multiples of 1/8 in [-1, 1] on the
             other 56: score (log2) = s_i.r_j + 128 beta_i gamma_j, a multiple of 1/64 below 2^12 -- exact in fp32 in any summation order.
             beta * 128 = -300, +300, +3008; "mixed": -300 / 0 / +300 by query row mod 3; "late": keys < late_edge(T) at -300, the others at +300
             (every key form's first tile all low where T > 128: alpha underflows to 0 at the next one).

Comparison, per element:  |got - want| <= r * 2^-9 * |want| + floor,  non-finite results rejected outright.  r = bf16 roundings on the path:
  O      r = 2   P fragment (cvt_block), stored result (store_rows_t)
  dv     r = 2   P fragment, stored result
  dk     r = 3   dS fragment, stored result, the forward's O (two roundings of its own) read back through delta
  dq     r = 3   dS fragment, stored result, the forward's O through delta
  delta  r = 2   the two roundings of the forward's O; the products and the row sum are fp32
The floor covers the elements whose reference is (nearly) zero.  MEASURED below is the largest |got - want| - r 2^-9 |want| the shipped
kernels showed on the MI355X over every case and form of tests/test_attention_structured_gpu.py (the least floor that accepts them; it
bounds the error on the elements with |want| < floor from above), and every floor is exactly FLOOR_FACTOR = 4 times it (the other tile
forms sum in another order) -- FLOORS is computed from MEASURED, one constant per output and INPUT FAMILY:
  selector                 measured  O 1.2e-7  dv 1.2e-7  delta 4.8e-7  dq 3.13e-2  dk 3.35e-1    floor  O 4.8e-7  dv 4.8e-7  delta 1.92e-6  dq 0.125  dk 1.34
  offset -300, +300,       measured  O 7.3e-3  dv 1.9e-2  delta 1.64e-1 dq 1.34e-1  dk 1.48       floor  O 0.029   dv 0.076   delta 0.66     dq 0.54   dk 5.9
    mixed, late
  offset +3008             measured  O 7.3e-3  dv 1.16e-2 delta 1.64e-1 dq 1.01e-1  dk 13.7       floor  O 0.029   dv 0.046   delta 0.66     dq 0.40   dk 55
  fp32 path, selector      measured  O 1.54e-5 dv 2.7e-23 dq 2.16e-6    dk 1.62e-6                (dv: the terms dO / size and their sums are exact in fp32)
  fp32 path, offset        measured  O 3.25e-5 dv 6.54e-5 dq 4.48e-5    dk 4.95e-3                (no +3008 case on this path)
(each measured figure is the printed one rounded UP in its last digit)
The families are kept apart because the error that no |want| bounds is the rounding of the dS (or P) fragment times the OTHER operand:
sum_i |dS_ij| |q_i| 2^-9 for dk.  On the selector inputs O, dv and delta are reproduced to fp32 rounding and only dS (multiples of 1/16 up
to ~200, more than 8 bits) rounds at all; on the offset inputs q carries the offset on 8 coordinates (|q| about 52 at +-300, 521 at +3008),
the terms of dk cancel, and the same rounding is worth ten times as much at +3008 as at +-300 -- so +3008 is a family of its own and the
coarse dk floor it needs is not lent to the +-300, mixed and late cases.  tests/test_attention_structured.py plants every fault on the
selector inputs and the forward's faults on the offset inputs too, and holds every floor below a tenth of what the faults produce.
fp32 path: the same rule with e32 (below) in place of r 2^-9, MEASURED_F32 -> FLOOR_F32 per family (no +3008 case on this path).
fp32 outputs (lse, the map kernels, everything on the fp32 path):  |got - want| <= e * |want| + floor32 with
  e = 8 ulp32(|s|max) ln 2 + (T + 2) 2^-24:   |s|max the largest |score| in log2 units (+ 64 for the partial sums of the 64-wide contraction);
  8 = 5 accumulation steps of the score's MFMA chain + the running-max subtraction + log2/exp2's ulp + the final multiply by ln 2; the row sum
  of T exp2 terms adds (T + 2) 2^-24 relative.  For lse itself the bound is absolute: e_lse = 8 ulp32(|lse| log2 e + 64) ln 2 + (T + 2) 2^-24
  (1.0e-4 on the selector inputs, 1.4e-3 at the +3008 offset where one fp32 ulp of lse is 2.4e-4; the old bound was 2e-3 everywhere).
  floor32 = FLOOR32 = 2^-20 for the map kernels is argued, not measured: their outputs are sums of NON-NEGATIVE terms w P and w P max(0, dP),
  so nothing cancels and e * |want| covers every element with a value; an element without one (selector inputs: no matched query in the
  window) is a sum of at most T < 2^9 terms below 4 * 1024 * 2^-44 (w, dP, an unmatched P), under 2^-23.
  The GPU tests print the largest |got - want| - e |want| they saw (3.6e-36 at the most with the shipped kernels).
"""
import math

import torch

ATTN_C = 0.125 * 1.4426950408889634          # what the q block carries when it reaches the bf16 kernels: q * scale * log2(e)
LN2 = math.log(2.0)
T_LIST = (1, 31, 33, 95, 96, 97, 127, 128, 129, 193, 257, 289)
TILES = (32, 96, 128)
SHAPES = tuple((2, T, 2) for T in T_LIST) + ((3, 97, 2), (2, 129, 3))
SELECTOR_KINDS = ("sel1", "sel2", "sel4", "pm")
OFFSET_KINDS = ("off-300", "off+300", "off+3008", "mixed", "late")
F32_OFFSET_KINDS = ("off-300", "off+300", "mixed", "late")
BOOK_SEED, BOOK_CAP, N_CODES = 0, 40, 393
SENTINEL = -77.0                             # exact in bf16, no input or result of these cases takes it
R = {"O": 2, "dv": 2, "dk": 3, "dq": 3, "delta": 2}
FLOOR_FACTOR = 4
FAMILIES = ("sel", "off", "off3008")
MEASURED = {"sel": {"O": 1.2e-7, "dv": 1.2e-7, "dk": 3.35e-1, "dq": 3.13e-2, "delta": 4.8e-7},
            "off": {"O": 7.3e-3, "dv": 1.9e-2, "dk": 1.48, "dq": 1.34e-1, "delta": 1.64e-1},
            "off3008": {"O": 7.3e-3, "dv": 1.16e-2, "dk": 1.37e+1, "dq": 1.01e-1, "delta": 1.64e-1}}
MEASURED_F32 = {"sel": {"O": 1.54e-5, "dq": 2.16e-6, "dk": 1.62e-6, "dv": 2.7e-23},
                "off": {"O": 3.25e-5, "dq": 4.48e-5, "dk": 4.95e-3, "dv": 6.54e-5}}
FLOORS = {fam: {name: FLOOR_FACTOR * m for name, m in per.items()} for fam, per in MEASURED.items()}
FLOOR_F32 = {fam: {name: FLOOR_FACTOR * m for name, m in per.items()} for fam, per in MEASURED_F32.items()}
FLOOR32 = 2.0 ** -20                         # the map kernels (argued, see the docstring; the GPU tests print how much of it is used)


def family(kind):
    return "sel" if kind in SELECTOR_KINDS else "off3008" if kind == "off+3008" else "off"


def floors(kind):
    return FLOORS[family(kind)]


def floors_f32(kind):
    return FLOOR_F32[family(kind)]


def late_edge(T):
    """"late": keys below this row sit 600 log2 units under the others.  128 where a sequence has more than one 128-key tile, so that the
    96-key and the 128-key form both begin with an all-low tile; 96 for the shorter ones, where only the 96-key form has a second tile."""
    return 128 if T > 128 else 96


def pad_rows(m):
    return (m + 127) // 128 * 128


def book(n=N_CODES, seed=BOOK_SEED):
    """[n, 64] of +-1 (float64) from a fixed torch seed; refused unless the largest off-diagonal correlation is within BOOK_CAP"""
    g = torch.Generator().manual_seed(seed)
    c = (torch.randint(0, 2, (n, 64), generator=g) * 2 - 1).double()
    corr = c @ c.T
    corr.fill_diagonal_(0)
    if corr.abs().max().item() > BOOK_CAP:
        raise ValueError(f"code book seed {seed}: largest correlation {corr.abs().max().item()} > {BOOK_CAP}")
    return c


def boundaries(T):
    """rows on a loop boundary of some kernel form: row 0, T-1, first and last row of every 32-row MFMA block, 96- and 128-row tile, and
    128-query workgroup"""
    out = {0, T - 1}
    for t in TILES:
        for e in range(0, T, t):
            out |= {e, min(e + t, T) - 1}
    return sorted(out)


def _perm(T, which):
    """(a * j + c) mod T with a coprime to T, a and c different for every `which`"""
    primes = [p for p in (3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47) if math.gcd(p, T) == 1] or [1]
    a, c = primes[which % len(primes)], (7 * which + 3) % T
    return (a * torch.arange(T) + c) % T


def group_sizes(T, g):
    """runs of g, the remainder split into 2 and 1: every size a power of two"""
    sizes, rest = [g] * (T // g), T % g
    for s in (2, 1):
        if rest >= s:
            sizes.append(s)
            rest -= s
    return sizes


class Case:
    """op: bf16 [pad(B*T), 3*inner] device operand (padding rows filled);  dout: bf16 [pad(B*T), inner];  out_pad: bf16 [pad(B*T), inner] what
    the padding rows of the forward's O are set to before a backward;  size [B,H,T] (selector: the matched group's size of every query)"""

    def __init__(self, kind, B, T, H):
        self.kind, self.B, self.T, self.H, self.inner = kind, B, T, H, H * 64
        self.rows = pad_rows(B * T)

    def exact_flat(self):
        """float64 [rows, 3*inner]: the q | k | v the device operand represents (unscaled q)"""
        e = self.op.double()
        e[:, : self.inner] /= ATTN_C
        return e

    def qkv(self, flat=None):
        """-> q, k, v float64 [B,H,T,64]"""
        flat = self.exact_flat() if flat is None else flat
        x = flat[: self.B * self.T].reshape(self.B, self.T, 3, self.H, 64)
        return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(3))

    def d_o(self):
        return self.dout[: self.B * self.T].double().reshape(self.B, self.T, self.H, 64).permute(0, 2, 1, 3)

    def smax(self):
        q, k, _ = self.qkv()
        return (q @ k.transpose(-1, -2)).abs().max().item() * ATTN_C


def _int_pattern(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).double()


def selector_case(B, T, H, kind):
    cs = Case(kind, B, T, H)
    g = {"sel1": 1, "sel2": 2, "sel4": 4, "pm": 2}[kind]
    c = book()
    sizes = group_sizes(T, g)
    assert len(sizes) <= N_CODES
    code_of_slot = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))       # slot (0..T-1) -> code
    size_of_slot = torch.repeat_interleave(torch.tensor(sizes), torch.tensor(sizes))
    first_of_slot = torch.cumsum(torch.tensor([0] + sizes[:-1]), 0).repeat_interleave(torch.tensor(sizes))
    rows, inner = cs.rows, cs.inner
    x = torch.zeros(rows, 3, H, 64, dtype=torch.float64)
    cs.size = torch.zeros(B, H, T, dtype=torch.long)
    cs.match = torch.zeros(B, H, T, T, dtype=torch.bool)
    nb = (rows + T - 1) // T                                                                      # the padding rows continue as batches B, B+1, ..
    for b in range(nb):
        for h in range(H):
            mu, tau = _perm(T, b * H + h), _perm(T, 5 + 3 * (b * H + h))
            kcode, ksize = code_of_slot[mu], size_of_slot[mu]                                     # key row j -> code, group size
            k = c[kcode].clone()
            if kind == "pm":                                                                       # pairs: c + e, c - e with e.c = 0, e on two coordinates
                second = (mu - first_of_slot[mu]) == 1
                d0 = (kcode * 2) % 63
                e = torch.zeros(T, 64, dtype=torch.float64)
                e[torch.arange(T), d0] = k[torch.arange(T), d0]
                e[torch.arange(T), d0 + 1] = -k[torch.arange(T), d0 + 1]
                pair = (ksize == 2).double()[:, None]
                k = k + pair * torch.where(second[:, None], -e, e)
            q = 2.0 * c[kcode[tau]]
            lo = b * T
            n = min(T, rows - lo)
            x[lo: lo + n, 0, h], x[lo: lo + n, 1, h] = q[:n], k[:n]
            if b < B:
                cs.size[b, h] = ksize[tau]
                cs.match[b, h] = kcode[tau][:, None] == kcode[None, :]
    x[:, 2] = _int_pattern((rows, H, 64), 101)
    cs.built = x.reshape(rows, 3 * inner)
    cs.op = cs.built.bfloat16()
    cs.dout = _int_pattern((rows, inner), 102).bfloat16()
    cs.out_pad = _int_pattern((rows, inner), 103).bfloat16()
    return cs


def offset_case(B, T, H, kind):
    cs = Case(kind, B, T, H)
    rows, inner = cs.rows, cs.inner
    g = torch.Generator().manual_seed(200 + T)
    x = torch.zeros(rows, 3, H, 64, dtype=torch.float64)
    x[:, :2, :, :56] = torch.randint(-8, 9, (rows, 2, H, 56), generator=g).double() / 8
    t = torch.arange(rows) % T                                                                    # row within its sample (padding rows continue the count)
    beta = {"off-300": -300.0, "off+300": 300.0, "off+3008": 3008.0, "late": 300.0}.get(kind)
    if kind == "mixed":
        bq = torch.tensor([-300.0, 0.0, 300.0])[t % 3]
    else:
        bq = torch.full((rows,), beta)
    gam = torch.where(t < late_edge(T), -1.0, 1.0).double() if kind == "late" else torch.ones(rows, dtype=torch.float64)
    x[:, 0, :, 56:] = (bq / 128 * 4)[:, None, None]
    x[:, 1, :, 56:] = (gam * 4)[:, None, None]
    x[:, 2] = _int_pattern((rows, H, 64), 111)
    cs.built = x.reshape(rows, 3 * inner)
    cs.op = cs.built.bfloat16()
    cs.dout = _int_pattern((rows, inner), 112).bfloat16()
    cs.out_pad = _int_pattern((rows, inner), 113).bfloat16()
    return cs


def random_case(B, T, H, amp=1.0, seed=51):
    """the inputs of the older tests (test_kernels_gpu.test_attention_fwd): uniform random q, k, v, zero padding rows"""
    cs = Case("random", B, T, H)
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((B * T, 3 * cs.inner), generator=g) * 2 - 1) * amp
    x[:, : cs.inner] *= ATTN_C
    cs.op = torch.zeros(cs.rows, 3 * cs.inner, dtype=torch.bfloat16)
    cs.op[: B * T] = x.bfloat16()
    cs.built = cs.op.double()
    cs.dout = torch.zeros(cs.rows, cs.inner, dtype=torch.bfloat16)
    cs.dout[: B * T] = (torch.rand((B * T, cs.inner), generator=g) * 2 - 1).bfloat16()
    return cs


def make_case(kind, B, T, H):
    return selector_case(B, T, H, kind) if kind in SELECTOR_KINDS else offset_case(B, T, H, kind)


# ------------------------------------------------------------------------------------------------ float64 reference
def attend(q, k, v, d_o, delta=None):
    """Softmax attention and its gradients written out (float64; q [.., Tq, 64], k, v [.., Tk, 64], d_o [.., Tq, 64]) so that a fault can be
    planted in any step; `delta` overrides rowsum(dO * O) in dS.  tests/test_attention_structured.py holds it against autograd."""
    s = q @ k.transpose(-1, -2) * 0.125
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    O = P @ v
    dl = (O * d_o).sum(-1)
    dP = d_o @ v.transpose(-1, -2)
    dS = P * (dP - (dl if delta is None else delta)[..., None])
    return {"O": O, "lse": lse, "P": P, "delta": dl, "dP": dP, "dq": 0.125 * dS @ k, "dk": 0.125 * dS.transpose(-1, -2) @ q,
            "dv": P.transpose(-1, -2) @ d_o}


def autograd_reference(cs, flat=None):
    """the reference of the existing tests: float64 softmax attention and torch autograd over the exact operand values"""
    q, k, v = (t.clone().requires_grad_(True) for t in cs.qkv(flat))
    s = q @ k.transpose(-1, -2) * 0.125
    o = s.softmax(-1) @ v
    o.backward(cs.d_o())
    return {"O": o.detach(), "lse": torch.logsumexp(s.detach(), -1), "delta": (o.detach() * cs.d_o()).sum(-1), "dq": q.grad, "dk": k.grad,
            "dv": v.grad}


def colsum_ref(P, w, q0, q1):
    """ops.attention_colsum's definition: sum_{q0 <= i < q1} w[b,i] P[b,h,i,:]"""
    return torch.einsum("bi,bhij->bhj", w[:, q0:q1], P[:, :, q0:q1])


def gradcolsum_ref(P, dP, w, q0, q1):
    """ops.attention_gradcolsum's definition: sum_{q0 <= i < q1} w[b,i] P[b,h,i,:] max(0, dP[b,h,i,:]), dP = dO . v^T"""
    return torch.einsum("bi,bhij->bhj", w[:, q0:q1], (P * dP.clamp_min(0))[:, :, q0:q1])


def windows(T):
    """query windows [q0, q1) that start and end on, and one off, every 32-row edge (clipped to the sequence, empty ones dropped)"""
    out = {(0, T)}
    for e in range(0, T + 1, 32):
        for a, b in ((e, e + 32), (e + 1, e + 33), (max(e - 1, 0), e + 31), (e, e + 1), (0, e), (0, e + 1)):
            a, b = min(a, T), min(b, T)
            if a < b:
                out.add((a, b))
    return sorted(out)


# ------------------------------------------------------------------------------------------------ comparison
def ulp32(x):
    return 2.0 ** (math.floor(math.log2(max(abs(x), 2.0 ** -126))) - 23)


def ratio(got, want, r, floor):
    """worst |got - want| / (r 2^-9 |want| + floor) over the elements; inf if any result is not finite"""
    got, want = got.double(), want.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    if got.numel() == 0:
        return 0.0
    return ((got - want).abs() / (r * 2.0 ** -9 * want.abs() + floor)).max().item()


def e32(smax, T):
    """relative bound of an fp32 result that is linear in the probabilities (see the module docstring)"""
    return 8 * ulp32(abs(smax) + 64) * LN2 + (T + 2) * 2.0 ** -24


def ratio32(got, want, smax, T, floor=FLOOR32):
    got, want = got.double(), want.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    if got.numel() == 0:
        return 0.0
    return ((got - want).abs() / (e32(smax, T) * want.abs() + floor)).max().item()


def ratio_lse(got, want, T):
    got, want = got.double(), want.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    ulp = torch.exp2(torch.floor(torch.log2(want.abs() / LN2 + 64)) - 23)
    return ((got - want).abs() / (8 * ulp * LN2 + (T + 2) * 2.0 ** -24)).max().item()


def excess(got, want, r):
    """largest |got - want| - r 2^-9 |want|: the least floor that would accept `got`"""
    return ((got.double().cpu() - want).abs() - r * 2.0 ** -9 * want.abs()).max().item() if want.numel() else 0.0


def excess32(got, want, smax, T):
    """the same for an fp32 result: largest |got - want| - e32 |want|"""
    return ((got.double().cpu() - want).abs() - e32(smax, T) * want.abs()).max().item() if want.numel() else 0.0


# ------------------------------------------------------------------------------------------------ planted faults
FAULTS = ("key_T_admitted", "key_T-1_dropped", "rows_past_T_in_dkdv", "head_K", "head_V", "batch_rows", "v_chunks_swapped", "delta_next_row")


def planted(cs, fault):
    """the float64 reference of `cs` with one deliberate error -> the outputs the error can reach, as {name: [B,H,T,..]}"""
    B, T, H = cs.B, cs.T, cs.H
    flat = cs.exact_flat().reshape(cs.rows, 3, H, 64)
    dflat = cs.dout.double().reshape(cs.rows, H, 64)
    q, k, v = cs.qkv()
    d_o = cs.d_o()
    if fault in ("key_T_admitted", "key_T-1_dropped"):
        n = T + 1 if fault == "key_T_admitted" else T - 1                # row b*T + T: the next sample's row 0, or the first padding row
        flat = torch.cat([flat, torch.zeros_like(flat[:1])])            # (no padding row at all: past the buffer the resource returns zeros)
        kk = torch.stack([flat[b * T: b * T + n, 1].permute(1, 0, 2) for b in range(B)])
        vv = torch.stack([flat[b * T: b * T + n, 2].permute(1, 0, 2) for b in range(B)])
        out = attend(q, kk, vv, d_o)
        dk, dv = torch.zeros_like(k), torch.zeros_like(v)                # (a dropped key gets no gradient)
        dk[:, :, : min(n, T)], dv[:, :, : min(n, T)] = out["dk"][:, :, :T], out["dv"][:, :, :T]
        return {x: out[x] for x in ("O", "lse", "delta", "dq")} | {"dk": dk, "dv": dv}
    if fault == "rows_past_T_in_dkdv":                                    # query rows T .. the next tile edge: the next sample's first rows.
        ext = max((T + t - 1) // t * t for t in (96, 128)) - T          # (past the last sample the buffer resource returns zeros: harmless there)
        assert ext > 0
        good = attend(q, k, v, d_o)
        dk, dv = good["dk"].clone(), good["dv"].clone()
        for b in range(B - 1):
            lo, hi = b * T + T, min(b * T + T + ext, cs.rows)
            extra = attend(flat[lo:hi, 0].permute(1, 0, 2), k[b], v[b], dflat[lo:hi].permute(1, 0, 2))
            dk[b] += extra["dk"]
            dv[b] += extra["dv"]
        return {"dk": dk, "dv": dv}
    if fault == "head_K":
        return _all(attend(q, k.roll(-1, 1), v, d_o))
    if fault == "head_V":
        return _all(attend(q, k, v.roll(-1, 1), d_o))
    if fault == "batch_rows":
        return _all(attend(q, k.roll(-1, 0), v.roll(-1, 0), d_o))
    if fault == "v_chunks_swapped":                                        # columns 16..23 <-> 24..31 of the last row of (batch 0, head 1)
        vv = v.clone()
        vv[0, 1, T - 1, 16:24], vv[0, 1, T - 1, 24:32] = v[0, 1, T - 1, 24:32], v[0, 1, T - 1, 16:24]
        return _all(attend(q, k, vv, d_o))
    if fault == "delta_next_row":
        good = attend(q, k, v, d_o)
        dl = good["delta"].reshape(-1).roll(-1).reshape(B, H, T)           # [B,H,T] is contiguous: the next entry of the buffer
        return {x: attend(q, k, v, d_o, delta=dl)[x] for x in ("dq", "dk")} | {"delta": dl}
    raise ValueError(fault)


def _all(out):
    return {x: out[x] for x in ("O", "lse", "delta", "dq", "dk", "dv")}


def m_never_lowered(cs):
    """fault 8: the running maximum starts at 0 and is never lowered -- fp32 arithmetic as the kernel's: P = exp2(s - 0), l = sum P, O = P.v / l,
    lse = (0 + log2 l) ln 2.  At the -300 offset every P underflows: l = 0."""
    q, k, v = cs.qkv()
    s2 = (q @ k.transpose(-1, -2) * ATTN_C).float()
    p = torch.exp2(s2)
    l = p.sum(-1)
    return {"O": (p @ v.float()) / l[..., None], "lse": torch.log2(l) * LN2, "l": l}


def rejections(cs, want, bad):
    """{output: ratio by which the comparison refuses `bad` (a planted() result) against the true reference `want`}"""
    return {name: ratio_lse(val, want[name], cs.T) if name == "lse" else ratio(val, want[name], R[name], floors(cs.kind)[name])
            for name, val in bad.items()}


def rejection(cs, want, bad):
    """the largest of rejections()"""
    return max(rejections(cs, want, bad).values())
