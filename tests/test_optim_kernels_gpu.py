"""gvk_adam_step called directly: ONE launch against the header formula of csrc/optim.hip in float64, from identical fp32 inputs (no
chained steps, so no drift), with guard elements around every parameter and behind the flat buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

BLOCK = 1024                  # elements per workgroup of gvk_adam_step (csrc/optim.hip: kAdamBlockElems)
U = 2.0 ** -24                # one IEEE fp32 rounding, relative
FLT_MIN = 2.0 ** -126         # below it a rounding is absolute, not relative
GUARD, TAIL = 8, 64
# 1, 3, 1023, 1024, 1025, 2048, 2049, 5 in an order whose flat offsets 1, 1025, 3073, 4098, 6147, 7170, 7175 are no multiples of 4;
# 1024 and 2048 end on a block boundary, every other tensor ends inside a block
SIZES = [1, 1024, 2048, 1025, 2049, 1023, 5, 3]
SENTINEL = 1e-30              # small, so that `p -= u` changes its bits for any u != 0 (a large sentinel would absorb the update)

# (beta1, bias_c1, bias_c2): step 1; step 17 of a run whose beta1 OneCycle has cycled to 0.87; a late step, both corrections within 1e-6 of 1
SETTINGS = {"step1": (0.9, 1 - 0.9, 1 - 0.999),
            "mid": (0.87, 1 - 0.87 ** 17, 1 - 0.999 ** 17),
            "late": (0.9, 1 - 3e-7, 1 - 6e-7)}
# (norm_sq or None, max_norm, roundings in g = grad * clip)
CLIPS = {"null": (None, 1e-3, 0),          # norm_sq == NULL: max_norm (which would clip by 1000) must be ignored
         "clipped": (1e6, 1.0, 4),         # clip ~ 1e-3
         "unclipped": (1e-4, 1.0, 0),      # clip == 1 exactly: the gradient is written back with its own bits
         "exact": (4.0, 2.0, 4)}           # norm == max_norm: the + 1e-6 puts clip just below 1


def f32(x):
    return np.float32(x)


def adam_tables(params, dev):
    """Pointer table and [nblocks][4] block table (tensor id, offset inside the tensor, offset into the flat buffers, count) for
    `params` laid out back to back in the flat buffers -- the layout FusedAdamOneCycle binds."""
    rows, off = [], 0
    for tid, p in enumerate(params):
        n = p.numel()
        for o in range(0, n, BLOCK):
            rows.append((tid, o, off + o, min(BLOCK, n - o)))
        off += n
    ptr = torch.tensor([p.data_ptr() for p in params], dtype=torch.int64, device=dev)
    blk = torch.tensor(rows, dtype=torch.int32, device=dev).contiguous()
    return ptr, blk, len(rows), off


def make_inputs(seed=11):
    """fp32 p, g, m, v over the flat index.  Element i is in regime i % 8:
    0: g = m = v = 0 (the parameter must keep its bits);  1: |g|, |m| ~ 1e-12, v ~ 1e-24, so sqrt(v) << eps = 1e-8 and eps decides the
    update;  2: |g| ~ 1e4, v ~ 1e7;  3-7: ordinary (g ~ N(0,1), m ~ N(0,0.1), 0 <= v < 0.01)."""
    r = np.random.default_rng(seed)
    n = sum(SIZES)
    reg = np.arange(n) % 8
    sign = lambda: np.where(r.random(n) < 0.5, -1.0, 1.0)
    p = r.standard_normal(n)
    g = r.standard_normal(n)
    m = 0.1 * r.standard_normal(n)
    v = 0.01 * r.random(n)
    tiny, big, zero = reg == 1, reg == 2, reg == 0
    g = np.where(tiny, sign() * 1e-12 * r.uniform(0.5, 2.0, n), g)
    m = np.where(tiny, sign() * 1e-12 * r.uniform(0.5, 2.0, n), m)
    v = np.where(tiny, 1e-24 * r.uniform(0.1, 1.0, n), v)
    g = np.where(big, sign() * 1e4 * r.uniform(0.5, 2.0, n), g)
    m = np.where(big, 1e3 * r.standard_normal(n), m)
    v = np.where(big, 1e7 * r.uniform(0.1, 1.0, n), v)
    g, m, v = (np.where(zero, 0.0, a) for a in (g, m, v))
    return tuple(a.astype(np.float32) for a in (p, g, m, v)), reg


def scalars(setting, clip):
    """Every scalar as the fp32 value the kernel receives."""
    b1, c1, c2 = SETTINGS[setting]
    ns, max_norm, kclip = CLIPS[clip]
    return dict(lr=f32(1e-3), b1=f32(b1), b2=f32(0.999), eps=f32(1e-8), c1=f32(c1), c2=f32(c2), max_norm=f32(max_norm),
                ns=None if ns is None else f32(ns), kclip=kclip)


def reference_f64(p, g, m, v, s):
    """The header formula of csrc/optim.hip in float64 on the fp32 inputs, and the rounding bound of every output (see the test)."""
    d = lambda x: np.asarray(x, dtype=np.float64)
    p, g, m, v = d(p), d(g), d(m), d(v)
    lr, b1, b2, eps, c1, c2 = (float(s[k]) for k in ("lr", "b1", "b2", "eps", "c1", "c2"))
    clip = 1.0 if s["ns"] is None else min(1.0, float(s["max_norm"]) / (np.sqrt(float(s["ns"])) + float(f32(1e-6))))
    k = s["kclip"]
    assert (k == 0) == (clip == 1.0)
    g1 = g * clip
    m1 = b1 * m + (1 - b1) * g1
    v1 = b2 * v + (1 - b2) * g1 * g1
    step, den = lr / c1, np.sqrt(v1) / np.sqrt(c2) + eps
    u = step * m1 / den
    p1 = p - u
    # the bound counts relative roundings: no intermediate of the kernel may fall into the subnormal range
    for x in (g1, b1 * m, (1 - b1) * g1, b2 * v, (1 - b2) * g1, (1 - b2) * g1 * g1, m1 / den, u):
        assert np.all((x == 0) | (np.abs(x) >= FLT_MIN))
    e_g = k * np.abs(g1)
    e_m = 2 * np.abs(b1 * m) + (k + 3) * np.abs((1 - b1) * g1)
    e_v = 2 * b2 * v + (2 * k + 4) * (1 - b2) * g1 * g1
    e_u = step / den * e_m + (k + 10) * np.abs(u)
    e_p = e_u + np.abs(p1)
    return dict(g=g1, m=m1, v=v1, u=u, p=p1, clip=clip), {n: 2 * U * e for n, e in (("g", e_g), ("m", e_m), ("v", e_v), ("u", e_u), ("p", e_p))}


def restated_f32(p, g, m, v, s):
    """adam_step_kernel operation by operation in numpy float32 (same order, no contraction)."""
    one = f32(1)
    if s["ns"] is None:
        clip = one
    else:
        c = s["max_norm"] / (np.sqrt(s["ns"]) + f32(1e-6))
        clip = one if c > one else c
    step, rs2 = s["lr"] / s["c1"], one / np.sqrt(s["c2"])
    g1 = g * clip
    m1 = s["b1"] * m + (one - s["b1"]) * g1
    v1 = s["b2"] * v + (one - s["b2"]) * g1 * g1
    p1 = p - step * (m1 / (np.sqrt(v1) * rs2 + s["eps"]))
    assert all(a.dtype == np.float32 for a in (g1, m1, v1, p1)) and all(type(x) is np.float32 for x in (clip, step, rs2))
    return dict(g=g1, m=m1, v=v1, p=p1)


def bits(t):
    return t.view(torch.int32)


def launch(dev, p, g, m, v, s):
    """One gvk_adam_step over SIZES.  Every parameter lives inside one arena, GUARD sentinels before and after it; behind the last one the
    arena goes on for another total + TAIL sentinels, so that a parameter write at a wrong offset still lands in memory this test owns
    and compares.  Returns the new (p, g, m, v) as numpy, after checking every element the launch must not write."""
    from gaviko_amd import lib
    total = sum(SIZES)
    arena = torch.full((sum(n + 2 * GUARD for n in SIZES) + total + TAIL,), SENTINEL, device=dev)
    params, written, a, off = [], torch.zeros(arena.numel(), dtype=torch.bool, device=dev), GUARD, 0
    for n in SIZES:
        params.append(arena[a: a + n])
        params[-1].copy_(torch.from_numpy(p[off: off + n]))
        written[a: a + n] = True
        a, off = a + n + 2 * GUARD, off + n
    tail = torch.from_numpy(np.random.default_rng(5).standard_normal(TAIL).astype(np.float32))
    flat, mm, vv = (torch.cat([torch.from_numpy(x), tail + i]).to(dev) for i, x in enumerate((g, m, v)))
    arena0, tails0 = arena.clone(), [t[total:].clone() for t in (flat, mm, vv)]
    ptr, blk, nblocks, tot = adam_tables(params, dev)
    assert tot == total and nblocks == sum(-(-n // BLOCK) for n in SIZES)
    norm_sq = None if s["ns"] is None else torch.tensor([float(s["ns"])], dtype=torch.float32, device=dev)
    d = lib.AdamDesc(ptr_tab=lib.ptr(ptr), blk_tab=lib.ptr(blk), grad=lib.ptr(flat), m=lib.ptr(mm), v=lib.ptr(vv),
                     norm_sq=None if norm_sq is None else lib.ptr(norm_sq), nblocks=nblocks,
                     **{k: float(s[n]) for k, n in (("lr", "lr"), ("beta1", "b1"), ("beta2", "b2"), ("eps", "eps"), ("bias_c1", "c1"),
                                                    ("bias_c2", "c2"), ("max_norm", "max_norm"))})
    lib.check(lib.load().gvk_adam_step(C.byref(d), lib.stream_ptr()), "gvk_adam_step")
    torch.cuda.synchronize()
    assert torch.equal(bits(arena)[~written], bits(arena0)[~written]), "a parameter write left its tensor's extent"
    for name, t, t0 in zip(("grad", "m", "v"), (flat, mm, vv), tails0):
        assert torch.equal(bits(t[total:]), bits(t0)), f"{name}: the tail behind the parameters was written"
    return tuple(x.cpu().numpy() for x in (torch.cat(params), flat[:total], mm[:total], vv[:total]))


@pytest.mark.gpu
@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_adam_step_one_launch_matches_float64(dev, setting, clip):
    """New p, m, v and the written-back gradient of one launch, element by element, against float64.

    The library is built with -ffp-contract=off and without fast-math, and hipcc's fp32 divide and sqrt are correctly rounded, so every
    operation of adam_step_kernel is one IEEE rounding, relative error <= u = 2**-24 (the inputs keep every intermediate out of the
    subnormal range; reference_f64 asserts it).  First-order bounds in magnitudes, with k = 4 roundings in the clipped gradient
    (sqrt, + 1e-6, divide, g * clip) and k = 0 where clip == 1 exactly (norm_sq NULL or the norm below max_norm):
      grad  |dg| <= k u |g|
      m     |dm| <= u (2 |b1 m0| + (k + 3) |(1 - b1) g|)          product and sum; 1 - b1, g, product, sum  (the two terms may cancel)
      v     |dv| <= u (2 b2 v0 + (2k + 4) (1 - b2) g^2)           product and sum; 1 - b2, g twice, two products, sum  (<= (2k + 4) u v)
      u     |du| <= step/den |dm| + (k + 10) u |u|                den = sqrt(v) rs2 + eps: (k + 2) + 1 from sqrt(v), 2 in rs2, product, sum
                                                                  = k + 7; then the divide, step = lr / bias_c1 and step * (..)
      p     |dp| <= |du| + u |p|                                  p = p - u
    The assertion uses twice these counts, for the float64 reference's own handling of the fp32 constants.  Not tuned to any result.

    Second assertion: the kernel restated operation by operation in numpy float32 gives the same bits."""
    (p, g, m, v), reg = make_inputs()
    s = scalars(setting, clip)
    want, bound = reference_f64(p, g, m, v, s)
    p1, g1, m1, v1 = launch(dev, p, g, m, v, s)
    got = dict(g=g1, m=m1, v=v1, p=p1)
    for name in ("g", "m", "v", "p"):                         # the update u is seen through p only: its bound is part of p's
        err = np.abs(got[name].astype(np.float64) - want[name])
        worst = int(np.argmax(err - bound[name]))
        print(f"{setting}/{clip} {name}: max err/bound {np.max(err / np.maximum(bound[name], 1e-300)):.3f} "
              f"(elem {worst}, regime {reg[worst]})")
        assert np.all(err <= bound[name]), (name, worst, got[name][worst], want[name][worst], bound[name][worst])
    zero = reg == 0
    assert np.array_equal(p1[zero].view(np.int32), p[zero].view(np.int32)), "g = m = v = 0 must leave the parameter's bits alone"
    assert not m1[zero].any() and not v1[zero].any()
    if s["kclip"] == 0:
        assert np.array_equal(g1.view(np.int32), g.view(np.int32)), "clip == 1: the gradient keeps its bits"
    else:
        assert want["clip"] < 1.0 and np.all(np.abs(g1[~zero]) < np.abs(g[~zero]))
    tiny = reg == 1                                          # the eps term decides: the update is ~ step * m / eps, far from m / sqrt(v)
    assert np.all(np.sqrt(want["v"][tiny]) / np.sqrt(float(s["c2"])) < 1e-2 * float(s["eps"]))
    same = restated_f32(p, g, m, v, s)
    for name, mine in (("g", g1), ("m", m1), ("v", v1), ("p", p1)):
        diff = np.flatnonzero(mine.view(np.int32) != same[name].view(np.int32))
        assert diff.size == 0, (f"{name} differs from the float32 restatement at {diff.size} elements", int(diff[0]),
                                mine[diff[0]], same[name][diff[0]])
