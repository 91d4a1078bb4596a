"""The volume kernels (gaviko_amd/csrc/augment.hip) and gvk_sumsq (gaviko_amd/csrc/optim.hip) with inputs whose reference is exact in any
order of operations, at the sizes where their loop structure changes.  Nothing here is measured and nothing has a tolerance, except the
general-affine case, which reuses the bound of test_data_metrics.py::test_spatial_transform_vs_oracle (1e-3 * |vol|.max()).

1. volume_minmax: a volume of values in [0, 1) with -1 and +2 planted.  The minimum and the maximum are exact whatever the order, and a
   kernel that skips the planted element, or reads past its slab into a neighbour's, returns another pair.  The planted positions sit on
   both sides of every boundary of the kernel: the slab edges, the four-times unrolled trip (256 float4 apart), the 256-stride loop after
   it, the short last slab, the empty slabs of a small volume.
2. rescale_intensity: the four float32 steps of the oracle, bit for bit, at the same sizes and past the 1024-block grid cap, for three
   output ranges, with the reduced (min, max) pair read back and sentinels behind the output.
3. spatial_transform: volumes whose voxels are all distinct; flips and signed-permutation affines with integer translations are plain
   gathers (the trilinear weights are exactly 0 and 1), written here with integer indexing, at widths on both sides of the 64-wide block
   and heights that are no multiple of 4.
4. gvk_sumsq: values from {+-1, +-2, +-3}; every partial sum is an integer below 2^24, so fp32 is exact in any order and the result
   must equal the int64 sum.  No zeros, so a dropped or repeated element changes it.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import data_ref


@pytest.fixture(scope="module")
def dev():
    from gaviko_amd import lib
    lib.require_device()
    return torch.device("cuda:0")


SENTINELS, SENTINEL = 64, -12345.0

V_LARGE = 4 * (256 * 1100 + 7)                    # per = 1101 float4 per slab with 256 slabs; the last slab is short
V_LIST = [4, 8, 1020, 1024, 1028, 30720, V_LARGE]
V_CAPPED = 4 * (2 * 262144 + 4321)                # rescale: more than two sweeps of the 1024-block grid, no multiple of 1024 float4
RANGES = [(0.0, 1.0), (-1.0, 1.0), (0.0, 255.0)]  # rescale: (out_min, out_max)


def _slabs():
    from gaviko_amd import lib
    return lib.load().gvk_minmax_partials() // 2


def _slab_bounds(V, slabs):
    """[(i0, i1)] in float4 units: the kernel's split, per = ceil(V4 / slabs); i0 >= i1 is an empty slab"""
    V4 = V // 4
    per = -(-V4 // slabs)
    return per, [(s * per, min(V4, s * per + per)) for s in range(slabs)]


def _positions(V, slabs):
    """element positions of section 1, those that exist, in a fixed order without repeats"""
    pos = [0, 3, 4, V - 1, V - 4, V - 5]
    if V == V_LARGE:
        per, bounds = _slab_bounds(V, slabs)
        for s in (0, 1, slabs // 2, slabs - 1):
            i0, i1 = bounds[s]
            pos += [4 * i0 - 1, 4 * i0]
            pos += [4 * min(i0 + k, i1 - 1) for k in (255, 256, 767, 768, 1023, 1024, per - 1)]
    out = []
    for p in pos:
        if 0 <= p < V and p not in out:
            out.append(p)
    return out


@functools.lru_cache(maxsize=None)
def _base(V):
    return np.random.default_rng(1000 + V % 997).random(V, dtype=np.float32)      # [0, 1)


def _planted(V, slabs):
    """[B][V]: case b = the base with -1 at p_b and +2 at q_b = the next position of the list (p_b != q_b)"""
    pos = _positions(V, slabs)
    x = np.tile(_base(V), (len(pos), 1))
    for b, p in enumerate(pos):
        q = pos[(b + 1) % len(pos)]
        assert p != q
        x[b, p], x[b, q] = -1.0, 2.0
    return x, pos


def _gauss(V, seed):
    return (np.random.default_rng(seed).standard_normal(V) * 300 + 1000).astype(np.float32)


def _with_sentinels(n, dev):
    """(the whole buffer, its first n elements as a contiguous view)"""
    full = torch.full((n + SENTINELS,), SENTINEL, dtype=torch.float32, device=dev)
    return full, full[:n]


def _sentinels_intact(full, n):
    return bool((full[n:] == SENTINEL).all().item()) and full.numel() == n + SENTINELS


# ------------------------------------------------------------------------------------------------ CPU: the test's own arithmetic
def test_planted_positions_cover_every_loop_boundary():
    slabs = _slabs()
    for V in V_LIST:
        pos = _positions(V, slabs)
        assert 2 <= len(pos) < 40 and len(set(pos)) == len(pos) and all(0 <= p < V for p in pos), V
    assert _positions(4, slabs) == [0, 3] and _positions(8, slabs) == [0, 3, 4, 7]
    per, bounds = _slab_bounds(V_LARGE, slabs)
    pos = set(_positions(V_LARGE, slabs))
    i0, i1 = bounds[1]
    assert per > 1024 + 1 and i1 - i0 == per                                  # the unrolled trip runs for all 256 threads, then the stride loop
    assert {4 * i0 - 1, 4 * i0, 4 * (i0 + 767), 4 * (i0 + 768), 4 * (i0 + 1024), 4 * (i1 - 1)} <= pos
    i0, i1 = bounds[-1]
    assert 768 < i1 - i0 < 1024 and 4 * i1 == V_LARGE and 4 * (i1 - 1) in pos    # short last slab: positions past it were clipped into it
    assert sum(a >= b for a, b in _slab_bounds(1020, slabs)[1]) == 1             # one empty slab
    assert sum(a >= b for a, b in _slab_bounds(1028, slabs)[1]) == slabs - 129   # per = 2: slabs from 129 on are empty
    x, pos = _planted(1028, slabs)
    assert (x.min(axis=1) == -1).all() and (x.max(axis=1) == 2).all() and ((x == -1).sum(axis=1) == 1).all()


def test_oracle_rescale_of_the_exact_inputs():
    slabs = _slabs()
    x, _ = _planted(1028, slabs)
    for lo, hi in RANGES:
        y = data_ref.rescale_intensity(x[3], lo, hi)
        assert y.dtype == np.float32 and y.min() == np.float32(lo) and y.max() == np.float32(hi)      # (-1 - -1) / 3 and (2 - -1) / 3 are exact
        c = np.full(8, 5, np.float32)
        assert np.array_equal(data_ref.rescale_intensity(c, lo, hi), c)


# ------------------------------------------------------------------------------------------------ 1. min / max
@pytest.mark.gpu
@pytest.mark.parametrize("V", V_LIST)
def test_minmax_finds_an_extremum_at_every_loop_boundary(dev, V):
    from gaviko_amd import ops
    slabs = _slabs()
    xh, pos = _planted(V, slabs)
    B = len(pos)
    x = torch.from_numpy(xh).to(dev)
    part = ops.minmax_partials(B, dev).fill_(float("nan"))
    ops.volume_minmax(x, part)
    y = torch.empty_like(x)
    mm = torch.full((2 * B,), float("nan"), device=dev)
    ops.rescale_intensity(x, part, y, minmax=mm)
    p3 = part.view(B, slabs, 2)
    want = torch.tensor([[-1.0, 2.0]] * B)
    assert torch.equal(mm.cpu().view(B, 2), want), (V, pos, mm.cpu().view(B, 2))
    assert torch.equal(torch.stack([p3[:, :, 0].min(dim=1).values, p3[:, :, 1].max(dim=1).values], dim=1).cpu(), want), (V, pos)
    # every slab's own pair: min and max are exact, so each partial equals numpy's over that slab; an empty slab holds (+inf, -inf)
    ph = p3.cpu().numpy()
    _, bounds = _slab_bounds(V, slabs)
    for s, (i0, i1) in enumerate(bounds):
        if i0 >= i1:
            assert (ph[:, s, 0] == np.inf).all() and (ph[:, s, 1] == -np.inf).all(), (V, s)
        else:
            seg = xh[:, 4 * i0: 4 * i1]
            assert np.array_equal(ph[:, s, 0], seg.min(axis=1)) and np.array_equal(ph[:, s, 1], seg.max(axis=1)), (V, s)


# ------------------------------------------------------------------------------------------------ 2. rescale
@pytest.mark.gpu
@pytest.mark.parametrize("V", V_LIST + [V_CAPPED])
def test_rescale_bit_exact_every_size_and_range(dev, V):
    from gaviko_amd import ops
    slabs = _slabs()
    if V == V_CAPPED:                                                     # not a section-1 size: plant at its ends
        planted = _base(V).copy()
        planted[V - 1], planted[0] = -1.0, 2.0
    else:
        planted = _planted(V, slabs)[0][-1]
    g = _gauss(V, 7)
    xh = np.stack([g, -g, np.full(V, 5, np.float32), planted])
    B = len(xh)
    x = torch.from_numpy(xh).to(dev)
    part = ops.minmax_partials(B, dev).fill_(float("nan"))
    ops.volume_minmax(x, part)
    for lo, hi in RANGES:
        full, y = _with_sentinels(B * V, dev)
        y = y.view(B, V)
        mm = torch.full((2 * B,), float("nan"), device=dev)
        ops.rescale_intensity(x, part, y, lo, hi, minmax=mm)
        yh = y.cpu().numpy()
        for b in range(B):
            assert np.array_equal(yh[b], data_ref.rescale_intensity(xh[b], lo, hi)), (V, lo, hi, b)
        assert np.array_equal(yh[2], xh[2])                               # the constant volume comes back unchanged
        assert np.array_equal(mm.cpu().numpy().reshape(B, 2), np.stack([xh.min(axis=1), xh.max(axis=1)], axis=1)), (V, lo, hi)
        assert _sentinels_intact(full, B * V), (V, lo, hi)
    full, y = _with_sentinels(B * V, dev)                                 # without the minmax pointer
    ops.rescale_intensity(x, part, y.view(B, V))
    assert np.array_equal(y.view(B, V).cpu().numpy()[0], data_ref.rescale_intensity(xh[0])) and _sentinels_intact(full, B * V)


@pytest.mark.gpu
def test_volume_size_no_multiple_of_four_is_refused(dev):
    from gaviko_amd import data, lib, ops
    x = torch.arange(12, dtype=torch.float32, device=dev).view(2, 6)
    part = ops.minmax_partials(2, dev).fill_(0.0)
    y = torch.full_like(x, SENTINEL)
    with pytest.raises(lib.GavikoHipError, match="gvk_volume_minmax.*multiple of 4"):
        ops.volume_minmax(x, part)
    with pytest.raises(lib.GavikoHipError, match="gvk_rescale_intensity.*multiple of 4"):
        ops.rescale_intensity(x, part, y)
    with pytest.raises(lib.GavikoHipError, match="gvk_volume_minmax.*multiple of 4"):
        data.eval_transforms()(torch.zeros(1, 1, 5, 7, 13, device=dev))
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all().item()) and bool((part == 0).all().item())      # refused before any launch


# ------------------------------------------------------------------------------------------------ 3. spatial transform
SHAPES = [(1, 1, 1), (2, 3, 5), (5, 4, 64), (3, 5, 65), (4, 7, 130), (7, 9, 63), (6, 2, 129), (3, 6, 160)]
OFFSET = 7.0                                                              # the minimum (= the pad value) is not 0


def _perm_vols(shape, B, seed=0):
    """[B][D][H][W]: each a permutation of arange(V) + OFFSET, so every voxel of a volume is distinct (and exact in float32)"""
    V = int(np.prod(shape))
    r = np.random.default_rng(seed + 31 * V)
    return np.stack([(r.permutation(V).astype(np.float32) + np.float32(OFFSET)).reshape(shape) for _ in range(B)])


def _gather_maps(shape):
    """(A, t): signed permutation matrices with integer translations -- the identity, each axis reflected about the volume, two axis swaps,
    a cyclic shift of the axes, translations that push the grid out on each side of each axis, and two combinations"""
    D, H, W = shape
    I = np.eye(3, dtype=np.int64)
    maps = [(I, (0, 0, 0))]
    for k in range(3):
        A, t = I.copy(), [0, 0, 0]
        A[k, k], t[k] = -1, shape[k] - 1
        maps.append((A, tuple(t)))
    maps += [(I[[1, 0, 2]], (0, 0, 0)), (I[[0, 2, 1]], (0, 0, 0)), (I[[2, 0, 1]], (0, 0, 0))]
    for k in range(3):
        for sgn in (1, -1):
            t = [0, 0, 0]
            t[k] = sgn * (k + 1)
            maps.append((I, tuple(t)))
    maps += [(I, (1, -1, 2)), (-I, (D, H - 1, W - 3)), (I[[0, 2, 1]], (-1, 2, 1))]
    return maps


def _source_index(shape, A, t, bits):
    """(p [D][H][W][3] clipped into the volume, inside [D][H][W]): p = A q + t with q the output index mirrored along the axes of `bits`"""
    shape = np.array(shape)
    idx = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    q = np.stack([shape[k] - 1 - idx[k] if bits & (1 << k) else idx[k] for k in range(3)], axis=-1)
    p = q @ np.asarray(A).T + np.asarray(t)
    return np.clip(p, 0, shape - 1), ((p >= 0) & (p < shape)).all(axis=-1)


def _gather(vol, A, t, bits):
    """out[z, y, x] = vol[A q + t], vol.min() where A q + t is outside"""
    p, inside = _source_index(vol.shape, A, t, bits)
    return np.where(inside, vol[p[..., 0], p[..., 1], p[..., 2]], vol.min()).astype(np.float32)


def _gather_cases(shape):
    """(vols [B], mats [B][3][4] float32, flags [B], the (A, t, bits) of every entry): every map with every flip"""
    cases = [(A, t, bits) for A, t in _gather_maps(shape) for bits in range(8)]
    mats = np.stack([np.concatenate([A, np.asarray(t)[:, None]], axis=1) for A, t, _ in cases]).astype(np.float32)
    flags = np.array([8 | bits for _, _, bits in cases], dtype=np.int32)
    return _perm_vols(shape, len(cases), seed=1), mats, flags, cases


GENERAL = [((1.05, 0.93, 1.08), (11.0, -7.0, 14.0)), ((0.9, 1.1, 1.0), (-15.0, 15.0, 3.0)), ((1.0, 1.0, 1.0), (0.0, 0.0, 12.0))]
GENERAL_FLAGS = [8, 9, 8 | 6]                                             # of test_data_metrics.py::test_spatial_transform_vs_oracle


@pytest.mark.parametrize("shape", SHAPES)
def test_gather_reference_equals_the_oracle(shape):
    """CPU: at integer coordinates the oracle's trilinear weights are exactly 0 and 1, so it must return the plain gather."""
    vols, mats, flags, cases = _gather_cases(shape)
    outside = 0
    for b, (A, t, bits) in enumerate(cases):
        want = _gather(vols[b], A, t, bits)
        assert np.array_equal(want, data_ref.spatial(vols[b], mats[b], bits)), (shape, b)
        outside += int(not _source_index(shape, A, t, bits)[1].all())
    assert outside >= 6 * 8                                               # each of the six one-axis translations pushes voxels outside
    for bits in range(8):
        assert np.array_equal(_gather(vols[bits], np.eye(3, dtype=np.int64), (0, 0, 0), bits), data_ref.flip(vols[bits], bits))


def _spatial_partials(x, poison=False):
    """the (min, max) table of x: the kernel's where it can run (V a multiple of 4); otherwise one slab per volume holds the pair and
    the others are empty.  poison: NaN everywhere (for entries that must not read it)."""
    from gaviko_amd import ops
    B = x.shape[0]
    part = ops.minmax_partials(B, x.device)
    if poison:
        return part.fill_(float("nan"))
    if (x.numel() // B) % 4 == 0:
        ops.volume_minmax(x, part)
        return part
    p3 = part.view(B, -1, 2)
    p3[:, :, 0], p3[:, :, 1] = float("inf"), float("-inf")
    rows, slab = torch.arange(B, device=x.device), (7 * torch.arange(B, device=x.device) + 3) % p3.shape[1]
    flat = x.reshape(B, -1)
    p3[rows, slab, 0], p3[rows, slab, 1] = flat.min(dim=1).values, flat.max(dim=1).values
    return part


def _run_spatial(dev, vols, mats, flags, poison=False):
    from gaviko_amd import ops
    x = torch.from_numpy(vols).to(dev)
    full, out = _with_sentinels(x.numel(), dev)
    ops.spatial_transform(x, out.view(x.shape), torch.from_numpy(mats).to(dev), torch.from_numpy(flags).to(dev), _spatial_partials(x, poison))
    assert _sentinels_intact(full, x.numel()), vols.shape
    return out.view(x.shape).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_spatial_flips_are_exact_and_read_no_matrix(dev, shape):
    vols = _perm_vols(shape, 8)
    out = _run_spatial(dev, vols, np.full((8, 3, 4), np.nan, np.float32), np.arange(8, dtype=np.int32), poison=True)
    for bits in range(8):
        assert np.array_equal(out[bits], data_ref.flip(vols[bits], bits)), (shape, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_spatial_integer_affines_are_exact_gathers(dev, shape):
    vols, mats, flags, cases = _gather_cases(shape)
    out = _run_spatial(dev, vols, mats, flags)
    for b, (A, t, bits) in enumerate(cases):
        assert np.array_equal(out[b], _gather(vols[b], A, t, bits)), (shape, A.tolist(), t, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_spatial_general_affine_vs_oracle(dev, shape):
    from gaviko_amd import data
    vols = _perm_vols(shape, len(GENERAL), seed=2)
    mats = np.stack([data.affine_matrix(s, d, (0, 0, 0), shape).astype(np.float32) for s, d in GENERAL])
    flags = np.array(GENERAL_FLAGS, dtype=np.int32)
    out = _run_spatial(dev, vols, mats, flags)
    for b in range(len(GENERAL)):
        want = data_ref.spatial(vols[b], mats[b], int(flags[b] & 7))
        assert np.abs(out[b] - want).max() < 1e-3 * np.abs(vols[b]).max(), (shape, b)


@pytest.mark.gpu
def test_spatial_in_place_is_refused(dev):
    from gaviko_amd import lib, ops
    x = torch.from_numpy(_perm_vols((2, 3, 5), 1)).to(dev)
    keep = x.clone()
    with pytest.raises(lib.GavikoHipError, match="in-place"):
        ops.spatial_transform(x, x, torch.zeros(1, 3, 4, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), _spatial_partials(x, poison=True))
    assert torch.equal(x, keep)


# ------------------------------------------------------------------------------------------------ 4. gvk_sumsq
SUMSQ_N = [1, 2, 3, 4, 5, 1023, 1024, 1025, 262143, 262144, 262145, 262147, 524290, 786435]


def _small_ints(n):
    """int64 [n] from {+-1, +-2, +-3}: no zeros, and 9 n < 2^24, so every partial sum of squares is an integer fp32 holds exactly"""
    r = np.random.default_rng(5000 + n)
    return r.integers(1, 4, n) * (2 * r.integers(0, 2, n) - 1)


def test_sumsq_inputs_make_fp32_exact():
    for n in SUMSQ_N:
        v = _small_ints(n)
        assert v.dtype == np.int64 and v.min() >= -3 and v.max() <= 3 and (v != 0).all() and 9 * n < 2 ** 24
    v = _small_ints(786435)
    assert {-3, -2, -1, 1, 2, 3} == set(np.unique(v).tolist())
    acc = np.float32(0)
    for s in np.add.reduceat((v * v).astype(np.float32), np.arange(0, len(v), 1024)):      # fp32 sums of fp32 pieces: still the integer
        acc = np.float32(acc + s)
    assert int(acc) == int((v * v).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_is_exact_on_small_integers(dev, n):
    from gaviko_amd import lib
    v = _small_ints(n)
    x = torch.from_numpy(v.astype(np.float32)).to(dev)
    assert x.data_ptr() % 16 == 0 and x.numel() == n
    want = torch.tensor([float(int((v * v).sum()))], dtype=torch.float32)
    scratch = torch.full((256,), float("nan"), device=dev)                # the final kernel adds all 256: an unwritten partial shows
    outs = []
    for _ in range(2):
        out = torch.full((1,), float("nan"), device=dev)
        lib.check(lib.load().gvk_sumsq(lib.ptr(x), n, lib.ptr(scratch), lib.ptr(out), lib.stream_ptr()), "gvk_sumsq")
        outs.append(out.cpu())
    assert torch.equal(outs[0], want), (n, outs[0].item(), want.item())
    assert torch.equal(outs[1], outs[0]), (n, outs[1].item())
    assert torch.equal(x.cpu(), torch.from_numpy(v.astype(np.float32)))   # the input is only read
