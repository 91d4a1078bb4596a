"""-m gpu: the GEMM epilogues whose residual / GELU' tile is requested by the main loop (EpiPrefetch in csrc/gemm_epilogue.hpp):
BIAS_RES_F32 (1), BIAS_RES_F32_BF16 (6) and GELU_BWD_BF16 (4) on the three- / four-stage 4-wave tiles and the eight-phase 256 x 256 tile.

Reference: float64 torch evaluation of the same epilogue on the bf16-rounded operands; tolerances are those of
tests/test_kernels_gpu.py::test_gemm_epilogues (3e-4 absolute on the fp32 output at these operand scales, 2^-7 of the largest value on
the bf16 copy, 2^-6 of the largest value on the GELU-backward output).  The row-statistic partials of epilogue 6 are 64-term fp32 sums of
the stored fp32 values: bound (64 + 3) 2^-24 sum|terms| (the forward bound of a recursive fp32 sum), terms taken from the kernel's own output.

Every operand the epilogue reads or writes sits at its exact size in a larger buffer filled with a sentinel, rows at a pitch larger than N:
whatever the launch may not write -- the halo, the pitch gaps, rows past M, rows outside the row panels -- must keep its bits.
Shapes the launcher refuses (N = 136: N must be a multiple of 64; K = 64 or N = 128 on the eight-phase tile; epilogue 6 there) must be
refused with an error and leave the outputs untouched.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SENT = -776.0            # exact in bf16 and fp32
HALO = 256               # elements in front of and behind every boxed operand (keeps 16-byte alignment for both dtypes)
MS = (1, 127, 129, 257)
NS = (128, 136, 768)
KS = (64, 128, 192, 832)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _bf16_round(x):
    return x.to(torch.bfloat16).float()


class Box:
    """rows x cols at pitch ld, exactly (rows - 1) ld + cols elements, inside a sentinel-filled buffer."""

    def __init__(self, rows, cols, ld, dtype, dev, data=None):
        self.rows, self.cols, self.ld = rows, cols, ld
        n = (rows - 1) * ld + cols
        self.buf = torch.full((HALO + n + HALO,), SENT, dtype=dtype, device=dev)
        self.t = self.buf[HALO:HALO + n]                       # what the launcher gets: contiguous, exact size
        if data is not None:
            self.mat().copy_(data.to(dev).to(dtype))
        self.before = self.buf.clone()

    def mat(self):
        return torch.as_strided(self.t, (self.rows, self.cols), (self.ld, 1))

    def untouched_outside(self, written_rows):
        """bit-equal to the state before the launch everywhere except the given rows x cols"""
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        m = torch.as_strided(keep[HALO:HALO + self.t.numel()], (self.rows, self.cols), (self.ld, 1))
        m[written_rows.to(self.buf.device)] = False
        it = torch.int32 if self.buf.dtype == torch.float32 else torch.int16
        return bool((self.buf.view(it)[keep] == self.before.view(it)[keep]).all())


_OPERANDS = {}
_LAST = {}               # the boxes of the latest launch, reachable when the launcher refuses it


def _operands(M, N, K):
    """bf16-rounded operands and the float64 product, computed once per shape and shared by every case"""
    key = (M, N, K)
    if key not in _OPERANDS:
        a = _bf16_round(_rand((M, K), 11))
        w = _bf16_round(_rand((N, K), 12, 2 / math.sqrt(K)))
        bias = _rand((N,), 13, 0.2)
        res = _rand((M, N), 14)
        pre = _bf16_round(_rand((M, N), 15, 3.0))             # GELU pre-activations / derivatives as the forward stores them (bf16)
        _OPERANDS[key] = (a, w, bias, res, pre, a.double() @ w.double().T)
    return _OPERANDS[key]


def _gelu_grad64(x):
    x = x.clone().requires_grad_(True)
    torch.nn.functional.gelu(x).sum().backward()
    return x.grad


def _launch(dev, epi, tile, M, N, K, *, inplace=False, panels=None, aux_is_grad=0, with_stats=True):
    """One launch with boxed operands.  Returns (boxes, written rows, float64 reference rows, extras)."""
    from gaviko_amd import ops
    a, w, bias, res, pre, prod = _operands(M, N, K)
    A = ops.act_zeros(M, K, torch.bfloat16, dev)
    A[:M] = a.to(dev).bfloat16()
    W = w.to(dev).bfloat16().contiguous()
    ldo = N + 8
    ldres = ldo if inplace else N + 12
    ldaux = N + 16
    rows = torch.zeros(M, dtype=torch.bool)
    if panels is None:
        rows[:] = True
        kw = {}
    else:
        mp, ms = panels
        for q in range(mp):
            rows[q * ms: q * ms + 64] = True
        kw = dict(m_panels=mp, m_stride=ms)
    out = {}
    if epi in (ops.EPI_BIAS_RES_F32, ops.EPI_BIAS_RES_F32_BF16):
        o = Box(M, N, ldo, torch.float32, dev, data=res if inplace else None)
        r = o if inplace else Box(M, N, ldres, torch.float32, dev, data=res)
        out["out"], out["res"] = o, r
        kw.update(bias=bias.to(dev), res=r.t, ldres=ldres)
        want = prod + bias.double() + res.double()
        if epi == ops.EPI_BIAS_RES_F32_BF16:
            o16 = Box(M, N, ldo, torch.bfloat16, dev)
            out["out16"] = o16
            kw.update(out1=o16.t)
            if with_stats and N % 128 == 0 and tile % 1000 in (0, 128):
                out["part"] = torch.full(((N // 64) * M * 2,), SENT, device=dev)
                out["pivot"] = _rand((M,), 16, 0.5).to(dev)
                kw.update(stat_part=out["part"], stat_pivot=out["pivot"])
    else:
        o = Box(M, N, ldo, torch.bfloat16, dev)
        x = Box(M, N, ldaux, torch.bfloat16, dev, data=pre)
        out["out"], out["aux"] = o, x
        kw.update(aux=x.t, ldaux=ldaux, aux_is_grad=aux_is_grad)
        want = prod * (pre.double() if aux_is_grad else _gelu_grad64(pre.double()))
    _LAST.clear()
    _LAST.update(out)
    ops.gemm_nt(A, W, M, out["out"].t, epilogue=epi, ldo=ldo, tile=tile, N=N, K=K, **kw)
    torch.cuda.synchronize()
    return out, rows, want


def _check(ops, epi, out, rows, want, M, N):
    got = out["out"].mat().cpu().double()
    w = want[rows]
    if epi == ops.EPI_GELU_BWD_BF16:
        assert (got[rows] - w).abs().max().item() < 2 ** -6 * w.abs().max().item()
        assert out["aux"].untouched_outside(torch.zeros(M, dtype=torch.bool)), "aux is read-only"
    else:
        assert (got[rows] - w).abs().max().item() < 3e-4
        if out["res"] is not out["out"]:
            assert out["res"].untouched_outside(torch.zeros(M, dtype=torch.bool)), "res is read-only when it is not the output"
        if epi == ops.EPI_BIAS_RES_F32_BF16:
            g16 = out["out16"].mat()
            assert (g16.cpu().double()[rows] - w).abs().max().item() < 2 ** -7 * w.abs().max().item()
            assert torch.equal(g16[rows.to(g16.device)], out["out"].mat()[rows.to(g16.device)].bfloat16()), "the bf16 copy is the rounding of the fp32 rows"
            assert out["out16"].untouched_outside(rows)
            if "part" in out:
                part = out["part"].view(N // 64, M, 2).cpu().double()
                dv = (got - out["pivot"].cpu().double()[:, None]).view(M, N // 64, 64).permute(1, 0, 2)
                s1, s2 = dv.sum(-1), (dv * dv).sum(-1)
                b1 = 67 * 2.0 ** -24 * dv.abs().sum(-1) + 1e-30
                b2 = 67 * 2.0 ** -24 * s2 + 1e-30
                assert ((part[..., 0] - s1).abs()[:, rows] <= b1[:, rows]).all()
                assert ((part[..., 1] - s2).abs()[:, rows] <= b2[:, rows]).all()
                assert (out["part"].view(N // 64, M, 2)[:, ~rows.to(out["part"].device)] == SENT).all(), "statistics of rows that are not computed"
    assert out["out"].untouched_outside(rows), "halo, pitch gaps, rows past M or outside the panels were written"


def _same_bits(a, b):
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return bool((a.view(it) == b.view(it)).all())


def _accepts(ops, epi, tile, N, K):
    """what gvk_gemm_nt_bf16 documents: N a multiple of 64 and of the tile's columns; the eight-phase tile: N % 256, K >= 128, no epilogue 6"""
    if N % 64 != 0:
        return False
    if tile == 8256256:
        return N % 256 == 0 and K >= 128 and epi != ops.EPI_BIAS_RES_F32_BF16
    return N % (tile % 1000) == 0


# tile codes: three-stage 128 / 96 / 64 x 128, four-stage 64 x 128, the eight-phase 256 x 256 kernel
@pytest.mark.parametrize("tile", [3128128, 8256256, 3096128, 3064128, 4064128])
@pytest.mark.parametrize("epi_name", ["EPI_BIAS_RES_F32", "EPI_GELU_BWD_BF16", "EPI_BIAS_RES_F32_BF16"])
def test_prefetched_epilogue_against_fp64(dev, epi_name, tile):
    from gaviko_amd import lib, ops
    epi = getattr(ops, epi_name)
    # the two tile kernels of the backbone get every shape; the other touched forms the shapes at which their loops differ (one k-tile,
    # fewer k-tiles than stages, more) on a ragged M
    ms = MS if tile in (3128128, 8256256) else (129,)
    ran = 0
    for M in ms:
        for N in NS:
            for K in KS:
                if not _accepts(ops, epi, tile, N, K):
                    with pytest.raises(lib.GavikoHipError):
                        _launch(dev, epi, tile, M, N, K)
                    torch.cuda.synchronize()
                    assert all(b.untouched_outside(torch.zeros(M, dtype=torch.bool)) for b in _LAST.values() if isinstance(b, Box))
                    continue
                out, rows, want = _launch(dev, epi, tile, M, N, K, aux_is_grad=(K // 64) & 1)
                _check(ops, epi, out, rows, want, M, N)
                again, _, _ = _launch(dev, epi, tile, M, N, K, aux_is_grad=(K // 64) & 1)
                assert _same_bits(out["out"].buf, again["out"].buf), "two launches differ"
                ran += 1
    assert ran > 0 or (tile == 8256256 and epi == ops.EPI_BIAS_RES_F32_BF16)


@pytest.mark.parametrize("tile", [3128128, 8256256, 4064128])
@pytest.mark.parametrize("epi_name", ["EPI_BIAS_RES_F32", "EPI_BIAS_RES_F32_BF16"])
def test_prefetched_residual_in_place(dev, epi_name, tile):
    """res aliases out0 (the engine's residual stream): a workgroup reads its tile early and writes it late, nobody else touches it"""
    from gaviko_amd import ops
    epi = getattr(ops, epi_name)
    for M in MS:
        for N, K in ((768, 64), (768, 192), (768, 832), (128, 128)):
            if not _accepts(ops, epi, tile, N, K):
                continue
            out, rows, want = _launch(dev, epi, tile, M, N, K, inplace=True)
            _check(ops, epi, out, rows, want, M, N)
            sep, _, _ = _launch(dev, epi, tile, M, N, K, inplace=False)
            assert torch.equal(out["out"].mat(), sep["out"].mat()), "in place and out of place differ"


@pytest.mark.parametrize("M", [257, 150])
@pytest.mark.parametrize("epi_name", ["EPI_BIAS_RES_F32", "EPI_GELU_BWD_BF16", "EPI_BIAS_RES_F32_BF16"])
def test_prefetched_epilogue_on_row_panels(dev, epi_name, M):
    """m_panels = 2, 64-row panels at m_stride = 129 (the launcher's own choice of tile: four-stage 64 x 128): rows 0..63 and 129..192 are
    computed, at M = 150 the second panel ends at row 149; every other row keeps the sentinel bit for bit.  The computed rows carry the
    bits of the full launch on the same tile."""
    from gaviko_amd import ops
    epi = getattr(ops, epi_name)
    for N in (128, 768):
        for K in KS:
            for inplace in ((False, True) if epi != ops.EPI_GELU_BWD_BF16 else (False,)):
                out, rows, want = _launch(dev, epi, 0, M, N, K, panels=(2, 129), inplace=inplace, aux_is_grad=1)
                _check(ops, epi, out, rows, want, M, N)
                full, _, _ = _launch(dev, epi, 4064128, M, N, K, aux_is_grad=1)
                r = rows.to(dev)
                assert _same_bits(out["out"].mat()[r].contiguous(), full["out"].mat()[r].contiguous())


@pytest.mark.parametrize("tile", [3128128, 8256256, 4064128])
def test_prefetch_leaves_the_arithmetic_alone(dev, tile):
    """The same tile kernel with the plain fp32 store gives the accumulators; the fused epilogues must be bit for bit
    (acc + bias) + res, its bf16 rounding, and bf16(acc * aux) -- operations, order and rounding as before, only the load moved."""
    from gaviko_amd import ops
    for M, N, K in ((257, 768, 832), (129, 768, 128), (127, 256, 192)):
        a, w, bias, res, pre, _ = _operands(M, N, K)
        A = ops.act_zeros(M, K, torch.bfloat16, dev)
        A[:M] = a.to(dev).bfloat16()
        W = w.to(dev).bfloat16().contiguous()
        acc_b = torch.zeros((M, N), device=dev)
        acc = torch.zeros((M, N), device=dev)
        ops.gemm_nt(A, W, M, acc_b, epilogue=ops.EPI_STORE_F32, bias=bias.to(dev), tile=tile)
        ops.gemm_nt(A, W, M, acc, epilogue=ops.EPI_STORE_F32, tile=tile)
        want = acc_b + res.to(dev)
        out, _, _ = _launch(dev, ops.EPI_BIAS_RES_F32, tile, M, N, K)
        assert _same_bits(out["out"].mat().contiguous(), want)
        if tile != 8256256:
            out, _, _ = _launch(dev, ops.EPI_BIAS_RES_F32_BF16, tile, M, N, K)
            assert _same_bits(out["out"].mat().contiguous(), want)
            assert _same_bits(out["out16"].mat().contiguous(), want.bfloat16())
        out, _, _ = _launch(dev, ops.EPI_GELU_BWD_BF16, tile, M, N, K, aux_is_grad=1)
        assert _same_bits(out["out"].mat().contiguous(), (acc * pre.to(dev)).bfloat16())
