"""-m gpu: the input-gradient kernels (csrc/input_grad.hip) against float64, outputs sentinel-filled to catch stray or missing writes:
the un-patchify (the inverse of patchify, with the attribution arithmetic), the patch-grid reduction and the two steps of the EVP
high-pass backward (the modulus, then the adjoint of the linear part)."""
import numpy as np
import pytest
import torch

from gaviko_amd import lib as L
from gaviko_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = float("nan")
# (B, volume, patch): the fixtures' patch (12, 16, 16) and an anisotropic one with pw = 4
SHAPES = [(1, (24, 32, 32), (12, 16, 16)), (3, (24, 32, 32), (12, 16, 16)), (3, (8, 12, 16), (2, 4, 4)), (2, (120, 160, 160), (12, 16, 16))]


def _vol(g, B, shape, dev):
    return torch.randn((B, 1) + shape, generator=g, dtype=torch.float64).float().to(dev)


def _cols_ref(x, patch):
    """float64 im2col of [B,1,D,H,W] -> [B*N, pd*ph*pw] (patchify's layout)."""
    B, _, D, H, W = x.shape
    pd, ph, pw = patch
    v = x.double().reshape(B, D // pd, pd, H // ph, ph, W // pw, pw).permute(0, 1, 3, 5, 2, 4, 6)
    return v.reshape(-1, pd * ph * pw)


@pytest.mark.parametrize("B,shape,patch", SHAPES)
def test_unpatchify_inverts_patchify_bitwise(dev, B, shape, patch):
    g = torch.Generator().manual_seed(1)
    x = _vol(g, B, shape, dev)
    n = B * int(np.prod(shape))
    cols = ops.act_zeros(n // int(np.prod(patch)), int(np.prod(patch)), torch.float32, dev)
    ops.patchify(x, cols, patch)
    out = torch.full_like(x, SENTINEL)
    ops.unpatchify(cols, out, patch)
    torch.cuda.synchronize()
    assert torch.equal(out, x)


@pytest.mark.parametrize("B,shape,patch", SHAPES[:3])
def test_unpatchify_attribution_arithmetic_against_float64(dev, B, shape, patch):
    """out = beta out + sum_j alpha G_j (x - x0) for nsum = 1 and 3, beta 0 (the sentinel is never read) and 0.5, with / without x, x0."""
    g = torch.Generator().manual_seed(2)
    K = int(np.prod(patch))
    for nsum in (1, 3):
        G = _vol(g, B * nsum, shape, dev)
        cols = _cols_ref(G, patch).float().contiguous()
        x, x0, prev = _vol(g, B, shape, dev), _vol(g, B, shape, dev), _vol(g, B, shape, dev)
        Gd = G.double().view(B, nsum, 1, *shape)
        for alpha, beta, use_x, use_x0 in ((1.0, 0.0, False, False), (0.25, 0.0, True, False), (-0.5, 0.5, True, True), (1.0 / 3, 1.0, False, False)):
            out = torch.full_like(x, SENTINEL) if beta == 0 else prev.clone()
            ops.unpatchify(cols, out, patch, x=x if use_x else None, x0=x0 if (use_x and use_x0) else None, alpha=alpha, beta=beta, nsum=nsum)
            fac = 1.0
            if use_x:
                fac = x.double() - (x0.double() if use_x0 else 0.0)
            want = beta * prev.double() + alpha * Gd.sum(1) * fac if beta != 0 else alpha * Gd.sum(1) * fac
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            err = (out.double() - want).abs().max().item() / max(1.0, want.abs().max().item())
            assert err < 4 * nsum * 2 ** -23, (nsum, alpha, beta, use_x, use_x0, err)
        assert cols.shape[1] == K


def test_unpatchify_split_sum_is_bitwise_the_one_call_sum(dev):
    """Summing 4 samples in one call or as 1 + 3 (beta = 1 for the second) gives the same bits: the sum is one FMA per step, in order."""
    g = torch.Generator().manual_seed(3)
    shape, patch = (24, 32, 32), (12, 16, 16)
    G = _vol(g, 4, shape, dev)
    cols = _cols_ref(G, patch).float().contiguous()
    x = _vol(g, 1, shape, dev)
    a = torch.full_like(x, SENTINEL)
    ops.unpatchify(cols, a, patch, x=x, alpha=0.25, nsum=4)
    b = torch.full_like(x, SENTINEL)
    rows = cols.shape[0] // 4
    ops.unpatchify(cols, b, patch, x=x, alpha=0.25, nsum=1)
    ops.unpatchify(cols[rows:], b, patch, x=x, alpha=0.25, beta=1.0, nsum=3)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("B,shape,patch", SHAPES)
def test_patch_reduce_against_float64(dev, B, shape, patch):
    g = torch.Generator().manual_seed(4)
    v = _vol(g, B, shape, dev)
    grid = tuple(s // p for s, p in zip(shape, patch))
    cols = _cols_ref(v, patch).view(B, *grid, -1)
    for absval in (True, False):
        out = torch.full((B,) + grid, SENTINEL, device=dev)
        ops.patch_reduce(v, out, patch, absval=absval)
        want = (cols.abs() if absval else cols).sum(-1)
        torch.cuda.synchronize()
        err = (out.double().cpu() - want.cpu()).abs().max().item()
        assert err < 2 * int(np.prod(patch)) * 2 ** -24 * max(1.0, cols.abs().sum(-1).max().item()), (absval, err)


def _highpass(D, H, W, freq=0.25):
    from gaviko_amd.engine import evp_highpass_operator
    hp, dm = evp_highpass_operator(D, H, W, freq)
    return hp, dm


@pytest.mark.parametrize("B,D,H,W", [(1, 120, 160, 160), (2, 64, 64, 32)])
def test_evp_highpass_backward_steps_against_float64(dev, B, D, H, W):
    """sign step: dout o sign(hp . x) on the filtered slices, dout o sign(x) elsewhere; linear step with hp^T: <H x, y> = <x, H^T y> to fp64
    precision, and both against float64."""
    g = torch.Generator().manual_seed(5)
    hp, dm = _highpass(D, H, W)
    assert 0 < int(np.asarray(dm).sum()) < D                     # both kinds of slice occur
    hpd = torch.from_numpy(np.asarray(hp, np.float64))
    dmask = torch.from_numpy(np.asarray(dm, np.int32)).to(dev)
    hp32, hpT32 = hpd.float().to(dev), hpd.t().contiguous().float().to(dev)
    x, y, dout = _vol(g, B, (D, H, W), dev), _vol(g, B, (D, H, W), dev), _vol(g, B, (D, H, W), dev)
    filt = torch.from_numpy(np.asarray(dm) != 0).view(1, 1, D, 1, 1)
    hx64 = torch.where(filt, torch.einsum("ik,bcdkj->bcdij", hp32.double().cpu(), x.double().cpu()), x.double().cpu())
    # sign step (where |hp . x| is far from 0 the sign is unambiguous in fp32)
    s = torch.full_like(x, SENTINEL)
    ops.evp_highpass_sign(x, hp32, dmask, dout, s)
    want = dout.double().cpu() * torch.sign(hx64)
    clear = hx64.abs() > 1e-4
    torch.cuda.synchronize()
    assert torch.isfinite(s).all()
    assert torch.equal(s.double().cpu()[clear], want[clear])
    # linear step, plain and accumulating, and the adjoint identity
    hx = torch.full_like(x, SENTINEL)
    ops.evp_highpass_linear(x, hp32, dmask, hx)
    hty = y.clone()
    ops.evp_highpass_linear(y, hpT32, dmask, hty, accumulate=False)
    acc = dout.clone()
    ops.evp_highpass_linear(y, hpT32, dmask, acc, accumulate=True)
    torch.cuda.synchronize()
    tol = 8 * H * 2 ** -24 * max(1.0, hx64.abs().max().item())
    assert (hx.double().cpu() - hx64).abs().max().item() < tol
    hty64 = torch.where(filt, torch.einsum("ki,bcdkj->bcdij", hp32.double().cpu(), y.double().cpu()), y.double().cpu())
    assert (hty.double().cpu() - hty64).abs().max().item() < tol
    assert (acc.double().cpu() - (dout.double().cpu() + hty64)).abs().max().item() < 2 * tol
    lhs = (hx.double() * y.double()).sum().item()
    rhs = (x.double() * hty.double()).sum().item()
    scale = (hx.double().abs() * y.double().abs()).sum().item()
    assert abs(lhs - rhs) < 1e-5 * scale, (lhs, rhs)


def test_input_grad_kernels_reject_bad_arguments(dev):
    x = torch.zeros((1, 1, 24, 32, 32), device=dev)
    cols = torch.zeros((8, 12 * 16 * 16), device=dev)
    with pytest.raises(L.GavikoHipError):
        ops.unpatchify(cols[:1], x, (12, 16, 16))                       # too few rows
    with pytest.raises(L.GavikoHipError):
        ops.unpatchify(cols, x, (12, 16, 16), x0=x)                     # x0 without x
    with pytest.raises(L.GavikoHipError):
        ops.patch_reduce(x, torch.zeros(1, device=dev), (12, 16, 16))  # output too small
    with pytest.raises(L.GavikoHipError):
        ops.unpatchify(torch.zeros((16, 2 * 4 * 6), device=dev), torch.zeros((1, 1, 8, 12, 18), device=dev), (2, 4, 6))   # pw % 4 != 0
    with pytest.raises(L.GavikoHipError):
        ops.evp_highpass_linear(x, torch.zeros((32, 32), device=dev), torch.zeros(24, dtype=torch.int32, device=dev), x)   # aliasing
