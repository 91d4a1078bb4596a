"""-m gpu: the perturbation kernels (csrc/perturb.hip) one by one through their ops wrappers, against plain torch constructions: the
rank, mask and volume kernels exactly (integers and selected bits), the score kernels against float64."""
import pytest
import torch

from gaviko_amd import ops

pytestmark = pytest.mark.gpu


def torch_rank(rel):
    """The inverse permutation of the stable descending argsort, row by row (CPU)."""
    order = torch.argsort(rel.cpu(), dim=1, descending=True, stable=True)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(rel.shape[1]).expand_as(order))
    return rank.to(torch.int32)


def i32(v, dev):
    return torch.tensor(v, dtype=torch.int32).to(dev)


@pytest.mark.parametrize("N", [1, 7, 64, 1000, 1331])
def test_patch_rank_is_the_stable_argsort_inverse(dev, N):
    g = torch.Generator().manual_seed(N)
    rows = [torch.randn(N, generator=g),                                          # random
            torch.randint(0, 4, (N,), generator=g).float(),                       # many ties
            torch.full((N,), 0.25),                                               # all equal
            torch.cat([torch.zeros(N // 3), torch.rand(N - N // 3, generator=g)]),   # a block of exact zeros first (gpa[i].global_)
            torch.where(torch.arange(N) % 2 == 0, torch.tensor(0.0), torch.tensor(-0.0))]   # signed zeros compare equal
    rel = torch.stack(rows).to(dev)
    want = torch_rank(rel)
    got = ops.patch_rank(rel)
    again = ops.patch_rank(rel)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(rows), N)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, again)
    assert torch.equal(got.cpu()[2], torch.arange(N, dtype=torch.int32))         # all equal: the patch order itself


def test_patch_mask_rank_matches_torch(dev):
    S, N = 3, 1000
    g = torch.Generator().manual_seed(1)
    rank = torch_rank(torch.randint(0, 50, (S, N), generator=g).float()).to(dev)
    src = [0, 1, 2, 1, 1, 0, 2]
    lo = [0, 0, 5, 17, 0, 999, 400]
    hi = [0, N, 5, 400, 1, N, N]                                                  # empty, everything, lo == hi, ...
    mask = torch.full((len(src), N), 7, dtype=torch.uint8, device=dev)
    ops.patch_mask_rank(rank, i32(src, dev), i32(lo, dev), i32(hi, dev), mask)
    r = rank.cpu()[torch.tensor(src)]
    want = ((r >= torch.tensor(lo)[:, None]) & (r < torch.tensor(hi)[:, None])).to(torch.uint8)
    assert torch.equal(mask.cpu(), want)
    assert int(want[0].sum()) == 0 and int(want[1].sum()) == N and int(want[2].sum()) == 0 and int(want[4].sum()) == 1


def test_patch_mask_box_matches_torch_including_clipped_boxes(dev):
    grid = (10, 10, 10)
    boxes = [(0, 5, 0, 5, 0, 5), (5, 10, 5, 10, 9, 12), (0, 0, 0, 10, 0, 10), (0, 10, 0, 10, 0, 10), (3, 4, 7, 8, 2, 3), (-2, 2, 8, 15, 0, 1)]
    mask = torch.full((len(boxes), 1000), 9, dtype=torch.uint8, device=dev)
    ops.patch_mask_box(i32(boxes, dev), mask, grid)
    want = torch.zeros((len(boxes),) + grid, dtype=torch.uint8)
    for i, (d0, d1, h0, h1, w0, w1) in enumerate(boxes):
        want[i, max(d0, 0):max(d1, 0), max(h0, 0):max(h1, 0), max(w0, 0):max(w1, 0)] = 1
    assert torch.equal(mask.cpu().view_as(want), want)
    grid2 = (2, 3, 5)                                                             # a grid with three different extents
    mask2 = torch.empty((1, 30), dtype=torch.uint8, device=dev)
    ops.patch_mask_box(i32([(1, 2, 0, 2, 3, 5)], dev), mask2, grid2)
    want2 = torch.zeros((1,) + grid2, dtype=torch.uint8)
    want2[0, 1:2, 0:2, 3:5] = 1
    assert torch.equal(mask2.cpu().view_as(want2), want2)


def special_volume(S, D, H, W, seed):
    """Random voxels with -0.0, denormals, infinities and a NaN payload among them: 'equal' below means the same 32 bits."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((S, 1, D, H, W), generator=g)
    bits = x.view(torch.int32).reshape(-1)
    n = bits.numel()
    pos = torch.randperm(n, generator=g)[:64]
    special = torch.tensor([-0x80000000, 0x00000001, 0x007FFFFF, -0x7FFFFFFF, 0x7F800000, 0x7FC01234, 0x00000000, -0x00800000], dtype=torch.int32)
    bits[pos] = special.repeat(8)
    return x


@pytest.mark.parametrize("geom", [((120, 160, 160), (12, 16, 16)), ((8, 12, 18), (4, 3, 6)), ((6, 8, 10), (3, 4, 5))],
                         ids=["cfg2", "pw6", "pw5"])
@pytest.mark.parametrize("fill", ["scalar", "shared_volume", "per_source_volume"])
def test_perturb_volume_is_torch_where_bit_for_bit(dev, geom, fill):
    (D, H, W), (pd, ph, pw) = geom
    S = 2
    src = [1, 0, 1, 1, 0]                                                         # sources repeat
    nd, nh, nw = D // pd, H // ph, W // pw
    N = nd * nh * nw
    g = torch.Generator().manual_seed(3)
    x = special_volume(S, D, H, W, 5)
    mask = (torch.rand((len(src), N), generator=g) < 0.4).to(torch.uint8)
    mask[3] = 1
    mask[4] = 0
    fs = base = None
    if fill == "scalar":
        fs = torch.tensor([-0.0, 1e-41])                                          # a signed zero and a denormal as fill values
        fillv = fs[torch.tensor(src)].view(-1, 1, 1, 1, 1).expand(len(src), 1, D, H, W)
    else:
        base = special_volume(1 if fill == "shared_volume" else S, D, H, W, 11)
        fillv = base[torch.tensor(src) if base.shape[0] == S else torch.zeros(len(src), dtype=torch.long)]
    up = mask.view(len(src), 1, nd, nh, nw).bool().repeat_interleave(pd, 2).repeat_interleave(ph, 3).repeat_interleave(pw, 4)
    want = torch.where(up, fillv.view(torch.int32), x[torch.tensor(src)].view(torch.int32))
    out = torch.full((len(src), 1, D, H, W), float("nan"), device=dev)
    ops.perturb_volume(x.to(dev), mask.to(dev), i32(src, dev), out, (pd, ph, pw), fill_scalar=None if fs is None else fs.to(dev),
                       base=None if base is None else base.to(dev))
    assert torch.equal(out.cpu().view(torch.int32), want)


def test_perturb_volume_rejects_bad_arguments(dev):
    from gaviko_amd.lib import GavikoHipError
    x = torch.zeros((1, 1, 4, 4, 8), device=dev)
    out = torch.zeros((2, 1, 4, 4, 8), device=dev)
    mask = torch.zeros((2, 4), dtype=torch.uint8, device=dev)
    src = i32([0, 0], dev)
    fs = torch.zeros(1, device=dev)
    with pytest.raises(GavikoHipError):
        ops.perturb_volume(x, mask, src, out, (2, 2, 8))                          # no fill at all
    with pytest.raises(GavikoHipError):
        ops.perturb_volume(x, mask, src, out, (2, 2, 8), fill_scalar=fs, base=x)  # both
    with pytest.raises(GavikoHipError):
        ops.perturb_volume(x, mask, src, out, (3, 2, 8), fill_scalar=fs)          # not divisible
    with pytest.raises(GavikoHipError):
        ops.perturb_volume(x, mask[:, :3].contiguous(), src, out, (2, 2, 8), fill_scalar=fs)
    with pytest.raises(GavikoHipError):
        ops.perturb_volume(out, mask, src, out, (2, 2, 8), fill_scalar=torch.zeros(2, device=dev))   # out overlaps x
    with pytest.raises(GavikoHipError):
        ops.perturb_volume(x.cpu(), mask, src, out, (2, 2, 8), fill_scalar=fs)


@pytest.mark.parametrize("K", [2, 5, 1000])
def test_perturb_scores_against_float64_softmax(dev, K):
    """fp32 exp / sum of K <= 4096 terms: probabilities to 1e-6 absolute; slots honoured; rows outside the chunk untouched."""
    g = torch.Generator().manual_seed(K)
    S, Bout, nslots = 3, 6, 11
    logits = (torch.randn((Bout, K), generator=g) * 4).to(dev)
    src = [0, 2, 1, 1, 0, 2]
    target = [K - 1, 0, K // 2]
    slot = [4, 0, 10, -1, 7, 2]                                                   # one padded sample that writes nowhere
    prob = torch.full((nslots,), -5.0, device=dev)
    logit = torch.full((nslots,), -5.0, device=dev)
    rows = torch.full((nslots, K), -5.0, device=dev)
    ops.perturb_scores(logits, i32(src, dev), i32(target, dev), i32(slot, dev), prob, logit, rows)
    p64 = torch.softmax(logits.double().cpu(), 1)
    wp, wl, wr = torch.full((nslots,), -5.0, dtype=torch.float64), torch.full((nslots,), -5.0), torch.full((nslots, K), -5.0)
    for o, sl in enumerate(slot):
        if sl >= 0:
            wp[sl] = p64[o, target[src[o]]]
            wl[sl] = logits[o, target[src[o]]].cpu()
            wr[sl] = logits[o].cpu()
    err = (prob.double().cpu() - wp).abs().max().item()
    print(f"perturb_scores K={K}: max |prob - float64| = {err:.3e}")
    assert err < 1e-6
    assert torch.equal(logit.cpu(), wl) and torch.equal(rows.cpu(), wr)
    # the gather-only form: rows without prob / logit
    rows2 = torch.full((nslots, K), -5.0, device=dev)
    ops.perturb_scores(logits, None, None, i32(slot, dev), None, None, rows2)
    assert torch.equal(rows2, rows)


def test_curve_auc_is_the_trapezoid_rule(dev):
    g = torch.Generator().manual_seed(9)
    S, N = 4, 1000
    ks = [0, 50, 100, 333, 334, 900, 1000]
    prob = torch.rand((S, len(ks)), generator=g).to(dev)
    auc = ops.curve_auc(prob, i32(ks, dev), N)
    xk = torch.tensor(ks, dtype=torch.float64) / N
    want = torch.trapezoid(prob.double().cpu(), xk, dim=1)
    err = (auc.double().cpu() - want).abs().max().item()
    print(f"curve_auc: max |auc - float64 trapezoid| = {err:.3e}")
    assert err < 1e-6
    assert torch.equal(auc, ops.curve_auc(prob, i32(ks, dev), N))
