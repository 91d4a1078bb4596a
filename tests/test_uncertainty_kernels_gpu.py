"""-m gpu: the kernels of csrc/uncertainty.hip on their own -- gvk_tta_volumes against torch.flip (bit for bit), gvk_predictive_stats
against a float64 numpy restatement, gvk_calibration_bins / metrics.calibration against a float64 numpy restatement fed the same fp32
probabilities -- and the calls each of them rejects."""
import numpy as np
import pytest
import torch

from gaviko_amd import metrics, ops
from gaviko_amd.lib import GavikoHipError
from test_uncertainty_golden import stats64

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ tta_volumes
def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32).to(dev)


@pytest.mark.parametrize("shape", [(120, 160, 160), (6, 10, 14), (5, 3, 8)], ids=["model", "odd_w14", "small_w8"])
def test_tta_volumes_equals_torch_flip_for_all_codes(dev, shape):
    """All 8 flip codes with a mixed source table, on the model volume (16-byte path), a small odd one with W % 4 != 0 (element path) and
    a small one with W % 4 == 0; the comparison is on the raw 32-bit words, so signed zeros, denormals and NaN payloads count."""
    S = 3
    D, H, W = shape
    g = torch.Generator().manual_seed(D * 1000 + W)
    x = torch.randn((S, 1, D, H, W), generator=g)
    x[0, 0, 0, 0, :4] = torch.tensor([-0.0, float("nan"), 1e-42, float("inf")])
    src = [0, 1, 2, 2, 1, 0, 1, 2, 0, 0]
    flip = [0, 1, 2, 3, 4, 5, 6, 7, 7, 0]
    xd = x.to(dev)
    out = torch.full((len(src), 1, D, H, W), 7.0, device=dev)
    ops.tta_volumes(xd, _i32(src, dev), _i32(flip, dev), out)
    again = torch.empty_like(out)
    ops.tta_volumes(xd, _i32(src, dev), _i32(flip, dev), again)
    got = out.cpu().view(torch.int32)
    assert torch.equal(got, again.cpu().view(torch.int32))
    for o, (s, f) in enumerate(zip(src, flip)):
        dims = [a + 2 for a in range(3) if f >> a & 1]
        want = torch.flip(x[s:s + 1], dims) if dims else x[s:s + 1]
        assert torch.equal(got[o:o + 1], want.contiguous().view(torch.int32)), (o, s, f)


def test_tta_volumes_rejects_bad_calls(dev):
    x = torch.zeros((2, 1, 4, 4, 8), device=dev)
    out = torch.zeros((3, 1, 4, 4, 8), device=dev)
    src, flip = _i32([0, 1, 0], dev), _i32([0, 1, 2], dev)
    ops.tta_volumes(x, src, flip, out)
    E = GavikoHipError
    with pytest.raises(E, match="overlap"):
        buf = torch.zeros((5, 1, 4, 4, 8), device=dev)
        ops.tta_volumes(buf[:2], src, flip, buf[1:4])
    with pytest.raises(E):
        ops.tta_volumes(x, src[:2], flip, out)                                    # src table of the wrong size
    with pytest.raises(E):
        ops.tta_volumes(x, src, _i32([0, 1, 2, 3], dev), out)                     # flip table of the wrong size
    with pytest.raises(E):
        ops.tta_volumes(x, src.long(), flip, out)                                 # not int32
    with pytest.raises(E):
        ops.tta_volumes(x, src.cpu(), flip, out)                                  # a host table
    with pytest.raises(E):
        ops.tta_volumes(x, src, flip, torch.zeros((3, 1, 4, 4, 4), device=dev))   # another geometry
    with pytest.raises(E):
        ops.tta_volumes(x.cpu(), src, flip, out)
    # more than 2^31 voxels per launch: the wrapper's guard compares shapes, and the library's own (checked before anything else is looked
    # at, nothing is launched) is asked directly with the sizes of a volume that is never allocated
    from gaviko_amd import lib as L
    rc = L.load().gvk_tta_volumes(x.data_ptr(), src.data_ptr(), flip.data_ptr(), out.data_ptr(), 2, 1, 1024, 1024, 1024, L.stream_ptr())
    assert rc != 0 and b"32-bit index range" in L.load().gvk_last_error()


# ------------------------------------------------------------------ predictive_stats
FLOATS = ("probs", "entropy", "expected_entropy", "mutual_info", "std", "variation_ratio")
TOL = 2e-6


def _check_stats(got, z, what):
    want = stats64(z.numpy())
    worst = {}
    for k in FLOATS:
        g = got[k].cpu().double().numpy()
        assert np.isfinite(g).all(), (what, k)
        worst[k] = float(np.abs(g - want[k]).max())
    print(f"{what}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"  (bound {TOL:.0e})")
    assert np.array_equal(got["votes"].cpu().numpy(), want["votes"]), what
    assert np.array_equal(got["pred"].cpu().numpy(), want["pred"]), what
    for k, v in worst.items():
        assert v <= TOL, (what, k, v)
    return want


@pytest.mark.parametrize("K", [2, 5, 64])
@pytest.mark.parametrize("S", [1, 7, 32])
def test_predictive_stats_match_float64(dev, K, S):
    """Float outputs within 2e-6 absolute of the float64 restatement (the bound the fused loss is held to against its fixtures: every
    quantity is at most ln 64 = 4.16, computed in fp32 from at most 32 * 64 terms); votes and pred exact.  Rows: random logits at three
    scales, rows with logits at +-80 (no NaN / Inf), a uniform row, and one sample whose members all agree."""
    B = 9
    g = torch.Generator().manual_seed(100 * K + S)
    z = torch.randn((B, S, K), generator=g)
    z[1] *= 5.0
    z[2] *= 0.05
    z[3] = torch.where(torch.rand((S, K), generator=g) < 0.5, torch.tensor(80.0), torch.tensor(-80.0))
    z[3, :, 0] = 80.0
    z[4] = 0.0                                                                    # uniform: the largest entropy, every class tied
    z[5] = z[5, :1]                                                               # identical members
    z[6, :, 1] = 80.0                                                             # one class certain: p = (0, 1, 0, ...) up to exp(-80)
    z[6, :, 0] = -80.0
    got = ops.predictive_stats(z.to(dev), B, S)
    want = _check_stats(got, z, f"K={K} S={S}")
    assert got["probs"].dtype == torch.float32 and got["pred"].dtype == torch.int32 and got["votes"].dtype == torch.int32
    assert tuple(got["probs"].shape) == (B, K) and tuple(got["std"].shape) == (B, K) and tuple(got["entropy"].shape) == (B,)
    assert (got["votes"].sum(1) == S).all()
    assert int(got["pred"][4]) == 0 and got["votes"][4].tolist() == [S] + [0] * (K - 1)       # ties: the lowest index
    assert float(got["mutual_info"].min()) >= 0.0
    assert abs(float(got["entropy"][4]) - np.log(K)) <= TOL and want["entropy"][6] < 1e-25
    if S == 1:
        assert float(got["mutual_info"].abs().max()) == 0.0 and float(got["std"].abs().max()) == 0.0
        assert torch.equal(got["entropy"], got["expected_entropy"])
        assert float(got["variation_ratio"].abs().max()) == 0.0
    again = ops.predictive_stats(z.to(dev), B, S)
    for k in got:
        assert torch.equal(got[k], again[k]), k


def test_predictive_stats_exact_tie_resolves_to_the_lowest_index(dev):
    """Hand-built.  Sample 0: two members whose logit rows are permutations of each other (classes 1 and 3 swapped), so the mean has
    classes 1 and 3 exactly equal and largest: pred = 1.  Sample 1: each member's own maximum is tied (five ways, three ways): both votes
    go to class 0, and so does pred."""
    z = torch.tensor([[[0.0, 2.0, 0.0, 1.0, -30.0], [0.0, 1.0, 0.0, 2.0, -30.0]],
                      [[1.0, 1.0, 1.0, 1.0, 1.0], [3.0, 3.0, 0.0, 0.0, 3.0]]])
    got = ops.predictive_stats(z.to(dev), 2, 2)
    p = got["probs"].cpu()
    assert float(p[0, 1]) == float(p[0, 3])                                       # exp, the sum and the division see the same values in both rows
    assert int(got["pred"][0]) == 1
    assert got["votes"][0].tolist() == [0, 1, 0, 1, 0] and abs(float(got["variation_ratio"][0]) - 0.5) == 0.0
    assert got["votes"][1].tolist() == [2, 0, 0, 0, 0] and int(got["pred"][1]) == 0
    want = stats64(z.numpy())
    assert np.array_equal(got["votes"].cpu().numpy(), want["votes"])


def test_predictive_stats_rejects_bad_calls(dev):
    E = GavikoHipError
    z = torch.zeros((2, 3, 5), device=dev)
    with pytest.raises(E):
        ops.predictive_stats(torch.zeros((2, 3, 1), device=dev), 2, 3)            # K < 2
    with pytest.raises(E):
        ops.predictive_stats(z, 2, 0)                                             # S < 1
    with pytest.raises(E, match="256"):
        ops.predictive_stats(torch.zeros((1, 1, 257), device=dev), 1, 1)          # K above the register budget: the limit is in the message
    ops.predictive_stats(torch.zeros((1, 1, 256), device=dev), 1, 1)
    with pytest.raises(E):
        ops.predictive_stats(z, 4, 3)                                             # not [B, S, K]
    with pytest.raises(E):
        ops.predictive_stats(z.cpu(), 2, 3)
    with pytest.raises(E):
        ops.predictive_stats(z.double(), 2, 3)
    # the library's own check (the wrapper is not the only guard)
    from gaviko_amd import lib as L
    t = torch.zeros(64, device=dev)
    rc = L.load().gvk_predictive_stats(z.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                       t.data_ptr(), 2, 3, 1, L.stream_ptr())
    assert rc != 0 and b"256" in L.load().gvk_last_error()


# ------------------------------------------------------------------ calibration
def calibration64(p32, y, nbins):
    """float64 numpy restatement, fed the same fp32 probabilities: the bins are compared against their edges i / nbins."""
    p = np.asarray(p32, dtype=np.float64)
    N, K = p.shape
    conf, pred = p.max(1), p.argmax(1)                                            # np.argmax: the first maximum
    count, correct, csum = np.zeros(nbins, np.int64), np.zeros(nbins, np.int64), np.zeros(nbins)
    for i in range(nbins):
        lo, hi = i / nbins, (i + 1) / nbins
        m = (conf > lo) & (conf <= hi)
        count[i], correct[i], csum[i] = m.sum(), (m & (pred == y)).sum(), conf[m].sum()
    assert count.sum() == N
    some = count > 0
    gap = np.abs(correct[some] / count[some] - csum[some] / count[some])
    onehot = np.eye(K)[y]
    tiny = float(np.finfo(np.float32).tiny)
    return {"count": count, "correct": correct, "ece": float((count[some] / N * gap).sum()), "mce": float(gap.max()),
            "brier": float(((p - onehot) ** 2).sum() / N), "nll": float(-np.log(np.maximum(p[np.arange(N), y], tiny)).sum() / N)}


def _proba_case(N, K, seed, dev):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, K - 1, (N,), generator=g)                                # class K - 1 never occurs as a label
    logits = 2.0 * torch.randn(N, K, generator=g) + 2.5 * torch.nn.functional.one_hot(y, K) * (torch.rand(N, 1, generator=g) > 0.3)
    proba = torch.softmax(logits, 1)
    proba[0] = torch.tensor([0.5, 0.5] + [0.0] * (K - 2))                         # confidence exactly on a bin edge (nbins even), a tie, p_y may be 0
    proba[1] = torch.tensor([0.0] * (K - 1) + [1.0])                              # confidence 1: the last bin; p_y = 0 for every label that occurs
    proba[2] = torch.tensor([0.25, 0.75] + [0.0] * (K - 2))                       # 0.75: an edge for nbins = 4, 20
    y[0], y[2] = 1, 0
    return proba.contiguous(), y


@pytest.mark.parametrize("N,K,nbins", [(257, 5, 15), (1500, 5, 10), (40, 3, 4), (700, 5, 20), (3, 5, 1)])
def test_calibration_matches_float64(dev, N, K, nbins):
    """Counts exact; ece, mce, brier and nll within 1e-12 (what the Evaluator's other metrics are held to).  Cases inside: a confidence
    exactly on a bin edge (0.5 with an even number of bins, 0.75 with 4 and 20), a class that never occurs, p_y = 0 (NLL = -log FLT_MIN)."""
    proba, y = _proba_case(N, K, N + nbins, dev)
    want = calibration64(proba.numpy(), y.numpy(), nbins)
    raw = ops.calibration_bins(proba.to(dev), y.to(dev), nbins)
    assert raw["count"].dtype == torch.int64 and raw["conf_sum"].dtype == torch.float64
    assert np.array_equal(raw["count"].cpu().numpy(), want["count"]) and np.array_equal(raw["correct"].cpu().numpy(), want["correct"])
    if nbins % 2 == 0:
        assert float(proba[0].max()) == 0.5 and want["count"][nbins // 2 - 1] >= 1          # (.., 0.5] holds the edge
    got = metrics.calibration(proba.to(dev), y.to(dev), bins=nbins)
    assert np.array_equal(got["bin_count"], want["count"])
    for k in ("ece", "mce", "brier", "nll"):
        print(f"N={N} K={K} nbins={nbins} {k}: got {got[k]:.15e} want {want[k]:.15e} diff {abs(got[k] - want[k]):.2e}")
    for k in ("ece", "mce", "brier", "nll"):
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    some = want["count"] > 0
    assert np.isnan(got["bin_accuracy"][~some]).all() and np.isnan(got["bin_confidence"][~some]).all()
    assert np.abs(got["bin_accuracy"][some] - want["correct"][some] / want["count"][some]).max() <= 1e-12
    assert got["nll"] > 87.0 / N                                                  # the p_y = 0 row contributes -log FLT_MIN = 87.3
    again = ops.calibration_bins(proba.to(dev), y.to(dev), nbins)
    for k in raw:
        assert torch.equal(raw[k], again[k]), k


def test_evaluator_reports_calibration_next_to_its_metrics(dev):
    N, K = 300, 5
    g = torch.Generator().manual_seed(7)
    y = torch.randint(0, K, (N,), generator=g)
    logits = torch.randn(N, K, generator=g) + 2.0 * torch.nn.functional.one_hot(y, K)
    ev = metrics.Evaluator(K, dev)
    for a in range(0, N, 64):
        ev.update(logits[a:a + 64].to(dev), y[a:a + 64].to(dev))
    r = ev.compute()
    assert {"accuracy", "quadratic_kappa", "auc", "confusion", "y_pred", "y_pred_proba", "y_test", "calibration"} <= set(r)
    want = calibration64(r["y_pred_proba"], y.numpy(), 15)
    cal = r["calibration"]
    assert np.array_equal(cal["bin_count"], want["count"]) and cal["bin_count"].sum() == N
    for k in ("ece", "mce", "brier", "nll"):
        assert abs(cal[k] - want[k]) <= 1e-12, (k, cal[k], want[k])


def test_calibration_rejects_bad_calls(dev):
    E = GavikoHipError
    p = torch.full((4, 5), 0.2, device=dev)
    y = torch.tensor([0, 1, 2, 3], device=dev)
    for nbins in (0, 255, 2.5, True):
        with pytest.raises(E):
            ops.calibration_bins(p, y, nbins)
    with pytest.raises(E):
        ops.calibration_bins(p, y[:3], 10)
    with pytest.raises(E):
        ops.calibration_bins(p, y.int(), 10)
    with pytest.raises(E):
        ops.calibration_bins(p.cpu(), y, 10)
    with pytest.raises(E):
        metrics.calibration(p, torch.tensor([0, 1, 2, 5], device=dev))            # a label outside [0, K)
    with pytest.raises(E):
        metrics.calibration(p.cpu(), y)
