"""-m gpu: gvk_roc_replicates through gaviko_amd.ops / metrics, against the host restatement of tests/roc_ref.py.

Every integer (total, auc2, at_spec, at_sens, at_cut, youden, the curve) must EQUAL the restatement.  ap may differ from its fsum value by
(N + 8) 2^-53 relative -- at most N non-negative float64 terms of one rounding each, added in any order (N - 1 roundings), and the division
by Pn, with room for the restatement's own two; it is the bound aurc is held to in test_selective_gpu.py.  Shapes: the smallest at which the
kernel takes another path (one row, two, three, either side of the 256-thread stride, either side of the 1024-entry scan tile and its carry,
a third tile, the documented limit 8192 where the LDS grant passes 64 KB)."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import roc_ref as rr
from gaviko_amd import metrics, ops
from gaviko_amd.lib import GavikoHipError

pytestmark = pytest.mark.gpu

SPEC, SENS = (0.5, 0.9, 0.95, 1.0), (0.0001, 0.5, 0.9, 1.0)
SPEC_BP, SENS_BP = (5000, 9000, 9500, 10000), (1, 5000, 9000, 10000)
U = 2.0 ** -53
INTEGERS = ("at_spec", "at_sens", "at_cut")


@functools.lru_cache(maxsize=None)
def _case(N, scores, labels):
    score, positive, grades = rr.case(N, 3 * N + 1, scores, labels)
    for a in (score, positive, grades):
        a.setflags(write=False)
    return score, positive, grades, tuple(rr.thresholds_for(score))


def _dev(dev, score, positive, strata):
    return (torch.from_numpy(np.array(score, dtype=np.float32)).to(dev), torch.from_numpy(positive.astype(np.int32)).to(dev),
            torch.from_numpy(np.array(strata, dtype=np.int64)).to(dev))


def _ap_close(got, want, N):
    return (math.isnan(got) and math.isnan(want)) or abs(got - want) <= (N + 8) * U * want


def _check(dev, score, positive, strata, thr, R, seed, stratified, resample=True):
    """the device's outputs of R resamples (or of the full sample) against the restatement; returns the device dict, the restatement's list, w"""
    N = score.size
    s, p, g = _dev(dev, score, positive, strata)
    tables = ops.roc_tables(s, p, g)
    kw = dict(replicates=R, seed=seed, stratified=stratified) if resample else dict(resample=False, curve=True)
    out = ops.roc_counts(p, g, tables, SPEC_BP, SENS_BP, rr.cut_rows(score, thr), **kw)
    again = ops.roc_counts(p, g, tables, SPEC_BP, SENS_BP, rr.cut_rows(score, thr), **kw)
    assert set(out) == {"total", "auc2", "ap", "at_spec", "at_sens", "at_cut", "youden"} | ({"tp", "fp"} if not resample else set())
    h = {k: v.cpu().numpy() for k, v in out.items()}
    assert h["ap"].dtype == np.float64 and h["auc2"].dtype == np.int64 and h["total"].shape == (R, 2) and h["youden"].shape == (R, 3)
    assert h["at_spec"].shape == (R, 4, 2) and h["at_sens"].shape == (R, 4, 2) and h["at_cut"].shape == (R, len(thr), 2)
    assert np.array_equal(h["ap"], again["ap"].cpu().numpy(), equal_nan=True)                 # two launches: the same bits
    refs, w = rr.replicates(score, positive, strata, SPEC_BP, SENS_BP, thr, seed, R, stratified, resample)
    for b, r in enumerate(refs):
        assert tuple(h["total"][b]) == r["total"] and sum(r["total"]) == N, (b, h["total"][b], r["total"])
        assert int(h["auc2"][b]) == r["auc2"], (b, h["auc2"][b], r["auc2"])
        for k in INTEGERS:
            assert np.array_equal(h[k][b], r[k]), (k, b, h[k][b], r[k])
        assert tuple(h["youden"][b]) == r["youden"], (b, h["youden"][b], r["youden"])
        print(f"N={N} b={b}: ap {h['ap'][b]!r} ref {r['ap']!r}")
        assert _ap_close(float(h["ap"][b]), r["ap"], N), (b, h["ap"][b], r["ap"])
    if N <= 1025:
        assert refs[0]["auc2"] == rr.auc2_pairs(score, positive, w[0])                          # the restatement's own sum, by pair counting
    if not resample:
        r = refs[0]
        group = np.searchsorted(-r["thresholds"], -score[np.argsort(-score, kind="stable")])      # the distinct score of every sorted position
        assert np.array_equal(h["tp"], r["tp"][group]) and np.array_equal(h["fp"], r["fp"][group])
    return out, refs, w


@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2049, 8192])
@pytest.mark.parametrize("draw", ["plain", "stratified", "full"])
def test_integers_equal_the_restatement_and_ap_is_within_its_bound(dev, N, draw):
    R = 1 if draw == "full" else (3 if N == 8192 else 5)
    for scores in ("continuous", "quarters", "equal"):
        for labels in ("mixed", "all", "none", "one"):
            score, positive, grades, thr = _case(N, scores, labels)
            if scores == "quarters" and N > 3:
                assert np.unique(score).size < N                                                # the scores do tie
            _check(dev, score, positive, grades, thr, R, 9, draw == "stratified", resample=draw != "full")


def test_empty_level_lists_and_the_binary_default_strata(dev):
    N = 257
    score, positive, _, _ = _case(N, "quarters", "mixed")
    s, p, _ = _dev(dev, score, positive, positive)
    tables = ops.roc_tables(s, p)                                                               # strata default to the binary label
    positive_strata = (p != 0).to(torch.int64)
    out = ops.roc_counts(p, positive_strata, tables, replicates=4, seed=2, stratified=True)
    assert out["at_spec"].shape == (4, 0, 2) and out["at_sens"].shape == (4, 0, 2) and out["at_cut"].shape == (4, 0, 2)
    refs, _ = rr.replicates(score, positive, positive.astype(np.int64), (), (), (), 2, 4, True)
    assert [tuple(t) for t in out["total"].cpu().numpy()] == [r["total"] for r in refs] == [(int(positive.sum()), int((~positive).sum()))] * 4
    assert out["auc2"].cpu().tolist() == [r["auc2"] for r in refs] and [tuple(y) for y in out["youden"].cpu().numpy()] == [r["youden"] for r in refs]
    plain = ops.roc_counts(p, None, tables, replicates=4, seed=2)                               # the plain draw reads no strata
    refs, _ = rr.replicates(score, positive, positive.astype(np.int64), (), (), (), 2, 4, False)
    assert plain["auc2"].cpu().tolist() == [r["auc2"] for r in refs]
    with pytest.raises(GavikoHipError):                                                         # the wrapper's own checks: a table of another length
        ops.roc_counts(p[:-1].contiguous(), positive_strata[:-1].contiguous(), tables)


@pytest.mark.parametrize("stratified", [False, True], ids=["plain", "stratified"])
def test_replicates_pair_with_bootstrap_counts(dev, stratified):
    """the same (seed, rule, strata) draws the same resample here and in gvk_bootstrap_counts: on the binary labels its confusion rows sum to
    (Nn, Pn), and with scores on a grid of 1 / 64 (1 - s is exact) its one-vs-rest pair count of class 1 over proba = [1 - s, s] is auc2"""
    N, R, seed = 300, 16, 3
    g = np.random.default_rng(8)
    positive = g.random(N) < 0.4
    score = (np.clip(np.round((0.5 + 0.2 * g.standard_normal(N) + 0.15 * positive) * 64), 0, 64) / 64).astype(np.float32)
    s, p, y = _dev(dev, score, positive, positive)
    out, _, w = _check(dev, score, positive, positive.astype(np.int64), (0.5,), R, seed, stratified)
    proba = torch.stack([1.0 - s, s], 1).contiguous()
    conf, cnt = ops.bootstrap_counts(y, torch.argmax(proba, 1).to(torch.int32), ops.bootstrap_tables(proba, y), R, seed, stratified)
    conf, cnt, total = conf.cpu().numpy(), cnt.cpu().numpy(), out["total"].cpu().numpy()
    assert np.array_equal(total[:, 0], conf[:, 1, :].sum(1)) and np.array_equal(total[:, 1], conf[:, 0, :].sum(1))
    assert np.array_equal(total[:, 0], (w * positive[None, :]).sum(1)) and (stratified or np.unique(total[:, 0]).size > 1)
    assert np.array_equal(out["auc2"].cpu().numpy(), cnt[:, 1, 0]) and np.array_equal(total, cnt[:, 1, 1:])


def _ref_scalars(score, positive, strata, thr, seed, R, stratified, spec_bp=SPEC_BP, sens_bp=SENS_BP):
    refs, _ = rr.replicates(score, positive, strata, spec_bp, sens_bp, thr, seed, R, stratified)
    rows = [rr.scalars(r, spec_bp, sens_bp, thr, score) for r in refs]
    return {k: np.array([row[k] for row in rows], dtype=np.float64) for k in rows[0]}


def _same_scalars(got, want, N):
    assert set(got) == set(want)
    for k in want:
        if k == "average_precision":
            assert all(_ap_close(float(a), float(b), N) for a, b in zip(got[k], want[k])), k
        else:
            assert np.array_equal(got[k], want[k], equal_nan=True), (k, got[k], want[k])


def test_undefined_replicates_are_counted_and_skipped(dev):
    N, R = 12, 64
    score, _, _ = rr.case(N, 5)
    positive = np.arange(N) == 4
    strata = positive.astype(np.int64)
    thr = (float(score[4]),)
    for seed in range(20):                                                # chosen on the host: some replicates lose the one positive row, not all
        want = _ref_scalars(score, positive, strata, thr, seed, R, False)
        lost = int(np.isnan(want["auc"]).sum())
        if 0 < lost < R:
            break
    assert 0 < lost < R
    s, p, _ = _dev(dev, score, positive, strata)
    r = metrics.roc_analysis(s, p, specificities=SPEC, sensitivities=SENS, thresholds=thr, replicates=R, seed=seed, level=0.9)
    _same_scalars(r.replicates, want, N)
    assert r.undefined["auc"] == lost == int((r.counts["total"][:, 0] == 0).sum()) and r.undefined["average_precision"] == lost
    assert r.undefined[f"ppv@thr={thr[0]}"] == int(np.isnan(want[f"ppv@thr={thr[0]}"]).sum())
    for k, v in want.items():
        assert r.undefined[k] == int(np.isnan(v).sum()), k
        if k != "average_precision":
            lo, hi = np.nanquantile(v, [(1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0])      # the documented expression, (1 -+ level) / 2
            assert r.ci[k] == (lo, hi) and r.stderr[k] == np.nanstd(v, ddof=1), k
    assert not math.isnan(r.ci["auc"][0]) and not math.isnan(r.stderr["auc"])                 # the interval skips the NaN replicates
    assert not math.isnan(r.auc) and r.positives == 1 and math.isnan(r.auc_se)      # one positive row: no DeLong variance


def test_roc_analysis_end_to_end(dev):
    from sklearn.metrics import average_precision_score, roc_auc_score, roc_curve
    N, R, seed = 300, 40, 6
    score, positive, grades, thr = _case(N, "quarters", "mixed")
    s, p, g = _dev(dev, score, positive, grades)
    r = metrics.roc_analysis(s, p != 0, specificities=SPEC, sensitivities=SENS, thresholds=thr, replicates=R, seed=seed, stratified=True, strata=g)
    assert isinstance(r, metrics.RocAnalysis) and (r.seed, r.stratified, r.level) == (seed, True, 0.95)
    ref = rr.roc(score, positive, np.ones(N, dtype=np.int64), SPEC_BP, SENS_BP, thr)
    Pn, Nn = ref["total"]
    fpr, tpr, th = roc_curve(positive, score, drop_intermediate=False)
    assert np.array_equal(r.thresholds, th.astype(np.float32)) and r.thresholds.dtype == np.float32 and np.isinf(r.thresholds[0])
    assert np.array_equal(r.tp[1:], ref["tp"]) and np.array_equal(r.fp[1:], ref["fp"]) and r.tp[0] == r.fp[0] == 0 and r.tp.dtype == np.int64
    assert np.array_equal(r.tpr, tpr) and np.array_equal(r.fpr, fpr) and (r.positives, r.negatives) == (Pn, Nn)
    assert r.auc == ref["auc2"] / (2.0 * Pn * Nn) and abs(r.auc - roc_auc_score(positive, score)) <= 1e-12
    assert _ap_close(r.average_precision, ref["ap"], N) and abs(r.average_precision - average_precision_score(positive, score)) <= 1e-12
    point = rr.scalars(ref, SPEC_BP, SENS_BP, thr, score)
    assert r.sensitivity_at == {q: point[f"sens@spec={q}"] for q in SPEC} and r.specificity_at == {q: point[f"spec@sens={q}"] for q in SENS}
    for q, bp in zip(SPEC, SPEC_BP):                                      # the best sensitivity sklearn's curve has at that specificity
        assert r.sensitivity_at[q] == tpr[(Nn - r.fp) * 10000 >= bp * Nn].max()
    for q, bp in zip(SENS, SENS_BP):
        ok = r.tp * 10000 >= bp * Pn                                      # ... and the smallest false-positive rate at that sensitivity
        assert r.specificity_at[q] == (Nn - r.fp[ok].min()) / Nn and r.fp[ok].min() / Nn == fpr[ok].min()
    for t in thr:
        got, call = r.at_threshold[t], score.astype(np.float64) >= t
        assert _same(got, {"sensitivity": point[f"sens@thr={t}"], "specificity": point[f"spec@thr={t}"], "ppv": point[f"ppv@thr={t}"],
                           "npv": point[f"npv@thr={t}"]})
        assert got["sensitivity"] == (call & positive).sum() / Pn and got["specificity"] == (~call & ~positive).sum() / Nn
        assert math.isnan(got["ppv"]) == (call.sum() == 0) and math.isnan(got["npv"]) == (call.sum() == N)
        if 0 < call.sum() < N:
            assert got["ppv"] == (call & positive).sum() / call.sum() and got["npv"] == (~call & ~positive).sum() / (~call).sum()
    assert r.youden == (point["youden_threshold"], point["youden_sensitivity"], point["youden_specificity"], point["youden_j"])
    assert r.youden[3] == pytest.approx((tpr - fpr).max(), abs=1e-12) and r.youden[0] in th[np.abs((tpr - fpr) - r.youden[3]) <= 1e-12]
    psi = rr.placements(score, positive)
    assert np.array_equal(r.placements, psi)
    exact = rr.delong_covariance_exact(psi, psi, positive)
    assert abs(Fraction(r.auc_se ** 2) - exact) <= 20 * Fraction(math.ulp(float(exact)))       # 16 ulp of the variance, sqrt and square: 4 more
    want = _ref_scalars(score, positive, grades, thr, seed, R, True)
    _same_scalars(r.replicates, want, N)
    assert set(r.replicates) == set(r.ci) == set(r.stderr) == set(r.undefined) and all(v == 0 for k, v in r.undefined.items() if "pv@" not in k)
    for k, v in want.items():
        assert r.replicates[k].dtype == np.float64 and r.replicates[k].shape == (R,)
        if k != "average_precision" and not np.isnan(v).all():
            lo, hi = np.nanquantile(v, [(1.0 - 0.95) / 2.0, (1.0 + 0.95) / 2.0])
            assert r.ci[k] == (lo, hi) and r.stderr[k] == np.nanstd(v, ddof=1), k
    assert r.ci["auc"][0] < r.auc < r.ci["auc"][1] and 0.5 * r.auc_se < r.stderr["auc"] < 2.0 * r.auc_se      # the two standard errors agree roughly
    assert set(r.counts) == {"total", "auc2", "ap", "at_spec", "at_sens", "at_cut", "youden"} and (r.counts["total"] == (Pn, Nn)).all()
    alone = metrics.roc_analysis(s, p)
    assert alone.replicates is None and alone.ci is None and alone.counts is None and alone.auc == r.auc and set(alone.sensitivity_at) == {0.9, 0.95}
    with pytest.raises(GavikoHipError, match="labels for"):
        metrics.roc_analysis(s, p[:-1])
    with pytest.raises(GavikoHipError, match="strata"):
        metrics.roc_analysis(s, p, strata=g + 64)


def test_roc_compare_is_the_paired_difference_with_delongs_test(dev):
    from scipy.stats import norm
    N, R, seed = 300, 32, 11
    score, positive, grades, _ = _case(N, "quarters", "mixed")
    other = rr.case(N, 17, "continuous")[0]
    other = (0.5 * other + 0.5 * score * (np.arange(N) % 3 > 0)).astype(np.float32)             # a weaker, correlated second model
    sa, p, g = _dev(dev, score, positive, grades)
    sb = torch.from_numpy(other).to(dev)
    kw = dict(specificities=(0.9,), sensitivities=(0.9,), thresholds=(0.5,), replicates=R, seed=seed, stratified=True, strata=g)
    c = metrics.roc_compare(sa, sb, p, **kw)
    a, b = metrics.roc_analysis(sa, p, **kw), metrics.roc_analysis(sb, p, **kw)
    assert isinstance(c, metrics.RocComparison) and np.array_equal(c.a.counts["total"], c.b.counts["total"])      # the same multiplicities
    assert set(c.delta) == set(a.replicates) == set(c.ci) == set(c.p_value) == set(c.delta_point)
    for k in c.delta:
        assert np.array_equal(c.delta[k], a.replicates[k] - b.replicates[k], equal_nan=True), k
        assert c.p_value[k] == metrics.paired_p_value(c.delta[k]) and c.ci[k] == metrics._interval(c.delta[k], 0.95)
    assert c.delta_point["auc"] == a.auc - b.auc > 0.0 and c.delta_point["spec@sens=0.9"] == a.specificity_at[0.9] - b.specificity_at[0.9]
    pa, pb = rr.placements(score, positive), rr.placements(other, positive)
    vaa, vbb, vab = (rr.delong_covariance_exact(x, y, positive) for x, y in ((pa, pa), (pb, pb), (pa, pb)))
    var = vaa + vbb - 2 * vab
    # each float64 covariance is within 16 ulp of its exact value; with a correlation below 0.99 the difference keeps at least 1 % of
    # var_a + var_b, so the three errors (at most 4 * 16 ulp of the larger variance) stay below 1e-12 of it, and the square root halves that
    assert float(vab) < 0.99 * math.sqrt(float(vaa) * float(vbb))
    z = (a.auc - b.auc) / math.sqrt(float(var))
    assert abs(c.delong_z - z) <= 1e-12 * abs(z) and c.delong_p == pytest.approx(2.0 * norm.sf(abs(z)), rel=1e-9)
    same = metrics.roc_compare(sa, sa, p, replicates=4)
    assert math.isnan(same.delong_z) and math.isnan(same.delong_p) and all((v == 0).all() for k, v in same.delta.items() if "pv@" not in k)


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))


def test_evaluator_roc_keyword(dev):
    import selective_ref as sr
    N, K = 257, 5
    logits, y = sr.case_logits(N, K, 33, 3.0)
    ev = metrics.Evaluator(K, dev)
    for a in range(0, N, 64):
        ev.update(torch.from_numpy(logits[a:a + 64]).to(dev), torch.from_numpy(y[a:a + 64]).to(dev))
    before = ev.compute(bootstrap=50, seed=2, stratified=True)
    out = ev.compute(bootstrap=50, seed=2, stratified=True, roc=2)
    assert set(out) == set(before) | {"roc"} and all(_same(out[k], before[k]) for k in before)
    assert _same(ev.compute(roc=None), ev.compute()) and "roc" not in ev.compute()
    r, bs = out["roc"], out["bootstrap"]
    assert isinstance(r, metrics.RocAnalysis) and (r.seed, r.stratified) == (bs.seed, bs.stratified) == (2, True)
    assert r.replicates["auc"].shape == (50,) and (r.positives, r.negatives) == (int((y >= 2).sum()), int((y < 2).sum()))
    # the K grades are the strata, as in bootstrap: replicate b is the same resample, its positives the rows of the confusion matrix from grade 2 up
    assert np.array_equal(r.counts["total"][:, 0], bs.confusion[:, 2:, :].sum((1, 2))) and (r.counts["total"].sum(1) == N).all()
    proba = out["y_pred_proba"]
    score = torch.from_numpy(proba).to(dev)[:, 2:].sum(1).cpu().numpy()
    ref = rr.roc(score, y >= 2, np.ones(N, dtype=np.int64))
    assert r.auc == ref["auc2"] / (2.0 * r.positives * r.negatives) and np.array_equal(r.thresholds[1:], ref["thresholds"])
    alone = ev.compute(roc=1)
    assert alone["roc"].replicates is None and alone["roc"].positives == int((y >= 1).sum())
    with pytest.raises(GavikoHipError, match="cut"):
        ev.compute(roc=5)
