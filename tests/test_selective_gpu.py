"""-m gpu: gvk_risk_coverage and gvk_temperature_fit through gaviko_amd.ops / metrics, against the host restatement of tests/selective_ref.py.

Risk-coverage: every integer (accepted, errors, at, total) must EQUAL the restatement; aurc may differ from its fsum value by (N + 8) 2^-53
relative -- the worst case of adding N non-negative float64 terms in any order (N - 1 roundings) plus the two roundings of a term (the
division, and the division by N), with room for the restatement's own two.  Shapes: the smallest at which the kernel takes another path (one
row, two, either side of a wave, a row past the 256-thread block, either side of the 1024-entry scan tile, the documented limit 8192).

Temperature: |beta - beta_ref| <= 2^-30 beta_ref where the optimum is inside the bracket -- the stop rule leaves at most 2^-40 beta, Newton's
remaining error is far below its last step, and the float64 accumulation noise of f' divided by f'' stays under that as long as f'' at the
optimum is at least 1e-2, which the test asserts on the host first; at a bound beta must be the bound exactly.  The NLLs match their fsum
values to 1e-12 (1 + max |beta z|)."""
import numpy as np
import pytest
import torch

import bootstrap_ref as br
import selective_ref as sr
from gaviko_amd import metrics, ops
from gaviko_amd.lib import GavikoHipError

pytestmark = pytest.mark.gpu

COVERAGES = (0.5, 0.8, 0.9, 0.95, 1.0)
U = 2.0 ** -53


def _dev(dev, score, y, pred):
    return torch.from_numpy(np.ascontiguousarray(score)).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(pred.astype(np.int32)).to(dev)


def _close(got, want, N):
    return abs(got - want) <= (N + 8) * U * want


def _check_replicates(dev, score, y, pred, R, seed, stratified, coverages=COVERAGES):
    """the device's integers of R resamples against the restatement; returns the device dict and the restatement's list"""
    N = score.size
    need = metrics.coverage_need(coverages, N)
    s, yd, pd = _dev(dev, score, y, pred)
    tables = ops.selective_tables(s, yd)
    out = ops.risk_coverage_counts(yd, pd, tables, need, R, seed, stratified)
    assert set(out) == {"aurc", "at", "total"}
    aurc, at, total = out["aurc"].cpu().numpy(), out["at"].cpu().numpy(), out["total"].cpu().numpy()
    assert aurc.dtype == np.float64 and aurc.shape == (R,) and at.shape == (R, len(need), 2) and total.shape == (R, 2)
    refs, w = sr.replicates(score, y, pred, need, seed, R, int(y.max()) + 1, stratified)
    for b, r in enumerate(refs):
        assert np.array_equal(at[b], r["at"]), (b, at[b], r["at"])
        assert tuple(total[b]) == r["total"] and total[b, 0] == N, (b, total[b], r["total"])
        print(f"N={N} R={R} b={b}: aurc {aurc[b]!r} ref {r['aurc']!r} rel {abs(aurc[b] - r['aurc']) / max(r['aurc'], 1e-300):.3e}")
        assert _close(aurc[b], r["aurc"], N), (b, aurc[b], r["aurc"])
    return out, refs, w


def _check_curve(dev, score, y, pred, coverages=COVERAGES):
    """the resample = 0 launch: the curve per sorted position, at and total against the restatement with unit multiplicities"""
    N = score.size
    need = metrics.coverage_need(coverages, N)
    s, yd, pd = _dev(dev, score, y, pred)
    tables = ops.selective_tables(s, yd)
    out = ops.risk_coverage_counts(yd, pd, tables, need, resample=False)
    r = sr.risk_coverage(score, y, pred, np.ones(N, dtype=np.int64), need)
    group = np.searchsorted(-r["thresholds"], -score[np.argsort(-score, kind="stable")])      # the distinct score of every sorted position
    assert np.array_equal(out["accepted"].cpu().numpy(), r["accepted"][group]) and np.array_equal(out["errors"].cpu().numpy(), r["errors"][group])
    assert np.array_equal(out["at"].cpu().numpy()[0], r["at"]) and tuple(out["total"].cpu().numpy()[0]) == r["total"]
    assert _close(float(out["aurc"].item()), r["aurc"], N)
    return out, r


@pytest.mark.parametrize("N,K,R", [(1, 2, 1), (2, 2, 3), (63, 5, 64), (65, 2, 3), (257, 5, 64), (1023, 2, 3), (1024, 5, 1), (1025, 5, 64),
                                   (8192, 2, 1), (8192, 5, 3)])
@pytest.mark.parametrize("stratified", [False, True], ids=["plain", "stratified"])
def test_integers_equal_the_restatement_and_aurc_is_within_its_bound(dev, N, K, R, stratified):
    score, y, pred, _ = sr.case_scores(N, K, N + K, quarters=True)
    assert N < 4 or np.unique(score).size < N                             # the scores do tie
    _check_replicates(dev, score, y, pred, R, 9, stratified)
    if not stratified:
        _check_curve(dev, score, y, pred)


def test_all_correct_all_wrong_all_tied_and_no_coverages(dev):
    N, R = 257, 8
    score, y, _, _ = sr.case_scores(N, 5, 11)
    out, refs, _ = _check_replicates(dev, score, y, y.copy(), R, 3, False)                     # every prediction correct
    assert (out["aurc"].cpu().numpy() == 0.0).all() and (out["total"].cpu().numpy()[:, 1] == 0).all()
    out, refs, _ = _check_replicates(dev, score, y, (y + 1) % 5, R, 3, False)                  # every prediction wrong
    assert all(r["aurc"] == 1.0 for r in refs) and (np.abs(out["aurc"].cpu().numpy() - 1.0) <= (N + 8) * U).all()
    assert (out["total"].cpu().numpy()[:, 1] == N).all()
    flat = np.full(N, 0.25, dtype=np.float32)                                                   # one threshold, coverage 1
    pred = br.case(N, 5, 11)[2]
    out, refs, _ = _check_replicates(dev, flat, y, pred, R, 3, True)
    assert (out["at"].cpu().numpy()[:, :, 0] == N).all()
    s, yd, pd = _dev(dev, flat, y, pred)
    rc = metrics.risk_coverage(s, yd, pd)
    assert rc.thresholds.tolist() == [0.25] and rc.coverage.tolist() == [1.0] and rc.accepted.tolist() == [N]
    assert rc.risk[0] == (pred != y).mean() == rc.aurc and all(v == (0.25, 1.0, rc.risk[0]) for v in rc.at.values())
    score, y, pred, _ = sr.case_scores(N, 5, 12)
    out, _, _ = _check_replicates(dev, score, y, pred, R, 3, False, coverages=())               # Q = 0
    assert out["at"].shape == (R, 0, 2)
    _check_curve(dev, score, y, pred, coverages=())
    s, yd, pd = _dev(dev, score, y, pred)
    rc = metrics.risk_coverage(s, yd, pd, coverages=())
    assert rc.at == {} and rc.replicates is None and rc.ci is None and rc.stderr is None


@pytest.mark.parametrize("stratified", [False, True], ids=["plain", "stratified"])
def test_replicates_pair_with_bootstrap(dev, stratified):
    """the same (seed, rule) draws the same resample here and in metrics.bootstrap: the errors of replicate b are N - trace(confusion[b])"""
    N, K, R, seed = 300, 5, 64, 3
    score, y, pred, proba = sr.case_scores(N, K, 300)
    s, yd, pd = _dev(dev, score, y, pred)
    out, _, w = _check_replicates(dev, score, y, pred, R, seed, stratified)
    bs = metrics.bootstrap(torch.from_numpy(proba).to(dev), yd, replicates=R, seed=seed, stratified=stratified, pred=pd)
    errors = out["total"].cpu().numpy()[:, 1]
    assert np.array_equal(errors, N - np.trace(bs.confusion, axis1=1, axis2=2))
    assert np.array_equal(errors, (w * (pred != y)[None, :]).sum(1)) and np.unique(errors).size > 1
    rc = metrics.risk_coverage(s, yd, pd, replicates=R, seed=seed, stratified=stratified, level=0.9)
    assert np.array_equal(rc.replicates["risk@1.0"], errors / N) and np.allclose(rc.replicates["risk@1.0"], 1.0 - bs.replicates["accuracy"], rtol=0, atol=1e-15)
    assert np.array_equal(rc.replicates["aurc"], out["aurc"].cpu().numpy())
    assert set(rc.replicates) == {"aurc"} | {f"risk@{q}" for q in COVERAGES} == set(rc.ci) == set(rc.stderr)
    for k, v in rc.replicates.items():
        assert v.dtype == np.float64 and v.shape == (R,)
        lo, hi = np.nanquantile(v, [0.05, 0.95])
        assert rc.ci[k] == (lo, hi) and rc.stderr[k] == np.nanstd(v, ddof=1), k
    assert (rc.seed, rc.stratified, rc.level) == (seed, stratified, 0.9)


def test_full_sample_curve_equals_numpy(dev):
    N, K = 1025, 5
    score, y, pred, _ = sr.case_scores(N, K, 77)
    s, yd, pd = _dev(dev, score, y, pred)
    rc = metrics.risk_coverage(s, yd, pd)
    wrong = pred != y
    thr = np.unique(score)[::-1]                                          # replicate-free numpy: counts at or above every distinct score
    accepted = np.array([(score >= v).sum() for v in thr])
    errors = np.array([(wrong & (score >= v)).sum() for v in thr])
    assert np.array_equal(rc.thresholds, thr) and rc.thresholds.dtype == np.float32
    assert np.array_equal(rc.accepted, accepted) and np.array_equal(rc.errors, errors) and rc.accepted.dtype == np.int64
    assert np.array_equal(rc.coverage, accepted / N) and np.array_equal(rc.risk, errors / accepted)
    assert rc.at[1.0] == (float(score.min()), 1.0, wrong.mean())
    for q, (t, c, r) in rc.at.items():
        i = np.flatnonzero(accepted >= metrics.coverage_need([q], N)[0])[0]
        assert (t, c, r) == (float(thr[i]), accepted[i] / N, errors[i] / accepted[i]), q
    ref = sr.risk_coverage(score, y, pred, np.ones(N, dtype=np.int64))
    assert _close(rc.aurc, ref["aurc"], N) and rc.optimal_aurc == metrics.optimal_aurc(N, int(wrong.sum())) and rc.eaurc == rc.aurc - rc.optimal_aurc
    assert 0.0 < rc.optimal_aurc < rc.aurc < wrong.mean()                 # a useful score: better than random abstention, worse than an oracle
    assert rc.replicates is None


def test_two_calls_give_the_same_bits(dev):
    score, y, pred, _ = sr.case_scores(1025, 5, 5)
    s, yd, pd = _dev(dev, score, y, pred)
    a = metrics.risk_coverage(s, yd, pd, replicates=64, seed=7)
    b = metrics.risk_coverage(s, yd, pd, replicates=64, seed=7)
    c = metrics.risk_coverage(s, yd, pd, replicates=64, seed=8)
    assert a.aurc == b.aurc == c.aurc
    for k in a.replicates:
        assert np.array_equal(a.replicates[k], b.replicates[k]), k
    assert not np.array_equal(a.replicates["aurc"], c.replicates["aurc"])
    with pytest.raises(GavikoHipError):                                   # the wrapper's own checks: a table of another length
        ops.risk_coverage_counts(yd, pd[:-1].contiguous(), ops.selective_tables(s, yd))


# ---- temperature --------------------------------------------------------------------------------------------------------------------

def _fit(dev, logits, y, **kw):
    return ops.temperature_fit(torch.from_numpy(logits).to(dev), torch.from_numpy(y).to(dev), **kw).cpu().numpy()


@pytest.mark.parametrize("N,K", [(1, 2), (65, 5), (1025, 3), (8192, 64)])
@pytest.mark.parametrize("factor", [3.0, 0.4], ids=["overconfident", "underconfident"])
def test_temperature_matches_the_root_of_the_gradient(dev, N, K, factor):
    logits, y = sr.case_logits(N, K, N + K, factor)
    beta_ref, bound_ref = sr.temperature(logits, y)
    if not bound_ref:
        assert sr.fsecond(logits, y, beta_ref) >= 1e-2                    # the condition of the 2^-30 bound
    st = _fit(dev, logits, y)
    T, beta, nll0, nll1, g, h, it, flags = st
    print(f"N={N} K={K} factor={factor}: beta {beta!r} ref {beta_ref!r} rel {abs(beta - beta_ref) / beta_ref:.3e} it {it} flags {flags} f' {g:.3e} f'' {h:.3e}")
    assert int(flags) & 1 and bool(int(flags) & 2) == bound_ref
    if bound_ref:
        assert beta == beta_ref and T in (0.05, 20.0) and it == 0         # one row can only ask for a bound
    else:
        assert abs(beta - beta_ref) <= 2.0 ** -30 * beta_ref and T == 1.0 / beta and 1 <= it <= 64
        assert abs(h - sr.fsecond(logits, y, beta)) <= 1e-9 * h and abs(g) <= 1e-9
    zmax = float(np.abs(logits.astype(np.float64)).max())
    assert abs(nll0 - sr.nll(logits, y, 1.0)) <= 1e-12 * (1.0 + zmax)
    assert abs(nll1 - sr.nll(logits, y, beta)) <= 1e-12 * (1.0 + beta * zmax)
    assert nll1 <= nll0
    assert np.array_equal(st, _fit(dev, logits, y))                       # two runs: the same bits


def test_temperature_bounds(dev):
    N, K = 257, 5
    logits, y = sr.case_logits(N, K, 9, 1.0)
    sure = logits.argmax(1).astype(np.int64)                              # separable, every row correct: the NLL falls all the way
    st = _fit(dev, logits, sure)
    assert st[0] == 0.05 and st[1] == 1.0 / 0.05 and int(st[7]) == 3 and st[4] <= 0.0 and st[6] == 0 and st[3] < st[2]
    st = _fit(dev, logits, sure, t_min=0.5, t_max=4.0)
    assert st[0] == 0.5 and st[1] == 2.0 and int(st[7]) == 3
    g = np.random.default_rng(4)
    strong, noise = (50.0 * g.standard_normal((N, K))).astype(np.float32), g.integers(0, K, N).astype(np.int64)
    assert sr.temperature(strong, noise) == (1.0 / 20.0, True)
    st = _fit(dev, strong, noise)                                         # labels unrelated to confident logits: as flat as allowed
    assert st[0] == 20.0 and st[1] == 1.0 / 20.0 and int(st[7]) == 3 and st[4] >= 0.0 and st[3] < st[2]
    assert abs(st[2] - sr.nll(strong, noise, 1.0)) <= 1e-12 * (1.0 + float(np.abs(strong).max()))


def test_fit_temperature_lowers_ece_and_scales_with_the_logits(dev):
    N, K = 1025, 5
    logits, y = sr.case_logits(N, K, 21, 3.0)
    z, yd = torch.from_numpy(logits).to(dev), torch.from_numpy(y).to(dev)
    fit = metrics.fit_temperature(z, yd)
    assert isinstance(fit, metrics.TemperatureFit) and fit.converged and not fit.at_bound and 1 <= fit.iterations <= 64
    assert fit.T > 1.5 and fit.nll_after < fit.nll_before and fit.ece_after < fit.ece_before
    beta_ref, _ = sr.temperature(logits, y)
    assert abs(1.0 / fit.T - beta_ref) <= 2.0 ** -30 * beta_ref
    assert torch.equal(fit.apply(z), z / fit.T)
    proba, pred = torch.empty_like(z), torch.empty(N, dtype=torch.int32, device=dev)
    ops.eval_rows(fit.apply(z).contiguous(), yd, proba, pred, torch.zeros(K * K, dtype=torch.int64, device=dev))
    assert fit.ece_after == metrics.calibration(proba, yd)["ece"]
    twice = metrics.fit_temperature(2.0 * z, yd)                          # exact doubling of every logit: beta halves
    assert abs(twice.T - 2.0 * fit.T) <= 2.0 ** -30 * 2.0 * fit.T
    bad = z.clone()
    bad[5, 1] = float("inf")
    with pytest.raises(GavikoHipError):
        metrics.fit_temperature(bad, yd)
    with pytest.raises(GavikoHipError):
        metrics.fit_temperature(z, yd + 1)


# ---- Evaluator ------------------------------------------------------------------------------------------------------------------------

def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return a == b


def test_evaluator_keywords(dev):
    N, K = 257, 5
    logits, y = sr.case_logits(N, K, 33, 3.0)
    ev = metrics.Evaluator(K, dev)
    for a in range(0, N, 64):
        ev.update(torch.from_numpy(logits[a:a + 64]).to(dev), torch.from_numpy(y[a:a + 64]).to(dev))
    before = ev.compute()
    assert set(before) == {"accuracy", "quadratic_kappa", "auc", "confusion", "y_pred", "y_pred_proba", "y_test", "calibration"}
    sel = ev.compute(selective=True, bootstrap=8, seed=2, stratified=True)
    assert set(sel) == set(before) | {"bootstrap", "report", "selective"}
    rc, bs = sel["selective"], sel["bootstrap"]
    assert isinstance(rc, metrics.RiskCoverage) and (rc.seed, rc.stratified) == (bs.seed, bs.stratified) == (2, True)
    assert rc.replicates["aurc"].shape == (8,) and np.array_equal(rc.replicates["risk@1.0"], (N - np.trace(bs.confusion, axis1=1, axis2=2)) / N)
    assert rc.at[1.0][2] == (N - np.trace(before["confusion"])) / N and np.array_equal(rc.thresholds, np.unique(before["y_pred_proba"].max(1))[::-1])
    alone = ev.compute(selective=True)
    assert set(alone) == set(before) | {"selective"} and alone["selective"].replicates is None and alone["selective"].aurc == rc.aurc
    after = ev.compute(selective=False, temperature=None)                 # the defaults, spelled out: today's dictionary, key for key
    assert _same(before, after) and _same(before, ev.compute())
    hot = ev.compute(temperature=2.0, selective=True)
    for k in ("y_pred", "confusion", "accuracy", "quadratic_kappa", "y_test"):
        assert _same(hot[k], before[k]), k
    want = torch.softmax(torch.from_numpy(logits) / 2.0, 1).numpy()
    assert np.abs(hot["y_pred_proba"] - want).max() < 1e-6 and hot["calibration"]["ece"] != before["calibration"]["ece"]
    assert np.array_equal(hot["selective"].thresholds, np.unique(hot["y_pred_proba"].max(1))[::-1])
    with pytest.raises(GavikoHipError):
        ev.compute(temperature=0.0)
