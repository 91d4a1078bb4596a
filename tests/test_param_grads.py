"""CPU: the reference of gvk_param_grads (tests/param_grads_ref.py) against naive loops, and the sizing of the call's scratch and ticket
words -- ops.param_grads_scratch_elems against the library's own size query (a host function: no device needed) and the ticket count
against ops.PGRAD_TICKETS -- for every call tests/test_param_grads_gpu.py makes (its case functions run dry here and only record their
shapes) and for the engine's two job mixes at the workload's shapes."""
import ctypes

import numpy as np
import pytest

import dropmask
import param_grads_ref as R


# ------------------------------------------------------------------ the reference against naive loops
def _naive_outer(narrow, wide, narrow2, wide2, ov, T, P, mean, rstd, mask):
    """Q[l][c], its term-magnitude sum, the column sums of wide' and S[l], one scalar at a time."""
    M, L = narrow.shape
    C = wide.shape[1]
    rows = []
    for m in range(M):
        n = [float(v) for v in narrow[m]]
        if ov is not None and m % T < P:
            n = [float(v) for v in ov.reshape(-1, L)[(m // T) * P + m % T]]
        w = []
        for c in range(C):
            x = float(wide[m][c])
            if mask is not None:
                x *= float(mask[m][c])
            if mean is not None:
                x = (x - float(mean[m])) * float(rstd[m])
            w.append(x)
        rows.append((n, w))
    if narrow2 is not None:
        for m in range(narrow2.shape[0]):
            rows.append(([float(v) for v in narrow2[m]], [float(v) for v in wide2[m]]))
    Q, aQ = np.zeros((L, C)), np.zeros((L, C))
    cs, S = np.zeros(C), np.zeros(L)
    for n, w in rows:
        for l in range(L):
            S[l] += n[l]
            for c in range(C):
                Q[l][c] += n[l] * w[c]
                aQ[l][c] += abs(n[l] * w[c])
        for c in range(C):
            cs[c] += w[c]
    return Q, aQ, cs, S


def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape).astype(np.float64)


@pytest.mark.parametrize("case", ["plain", "override", "second", "ln", "drop", "affine"])
def test_reference_against_naive_loops(case):
    rng = np.random.default_rng(3)
    L, C, B, T, P = 4, 12, 2, 5, 2
    M = B * T
    narrow, wide = _ints(rng, (M, L), -3, 3), _ints(rng, (M, C), -3, 3)
    kw, nv = {}, dict(narrow2=None, wide2=None, ov=None, T=0, P=0, mean=None, rstd=None, mask=None)
    if case == "override":
        ov = _ints(rng, (B, P, L), 5, 9)
        kw, nv = dict(lat_override=ov, T=T, P=P), dict(nv, ov=ov, T=T, P=P)
    if case == "second":
        n2, w2 = _ints(rng, (3, L), -3, 3), _ints(rng, (3, C), -3, 3)
        kw, nv = dict(narrow2=n2, wide2=w2), dict(nv, narrow2=n2, wide2=w2)
    if case in ("ln", "affine"):
        mean, rstd = _ints(rng, (M,), -2, 2), rng.choice([0.5, 1.0, 2.0], M)
        kw, nv = dict(mean=mean, rstd=rstd), dict(nv, mean=mean, rstd=rstd)
    if case == "drop":
        kw, nv = dict(drop_p=0.5, seed=9, seed_word=100), dict(nv, mask=dropmask.rows_mask(109, M, C, 0.5))
        assert 0 < (nv["mask"] == 0).sum() < M * C and set(np.unique(nv["mask"])) == {0.0, 2.0}
    Q, aQ, cs, S = _naive_outer(narrow, wide, **nv)
    if case != "affine":
        prev = _ints(rng, (L, C), -3, 3)
        got = R.outer(narrow, wide, want_colsum=True, **kw)
        assert np.array_equal(got["out"][0], Q) and np.array_equal(got["out"][1], aQ) and np.array_equal(got["colsum"][0], cs)
        got = R.outer(narrow, wide, transposed=True, prev=dict(out=prev.T), **kw)
        assert np.array_equal(got["out"][0], prev.T + Q.T) and np.array_equal(got["out"][1], np.abs(prev.T) + aQ.T) and "colsum" not in got
        got = R.outer(narrow, wide, want_out=False, want_colsum=True, **kw)
        assert set(got) == {"colsum"} and got["colsum"][1].shape == (C,)
        return
    W, g, b = _ints(rng, (L, C), -2, 2), _ints(rng, (C,), -2, 2), _ints(rng, (C,), -2, 2)
    prev = dict(out=_ints(rng, (L, C), -3, 3), dgamma=_ints(rng, (C,), -3, 3), dbeta=_ints(rng, (C,), -3, 3), dbias=_ints(rng, (L,), -3, 3))
    got = R.outer(narrow, wide, aff_w=W, aff_gamma=g, aff_beta=b, prev=prev, **kw)
    for l in range(L):
        assert got["dbias"][0][l] == prev["dbias"][l] + S[l]
        for c in range(C):
            assert got["out"][0][l][c] == prev["out"][l][c] + g[c] * Q[l][c] + b[c] * S[l]
    for c in range(C):
        assert got["dgamma"][0][c] == prev["dgamma"][c] + sum(W[l][c] * Q[l][c] for l in range(L))
        assert got["dbeta"][0][c] == prev["dbeta"][c] + sum(W[l][c] * S[l] for l in range(L))
        assert got["dgamma"][1][c] == abs(prev["dgamma"][c]) + sum(abs(W[l][c]) * aQ[l][c] for l in range(L))
    assert np.array_equal(got["Q"][0], Q) and np.array_equal(got["S"][0], S)
    assert "dbias" not in R.outer(narrow, wide, aff_w=W, aff_gamma=g, aff_beta=b, want_dbias=False, **kw)
    assert R.exact(*got.values()) and not R.exact((Q, aQ * 2.0 ** 22))


def test_reference_small_jobs_against_naive_loops():
    rng = np.random.default_rng(4)
    a, a2, b = _ints(rng, (7, 3), -3, 3), _ints(rng, (4, 3), -3, 3), _ints(rng, (7, 5), -3, 3)
    v, bud = R.small(a, a2=a2, prev=np.array([1.0, -2.0, 3.0]))
    for j in range(3):
        assert v[j] == [1.0, -2.0, 3.0][j] + sum(a[m][j] for m in range(7)) + sum(a2[m][j] for m in range(4))
        assert bud[j] == abs([1.0, -2.0, 3.0][j]) + sum(abs(a[m][j]) for m in range(7)) + sum(abs(a2[m][j]) for m in range(4))
    v, bud = R.small(a, b)
    for j in range(3):
        for l in range(5):
            assert v[j][l] == sum(a[m][j] * b[m][l] for m in range(7)) and bud[j][l] == sum(abs(a[m][j] * b[m][l]) for m in range(7))
    with pytest.raises(ValueError):
        R.small(a, b, a2=a2)
    with pytest.raises(ValueError):
        R.outer(a, b, narrow2=a, wide2=b, drop_p=0.5)


# ------------------------------------------------------------------ sizing
def _gpu_file_calls():
    import test_param_grads_gpu as G
    from gaviko_amd import lib
    count = lib.load().gvk_gpa_gate_param_count
    pg = G.PG(None)
    for L in G.WIDTHS:
        G.case_plain(pg, L)
        G.case_mixes(pg, L, count)
    for L in (8, 16, 28):
        G.case_two_streams(pg, L)
    for L in (4, 20, 24):
        G.case_override(pg, L)
    for L in (8, 16, 20, 28):
        G.case_ln_drop_affine(pg, L)
    G.case_small(pg)
    G.case_product_shape(pg, count)
    G.case_fullest(pg)
    return set(pg.calls)


def _engine_calls():
    from gaviko_amd import lib
    count = lib.load().gvk_gpa_gate_param_count
    T, N, P = 1033, 1000, 32
    calls = set()
    for B in (1, 2, 4, 8):
        for C in (192, 768, 1024):
            for L in (4, 8, 12, 16, 20, 24, 28):
                M, BN, BP = B * T, B * N, B * P
                calls.add((L, C, ((M, 0, C), (M, BN, C)),
                           ((B, count(L, P), 0), (BP, L, L), (BP, L, 0), (BP, L, L), (BP, L, 0), (M + BN, L, 0))))
                calls.add((L, C, ((BN, 0, C), (BN, 0, C), (BN, 0, 3 * L)), ()))
    return calls


@pytest.fixture(scope="module")
def calls():
    """(L, C, ((M, M2, C_k) per outer job), ((rows, J, L_b) per small job)) of every call to be sized."""
    got = _gpu_file_calls()
    assert len(got) > 300 and max(len(c[2]) for c in got) == 3 and max(len(c[3]) for c in got) == 8
    return sorted(got | _engine_calls())


def test_scratch_bound_covers_the_library_size_query(calls):
    """ops.param_grads_scratch_elems (what the engine allocates by) >= gvk_param_grads_scratch (what the call will ask for)."""
    from gaviko_amd import lib, ops
    query = lib.load().gvk_param_grads_scratch
    for L, C, outer, small in calls:
        arr = (lib.PgradOuter * max(1, len(outer)))()
        for k, (M, M2, Ck) in enumerate(outer):
            arr[k].M, arr[k].M2, arr[k].C = M, M2, Ck
            arr[k].narrow2 = ctypes.c_void_p(8 if M2 else None)                 # (only tested against NULL by the query)
        jobs = (lib.ReduceJob * max(1, len(small)))()
        for k, (rows, J, Lb) in enumerate(small):
            jobs[k].M, jobs[k].J, jobs[k].L = rows, J, Lb
            jobs[k].b = ctypes.c_void_p(8 if Lb else None)
        need = query(arr, len(outer), jobs, len(small), C, L)
        have = ops.param_grads_scratch_elems(L, [(Ck + 63) // 64 for _, _, Ck in outer], [J * Lb if Lb else J for _, J, Lb in small])
        assert 0 < need <= have, (L, C, outer, small, need, have)


def test_ticket_words_fit(calls):
    from gaviko_amd import ops
    most = 0
    for L, C, outer, small in calls:
        n = R.ticket_words([Ck for _, _, Ck in outer], [J * Lb if Lb else J for _, J, Lb in small])
        assert n <= ops.PGRAD_TICKETS, (L, C, outer, small, n)
        most = max(most, n)
    assert most >= 56                                                            # (the GPA gates' 3525 column sums alone take 56)
