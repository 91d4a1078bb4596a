"""Reference of gvk_param_grads (include/gaviko_hip.h: the gvk_pgrad_outer and gvk_reduce_job comments) in float64 -- numpy only, no
torch, no GPU, and nothing of the kernel's tiling: whole-matrix products over all rows at once.

Every output comes as a pair (value, budget).  budget = the sum of the ABSOLUTE values of the terms that make up that output (the previous
contents of an accumulating destination included).  It is the exactness budget of the integer tests: when every input is a multiple of
0.5 and every budget stays below 2^23, every partial sum of those terms, in any order and any grouping, is a float32 without rounding, so
a kernel that sums on fp32 hardware must reproduce `value` bit for bit (tests/test_param_grads_gpu.py)."""
import numpy as np

import dropmask

EXACT = float(2 ** 23)


def _f(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def narrow_rows(narrow, lat_override=None, T=0, P=0):
    """narrow' [M][L]: row m = s*T + t of `narrow`, but lat_override[s*P + t] where t < P."""
    comb = np.array(narrow, dtype=np.float64)
    if lat_override is None:
        return comb
    if not 0 < P <= T:
        raise ValueError("override needs 0 < P <= T")
    M, L = comb.shape
    ov = _f(lat_override).reshape(-1, L)
    m = np.arange(M)
    s, t = m // T, m % T
    sel = t < P
    comb[sel] = ov[s[sel] * P + t[sel]]
    return comb


def wide_rows(wide, mean=None, rstd=None, drop_p=0.0, seed=0, seed_word=0):
    """wide' [M][C]: element (m, c) times the dropout mask of index m*C + c (seed + the seed word), then (. - mean[m]) * rstd[m] -- the
    order both the one-launch kernel and gvk_outer_reduce apply them in (a dropped input in front of the row normalisation)."""
    w = np.array(wide, dtype=np.float64)
    if drop_p > 0:
        w = w * dropmask.rows_mask(int(seed) + int(seed_word), w.shape[0], w.shape[1], drop_p).astype(np.float64)
    if (mean is None) != (rstd is None):
        raise ValueError("mean / rstd must come together")
    if mean is not None:
        w = (w - _f(mean).reshape(-1, 1)) * _f(rstd).reshape(-1, 1)
    return w


def _acc(value, budget, prev):
    if prev is None:
        return value, budget
    prev = _f(prev).reshape(value.shape)
    return prev + value, np.abs(prev) + budget


def outer(narrow, wide, narrow2=None, wide2=None, lat_override=None, T=0, P=0, mean=None, rstd=None, drop_p=0.0, seed=0, seed_word=0,
          transposed=False, want_out=True, want_colsum=False, aff_w=None, aff_gamma=None, aff_beta=None, want_dbias=True, prev=None):
    """One gvk_pgrad_outer job -> {name: (value, budget)}.  prev = {name: previous contents} makes the job an accumulating one (names:
    out, colsum, dgamma, dbeta, dbias).  With aff_w the job has the LayerNorm-affine epilogue; the raw Q and S it is made of are returned
    too (names Q, S) because their budgets bound the kernel's intermediate sums."""
    prev = prev or {}
    n = narrow_rows(narrow, lat_override, T, P)
    w = wide_rows(wide, mean, rstd, drop_p, seed, seed_word)
    if narrow2 is not None:
        if mean is not None or lat_override is not None or drop_p > 0:
            raise ValueError("the second source takes plain rows only")
        n = np.concatenate([n, _f(narrow2)], axis=0)
        w = np.concatenate([w, _f(wide2)], axis=0)
    Q, aQ = n.T @ w, np.abs(n).T @ np.abs(w)                     # [L][C]
    res = {}
    if aff_w is None:
        if want_out:
            res["out"] = _acc(Q.T.copy(), aQ.T.copy(), prev.get("out")) if transposed else _acc(Q, aQ, prev.get("out"))
        if want_colsum:
            res["colsum"] = _acc(w.sum(0), np.abs(w).sum(0), prev.get("colsum"))
        return res
    if transposed or want_colsum:
        raise ValueError("the affine epilogue takes out [L][C] and no colsum")
    S, aS = n.sum(0), np.abs(n).sum(0)                           # [L]
    W, g, b = _f(aff_w), _f(aff_gamma), _f(aff_beta)
    res["Q"], res["S"] = (Q, aQ), (S, aS)
    res["out"] = _acc(g[None, :] * Q + b[None, :] * S[:, None], np.abs(g)[None, :] * aQ + np.abs(b)[None, :] * aS[:, None], prev.get("out"))
    res["dgamma"] = _acc((W * Q).sum(0), (np.abs(W) * aQ).sum(0), prev.get("dgamma"))
    res["dbeta"] = _acc((W * S[:, None]).sum(0), (np.abs(W) * aS[:, None]).sum(0), prev.get("dbeta"))
    if want_dbias:
        res["dbias"] = _acc(S.copy(), aS.copy(), prev.get("dbias"))
    return res


def small(a, b=None, a2=None, prev=None):
    """One gvk_reduce_job -> (value, budget): b is None: out[j] = sum_m a[m][j] (+ the rows of a2); else out[j][l] = sum_m a[m][j] b[m][l]."""
    a = _f(a)
    if b is None:
        if a2 is not None:
            a = np.concatenate([a, _f(a2)], axis=0)
        return _acc(a.sum(0), np.abs(a).sum(0), prev)
    if a2 is not None:
        raise ValueError("a second source goes with a column sum only")
    b = _f(b)
    return _acc(a.T @ b, np.abs(a).T @ np.abs(b), prev)


def exact(*pairs):
    """Do all these (value, budget) pairs satisfy the exactness condition (budget < 2^23 everywhere)?"""
    return all(float(np.max(bud, initial=0.0)) < EXACT for _, bud in pairs)


# ------------------------------------------------------------------ sizes (the host side of gvk_param_grads, restated)
def ticket_words(outer_cols, small_outputs):
    """Ticket words one call needs: one per 64-column tile of every outer job and one per 64 outputs of every small job."""
    return sum((c + 63) // 64 for c in outer_cols) + sum((o + 63) // 64 for o in small_outputs)
