"""Host restatement of gvk_conformal_scores and gvk_conformal_splits (gaviko_amd/csrc/conformal.hip) -- test infrastructure: the three
scores in numpy float32, one rounding per operation as include/gaviko_hip.h states them; the split kernel's integers from its definitions
(keys, argsort, per-segment order statistic, compares, histograms); and a deliberately naive second definition (sets built row by row from
the sorted probabilities, the quantile by np.sort of the calibration scores) that the restatement is checked against."""
import numpy as np

from dropmask import hash_u32

F32 = np.float32
KINDS = ("lac", "aps", "raps")


def row_u(seed: int, N: int) -> np.ndarray:
    """u_n = float(hash_u32(seed, n) >> 8) * 2^-24, float32 [N] (exact: 24 bits)"""
    return (hash_u32(seed, np.arange(N, dtype=np.uint64)) >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


def ranks(proba: np.ndarray) -> np.ndarray:
    """r[n, k] = #{j : p_j > p_k or (p_j == p_k and j < k)}, int64 [N, K]"""
    p = np.asarray(proba, dtype=F32)
    K = p.shape[1]
    j, k = np.arange(K)[:, None], np.arange(K)[None, :]
    above = (p[:, :, None] > p[:, None, :]) | ((p[:, :, None] == p[:, None, :]) & (j < k)[None])     # [n, j, k]
    return above.sum(1).astype(np.int64)


def scores(proba, kind="lac", randomized=False, seed=0, k_reg=1, lam=0.01) -> np.ndarray:
    """float32 [N, K] (row-major; the device buffer is its transpose), every operation a single float32 rounding"""
    p = np.ascontiguousarray(proba, dtype=F32)
    N, K = p.shape
    if kind == "lac":
        return F32(1.0) - p
    r = ranks(p)
    pi = np.argsort(r, axis=1, kind="stable")                               # pi[n, r] = the class of rank r
    rows = np.arange(N)
    c = np.zeros(N, dtype=F32)
    before, after = np.empty((N, K), dtype=F32), np.empty((N, K), dtype=F32)
    for q in range(K):
        c1 = (c + p[rows, pi[:, q]]).astype(F32)
        before[rows, pi[:, q]], after[rows, pi[:, q]] = c, c1
        c = c1
    if randomized:
        s = (before + (row_u(seed, N)[:, None] * p).astype(F32)).astype(F32)
    else:
        s = after
    if kind == "raps":
        pen = (F32(lam) * np.maximum(0, r + 1 - int(k_reg)).astype(F32)).astype(F32)
        s = (s + pen).astype(F32)
    return s


def tables(scores_kn: np.ndarray, labels: np.ndarray, mondrian: bool):
    """(order int64 [N], seg_off int64 [G + 1], sorted_score f32 [N]): the rows grouped by segment, ascending by true-class score inside, stable"""
    K, N = scores_kn.shape
    true = scores_kn[labels, np.arange(N)]
    order = np.argsort(true, kind="stable")
    if mondrian:
        order = order[np.argsort(labels[order], kind="stable")]
        off = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=K))]).astype(np.int64)
    else:
        off = np.array([0, N], dtype=np.int64)
    return order.astype(np.int64), off, true[order]


def split_keys(seed: int, b: int, N: int) -> np.ndarray:
    i = np.arange(N, dtype=np.uint64)
    return (hash_u32(seed, np.uint64(b * N) + i) & np.uint32(0xFFFFE000)) | i.astype(np.uint32)


def calibration_rows(seed: int, b: int, N: int, n_cal: int) -> np.ndarray:
    """bool [N]: the n_cal rows with the smallest keys"""
    cal = np.zeros(N, dtype=bool)
    cal[np.argsort(split_keys(seed, b, N), kind="stable")[:n_cal]] = True
    return cal


def level_m(n_g: int, alpha: float) -> int:
    """the order statistic asked for: (int)ceil((double)(n_g + 1) * (1.0 - alpha)), at least 1"""
    return max(1, int(np.ceil(np.float64(n_g + 1) * (1.0 - np.float64(alpha)))))


def splits(scores_kn, labels, order, seg_off, alphas, n_cal: int, R: int, seed: int) -> dict:
    """The outputs of gvk_conformal_splits, int32, plus qhat float32 [R, Q, G] (the thresholds as scores)."""
    S = np.ascontiguousarray(scores_kn, dtype=F32)
    K, N = S.shape
    labels = np.asarray(labels, dtype=np.int64)
    G, Q = len(seg_off) - 1, len(alphas)
    seg = (lambda k: 0) if G == 1 else (lambda k: k)
    true_sorted = S[labels[order], order]
    out = {"qpos": np.full((R, Q, G), -1, np.int32), "n_seg": np.zeros((R, G), np.int32), "size_hist": np.zeros((R, Q, K + 1), np.int32),
           "covered_by_size": np.zeros((R, Q, K + 1), np.int32), "class_test": np.zeros((R, K), np.int32),
           "class_covered": np.zeros((R, Q, K), np.int32), "qhat": np.full((R, Q, G), np.inf, F32)}
    col = np.array([seg(k) for k in range(K)])
    for b in range(R):
        cal = calibration_rows(seed, b, N, n_cal)
        flags = cal[order]
        for g in range(G):
            members = int(seg_off[g]) + np.nonzero(flags[seg_off[g]:seg_off[g + 1]])[0]      # sorted positions of the segment's calibration rows
            out["n_seg"][b, g] = members.size
            for q, a in enumerate(alphas):
                m = level_m(members.size, a)
                if m <= members.size:
                    out["qpos"][b, q, g] = members[m - 1]
                    out["qhat"][b, q, g] = true_sorted[members[m - 1]]
        test = np.nonzero(~cal)[0]
        y = labels[test]
        out["class_test"][b] = np.bincount(y, minlength=K)
        for q in range(Q):
            inset = S[:, test] <= out["qhat"][b, q, col][:, None]             # [K, n_test]
            size = inset.sum(0)
            covered = inset[y, np.arange(test.size)]
            out["size_hist"][b, q] = np.bincount(size, minlength=K + 1)
            out["covered_by_size"][b, q] = np.bincount(size[covered], minlength=K + 1)
            out["class_covered"][b, q] = np.bincount(y[covered], minlength=K)
    return out


# ---- the naive second definition ----------------------------------------------------------------------------------------------------
def naive_row_scores(p_row, kind, u=None, k_reg=1, lam=0.01):
    """one row: [(class, score)] in descending order of probability (ties: the lower class first), float32 arithmetic step by step"""
    ranked = sorted(range(len(p_row)), key=lambda k: (-float(p_row[k]), k))
    out, c = [], F32(0.0)
    for r, k in enumerate(ranked):
        pk = F32(p_row[k])
        if kind == "lac":
            s = F32(F32(1.0) - pk)
        else:
            s = F32(c + pk) if u is None else F32(c + F32(F32(u) * pk))
            if kind == "raps":
                s = F32(s + F32(F32(lam) * F32(max(0, r + 1 - k_reg))))
        c = F32(c + pk)
        out.append((k, s))
    return out


def naive_split(proba, labels, cal, alphas, kind="lac", mondrian=False, randomized=False, seed=0, k_reg=1, lam=0.01) -> dict:
    """One split, from the definitions alone: cal bool [N] marks the calibration rows.  The quantile is np.sort(calibration scores)[m - 1]
    (+inf when m exceeds their number), a test row's set is built class by class from its sorted probabilities.
    -> qhat f32 [Q, G], size_hist / covered_by_size [Q, K + 1], class_test [K], class_covered [Q, K]"""
    p = np.asarray(proba, dtype=F32)
    N, K = p.shape
    u = row_u(seed, N) if randomized else [None] * N
    rows = [dict(naive_row_scores(p[n], kind, u[n], k_reg, lam)) for n in range(N)]
    G, Q = (K if mondrian else 1), len(alphas)
    qhat = np.full((Q, G), np.inf, F32)
    for g in range(G):
        mine = np.sort(np.array([rows[n][labels[n]] for n in range(N) if cal[n] and (not mondrian or labels[n] == g)], dtype=F32))
        for q, a in enumerate(alphas):
            m = int(np.ceil((mine.size + 1) * (1.0 - a)))
            if m <= mine.size:                                                # m >= 1: alpha < 1
                qhat[q, g] = mine[m - 1]
    out = {"qhat": qhat, "size_hist": np.zeros((Q, K + 1), np.int64), "covered_by_size": np.zeros((Q, K + 1), np.int64),
           "class_test": np.zeros(K, np.int64), "class_covered": np.zeros((Q, K), np.int64)}
    for n in range(N):
        if cal[n]:
            continue
        out["class_test"][labels[n]] += 1
        for q in range(Q):
            chosen = {k for k, s in rows[n].items() if s <= qhat[q, k if mondrian else 0]}
            out["size_hist"][q, len(chosen)] += 1
            if labels[n] in chosen:
                out["covered_by_size"][q, len(chosen)] += 1
                out["class_covered"][q, labels[n]] += 1
    return out


# ---- evaluation sets ----------------------------------------------------------------------------------------------------------------
def case(N: int, K: int, seed: int, ties: bool = False, sizes=None):
    """(proba f32 [N, K], labels int64 [N]): the float32 softmax of noise + 2 on the label's column.  ties: probabilities quantised to
    multiples of 1/16 (most rows then hold equal probabilities in several classes, and many rows share a true-class score), with the first
    class duplicated into the last, and a one-hot row at row 0.  sizes: the class sizes (labels shuffled), else uniform labels."""
    g = np.random.default_rng(seed)
    labels = g.permutation(np.repeat(np.arange(K), sizes)) if sizes is not None else g.integers(0, K, N)
    labels = labels.astype(np.int64)
    assert labels.size == N
    z = g.standard_normal((N, K)) + 2.0 * np.eye(K)[labels]
    e = np.exp(z - z.max(1, keepdims=True))
    p = (e / e.sum(1, keepdims=True)).astype(F32)
    if ties:
        p = (np.round(p * 16) / 16).astype(F32)
        p[:, K - 1] = p[:, 0]
        p[0] = 0
        p[0, K // 2] = 1
    return p, labels
