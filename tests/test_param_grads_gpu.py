"""-m gpu: gvk_param_grads (csrc/paramgrad.hip) against tests/param_grads_ref.py, EXACTLY.

The kernel multiplies on the fp32 matrix cores and adds in fp32.  Every input here is a small integer (rstd from {0.5, 1, 2}, the dropout
scale exactly 2), so every term is a multiple of 0.5, and every test asserts on the host -- from the reference's sums of absolute term
values -- that each output's terms stay below 2^23 in total.  Every partial sum is then a float32 without rounding whatever the order, and
the kernel has to equal the integer reference bit for bit: torch.equal, no tolerance anywhere in this file.

Every launch goes through `launch` below, which also
  * fills the scratch with NaN first (a partial that is read but was never written poisons the result),
  * keeps every destination inside a larger buffer with 64 sentinel floats on either side (one torch.equal of the whole buffer checks the
    values and the guard bands),
  * checks that the ticket words are zero afterwards, on ONE ticket tensor shared by every launch of the file (so each launch inherits the
    words a different job mix left behind),
  * sizes the scratch by ops.param_grads_scratch_elems to the float (the wrapper's bound is then under test too).

The case functions (case_*) take the shared state `pg`; with pg.dev None they run dry and only record the shapes of their calls, which is
how tests/test_param_grads.py checks the scratch and ticket bounds of exactly these calls without a GPU.

The row counts of case_plain come from the code: a k-step is 4 rows, a wave takes chunks of 16 rows (below M = 4 some waves have no row),
a pipeline trip is 4 chunks (256 rows per workgroup), kPgMinRows = 128 rows per workgroup (a second row range from 129 rows on), the last
arriver sums the ranges in batches of 16 (16 / 17 ranges at 2048 / 2049 rows of one column tile), kPgMaxSg = 64 caps the ranges (8200
rows).  Dropout needs a seed word (the host refuses drop_p > 0 without one, case (g)), so "with and without seed_ptr" is a zero and a
non-zero word here: the job's own seed alone, and seed + word."""
import numpy as np
import pytest
import torch

import param_grads_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = [4, 8, 12, 16, 20, 24, 28]
GUARD = 64
SENT = -54321.0
PLAIN_M = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 2048, 2049, 8200]
PLAIN_C = [4, 60, 64, 68, 132]
PLAIN_SHAPES = [(M, C) for C in (4, 68) for M in PLAIN_M] + [(M, C) for M in (5, 129, 2049) for C in (60, 64, 132)]
PLAIN_VARIANTS = [(0, True, True), (1, True, True), (0, True, False), (1, True, False), (0, False, True)]     # transposed, out, colsum
ONEHOT_SHAPES = [(17, 4), (129, 68), (2049, 132), (8200, 68)]


class PG:
    """What the launches of this file share: the device, ONE ticket tensor, a scratch pool.  dev None = dry run (shapes only)."""

    def __init__(self, dev):
        self.dev, self.dry, self.calls, self.pool = dev, dev is None, [], None
        if not self.dry:
            from gaviko_amd import ops
            self.tick = torch.zeros(ops.PGRAD_TICKETS, dtype=torch.int32, device=dev)

    def ints(self, rng, shape, lo, hi):
        return np.zeros(shape, np.int8) if self.dry else rng.integers(lo, hi + 1, shape).astype(np.int8)

    def choice(self, rng, shape, values):
        return np.zeros(shape) if self.dry else rng.choice(np.asarray(values, np.float64), shape)

    def up(self, a):
        return None if self.dry or a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)

    def scratch(self, n):
        if self.pool is None or self.pool.numel() < n:
            self.pool = torch.empty(max(n, 1 << 20), device=self.dev)
        s = self.pool[:n]
        s.fill_(float("nan"))
        return s


@pytest.fixture(scope="module")
def pg(dev):
    return PG(dev)


class Src:
    """Input arrays of one or more jobs: the host copy (what the reference reads) and, uploaded once, the float32 device copy."""

    def __init__(self, pg, **arrays):
        self.np = {k: v for k, v in arrays.items() if v is not None}
        self.t = {k: pg.up(v) for k, v in self.np.items()}

    def plus(self, other):
        """These arrays and `other`'s, sharing the uploaded copies of both."""
        both = Src(None)
        both.np, both.t = dict(self.np, **other.np), dict(self.t, **other.t)
        return both


class Dest:
    """A destination of n floats inside a buffer with GUARD sentinel floats on both sides, prefilled with integers."""

    def __init__(self, pg, n, rng):
        self.n = n
        self.host = np.full(n + 2 * GUARD, SENT, np.float32)
        self.host[GUARD:GUARD + n] = pg.ints(rng, n, -3, 3)
        self.buf = pg.up(self.host)
        self.view = None if pg.dry else self.buf[GUARD:GUARD + n]

    def prev(self):
        return self.host[GUARD:GUARD + self.n].astype(np.float64)

    def check(self, pg, value, what):
        v32 = np.asarray(value, np.float64).reshape(-1).astype(np.float32)
        assert np.array_equal(v32.astype(np.float64), np.asarray(value, np.float64).reshape(-1)), f"{what}: the reference is no float32"
        self.host[GUARD:GUARD + self.n] = v32
        if torch.equal(self.buf, pg.up(self.host)):
            return
        got = self.buf.cpu().numpy()
        g0, g1 = got[:GUARD], got[GUARD + self.n:]
        assert np.array_equal(g0, self.host[:GUARD]) and np.array_equal(g1, self.host[GUARD + self.n:]), \
            f"{what}: guard band overwritten ({int((g0 != SENT).sum())} floats in front, {int((g1 != SENT).sum())} behind)"
        bad = np.flatnonzero(~(got == self.host))
        raise AssertionError(f"{what}: {bad.size} of {self.n} elements differ, first at {bad[0] - GUARD}: got {got[bad[0]]!r}, "
                             f"want {self.host[bad[0]]!r}")


_SRC_FIELDS = ("narrow", "wide", "narrow2", "wide2", "lat_override", "mean", "rstd", "aff_w", "aff_gamma", "aff_beta")
_DEST_FIELDS = {"out": "out", "colsum": "colsum", "dgamma": "aff_dgamma", "dbeta": "aff_dbeta", "dbias": "aff_dbias"}


class Outer:
    """One gvk_pgrad_outer job: inputs from `src`, guarded destinations of its own, the reference's view of their contents."""

    def __init__(self, pg, L, C, src, rng, T=0, P=0, drop_p=0.0, seed=0, transposed=0, out=True, colsum=False, dbias=True, own_C=False):
        s = src.np
        self.src, self.C, self.aff = src, C, "aff_w" in s
        self.M, self.M2 = s["narrow"].shape[0], (s["narrow2"].shape[0] if "narrow2" in s else 0)
        self.ref_kw = dict({k: s.get(k) for k in _SRC_FIELDS}, T=T, P=P, drop_p=drop_p, seed=seed, transposed=bool(transposed), want_out=out,
                           want_colsum=colsum, want_dbias=dbias)
        sizes = {}
        if out:
            sizes["out"] = L * C
        if colsum:
            sizes["colsum"] = C
        if self.aff:
            sizes.update(dgamma=C, dbeta=C)
            if dbias:
                sizes["dbias"] = L
        self.dest = {k: Dest(pg, n, rng) for k, n in sizes.items()}
        self.scalars = dict(M=self.M, M2=self.M2, T=T, P=P, transposed=int(transposed), C=C if own_C else 0, drop_p=drop_p, seed=seed)

    def job(self, acc):
        d = dict(self.scalars, accumulate=int(acc))
        d.update({k: self.src.t[k] for k in _SRC_FIELDS if k in self.src.t})
        d.update({_DEST_FIELDS[k]: v.view for k, v in self.dest.items()})
        return d

    def expect(self, acc, seed_word):
        prev = {k: d.prev() for k, d in self.dest.items()} if acc else None
        return R.outer(**self.ref_kw, seed_word=seed_word, prev=prev)


class Small:
    """One gvk_reduce_job: column sums of a (+ a2), or the product a^T b."""

    def __init__(self, pg, rng, a, b=None, a2=None, ta=None, tb=None, ta2=None):
        self.a, self.b, self.a2 = a, b, a2
        self.ta = pg.up(a) if ta is None else ta
        self.tb = pg.up(b) if tb is None else tb
        self.ta2 = pg.up(a2) if ta2 is None else ta2
        self.rows, self.J, self.Lb = a.shape[0] + (a2.shape[0] if a2 is not None else 0), a.shape[1], (b.shape[1] if b is not None else 0)
        self.nout = self.J * self.Lb if b is not None else self.J
        self.dest = Dest(pg, self.nout, rng)

    def job(self, acc):
        return (self.ta, self.tb, self.dest.view, int(acc)) + ((self.ta2,) if self.a2 is not None else ())

    def expect(self, acc):
        return R.small(self.a, self.b, self.a2, prev=self.dest.prev().reshape((self.J, self.Lb) if self.b is not None else (self.J,)) if acc else None)


def launch(pg, C, L, outers=(), smalls=(), acc=0, seed_word=None, what=""):
    """One gvk_param_grads call and every check that goes with it (module docstring)."""
    pg.calls.append((L, C, tuple((o.M, o.M2, o.C) for o in outers), tuple((s.rows, s.J, s.Lb) for s in smalls)))
    if pg.dry:
        return
    from gaviko_amd import ops
    what = f"{what} L={L} C={C} acc={acc}"
    ex_o = [o.expect(acc, seed_word or 0) for o in outers]
    ex_s = [s.expect(acc) for s in smalls]
    for k, r in enumerate(ex_o):
        assert R.exact(*r.values()), f"{what}: outer job {k}: the inputs break the exactness condition (a term sum reaches 2^23)"
    assert R.exact(*ex_s), f"{what}: a small job's inputs break the exactness condition"
    scratch = pg.scratch(ops.param_grads_scratch_elems(L, [(o.C + 63) // 64 for o in outers], [s.nout for s in smalls]))
    seedw = None if seed_word is None else torch.full((1,), seed_word, dtype=torch.int64, device=pg.dev)
    ops.param_grads([o.job(acc) for o in outers], [s.job(acc) for s in smalls], scratch, pg.tick, C, L, seed_ptr=seedw)
    for k, (o, r) in enumerate(zip(outers, ex_o)):
        for name, d in o.dest.items():
            d.check(pg, r[name][0], f"{what}: outer job {k} (M={o.M} M2={o.M2} C={o.C}) {name}")
    for k, (s, r) in enumerate(zip(smalls, ex_s)):
        s.dest.check(pg, r[0], f"{what}: small job {k} (rows={s.rows} J={s.J} L={s.Lb})")
    assert int(pg.tick.abs().max()) == 0, f"{what}: ticket words not zero after the launch"


def _rng(*key):
    return np.random.default_rng([20261021, *key])


# ------------------------------------------------------------------ (a) plain outer product, every width
def case_plain(pg, L):
    for M, C in PLAIN_SHAPES:
        rng = _rng(1, L, M, C)
        src = Src(pg, narrow=pg.ints(rng, (M, L), -3, 3), wide=pg.ints(rng, (M, C), -3, 3))
        for tr, out, cs in PLAIN_VARIANTS:
            job = Outer(pg, L, C, src, rng, transposed=tr, out=out, colsum=cs)
            for acc in (0, 1, 1):
                launch(pg, C, L, [job], acc=acc, what=f"plain tr={tr} out={out} colsum={cs}")
    for M, C in ONEHOT_SHAPES:                     # narrow row m = e_(m mod L), one non-zero per wide row: the output says which rows were counted
        m = np.arange(M)
        narrow, wide = np.zeros((M, L), np.int8), np.zeros((M, C), np.int8)
        narrow[m, m % L] = 1
        wide[m, m % C] = (m % 7) - 3
        src = Src(pg, narrow=narrow, wide=wide)
        for tr in (0, 1):
            job = Outer(pg, L, C, src, _rng(2, L, M, C), transposed=tr, colsum=True)
            for acc in (0, 1):
                launch(pg, C, L, [job], acc=acc, what=f"one-hot tr={tr}")


@pytest.mark.parametrize("L", WIDTHS)
def test_plain_outer_product_at_every_width(pg, L):
    """(a) out / colsum of one job, both layouts, with and without either output, overwrite and two accumulating calls, at the row counts
    and column counts where the row partition and the column tiling change (module docstring); plus the one-hot inputs."""
    case_plain(pg, L)


# ------------------------------------------------------------------ (b) two token streams
def case_two_streams(pg, L):
    k = 0
    for C in (60, 132):
        for M in (1, 3, 17, 130):
            for M2 in (1, 5, 64, 131):
                rng = _rng(3, L, C, M, M2)
                src = Src(pg, narrow=pg.ints(rng, (M, L), -3, 3), wide=pg.ints(rng, (M, C), -3, 3),
                          narrow2=pg.ints(rng, (M2, L), -3, 3), wide2=pg.ints(rng, (M2, C), -3, 3))
                job = Outer(pg, L, C, src, rng, transposed=k & 1, colsum=bool(k & 2))
                bias = Small(pg, rng, src.np["narrow"], a2=src.np["narrow2"], ta=src.t["narrow"], ta2=src.t["narrow2"])
                k += 1
                for acc in (0, 1):
                    launch(pg, C, L, [job], [bias], acc=acc, what="two streams")


@pytest.mark.parametrize("L", [8, 16, 28])
def test_two_token_streams_joined_at_any_row(pg, L):
    """(b) the second source appended after row M, with the boundary inside a k-step, inside a chunk and across a row-range boundary; the
    two-source column sum of the narrow rows (proj_down's bias) rides along as a small job."""
    case_two_streams(pg, L)


# ------------------------------------------------------------------ (c) override rows
def case_override(pg, L):
    for B, T, P in ((1, 1, 1), (3, 5, 1), (3, 5, 5), (2, 33, 8), (2, 1033, 32)):
        for C in (60, 132):
            rng = _rng(4, L, B, T, P, C)
            M = B * T
            enh = pg.choice(rng, (B, P, L), [-3.0, 3.0])                  # disjoint from the xl values: a row read from the wrong source shows
            src = Src(pg, narrow=pg.ints(rng, (M, L), -2, 2), wide=pg.ints(rng, (M, C), -3, 3), lat_override=enh)
            for tr in (1, 0):
                job = Outer(pg, L, C, src, rng, T=T, P=P, transposed=tr, colsum=bool(tr))
                for acc in (0, 1):
                    launch(pg, C, L, [job], acc=acc, what=f"override B={B} T={T} P={P} tr={tr}")


@pytest.mark.parametrize("L", [4, 20, 24])
def test_override_rows_of_every_sample(pg, L):
    """(c) narrow rows t < P of every T-row sample come from lat_override (values +-3 against [-2, 2] elsewhere)."""
    case_override(pg, L)


# ------------------------------------------------------------------ (d) mean / rstd, dropout, the affine epilogue
def case_ln_drop_affine(pg, L):
    for M in (1, 17, 129, 600):
        for C in (60, 64, 132):
            rng = _rng(5, L, M, C)
            narrow, wide = pg.ints(rng, (M, L), -3, 3), pg.ints(rng, (M, C), -3, 3)
            mean, rstd = pg.ints(rng, (M,), -2, 2), pg.choice(rng, (M,), [0.5, 1.0, 2.0])
            aff = Src(pg, aff_w=pg.ints(rng, (L, C), -2, 2), aff_gamma=pg.ints(rng, (C,), -2, 2), aff_beta=pg.ints(rng, (C,), -2, 2))
            plain = Src(pg, narrow=narrow, wide=wide)
            ln = plain.plus(Src(pg, mean=mean, rstd=rstd))
            aff_plain, aff_ln = plain.plus(aff), ln.plus(aff)
            w = f"M={M}"
            # each alone
            launch(pg, C, L, [Outer(pg, L, C, ln, rng, colsum=True)], what=w + " mean/rstd")
            launch(pg, C, L, [Outer(pg, L, C, ln, rng, transposed=1)], what=w + " mean/rstd transposed")
            drop = Outer(pg, L, C, plain, rng, drop_p=0.5, seed=2 * M + 1, transposed=1, colsum=True)
            launch(pg, C, L, [drop], seed_word=0, what=w + " dropout, zero seed word")
            launch(pg, C, L, [drop], seed_word=77123 + C, acc=1, what=w + " dropout, seed word")
            for src, dbias, name in ((aff_plain, False, " affine, no dbias"), (aff_ln, True, " affine + mean/rstd")):
                job = Outer(pg, L, C, src, rng, dbias=dbias)
                for acc in (0, 1):
                    launch(pg, C, L, [job], acc=acc, what=w + name)
            # together, as the MWSA stream issues them: proj_up behind dropout beside LayerNorm + proj_down through the affine epilogue
            jobs = [Outer(pg, L, C, plain, rng, drop_p=0.5, seed=9, transposed=1, colsum=True), Outer(pg, L, C, aff_ln, rng)]
            for acc in (0, 1):
                launch(pg, C, L, jobs, seed_word=4242, acc=acc, what=w + " dropout job + affine job")
            # one job with both: the mask applies to the element, the row statistics to the masked element
            launch(pg, C, L, [Outer(pg, L, C, ln, rng, drop_p=0.5, seed=3, colsum=True)], seed_word=11, what=w + " dropout + mean/rstd in one job")


@pytest.mark.parametrize("L", [8, 16, 20, 28])
def test_row_statistics_dropout_and_affine_epilogue(pg, L):
    """(d) wide' = (wide - mean) * rstd, the regenerated dropout mask (p = 0.5: the scale is exactly 2), the LayerNorm-affine epilogue
    (dWd, dgamma, dbeta, dbias given and absent, accumulating), each alone and in one call."""
    case_ln_drop_affine(pg, L)


# ------------------------------------------------------------------ (e) small jobs
SMALL_J = [1, 63, 64, 65, 3525]
SMALL_M = [1, 31, 33, 256, 257, 8192, 8193, 8300]
PROD_JL = [(4, 4), (20, 20), (60, 20), (84, 28)]
PROD_M = [1, 33, 257, 600]
A2_MM = [(1, 1), (5, 3), (30, 7), (257, 131)]


def case_small(pg):
    rng = _rng(6)
    big = {J: pg.ints(rng, (max(SMALL_M), J), -3, 3) for J in SMALL_J}          # rows [:M] of one array per width: uploaded once
    tbig = {J: pg.up(a) for J, a in big.items()}
    for M in SMALL_M:
        jobs = [Small(pg, rng, big[J][:M], ta=None if pg.dry else tbig[J][:M]) for J in SMALL_J]
        for acc in (0, 1):
            launch(pg, 64, 20, [], jobs, acc=acc, what=f"column sums M={M}")
    pa = {JL: (pg.ints(rng, (max(PROD_M), JL[0]), -3, 3), pg.ints(rng, (max(PROD_M), JL[1]), -3, 3)) for JL in PROD_JL}
    tpa = {JL: (pg.up(a), pg.up(b)) for JL, (a, b) in pa.items()}
    for M in PROD_M:
        jobs = [Small(pg, rng, pa[JL][0][:M], pa[JL][1][:M], ta=None if pg.dry else tpa[JL][0][:M], tb=None if pg.dry else tpa[JL][1][:M])
                for JL in PROD_JL]
        for acc in (0, 1):
            launch(pg, 64, 20, [], jobs, acc=acc, what=f"products M={M}")
    jobs = [Small(pg, rng, pg.ints(rng, (M, J), -3, 3), a2=pg.ints(rng, (M2, J), -3, 3)) for M, M2 in A2_MM for J in (20, 65)]
    for acc in (0, 1):
        launch(pg, 64, 20, [], jobs, acc=acc, what="two-source column sums")


def test_small_jobs(pg):
    """(e) the column sums (1 to 32 row slabs, past 32 x 256 rows, 1 to 56 output chunks), the J x L products and the two-source column
    sum with its boundary inside the 8-row unroll -- calls with no outer job at all."""
    case_small(pg)


# ------------------------------------------------------------------ (f) the engine's two mixes and the fullest list
def gpa_mix(pg, L, C, B, T, P, N, ng, key):
    """The GPA stream's call (engine_gaviko.py): proj_up over override rows (transposed, colsum), proj_down fed by both token streams, the
    gate parameters' column sums, two L x L products with their bias sums, proj_down's bias over both streams."""
    rng = _rng(7, L, C, B, T, key)
    M, BN, BP = B * T, B * N, B * P
    up = Src(pg, narrow=pg.ints(rng, (M, L), -2, 2), wide=pg.ints(rng, (M, C), -3, 3), lat_override=pg.choice(rng, (B, P, L), [-3.0, 3.0]))
    down = Src(pg, narrow=pg.ints(rng, (M, L), -3, 3), wide=pg.ints(rng, (M, C), -3, 3),
               narrow2=pg.ints(rng, (BN, L), -3, 3), wide2=pg.ints(rng, (BN, C), -3, 3))
    outers = [Outer(pg, L, C, up, rng, T=T, P=P, transposed=1, colsum=True), Outer(pg, L, C, down, rng)]
    gp, dqg, dql, prm = pg.ints(rng, (B, ng), -3, 3), pg.ints(rng, (BP, L), -3, 3), pg.ints(rng, (BP, L), -3, 3), pg.ints(rng, (BP, L), -3, 3)
    tg, tl, tp = pg.up(dqg), pg.up(dql), pg.up(prm)
    smalls = [Small(pg, rng, gp), Small(pg, rng, dqg, prm, ta=tg, tb=tp), Small(pg, rng, dqg, ta=tg), Small(pg, rng, dql, prm, ta=tl, tb=tp),
              Small(pg, rng, dql, ta=tl), Small(pg, rng, down.np["narrow"], a2=down.np["narrow2"], ta=down.t["narrow"], ta2=down.t["narrow2"])]
    return outers, smalls


def mwsa_mix(pg, L, C, B, N, key, small=True):
    """The MWSA stream's call: proj_up behind proj_drop, LayerNorm + proj_down through the affine epilogue, the qkv matrix as a third job
    of 3L columns (and the same product as a small job, as test_param_grads_one_launch runs it)."""
    rng = _rng(8, L, C, B, N, key)
    BN = B * N
    upj = Src(pg, narrow=pg.ints(rng, (BN, L), -3, 3), wide=pg.ints(rng, (BN, C), -3, 3))
    aff = Src(pg, narrow=pg.ints(rng, (BN, L), -3, 3), wide=pg.ints(rng, (BN, C), -3, 3), mean=pg.ints(rng, (BN,), -2, 2),
              rstd=pg.choice(rng, (BN,), [0.5, 1.0, 2.0]), aff_w=pg.ints(rng, (L, C), -2, 2), aff_gamma=pg.ints(rng, (C,), -2, 2),
              aff_beta=pg.ints(rng, (C,), -2, 2))
    qkv = Src(pg, narrow=pg.ints(rng, (BN, L), -3, 3), wide=pg.ints(rng, (BN, 3 * L), -3, 3))
    outers = [Outer(pg, L, C, upj, rng, drop_p=0.5, seed=2 * 7 + 1, transposed=1, colsum=True), Outer(pg, L, C, aff, rng),
              Outer(pg, L, 3 * L, qkv, rng, transposed=1, own_C=True)]
    smalls = [Small(pg, rng, qkv.np["wide"], qkv.np["narrow"], ta=qkv.t["wide"], tb=qkv.t["narrow"])] if small else []
    return outers, smalls


def _twice_then_accumulate(pg, C, L, outers, smalls, seed_word, what):
    """Overwrite twice back to back (both must give the reference's bits, hence each other's), then accumulate."""
    for acc in (0, 0, 1):
        launch(pg, C, L, outers, smalls, acc=acc, seed_word=seed_word, what=what)


def case_mixes(pg, L, gate_count):
    B, T, P, N = 2, 41, 8, 27
    for C in (64, 192):
        _twice_then_accumulate(pg, C, L, *gpa_mix(pg, L, C, B, T, P, N, gate_count(L, P), 0), None, "GPA mix")
        _twice_then_accumulate(pg, C, L, *mwsa_mix(pg, L, C, B, N, 0), 77123, "MWSA mix")


def case_product_shape(pg, gate_count):
    L, C, B, T, P, N = 20, 768, 2, 1033, 32, 1000
    _twice_then_accumulate(pg, C, L, *gpa_mix(pg, L, C, B, T, P, N, gate_count(L, P), 1), None, "GPA mix, product shape")
    _twice_then_accumulate(pg, C, L, *mwsa_mix(pg, L, C, B, N, 1), 77123, "MWSA mix, product shape")


def case_fullest(pg):
    L, C, B, T, P, N = 24, 132, 2, 41, 8, 27
    rng = _rng(9)
    outers, one = mwsa_mix(pg, L, C, B, N, 2)
    _, six = gpa_mix(pg, L, C, B, T, P, N, 700, 2)
    smalls = one + six + [Small(pg, rng, pg.ints(rng, (300, 65), -3, 3))]
    assert len(outers) == 3 and len(smalls) == 8
    _twice_then_accumulate(pg, C, L, outers, smalls, 5, "3 outer + 8 small jobs")


def _gate_count(L, P):
    from gaviko_amd import ops
    return ops.gpa_gate_param_count(L, P)


@pytest.mark.parametrize("L", WIDTHS)
def test_engine_job_mixes_at_every_width(pg, L):
    """(f) the GPA mix (2 outer + 6 small jobs) and the MWSA mix (3 outer jobs, the third 3L columns wide: two column tiles from L = 24,
    + 1 small) at a small token grid, each twice back to back with the same bits, then accumulating."""
    case_mixes(pg, L, _gate_count)


def test_engine_job_mixes_at_the_product_shape(pg):
    """(f) both mixes at T = 1033, N = 1000, C = 768, L = 20 -- what test_param_grads_one_launch covers within a bound, here exactly."""
    case_product_shape(pg, _gate_count)


def test_fullest_job_list(pg):
    """(f) one call with 3 outer and 8 small jobs."""
    case_fullest(pg)


# ------------------------------------------------------------------ (g) refusals
def test_refusals_leave_the_wrapper_usable(pg):
    """(g) Every call below is refused by the LIBRARY (gvk_param_grads, csrc/paramgrad.hip: the wrapper's own checks -- dtype, device, element
    counts -- pass on purpose, the message is matched against the source's), launches nothing, and leaves the ticket words zero; after
    each one a small valid call gives the exact result."""
    from gaviko_amd import lib, ops
    dev, L, C, M = pg.dev, 8, 64, 40
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    nar, wid, out, col, vecM, vecC = z(M, L), z(M, C), z(L * C), z(C), z(M), z(C)
    sc = z(ops.param_grads_scratch_elems(L, [1, 1, 1, 1], [64] * 9))
    ok = dict(narrow=nar, wide=wid, out=out, M=M)
    aff = dict(ok, aff_w=z(L, C), aff_gamma=vecC, aff_beta=vecC, aff_dgamma=z(C), aff_dbeta=z(C))
    two = dict(ok, narrow2=nar, wide2=wid, M2=M)
    sm = (nar, None, z(L), 0)
    seedw = torch.zeros(1, dtype=torch.int64, device=dev)
    rng = _rng(10)
    probe = Outer(pg, L, C, Src(pg, narrow=pg.ints(rng, (M, L), -3, 3), wide=pg.ints(rng, (M, C), -3, 3)), rng, colsum=True)

    def refused(match, outer, small=(), C_=C, L_=L, scratch=sc, tick=None, seed_ptr=None):
        with pytest.raises(lib.GavikoHipError, match=r"gvk_param_grads failed.*" + match):
            ops.param_grads(list(outer), list(small), scratch, pg.tick if tick is None else tick, C_, L_, seed_ptr=seed_ptr)
        assert int(pg.tick.abs().max()) == 0
        launch(pg, C, L, [probe], what="after a refusal: " + match)

    refused("up to 3 outer and 8 small jobs", [ok] * 4)
    refused("up to 3 outer and 8 small jobs", [ok], [sm] * 9)
    refused("L=6 a multiple of 4 up to 28", [ok], L_=6)
    refused("L=32 a multiple of 4 up to 28", [dict(ok, narrow=z(M, 32), out=z(32 * C))], L_=32)
    refused("C=6 must be a multiple of 4", [ok], C_=6)
    refused(r"outer job 0: C=6 must be a multiple of 4", [dict(ok, C=6)])
    refused("override needs 0 < P <= T", [dict(ok, lat_override=z(M, L), T=4, P=5)])
    refused("the second source takes plain rows only", [dict(two, mean=vecM, rstd=vecM)])
    refused("the second source takes plain rows only", [dict(two, lat_override=z(M, L), T=8, P=2)])
    refused("the second source takes plain rows only", [dict(two, drop_p=0.5)], seed_ptr=seedw)
    refused("the affine epilogue needs", [dict(aff, transposed=1)])
    refused("the affine epilogue needs", [dict(aff, colsum=col)])
    refused("mean / rstd must come together", [dict(ok, mean=vecM)])
    refused(r"drop_p in \[0,1\) and a seed word", [dict(ok, drop_p=0.5)])
    refused("1 ticket words given, 2 needed", [ok, ok], tick=torch.zeros(1, dtype=torch.int32, device=dev))
    refused("scratch holds 64 floats", [ok], scratch=z(64))
