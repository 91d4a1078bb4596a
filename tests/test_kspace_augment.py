"""CPU: the host half of RandomGhosting / RandomSpike / RandomGamma / RandomAnisotropy (gaviko_amd/data.py): the tables the kernels of
csrc/kspace.hip consume against the literal np.fft algorithms and direct float64 evaluations of tests/kspace_ref.py, the parameter
sampling, and that a compose without the new transforms consumes the random stream it consumed before they existed."""
import math

import numpy as np
import pytest

import kspace_ref
from gaviko_amd import data, ops


def _vol(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape) * 300 + 1000


# ---- ghosting: the convolution row is the spectrum edit ---------------------------------------------------------------------------------
# (shape, axis, n, g): even and odd N, n dividing N and not, n > N, g = 1, n = 1 (every plane but the centre)
GHOST = [((8, 6, 10), 0, 2, 0.7), ((8, 6, 10), 1, 4, 0.5), ((8, 6, 10), 2, 3, 1.0), ((7, 9, 5), 0, 3, 0.6), ((7, 9, 5), 1, 3, 1.0),
         ((7, 9, 5), 2, 9, 0.8), ((4, 12, 6), 1, 5, 0.25), ((4, 12, 6), 2, 1, 0.9), ((2, 3, 4), 0, 2, 1.0)]


@pytest.mark.parametrize("shape,axis,n,g", GHOST)
def test_ghosting_table_is_the_spectrum_edit(shape, axis, n, g):
    x = _vol(shape, 1)
    N = shape[axis]
    row = data.ghosting_tables([n], [g], [N])
    assert row.shape == (1, ops.AXIS_CONV_MAX_N) and row.dtype == np.float32 and not row[0, N:].any()
    # the float64 row, rebuilt here from the definition, against the literal algorithm to 1e-12; the table is its float32 rounding
    S = [j for j in range(0, N, n) if j != N // 2]
    m = np.arange(N)
    c = (m == 0) - (g / N) * sum(np.cos(2 * np.pi * (j - N // 2) * m / N) for j in S) if S else (m == 0).astype(np.float64)
    ref = kspace_ref.ghosting_fft(x, n, axis, g)
    err = np.abs(kspace_ref.circular_conv(x, c, axis) - ref).max() / np.abs(ref).max()
    print(f"ghosting {shape} axis {axis} n {n} g {g}: |S| {len(S)} relative error {err:.2e}")
    assert err <= 1e-12
    assert np.abs(row[0, :N] - c).max() <= 2.0 ** -24 * max(1.0, np.abs(c).max())
    # c[0] = 1 - g |S| / N (every cosine is 1 at m = 0); the row sums to 1, the mask's value at the restored centre plane (the DC term)
    assert abs(float(row[0, 0]) - (1 - g * len(S) / N)) <= 2.0 ** -24
    assert abs(row[0, :N].astype(np.float64).sum() - 1.0) <= N * 2.0 ** -24


def test_ghosting_identity_cases_give_the_unit_impulse():
    impulse = np.zeros(ops.AXIS_CONV_MAX_N, dtype=np.float32)
    impulse[0] = 1
    for n, g, N in [(0, 0.7, 12), (5, 0.0, 12), (0, 0.0, 7), (20, 0.5, 9)]:        # the last: n > N leaves only j = 0 ...
        row = data.ghosting_tables([n], [g], [N])[0]
        if (n, N) == (20, 9):
            assert abs(float(row[0]) - (1 - g / N)) < 1e-6                           # ... which is not the identity
        else:
            assert np.array_equal(row, impulse), (n, g, N)
    assert np.array_equal(kspace_ref.ghosting_fft(_vol((3, 4, 5), 2), 0, 1, 0.5), _vol((3, 4, 5), 2))
    for bad in (1, 257):
        with pytest.raises(ValueError, match="2..256 are built"):
            data.ghosting_tables([2], [0.5], [bad])


# ---- spikes: the closed cosine form is the spectrum edit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 6, 10), (7, 9, 5)])
@pytest.mark.parametrize("positions", [[(0.0, 0.0, 0.0)], [(1 - 2.0 ** -40, 1 - 2.0 ** -40, 1 - 2.0 ** -40)],
                                       [(0.3, 0.72, 0.05), (0.0, 0.999999, 0.5), (0.51, 0.49, 0.77), (0.9, 0.1, 0.0)]])
def test_spike_closed_form_is_the_spectrum_edit(shape, positions):
    x = _vol(shape, 3) - (2000 if len(positions) == 4 else 0)                        # one volume with a negative mean
    ref = kspace_ref.spike_fft(x, positions, 1.7)
    got, total = kspace_ref.spike_cosine(x, positions, 1.7)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"spike {shape} S {len(positions)}: indices {kspace_ref.spike_indices(positions, shape)} relative error {err:.2e}")
    assert err <= 1e-12 and np.abs(total).max() > 0.5
    # the tables: cos / sin of the per-axis phases; their angle-addition product is the cosine of the sum
    tab = data.spike_tables(positions, shape).astype(np.float64)
    assert tab.shape == (ops.SPIKE_MAX, 2, sum(shape)) and not tab[len(positions):].any()
    D, H, W = shape
    rebuilt = np.zeros(shape)
    for s in range(len(positions)):
        (c0, s0), (c1, s1), (c2, s2) = [(tab[s, 0, o:o + n].reshape(sh), tab[s, 1, o:o + n].reshape(sh))
                                        for o, n, sh in ((0, D, (-1, 1, 1)), (D, H, (1, -1, 1)), (D + H, W, (1, 1, -1)))]
        rebuilt += c0 * (c1 * c2 - s1 * s2) - s0 * (s1 * c2 + c1 * s2)
    assert np.abs(rebuilt - total).max() <= len(positions) * 8 * 2.0 ** -24           # six float32 table entries per spike, each within 2^-25 ... generous


def test_spike_tables_rejections():
    for S in (0, 5):
        with pytest.raises(ValueError, match="1..4 are built"):
            data.spike_tables(np.full((S, 3), 0.5), (4, 4, 4))
    with pytest.raises(ValueError, match=r"in \[0, 1\)"):
        data.spike_tables([(0.5, 1.0, 0.5)], (4, 4, 4))


# ---- anisotropy: the two-tap tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 5, 12, 33, 160])
@pytest.mark.parametrize("f", [1.0, 1.5, 2.0, 3.7, 5.0, 400.0])
def test_anisotropy_tables_vs_direct_evaluation(N, f):
    src, w = data.anisotropy_tables(f, N)
    s0, s1, wd = kspace_ref.anisotropy_coordinates(f, N)
    assert src.dtype == np.int32 and w.dtype == np.float32 and src.shape == (N, 2) and w.shape == (N,)
    assert np.array_equal(src[:, 0], s0) and np.array_equal(src[:, 1], s1) and np.array_equal(w, wd.astype(np.float32))
    assert src.min() >= 0 and src.max() <= N - 1 and (w >= 0).all() and (w <= 1).all()
    n_low = max(1, math.ceil(N / f))
    assert len(set(src.ravel().tolist())) <= n_low                                  # only the low-resolution samples are ever read
    if f == 1.0:
        assert np.array_equal(src[:, 0], np.arange(N)) and not w.any()
    if f > N:                                                                        # one low sample: a constant line
        assert n_low == 1 and len(set(src.ravel().tolist())) == 1 and not w.any()
    # clamps at both ends: the first and last outputs sit outside the low grid's centres and copy its first and last sample
    assert w[0] == 0 or f == 1.0 or (0.5 / f - 0.5) >= 0
    assert src[0, 0] == s0[0] == min(max(math.floor((0.5 * f - 0.5) + 0.5), 0), N - 1)
    assert w[N - 1] == 0 or ((N - 0.5) / f - 0.5) < n_low - 1


def test_anisotropy_tables_padding_and_errors():
    src, w = data.anisotropy_tables(2.0, 5, n_max=9)
    assert src.shape == (9, 2) and w.shape == (9,) and not src[5:].any() and not w[5:].any()
    assert np.array_equal(src[:5], data.anisotropy_tables(2.0, 5)[0])
    with pytest.raises(ValueError):
        data.anisotropy_tables(0.9, 5)


# ---- sampling ----------------------------------------------------------------------------------------------------------------------------------
def _freq_ok(count, n, p):
    return abs(count - n * p) <= 4.5 * math.sqrt(n * p * (1 - p))


def test_ghosting_sampling():
    t = data.RandomGhosting(num_ghosts=(4, 10), axes=(0, 1, 2), intensity=(0.5, 1))
    rng = np.random.default_rng(0)
    draws = [t.sample(rng) for _ in range(3000)]
    assert all(d[0] == "RandomGhosting" for d in draws)
    n = np.array([d[1]["num_ghosts"] for d in draws])
    ax = np.array([d[1]["axis"] for d in draws])
    g = np.array([d[1]["intensity"] for d in draws])
    assert n.min() == 4 and n.max() == 10 and all(isinstance(d[1]["num_ghosts"], int) for d in draws)      # inclusive at both ends
    assert all(_freq_ok((n == v).sum(), 3000, 1 / 7) for v in range(4, 11))
    assert all(_freq_ok((ax == a).sum(), 3000, 1 / 3) for a in (0, 1, 2))
    assert g.min() >= 0.5 and g.max() <= 1 and 0.7 < g.mean() < 0.8
    # draw order: p, n, axis, g
    rng, twin = np.random.default_rng(5), np.random.default_rng(5)
    d = t.sample(rng)[1]
    twin.random()
    assert d["num_ghosts"] == int(twin.integers(4, 11)) and d["axis"] == (0, 1, 2)[int(twin.integers(3))] and d["intensity"] == float(twin.uniform(0.5, 1))
    one = data.RandomGhosting(num_ghosts=3, axes=1, intensity=0.4)
    assert one.num_ghosts == (0, 3) and one.axes == (1,) and one.intensity == (0.0, 0.4)
    drawn = {one.sample(rng)[1]["num_ghosts"] for _ in range(200)}
    assert drawn == {0, 1, 2, 3}
    for kw in (dict(num_ghosts=-1), dict(num_ghosts=(5, 2)), dict(num_ghosts=2.5), dict(axes=(3,)), dict(axes=("LR",)), dict(axes=()),
               dict(intensity=-0.1), dict(intensity=(0.9, 0.1)), dict(restore=-0.1), dict(restore=1.5)):
        with pytest.raises(ValueError):
            data.RandomGhosting(**kw)


def test_spike_gamma_anisotropy_sampling():
    rng = np.random.default_rng(1)
    sp = data.RandomSpike(num_spikes=3, intensity=(1, 3))
    d = [sp.sample(rng)[1] for _ in range(500)]
    pos = np.stack([v["positions"] for v in d])
    assert pos.shape == (500, 3, 3) and pos.min() >= 0 and pos.max() < 1 and all(1 <= v["intensity"] <= 3 for v in d)
    rng, twin = np.random.default_rng(6), np.random.default_rng(6)
    got = sp.sample(rng)[1]
    twin.random()
    assert np.array_equal(got["positions"], twin.random((3, 3))) and got["intensity"] == float(twin.uniform(1, 3))      # p, positions, then g
    assert data.RandomSpike(intensity=2).intensity == (-2.0, 2.0)
    with pytest.raises(NotImplementedError, match="1..4 are built"):
        data.RandomSpike(num_spikes=5)
    with pytest.raises(NotImplementedError):
        data.RandomSpike(num_spikes=(1, 2))
    with pytest.raises(ValueError):
        data.RandomSpike(num_spikes=0)

    ga = data.RandomGamma()
    d = [ga.sample(rng)[1] for _ in range(500)]
    assert all(-0.3 <= v["log_gamma"] <= 0.3 and v["gamma"] == math.exp(v["log_gamma"]) for v in d)
    assert data.RandomGamma(log_gamma=0.2).log_gamma == (-0.2, 0.2)
    with pytest.raises(ValueError):
        data.RandomGamma(log_gamma=(0.3, -0.3))

    an = data.RandomAnisotropy()
    rng = np.random.default_rng(2)
    d = [an.sample(rng)[1] for _ in range(3000)]
    ax = np.array([v["axis"] for v in d])
    assert all(_freq_ok((ax == a).sum(), 3000, 1 / 3) for a in (0, 1, 2)) and all(1.5 <= v["downsampling"] <= 5 for v in d)
    rng, twin = np.random.default_rng(7), np.random.default_rng(7)
    got = an.sample(rng)[1]
    twin.random()
    assert got["axis"] == int(twin.integers(3)) and got["downsampling"] == float(twin.uniform(1.5, 5))                  # p, axis, then f
    assert data.RandomAnisotropy(axes=2, downsampling=3).downsampling == (1.0, 3.0)
    for kw in (dict(downsampling=0.5), dict(downsampling=(0.9, 2)), dict(downsampling=(3, 2)), dict(axes=(0, 4))):
        with pytest.raises(ValueError):
            data.RandomAnisotropy(**kw)
    with pytest.raises(NotImplementedError):
        data.RandomAnisotropy(image_interpolation="bspline")


@pytest.mark.parametrize("cls", ["RandomGhosting", "RandomSpike", "RandomGamma", "RandomAnisotropy"])
def test_p_gates_the_draw(cls):
    t = getattr(data, cls)(p=0.25)
    rng = np.random.default_rng(3)
    hits = sum(t.sample(rng) is not None for _ in range(3000))
    assert _freq_ok(hits, 3000, 0.25)
    rng, twin = np.random.default_rng(4), np.random.default_rng(4)
    assert getattr(data, cls)(p=0.0).sample(rng) is None
    twin.random()
    assert rng.random() == twin.random()                                            # a transform that is not applied consumed one uniform


# ---- the compose ---------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    return type(a) is type(b) and a == b


@pytest.mark.parametrize("motion", [False, True])
def test_stream_of_a_compose_without_the_new_transforms_is_unchanged(motion):
    """train_transforms(intensity=True[, motion=True]) draws what the same list built from the earlier classes alone draws."""
    group = {data.RandomNoise(): 1, data.RandomBiasField(): 1, data.RandomBlur(std=(0, 1.5)): 1}
    if motion:
        group = {data.RandomNoise(): 0.25, data.RandomBiasField(): 0.25, data.RandomBlur(std=(0, 1.5)): 0.25, data.RandomMotion(): 0.25}
    for seed in (0, 7, 11):
        new = data.train_transforms(seed, intensity=True, motion=motion, artifacts=False)
        old = data.DeviceCompose([data.RandomAffine(degrees=15, p=0.5), data.RandomFlip(axes=(0,), flip_probability=0.5), data.OneOf(group, p=0.75),
                                  data.RescaleIntensity((0, 1))], seed)
        assert [type(t) for t in new.intensity[0].transforms] == [type(t) for t in old.intensity[0].transforms]
        assert np.array_equal(new.intensity[0].weights, old.intensity[0].weights)
        for _ in range(3):
            m1, f1 = new.sample(16, (8, 12, 20))
            m2, f2 = old.sample(16, (8, 12, 20))
            assert np.array_equal(m1, m2) and np.array_equal(f1, f2)
            assert _same(new.last_params, old.last_params) and _same(new.last_intensity, old.last_intensity)
        assert new.rng.random() == old.rng.random()


def test_artifacts_join_the_intensity_group_with_equal_weights():
    for motion, n in ((False, 7), (True, 8)):
        tf = data.train_transforms(0, intensity=True, motion=motion, artifacts=True)
        one = tf.intensity[0]
        assert [type(t).__name__ for t in one.transforms][-4:] == ["RandomGhosting", "RandomSpike", "RandomGamma", "RandomAnisotropy"]
        assert len(one.transforms) == n and np.allclose(one.weights, 1 / n) and one.p == 0.75
        tf.sample(64, (8, 12, 20))
        names = {d[0] for d in tf.last_intensity if d}
        assert names >= {"RandomGhosting", "RandomSpike", "RandomGamma", "RandomAnisotropy"}
    with pytest.raises(ValueError, match="needs intensity=True"):
        data.train_transforms(0, artifacts=True)
    pre = data.DataPreprocessor({"data": {"intensity_augment": True, "artifact_augment": True}}, seed=1)
    assert len(pre.train_transforms.intensity[0].transforms) == 7 and not pre.val_transforms.intensity
    assert len(data.DataPreprocessor({"data": {"intensity_augment": True}}, seed=1).train_transforms.intensity[0].transforms) == 3


def test_built_list_and_refusals():
    assert data._BUILT.startswith("RandomAffine (at most one), RandomFlip, RandomNoise, RandomBiasField, RandomBlur, RandomMotion, OneOf of the last ")
    for name in ("RandomGhosting", "RandomSpike", "RandomGamma", "RandomAnisotropy"):
        assert data._BUILT.index(name) > data._BUILT.index("ZNormalization")
        assert getattr(data, name) in data.INTENSITY_TRANSFORMS
        with pytest.raises(NotImplementedError, match="spatial"):                   # not in a spatial OneOf
            data.OneOf([data.RandomAffine(), getattr(data, name)()])
        with pytest.raises(NotImplementedError, match="spatial"):
            data.OneOf([getattr(data, name)(), data.RandomElasticDeformation()])
    both = data.DeviceCompose([data.RandomGhosting(), data.OneOf([data.RandomGamma(), data.RandomSpike()]), data.RandomAnisotropy(),
                               data.RescaleIntensity((0, 1))], seed=0)             # singly and inside an intensity OneOf
    both.sample(4, (8, 12, 20))
    assert all(len(d) == 3 and d[0][0] == "RandomGhosting" and d[2][0] == "RandomAnisotropy" for d in both.last_intensity)
    assert (ops.AXIS_CONV_MAX_N, ops.SPIKE_MAX) == (256, 4)
