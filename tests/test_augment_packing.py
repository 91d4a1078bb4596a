"""CPU: the batch assembly between the per-sample draws and the device launches (gaviko_amd/data.py).  The `pack_*` functions row by row
against the single-sample `*_tables` functions and the defaults that make a kernel copy a sample; the group table against
INTENSITY_TRANSFORMS; the one shape check of the one-channel volume passes of `ops`; and, with every `ops` entry point replaced by a recorder, which launches `apply_intensity` and the normalisers make
and in which order."""
import numpy as np
import pytest
import torch

from gaviko_amd import data, ops

B, SHAPE = 4, (5, 6, 8)                                                    # three different extents
RNG = np.random.default_rng(77)

# hand-written draws, the entries of DeviceCompose.last_intensity
NOISE = ("RandomNoise", dict(mean=0.25, std=0.125, seed=2 ** 63 + 0x1234_5678_9ABC))
BIAS1 = ("RandomBiasField", dict(coefficients=RNG.uniform(-0.5, 0.5, 4), order=1))
BIAS3 = ("RandomBiasField", dict(coefficients=RNG.uniform(-0.5, 0.5, 20), order=3))
BLUR_A = ("RandomBlur", dict(std=np.array([1.5, 0.3, 1.2])))
BLUR_B = ("RandomBlur", dict(std=np.array([0.0, 2.5, 0.6])))
MOTION1 = ("RandomMotion", dict(degrees=RNG.uniform(-10, 10, (1, 3)), translation=RNG.uniform(-3, 3, (1, 3)), times=np.array([0.55])))
MOTION3 = ("RandomMotion", dict(degrees=RNG.uniform(-10, 10, (3, 3)), translation=RNG.uniform(-3, 3, (3, 3)), times=np.array([0.2, 0.45, 0.8])))
GHOST_0 = ("RandomGhosting", dict(num_ghosts=2, axis=0, intensity=0.7))
GHOST_1 = ("RandomGhosting", dict(num_ghosts=3, axis=1, intensity=0.5))
GAMMA = ("RandomGamma", dict(log_gamma=0.25, gamma=float(np.exp(0.25))))
SPIKE = ("RandomSpike", dict(positions=RNG.random((2, 3)), intensity=1.75))
ANISO_2 = ("RandomAnisotropy", dict(axis=2, downsampling=2.5))
ANISO_0 = ("RandomAnisotropy", dict(axis=0, downsampling=1.7))


def _is(a, dtype, shape):
    return isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == tuple(shape)


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- packers against the single-sample functions ------------------------------------------------------------------------------------------
def test_pack_pointwise_rows_orders_and_seeds():
    draws = [BIAS1, None, BLUR_A, BIAS3]                                    # orders 1 and 3 in one batch, a foreign class, nothing
    kind, noise, seeds, coeff, order = data.pack_pointwise(draws)
    assert _is(kind, np.int32, (B,)) and _is(noise, np.float32, (B, 2)) and _is(seeds, np.uint64, (B,)) and _is(coeff, np.float32, (B, ops.BIAS_COEFFS))
    assert order == 3 and kind.tolist() == [ops.INTENSITY_BIAS, ops.INTENSITY_COPY, ops.INTENSITY_COPY, ops.INTENSITY_BIAS]
    for b in (0, 3):
        p = draws[b][1]
        assert _bits(coeff[b], data.bias_coefficients(p["coefficients"], p["order"], 3).astype(np.float32))
    assert np.count_nonzero(coeff[0]) == 4                                  # the order-1 field laid out among the order-3 terms
    assert not coeff[1:3].any() and not noise.any() and not seeds.any()

    draws = [NOISE, None, GAMMA, BIAS1]                                     # the launch's order is the batch maximum, not a constant
    kind, noise, seeds, coeff, order = data.pack_pointwise(draws)
    assert order == 1 and kind.tolist() == [ops.INTENSITY_NOISE, ops.INTENSITY_COPY, ops.INTENSITY_COPY, ops.INTENSITY_BIAS]
    assert _bits(noise[0], np.array([0.125, 0.25], dtype=np.float32)) and not noise[1:].any()          # (std, mean)
    assert _bits(coeff[3, :4], data.bias_coefficients(BIAS1[1]["coefficients"], 1, 1).astype(np.float32)) and not coeff[3, 4:].any() and not coeff[:3].any()
    assert seeds.tolist() == [NOISE[1]["seed"], 0, 0, 0]
    as_i64 = seeds.view(np.int64)                                           # what the launcher uploads: the same 64 bits
    assert as_i64.dtype == np.int64 and as_i64[0] < 0 and int(torch.from_numpy(as_i64)[0]) % 2 ** 64 == NOISE[1]["seed"]
    assert as_i64.view(np.uint64).tolist() == seeds.tolist()

    assert data.pack_pointwise([None, NOISE, None, None])[4] == 0           # no bias field drawn


def test_pack_blur_rows():
    draws = [BLUR_A, None, NOISE, BLUR_B]
    weights, radius = data.pack_blur(draws)
    assert _is(weights, np.float32, (B, 3, ops.BLUR_TAPS)) and _is(radius, np.int32, (B, 3))
    for b in (0, 3):
        w, r = data.blur_tables([draws[b][1]["std"]])
        assert _bits(weights[b], w[0]) and _bits(radius[b], r[0])
    assert radius[3, 0] == 0 and radius[3, 1] == 10                         # a skipped axis beside a blurred one
    for b in (1, 2):                                                        # sigma 0: radius 0 with the single weight 1
        assert not radius[b].any() and (weights[b, :, 0] == 1).all() and not weights[b, :, 1:].any()


def test_pack_motion_rows_and_batch_maximum():
    draws = [MOTION1, None, GHOST_0, MOTION3]
    mats, ctab, live, K = data.pack_motion(draws, SHAPE)
    assert K == 3 and _is(mats, np.float32, (B, 3, 3, 4)) and _is(ctab, np.float32, (B, 4, SHAPE[2])) and _is(live, np.int32, (B,))
    assert live.tolist() == [1, 0, 0, 1]
    eye = np.eye(3, 4, dtype=np.float32)
    for b in (0, 3):
        p = draws[b][1]
        k = len(p["times"])
        assert _bits(ctab[b, :k + 1], data.motion_tables(p["times"], SHAPE[2])[0][0]) and not ctab[b, k + 1:].any()
        for j in range(k):
            assert _bits(mats[b, j], data.affine_matrix((1, 1, 1), p["degrees"][j], p["translation"][j], SHAPE).astype(np.float32))
            assert not _bits(mats[b, j], eye)
        assert all(_bits(m, eye) for m in mats[b, k:])                      # the short sample's other movements: identity
    for b in (1, 2):
        assert not ctab[b].any() and all(_bits(m, eye) for m in mats[b])
    assert data.pack_motion([None, MOTION1, None, None], SHAPE)[3] == 1


def test_pack_ghosting_rows():
    draws = [GHOST_0, None, SPIKE, GHOST_1]                                 # two live samples on different axes
    ctab, axis, live = data.pack_ghosting(draws, SHAPE)
    assert _is(ctab, np.float32, (B, ops.AXIS_CONV_MAX_N)) and _is(axis, np.int32, (B,)) and _is(live, np.int32, (B,))
    assert axis.tolist() == [0, 2, 2, 1] and live.tolist() == [1, 0, 0, 1]
    for b in (0, 3):
        p = draws[b][1]
        assert _bits(ctab[b], data.ghosting_tables([p["num_ghosts"]], [p["intensity"]], [SHAPE[p["axis"]]])[0]) and ctab[b, 1:].any()
    for b in (1, 2):                                                        # not live: the unit impulse of an axis of shape[2] voxels
        assert _bits(ctab[b], data.ghosting_tables([0], [0.0], [SHAPE[2]])[0]) and ctab[b, 0] == 1 and not ctab[b, 1:].any()


def test_pack_gamma_spike_rows():
    draws = [GAMMA, SPIKE, None, BLUR_A]
    kind, gamma, amp, nspikes, tab = data.pack_gamma_spike(draws, SHAPE)
    assert _is(kind, np.int32, (B,)) and _is(gamma, np.float32, (B,)) and _is(amp, np.float32, (B,)) and _is(nspikes, np.int32, (B,))
    assert _is(tab, np.float32, (B, ops.SPIKE_MAX, 2, sum(SHAPE)))
    assert kind.tolist() == [ops.KSPACE_GAMMA, ops.KSPACE_SPIKE, ops.KSPACE_COPY, ops.KSPACE_COPY]
    assert _bits(gamma, np.array([GAMMA[1]["gamma"], 1, 1, 1], dtype=np.float32))
    assert _bits(amp, np.array([0, 1.75, 0, 0], dtype=np.float32)) and nspikes.tolist() == [0, 2, 0, 0]
    assert _bits(tab[1], data.spike_tables(SPIKE[1]["positions"], SHAPE)) and tab[1, :2].any() and not tab[1, 2:].any()
    assert not tab[0].any() and not tab[2:].any()


def test_pack_anisotropy_rows():
    draws = [ANISO_2, None, NOISE, ANISO_0]                                 # two live samples on different axes
    src, w, axis, live = data.pack_anisotropy(draws, SHAPE)
    n_max = max(SHAPE)
    assert _is(src, np.int32, (B, n_max, 2)) and _is(w, np.float32, (B, n_max)) and _is(axis, np.int32, (B,)) and _is(live, np.int32, (B,))
    assert axis.tolist() == [2, 0, 0, 0] and live.tolist() == [1, 0, 0, 1]
    for b in (0, 3):
        p = draws[b][1]
        s, ww = data.anisotropy_tables(p["downsampling"], SHAPE[p["axis"]], n_max)
        assert _bits(src[b], s) and _bits(w[b], ww) and w[b].any()
    assert not src[3, SHAPE[0]:].any() and not w[3, SHAPE[0]:].any()        # the short axis fills its own extent only
    assert not src[1:3].any() and not w[1:3].any()


def test_pack_elastic_rows():
    n = (5, 4, 6)
    fields = [None, RNG.uniform(-2, 2, n + (3,)), None, RNG.uniform(-2, 2, n + (3,))]
    ctrl, live = data.pack_elastic(fields, n)
    assert _is(ctrl, np.float32, (B,) + n + (3,)) and _is(live, np.int32, (B,)) and live.tolist() == [0, 1, 0, 1]
    for b in (1, 3):
        assert _bits(ctrl[b], fields[b].astype(np.float32))
    assert not ctrl[0].any() and not ctrl[2].any()


# ---- the group table ---------------------------------------------------------------------------------------------------------------------
def test_every_intensity_transform_is_served_by_exactly_one_group():
    served = [name for names, _ in data.INTENSITY_GROUPS for name in names]
    classes = [c.__name__ for c in data.INTENSITY_TRANSFORMS]
    assert sorted(served) == sorted(classes)                                # each class once, and nothing else
    assert all(callable(launch) for _, launch in data.INTENSITY_GROUPS)
    assert [names for names, _ in data.INTENSITY_GROUPS] == [("RandomNoise", "RandomBiasField"), ("RandomBlur",), ("RandomMotion",), ("RandomGhosting",),
                                                             ("RandomGamma", "RandomSpike"), ("RandomAnisotropy",)]
    for c in data.INTENSITY_TRANSFORMS:                                     # the name a draw carries is the name the table is keyed on
        assert c(p=1.0).sample(np.random.default_rng(0))[0] == c.__name__


# ---- one check for one-channel volumes ------------------------------------------------------------------------------------------------------
def test_volume_passes_reject_shapes_that_are_not_one_channel(monkeypatch):
    from gaviko_amd import lib
    monkeypatch.setattr(ops, "_chk", lambda *a, **k: None)                  # the device / dtype checks need a GPU; the shape check does not
    flat, two = torch.zeros(2, 6, 8), torch.zeros(2, 2, 5, 6, 8)            # fewer than four dimensions; two channels
    for x in (flat, two):
        for what, call in (("gaussian_blur3d", lambda: ops.gaussian_blur3d(x, x, x, None, None, 0)),
                           ("intensity_pointwise", lambda: ops.intensity_pointwise(x, x, None, None, None, None)),
                           ("motion_artifact", lambda: ops.motion_artifact(x, x, None, None, None, None, 1)),
                           ("elastic_deform", lambda: ops.elastic_deform(x, x, None, None, None)),
                           ("axis_gather2", lambda: ops.axis_gather2(x, x, None, None, None, None))):
            with pytest.raises(lib.GavikoHipError, match=rf"{what} in: one channel, \[B, D, H, W\] or \[B, 1, D, H, W\]"):
                call()


# ---- launch sequence ---------------------------------------------------------------------------------------------------------------------
LAUNCHES = ("volume_minmax", "volume_stats", "volume_order_stats", "normalize_intensity", "rescale_intensity", "intensity_pointwise", "gaussian_blur3d",
            "motion_artifact", "axis_circular_conv", "gamma_spike", "axis_gather2")


@pytest.fixture
def calls(monkeypatch):
    """Every `ops` function the stage and the normalisers reach, replaced: [(name, args, kwargs)] in call order."""
    log = []
    returns = dict(minmax_partials=lambda n, dev: torch.zeros(2 * n),
                   volume_stats=lambda x, *a, **k: (torch.ones((x.shape[0], ops.NORMALIZE_STATS), dtype=torch.float64), torch.zeros(x.shape[0], dtype=torch.int64)),
                   volume_order_stats=lambda x, s, q, *a, **k: (torch.zeros((x.shape[0], len(q), 2)), torch.zeros((x.shape[0], len(q)))),
                   normalize_intensity=lambda x, *a, **k: torch.zeros(x.shape[0], dtype=torch.int32))
    for name in ("minmax_partials",) + LAUNCHES:
        def recorder(*a, _name=name, **k):
            log.append((_name, a, k))
            return returns[_name](*a, **k) if _name in returns else None
        monkeypatch.setattr(ops, name, recorder)
    return log


def _launched(calls):
    return [c[0] for c in calls if c[0] != "minmax_partials"]              # the partials buffer is an allocation, not a launch


def _x():
    return torch.arange(B * int(np.prod(SHAPE)), dtype=torch.float32).reshape((B, 1) + SHAPE)


def test_nothing_drawn_launches_nothing(calls):
    x = _x()
    assert data.apply_intensity(x, [None] * B) is x and calls == []


def test_gamma_alone_takes_no_statistics(calls):
    x = _x()
    y = data.apply_intensity(x, [GAMMA, None, GAMMA, None])
    assert _launched(calls) == ["gamma_spike"] and y is not x and y is calls[0][1][1] and calls[0][1][0] is x
    stats = calls[0][1][-1]                                                 # a zero table stands in
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (B, ops.NORMALIZE_STATS) and not stats.any()


def test_a_spike_takes_the_statistics_first(calls):
    x = _x()
    data.apply_intensity(x, [GAMMA, None, SPIKE, None])
    assert _launched(calls) == ["volume_stats", "gamma_spike"]
    (_, sa, sk), (_, ga, _) = calls
    assert sa[0] is x and sa[1] is None and sk == dict(want_std=False)
    assert ga[0] is x and ga[-1].all() and tuple(ga[-1].shape) == (B, ops.NORMALIZE_STATS)          # the recorder's table of ones reached the launch


def test_motion_takes_the_minimum_of_its_input_first(calls):
    x = _x()
    data.apply_intensity(x, [None, MOTION3, None, MOTION1])
    assert _launched(calls) == ["volume_minmax", "motion_artifact"]
    part = calls[1][1][1]
    assert [c[0] for c in calls][0] == "minmax_partials" and calls[1][1][0] is x
    assert calls[2][1][0] is x and calls[2][1][5] is part and calls[2][1][6] == 3


def test_groups_launch_in_table_order_once_each(calls):
    x = _x()
    y = data.apply_intensity(x, [ANISO_2, BLUR_A, NOISE, None])
    assert _launched(calls) == ["intensity_pointwise", "gaussian_blur3d", "axis_gather2"]
    assert calls[0][1][0] is x and calls[1][1][0] is calls[0][1][1] and calls[2][1][0] is calls[1][1][1] and y is calls[2][1][1]   # a chain
    seeds = calls[0][1][4]
    assert seeds.dtype == torch.int64 and int(seeds[2]) % 2 ** 64 == NOISE[1]["seed"]


def test_normalisers_keep_their_launches(calls):
    x, part = _x(), torch.zeros(2 * B)
    y, status = data.RescaleIntensity((0, 1)).apply(x, part)
    assert [c[0] for c in calls] == ["volume_minmax", "rescale_intensity"] and status is None
    assert calls[0][1] == (x, part) and calls[1][1][:3] == (x, part, y) and calls[1][1][3:] == (0.0, 1.0)
    del calls[:]
    y, status = data.RescaleIntensity((0, 1), percentiles=(0.5, 99.5)).apply(x, part)
    assert [c[0] for c in calls] == ["volume_stats", "volume_order_stats", "normalize_intensity"]
    assert status is not None and tuple(status.shape) == (B,) and tuple(y.shape) == tuple(x.shape) and y is not x
    assert calls[0][2] == dict(want_std=False) and calls[1][1][2] == (0.5, 99.5) and calls[2][1][3] == ops.NORMALIZE_RESCALE
    del calls[:]
    y, status = data.ZNormalization(masking_method=data.ZNormalization.mean).apply(x, part)
    assert [c[0] for c in calls] == ["volume_stats", "normalize_intensity"]
    assert status is not None and calls[0][1][1] == "mean" and calls[0][2] == dict(want_std=True) and calls[1][1][3] == ops.NORMALIZE_ZNORM
