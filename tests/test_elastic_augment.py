"""CPU: host side of RandomElasticDeformation (gaviko_amd/data.py): torchio's parameter sampling, locked borders, errors and folding warning,
the draw order inside DeviceCompose (and that a compose without it consumes the stream it always did), the spatial OneOf, the switches
that put it into the training pipeline, and the float64 restatement (tests/elastic_ref.py) against closed forms and scipy.  The kernel
itself: tests/test_elastic_augment_gpu.py."""
import warnings

import numpy as np
import pytest
from scipy import ndimage

import elastic_ref
from gaviko_amd import data, ops


# ------------------------------------------------------------------------------------------------ sampling
def test_parameter_bounds_per_axis_and_p():
    rng = np.random.default_rng(11)
    el = data.RandomElasticDeformation(num_control_points=(5, 7, 9), max_displacement=(0, 3, 12), locked_borders=0)
    seen = np.zeros(3)
    for _ in range(50):
        f = el.sample(rng)
        assert f.shape == (5, 7, 9, 3) and f.dtype == np.float64
        assert not f[..., 0].any() and (np.abs(f[..., 1]) <= 3).all() and (np.abs(f[..., 2]) <= 12).all()
        seen = np.maximum(seen, np.abs(f).max(axis=(0, 1, 2)))
    assert seen[1] > 2.9 and seen[2] > 11.6                                            # the ranges are filled, both signs
    assert (f[..., 1] < 0).any() and (f[..., 1] > 0).any()
    default = data.RandomElasticDeformation()                                           # tio.RandomElasticDeformation()
    assert default.num_control_points == (7, 7, 7) and default.max_displacement == (7.5, 7.5, 7.5)
    assert default.locked_borders == 2 and default.p == 1.0
    half = data.RandomElasticDeformation(p=0.5)
    n = sum(half.sample(rng) is not None for _ in range(400))
    assert 150 <= n <= 250, n                                                           # 200 +- 5 sigma (sigma = 10)


def test_draw_order_replayed_on_a_second_generator():
    """One uniform for p, then n0 n1 n2 3 uniforms in grid order mapped to U(-max_a, max_a), and nothing more."""
    el = data.RandomElasticDeformation(num_control_points=(4, 5, 6), max_displacement=(1, 2, 4), locked_borders=0, p=0.6)
    rng, r = np.random.default_rng(31), np.random.default_rng(31)
    seen = 0
    for _ in range(40):
        got = el.sample(rng)
        if r.random() >= 0.6:
            assert got is None
            continue
        want = (r.random((4, 5, 6, 3)) - 0.5) * 2 * np.array([1.0, 2.0, 4.0])
        assert np.array_equal(got, want)
        seen += 1
    assert seen > 10 and rng.random() == r.random()


@pytest.mark.parametrize("locked", [0, 1, 2])
def test_locked_borders(locked):
    el = data.RandomElasticDeformation(num_control_points=(6, 7, 8), max_displacement=5, locked_borders=locked)
    f = el.sample(np.random.default_rng(5))
    mag = np.abs(f).sum(axis=-1)                                                        # (a zero draw has probability 0)
    for a in range(3):
        layers = np.moveaxis(mag, a, 0)
        n = layers.shape[0]
        for i in range(n):
            depth = min(i, n - 1 - i)                                                   # 0 = the outermost layer
            if depth < locked:
                assert not layers[i].any(), (a, i)
    inner = mag[locked:6 - locked, locked:7 - locked, locked:8 - locked]
    assert inner.size and (inner > 0).all()                                             # and nothing else was zeroed


def test_errors_follow_torchio():
    with pytest.raises(ValueError, match="at least 4 control points"):
        data.RandomElasticDeformation(num_control_points=3)
    with pytest.raises(ValueError, match="at least 4 control points"):
        data.RandomElasticDeformation(num_control_points=(7, 3, 7))
    with pytest.raises(ValueError, match="identity"):
        data.RandomElasticDeformation(num_control_points=(7, 7, 4))                     # locked_borders = 2 by default
    data.RandomElasticDeformation(num_control_points=4, locked_borders=1)
    with pytest.raises(ValueError):
        data.RandomElasticDeformation(locked_borders=3)
    with pytest.raises(ValueError):
        data.RandomElasticDeformation(num_control_points=(7, 7))
    with pytest.raises(NotImplementedError, match="linear"):
        data.RandomElasticDeformation(image_interpolation="bspline")
    assert ops.ELASTIC_MAX_CONTROL_POINTS == 16
    data.RandomElasticDeformation(num_control_points=16)
    with pytest.raises(NotImplementedError, match=r"4\.\.16"):
        data.RandomElasticDeformation(num_control_points=(7, 17, 7))


def test_folding_warning_on_the_first_call_only():
    el = data.RandomElasticDeformation(num_control_points=7, max_displacement=7.5, p=1.0)
    tf = data.DeviceCompose([el, data.RescaleIntensity()], seed=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                                  # nothing is raised before the shape is known
        data.DeviceCompose([data.RandomElasticDeformation()], seed=0)
    with pytest.warns(RuntimeWarning, match="fold"):                                    # h = 24 / 4 = 6: 7.5 >= 3
        tf.sample(2, (24, 32, 40))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tf.sample(2, (24, 32, 40))                                                      # once
        ok = data.DeviceCompose([data.RandomElasticDeformation()], seed=0)
        ok.sample(1, (120, 160, 160))                                                   # h = 30, 40, 40: 7.5 is below half of each
        edge = data.DeviceCompose([data.RandomElasticDeformation(max_displacement=(14.9, 0, 0))], seed=0)
        edge.sample(1, (120, 160, 160))
    with pytest.warns(RuntimeWarning):
        data.DeviceCompose([data.RandomElasticDeformation(max_displacement=(15, 0, 0))], seed=0).sample(1, (120, 160, 160))   # >= h / 2


# ------------------------------------------------------------------------------------------------ inside DeviceCompose
def _members():
    return (data.RandomAffine(degrees=15, p=0.5), data.RandomFlip(axes=(0, 2), flip_probability=0.5),
            data.OneOf({data.RandomNoise(): 1, data.RandomBiasField(): 1, data.RandomBlur(std=(0, 1.5)): 1}, p=0.75))


def _same_draw(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (tuple, list)) and len(a) == 2 and isinstance(a[0], str):        # (class name, params)
        return a[0] == b[0] and a[1].keys() == b[1].keys() and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def test_a_compose_without_elastic_consumes_the_stream_it_always_did():
    """The replay below is the per-sample order the class has always had -- affine, flips, intensity -- on a second generator."""
    aff, flip, one = _members()
    tf = data.DeviceCompose([aff, flip, one, data.RescaleIntensity()], seed=77)
    assert tf.elastic == [] and tf.spatial == []
    mats, flags = tf.sample(24, (12, 16, 20))
    assert mats.shape == (24, 3, 4) and flags.shape == (24,)
    r = np.random.default_rng(77)
    for b in range(24):
        want_aff, want_bits, want_int = aff.sample(r), flip.sample(r), one.sample(r)
        bits, got_aff = tf.last_params[b]                                               # stays the 2-tuple
        assert bits == want_bits and _same_draw(got_aff, want_aff) and _same_draw(tf.last_intensity[b], want_int)
        assert flags[b] == want_bits | (8 if want_aff is not None else 0)
    assert tf.rng.random() == r.random()
    assert tf.last_elastic == [None] * 24


def test_draw_order_with_elastic_listed():
    """elastic, affine, flips, intensity -- wherever the elastic transform stands in the list."""
    aff, flip, one = _members()
    el = data.RandomElasticDeformation(num_control_points=(4, 5, 6), locked_borders=1, p=0.5)
    tf = data.DeviceCompose([aff, flip, el, one, data.RescaleIntensity()], seed=78)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tf.sample(24, (12, 16, 20))
    r = np.random.default_rng(78)
    for b in range(24):
        want_el, want_aff, want_bits, want_int = el.sample(r), aff.sample(r), flip.sample(r), one.sample(r)
        assert (tf.last_elastic[b] is None) == (want_el is None)
        assert want_el is None or (np.array_equal(tf.last_elastic[b], want_el) and tf.last_elastic[b].dtype == np.float64)
        assert tf.last_params[b][0] == want_bits and _same_draw(tf.last_params[b][1], want_aff) and _same_draw(tf.last_intensity[b], want_int)
    assert tf.rng.random() == r.random()
    combos = {(e is not None, p[1] is not None) for e, p in zip(tf.last_elastic, tf.last_params)}
    assert len(combos) == 4                                                             # listed singly, a sample may get both


def test_spatial_one_of_frequencies_and_exclusivity():
    one = data.OneOf({data.RandomAffine(degrees=15): 0.8, data.RandomElasticDeformation(num_control_points=5, locked_borders=1): 0.2}, p=0.5)
    assert one.spatial
    tf = data.DeviceCompose([one, data.RandomFlip(0), data.RescaleIntensity()], seed=9)
    assert tf.affine == [] and tf.elastic == [] and tf.spatial == [one]
    applied = affine = total = 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        while applied < 1000:
            tf.sample(50, (12, 16, 20))
            for el, (_, aff) in zip(tf.last_elastic, tf.last_params):
                assert el is None or aff is None                                        # never both members
                if applied < 1000 and (el is not None or aff is not None):
                    applied += 1
                    affine += aff is not None
                total += 1
    assert abs(affine / 1000 - 0.8) <= 0.06, affine                                     # sigma = 0.0126
    assert abs(applied / total - 0.5) <= 0.1
    # draws: the OneOf's p, its choice, the member's own, then the flips
    tf = data.DeviceCompose([one, data.RandomFlip(0)], seed=10)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        tf.sample(16, (12, 16, 20))
    r = np.random.default_rng(10)
    for b in range(16):
        pick = one.sample(r)
        bits = data.RandomFlip(0).sample(r)
        assert tf.last_params[b][0] == bits
        assert (pick is None) == (tf.last_elastic[b] is None and tf.last_params[b][1] is None)
        if pick is not None:
            assert _same_draw(tf.last_params[b][1] if isinstance(pick[0], data.RandomAffine) else tf.last_elastic[b], pick[1])
    assert tf.rng.random() == r.random()


def test_what_device_compose_and_one_of_refuse():
    el, aff = data.RandomElasticDeformation, data.RandomAffine
    with pytest.raises(NotImplementedError, match="spatial"):
        data.OneOf({aff(): 1, data.RandomNoise(): 1})
    with pytest.raises(NotImplementedError, match="spatial"):
        data.OneOf([data.RandomBlur(), el()])
    with pytest.raises(NotImplementedError, match="OneOf is not built"):
        data.OneOf([data.OneOf([aff()]), el()])                                         # nested
    with pytest.raises(NotImplementedError, match="RandomFlip is not built"):
        data.OneOf([aff(), data.RandomFlip()])
    with pytest.raises(NotImplementedError, match="RandomElasticDeformation"):
        data.DeviceCompose([el(), el()])
    with pytest.raises(NotImplementedError):
        data.DeviceCompose([data.OneOf([el(), el(num_control_points=5)])])
    with pytest.raises(NotImplementedError):
        data.DeviceCompose([data.OneOf([aff(), el()]), aff()])                          # in place of the single ones, not beside them
    with pytest.raises(NotImplementedError):
        data.DeviceCompose([data.OneOf([aff()]), data.OneOf([el()])])
    data.DeviceCompose([data.OneOf([aff(degrees=5), aff(degrees=20)])])                 # several affines are fine: one matrix per sample


def test_train_transforms_elastic_switch():
    tf = data.train_transforms(seed=4, elastic=True)
    assert tf.affine == [] and tf.elastic == [] and len(tf.spatial) == 1 and len(tf.flips) == 1 and tf.intensity == []
    one = tf.spatial[0]
    assert one.p == 0.5 and np.allclose(one.weights, [0.8, 0.2])
    aff, el = one.transforms
    assert isinstance(aff, data.RandomAffine) and aff.degrees == (-15.0, 15.0) and aff.p == 1.0
    assert isinstance(el, data.RandomElasticDeformation) and el.num_control_points == (7, 7, 7) and el.max_displacement == (7.5,) * 3 and el.p == 1.0
    full = data.train_transforms(seed=4, intensity=True, motion=True, elastic=True)
    assert len(full.spatial) == 1 and len(full.intensity) == 1 and len(full.intensity[0].transforms) == 4
    # the defaults reproduce today's objects and today's stream
    a, b = data.train_transforms(seed=4), data.train_transforms(seed=4, elastic=False)
    for t in (a, b):
        assert t.spatial == [] and t.elastic == [] and len(t.affine) == 1 and t.affine[0].p == 0.5 and t.affine[0].degrees == (-15.0, 15.0)
    a.sample(16, (12, 16, 20))
    r = np.random.default_rng(4)
    for bb in range(16):
        want_aff, want_bits = data.RandomAffine(degrees=15, p=0.5).sample(r), data.RandomFlip(axes=(0,)).sample(r)
        assert a.last_params[bb][0] == want_bits and _same_draw(a.last_params[bb][1], want_aff)
    assert a.rng.random() == r.random()


def test_data_preprocessor_obeys_elastic_augment():
    pre = data.DataPreprocessor({"data": {}}, seed=0)
    assert pre.train_transforms.spatial == [] and len(pre.train_transforms.affine) == 1
    pre = data.DataPreprocessor({"data": {"elastic_augment": True}}, seed=0)
    assert len(pre.train_transforms.spatial) == 1 and pre.train_transforms.affine == []
    assert pre.val_transforms.spatial == [] and pre.test_transforms.elastic == []
    pre = data.DataPreprocessor({"data": {"elastic_augment": False, "intensity_augment": True}}, seed=0)
    assert pre.train_transforms.spatial == [] and len(pre.train_transforms.intensity) == 1


# ------------------------------------------------------------------------------------------------ the float64 restatement
SHAPES = [((5, 6, 70), (4, 4, 4)), ((9, 13, 33), (4, 7, 10)), ((24, 32, 40), (7, 7, 7)), ((24, 32, 40), (16, 16, 16))]


@pytest.mark.parametrize("shape,n", SHAPES)
def test_reference_constant_field_is_reproduced(shape, n):
    """partition of unity: the weights of every voxel sum to 1"""
    c = np.array([1.5, -2.25, 3.0])
    d = elastic_ref.dense_field(np.broadcast_to(c, n + (3,)), shape)
    assert d.shape == (3,) + shape
    err = np.abs(d - c[:, None, None, None]).max()
    assert err <= 1e-12, err
    for S, k in zip(shape, n):
        B = elastic_ref.basis_matrix(S, k)
        assert (B >= 0).all() and ((B > 0).sum(axis=1) <= 4).all()


@pytest.mark.parametrize("shape,n", SHAPES)
def test_reference_linear_field_gives_linear_displacement(shape, n):
    """Cubic B-splines reproduce linear functions: control point j sits at u = j - 1 cells from the low face, so a coarse field a + g.j
    gives d(q) = a + g.(u(q) + 1), u_a(q) = (q_a + 0.5) (n_a - 3) / S_a -- linear in q, also across the cell borders."""
    g, a = np.array([0.3, -0.2, 0.15]), 0.7
    j = np.stack(np.meshgrid(*(np.arange(k, dtype=np.float64) for k in n), indexing="ij"), axis=-1)
    coarse = np.zeros(n + (3,))
    coarse[..., 1] = a + j @ g
    d = elastic_ref.dense_field(coarse, shape)
    u = [(np.arange(S) + 0.5) * (k - 3) / S for S, k in zip(shape, n)]
    want = a + g[0] * (u[0][:, None, None] + 1) + g[1] * (u[1][None, :, None] + 1) + g[2] * (u[2][None, None, :] + 1)
    err = np.abs(d[1] - want).max()
    assert err <= 1e-12 and not d[0].any() and not d[2].any(), err


def test_reference_locked_borders_at_the_outer_voxel_layers():
    """What locked_borders = 2 does at the faces of the volume, from the definition: the outer voxel layer (q = 0) lies at t = 0.5 / h in cell
    0, whose control points are layers 0..3; with layers 0 and 1 zero its displacement is B2(t) c2 + B3(t) c3 contracted over the other two
    axes -- layer 2 still weighs at least 1/6, so it is damped there, NOT zero (checked: a constant interior field of 1 leaves
    B2(t) + B3(t) at q = 0).  It is exactly zero at a voxel whose four control layers are all zero: on the outer voxel layers as soon as
    layers 2 and 3 vanish as well, which the second half checks with a field locked four deep."""
    shape, n = (24, 32, 40), (9, 9, 9)
    el = data.RandomElasticDeformation(num_control_points=n, max_displacement=5, locked_borders=2)
    coarse = el.sample(np.random.default_rng(3))
    d = elastic_ref.dense_field(coarse, shape)
    for a in range(3):
        B = [elastic_ref.basis_matrix(S, k) for S, k in zip(shape, n)]
        for face, layers in ((0, (2, 3)), (shape[a] - 1, (n[a] - 4, n[a] - 3))):
            t = 0.5 * (n[a] - 3) / shape[a]
            b2, b3 = (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6
            w = {layers[0]: b2 if face == 0 else b3, layers[1]: b3 if face == 0 else b2}                # mirrored at the far face
            others = [x for x in range(3) if x != a]
            want = sum(wk * np.einsum("pi,qj,ijc->cpq", B[others[0]], B[others[1]], np.take(coarse, k, axis=a)) for k, wk in w.items())
            got = np.take(d, face, axis=a + 1)
            assert np.abs(got - want).max() <= 1e-12 and np.abs(got).max() > 1e-3                       # the closed form, and not zero
    ones = np.zeros(n + (3,))
    ones[2:-2, 2:-2, 2:-2] = 1.0
    t = 0.5 * (n[0] - 3) / shape[0]
    assert abs(elastic_ref.dense_field(ones, shape)[0, 0, 12, 20] - ((-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6 + t ** 3 / 6)) <= 1e-12
    deep = coarse.copy()                                                                # four layers deep: cell 0 and cell M - 1 see zeros only
    for a in range(3):
        v = np.moveaxis(deep, a, 0)
        v[:4], v[-4:] = 0.0, 0.0
    dd = elastic_ref.dense_field(deep, shape)
    assert np.abs(dd).max() > 1e-3
    for a in range(3):
        h = shape[a] / (n[a] - 3)
        cell = int(np.ceil(h - 0.5))                                                    # voxels with u < 1
        assert not np.take(dd, range(cell), axis=a + 1).any() and not np.take(dd, range(shape[a] - cell, shape[a]), axis=a + 1).any()


def test_reference_read_equals_scipy_map_coordinates():
    rng = np.random.default_rng(8)
    shape = (9, 13, 33)
    vol = rng.standard_normal(shape) * 300 + 1000
    pad = float(vol.min())
    coarse = rng.uniform(-6, 6, (5, 6, 7, 3))                                           # unlocked: the read leaves the volume
    pos = elastic_ref.grid(shape) + elastic_ref.dense_field(coarse, shape)
    assert (pos.min(axis=(1, 2, 3)) < 0).all() and (pos.max(axis=(1, 2, 3)) > np.array(shape) - 1).all() and pos.min() < -1   # on every face
    got = elastic_ref.trilinear_read(vol, pos, pad)
    want = ndimage.map_coordinates(vol, pos, order=1, mode="grid-constant", cval=pad)
    err = np.abs(got - want).max()
    assert err <= 1e-9 * np.abs(vol).max(), err
    assert np.array_equal(elastic_ref.deform(vol, coarse), got)
    assert np.array_equal(elastic_ref.deform(vol, np.zeros((4, 4, 4, 3))), vol)         # the identity
