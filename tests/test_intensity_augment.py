"""CPU: host side of the intensity augmentation (gaviko_amd/data.py): the blur weight table against scipy, the parameter sampling of
RandomNoise / RandomBiasField / RandomBlur / OneOf, and that DeviceCompose without an intensity transform consumes the random stream it
always did.  The kernels themselves: tests/test_intensity_augment_gpu.py."""
import numpy as np
import pytest

import intensity_ref
from gaviko_amd import data


def test_blur_tables_equal_scipy_impulse_response():
    from scipy import ndimage
    sig = np.array([[1.5, 0.3, 1.2], [0.1, 0.9, 0.0], [4.0, 2.0, 0.124], [0.0, 0.0, 0.0]])
    weights, radius = data.blur_tables(sig)
    assert weights.shape == (4, 3, 33) and weights.dtype == np.float32 and radius.dtype == np.int32
    assert radius.tolist() == [[6, 1, 5], [0, 4, 0], [16, 8, 0], [0, 0, 0]]            # int(4 sigma + 0.5); 0.124 -> 0, 0.125 would be 1
    for b in range(4):
        for a in range(3):
            r = radius[b, a]
            r_ref, w_ref = intensity_ref.weight_table(sig[b, a])
            assert r == r_ref
            imp = np.zeros(101)
            imp[50] = 1.0
            resp = ndimage.gaussian_filter(imp, sigma=sig[b, a])                       # the impulse response IS scipy's tap table
            assert np.count_nonzero(resp) == 2 * r + 1
            taps = weights[b, a, :2 * r + 1]
            assert np.array_equal(taps, resp[50 - r:51 + r].astype(np.float32)) and np.array_equal(taps, w_ref.astype(np.float32))
            assert not weights[b, a, 2 * r + 1:].any()
    assert (weights[3, :, 0] == 1.0).all()                                             # skipped axes: the identity tap
    with pytest.raises(ValueError, match="sigma above 4"):
        data.blur_tables([[4.2, 1.0, 1.0]])
    with pytest.raises(NotImplementedError, match="sigma above 4"):
        data.RandomBlur(std=(0, 5))


def test_sampling_ranges():
    rng = np.random.default_rng(11)
    noise, bias, blur = data.RandomNoise(mean=2.0), data.RandomBiasField(), data.RandomBlur(std=(0, 1.5))
    seeds = set()
    for _ in range(2000):
        name, p = noise.sample(rng)
        assert name == "RandomNoise" and -2.0 <= p["mean"] <= 2.0 and 0.0 <= p["std"] <= 0.25 and 0 <= p["seed"] < 2 ** 64
        seeds.add(p["seed"])
        name, p = bias.sample(rng)
        assert name == "RandomBiasField" and p["order"] == 3 and p["coefficients"].shape == (20,) and (np.abs(p["coefficients"]) <= 0.5).all()
        name, p = blur.sample(rng)
        assert name == "RandomBlur" and p["std"].shape == (3,) and ((0 <= p["std"]) & (p["std"] <= 1.5)).all()
    assert len(seeds) == 2000 and max(seeds) >= 2 ** 63                                # 64-bit draws
    assert data.RandomNoise().sample(rng)[1]["mean"] == 0.0                            # tio default mean=0
    assert [len(data.bias_terms(o)) for o in range(4)] == [1, 4, 10, 20] and data.bias_terms(1) == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
    assert data.bias_terms(3) == intensity_ref.bias_terms(3)
    assert len(data.RandomBiasField(order=1).sample(rng)[1]["coefficients"]) == 4
    c = data.bias_coefficients([1.0, 2.0, 3.0, 4.0], 1, 3)                             # (0,0,0) (0,0,1) (0,1,0) (1,0,0) inside the order-3 list
    assert c.shape == (20,) and [c[data.bias_terms(3).index(t)] for t in data.bias_terms(1)] == [1.0, 2.0, 3.0, 4.0] and c.sum() == 10.0
    n = sum(data.RandomNoise(p=0.3).sample(rng) is not None for _ in range(3000))
    assert 800 < n < 1000                                                              # p = 0.3: 900 +- 4.5 sigma
    with pytest.raises(NotImplementedError):
        data.RandomBiasField(order=4)


def test_one_of_frequencies():
    rng = np.random.default_rng(5)
    one = data.OneOf({data.RandomNoise(): 2, data.RandomBiasField(): 1, data.RandomBlur(): 1}, p=0.75)
    assert np.allclose(one.weights, [0.5, 0.25, 0.25])
    N = 4000
    counts = {None: 0, "RandomNoise": 0, "RandomBiasField": 0, "RandomBlur": 0}
    for _ in range(N):
        d = one.sample(rng)
        counts[d[0] if d else None] += 1
    # binomial standard deviations at N = 4000 are <= 32: five of them
    assert abs(counts[None] - 0.25 * N) < 160 and abs(counts["RandomNoise"] - 0.375 * N) < 160
    assert abs(counts["RandomBiasField"] - 0.1875 * N) < 160 and abs(counts["RandomBlur"] - 0.1875 * N) < 160
    eq = data.OneOf([data.RandomNoise(), data.RandomBlur()])
    assert np.allclose(eq.weights, [0.5, 0.5]) and all(eq.sample(rng) is not None for _ in range(50))     # p = 1: always exactly one


def test_no_intensity_transform_consumes_the_same_stream():
    """The documented draw order per sample: RandomAffine (one uniform for p; when applied 3 scales, 3 angles, 3 translations), then one
    uniform per RandomFlip axis -- replayed here on a second generator with the same seed."""
    tf = data.train_transforms(seed=31)
    assert not tf.intensity
    B, shape = 64, (12, 16, 20)
    mats, flags = tf.sample(B, shape)
    r = np.random.default_rng(31)
    for b in range(B):
        aff = None
        if r.random() < 0.5:
            aff = (r.uniform(0.9, 1.1, 3), r.uniform(-15.0, 15.0, 3), r.uniform(0.0, 0.0, 3))
        bits = 1 if r.random() < 0.5 else 0
        got_bits, got_aff = tf.last_params[b]
        assert got_bits == bits and (got_aff is None) == (aff is None) and flags[b] == bits | (8 if aff is not None else 0)
        if aff is not None:
            assert all(np.array_equal(g, w) for g, w in zip(got_aff, aff))
            assert np.array_equal(mats[b], data.affine_matrix(*aff, shape).astype(np.float32))
    assert tf.rng.random() == r.random()                                               # and nothing more was drawn
    assert tf.last_intensity == [None] * B


def test_intensity_draws_follow_the_spatial_draws_of_each_sample():
    tf = data.train_transforms(seed=31, intensity=True)
    one = tf.intensity[0]
    assert isinstance(one, data.OneOf) and [type(t).__name__ for t in one.transforms] == ["RandomNoise", "RandomBiasField", "RandomBlur"]
    assert one.p == 0.75 and np.allclose(one.weights, 1 / 3) and one.transforms[2].std == (0.0, 1.5)
    tf.sample(16, (12, 16, 20))
    r = np.random.default_rng(31)
    kinds = set()
    for b in range(16):
        aff = data.RandomAffine(degrees=15, p=0.5).sample(r)
        bits = data.RandomFlip(axes=(0,)).sample(r)
        want = data.OneOf(one.transforms, p=0.75).sample(r)
        assert tf.last_params[b][0] == bits and (tf.last_params[b][1] is None) == (aff is None)
        got = tf.last_intensity[b]
        assert (got is None) == (want is None)
        if got is not None:
            assert got[0] == want[0] and all(np.array_equal(got[1][k], want[1][k]) for k in want[1])
            kinds.add(got[0])
    assert len(kinds) >= 2
    two = data.DeviceCompose([data.RandomNoise(), data.RandomBlur(p=0.0), data.RescaleIntensity()], seed=1)   # listed singly: a tuple per sample
    two.sample(3, (4, 4, 4))
    assert all(d[0][0] == "RandomNoise" and d[1] is None for d in two.last_intensity)


def test_default_train_transforms_hold_no_intensity_transform():
    tf = data.train_transforms(seed=0)
    assert tf.intensity == [] and [type(t).__name__ for t in tf.affine + tf.flips + tf.rescale] == ["RandomAffine", "RandomFlip", "RescaleIntensity"]
    pre = data.DataPreprocessor({"data": {}}, seed=0)
    assert pre.train_transforms.intensity == [] and pre.val_transforms.intensity == []
    pre = data.DataPreprocessor({"data": {"intensity_augment": True}}, seed=0)
    assert len(pre.train_transforms.intensity) == 1 and pre.val_transforms.intensity == [] and pre.test_transforms.intensity == []


def test_unknown_transform_still_raises():
    class RandomMotion:
        pass

    with pytest.raises(NotImplementedError, match="RandomNoise, RandomBiasField, RandomBlur"):
        data.DeviceCompose([data.RandomFlip(), RandomMotion(), data.RescaleIntensity()])
    with pytest.raises(NotImplementedError, match="RandomMotion"):
        data.OneOf({data.RandomNoise(): 1, RandomMotion(): 1})
    with pytest.raises(NotImplementedError):
        data.OneOf([data.OneOf([data.RandomNoise()])])                                 # no nesting
    with pytest.raises(NotImplementedError):
        data.DeviceCompose([data.RescaleIntensity(), data.RescaleIntensity()])


def test_reference_restatement_is_self_consistent():
    """intensity_ref against closed forms: the noise field is standard normal, the bias field of a known polynomial, n = 1 axes."""
    z = intensity_ref.noise_z(1234567890123456789, 200000)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01 and np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2)) + 1e-12
    assert not np.array_equal(z[:1000], intensity_ref.noise_z(1234567890123456790, 1000))
    f = intensity_ref.bias_field((3, 1, 5), [0.5, 0.25, 7.0, -1.0], 1)                 # exp(0.5 + 0.25 c2 + 7 c1 - c0) with c1 = 0 on the n = 1 axis
    c0, c2 = np.array([-1.0, 0.0, 1.0])[:, None, None], np.linspace(-1, 1, 5)[None, None, :]
    assert np.allclose(f, np.exp(0.5 + 0.25 * c2 - c0), rtol=1e-12, atol=0)
