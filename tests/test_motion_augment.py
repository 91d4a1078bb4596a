"""CPU: host side of RandomMotion (gaviko_amd/data.py): the circular-convolution tables against torchio's compositing written literally
with np.fft (tests/motion_ref.py), the parameter sampling and its draw order, and the switches that put RandomMotion into the training
pipeline.  The kernel itself: tests/test_motion_augment_gpu.py."""
import numpy as np
import pytest

import motion_ref
from gaviko_amd import data

# (W, times, the hand-stated source order of the slabs)
TABLE_CASES = [
    (20, [0.3], [1, 0]),                           # K = 1, t < 0.5: none above 0.5, so entries 0 and K swap
    (20, [0.7], [0, 1]),                           # K = 1, t > 0.5: index 0 swaps with itself
    (33, [0.3, 0.7], [1, 0, 2]),                   # default-like times: the original fills the centre; odd W
    (68, [0.25, 0.45], [2, 1, 0]),                 # both below 0.5
    (68, [0.55, 0.8], [0, 1, 2]),                  # both above 0.5
    (20, [0.31, 0.34], [2, 1, 0]),                 # int(6.2) = int(6.8) = 6: the middle slab is empty
    (160, [0.2, 0.5, 0.77], [2, 1, 0, 3]),         # K = 3; 0.5 is not above 0.5: index 2 is the first
    (160, [0.26, 0.52, 0.74], [1, 0, 2, 3]),
    (33, [0.1, 0.2, 0.3], [3, 1, 2, 0]),
]


@pytest.mark.parametrize("W,times,order", TABLE_CASES)
def test_motion_tables_equal_the_fft_composite_impulse_response(W, times, order):
    K = len(times)
    ctab, src = data.motion_tables([times], W)
    assert ctab.shape == (1, K + 1, W) and ctab.dtype == np.float32 and src.shape == (1, K + 1)
    assert src[0].tolist() == order
    for s in range(K + 1):
        images = [np.zeros(W) for _ in range(K + 1)]
        images[s][0] = 1.0
        resp = motion_ref.composite(images, times)                                    # the impulse response IS the kernel of image s
        err = np.abs(ctab[0, s] - resp).max()
        assert err <= 1e-6, (s, err)                                                   # float32 rounding of values <= 1
        vol = [np.zeros((3, 4, W)) for _ in range(K + 1)]                              # in 3-D the other two axes cancel: one line answers
        vol[s][1, 2, 5] = 1.0
        resp3 = motion_ref.composite(vol, times)
        assert np.abs(resp3[1, 2] - np.roll(resp, 5)).max() <= 1e-14
        resp3[1, 2] = 0.0
        assert np.abs(resp3).max() <= 1e-14
    impulse = np.zeros(W)
    impulse[0] = 1.0
    assert np.abs(ctab[0].astype(np.float64).sum(axis=0) - impulse).max() <= (K + 1) * 2.0 ** -24
    edges = [0] + [int(W * t) for t in times] + [W]
    if any(a == b for a, b in zip(edges, edges[1:])):
        assert not ctab[0, order[[a == b for a, b in zip(edges, edges[1:])].index(True)]].any()        # an empty slab: a zero kernel


def test_motion_tables_per_sample_rows():
    ctab, src = data.motion_tables([[0.3, 0.7], [0.55, 0.8], [0.25, 0.45]], 68)
    assert src.tolist() == [[1, 0, 2], [0, 1, 2], [2, 1, 0]]
    for b, t in enumerate([[0.3, 0.7], [0.55, 0.8], [0.25, 0.45]]):
        assert np.array_equal(ctab[b], data.motion_tables(t, 68)[0][0])               # a 1-D times argument is one sample


def test_sampling_ranges_and_times():
    rng = np.random.default_rng(13)
    mo, wide = data.RandomMotion(), data.RandomMotion(degrees=(2, 5), translation=3, num_transforms=4)
    for _ in range(2000):
        name, p = mo.sample(rng)
        assert name == "RandomMotion" and p["degrees"].shape == (2, 3) and p["translation"].shape == (2, 3) and p["times"].shape == (2,)
        assert (np.abs(p["degrees"]) <= 10).all() and (np.abs(p["translation"]) <= 10).all()
        assert 0 < p["times"][0] < p["times"][1] < 1
        assert abs(p["times"][0] - 1 / 3) <= 0.1 + 1e-12 and abs(p["times"][1] - 2 / 3) <= 0.1 + 1e-12     # 0.3 step, step = 1/3
        name, p = wide.sample(rng)
        assert p["degrees"].shape == (4, 3) and ((2 <= p["degrees"]) & (p["degrees"] <= 5)).all() and (np.abs(p["translation"]) <= 3).all()
        assert (np.diff(np.r_[0.0, p["times"], 1.0]) > 0).all()
    n = sum(data.RandomMotion(p=0.3).sample(rng) is not None for _ in range(3000))
    assert abs(n - 900) < 113                                                          # p = 0.3: 900 +- 4.5 sigma (sigma = 25.1)
    for bad in (0, 5):
        with pytest.raises(NotImplementedError):
            data.RandomMotion(num_transforms=bad)
    with pytest.raises(NotImplementedError):
        data.RandomMotion(image_interpolation="nearest")


def test_draw_order_replayed_on_a_second_generator():
    """One uniform for p, degrees [K][3], translation [K][3], then the K time perturbations ~ U(+-0.3 step) added to step (1..K)."""
    mo = data.RandomMotion(degrees=7, translation=(-2, 6), num_transforms=3, p=0.6)
    rng, r = np.random.default_rng(31), np.random.default_rng(31)
    seen = 0
    for _ in range(64):
        got = mo.sample(rng)
        if r.random() >= 0.6:
            assert got is None
            continue
        deg, tr = r.uniform(-7.0, 7.0, (3, 3)), r.uniform(-2.0, 6.0, (3, 3))
        times = 0.25 * np.arange(1, 4) + r.uniform(-0.3 * 0.25, 0.3 * 0.25, 3)
        assert got[0] == "RandomMotion" and np.array_equal(got[1]["degrees"], deg) and np.array_equal(got[1]["translation"], tr)
        assert np.array_equal(got[1]["times"], times)
        seen += 1
    assert seen > 20 and rng.random() == r.random()                                    # and nothing more was drawn


def test_train_transforms_motion_switch():
    tf = data.train_transforms(seed=31, intensity=True, motion=True)
    one = tf.intensity[0]
    assert isinstance(one, data.OneOf) and [type(t).__name__ for t in one.transforms] == ["RandomNoise", "RandomBiasField", "RandomBlur", "RandomMotion"]
    assert one.p == 0.75 and np.array_equal(one.weights, [0.25] * 4) and one.transforms[2].std == (0.0, 1.5)
    mo = one.transforms[3]
    assert mo.degrees == (-10.0, 10.0) and mo.translation == (-10.0, 10.0) and mo.num_transforms == 2 and mo.p == 1.0    # tio.RandomMotion()
    three = data.train_transforms(seed=31, intensity=True).intensity[0]                # intensity alone: the three-member group, unchanged
    assert [type(t).__name__ for t in three.transforms] == ["RandomNoise", "RandomBiasField", "RandomBlur"] and np.allclose(three.weights, 1 / 3)
    assert [type(t).__name__ for t in data.train_transforms(seed=31, intensity=True, motion=False).intensity[0].transforms] == \
        ["RandomNoise", "RandomBiasField", "RandomBlur"]
    with pytest.raises(ValueError, match="intensity=True"):
        data.train_transforms(seed=31, motion=True)
    # the draws of the four-member pipeline follow each sample's spatial draws, as for the three-member one
    tf.sample(32, (12, 16, 20))
    r = np.random.default_rng(31)
    kinds = set()
    for b in range(32):
        aff = data.RandomAffine(degrees=15, p=0.5).sample(r)
        bits = data.RandomFlip(axes=(0,)).sample(r)
        want = data.OneOf(one.transforms, p=0.75).sample(r)
        assert tf.last_params[b][0] == bits and (tf.last_params[b][1] is None) == (aff is None)
        got = tf.last_intensity[b]
        assert (got is None) == (want is None)
        if got is not None:
            assert got[0] == want[0] and all(np.array_equal(got[1][k], want[1][k]) for k in want[1])
            kinds.add(got[0])
    assert "RandomMotion" in kinds and len(kinds) >= 3


def test_data_preprocessor_obeys_motion_augment():
    names = lambda tf: [type(t).__name__ for t in tf.intensity[0].transforms]          # noqa: E731
    pre = data.DataPreprocessor({"data": {"intensity_augment": True}}, seed=0)
    assert names(pre.train_transforms) == ["RandomNoise", "RandomBiasField", "RandomBlur"]
    pre = data.DataPreprocessor({"data": {"intensity_augment": True, "motion_augment": True}}, seed=0)
    assert names(pre.train_transforms) == ["RandomNoise", "RandomBiasField", "RandomBlur", "RandomMotion"]
    assert pre.val_transforms.intensity == [] and pre.test_transforms.intensity == []
    pre = data.DataPreprocessor({"data": {"intensity_augment": True, "motion_augment": False}}, seed=0)
    assert names(pre.train_transforms) == ["RandomNoise", "RandomBiasField", "RandomBlur"]
    with pytest.raises(ValueError):
        data.DataPreprocessor({"data": {"motion_augment": True}}, seed=0)


def test_one_of_frequencies_with_four_members():
    rng = np.random.default_rng(5)
    one = data.OneOf({data.RandomNoise(): 0.25, data.RandomBiasField(): 0.25, data.RandomBlur(): 0.25, data.RandomMotion(): 0.25}, p=0.75)
    N = 4000
    counts = {None: 0, "RandomNoise": 0, "RandomBiasField": 0, "RandomBlur": 0, "RandomMotion": 0}
    for _ in range(N):
        d = one.sample(rng)
        counts[d[0] if d else None] += 1
    # binomial standard deviations at N = 4000 are <= 32: five of them
    assert abs(counts[None] - 0.25 * N) < 160
    assert all(abs(counts[k] - 0.1875 * N) < 160 for k in ("RandomNoise", "RandomBiasField", "RandomBlur", "RandomMotion"))
    assert data.RandomMotion in data.INTENSITY_TRANSFORMS
    single = data.DeviceCompose([data.RandomMotion(p=1.0), data.RescaleIntensity()], seed=1)      # listed singly
    single.sample(3, (4, 4, 4))
    assert all(d[0] == "RandomMotion" for d in single.last_intensity)


def test_foreign_classes_still_raise_and_the_plain_stream_is_unchanged():
    class RandomMotion:                                                                 # a foreign class that happens to carry the name
        pass

    with pytest.raises(NotImplementedError, match="RandomNoise, RandomBiasField, RandomBlur"):
        data.DeviceCompose([data.RandomFlip(), RandomMotion(), data.RescaleIntensity()])
    with pytest.raises(NotImplementedError, match="RandomMotion"):
        data.OneOf({data.RandomNoise(): 1, RandomMotion(): 1})
    a, b = data.train_transforms(seed=3), data.train_transforms(seed=3, intensity=False, motion=False)
    a.sample(16, (12, 16, 20))
    b.sample(16, (12, 16, 20))
    assert a.rng.random() == b.rng.random() and a.last_intensity == [None] * 16
