"""CPU: the host side of the intensity normalisers (data.RescaleIntensity with percentiles / masking_method, data.ZNormalization, their
place in DeviceCompose and the `normalization` switch) and the numpy reference (tests/normalize_ref.py) against closed forms.  No kernel
runs here; tests/test_normalize_gpu.py holds the kernels to the same reference."""
import numpy as np
import pytest

import normalize_ref as ref
from gaviko_amd import data


# ---- constructors ---------------------------------------------------------------------------------------------------------------------
def test_rescale_defaults_are_the_plain_minmax():
    t = data.RescaleIntensity()
    assert (t.out_min, t.out_max, t.percentiles, t.masking_method, t.plain) == (0.0, 1.0, (0.0, 100.0), None, True)
    assert data.RescaleIntensity((0, 1), percentiles=(0, 100), masking_method=None).plain
    assert not data.RescaleIntensity(percentiles=(0.5, 99.5)).plain
    assert not data.RescaleIntensity(masking_method="mean").plain
    assert not data.RescaleIntensity(masking_method=0.0).plain


@pytest.mark.parametrize("bad", [(-1, 100), (0, 100.5), (60, 40), (1, 2, 3), (50,)])
def test_rescale_rejects_bad_percentiles(bad):
    with pytest.raises(ValueError):
        data.RescaleIntensity(percentiles=bad)


@pytest.mark.parametrize("cls", [data.RescaleIntensity, data.ZNormalization])
@pytest.mark.parametrize("bad", [lambda x: x > 0, "label", "median", True, (1, 2)])
def test_unbuilt_masks_are_refused(cls, bad):
    with pytest.raises(NotImplementedError):
        cls(masking_method=bad)


def test_mask_rules_and_the_alias():
    assert data.ZNormalization.mean == "mean"
    assert data.ZNormalization(masking_method=data.ZNormalization.mean).masking_method == "mean"
    assert data.ZNormalization().masking_method is None
    assert data.ZNormalization(masking_method=3).masking_method == 3.0
    assert data.RescaleIntensity(percentiles=(50, 50), masking_method=-2.5).masking_method == -2.5


# ---- DeviceCompose bookkeeping --------------------------------------------------------------------------------------------------------
def test_compose_sorts_the_normalisers():
    r, z = data.RescaleIntensity(percentiles=(1, 99)), data.ZNormalization()
    c = data.DeviceCompose([data.RandomFlip(), r])
    assert c.rescale == [r] and c.znorm == [] and c.last_norm_status is None
    c = data.DeviceCompose([z, data.RandomFlip()])
    assert c.rescale == [] and c.znorm == [z]


@pytest.mark.parametrize("pair", [(data.RescaleIntensity, data.RescaleIntensity), (data.RescaleIntensity, data.ZNormalization),
                                  (data.ZNormalization, data.ZNormalization)])
def test_at_most_one_normaliser(pair):
    with pytest.raises(NotImplementedError):
        data.DeviceCompose([pair[0](), pair[1]()])


def test_built_list_keeps_its_beginning():
    assert data._BUILT.startswith("RandomAffine (at most one), RandomFlip, RandomNoise, RandomBiasField, RandomBlur, RandomMotion, OneOf of the last "
                                  "four, RescaleIntensity (at most one); RandomElasticDeformation (at most one)")
    assert "ZNormalization" in data._BUILT and data._BUILT.index("ZNormalization") > data._BUILT.index("RandomElasticDeformation")


@pytest.mark.parametrize("kw", [dict(), dict(intensity=True, motion=True), dict(elastic=True, intensity=True)])
def test_the_normaliser_draws_nothing(kw):
    draws = []
    for norm in ("minmax", "percentile", "znorm"):
        c = data.train_transforms(seed=11, normalization=norm, **kw)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mats, flags = c.sample(5, (24, 32, 40))
        draws.append((mats, flags, repr(c.last_params), repr(c.last_intensity), repr(c.last_elastic), c.rng.random()))
    for d in draws[1:]:
        assert np.array_equal(d[0], draws[0][0]) and np.array_equal(d[1], draws[0][1]) and d[2:] == draws[0][2:]


# ---- the normalization switch ---------------------------------------------------------------------------------------------------------
def _last(c):
    return (c.rescale + c.znorm)[0]


def test_normalization_switch():
    for make in (lambda n: data.train_transforms(seed=0, normalization=n), data.eval_transforms):
        t = _last(make("minmax"))
        assert isinstance(t, data.RescaleIntensity) and t.plain and (t.out_min, t.out_max) == (0.0, 1.0)
        t = _last(make("percentile"))
        assert isinstance(t, data.RescaleIntensity) and t.percentiles == (0.5, 99.5) and t.masking_method is None and (t.out_min, t.out_max) == (0.0, 1.0)
        t = _last(make("znorm"))
        assert isinstance(t, data.ZNormalization) and t.masking_method == "mean"
        with pytest.raises(ValueError):
            make("histogram")
    assert _last(data.train_transforms()).plain and _last(data.eval_transforms()).plain


def test_preprocessor_reads_the_normalization():
    pre = data.DataPreprocessor({"data": {}}, seed=0)
    assert all(_last(c).plain for c in (pre.train_transforms, pre.val_transforms, pre.test_transforms))
    pre = data.DataPreprocessor({"data": {"normalization": "znorm"}}, seed=0)
    assert all(isinstance(_last(c), data.ZNormalization) for c in (pre.train_transforms, pre.val_transforms, pre.test_transforms))
    pre = data.DataPreprocessor({"data": {"normalization": "percentile", "intensity_augment": True}}, seed=0)
    assert all(_last(c).percentiles == (0.5, 99.5) for c in (pre.train_transforms, pre.val_transforms, pre.test_transforms))
    assert pre.train_transforms.intensity


# ---- the reference against closed forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 101, 4097])
def test_ref_percentiles_of_arange(n):
    x = np.random.default_rng(n).permutation(n).astype(np.float32)
    qs = (0, 0.5, 25, 50, 99.5, 100)
    pairs, cut, cnt = ref.order_stats(x, qs)
    assert cnt == n
    for j, q in enumerate(qs):
        v = (n - 1) * (q / 100.0)
        assert pairs[j, 0] == np.floor(v) and pairs[j, 1] == min(np.floor(v) + 1, n - 1)
        assert abs(float(cut[j]) - v) <= 2.0 ** -23 * max(v, 1.0)              # p (n - 1) / 100, one float32 rounding of a float64 value
        assert cut[j] == ref.linear_cutoff(pairs[j, 0], pairs[j, 1], n, q)        # numpy evaluates exactly the written rule


def test_ref_two_valued_volume():
    x = np.array([5.0] * 30 + [9.0] * 10, dtype=np.float32)                      # sorted: ranks 0..29 are 5, ranks 30..39 are 9
    pairs, cut, n = ref.order_stats(np.random.default_rng(0).permutation(x), (0, 50, 74, 75, 76, 100))
    assert n == 40
    assert pairs.tolist() == [[5, 5], [5, 5], [5, 5], [5, 9], [5, 9], [9, 9]]  # v = 0, 19.5, 28.86, 29.25, 29.64, 39
    assert cut[[0, 1, 2, 5]].tolist() == [5, 5, 5, 9]
    assert cut[3] == np.float32(5 + 4 * 0.25) and abs(float(cut[4]) - (5 + 4 * 0.64)) < 1e-5
    s = ref.stats(x)
    assert (s["min"], s["max"], s["n"]) == (5.0, 9.0, 40) and s["mean"] == 6.0
    assert abs(s["std"] - np.sqrt((30 * 1.0 + 10 * 9.0) / 39)) < 1e-14
    m = ref.stats(x, "mean")                                                     # above the mean 6: the ten nines
    assert (m["n"], m["mean"], m["std"]) == (10, 9.0, 0.0)
    assert ref.znorm(x, "mean")[1] == 2 and ref.znorm(x, 100.0)[1] == 1 and ref.znorm(x)[1] == 0


@pytest.mark.parametrize("q", [(0.5, 99.5), (1, 99), (25, 75), (0, 100)])
def test_ref_clipped_extremes_are_the_cutoffs(q):
    x = (np.random.default_rng(3).standard_normal(5001) * 1000).astype(np.float32)
    _, cut, _ = ref.order_stats(x, q)
    clipped = np.clip(x, cut[0], cut[1])
    assert clipped.min() == cut[0] and clipped.max() == cut[1]
    y, status = ref.rescale(x, 0.0, 1.0, q)
    assert status == 0 and y.min() == 0.0 and y.max() == 1.0


def test_ref_rescale_matches_the_oracle_on_the_defaults():
    from oracle import data_ref
    x = (np.random.default_rng(5).standard_normal(4099) * 300 + 1000).astype(np.float32)
    y, status = ref.rescale(x, 0.0, 1.0)
    assert status == 0 and np.array_equal(y.view(np.uint32), data_ref.rescale_intensity(x).view(np.uint32))
    const = np.full(17, 3.5, np.float32)
    y, status = ref.rescale(const)
    assert status == 2 and np.array_equal(y, const)
    assert ref.rescale(x, percentiles=(50, 50))[1] == 2 and ref.rescale(x, rule=1e9)[1] == 1


def test_ref_znorm_moments():
    x = (np.random.default_rng(7).standard_normal(3001) * 40 + 100).astype(np.float32)
    for rule in (None, "mean", 90.0):
        y, status = ref.znorm(x, rule)
        m = ref.mask_of(x, rule)
        assert status == 0 and abs(y[m].mean()) < 1e-12 and abs(y[m].std(ddof=1) - 1) < 1e-12


def test_ref_mask_of_mean_is_the_float32_compare():
    x = np.array([1, 2, 3, 4, 10], np.float32)                                    # mean 4: only 10 is above it
    assert ref.mask_of(x, "mean").tolist() == [False, False, False, False, True]
    assert ref.mask_of(x, 3).tolist() == [False, False, False, True, True]
    assert ref.mask_of(np.array([-0.0, 0.0], np.float32), 0.0).tolist() == [False, False]


# ---- the input families of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ref.STD_FAMILIES)
def test_families_keep_the_std_bound_meaningful(fam):
    """the GPU test's relative bound on the std assumes std >= |mean| / 64 (the error of the mean is then second order)"""
    for V in (64, 65, 1023, 4097):
        x = ref.family(fam, V)
        assert x.shape == (3, V) and x.dtype == np.float32 and np.isfinite(x).all()
        for b in range(3):
            for rule in (None, "mean"):
                s = ref.stats(x[b], rule)
                assert s["n"] < 2 or s["std"] >= abs(s["mean"]) / 64, (fam, V, b, rule, s)


def test_families_are_what_they_say():
    x = ref.family("zeros60", 4097)
    assert 0.55 < np.mean(x == 0) < 0.65 and x.min() == 0
    s = ref.family("special", 70001)
    assert s[0].max() == np.float32(3e38) and s[0].min() == np.float32(-3e38)
    for b in range(3):
        assert np.any(np.signbit(s[b]) & (s[b] == 0)) and np.any(~np.signbit(s[b]) & (s[b] == 0))
        assert np.any((s[b] != 0) & (np.abs(s[b]) < np.finfo(np.float32).tiny)) and s[b].max() > 2e38 and s[b].min() < -2e38
    lo, hi = ref.family("low10", 4097).view(np.uint32), ref.family("high11", 4097).view(np.uint32)
    assert len(np.unique(lo >> 10)) == 1 and len(np.unique(lo)) > 900
    assert len(np.unique(hi & 0x1FFFFF)) == 1 and len(np.unique(hi)) > 1000
    assert len({ref.family("constant", 5)[b, 0] for b in range(3)}) == 3
