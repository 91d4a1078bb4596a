"""CPU: the host half of gaviko_amd.data.Conform -- the banded tables of `conform_tables`, the pass plan of `ops.conform_plan`, the ragged
batch and its collate function, the argument errors and the DataPreprocessor wiring.  The tables are applied in float64 (dtype=np.float64:
before their one rounding to float32) and compared within 1e-12 with F.interpolate (trilinear / nearest-exact, align_corners=False),
with scipy.ndimage.gaussian_filter1d(mode='nearest') followed by that interpolation, and with the plain loops of tests/conform_ref.py."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy import ndimage
from torch.utils.data import DataLoader, Dataset

import conform_ref
from gaviko_amd import data as gdata
from gaviko_amd import lib, ops
from gaviko_amd.data import Conform, CropOrPad, RaggedBatch, Resample, Resize, collate_ragged, conform_tables

SRC, DST = (13, 22, 37), (9, 31, 20)


def _dense(tables, b, a, n, target_shape):
    """Row q of axis a as a dense float64 row over the n inputs."""
    start, w, inside = tables.axis(b, a, target_shape)
    M = np.zeros((len(start), n), dtype=np.float64)
    for q in range(len(start)):
        if inside[q]:
            for t in range(w.shape[1]):
                if w[q, t] != 0:
                    M[q, start[q] + t] += w[q, t]
    return M


def _apply(tables, b, x, target_shape):
    M = [_dense(tables, b, a, x.shape[a], target_shape) for a in range(3)]
    return np.einsum("ai,bj,ck,ijk->abc", M[0], M[1], M[2], x.astype(np.float64))


def _volume(shape, seed=0):
    return np.random.default_rng(seed).normal(size=shape)


def test_resize_linear_is_trilinear_interpolate():
    x = _volume(SRC)
    for src, dst in ((SRC, DST), (DST, SRC), ((1, 5, 3), (4, 5, 2))):
        x = _volume(src, 1)
        t = conform_tables([src], [(1, 1, 1)], [Resize(dst, antialias=False)], dst, dtype=np.float64)
        want = F.interpolate(torch.from_numpy(x)[None, None], size=dst, mode="trilinear", align_corners=False)[0, 0].numpy()
        err = np.abs(_apply(t, 0, x, dst) - want).max()
        assert err <= 1e-12, err
        assert t.weights.shape[2] == 2 or src == (1, 5, 3)
        np.testing.assert_allclose(t.geometry[0, :, 0], np.array(src) / np.array(dst), rtol=0, atol=0)


def test_resize_nearest_is_nearest_exact():
    for src, dst in ((SRC, DST), (DST, SRC)):
        x = _volume(src, 2)
        for antialias in (False, True):                                   # ignored under nearest
            t = conform_tables([src], [(1, 1, 1)], [Resize(dst, "nearest", antialias=antialias)], dst, dtype=np.float64)
            want = F.interpolate(torch.from_numpy(x)[None, None], size=dst, mode="nearest-exact")[0, 0].numpy()
            assert np.array_equal(_apply(t, 0, x, dst), want)
            assert t.weights.shape[2] == 1 and (t.weights == 1).all() and t.inside.all()


def test_resize_antialias_is_gaussian_filter_then_interpolation():
    x = _volume(SRC, 3)
    t = conform_tables([SRC], [(1, 1, 1)], [Resize(DST)], DST, dtype=np.float64)
    y = x
    for a in range(3):
        r = SRC[a] / DST[a]
        if r > 1:
            sigma = math.sqrt((r * r - 1) / (8 * math.log(2)))
            y = ndimage.gaussian_filter1d(y, sigma, axis=a, mode="nearest", truncate=4.0)
            assert t.taps[0, a] <= 2 * int(4 * sigma + 0.5) + 2
        else:
            assert t.taps[0, a] == 2                                      # the axis that grows is not smoothed
    want = F.interpolate(torch.from_numpy(y)[None, None], size=DST, mode="trilinear", align_corners=False)[0, 0].numpy()
    err = np.abs(_apply(t, 0, x, DST) - want).max()
    assert err <= 1e-12, err
    assert np.abs(_apply(t, 0, x, DST) - conform_ref.conform(x, (1, 1, 1), "resize", DST, DST)).max() <= 1e-12


@pytest.mark.parametrize("r,taps", [(2.0, 8), (3.0, 11), (96 / 33, 12), (4.0, 16)])
def test_band_of_the_antialiased_row(r, taps):
    """2 radius + 2 taps: 8 at r = 2, 12 near r = 3, 16 at r = 4; at r = 3 exactly the positions are whole voxels and one tap falls away."""
    n = 96
    assert taps <= 2 * conform_ref.gaussian(r)[1] + 2
    t = conform_tables([(n, 4, 4)], [(1, 1, 1)], [Resize((int(n / r), 4, 4))], (int(n / r), 4, 4))
    assert t.taps[0].tolist() == [taps, 1, 1] and t.weights.shape[2] == taps
    w = t.axis(0, 0, (int(n / r), 4, 4))[1].astype(np.float64)
    assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1).max() < taps * 2.0 ** -24


def test_sixteen_tap_refusal_names_sample_axis_and_factor():
    with pytest.raises(ValueError, match=r"sample 1, axis 2: .*factor 5 needs 17 taps"):
        conform_tables([(8, 8, 8), (8, 8, 100)], [(1, 1, 1), (1, 1, 1)], [Resize((8, 8, 20))], (8, 8, 20))
    conform_tables([(8, 8, 100)], [(1, 1, 1)], [Resize((8, 8, 20), antialias=False)], (8, 8, 20))      # two taps: any factor


@pytest.mark.parametrize("m,N,c", [(10, 10, 0), (10, 14, 2), (10, 15, 3), (10, 11, 1), (14, 10, -2), (15, 10, -3), (11, 10, -1), (1, 10, 5), (10, 1, -5)])
def test_crop_and_pad_offsets(m, N, c):
    assert conform_ref.front_pad(m, N) == c
    t = conform_tables([(m, 3, 3)], [(1, 1, 1)], [CropOrPad((N, 3, 3))], (N, 3, 3))
    start, w, inside = t.axis(0, 0, (N, 3, 3))
    assert t.geometry[0, 0].tolist() == [1.0, float(c)] and t.taps[0].tolist() == [1, 1, 1] and t.weights.shape[2] == 1
    for q in range(N):
        u = q - c
        assert bool(inside[q]) == (0 <= u < m)
        if inside[q]:
            assert start[q] == u and w[q, 0] == 1.0                        # one tap of weight exactly 1
    front = int(np.argmax(inside))                                         # rows in front of / behind the volume
    assert (front, N - front - int(inside.sum())) == ((math.ceil((N - m) / 2), (N - m) // 2) if N >= m else (0, 0))


def test_resample_intermediate_lengths():
    shapes, spacing = [(13, 22, 37), (1, 5, 3), (7, 9, 70)], [(1.0, 0.7, 0.6), (2.0, 1.0, 0.8), (1.5, 2.0, 0.34)]
    N = (10, 16, 24)
    t = conform_tables(shapes, spacing, [Resample(1.0), CropOrPad(N)], N, dtype=np.float64)
    for b in range(3):
        for a in range(3):
            r = 1.0 / spacing[b][a]
            m = max(1, math.floor(shapes[b][a] / r + 1e-9))
            assert conform_ref.lengths(shapes[b][a], spacing[b][a], "resample", 1.0) == (r, m)
            assert t.geometry[b, a].tolist() == [r, float(conform_ref.front_pad(m, N[a]))]
            assert int(t.axis(b, a, N)[2].sum()) == min(m, N[a])
    assert conform_ref.lengths(1, 2.0, "resample", 1.0) == (0.5, 2) and conform_ref.lengths(1, 0.25, "resample", 1.0) == (4.0, 1)
    assert conform_ref.lengths(30, 0.1, "resample", 1.0)[1] == 3          # 30 / 10 = 2.999.. in floating point: the 1e-9 guard
    for b in range(3):                                                     # the whole map against the plain loops
        x = _volume(shapes[b], 10 + b)
        want = conform_ref.conform(x, spacing[b], "resample", (1.0, 1.0, 1.0), N, pad=0.0)
        got = conform_ref.apply_tables(x, [t.axis(b, a, N) for a in range(3)], 0.0)
        assert np.abs(got - want).max() <= 1e-12
    anis = conform_tables(shapes[:1], spacing[:1], [Resample((2.0, 1.0, 0.5), antialias=False), CropOrPad(N)], N)
    assert anis.geometry[0, :, 0].tolist() == [2.0, 1.0 / 0.7, 0.5 / 0.6]


def test_tables_are_rounded_once_and_reads_stay_inside():
    shapes, spacing, N = [(13, 22, 37), (7, 9, 70)], [(1.0, 0.7, 0.6), (1.5, 2.0, 0.34)], (10, 16, 24)
    t64 = conform_tables(shapes, spacing, [Resample(1.0), CropOrPad(N)], N, dtype=np.float64)
    t32 = conform_tables(shapes, spacing, [Resample(1.0), CropOrPad(N)], N)
    assert t32.weights.dtype == np.float32 and np.array_equal(t32.weights, t64.weights.astype(np.float32))
    assert t32.weights.shape[2] == int(t32.taps.max()) == 12               # 0.34 -> 1.0: a factor of 2.94
    for b in range(2):
        for a in range(3):
            start, _, inside = t32.axis(b, a, N)
            assert (start[inside] >= 0).all() and (start[inside] + t32.taps[b, a] <= shapes[b][a]).all()


def test_plan_orders_the_passes_by_reduction():
    shapes, spacing, N = [(144, 384, 384), (10, 16, 24), (20, 16, 24)], [(0.7, 0.37, 0.37), (1, 1, 1), (0.5, 1, 1)], (10, 16, 24)
    t = conform_tables(shapes, spacing, [Resample(1.0), CropOrPad(N)], N)
    plan = ops.conform_plan(shapes, N, t.start, t.weights, t.inside, t.taps)
    assert plan["npass"] == 3 and plan["exact"].tolist() == [[False] * 3, [True] * 3, [False, True, True]]
    meta = plan["meta"]
    assert meta[:, 0, 12].tolist() == [1, 2, 0]                            # H and W shrink most (a tie goes to the lower axis), D last
    assert meta[0, 0, 6:12].tolist() == [144, 384, 384, 144, 16, 384] and meta[2, 0, 6:12].tolist() == [144, 16, 24, 10, 16, 24]
    assert meta[:, 1, 0].tolist() == [1, 0, 0] and meta[0, 1, 3:6].tolist() == [ops.CONFORM_GATHER] * 3 and meta[0, 1, 12] == -1
    assert meta[0, 2, 3:6].tolist() == [ops.CONFORM_CONTRACT, ops.CONFORM_GATHER, ops.CONFORM_GATHER] and meta[:, 2, 0].tolist() == [1, 0, 0]
    assert meta[:, :, 2].tolist() == [[0, 1, 1], [0, 0, 0], [1, 0, 0]]     # each sample's last pass writes the batch tensor
    assert plan["scratch"] == 144 * 16 * 384 + 144 * 16 * 24 and plan["dst_off"][2, 0] == 0 and plan["dst_off"][0, 2] == 2 * 10 * 16 * 24


def test_argument_errors():
    for bad in (lambda: CropOrPad((4, 4, 4), padding_mode="reflect"), lambda: CropOrPad((4, 4, 4), mask_name="brain"),
                lambda: Resize((4, 4, 4), image_interpolation="bspline"), lambda: Resample(1.0, image_interpolation="cubic"),
                lambda: Resample("t1.nii.gz"), lambda: Conform([CropOrPad(4), Resize(4)]), lambda: Conform([Resize(4), Resample(1.0)]),
                lambda: Conform([]), lambda: Conform([gdata.RandomFlip()])):
        with pytest.raises(NotImplementedError, match="built"):
            bad()
    for bad in (lambda: CropOrPad((4, 4)), lambda: CropOrPad((4, 0, 4)), lambda: Resample(0.0), lambda: Resample((1.0, -1.0, 1.0)),
                lambda: Conform([Resample(1.0)]), lambda: CropOrPad(4, padding_mode=float("nan")),
                lambda: conform_tables([(4, 4, 4)], [(1, 1, 1)], [CropOrPad(8)], (8, 8, 9)),
                lambda: conform_tables([(4, 4, 0)], [(1, 1, 1)], [CropOrPad(8)], (8, 8, 8)),
                lambda: conform_tables([(4, 4, 4)], [(1, 0, 1)], [CropOrPad(8)], (8, 8, 8))):
        with pytest.raises(ValueError):
            bad()
    assert Conform([Resize((4, 5, 6))]).target_shape == (4, 5, 6) and Conform([Resample(2), CropOrPad(7, "minimum")]).target_shape == (7, 7, 7)
    with pytest.raises(RuntimeError, match="GPU"):
        Conform([CropOrPad(4)])(collate_ragged([(np.zeros((3, 3, 3), np.float32), np.ones(3))]))
    with pytest.raises(lib.GavikoHipError, match="HIP device"):               # the ops wrappers refuse host tensors before any table is read
        ops.ragged_minmax(torch.zeros(8), [0], [(2, 2, 2)])
    with pytest.raises(lib.GavikoHipError, match="HIP device"):
        ops.conform_volumes(torch.zeros(8), [0], [(2, 2, 2)], np.zeros((1, 6), np.int32), np.ones((1, 6, 1), np.float32), np.ones((1, 6), bool),
                            np.ones((1, 3), np.int32), (2, 2, 2))


class _Ragged(Dataset):
    SHAPES = [(3, 4, 5), (2, 2, 7), (4, 1, 3), (1, 1, 1), (5, 3, 2)]

    def __init__(self, labels=True):
        self.labels = labels

    def __len__(self):
        return len(self.SHAPES)

    def __getitem__(self, i):
        vol = torch.arange(int(np.prod(self.SHAPES[i])), dtype=torch.float32).view(1, *self.SHAPES[i]) + 100.0 * i
        spacing = torch.tensor([1.0 + i, 0.5, 0.25 * (i + 1)], dtype=torch.float64)
        return (vol, spacing, i % 3) if self.labels else (vol, spacing)


def test_collate_ragged_and_pin_memory_through_a_dataloader():
    for labels in (True, False):
        ds = _Ragged(labels)
        loader = DataLoader(ds, batch_size=3, shuffle=False, num_workers=2, pin_memory=True, collate_fn=collate_ragged)
        seen = 0
        for batch in loader:
            rb, y = batch if labels else (batch, None)
            assert isinstance(rb, RaggedBatch) and len(rb) == rb.shapes.shape[0] and len(rb) in (3, 2)
            assert rb.data.dtype == torch.float32 and rb.offsets.dtype == torch.int64 and rb.shapes.dtype == torch.int32 and rb.spacing.dtype == torch.float64
            assert rb.offsets.shape == (len(rb) + 1,) and (rb.offsets[:-1] % gdata.RAGGED_ALIGN == 0).all() and int(rb.offsets[-1]) == rb.data.numel()
            for b in range(len(rb)):
                vol, spacing = ds[seen + b][0], ds[seen + b][1]
                assert torch.equal(rb.volume(b), vol[0]) and torch.equal(rb.spacing[b], spacing)
            if labels:
                assert y.tolist() == [(seen + b) % 3 for b in range(len(rb))]
            if torch.cuda.is_available():
                assert rb.data.is_pinned() and rb.pin_memory().data.is_pinned()
            moved = rb.to("cpu")
            assert isinstance(moved, RaggedBatch) and moved.shapes is rb.shapes and moved.spacing is rb.spacing
            seen += len(rb)
        assert seen == len(ds)
    one = collate_ragged([(np.ones((2, 3, 4), np.float32), (1.0, 2.0, 3.0))])         # (D, H, W) arrays and plain tuples as well
    assert len(one) == 1 and one.shapes.tolist() == [[2, 3, 4]] and one.spacing.tolist() == [[1.0, 2.0, 3.0]]
    with pytest.raises(ValueError):
        collate_ragged([(np.ones((2, 3), np.float32), (1.0, 1.0, 1.0))])


def test_volume_dataset_reads_shape_and_spacing(tmp_path):
    import pandas as pd
    rng = np.random.default_rng(0)
    vols = [rng.normal(size=s).astype(np.float32) for s in ((3, 4, 5), (2, 6, 3))]
    np.savez(tmp_path / "a.npz", data=vols[0], spacing=np.array([0.7, 0.37, 0.37]))
    np.savez(tmp_path / "b.npz", data=vols[1])
    df = pd.DataFrame(dict(mri_path=["a.npz", "b.npz"], kl_grade=[2, 4], subset=["train", "train"]))
    ds = gdata.VolumeDataset(df, image_folder=str(tmp_path))
    v, s, y = ds[0]
    assert v.shape == (1, 3, 4, 5) and v.dtype == torch.float32 and s.tolist() == [0.7, 0.37, 0.37] and y == 2
    assert ds[1][1].tolist() == [1.0, 1.0, 1.0] and len(ds) == 2
    assert len(gdata.VolumeDatasetPrediction(df, image_folder=str(tmp_path))[1]) == 2
    rb, labels = collate_ragged([ds[0], ds[1]])
    assert torch.equal(rb.volume(1), torch.from_numpy(vols[1])) and labels.tolist() == [2, 4]


def test_data_preprocessor_without_conform_is_unchanged(tmp_path):
    import pandas as pd
    np.savez(tmp_path / "a.npz", data=np.zeros((4, 4, 4), np.float32))
    pd.DataFrame(dict(mri_path=["a.npz"] * 3, kl_grade=[0, 1, 2], subset=["train", "val", "test"])).to_csv(tmp_path / "d.csv", index=False)
    cfg = dict(data=dict(data_path=str(tmp_path / "d.csv"), image_folder=str(tmp_path), batch_size=1, num_workers=0))
    pre = gdata.DataPreprocessor(cfg, seed=3)
    assert pre.conform is None and pre.batch_mix is None
    loaders = pre.preprocess()
    assert all(type(d) is gdata.CustomDataset for d in loaders[3:]) and all(l.collate_fn is not collate_ragged for l in loaders[:3])
    x, y = next(iter(loaders[0]))
    assert x.shape == (1, 1, 4, 4, 4) and y.tolist() == [0]
    same = gdata.train_transforms(3)                                       # the random stream is the one a plain compose draws
    assert pre.train_transforms.rng.random(4).tolist() == same.rng.random(4).tolist()
    cfg["data"]["conform"] = dict(target_shape=(6, 6, 6), spacing=1.0, padding_mode="minimum", antialias=False)
    pre = gdata.DataPreprocessor(cfg, seed=3)
    assert isinstance(pre.conform, Conform) and pre.conform.target_shape == (6, 6, 6) and pre.conform.crop.padding_mode == "minimum"
    assert isinstance(pre.conform.resample, Resample) and not pre.conform.resample.antialias
    loaders = pre.preprocess()
    assert all(type(d) is gdata.VolumeDataset for d in loaders[3:])
    rb, y = next(iter(loaders[1]))
    assert isinstance(rb, RaggedBatch) and rb.shapes.tolist() == [[4, 4, 4]] and y.tolist() == [1]
    assert isinstance(gdata.conform_from_config(dict(target_shape=5, resize=(5, 6, 7))).resample, Resize)
    with pytest.raises(ValueError):
        gdata.conform_from_config(dict(target_shape=5, resize=5, spacing=1.0))
    with pytest.raises(ValueError):
        gdata.conform_from_config(dict(spacing=1.0))
