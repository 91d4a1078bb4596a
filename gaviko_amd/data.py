"""Data side of train.py:33-78 / data/dataset.py with the transforms on the device.

The reference reads one `.npz['data']` (120,160,160) per sample, adds the channel axis and runs torchio transforms on the CPU in the
DataLoader workers (train: RandomAffine(degrees=15, p=.5) + RandomFlip(axes=(0), p=.5), then RescaleIntensity((0,1)); val/test:
RescaleIntensity only).  Here the datasets return the RAW volume (the npz read stays on the host, in workers, into pinned memory)
and the transforms run on the whole batch once it is in HBM, as three HBM-bound kernels (`csrc/augment.hip`):

    x = batch.to(device, non_blocking=True)          # [B, 1, D, H, W] raw
    x = pre.train_transforms(x)                      # affine + flip in one resampling pass, then min/max + rescale

torchio 0.20.16 (requirements.txt:6) and its SimpleITK backend are not installed here, so:
* RescaleIntensity and RandomFlip follow torchio's published arithmetic exactly (float32 steps in the same order; exact gathers);
* RandomAffine keeps torchio's parameterisation (per-axis scale ~ U(1-s, 1+s) with s = 0.1 by default, per-axis angle ~ U(-d, d),
  rotation about the image centre, linear interpolation, padding with the volume minimum) but its axis/sign conventions are this
  module's own (rotation R = R2.R1.R0 about the array axes), not SimpleITK's LPS ones: same augmentation distribution up to
  axis naming, not the same voxels for the same seed.  Parity vs torchio is UNPINNED; the kernels are pinned against
  `oracle/data_ref.py` (numpy) and scipy.ndimage.affine_transform.

The intensity group train.py:43-48 declares (RandomNoise, RandomBiasField, RandomBlur, RandomMotion; its OneOf line is commented out in
the shipped script) is built too: `train_transforms(intensity=True)` puts `OneOf` of the first three (two kernels, `csrc/intensity.hip`)
between the spatial pass and RescaleIntensity, `motion=True` makes it the reference's four-member dict.  RandomMotion (k-space
compositing of rigidly moved copies) is one fused kernel (`csrc/motion.hip`) and needs no FFT: torchio's slabs lie along the last array
axis only, so a real circular convolution along W per moved image is all that is left (`motion_tables`).  The parameter
sampling is torchio's; the noise field comes from this package's counter hash, not torch's generator, the bias-field axes are the
array axes, and RandomMotion's movements use this module's RandomAffine conventions, translate in voxels (the reference's arrays have
spacing 1) and are not demeaned: same distributions, not the same voxels for the same seed.  Parity vs torchio is UNPINNED here as well;
the kernels are pinned against scipy.ndimage.gaussian_filter, a numpy restatement (`tests/intensity_ref.py`) and torchio's compositing
written literally with np.fft (`tests/motion_ref.py`).

RandomElasticDeformation (not in the reference's Compose; torchio's documented companion of RandomAffine, `train_transforms(elastic=True)`)
is one more resampling kernel (`csrc/elastic.hip`): ITK's order-3 B-spline transform over the image extent, evaluated separably, and the
trilinear read of the affine pass.  It keeps torchio's signature, sampling and errors; its axes are the array axes, displacements are in
voxels, the locked borders are zeroed on all three axes, and inside DeviceCompose it always runs before the affine/flip pass: same
distributions, not the same voxels for the same seed.  Parity vs torchio / SimpleITK is UNPINNED; the kernel is pinned against a float64
restatement (`tests/elastic_ref.py`) that is itself checked against scipy.ndimage.map_coordinates.

The last step of every batch is a normaliser.  The reference's is the plain RescaleIntensity((0, 1)) (two kernels of `csrc/augment.hip`,
kept bit for bit as the default); torchio's three MRI normalisers -- RescaleIntensity with percentiles and a mask, ZNormalization
(`normalization='percentile'` / `'znorm'`) and HistogramStandardization (an instance, alone or in a list before one of the strings) -- run on exact per-volume order statistics and float64 moments computed on the device without a
sort or a host read (`csrc/normalize.hip`).  Empty masks and zero ranges become a per-sample status word (`DeviceCompose.last_norm_status`)
where torchio warns or raises; cutoffs are rounded to float32 before the clip.  Parity vs torchio is UNPINNED; the kernels are pinned against
np.sort / np.percentile / math.fsum (`tests/normalize_ref.py`).  HistogramStandardization maps 11 landmarks (percentiles of the masked voxels, found
in four sweeps whatever their number: `ops.volume_landmarks`) onto landmarks that `HistogramStandardization.train` learns on the device from the
training batches; it keeps torchio's arithmetic (`tests/histstd_ref.py`), with float32 landmarks, the array-axis mask rules only, and the map
evaluated in float64 and rounded once; an empty mask is a status word (`DeviceCompose.last_hist_status`).

The rest of torchio's MRI augmentation family (`train_transforms(intensity=True, artifacts=True)`, `csrc/kspace.hip`) joins the intensity
group: RandomGhosting reduces the way RandomMotion did, to a real circular convolution along the one axis its k-space mask depends on (any of
the three, drawn per sample, on the fp32 matrix cores); a RandomSpike is one cosine added in image space, its phase tabulated per axis on the
host; RandomGamma is a streaming power; RandomAnisotropy collapses to a two-tap gather along one axis.  They keep torchio's signatures, value
ranges and errors; ghosting restores exactly the centre plane (not a band of relative width `restore`), a spike's amplitude is g |mean(x)|
(torchio's g max|F| / V for a non-negative volume), anisotropy clamps at the edges where torchio pads.  Parity vs torchio is UNPINNED; the kernels
are pinned against the literal np.fft algorithms and float64 restatements (`tests/kspace_ref.py`).

`BatchMix` (not in the reference; timm.data.Mixup's arguments and arithmetic) is the one transform that combines two samples: Mixup and
CutMix of the normalised batch in one streaming launch (`csrc/batchmix.hip`), with the mixed target returned as the pair `MixedTarget` that
the fused losses take (`losses.py`, `gvk_loss_mixed_fwd_bwd`).  It has its own random stream, so DeviceCompose's is untouched; partners come
from a permutation, not timm's flipped batch.  The kernel is pinned against a float64 restatement (`tests/batchmix_ref.py`).

Everything above starts from a batch that is already on the model's grid; the reference's data set was resampled offline.  `Conform` is
torchio's first stage for scans that are not: `Resample` to a spacing or `Resize`, then `CropOrPad`, on a `RaggedBatch` of volumes of unequal
shape and spacing (`VolumeDataset`, `collate_ragged`), as up to three streaming passes over the packed buffer (`csrc/conform.hip`).  The classes
keep torchio's names and arguments; the geometry (edge-aligned positions, Cardoso et al.'s antialiasing sigma, centred crop / pad) is this
module's own definition, on the array axes and in the samples' own spacing units, with no orientation or affine handling.  Parity vs torchio /
SimpleITK is UNPINNED; the tables are pinned against F.interpolate and scipy.ndimage.gaussian_filter1d, the kernels against a float64
restatement (`tests/conform_ref.py`).
"""
from __future__ import annotations

import functools
import math
import os
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from . import ops


# ---- datasets: data/dataset.py:5-49 -------------------------------------------------------------------------------------------
class CustomDataset(Dataset):
    """dataset.py:5-28.  `transforms` (optional) is a host-side callable on the (1,D,H,W) array, as in the reference; leave it None to
    get the raw float32 volume and apply `DeviceCompose` to the batch on the GPU."""

    def __init__(self, dataframe, transforms=None, image_folder=None):
        self.df = dataframe
        self.transforms = transforms
        self.image_folder = image_folder

    def _path(self, index):
        p = self.df.loc[index]["mri_path"]
        return p if not self.image_folder else os.path.join(self.image_folder, p)

    def _volume(self, index):
        mri_object = np.load(self._path(index))["data"]
        mri_object = np.expand_dims(mri_object, 0)                       # (1 x 120 x 160 x 160)
        if self.transforms is not None:
            mri_object = self.transforms(mri_object)
        return torch.as_tensor(np.ascontiguousarray(mri_object, dtype=np.float32))

    def __getitem__(self, index):
        return self._volume(index), self.df.loc[index]["kl_grade"]

    def __len__(self):
        return len(self.df)


class CustomDatasetPrediction(CustomDataset):
    """dataset.py:30-49: no image_folder, no label."""

    def __init__(self, dataframe, transforms=None):
        super().__init__(dataframe, transforms, None)

    def __getitem__(self, index):
        return self._volume(index)


class VolumeDataset(Dataset):
    """The CSV columns of `CustomDataset`, for scans that are NOT on the model's grid yet: returns (volume, spacing, label) with the raw
    float32 volume (1, D, H, W) of whatever shape the file holds and spacing float64 [3] = npz[spacing_key] in array-axis order, (1, 1, 1)
    where the file has no such key.  Batches of it are built by `collate_ragged` and brought onto the grid by `Conform`."""

    def __init__(self, dataframe, image_folder=None, spacing_key: str = "spacing"):
        self.df, self.image_folder, self.spacing_key = dataframe, image_folder, spacing_key

    def _path(self, index):
        p = self.df.loc[index]["mri_path"]
        return p if not self.image_folder else os.path.join(self.image_folder, p)

    def _volume(self, index):
        with np.load(self._path(index)) as npz:
            vol = np.ascontiguousarray(npz["data"], dtype=np.float32)
            spacing = np.asarray(npz[self.spacing_key], dtype=np.float64).reshape(-1) if self.spacing_key in npz.files else np.ones(3)
        if vol.ndim != 3 or spacing.shape != (3,) or not (spacing > 0).all():
            raise ValueError(f"{self._path(index)}: a (D, H, W) volume and three positive spacings expected, got {vol.shape} and {spacing}")
        return torch.from_numpy(vol[None]), torch.from_numpy(spacing)

    def __getitem__(self, index):
        return (*self._volume(index), self.df.loc[index]["kl_grade"])

    def __len__(self):
        return len(self.df)


class VolumeDatasetPrediction(VolumeDataset):
    """`VolumeDataset` without the label: (volume, spacing)."""

    def __getitem__(self, index):
        return self._volume(index)


class RaggedBatch(NamedTuple):
    """A batch of volumes of unequal shape, packed: data float32 [total] holds every volume's voxels in [D][H][W] order one after another,
    sample b at elements offsets[b] .. offsets[b] + prod(shapes[b]); offsets int64 [B + 1], shapes int32 [B][3], spacing float64 [B][3] (array-axis
    order).  Only `data` ever goes to the device: offsets, shapes and spacing are what the host builds the tables of `Conform` from, and they
    stay where the host can read them without waiting for the GPU.  len() is B."""
    data: torch.Tensor
    offsets: torch.Tensor
    shapes: torch.Tensor
    spacing: torch.Tensor

    def __len__(self):
        return int(self.shapes.shape[0])

    def to(self, device, non_blocking: bool = False):
        return RaggedBatch(self.data.to(device, non_blocking=non_blocking), self.offsets, self.shapes, self.spacing)

    def pin_memory(self):
        return RaggedBatch(self.data.pin_memory(), self.offsets, self.shapes, self.spacing)

    def volume(self, b: int) -> torch.Tensor:
        """Sample b as a [D][H][W] view of the packed buffer."""
        o, s = int(self.offsets[b]), [int(v) for v in self.shapes[b]]
        return self.data[o:o + s[0] * s[1] * s[2]].view(*s)


RAGGED_ALIGN = 4          # collate_ragged starts every sample at a multiple of 4 elements (16 bytes); the kernels do not rely on it


def collate_ragged(samples):
    """`collate_fn` for `VolumeDataset`: samples (volume, spacing, label) -> (RaggedBatch, labels), samples (volume, spacing) -> RaggedBatch.
    A volume is (1, D, H, W) or (D, H, W), a tensor or an array."""
    vols = [torch.as_tensor(s[0], dtype=torch.float32) for s in samples]
    vols = [v[0] if v.dim() == 4 and v.shape[0] == 1 else v for v in vols]
    if any(v.dim() != 3 or v.numel() == 0 for v in vols):
        raise ValueError(f"collate_ragged: volumes are (1, D, H, W) or (D, H, W), got {[tuple(v.shape) for v in vols]}")
    offsets, end = [], 0
    for v in vols:
        offsets.append(-(-end // RAGGED_ALIGN) * RAGGED_ALIGN)
        end = offsets[-1] + v.numel()
    data = torch.zeros(end, dtype=torch.float32)
    for o, v in zip(offsets, vols):
        data[o:o + v.numel()] = v.reshape(-1)
    batch = RaggedBatch(data, torch.tensor(offsets + [end], dtype=torch.int64), torch.tensor([list(v.shape) for v in vols], dtype=torch.int32),
                        torch.stack([torch.as_tensor(s[1], dtype=torch.float64).reshape(3) for s in samples]))
    if len(samples[0]) == 2:
        return batch
    return batch, torch.as_tensor(np.asarray([s[2] for s in samples]))


# ---- device transforms ----------------------------------------------------------------------------------------------------------
def _pair(v, name):
    if isinstance(v, (int, float)):
        return (-float(v), float(v))
    v = tuple(float(t) for t in v)
    if len(v) != 2:
        raise ValueError(f"{name}: a number or a (low, high) pair")
    return v


class RandomFlip:
    """tio.RandomFlip(axes, flip_probability): every listed spatial axis is mirrored independently with that probability."""

    def __init__(self, axes=0, flip_probability: float = 0.5):
        axes = (axes,) if isinstance(axes, int) else tuple(axes)
        if any(a not in (0, 1, 2) for a in axes):
            raise ValueError("RandomFlip: axes are spatial axes 0, 1, 2")
        self.axes, self.p = axes, float(flip_probability)

    def sample(self, rng: np.random.Generator) -> int:
        bits = 0
        for a in self.axes:
            if rng.random() < self.p:
                bits |= 1 << a
        return bits


class RandomAffine:
    """tio.RandomAffine(scales=0.1, degrees=10, translation=0, isotropic=False, center='image', default_pad_value='minimum',
    image_interpolation='linear', p=1) -- the subset train.py:40 uses, torchio's parameter sampling."""

    def __init__(self, scales=0.1, degrees=10, translation=0, isotropic: bool = False, center: str = "image", default_pad_value="minimum",
                 image_interpolation: str = "linear", p: float = 1.0):
        if center != "image" or default_pad_value != "minimum" or image_interpolation != "linear":
            raise NotImplementedError("RandomAffine: only center='image', default_pad_value='minimum', image_interpolation='linear' are built")
        self.scales = (1.0 - float(scales), 1.0 + float(scales)) if isinstance(scales, (int, float)) else tuple(float(s) for s in scales)
        self.degrees, self.translation = _pair(degrees, "degrees"), _pair(translation, "translation")
        self.isotropic, self.p = bool(isotropic), float(p)

    def sample(self, rng: np.random.Generator):
        """None (not applied) or (scales[3], degrees[3], translation[3])."""
        if rng.random() >= self.p:
            return None
        s = rng.uniform(self.scales[0], self.scales[1], 3)
        if self.isotropic:
            s[:] = s[0]
        return s, rng.uniform(self.degrees[0], self.degrees[1], 3), rng.uniform(self.translation[0], self.translation[1], 3)


def affine_matrix(scales, degrees, translation, shape) -> np.ndarray:
    """3x4 map from an OUTPUT voxel q to the input position p = A q + t for the forward transform T(p) = c + R S (p - c) + tr about the
    image centre c, R = R2 R1 R0 (Rk: rotation by degrees[k] about array axis k), S = diag(scales): A = S^-1 R^T, t = c - A (c + tr)."""
    a = np.radians(np.asarray(degrees, dtype=np.float64))
    c0, s0, c1, s1, c2, s2 = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    r0 = np.array([[1, 0, 0], [0, c0, -s0], [0, s0, c0]])
    r1 = np.array([[c1, 0, s1], [0, 1, 0], [-s1, 0, c1]])
    r2 = np.array([[c2, -s2, 0], [s2, c2, 0], [0, 0, 1]])
    A = np.diag(1.0 / np.asarray(scales, dtype=np.float64)) @ (r2 @ r1 @ r0).T
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    t = c - A @ (c + np.asarray(translation, dtype=np.float64))
    return np.concatenate([A, t[:, None]], axis=1)


def _triple(v, name, kind):
    if isinstance(v, (int, float)):
        return (kind(v),) * 3
    v = tuple(kind(t) for t in v)
    if len(v) != 3:
        raise ValueError(f"{name}: a number or one value per array axis")
    return v


class RandomElasticDeformation:
    """tio.RandomElasticDeformation(num_control_points=7, max_displacement=7.5, locked_borders=2, image_interpolation='linear', p=1): a
    random displacement on a coarse grid of control points, interpolated with cubic B-splines (`csrc/elastic.hip`).  num_control_points and
    max_displacement are a number or one value per array axis; displacements are in voxels (the reference's arrays have spacing 1).
    locked_borders = 1 zeroes the outermost layer of control points on every axis, 2 the outer two layers.  Draws: one uniform for p, then
    n0 n1 n2 3 uniforms in grid order, u -> (u - 0.5) 2 max_a for component a."""

    def __init__(self, num_control_points=7, max_displacement=7.5, locked_borders: int = 2, image_interpolation: str = "linear", p: float = 1.0):
        self.num_control_points = _triple(num_control_points, "num_control_points", int)
        self.max_displacement = _triple(max_displacement, "max_displacement", float)
        if any(n < 4 for n in self.num_control_points):
            raise ValueError(f"RandomElasticDeformation: at least 4 control points per axis (cubic B-splines), not {self.num_control_points}")
        if any(m < 0 for m in self.max_displacement):
            raise ValueError("RandomElasticDeformation: max_displacement is non-negative")
        if locked_borders not in (0, 1, 2):
            raise ValueError("RandomElasticDeformation: locked_borders is 0, 1 or 2")
        if locked_borders == 2 and 4 in self.num_control_points:
            raise ValueError("RandomElasticDeformation: locked_borders = 2 with 4 control points on an axis zeroes them all (an identity transform); "
                             "use more control points or locked_borders 0 or 1")
        if image_interpolation != "linear":
            raise NotImplementedError("RandomElasticDeformation: only image_interpolation='linear' is built")
        if any(n > ops.ELASTIC_MAX_CONTROL_POINTS for n in self.num_control_points):
            raise NotImplementedError(f"RandomElasticDeformation: 4..{ops.ELASTIC_MAX_CONTROL_POINTS} control points per axis are built")
        self.locked_borders, self.p = int(locked_borders), float(p)
        self._checked_shape = None

    def check_folding(self, shape) -> None:
        """torchio's folding warning, once the shape is known (DeviceCompose calls this on its first batch): a displacement of half a mesh
        cell h_a = S_a / (n_a - 3) or more can fold the volume over itself."""
        if self._checked_shape is not None:
            return
        self._checked_shape = tuple(shape)
        spacing = [S / (n - 3) for S, n in zip(shape, self.num_control_points)]
        if any(m >= h / 2 for m, h in zip(self.max_displacement, spacing)):
            import warnings
            warnings.warn(f"RandomElasticDeformation: max_displacement {self.max_displacement} is not below half the control-point spacing "
                          f"{tuple(round(h, 4) for h in spacing)} on every axis (volume {tuple(shape)}, {self.num_control_points} control points): "
                          "the deformation may fold the volume", RuntimeWarning, stacklevel=2)

    def sample(self, rng: np.random.Generator):
        """None (not applied) or the coarse field float64 [n0][n1][n2][3], locked borders already zero."""
        if rng.random() >= self.p:
            return None
        coarse = (rng.random(self.num_control_points + (3,)) - 0.5) * 2.0 * np.asarray(self.max_displacement, dtype=np.float64)
        for i in range(self.locked_borders):
            for a in range(3):
                layers = np.moveaxis(coarse, a, 0)                          # a view
                layers[i], layers[-1 - i] = 0.0, 0.0
        return coarse


SPATIAL_ONE_OF_MEMBERS = (RandomAffine, RandomElasticDeformation)


def _masking_method(m, name):
    """None, 'mean' or a float threshold: the mask rules `ops.volume_stats` knows."""
    if m is None or (isinstance(m, str) and m == "mean"):
        return m
    if isinstance(m, (int, float)) and not isinstance(m, bool):
        return float(m)
    raise NotImplementedError(f"{name}: masking_method is None, 'mean' or a number (voxels above it); {m!r} (callables, label names) is not built")


class RescaleIntensity:
    """tio.RescaleIntensity(out_min_max, percentiles, masking_method): the volume is clipped to the two percentiles of its masked voxels and
    the clipped range goes to [out_min, out_max].  The defaults (percentiles (0, 100), no mask) are the plain per-volume min-max and keep its
    two kernels; anything else runs the exact order statistics of `csrc/normalize.hip`."""

    def __init__(self, out_min_max=(0, 1), percentiles=(0, 100), masking_method=None):
        self.out_min, self.out_max = float(out_min_max[0]), float(out_min_max[1])
        percentiles = tuple(float(p) for p in percentiles)
        if len(percentiles) != 2 or not 0.0 <= percentiles[0] <= percentiles[1] <= 100.0:
            raise ValueError(f"RescaleIntensity: percentiles are (low, high) with 0 <= low <= high <= 100, not {percentiles}")
        self.percentiles = percentiles
        self.masking_method = _masking_method(masking_method, "RescaleIntensity")

    @property
    def plain(self) -> bool:
        """True for the min-max rescale this package had first (its own two kernels, its own bits)."""
        return self.percentiles == (0.0, 100.0) and self.masking_method is None

    def apply(self, x: torch.Tensor, partials: torch.Tensor):
        """(y, status) for the batch x: status is None on the plain path (min/max into the scratch `partials` of `ops.minmax_partials`),
        otherwise the int32 [B] device words of `ops.normalize_intensity`."""
        y = torch.empty_like(x)
        if self.plain:
            ops.volume_minmax(x, partials)
            ops.rescale_intensity(x, partials, y, self.out_min, self.out_max)
            return y, None
        stats, _ = ops.volume_stats(x, self.masking_method, want_std=False)
        _, cutoffs = ops.volume_order_stats(x, stats, self.percentiles)
        return y, ops.normalize_intensity(x, y, stats, ops.NORMALIZE_RESCALE, cutoffs, self.out_min, self.out_max)


class ZNormalization:
    """tio.ZNormalization(masking_method): y = (x - mean) / std with the mean and the unbiased standard deviation of the masked voxels.
    `ZNormalization.mean` is torchio's name for the rule 'voxels above the volume mean'."""

    mean = "mean"

    def __init__(self, masking_method=None):
        self.masking_method = _masking_method(masking_method, "ZNormalization")

    def apply(self, x: torch.Tensor, partials: torch.Tensor = None):
        """(y, status) for the batch x, as `RescaleIntensity.apply`; `partials` is not used."""
        stats, _ = ops.volume_stats(x, self.masking_method, want_std=True)
        y = torch.empty_like(x)
        return y, ops.normalize_intensity(x, y, stats, ops.NORMALIZE_ZNORM)


# ---- tio.HistogramStandardization (Nyul & Udupa): torchio's arithmetic on this package's order statistics -------------------------------
DEFAULT_CUTOFF = (0.01, 0.99)
LANDMARK_APPLY_INDEX = (0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12)      # of the 13 trained percentiles, the 11 the map uses (the quartiles 25 / 75 are left out)


def landmark_percentiles(cutoff=DEFAULT_CUTOFF) -> np.ndarray:
    """torchio's _standardize_cutoff and _get_percentiles: the sorted set of the two cutoffs (in percent, the low one clamped to [0, 9], the
    high one to [91, 100]), the quartiles and the deciles -- always 13 distinct values, float64."""
    if len(cutoff) != 2:
        raise ValueError(f"HistogramStandardization: cutoff is (low, high) as fractions, not {cutoff!r}")
    c = np.asarray([float(cutoff[0]), float(cutoff[1])], dtype=np.float64)
    c[0] = max(0.0, c[0])
    c[1] = min(1.0, c[1])
    c[0] = min(c[0], 0.09)
    c[1] = max(c[1], 0.91)
    every = (100 * c).tolist() + np.arange(25, 100, 25).tolist() + np.arange(10, 100, 10).tolist()
    return np.array(sorted(set(every)), dtype=np.float64)


def average_mapping(database) -> np.ndarray:
    """torchio's _get_average_mapping on a database [N][13] of per-volume landmarks, float64: every volume's (first, last) landmark is
    taken to (0, 100), and the 13 trained landmarks are the mean of the volumes' landmarks on that scale."""
    database = np.asarray(database, dtype=np.float64)
    if database.ndim != 2 or database.shape[0] < 1:
        raise ValueError(f"average_mapping: a database [N >= 1][landmarks], not shape {database.shape}")
    pc1, pc2 = database[:, 0], database[:, -1]
    s1, s2 = 0.0, 100.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        slopes = np.nan_to_num((s2 - s1) / (pc2 - pc1))
        intercepts = np.mean(s1 - slopes * pc1)
        return slopes.dot(database) / len(database) + intercepts


def landmark_database(batches, masking_method=None, cutoff=None):
    """The training database of `HistogramStandardization.train`: (float64 [N][13], skipped).  Per batch one `ops.volume_stats` and one
    `ops.volume_landmarks` launch at 13 percentiles; the rows stay on the device and come to the host in one copy at the end.  A volume whose
    mask is empty has no landmarks: it is left out and counted in `skipped`."""
    rule = _masking_method(masking_method, "HistogramStandardization.train")
    q = landmark_percentiles(cutoff or DEFAULT_CUTOFF)
    rows = []
    for batch in batches:
        x = batch[0] if isinstance(batch, (tuple, list)) else batch
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("HistogramStandardization.train: the batches are device tensors [B, 1, D, H, W] or (tensor, labels) pairs "
                               "(there is no CPU path)")
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        stats, count = ops.volume_stats(x, rule, want_std=False)
        _, cutoffs = ops.volume_landmarks(x, stats, q)
        rows.append(torch.cat([cutoffs.double(), count.double().unsqueeze(1)], dim=1))          # float32 and counts below 2^31: exact
    if not rows:
        raise ValueError("HistogramStandardization.train: no batches")
    table = torch.cat(rows).cpu().numpy()                                                       # the one copy to the host
    keep = table[:, -1] > 0
    return np.ascontiguousarray(table[keep, :-1]), int((~keep).sum())


class HistogramStandardization:
    """tio.HistogramStandardization(landmarks, masking_method): a piecewise-linear map that takes the volume's own histogram landmarks (the
    percentiles `landmark_percentiles(cutoff)` of its masked voxels, 11 of the 13) onto landmarks trained once on the training set
    (`HistogramStandardization.train`).  `landmarks` is the 13 trained values or a path np.load reads.  The mask only selects the voxels the
    percentiles come from; every voxel is mapped.  torchio's recipe follows it with ZNormalization(masking_method=ZNormalization.mean).
    The landmarks are the float32 cutoffs of `ops.volume_order_stats`; the map is evaluated in float64 and rounded to float32 once."""

    last_train_skipped = 0                                        # volumes the last `train` left out because their mask was empty

    def __init__(self, landmarks, masking_method=None, cutoff=DEFAULT_CUTOFF, epsilon: float = 1e-5):
        if isinstance(landmarks, (str, os.PathLike)):
            landmarks = np.load(landmarks)
        m = np.asarray(landmarks, dtype=np.float64)
        self.percentiles = landmark_percentiles(cutoff or DEFAULT_CUTOFF)
        if m.shape != (len(self.percentiles),) or not np.all(np.isfinite(m)) or np.any(np.diff(m) < 0):
            raise ValueError(f"HistogramStandardization: landmarks are {len(self.percentiles)} finite values that do not decrease, got {landmarks!r}")
        if not float(epsilon) >= 0.0:
            raise ValueError(f"HistogramStandardization: epsilon is not negative, got {epsilon!r}")
        self.landmarks = m
        self.cutoff = tuple(self.percentiles[[0, -1]] / 100)
        self.epsilon = float(epsilon)
        self.masking_method = _masking_method(masking_method, "HistogramStandardization")

    def apply(self, x: torch.Tensor, partials: torch.Tensor = None):
        """(y, status) for the batch x, as `RescaleIntensity.apply`; `partials` is not used.  status int32 [B]: 0 standardised, 1 empty mask
        (the sample comes back unchanged)."""
        idx = list(LANDMARK_APPLY_INDEX)
        stats, _ = ops.volume_stats(x, self.masking_method, want_std=False)
        _, cutoffs = ops.volume_landmarks(x, stats, self.percentiles[idx])
        y = torch.empty_like(x)
        return y, ops.histogram_standardize(x, y, stats, cutoffs, self.landmarks[idx], self.epsilon)

    @classmethod
    def train(cls, batches, masking_method=None, cutoff=None, output_path=None) -> np.ndarray:
        """torchio's HistogramStandardization.train on the device: `batches` is any iterable of device tensors [B, 1, D, H, W] or
        (tensor, labels) pairs (a loader composed with `.to(device)` or `Conform`).  Returns the 13 trained landmarks, float64, and saves
        them as .npy when output_path is given.  Volumes with an empty mask are left out; their number is `cls.last_train_skipped`."""
        database, skipped = landmark_database(batches, masking_method, cutoff)
        cls.last_train_skipped = skipped
        if skipped:
            import warnings
            warnings.warn(f"HistogramStandardization.train: {skipped} volume(s) with an empty mask were left out of the landmark database")
        if len(database) == 0:
            raise ValueError("HistogramStandardization.train: every volume had an empty mask")
        landmarks = average_mapping(database)
        if output_path is not None:
            np.save(output_path, landmarks)
        return landmarks


# ---- intensity transforms: train.py:43-48 --------------------------------------------------------------------------------------------
# Each `sample(rng)` returns None (not applied) or (class name, params) and draws, in this order: one uniform for p, then the
# parameters as listed in its docstring.  Parity with torchio itself is unpinned (module docstring).
class RandomNoise:
    """tio.RandomNoise(mean=0, std=(0, 0.25), p=1): y = x + N(mean, std).  A scalar mean m means mean ~ U(-m, m), a scalar std d means
    std ~ U(0, d).  Draws: mean, std, a 64-bit seed of the counter-hash noise field (`csrc/intensity.hip`)."""

    def __init__(self, mean=0, std=(0, 0.25), p: float = 1.0):
        self.mean = _pair(mean, "mean")
        self.std = (0.0, float(std)) if isinstance(std, (int, float)) else _pair(std, "std")
        if self.std[0] < 0 or self.std[1] < self.std[0]:
            raise ValueError("RandomNoise: std is a non-negative number or a (low, high) pair with 0 <= low <= high")
        self.p = float(p)

    def sample(self, rng: np.random.Generator):
        if rng.random() >= self.p:
            return None
        mean, std = rng.uniform(*self.mean), rng.uniform(*self.std)
        return "RandomNoise", dict(mean=float(mean), std=float(std), seed=int(rng.integers(0, 2 ** 64, dtype=np.uint64)))


def bias_terms(order: int):
    """Exponents (a, b, c) of the bias-field polynomial in coefficient order: torchio's nested loops over x, y, z orders, which are array
    axes 0, 1, 2 here."""
    return [(a, b, c) for a in range(order + 1) for b in range(order + 1 - a) for c in range(order + 1 - a - b)]


class RandomBiasField:
    """tio.RandomBiasField(coefficients=0.5, order=3, p=1): y = x * exp(P), P a polynomial of total degree <= order in the three array
    coordinates normalised to [-1, 1].  Draws: one coefficient ~ U(-c, c) per term of `bias_terms(order)`, in that order."""

    def __init__(self, coefficients=0.5, order: int = 3, p: float = 1.0):
        if not 0 <= int(order) <= 3:
            raise NotImplementedError("RandomBiasField: polynomial orders 0..3 are built")
        self.coefficients, self.order, self.p = _pair(coefficients, "coefficients"), int(order), float(p)

    def sample(self, rng: np.random.Generator):
        if rng.random() >= self.p:
            return None
        return "RandomBiasField", dict(coefficients=rng.uniform(self.coefficients[0], self.coefficients[1], len(bias_terms(self.order))), order=self.order)


class RandomBlur:
    """tio.RandomBlur(std=(0, 2), p=1): scipy.ndimage.gaussian_filter with one sigma ~ U(low, high) per array axis (spacing 1).  A scalar
    std d means U(0, d).  Draws: the three sigmas.  sigma above 4 (kernel radius above 16) is not built."""

    def __init__(self, std=(0, 2), p: float = 1.0):
        self.std = (0.0, float(std)) if isinstance(std, (int, float)) else _pair(std, "std")
        if self.std[0] < 0 or self.std[1] < self.std[0]:
            raise ValueError("RandomBlur: std is a non-negative number or a (low, high) pair with 0 <= low <= high")
        if int(4.0 * self.std[1] + 0.5) > ops.BLUR_MAX_RADIUS:
            raise NotImplementedError("RandomBlur: sigma above 4 (kernel radius above 16) is not built")
        self.p = float(p)

    def sample(self, rng: np.random.Generator):
        if rng.random() >= self.p:
            return None
        return "RandomBlur", dict(std=rng.uniform(self.std[0], self.std[1], 3))


class RandomMotion:
    """tio.RandomMotion(degrees=10, translation=10, num_transforms=2, image_interpolation='linear', p=1): k-space compositing of the volume
    with num_transforms rigidly moved copies (`motion_tables`, `csrc/motion.hip`).  Draws: degrees [K][3], translation [K][3] (voxels: the
    reference's arrays have spacing 1), then K perturbations ~ U(-0.3 step, 0.3 step) of the times step (1..K), step = 1 / (K + 1).  The
    movements follow `affine_matrix` (this module's axis conventions, about the image centre) and are not demeaned."""

    def __init__(self, degrees=10, translation=10, num_transforms: int = 2, image_interpolation: str = "linear", p: float = 1.0):
        if image_interpolation != "linear":
            raise NotImplementedError("RandomMotion: only image_interpolation='linear' is built")
        if not 1 <= int(num_transforms) <= ops.MOTION_MAX_TRANSFORMS:
            raise NotImplementedError(f"RandomMotion: num_transforms 1..{ops.MOTION_MAX_TRANSFORMS} are built")
        self.degrees, self.translation = _pair(degrees, "degrees"), _pair(translation, "translation")
        self.num_transforms, self.p = int(num_transforms), float(p)

    def sample(self, rng: np.random.Generator):
        if rng.random() >= self.p:
            return None
        K = self.num_transforms
        degrees = rng.uniform(self.degrees[0], self.degrees[1], (K, 3))
        translation = rng.uniform(self.translation[0], self.translation[1], (K, 3))
        step = 1.0 / (K + 1)
        times = step * np.arange(1, K + 1) + rng.uniform(-0.3 * step, 0.3 * step, K)
        return "RandomMotion", dict(degrees=degrees, translation=translation, times=times)


def _axes(axes, name):
    axes = (axes,) if isinstance(axes, int) else tuple(axes)
    if not axes or any(not isinstance(a, (int, np.integer)) or isinstance(a, bool) or a not in (0, 1, 2) for a in axes):
        raise ValueError(f"{name}: axes are array axes 0, 1, 2 (anatomical labels are not built), not {axes!r}")
    return tuple(int(a) for a in axes)


class RandomGhosting:
    """tio.RandomGhosting(num_ghosts=(4, 10), axes=(0, 1, 2), intensity=(0.5, 1), restore=0.02, p=1): every n-th plane of the shifted spectrum
    along one axis is scaled by 1 - g and the centre plane N // 2 is put back (`ghosting_tables`, `csrc/kspace.hip`).  A scalar num_ghosts n
    means U{0..n}, a scalar intensity d means U(0, d).  Draws: n, an integer uniform on [low, high] inclusive; the axis, uniform over axes; g.
    n == 0 or g == 0 is the identity.  restore is accepted and validated for signature compatibility only: exactly the centre plane is
    restored, where torchio restores a band of that relative width."""

    def __init__(self, num_ghosts=(4, 10), axes=(0, 1, 2), intensity=(0.5, 1), restore: float = 0.02, p: float = 1.0):
        ng = tuple(num_ghosts) if isinstance(num_ghosts, (tuple, list)) else (0, num_ghosts)
        if len(ng) != 2 or any(not isinstance(v, (int, np.integer)) or isinstance(v, bool) for v in ng) or not 0 <= ng[0] <= ng[1]:
            raise ValueError(f"RandomGhosting: num_ghosts is a non-negative integer or a (low, high) pair of them with low <= high, not {num_ghosts!r}")
        self.num_ghosts = (int(ng[0]), int(ng[1]))
        self.axes = _axes(axes, "RandomGhosting")
        self.intensity = (0.0, float(intensity)) if isinstance(intensity, (int, float)) else _pair(intensity, "intensity")
        if self.intensity[0] < 0 or self.intensity[1] < self.intensity[0]:
            raise ValueError("RandomGhosting: intensity is a non-negative number or a (low, high) pair with 0 <= low <= high")
        if not 0.0 <= float(restore) <= 1.0:
            raise ValueError(f"RandomGhosting: restore is in [0, 1], not {restore}")
        self.restore, self.p = float(restore), float(p)

    def sample(self, rng: np.random.Generator):
        if rng.random() >= self.p:
            return None
        n = int(rng.integers(self.num_ghosts[0], self.num_ghosts[1] + 1))
        axis = self.axes[int(rng.integers(len(self.axes)))]
        return "RandomGhosting", dict(num_ghosts=n, axis=axis, intensity=float(rng.uniform(*self.intensity)))


class RandomSpike:
    """tio.RandomSpike(num_spikes=1, intensity=(1, 3), p=1): num_spikes points of the shifted spectrum get A added and the real part is kept:
    stripes y = x + (A / V) sum_s cos(2 pi sum_a (k_sa - N_a // 2) x_a / N_a), k_sa = floor(pos_sa N_a), with A / V = g |mean(x)|, which is
    torchio's g max|F| / V for a non-negative volume (`spike_tables`, `csrc/kspace.hip`).  num_spikes is a fixed integer 1..4; a scalar
    intensity d means U(-d, d).  Draws: positions U(0, 1) [num_spikes][3], then g."""

    def __init__(self, num_spikes: int = 1, intensity=(1, 3), p: float = 1.0):
        if not isinstance(num_spikes, (int, np.integer)) or isinstance(num_spikes, bool):
            raise NotImplementedError("RandomSpike: a fixed integer number of spikes is built, not a range")
        if num_spikes < 1:
            raise ValueError("RandomSpike: num_spikes is at least 1")
        if num_spikes > ops.SPIKE_MAX:
            raise NotImplementedError(f"RandomSpike: num_spikes 1..{ops.SPIKE_MAX} are built")
        self.num_spikes, self.intensity, self.p = int(num_spikes), _pair(intensity, "intensity"), float(p)
        if self.intensity[1] < self.intensity[0]:
            raise ValueError("RandomSpike: intensity is a number or a (low, high) pair with low <= high")

    def sample(self, rng: np.random.Generator):
        if rng.random() >= self.p:
            return None
        positions = rng.random((self.num_spikes, 3))
        return "RandomSpike", dict(positions=positions, intensity=float(rng.uniform(*self.intensity)))


class RandomGamma:
    """tio.RandomGamma(log_gamma=(-0.3, 0.3), p=1): y = sign(x) |x|^gamma, gamma = exp(beta), beta ~ U(low, high); a scalar d means U(-d, d).
    Draws: beta.  Zeros stay zero with their sign (torchio rescales nothing either; its warning about negative voxels is not raised)."""

    def __init__(self, log_gamma=(-0.3, 0.3), p: float = 1.0):
        self.log_gamma, self.p = _pair(log_gamma, "log_gamma"), float(p)
        if self.log_gamma[1] < self.log_gamma[0]:
            raise ValueError("RandomGamma: log_gamma is a number or a (low, high) pair with low <= high")

    def sample(self, rng: np.random.Generator):
        if rng.random() >= self.p:
            return None
        beta = float(rng.uniform(*self.log_gamma))
        return "RandomGamma", dict(log_gamma=beta, gamma=math.exp(beta))


class RandomAnisotropy:
    """tio.RandomAnisotropy(axes=(0, 1, 2), downsampling=(1.5, 5), image_interpolation='linear', p=1): the volume is downsampled along one axis
    by f with nearest neighbour and brought back to its shape with linear interpolation (`anisotropy_tables`, `csrc/kspace.hip`).  A scalar
    downsampling d means U(1, d).  Draws: the axis, uniform over axes; f.  The edges are clamped where torchio pads."""

    def __init__(self, axes=(0, 1, 2), downsampling=(1.5, 5), image_interpolation: str = "linear", p: float = 1.0):
        if image_interpolation != "linear":
            raise NotImplementedError("RandomAnisotropy: only image_interpolation='linear' is built")
        self.axes = _axes(axes, "RandomAnisotropy")
        self.downsampling = (1.0, float(downsampling)) if isinstance(downsampling, (int, float)) else _pair(downsampling, "downsampling")
        if self.downsampling[0] < 1 or self.downsampling[1] < self.downsampling[0]:
            raise ValueError("RandomAnisotropy: downsampling is a number >= 1 or a (low, high) pair with 1 <= low <= high")
        self.p = float(p)

    def sample(self, rng: np.random.Generator):
        if rng.random() >= self.p:
            return None
        axis = self.axes[int(rng.integers(len(self.axes)))]
        return "RandomAnisotropy", dict(axis=axis, downsampling=float(rng.uniform(*self.downsampling)))


INTENSITY_TRANSFORMS = (RandomNoise, RandomBiasField, RandomBlur, RandomMotion, RandomGhosting, RandomSpike, RandomGamma, RandomAnisotropy)
_BUILT = ("RandomAffine (at most one), RandomFlip, RandomNoise, RandomBiasField, RandomBlur, RandomMotion, OneOf of the last four, "
          "RescaleIntensity (at most one); RandomElasticDeformation (at most one), OneOf of RandomAffine and RandomElasticDeformation in place of "
          "the two; ZNormalization in place of RescaleIntensity (at most one normaliser, it runs last), RescaleIntensity percentiles and "
          "masking_method None / 'mean' / a threshold; RandomGhosting, RandomSpike, RandomGamma, RandomAnisotropy, singly or in the intensity OneOf; "
          "HistogramStandardization (at most one; it runs before the one RescaleIntensity / ZNormalization and may be listed with it)")


class OneOf:
    """tio.OneOf(transforms, p=1): with probability p exactly one member is applied, chosen by weight (a dict transform -> weight, or a
    sequence with equal weights; weights are normalised).  The member's own p still applies.  Draws: one uniform for p, one for the choice,
    then the member's.  The members are all intensity transforms, or all spatial ones (RandomAffine, RandomElasticDeformation: `spatial` is
    then True and `sample` returns None or (member, the member's draw))."""

    def __init__(self, transforms, p: float = 1.0):
        items = list(transforms.items()) if isinstance(transforms, dict) else [(t, 1.0) for t in transforms]
        if not items:
            raise ValueError("OneOf: at least one transform")
        for t, w in items:
            if not isinstance(t, INTENSITY_TRANSFORMS + SPATIAL_ONE_OF_MEMBERS):
                raise NotImplementedError(f"OneOf: {type(t).__name__} is not built on the device ({_BUILT})")
            if w < 0:
                raise ValueError("OneOf: weights are non-negative")
        total = float(sum(w for _, w in items))
        if total <= 0:
            raise ValueError("OneOf: the weights sum to zero")
        self.transforms = [t for t, _ in items]
        self.spatial = isinstance(self.transforms[0], SPATIAL_ONE_OF_MEMBERS)
        if any(isinstance(t, SPATIAL_ONE_OF_MEMBERS) != self.spatial for t in self.transforms):
            raise NotImplementedError("OneOf: spatial (RandomAffine, RandomElasticDeformation) and intensity members in one OneOf are not built: "
                                      "the spatial transforms run as passes of their own before the intensity ones")
        self.weights = np.array([w / total for _, w in items], dtype=np.float64)
        self.p = float(p)

    def sample(self, rng: np.random.Generator):
        if rng.random() >= self.p:
            return None
        i = min(int(np.searchsorted(np.cumsum(self.weights), rng.random(), side="right")), len(self.transforms) - 1)
        draw = self.transforms[i].sample(rng)
        return (self.transforms[i], draw) if self.spatial else draw


# ---- host tables of the intensity launches ---------------------------------------------------------------------------------------------
# A `*_tables` function builds the rows of given samples; a `pack_*` function assembles one launch's tables for a batch from its draws,
# draws[b] = None or (class name, params) as in `DeviceCompose.last_intensity`: numpy only, rows of samples that drew anything else keep
# the defaults that make the kernel copy them.
def _drew(draws, name):
    """[(b, params)] of the samples that drew `name`."""
    return [(b, d[1]) for b, d in enumerate(draws) if d and d[0] == name]


def blur_tables(sigmas):
    """Host half of `ops.gaussian_blur3d` for sigmas [B][3]: (weights float32 [B][3][2R+1], radius int32 [B][3]) exactly as
    scipy.ndimage.gaussian_filter builds them (truncate = 4.0: radius int(4 sigma + 0.5), exp(-0.5 k^2 / sigma^2) normalised in float64; an
    axis with sigma <= 1e-15 is skipped = radius 0 with the single weight 1)."""
    s = np.asarray(sigmas, dtype=np.float64).reshape(-1, 3)
    weights = np.zeros((len(s), 3, ops.BLUR_TAPS), dtype=np.float32)
    weights[:, :, 0] = 1.0
    radius = np.zeros((len(s), 3), dtype=np.int32)
    for b in range(len(s)):
        for a in range(3):
            if s[b, a] > 1e-15:
                r = int(4.0 * s[b, a] + 0.5)
                if r > ops.BLUR_MAX_RADIUS:
                    raise ValueError(f"blur_tables: sigma {s[b, a]} needs radius {r}; sigma above 4 (radius above {ops.BLUR_MAX_RADIUS}) is not built")
                k = np.arange(-r, r + 1, dtype=np.float64)
                w = np.exp(-0.5 / (s[b, a] * s[b, a]) * k ** 2)
                weights[b, a, :2 * r + 1] = w / w.sum()
                radius[b, a] = r
    return weights, radius


def pack_blur(draws):
    """`blur_tables` of the batch: sigma 0 on every axis (radius 0, the single weight 1) for a sample that drew no blur."""
    sig = np.zeros((len(draws), 3), dtype=np.float64)
    for b, p in _drew(draws, "RandomBlur"):
        sig[b] = p["std"]
    return blur_tables(sig)


def bias_coefficients(coefficients, order: int, to_order: int) -> np.ndarray:
    """The coefficients of an order-`order` bias field laid out for a launch at `to_order` >= order (the missing terms are zero)."""
    have = {t: c for t, c in zip(bias_terms(order), coefficients)}
    return np.array([have.get(t, 0.0) for t in bias_terms(to_order)], dtype=np.float64)


def pack_pointwise(draws):
    """Tables of `ops.intensity_pointwise`: (kind int32 [B], noise float32 [B][2] = (std, mean), seeds uint64 [B], coeff float32
    [B][ops.BIAS_COEFFS], order).  order is the largest bias-field order of the batch (0 without one), every field laid out for it."""
    B = len(draws)
    kind, noise = np.zeros(B, dtype=np.int32), np.zeros((B, 2), dtype=np.float32)
    seeds, coeff = np.zeros(B, dtype=np.uint64), np.zeros((B, ops.BIAS_COEFFS), dtype=np.float32)
    order = max([p["order"] for _, p in _drew(draws, "RandomBiasField")], default=0)
    for b, p in _drew(draws, "RandomNoise"):
        kind[b], noise[b], seeds[b] = ops.INTENSITY_NOISE, (p["std"], p["mean"]), p["seed"]
    for b, p in _drew(draws, "RandomBiasField"):
        c = bias_coefficients(p["coefficients"], p["order"], order)
        kind[b], coeff[b, :len(c)] = ops.INTENSITY_BIAS, c
    return kind, noise, seeds, coeff, order


def motion_tables(times, W: int):
    """Host half of `ops.motion_artifact` for sorted times [B][K] in (0, 1): (ctab float32 [B][K+1][W], src int64 [B][K+1]).  torchio fills
    the shifted spectrum along the last axis in K+1 slabs [e_j, e_j+1), e = [0, int(W t_1), .., int(W t_K), W]; slab j comes from image
    src[j], where src is [0, 1, .., K] (0 = the unmoved volume) with entries 0 and i swapped, i = the first index with t_i > 0.5 or K if
    there is none (its sort_spectra: the unmoved volume fills the centre of k-space).  Row s of ctab is the real circular convolution kernel
    that slab stands for, c_s[m] = (1/W) sum_{j in the slab of s} cos(2 pi (j - W//2) m / W), in float64 and then rounded; the rows sum to
    the unit impulse."""
    t = np.asarray(times, dtype=np.float64)
    t = t.reshape(1, -1) if t.ndim == 1 else t
    B, K = t.shape
    W = int(W)
    ctab, src = np.zeros((B, K + 1, W), dtype=np.float32), np.zeros((B, K + 1), dtype=np.int64)
    m = np.arange(W, dtype=np.float64)
    for b in range(B):
        edges = [0] + [int(W * v) for v in t[b]] + [W]
        order = list(range(K + 1))
        late = np.nonzero(t[b] > 0.5)[0]
        i = int(late[0]) if len(late) else K
        order[0], order[i] = order[i], order[0]
        for j, s in enumerate(order):
            freq = np.arange(edges[j], edges[j + 1], dtype=np.float64) - W // 2
            ctab[b, s] = np.cos(2.0 * np.pi * freq[:, None] * m[None, :] / W).sum(axis=0) / W
        src[b] = order
    return ctab, src


def pack_motion(draws, shape):
    """Tables of `ops.motion_artifact` for volumes of `shape`: (mats float32 [B][K][3][4], ctab float32 [B][K+1][W], live int32 [B], K), K the
    largest number of movements in the batch.  A sample with fewer keeps identity maps and zero kernel rows for the rest."""
    moved = _drew(draws, "RandomMotion")
    B, W, K = len(draws), shape[2], max(len(p["times"]) for _, p in moved)
    mats = np.tile(np.eye(3, 4, dtype=np.float32), (B, K, 1, 1))
    ctab, live = np.zeros((B, K + 1, W), dtype=np.float32), np.zeros(B, dtype=np.int32)
    for b, p in moved:
        k = len(p["times"])
        ctab[b, :k + 1], live[b] = motion_tables(p["times"], W)[0][0], 1
        for j in range(k):
            mats[b, j] = affine_matrix((1, 1, 1), p["degrees"][j], p["translation"][j], shape).astype(np.float32)
    return mats, ctab, live, K


def ghosting_tables(num_ghosts, intensity, N) -> np.ndarray:
    """Host half of `ops.axis_circular_conv` for RandomGhosting draws: ctab float32 [B][ops.AXIS_CONV_MAX_N], row b = the real circular
    convolution kernel along an axis of N[b] voxels (entries N[b].. are zero) that scaling the planes j % n == 0, j != N // 2, of the shifted
    spectrum by 1 - g stands for: c[m] = delta[m] - (g / N) sum_{j in S} cos(2 pi (j - N // 2) m / N), the phase reduced modulo N in integers,
    summed in float64 and then rounded.  n == 0 or g == 0 gives the unit impulse; c[0] = 1 - g |S| / N and the row sums to 1 (the centre plane, the DC term, is kept)."""
    n_, g_, N_ = np.atleast_1d(num_ghosts), np.atleast_1d(intensity), np.atleast_1d(N)
    ctab = np.zeros((len(n_), ops.AXIS_CONV_MAX_N), dtype=np.float32)
    for b, (n, g, N) in enumerate(zip(n_, g_, N_)):
        n, g, N = int(n), float(g), int(N)
        if not 2 <= N <= ops.AXIS_CONV_MAX_N:
            raise ValueError(f"ghosting_tables: an axis of {N} voxels; 2..{ops.AXIS_CONV_MAX_N} are built")
        if n < 0:
            raise ValueError("ghosting_tables: num_ghosts is non-negative")
        c = np.zeros(N, dtype=np.float64)
        c[0] = 1.0
        if n > 0 and g != 0.0:
            j = np.array([j for j in range(0, N, n) if j != N // 2], dtype=np.int64)
            m = np.arange(N, dtype=np.int64)
            phase = ((j[:, None] - N // 2) * m[None, :]) % N
            c -= (g / N) * np.cos(2.0 * np.pi * phase / N).sum(axis=0)
        ctab[b, :N] = c
    return ctab


def pack_ghosting(draws, shape):
    """Tables of `ops.axis_circular_conv` for volumes of `shape`: (ctab, axis int32 [B], live int32 [B]).  A sample that drew no ghosting gets
    the unit impulse along the last axis and live 0."""
    B = len(draws)
    n, g, N = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.float64), np.full(B, shape[2], dtype=np.int64)
    axis, live = np.full(B, 2, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, p in _drew(draws, "RandomGhosting"):
        n[b], g[b], axis[b], N[b], live[b] = p["num_ghosts"], p["intensity"], p["axis"], shape[p["axis"]], 1
    return ghosting_tables(n, g, N), axis, live


def spike_tables(positions, shape) -> np.ndarray:
    """Host half of `ops.gamma_spike` for the spikes of ONE sample, positions [S][3] in [0, 1): float32 [ops.SPIKE_MAX][2][D + H + W], entry
    [s][0 / 1][offset_a + x] = cos / sin(2 pi ((k_sa - N_a // 2) x mod N_a) / N_a) with k_sa = floor(pos_sa N_a) (at most N_a - 1) and offsets
    0, D, D + H: the phase is reduced in integers, evaluated in float64 and then rounded.  Rows S.. are zero."""
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    if not 1 <= len(pos) <= ops.SPIKE_MAX:
        raise ValueError(f"spike_tables: {len(pos)} spikes; 1..{ops.SPIKE_MAX} are built")
    if (pos < 0).any() or (pos >= 1).any():
        raise ValueError("spike_tables: positions are in [0, 1)")
    tab = np.zeros((ops.SPIKE_MAX, 2, int(sum(shape))), dtype=np.float32)
    for s in range(len(pos)):
        off = 0
        for a, N in enumerate(int(v) for v in shape):
            k = min(int(np.floor(pos[s, a] * N)), N - 1)
            phase = 2.0 * np.pi * (((k - N // 2) * np.arange(N, dtype=np.int64)) % N) / N
            tab[s, 0, off:off + N], tab[s, 1, off:off + N] = np.cos(phase), np.sin(phase)
            off += N
    return tab


def pack_gamma_spike(draws, shape):
    """Tables of `ops.gamma_spike` for volumes of `shape`: (kind int32 [B], gamma float32 [B], amp float32 [B], nspikes int32 [B], tab float32
    [B][ops.SPIKE_MAX][2][D + H + W]); gamma 1 and zeros for a sample that drew neither."""
    B = len(draws)
    kind, gamma, amp = np.zeros(B, dtype=np.int32), np.ones(B, dtype=np.float32), np.zeros(B, dtype=np.float32)
    nspikes, tab = np.zeros(B, dtype=np.int32), np.zeros((B, ops.SPIKE_MAX, 2, sum(shape)), dtype=np.float32)
    for b, p in _drew(draws, "RandomGamma"):
        kind[b], gamma[b] = ops.KSPACE_GAMMA, p["gamma"]
    for b, p in _drew(draws, "RandomSpike"):
        kind[b], amp[b], nspikes[b], tab[b] = ops.KSPACE_SPIKE, p["intensity"], len(p["positions"]), spike_tables(p["positions"], shape)
    return kind, gamma, amp, nspikes, tab


def anisotropy_tables(downsampling, N: int, n_max: Optional[int] = None):
    """Host half of `ops.axis_gather2` for ONE sample's factor f >= 1 along an axis of N voxels: (src int32 [n_max][2], w float32 [n_max]), n_max
    = N unless given.  All in float64: n_low = max(1, ceil(N / f)) low-resolution samples, sample j = the original voxel nearest to
    (j + 0.5) f - 0.5 (floor(c + 0.5), clamped to 0..N-1); output voxel i sits at u = (i + 0.5) / f - 0.5 on the low grid, clamped to
    [0, n_low - 1]; src[i] = the voxels of low samples floor(u) and min(floor(u) + 1, n_low - 1), w[i] = float32(u - floor(u)).  f == 1 gives
    src[i][0] = i and w = 0."""
    f, N = float(downsampling), int(N)
    if f < 1.0 or N < 1:
        raise ValueError("anisotropy_tables: downsampling >= 1 along an axis of at least one voxel")
    n_max = N if n_max is None else int(n_max)
    n_low = max(1, int(np.ceil(N / f)))
    low = np.clip(np.floor((np.arange(n_low, dtype=np.float64) + 0.5) * f - 0.5 + 0.5), 0, N - 1).astype(np.int64)
    u = np.clip((np.arange(N, dtype=np.float64) + 0.5) / f - 0.5, 0.0, float(n_low - 1))
    j0 = np.floor(u).astype(np.int64)
    j1 = np.minimum(j0 + 1, n_low - 1)
    src, w = np.zeros((n_max, 2), dtype=np.int32), np.zeros(n_max, dtype=np.float32)
    src[:N, 0], src[:N, 1], w[:N] = low[j0], low[j1], (u - j0).astype(np.float32)
    return src, w


def pack_anisotropy(draws, shape):
    """Tables of `ops.axis_gather2` for volumes of `shape`: (src int32 [B][max(shape)][2], w float32 [B][max(shape)], axis int32 [B], live
    int32 [B]); zeros for a sample that drew no anisotropy."""
    B, n_max = len(draws), max(shape)
    src, w = np.zeros((B, n_max, 2), dtype=np.int32), np.zeros((B, n_max), dtype=np.float32)
    axis, live = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b, p in _drew(draws, "RandomAnisotropy"):
        axis[b], live[b] = p["axis"], 1
        src[b], w[b] = anisotropy_tables(p["downsampling"], shape[p["axis"]], n_max)
    return src, w, axis, live


def pack_elastic(fields, num_control_points):
    """Tables of `ops.elastic_deform`: (ctrl float32 [B][n0][n1][n2][3], live int32 [B]) from fields[b] = None or a sample's coarse field
    (`RandomElasticDeformation.sample`)."""
    ctrl = np.zeros((len(fields),) + tuple(num_control_points) + (3,), dtype=np.float32)
    live = np.zeros(len(fields), dtype=np.int32)
    for b, f in enumerate(fields):
        if f is not None:
            ctrl[b], live[b] = f, 1
    return ctrl, live


# ---- the intensity launches: one launcher per kernel, each uploads its packer's tables and runs the batch through one `ops` entry point ------
def _dev(a: np.ndarray, device) -> torch.Tensor:
    return torch.from_numpy(a).to(device)


def _launch_pointwise(x, draws):
    kind, noise, seeds, coeff, order = pack_pointwise(draws)
    y = torch.empty_like(x)
    ops.intensity_pointwise(x, y, _dev(kind, x.device), _dev(noise, x.device), _dev(seeds.view(np.int64), x.device), _dev(coeff, x.device), order)
    return y


def _launch_blur(x, draws):
    weights, radius = pack_blur(draws)
    y, scratch = torch.empty_like(x), torch.empty_like(x)
    ops.gaussian_blur3d(x, y, scratch, _dev(weights, x.device), _dev(radius, x.device), int(radius.max()))
    return y


def _launch_motion(x, draws):
    mats, ctab, live, K = pack_motion(draws, tuple(x.shape[-3:]))
    part = ops.minmax_partials(x.shape[0], x.device)
    ops.volume_minmax(x, part)                                            # pad value of the movements = this stage's input minimum
    y = torch.empty_like(x)
    ops.motion_artifact(x, y, _dev(mats, x.device), _dev(ctab, x.device), _dev(live, x.device), part, K)
    return y


def _launch_ghosting(x, draws):
    ctab, axis, live = pack_ghosting(draws, tuple(x.shape[-3:]))
    y = torch.empty_like(x)
    ops.axis_circular_conv(x, y, _dev(ctab, x.device), _dev(axis, x.device), _dev(live, x.device))
    return y


def _launch_gamma_spike(x, draws):
    tables = pack_gamma_spike(draws, tuple(x.shape[-3:]))
    # the spikes scale with the mean of this stage's input, taken on the device and never read here
    stats = ops.volume_stats(x, None, want_std=False)[0] if _drew(draws, "RandomSpike") else \
        torch.zeros((x.shape[0], ops.NORMALIZE_STATS), dtype=torch.float64, device=x.device)
    y = torch.empty_like(x)
    ops.gamma_spike(x, y, *[_dev(t, x.device) for t in tables], stats)
    return y


def _launch_anisotropy(x, draws):
    tables = pack_anisotropy(draws, tuple(x.shape[-3:]))
    y = torch.empty_like(x)
    ops.axis_gather2(x, y, *[_dev(t, x.device) for t in tables])
    return y


# (the class names a launch serves, its launcher), in launch order: a new intensity transform adds or joins a row here
INTENSITY_GROUPS = ((("RandomNoise", "RandomBiasField"), _launch_pointwise),
                    (("RandomBlur",), _launch_blur),
                    (("RandomMotion",), _launch_motion),
                    (("RandomGhosting",), _launch_ghosting),
                    (("RandomGamma", "RandomSpike"), _launch_gamma_spike),
                    (("RandomAnisotropy",), _launch_anisotropy))


def apply_intensity(x: torch.Tensor, draws) -> torch.Tensor:
    """One listed intensity transform on the batch: draws[b] = None or (class name, params).  At most one launch per group of
    INTENSITY_GROUPS, each only when a sample drew one of its classes; samples that drew anything else ride along as copies."""
    drawn = {d[0] for d in draws if d}
    for names, launch in INTENSITY_GROUPS:
        if drawn.intersection(names):
            x = launch(x, draws)
    return x


class DeviceCompose:
    """The transforms of train.py:38-62 on a batch [B, 1, D, H, W] (or [B, D, H, W]) already on the GPU.  Affine and flips are merged
    into one resampling pass (affine first, flips on its output), the intensity transforms (singly or inside OneOf) follow in listed
    order, the one normaliser (RescaleIntensity or ZNormalization) runs last, as in the reference's Compose, and a HistogramStandardization
    runs just before it wherever it is listed (it draws nothing; its status words are `last_hist_status`).  RandomElasticDeformation is a resampling pass of its own BEFORE the
    affine/flip pass wherever it is listed: torchio would apply the spatial transforms in listed order, here elastic always runs first
    (a sample that draws both is interpolated twice, as in torchio).  A OneOf of RandomAffine / RandomElasticDeformation members may stand
    in place of the single affine and/or elastic: each sample then gets at most one of them.  Per sample the random draws are: elastic,
    affine (or the spatial OneOf in their place), flips, then every intensity transform in listed order; a compose that lists no elastic
    transform and no spatial OneOf consumes the stream it consumed before they existed."""

    def __init__(self, transforms: Sequence, seed: Optional[int] = None):
        self.affine = [t for t in transforms if isinstance(t, RandomAffine)]
        self.elastic = [t for t in transforms if isinstance(t, RandomElasticDeformation)]
        self.spatial = [t for t in transforms if isinstance(t, OneOf) and t.spatial]     # in place of the single affine and/or elastic
        self.flips = [t for t in transforms if isinstance(t, RandomFlip)]
        self.rescale = [t for t in transforms if isinstance(t, RescaleIntensity)]
        self.znorm = [t for t in transforms if isinstance(t, ZNormalization)]
        self.hist = [t for t in transforms if isinstance(t, HistogramStandardization)]
        self.intensity = [t for t in transforms if isinstance(t, INTENSITY_TRANSFORMS) or (isinstance(t, OneOf) and not t.spatial)]
        elastic = self.elastic + [t for one in self.spatial for t in one.transforms if isinstance(t, RandomElasticDeformation)]
        if len(self.affine) > 1 or len(self.rescale) + len(self.znorm) > 1 or len(elastic) > 1 or len(self.spatial) > 1 or \
                (self.spatial and (self.affine or self.elastic)) or len(self.hist) > 1 or \
                len(self.affine) + len(self.elastic) + len(self.spatial) + len(self.flips) + len(self.rescale) + len(self.znorm) + \
                len(self.hist) + len(self.intensity) != len(transforms):
            raise NotImplementedError(f"DeviceCompose: {_BUILT}; anything else is not built")
        self._elastic = elastic[0] if elastic else None                   # the one elastic transform, listed singly or inside the spatial OneOf
        self.rng = np.random.default_rng(seed)
        self.last_params = None                                           # [(flip bits, affine params or None)] of the last call: tests, logging
        self.last_elastic = None                                          # per sample None or the coarse field float64 [n0][n1][n2][3], borders locked
        # the intensity draws of the last call, one entry per sample: None or (class name, params) -- with several intensity transforms
        # listed, a tuple of such entries in listed order
        self.last_intensity = None
        # int32 [B] on the device after a call that ran a percentile / masked rescale or a z-normalisation: 0 normalised, 1 empty mask,
        # 2 zero range or zero std (such samples come back unchanged).  Never synchronised on here; None after any other call.
        self.last_norm_status = None
        # int32 [B] on the device after a call that ran a HistogramStandardization: 0 standardised, 1 empty mask (the sample went on unchanged)
        self.last_hist_status = None

    def sample(self, B: int, shape):
        mats = np.tile(np.eye(3, 4, dtype=np.float32), (B, 1, 1))
        flags = np.zeros(B, dtype=np.int32)
        params, draws, fields = [], [], []
        if self._elastic is not None:
            self._elastic.check_folding(shape)
        for b in range(B):
            if self.spatial:
                pick = self.spatial[0].sample(self.rng) or (None, None)
                el, aff = (None, pick[1]) if isinstance(pick[0], RandomAffine) else (pick[1], None)
            else:
                el = self.elastic[0].sample(self.rng) if self.elastic else None
                aff = self.affine[0].sample(self.rng) if self.affine else None
            fields.append(el)
            bits = 0
            for f in self.flips:
                bits ^= f.sample(self.rng)
            if aff is not None:
                mats[b] = affine_matrix(*aff, shape).astype(np.float32)
                bits |= 8
            flags[b] = bits
            params.append((bits & 7, aff))
            d = tuple(t.sample(self.rng) for t in self.intensity)
            draws.append(d[0] if len(d) == 1 else (d or None))
        self.last_params, self.last_intensity, self.last_elastic = params, draws, fields
        return mats, flags

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("DeviceCompose runs on the GPU: move the batch first (there is no CPU path)")
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        B, shape = x.shape[0], tuple(x.shape[-3:])
        part = ops.minmax_partials(B, x.device)
        if self.affine or self.elastic or self.spatial or self.flips or self.intensity:
            mats, flags = self.sample(B, shape)
            if any(f is not None for f in self.last_elastic):             # elastic first, a pass of its own (class docstring)
                ctrl, live = pack_elastic(self.last_elastic, self._elastic.num_control_points)
                ops.volume_minmax(x, part)                                # pad value = this pass's input minimum
                out = torch.empty_like(x)
                ops.elastic_deform(x, out, _dev(ctrl, x.device), _dev(live, x.device), part)
                x = out
            if flags.any():
                ops.volume_minmax(x, part)                                # pad value of the resampling = the input volume's minimum
                out = torch.empty_like(x)
                ops.spatial_transform(x, out, _dev(mats, x.device), _dev(flags, x.device), part)
                x = out
            for s in range(len(self.intensity)):
                x = apply_intensity(x, [d if len(self.intensity) == 1 else (d[s] if d else None) for d in self.last_intensity])
        self.last_norm_status = self.last_hist_status = None
        for t in self.hist:                                               # histogram standardisation, then ...
            x, self.last_hist_status = t.apply(x, part)
        for t in self.rescale + self.znorm:                               # ... the one normaliser, if any
            x, self.last_norm_status = t.apply(x, part)
        return x


# ---- geometry: torchio's first stage (Resample / Resize / CropOrPad) for a ragged batch ---------------------------------------------------
# Per sample and array axis, with input length n, input spacing s and target length N (this module's own definitions; parity with torchio
# / SimpleITK is unpinned, module docstring):
#   Resample to spacing t: r = t / s, intermediate length m = max(1, floor(n / r + 1e-9)); Resize to N: r = n / N, m = N.  Intermediate index
#     u reads the input position p = (u + 0.5) r - 0.5 (edges aligned).
#   linear: p clamped to [0, n - 1], taps floor(p) and min(floor(p) + 1, n - 1) with weights 1 - g and g (F.interpolate, align_corners=False,
#     no antialiasing); nearest: the tap min(floor(p + 0.5), n - 1) ('nearest-exact'; antialias is ignored).
#   antialias, linear, r > 1: the axis is first smoothed by a Gaussian of sigma = sqrt((r^2 - 1) / (8 ln 2)) voxels (Cardoso et al.), truncated
#     at int(4 sigma + 0.5), normalised, the edge value repeated (scipy.ndimage.gaussian_filter1d(mode='nearest')).  Filter and interpolation are
#     linear maps along one axis: they are composed into one banded row of at most 2 radius + 2 taps.
#   CropOrPad from m to N, d = N - m: padding puts ceil(d / 2) voxels in front and floor(d / 2) behind, cropping removes ceil(-d / 2) in front
#     and floor(-d / 2) behind; output index q is intermediate index u = q - c, c the signed front pad, and a voxel with u outside [0, m) on
#     any axis is the pad value.
def _positive_triple(v, name, kind):
    t = _triple(v, name, kind)
    if any(not x > 0 for x in t):
        raise ValueError(f"{name}: positive values, not {v!r}")
    return t


def _interpolation(v, name):
    if v not in ("nearest", "linear"):
        raise NotImplementedError(f"{name}: image_interpolation 'nearest' and 'linear' are built, not {v!r}")
    return v


class CropOrPad:
    """tio.CropOrPad(target_shape, padding_mode=0): centred crop and / or pad to target_shape (a number or one length per array axis).
    padding_mode is a number or 'minimum' (the sample's own input minimum, taken on the device)."""

    def __init__(self, target_shape, padding_mode=0, mask_name=None, labels=None):
        if mask_name is not None or labels is not None:
            raise NotImplementedError("CropOrPad: target_shape and padding_mode (a number or 'minimum') are built; mask_name and labels are not")
        if isinstance(padding_mode, str) and padding_mode != "minimum" or isinstance(padding_mode, bool) or \
                not isinstance(padding_mode, (str, int, float, np.integer, np.floating)):
            raise NotImplementedError(f"CropOrPad: padding_mode is a number or 'minimum'; {padding_mode!r} is not built")
        if not isinstance(padding_mode, str) and not math.isfinite(padding_mode):
            raise ValueError("CropOrPad: a finite pad value")
        self.target_shape = _positive_triple(target_shape, "CropOrPad target_shape", int)
        self.padding_mode = padding_mode if isinstance(padding_mode, str) else float(padding_mode)


class Resize:
    """tio.Resize(target_shape, image_interpolation='linear'): every sample is resampled to target_shape whatever its spacing.  antialias
    (not torchio's: it resizes without) smooths an axis that shrinks as `Resample` does."""

    def __init__(self, target_shape, image_interpolation: str = "linear", antialias: bool = True):
        self.target_shape = _positive_triple(target_shape, "Resize target_shape", int)
        self.image_interpolation, self.antialias = _interpolation(image_interpolation, "Resize"), bool(antialias)


class Resample:
    """tio.Resample(target=1, image_interpolation='linear', antialias): every sample is resampled to the spacing `target` (a number or one
    spacing per array axis, in the units of the samples' own spacing).  A reference image or path as target is not built."""

    def __init__(self, target=1.0, image_interpolation: str = "linear", antialias: bool = True):
        if isinstance(target, (str, bytes, os.PathLike)) or isinstance(target, bool) or \
                not isinstance(target, (int, float, np.integer, np.floating, tuple, list, np.ndarray)):
            raise NotImplementedError(f"Resample: target is a spacing (a number or one per array axis); {target!r} (a reference image or path) is not built")
        self.target = _positive_triple(target.tolist() if isinstance(target, np.ndarray) else target, "Resample target", float)
        self.image_interpolation, self.antialias = _interpolation(image_interpolation, "Resample"), bool(antialias)


def _conform_stages(transforms):
    """(the one Resample or Resize or None, the one CropOrPad or None, target_shape) of a Conform's transforms."""
    transforms = list(transforms)
    res = [t for t in transforms if isinstance(t, (Resample, Resize))]
    crop = [t for t in transforms if isinstance(t, CropOrPad)]
    if len(res) + len(crop) != len(transforms) or len(res) > 1 or len(crop) > 1 or not transforms or (res and crop and transforms[0] is crop[0]):
        raise NotImplementedError("Conform: at most one Resample or Resize, followed by at most one CropOrPad, is built")
    if not crop and isinstance(res[0], Resample):
        raise ValueError("Conform: a Resample alone gives every sample its own output shape; follow it with a CropOrPad")
    return (res[0] if res else None), (crop[0] if crop else None), (crop[0] if crop else res[0]).target_shape


def _conform_axis(n: int, r: float, m: int, N: int, interpolation: str, antialias: bool):
    """One axis of one sample, all in float64: (start int64 [N], rows [N][K], inside bool [N], c).  Row q of the composed map (Gaussian,
    interpolation, crop / pad) reads the inputs start[q] .. start[q] + K - 1; K is the widest band of the axis and start[q] + K <= n."""
    u = np.arange(m)
    p = (u + 0.5) * r - 0.5
    A = np.zeros((m, n), dtype=np.float64)
    if interpolation == "nearest":
        A[u, np.clip(np.floor(p + 0.5).astype(np.int64), 0, n - 1)] = 1.0
    else:
        p = np.clip(p, 0.0, float(n - 1))
        i0 = np.floor(p).astype(np.int64)
        g = p - i0
        np.add.at(A, (u, i0), 1.0 - g)
        np.add.at(A, (u, np.minimum(i0 + 1, n - 1)), g)
        if antialias and r > 1.0:
            sigma = math.sqrt((r * r - 1.0) / (8.0 * math.log(2.0)))
            radius = int(4.0 * sigma + 0.5)
            k = np.arange(-radius, radius + 1, dtype=np.float64)
            w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
            w /= w.sum()
            G, j = np.zeros((n, n), dtype=np.float64), np.arange(n)
            for kk, wk in zip(range(-radius, radius + 1), w):
                np.add.at(G, (j, np.clip(j + kk, 0, n - 1)), wk)
            A = A @ G
    nz = A != 0.0
    first, last = nz.argmax(axis=1), n - 1 - nz[:, ::-1].argmax(axis=1)
    K = int((last - first + 1).max())
    first = np.minimum(first, n - K)
    rows_m = A[u[:, None], first[:, None] + np.arange(K)[None, :]]
    d = N - m
    c = -(-d // 2) if d >= 0 else -((1 - d) // 2)                     # the signed front pad: ceil(d / 2), or minus ceil(-d / 2)
    uu = np.arange(N) - c
    inside = (uu >= 0) & (uu < m)
    uu = np.clip(uu, 0, m - 1)
    return np.where(inside, first[uu], 0), np.where(inside[:, None], rows_m[uu], 0.0), inside, c


class ConformTables(NamedTuple):
    """The host tables of one `Conform` call, the three axes concatenated at offsets 0, D, D + H: start int32 [B][D + H + W], weights float32
    [B][D + H + W][T] (T = the largest band of the batch), inside bool [B][D + H + W], taps int32 [B][3] (each sample's own band per axis),
    geometry float64 [B][3][2] = (r, c) per sample and axis."""
    start: np.ndarray
    weights: np.ndarray
    inside: np.ndarray
    taps: np.ndarray
    geometry: np.ndarray

    def axis(self, b: int, a: int, target_shape):
        """(start [N], weights [N][T], inside [N]) of sample b along axis a."""
        off = int(sum(target_shape[:a]))
        rows = slice(off, off + int(target_shape[a]))
        return self.start[b, rows], self.weights[b, rows], self.inside[b, rows]


_conform_axis_cached = functools.lru_cache(maxsize=1024)(_conform_axis)      # scans of one protocol repeat their shapes


def conform_tables(shapes, spacing, transforms, target_shape, dtype=np.float32) -> ConformTables:
    """The banded tables (section comment above) that bring samples of `shapes` [B][3] and `spacing` [B][3] onto target_shape through
    `transforms` (what `Conform` takes).  Float64 throughout, the weights rounded to float32 once (dtype=np.float64 keeps them unrounded: tests).  A pure crop, pad or identity yields one tap
    of weight exactly 1.  A band wider than ops.CONFORM_MAX_TAPS = 16 (antialiasing at a factor above about 4.5) is refused."""
    res, crop, want = _conform_stages(transforms)
    N = tuple(int(v) for v in target_shape)
    if N != tuple(want):
        raise ValueError(f"conform_tables: the transforms end on {tuple(want)}, not on target_shape {N}")
    shapes = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    spacing = np.asarray(spacing, dtype=np.float64).reshape(-1, 3)
    if len(shapes) != len(spacing) or len(shapes) < 1 or (shapes < 1).any() or not (spacing > 0).all():
        raise ValueError("conform_tables: shapes [B][3] of positive lengths and spacing [B][3] of positive spacings expected")
    B, S = len(shapes), sum(N)
    per, geometry, taps = [], np.zeros((B, 3, 2), dtype=np.float64), np.ones((B, 3), dtype=np.int32)
    for b in range(B):
        for a in range(3):
            n = int(shapes[b, a])
            if isinstance(res, Resample):
                r = res.target[a] / float(spacing[b, a])
                m = max(1, int(math.floor(n / r + 1e-9)))
            elif isinstance(res, Resize):
                r, m = n / float(res.target_shape[a]), res.target_shape[a]
            else:
                r, m = 1.0, n
            interp, anti = (res.image_interpolation, res.antialias) if res is not None else ("nearest", False)
            start, rows, inside, c = _conform_axis_cached(n, r, m, N[a] if crop is not None else m, interp, anti)
            if rows.shape[1] > ops.CONFORM_MAX_TAPS:
                raise ValueError(f"conform_tables: sample {b}, axis {a}: antialiased resampling by the factor {r:.4g} needs {rows.shape[1]} taps; "
                                 f"at most {ops.CONFORM_MAX_TAPS} are built (factors up to about 4.5)")
            per.append((start, rows, inside))
            geometry[b, a], taps[b, a] = (r, c), rows.shape[1]
    T = int(taps.max())
    start, weights, inside = np.zeros((B, S), np.int32), np.zeros((B, S, T), dtype), np.zeros((B, S), bool)
    off = np.concatenate([[0], np.cumsum(N)])
    for b in range(B):
        for a in range(3):
            s, w, i = per[b * 3 + a]
            rows = slice(off[a], off[a + 1])
            start[b, rows], weights[b, rows, :w.shape[1]], inside[b, rows] = s, w, i
    return ConformTables(start, weights, inside, taps, geometry)


class Conform:
    """Raw volumes of any shape and spacing onto the model's grid, on the device, in one call: `x = conform(ragged.to(device))` gives float32
    [B, 1, D, H, W] for a `RaggedBatch`.  transforms: at most one `Resample` or `Resize`, followed by at most one `CropOrPad` (a Resample alone
    is refused: its output shape would differ per sample).  The host builds one banded table per sample and axis (`conform_tables`); the
    device gathers and contracts (`ops.conform_volumes`, csrc/conform.hip).  An axis that is only cropped, padded or already conforming, and
    every axis under 'nearest', moves bits.  `last_geometry` float64 [B][3][2] holds (r, c) of the last call per sample and axis: output index q
    sits at the input position (q - c + 0.5) r - 0.5 of the scan's own grid."""

    def __init__(self, transforms: Sequence):
        self.transforms = list(transforms)
        self.resample, self.crop, self.target_shape = _conform_stages(self.transforms)
        self.last_geometry = None

    def __call__(self, ragged: RaggedBatch) -> torch.Tensor:
        if not ragged.data.is_cuda:
            raise RuntimeError("Conform runs on the GPU: move the batch first, ragged.to(device) (there is no CPU path)")
        shapes, offsets = ragged.shapes.cpu().numpy(), ragged.offsets.cpu().numpy()
        t = conform_tables(shapes, ragged.spacing.cpu().numpy(), self.transforms, self.target_shape)
        self.last_geometry = t.geometry
        mode = self.crop.padding_mode if self.crop is not None else 0.0
        partials = None
        if mode == "minimum" and not t.inside.all():                      # the pad value = the sample's own minimum, never read here
            partials = ops.ragged_minmax(ragged.data, offsets, shapes)
        out = ops.conform_volumes(ragged.data, offsets, shapes, t.start, t.weights, t.inside, t.taps, self.target_shape,
                                  pad_value=0.0 if mode == "minimum" else mode, partials=partials)
        return out.unsqueeze(1)


def conform_from_config(c) -> Conform:
    """config['data']['conform']: target_shape, one of spacing (-> Resample) / resize (-> Resize) or neither, and optionally
    image_interpolation, antialias, padding_mode."""
    known = {"target_shape", "spacing", "resize", "image_interpolation", "antialias", "padding_mode", "spacing_key"}
    if "target_shape" not in c or set(c) - known or ("spacing" in c and "resize" in c):
        raise ValueError(f"config['data']['conform']: target_shape and at most one of spacing / resize, with the options {sorted(known)}; got {sorted(c)}")
    opts = dict(image_interpolation=c.get("image_interpolation", "linear"), antialias=c.get("antialias", True))
    stages = [Resample(c["spacing"], **opts)] if "spacing" in c else [Resize(c["resize"], **opts)] if "resize" in c else []
    return Conform(stages + [CropOrPad(c["target_shape"], c.get("padding_mode", 0))])


class MixedTarget(NamedTuple):
    """The target of a mixed batch, kept as the pair it came from: row i is class a[i] with weight lam[i] and class b[i] with 1 - lam[i].
    a, b int64 [B], lam float32 [B], device tensors.  The fused losses take it as `target` (losses._FusedLoss.forward)."""
    a: torch.Tensor
    b: torch.Tensor
    lam: torch.Tensor

    def dense(self, num_classes: int, smoothing: float = 0.0) -> torch.Tensor:
        """[B][K] probability rows (1 - e)(lam onehot(a) + (1 - lam) onehot(b)) + e / K in plain torch: for metrics of one's own and for tests."""
        lam = self.lam.to(torch.float64).unsqueeze(1)
        one = lambda t: torch.nn.functional.one_hot(t, num_classes).to(torch.float64)  # noqa: E731
        return (1.0 - smoothing) * (lam * one(self.a) + (1.0 - lam) * one(self.b)) + smoothing / num_classes


def mix_box(lam: float, centre, shape):
    """timm's rand_bbox carried to three axes: r = (1 - lam)^(1/3), side s_a = int(N_a r), the half-open range [clip(c_a - s_a // 2),
    clip(c_a + s_a // 2)) per axis, and lam corrected to 1 - box volume / V.  Returns ((d0, d1, h0, h1, w0, w1), lam)."""
    r = (1.0 - lam) ** (1.0 / 3.0)
    box, vol = [], 1
    for c, n in zip(centre, shape):
        s = int(n * r)
        lo, hi = int(np.clip(c - s // 2, 0, n)), int(np.clip(c + s // 2, 0, n))
        box += [lo, hi]
        vol *= hi - lo
    return tuple(box), 1.0 - vol / float(np.prod([int(n) for n in shape]))


class BatchMix:
    """timm.data.Mixup on a batch of volumes already on the GPU: `x, target = mix(x, labels)`, called AFTER DeviceCompose (timm mixes
    normalised tensors), one launch (csrc/batchmix.hip).  Arguments and meanings are timm's: Mixup with lam ~ Beta(mixup_alpha, mixup_alpha),
    CutMix with a box of volume share 1 - lam, lam ~ Beta(cutmix_alpha, cutmix_alpha); `prob` applies a unit at all, `switch_prob` picks CutMix
    when both alphas are live; mode 'elem' draws per sample, 'batch' once for the batch.  Unlike timm, a sample's partner is perm[b] of a random
    permutation (not the flipped batch), and the mixed target comes back as the pair MixedTarget(labels, labels[perm], lam).

    Its random stream is its own (np.random.default_rng(seed)).  Per unit, always all of them so that the stream does not depend on the
    outcomes: one uniform for `prob`, one for the switch (CutMix when it is < switch_prob and both alphas are > 0, otherwise the only live
    alpha), lam = rng.beta(alpha, alpha) of the chosen kind, three box centres rng.integers(N_a); after all units one rng.permutation(B).
    A unit that is not applied, and a CutMix whose box came out empty, is a copy with lam = 1; in 'elem' mode so is a sample whose partner is
    itself ('batch' mode keeps one mode, lam and box for every sample: mixing a volume with itself changes nothing beyond rounding)."""

    def __init__(self, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0, prob: float = 1.0, switch_prob: float = 0.5, mode: str = "elem",
                 seed: Optional[int] = None):
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError(f"BatchMix: the alphas must not be negative, got {mixup_alpha}, {cutmix_alpha}")
        if mixup_alpha == 0 and cutmix_alpha == 0:
            raise ValueError("BatchMix: mixup_alpha and cutmix_alpha are both 0, which mixes nothing")
        if not 0.0 <= prob <= 1.0 or not 0.0 <= switch_prob <= 1.0:
            raise ValueError(f"BatchMix: prob and switch_prob lie in [0, 1], got {prob}, {switch_prob}")
        if mode not in ("elem", "batch"):
            raise ValueError(f"BatchMix: mode is 'elem' or 'batch', not {mode!r}")
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob, self.mode = float(mixup_alpha), float(cutmix_alpha), float(prob), float(switch_prob), mode
        self.rng = np.random.default_rng(seed)
        self.last_mix = None                                              # dict(mode, lam, box, perm) of the last call, numpy arrays

    def _unit(self, shape):
        """(mode, lam, box) of one unit; consumes the same draws whatever comes out."""
        applied = self.rng.random() < self.prob
        switch = self.rng.random()
        cut = self.mixup_alpha == 0 or (self.cutmix_alpha > 0 and switch < self.switch_prob)
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(self.rng.beta(alpha, alpha))
        centre = [int(self.rng.integers(n)) for n in shape]
        if not applied:
            return ops.MIX_COPY, 1.0, (0,) * 6
        if not cut:
            return ops.MIX_MIXUP, lam, (0,) * 6
        box, lam = mix_box(lam, centre, shape)
        if any(box[2 * a + 1] <= box[2 * a] for a in range(3)):
            return ops.MIX_COPY, 1.0, (0,) * 6
        return ops.MIX_CUTMIX, lam, box

    def sample(self, B: int, shape) -> dict:
        """The host tables of one call: mode int32 [B], lam float64 [B], box int32 [B][6], perm int32 [B].  Pure host work."""
        shape = tuple(int(n) for n in shape)
        units = [self._unit(shape) for _ in range(B)] if self.mode == "elem" else [self._unit(shape)] * B
        perm = self.rng.permutation(B).astype(np.int32)
        mode = np.array([u[0] for u in units], dtype=np.int32)
        lam = np.array([u[1] for u in units], dtype=np.float64)
        box = np.array([u[2] for u in units], dtype=np.int32).reshape(B, 6)
        if self.mode == "elem":
            own = perm == np.arange(B)
            mode[own], lam[own], box[own] = ops.MIX_COPY, 1.0, 0
        self.last_mix = dict(mode=mode, lam=lam, box=box, perm=perm)
        return self.last_mix

    def __call__(self, x: torch.Tensor, labels: torch.Tensor):
        if not x.is_cuda:
            raise RuntimeError("BatchMix runs on the GPU: move the batch first (there is no CPU path)")
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        t = self.sample(x.shape[0], tuple(x.shape[-3:]))
        labels = labels.to(device=x.device, dtype=torch.int64).contiguous().view(-1)
        lam32 = t["lam"].astype(np.float32)
        target = MixedTarget(labels, labels[torch.from_numpy(t["perm"].astype(np.int64)).to(x.device)], torch.from_numpy(lam32).to(x.device))
        if (t["mode"] == ops.MIX_COPY).all():
            return x, target
        out = torch.empty_like(x)
        ops.batch_mix(x, out, t["mode"], lam32, t["perm"], t["box"])
        return out, target


def normalizer(normalization="minmax"):
    """The batch's last step: 'minmax' = RescaleIntensity((0, 1)) as in train.py:50,58; 'percentile' = torchio's MRI recipe
    RescaleIntensity((0, 1), percentiles=(0.5, 99.5)); 'znorm' = ZNormalization(masking_method=ZNormalization.mean).  A
    `HistogramStandardization` instance stands for itself, and a list [HistogramStandardization(...), one of the three strings] gives the list
    of the two transforms (torchio's recipe is the instance followed by 'znorm').  A dict {"histogram": {landmarks, masking_method, cutoff,
    epsilon}, "then": string} is the configuration-file form of that list; `then` is optional."""
    if isinstance(normalization, HistogramStandardization):
        return normalization
    if isinstance(normalization, dict):
        if "histogram" not in normalization or set(normalization) - {"histogram", "then"}:
            raise ValueError(f"normalization as a dict is {{'histogram': {{...}}, 'then': 'znorm' | 'percentile' | 'minmax'}}, not {normalization!r}")
        first = HistogramStandardization(**normalization["histogram"])
        return [first] + ([normalizer(str(normalization["then"]))] if normalization.get("then") is not None else [])
    if isinstance(normalization, (list, tuple)):
        if len(normalization) != 2 or not isinstance(normalization[0], HistogramStandardization) or not isinstance(normalization[1], str):
            raise ValueError(f"normalization as a list is [HistogramStandardization(...), 'znorm' | 'percentile' | 'minmax'], not {normalization!r}")
        return [normalization[0], normalizer(normalization[1])]
    if normalization == "minmax":
        return RescaleIntensity((0, 1))
    if normalization == "percentile":
        return RescaleIntensity((0, 1), percentiles=(0.5, 99.5))
    if normalization == "znorm":
        return ZNormalization(masking_method=ZNormalization.mean)
    raise ValueError(f"normalization is 'minmax', 'percentile' or 'znorm' (or a HistogramStandardization, alone or in a list before one of "
                     f"them), not {normalization!r}")


def _normalizers(normalization) -> list:
    n = normalizer(normalization)
    return list(n) if isinstance(n, list) else [n]


def train_transforms(seed: Optional[int] = None, intensity: bool = False, motion: bool = False, elastic: bool = False,
                     normalization="minmax", artifacts: bool = False) -> DeviceCompose:
    """train.py:38-52.  The shipped script declares an intensity_augment dict (43-48) and leaves its `tio.OneOf(intensity_augment, p=0.75)`
    line (51) commented out, so the default here has no intensity transform.  intensity=True switches that line on, on the device, with
    the three members this package had first (RandomMotion's 0.25 spread over them); motion=True as well makes it the reference's dict
    as declared, four members at 0.25.  elastic=True (not in the reference) replaces the affine by torchio's documented recipe, the affine
    in 0.8 and RandomElasticDeformation() in 0.2 of the samples that the group's p = 0.5 selects.  normalization picks the last step
    (`normalizer`); it draws nothing, so the random stream does not depend on it.  artifacts=True (not in the reference) adds torchio's other
    MRI artifacts, RandomGhosting(), RandomSpike(), RandomGamma() and RandomAnisotropy() with their defaults, to the intensity group, every
    member of the group at the same weight: 1/7 each, 1/8 each with motion=True."""
    if motion and not intensity:
        raise ValueError("train_transforms: motion=True adds RandomMotion to the intensity group and needs intensity=True")
    if artifacts and not intensity:
        raise ValueError("train_transforms: artifacts=True adds RandomGhosting, RandomSpike, RandomGamma and RandomAnisotropy to the intensity group "
                         "and needs intensity=True")
    affine = OneOf({RandomAffine(degrees=15): 0.8, RandomElasticDeformation(): 0.2}, p=0.5) if elastic else RandomAffine(degrees=15, p=0.5)
    spatial = [affine, RandomFlip(axes=(0,), flip_probability=0.5)]
    group = {RandomNoise(): 1, RandomBiasField(): 1, RandomBlur(std=(0, 1.5)): 1}
    if motion:
        group = {RandomNoise(): 0.25, RandomBiasField(): 0.25, RandomBlur(std=(0, 1.5)): 0.25, RandomMotion(): 0.25}
    if artifacts:
        group = {t: 1 for t in list(group) + [RandomGhosting(), RandomSpike(), RandomGamma(), RandomAnisotropy()]}
    one_of = [OneOf(group, p=0.75)] if intensity else []
    return DeviceCompose(spatial + one_of + _normalizers(normalization), seed)


def eval_transforms(normalization="minmax") -> DeviceCompose:
    """train.py:54-60: val and test."""
    return DeviceCompose(_normalizers(normalization))


class DataPreprocessor:
    """train.py:33-78: same CSV columns (`subset`, `mri_path`, `kl_grade`), same loaders and return tuple; the transforms are the
    device-side `train_transforms` / `val_transforms` attributes to call on each batch after `.to(device)`.  config['data']['intensity_augment']
    (default False) adds the intensity OneOf of `train_transforms(intensity=True)`, config['data']['motion_augment'] (default False)
    RandomMotion to it (`motion=True`), config['data']['elastic_augment'] (default False) puts the affine / elastic OneOf of
    `train_transforms(elastic=True)` in place of the affine, config['data']['normalization'] (default 'minmax'; 'percentile', 'znorm') picks
    the last step of all three splits (`normalizer`; a dict {"histogram": {"landmarks": path, "masking_method": ..., "cutoff": ...}, "then":
    "znorm"} puts a `HistogramStandardization` before it, `then` is optional and without it nothing follows), config['data']['artifact_augment'] (default False) adds RandomGhosting, RandomSpike,
    RandomGamma and RandomAnisotropy to the intensity OneOf (`artifacts=True`; it needs intensity_augment).  config['data']['batch_mix'] (absent by
    default: `batch_mix` is None) is a dict of `BatchMix` arguments and builds the `batch_mix` attribute, to call on the training batch and its
    labels after `train_transforms`.  config['data']['conform'] (absent by default: `conform` is None and nothing changes) is a dict with
    target_shape and spacing (`Resample`) or resize (`Resize`), optionally image_interpolation, antialias, padding_mode and spacing_key
    (`conform_from_config`): the loaders then read raw volumes of any shape (`VolumeDataset` + `collate_ragged`, batches are
    (RaggedBatch, labels)) and the `conform` attribute brings a batch onto the grid, `x = pre.conform(ragged.to(device))`, before
    `train_transforms` / `val_transforms`."""

    def __init__(self, config, seed: Optional[int] = None):
        self.config = config
        intensity = bool(config["data"].get("intensity_augment", False))
        motion = bool(config["data"].get("motion_augment", False))
        elastic = bool(config["data"].get("elastic_augment", False))
        norm = config["data"].get("normalization", "minmax")
        artifacts = bool(config["data"].get("artifact_augment", False))
        self.train_transforms, self.val_transforms, self.test_transforms = (train_transforms(seed, intensity, motion, elastic, norm, artifacts=artifacts),
                                                                            eval_transforms(norm), eval_transforms(norm))
        mix = config["data"].get("batch_mix")
        self.batch_mix = BatchMix(**mix) if mix is not None else None
        conform = config["data"].get("conform")
        self.conform = conform_from_config(conform) if conform is not None else None

    def preprocess(self, df=None):
        import pandas as pd
        d = self.config["data"]
        df = pd.read_csv(d["data_path"])
        sub = {s: df[df["subset"] == s].reset_index(drop=True) for s in ("train", "val", "test")}
        if self.conform is not None:
            ds = {s: VolumeDataset(sub[s], image_folder=d["image_folder"], spacing_key=d["conform"].get("spacing_key", "spacing")) for s in sub}
            mk = lambda s, shuffle: DataLoader(ds[s], batch_size=d["batch_size"], shuffle=shuffle, num_workers=d["num_workers"], pin_memory=True,  # noqa: E731
                                               collate_fn=collate_ragged)
            return mk("train", True), mk("val", False), mk("test", False), ds["train"], ds["val"], ds["test"]
        ds = {s: CustomDataset(sub[s], transforms=None, image_folder=d["image_folder"]) for s in sub}
        mk = lambda s, shuffle: DataLoader(ds[s], batch_size=d["batch_size"], shuffle=shuffle, num_workers=d["num_workers"], pin_memory=True)  # noqa: E731
        return mk("train", True), mk("val", False), mk("test", False), ds["train"], ds["val"], ds["test"]
