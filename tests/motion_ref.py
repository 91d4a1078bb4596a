"""Host-side reference of tio.RandomMotion (gaviko_amd/csrc/motion.hip, data.motion_tables) in float64 numpy -- test infrastructure, in the
style of tests/intensity_ref.py.  `composite` is torchio's algorithm written literally with np.fft: the shifted n-dimensional spectrum of
every image, sort_spectra, a slab copy along the last axis, the inverse transform, the real part.  It never uses the circular-convolution
restatement the kernel is built on, so agreement pins that restatement as well as the kernel.  torchio is not installed here: this pins
the published algorithm, not torchio itself."""
import numpy as np

from oracle import data_ref


def _spectrum(a):
    return np.fft.fftshift(np.fft.fftn(np.fft.ifftshift(a)))


def _image(s):
    return np.fft.fftshift(np.fft.ifftn(np.fft.ifftshift(s)))


def sort_spectra(spectra, times):
    """torchio's: the original spectrum (entry 0) changes places with the first one whose time is above 0.5, or with the last one."""
    late = np.nonzero(np.asarray(times) > 0.5)[0]
    index = int(late.min()) if len(late) else len(spectra) - 1
    spectra[0], spectra[index] = spectra[index], spectra[0]


def composite(images, times):
    """images: the unmoved array and one array per movement, any number of axes; times: the sorted movement times in (0, 1)."""
    times = np.asarray(times, dtype=np.float64)
    spectra = [_spectrum(np.asarray(im, dtype=np.float64)) for im in images]
    assert len(spectra) == len(times) + 1
    sort_spectra(spectra, times)
    result = np.empty_like(spectra[0])
    last = result.shape[-1]
    indices = (last * times).astype(int).tolist() + [last]
    ini = 0
    for spectrum, fin in zip(spectra, indices):
        result[..., ini:fin] = spectrum[..., ini:fin]
        ini = fin
    return _image(result).real


def moved_images(vol, degrees, translation):
    """[vol, vol under movement 1, ..]: oracle.data_ref.affine_resample through data.affine_matrix at unit scale, padded with the minimum."""
    from gaviko_amd import data
    pad = float(vol.min())
    mats = [data.affine_matrix((1, 1, 1), d, t, vol.shape).astype(np.float32) for d, t in zip(degrees, translation)]
    return [vol] + [data_ref.affine_resample(vol, m, pad) for m in mats]


def apply(vol, draw):
    """One `DeviceCompose.last_intensity` entry ("RandomMotion", params) on a float32 volume, in float64."""
    name, p = draw
    assert name == "RandomMotion"
    return composite(moved_images(vol, p["degrees"], p["translation"]), p["times"])


def abs_convolution(ctab, images):
    """sum_s |c_s| (*) |img_s| along the last axis (circular), float64: the magnitude that the rounding of an fp32 dot product scales with."""
    W = images[0].shape[-1]
    idx = (np.arange(W)[None, :] - np.arange(W)[:, None]) % W          # [w'][w] -> (w - w') mod W
    total = np.zeros(images[0].shape, dtype=np.float64)
    for c, im in zip(np.asarray(ctab, dtype=np.float64), images):
        total += np.abs(np.asarray(im, dtype=np.float64)) @ np.abs(c)[idx]
    return total
