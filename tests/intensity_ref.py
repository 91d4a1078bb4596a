"""Host-side restatement of the intensity kernels (gaviko_amd/csrc/intensity.hip) in numpy / scipy -- test infrastructure, in the style
of tests/dropmask.py.  Everything is float64: the noise field rebuilt from the counter hash, the bias field, the blur as
scipy.ndimage.gaussian_filter with its defaults, and the weight table as scipy builds it.  torchio is not installed here, so these pin
the kernels against the published algorithms, not against torchio itself."""
import numpy as np

from dropmask import hash_u32


def noise_z(seed: int, n: int) -> np.ndarray:
    """z(i), i < n: Box-Muller on hash_u32(seed, 2i) and hash_u32(seed, 2i + 1); u1 in (0, 1], u2 in [0, 1), both multiples of 2^-24."""
    i = np.arange(n, dtype=np.uint64)
    u1 = ((hash_u32(seed, np.uint64(2) * i) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (hash_u32(seed, np.uint64(2) * i + np.uint64(1)) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise(vol: np.ndarray, std: float, mean: float, seed: int) -> np.ndarray:
    """x + (std z + mean) with std and mean as the float32 values the kernel receives."""
    return vol.astype(np.float64) + (float(np.float32(std)) * noise_z(seed, vol.size).reshape(vol.shape) + float(np.float32(mean)))


def bias_terms(order: int):
    return [(a, b, c) for a in range(order + 1) for b in range(order + 1 - a) for c in range(order + 1 - a - b)]


def bias_field(shape, coefficients, order: int) -> np.ndarray:
    """exp(sum_j coeff[j] c0^a c1^b c2^c), ck = (k - (n-1)/2) / ((n-1)/2) along array axis k (0 when n = 1); the coefficients are the
    float32 values the kernel receives."""
    axes = []
    for n in shape:
        h = (n - 1) / 2.0
        axes.append((np.arange(n, dtype=np.float64) - h) / h if n > 1 else np.zeros(1))
    c0, c1, c2 = np.meshgrid(*axes, indexing="ij")
    P = np.zeros(shape, dtype=np.float64)
    coeff = np.asarray(coefficients, dtype=np.float32).astype(np.float64)
    for j, (a, b, c) in enumerate(bias_terms(order)):
        P += coeff[j] * c0 ** a * c1 ** b * c2 ** c
    return np.exp(P)


def bias(vol: np.ndarray, coefficients, order: int) -> np.ndarray:
    return vol.astype(np.float64) * bias_field(vol.shape, coefficients, order)


def blur(vol: np.ndarray, sigmas) -> np.ndarray:
    from scipy import ndimage
    return ndimage.gaussian_filter(vol.astype(np.float64), sigma=tuple(float(s) for s in sigmas))


def weight_table(sigma: float):
    """(radius, weights float64 [2 radius + 1]) of one axis as scipy.ndimage.gaussian_filter1d builds them (truncate = 4.0); radius 0 with the
    single weight 1 for an axis scipy skips (sigma <= 1e-15)."""
    if sigma <= 1e-15:
        return 0, np.ones(1)
    r = int(4.0 * sigma + 0.5)
    k = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return r, w / w.sum()


def apply(vol: np.ndarray, draw) -> np.ndarray:
    """One `DeviceCompose.last_intensity` entry (None or (name, params)) on a float volume, in float64."""
    if draw is None:
        return vol.astype(np.float64)
    name, p = draw
    if name == "RandomNoise":
        return noise(vol, p["std"], p["mean"], p["seed"])
    if name == "RandomBiasField":
        return bias(vol, p["coefficients"], p["order"])
    if name == "RandomBlur":
        return blur(vol, p["std"])
    raise ValueError(name)
