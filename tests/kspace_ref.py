"""Host-side references of tio.RandomGhosting / RandomSpike / RandomGamma / RandomAnisotropy (gaviko_amd/csrc/kspace.hip and the table
builders of gaviko_amd/data.py) in float64 numpy -- test infrastructure, in the style of tests/motion_ref.py.  `ghosting_fft` and `spike_fft`
are the algorithms written literally with np.fft on the full 3-D spectrum; they never use the circular-convolution or closed-cosine
restatements the kernels are built on, so agreement pins those restatements as well as the kernels.  torchio is not installed here: this
pins the definitions INTEGRATION.md states, not torchio itself."""
import numpy as np


# ---- ghosting ----------------------------------------------------------------------------------------------------------------------------
def ghosting_fft(vol, num_ghosts: int, axis: int, intensity: float):
    """Every plane j % n == 0 of the shifted spectrum along `axis` times 1 - g, the centre plane N // 2 put back, the real part kept."""
    x = np.asarray(vol, dtype=np.float64)
    if num_ghosts == 0 or intensity == 0:
        return x.copy()
    spectrum = np.fft.fftshift(np.fft.fftn(x))
    N = x.shape[axis]
    planes = np.moveaxis(spectrum, axis, 0)                                # a view
    centre = planes[N // 2].copy()
    planes[::num_ghosts] *= 1.0 - intensity
    planes[N // 2] = centre
    return np.fft.ifftn(np.fft.ifftshift(spectrum)).real


def circular_conv(vol, c, axis: int):
    """y[..i..] = sum_i' c[(i - i') mod N] x[..i'..] along `axis`, float64, with the first N entries of c."""
    x = np.moveaxis(np.asarray(vol, dtype=np.float64), axis, 0)
    N = x.shape[0]
    c = np.asarray(c, dtype=np.float64)[:N]
    circ = c[(np.arange(N)[:, None] - np.arange(N)[None, :]) % N]          # [i][i'] -> (i - i') mod N
    return np.moveaxis(np.tensordot(circ, x, axes=(1, 0)), 0, axis)


def abs_circular_conv(vol, c, axis: int):
    """|c| (*) |x| along `axis`: the magnitude the rounding of an fp32 dot product scales with."""
    return circular_conv(np.abs(np.asarray(vol, dtype=np.float64)), np.abs(np.asarray(c, dtype=np.float64)), axis)


# ---- spikes ------------------------------------------------------------------------------------------------------------------------------
def spike_indices(positions, shape):
    pos = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    return [[min(int(np.floor(p * n)), n - 1) for p, n in zip(row, shape)] for row in pos]


def spike_amplitude(vol, intensity: float) -> float:
    """A / V = g |mean(x)| (float64 mean)"""
    return float(intensity) * abs(float(np.asarray(vol, dtype=np.float64).mean()))


def spike_fft(vol, positions, intensity: float):
    """A = (A / V) V added to the shifted spectrum at floor(pos * N) of every spike, the real part kept."""
    x = np.asarray(vol, dtype=np.float64)
    spectrum = np.fft.fftshift(np.fft.fftn(x))
    for k in spike_indices(positions, x.shape):
        spectrum[tuple(k)] += spike_amplitude(x, intensity) * x.size
    return np.fft.ifftn(np.fft.ifftshift(spectrum)).real


def spike_cosine(vol, positions, intensity: float):
    """The closed form y = x + (A / V) sum_s cos(2 pi sum_a ((k_sa - N_a // 2) x_a mod N_a) / N_a), float64; also returns the bare sum."""
    x = np.asarray(vol, dtype=np.float64)
    total = np.zeros(x.shape, dtype=np.float64)
    for k in spike_indices(positions, x.shape):
        phase = np.zeros(x.shape, dtype=np.float64)
        for a, n in enumerate(x.shape):
            turn = (((k[a] - n // 2) * np.arange(n, dtype=np.int64)) % n) / n
            phase += turn.reshape([-1 if i == a else 1 for i in range(3)])
        total += np.cos(2.0 * np.pi * phase)
    return x + spike_amplitude(x, intensity) * total, total


# ---- gamma -------------------------------------------------------------------------------------------------------------------------------
def gamma(vol, g):
    """sign(x) |x|^gamma in float64, for the float32 gamma the device receives"""
    x = np.asarray(vol, dtype=np.float64)
    return np.copysign(np.power(np.abs(x), float(np.float32(g))), x)


# ---- anisotropy --------------------------------------------------------------------------------------------------------------------------
def anisotropy_coordinates(f: float, N: int):
    """(s0, s1, w) per output index, evaluated voxel by voxel in float64 with Python scalars: a direct statement of the definition."""
    import math
    n_low = max(1, math.ceil(N / f))
    low = [min(max(math.floor(((j + 0.5) * f - 0.5) + 0.5), 0), N - 1) for j in range(n_low)]
    s0, s1, w = [], [], []
    for i in range(N):
        u = min(max((i + 0.5) / f - 0.5, 0.0), float(n_low - 1))
        j0 = math.floor(u)
        s0.append(low[j0])
        s1.append(low[min(j0 + 1, n_low - 1)])
        w.append(u - j0)
    return np.array(s0), np.array(s1), np.array(w, dtype=np.float64)


def anisotropy(vol, axis: int, f: float):
    """The float32 restatement of the kernel's stated form: y = x0 if w == 0 else fmaf(w, x1 - x0, x0), w rounded to float32; the fused
    multiply-add is formed in float64, where the product of two float32 values is exact and, for the integer-valued volumes below 2^12 the
    bit-exact tests use, so is its sum with x0 whenever w is at least 2^-16 (product and x0 then span at most 52 bits); a smaller w moves
    x0 by far less than half a float32 ulp in either arithmetic.  One rounding to float32 follows, as in fmaf."""
    x = np.moveaxis(np.asarray(vol, dtype=np.float32), axis, 0)
    s0, s1, w = anisotropy_coordinates(f, x.shape[0])
    w32 = w.astype(np.float32)
    x0, x1 = x[s0], x[s1]
    diff = (x1 - x0).astype(np.float32)
    wb = w32.reshape(-1, 1, 1)
    y = (wb.astype(np.float64) * diff.astype(np.float64) + x0.astype(np.float64)).astype(np.float32)
    return np.moveaxis(np.where(wb == 0, x0, y), 0, axis)


# ---- DeviceCompose.last_intensity entries ----------------------------------------------------------------------------------------------------
def apply(vol, draw):
    """One ("RandomGhosting" | "RandomSpike" | "RandomGamma" | "RandomAnisotropy", params) entry on a float32 volume."""
    name, p = draw
    if name == "RandomGhosting":
        return ghosting_fft(vol, p["num_ghosts"], p["axis"], p["intensity"])
    if name == "RandomSpike":
        return spike_fft(vol, p["positions"], np.float32(p["intensity"]))
    if name == "RandomGamma":
        return gamma(vol, p["gamma"])
    if name == "RandomAnisotropy":
        return anisotropy(vol, p["axis"], p["downsampling"]).astype(np.float64)
    raise AssertionError(name)
