"""Host-side reference of tio.RandomElasticDeformation (gaviko_amd/csrc/elastic.hip) in float64 numpy -- test infrastructure, in the style of
tests/motion_ref.py.  The dense displacement is ITK's order-3 BSplineTransform over the image extent written as three 1-D basis matrices
[S_a][n_a] contracted with the coarse field (never the kernel's row-coefficient order), the read is trilinear with a pad value outside
the volume.  torchio and SimpleITK are not installed here: this pins the published definition, not those libraries."""
import numpy as np


def basis_matrix(S: int, n: int) -> np.ndarray:
    """[S][n]: row q holds the weights of the n control points at output index q of an axis with S voxels.  Mesh size M = n - 3,
    h = S / M, u = (q + 0.5) / h, i = min(floor(u), M - 1), t = u - i; control points i..i+3 get the four cubic B-spline pieces."""
    M = n - 3
    assert M >= 1
    u = (np.arange(S, dtype=np.float64) + 0.5) / (S / M)
    i = np.minimum(np.floor(u).astype(np.int64), M - 1)
    t = u - i
    pieces = [(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6]
    out = np.zeros((S, n), dtype=np.float64)
    for j, p in enumerate(pieces):
        out[np.arange(S), i + j] = p
    return out


def dense_field(coarse, shape) -> np.ndarray:
    """coarse [n0][n1][n2][3] (voxels, component a along array axis a) -> d [3][D][H][W]"""
    coarse = np.asarray(coarse, dtype=np.float64)
    B0, B1, B2 = (basis_matrix(S, n) for S, n in zip(shape, coarse.shape[:3]))
    return np.einsum("zi,yj,xk,ijkc->czyx", B0, B1, B2, coarse, optimize=True)


def trilinear_read(vol, pos, pad: float) -> np.ndarray:
    """vol [D][H][W] read at the positions pos [3][...] (voxels); the 8 neighbours weigh in trilinearly, those outside the volume read pad"""
    vol = np.asarray(vol, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.float64)
    base = np.floor(pos)
    frac = pos - base
    base = base.astype(np.int64)
    out = np.zeros(pos.shape[1:], dtype=np.float64)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                idx = [base[0] + dz, base[1] + dy, base[2] + dx]
                ok = np.ones(out.shape, dtype=bool)
                for a in range(3):
                    ok &= (idx[a] >= 0) & (idx[a] < vol.shape[a])
                v = np.where(ok, vol[tuple(np.clip(idx[a], 0, vol.shape[a] - 1) for a in range(3))], pad)
                w = (frac[0] if dz else 1 - frac[0]) * (frac[1] if dy else 1 - frac[1]) * (frac[2] if dx else 1 - frac[2])
                out += w * v
    return out


def grid(shape) -> np.ndarray:
    """[3][D][H][W]: the voxel indices"""
    return np.stack(np.meshgrid(*(np.arange(S, dtype=np.float64) for S in shape), indexing="ij"))


def deform(vol, coarse, pad=None) -> np.ndarray:
    """The whole transform in float64: out[q] = vol read at q + d(q); pad defaults to the volume minimum."""
    vol = np.asarray(vol)
    pad = float(vol.min()) if pad is None else pad
    return trilinear_read(vol, grid(vol.shape) + dense_field(coarse, vol.shape), pad)


def apply(vol, coarse) -> np.ndarray:
    """One `DeviceCompose.last_elastic` entry (None or the coarse field) on a volume, in float64."""
    return np.asarray(vol, dtype=np.float64) if coarse is None else deform(vol, coarse)
