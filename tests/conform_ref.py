"""Float64 restatement of gaviko_amd.data.Conform (Resample / Resize, then CropOrPad) in plain numpy loops over the definitions of
INTEGRATION.md; nothing here is derived from data.conform_tables.  Per axis with input length n, spacing s, target length N:

  Resample to spacing t: r = t / s, m = max(1, floor(n / r + 1e-9));  Resize to N: r = n / N, m = N;  position p = (u + 0.5) r - 0.5
  linear: p clamped to [0, n - 1], taps floor(p) and min(floor(p) + 1, n - 1), weights 1 - g and g;  nearest: min(floor(p + 0.5), n - 1)
  antialias (linear, r > 1): a Gaussian of sigma = sqrt((r^2 - 1) / (8 ln 2)), truncated at int(4 sigma + 0.5), normalised, edge repeated, first
  CropOrPad m -> N, d = N - m: pad ceil(d / 2) in front, floor(d / 2) behind; crop ceil(-d / 2) in front, floor(-d / 2) behind

`apply_tables` is the other half the GPU tests need: the float64 evaluation of GIVEN banded tables (the float32-rounded ones the kernel
reads), so that the comparison measures the kernel's arithmetic and not the rounding of the tables."""
import math

import numpy as np


def lengths(n, s, kind, target):
    """(r, m) of one axis: kind 'resample' (target = the spacing t), 'resize' (target = N) or None."""
    if kind == "resample":
        r = target / s
        return r, max(1, int(math.floor(n / r + 1e-9)))
    if kind == "resize":
        return n / target, int(target)
    return 1.0, int(n)


def front_pad(m, N):
    """The signed front pad c of CropOrPad m -> N: output index q is intermediate index q - c."""
    d = N - m
    return int(math.ceil(d / 2)) if d >= 0 else -int(math.ceil(-d / 2))


def gaussian(r):
    """The antialiasing kernel of the factor r > 1: (weights [2 radius + 1], radius)."""
    sigma = math.sqrt((r * r - 1.0) / (8.0 * math.log(2.0)))
    radius = int(4.0 * sigma + 0.5)
    w = [math.exp(-0.5 * (k / sigma) ** 2) for k in range(-radius, radius + 1)]
    total = math.fsum(w)
    return [v / total for v in w], radius


def smooth_line(x, r):
    """One line smoothed along itself (edge value repeated)."""
    w, radius = gaussian(r)
    n = len(x)
    return np.array([math.fsum(w[k + radius] * x[min(max(j + k, 0), n - 1)] for k in range(-radius, radius + 1)) for j in range(n)])


def resample_line(x, r, m, interpolation, antialias):
    """One line of n voxels -> m voxels, float64.  A nearest tap, and a linear tap of weight exactly 1, move the value (signed zeros kept)."""
    n = len(x)
    if interpolation == "linear" and antialias and r > 1.0:
        x = smooth_line(x, r)
    out = np.empty(m, dtype=np.float64)
    for u in range(m):
        p = (u + 0.5) * r - 0.5
        if interpolation == "nearest":
            out[u] = x[min(int(math.floor(p + 0.5)), n - 1)]
            continue
        p = min(max(p, 0.0), float(n - 1))
        i0 = int(math.floor(p))
        i1, g = min(i0 + 1, n - 1), p - i0
        out[u] = x[i0] if g == 0.0 or i1 == i0 else (1.0 - g) * x[i0] + g * x[i1]
    return out


def conform(vol, spacing, kind, target, target_shape, interpolation="linear", antialias=True, pad=0.0):
    """One sample [D][H][W] (any float dtype) onto target_shape, float64.  kind / target as in `lengths` (target a triple); pad a number or
    'minimum' (the input's own minimum).  An axis with r == 1 and m == n is left alone."""
    x = np.asarray(vol, dtype=np.float64)
    pad_value = float(np.min(vol)) if isinstance(pad, str) else float(pad)
    for a in range(3):
        n = x.shape[a]
        r, m = lengths(n, float(spacing[a]), kind, None if kind is None else target[a])
        if kind is None or (r == 1.0 and m == n):
            continue
        moved = np.moveaxis(x, a, -1)
        new = np.empty(moved.shape[:-1] + (m,), dtype=np.float64)
        for i in np.ndindex(*moved.shape[:-1]):
            new[i] = resample_line(moved[i], r, m, interpolation, antialias)
        x = np.moveaxis(new, -1, a)
    out = np.full(tuple(target_shape), pad_value, dtype=np.float64)
    c = [front_pad(x.shape[a], target_shape[a]) for a in range(3)]
    for q0 in range(target_shape[0]):
        for q1 in range(target_shape[1]):
            for q2 in range(target_shape[2]):
                u = (q0 - c[0], q1 - c[1], q2 - c[2])
                if all(0 <= u[a] < x.shape[a] for a in range(3)):
                    out[q0, q1, q2] = x[u]
    return out


def apply_tables(vol, tables, pad):
    """Float64 evaluation of banded tables: tables[a] = (start [N], weights [N][T], inside [N]) along axis a; row q reads the inputs
    start[q] + t with weights[q][t] (taps of weight zero are not read).  A voxel outside on any axis is `pad`."""
    x = np.asarray(vol, dtype=np.float64)
    for a in range(3):
        start, weights, inside = tables[a]
        moved = np.moveaxis(x, a, 0)
        new = np.zeros((len(start),) + moved.shape[1:], dtype=np.float64)
        for q in range(len(start)):
            if inside[q]:
                for t in range(weights.shape[1]):
                    if weights[q, t] != 0:
                        new[q] += np.float64(weights[q, t]) * moved[int(start[q]) + t]
        x = np.moveaxis(new, 0, a)
    out = x.copy()
    for a in range(3):
        idx = [slice(None)] * 3
        idx[a] = ~np.asarray(tables[a][2], dtype=bool)
        out[tuple(idx)] = float(pad)
    return out
