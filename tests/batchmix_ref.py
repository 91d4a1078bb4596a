"""Float64 restatements of gvk_batch_mix's three modes and of BatchMix's box rule (a helper, not a test).

Written from the definitions, not from the kernel: a sample is copied, blended with its partner, or has the partner pasted into a half-open
box.  Copy and CutMix move values and are compared bit for bit; Mixup is evaluated in float64 with lam taken as the float32 value the kernel
reads, and `mixup_bound` is the elementwise rounding bound of its float32 evaluation."""
import numpy as np

COPY, MIXUP, CUTMIX = 0, 1, 2


def rand_box(lam, centre, shape):
    """timm's rand_bbox on three axes: ((d0, d1, h0, h1, w0, w1), corrected lam), all in Python integers and float64."""
    r = (1.0 - lam) ** (1.0 / 3.0)
    box, vol, V = [], 1, 1
    for c, n in zip(centre, shape):
        s = int(n * r)
        lo, hi = min(max(c - s // 2, 0), n), min(max(c + s // 2, 0), n)
        box += [lo, hi]
        vol *= hi - lo
        V *= n
    return tuple(box), 1.0 - vol / V


def mix(x, mode, lam, perm, box):
    """x [B][D][H][W] -> float64 [B][D][H][W].  Dead samples' lam, perm and box entries are not looked at."""
    x = np.asarray(x)
    out = np.empty(x.shape, dtype=np.float64)
    for b in range(x.shape[0]):
        if mode[b] == COPY:
            out[b] = x[b]
        elif mode[b] == MIXUP:
            l = np.float64(np.float32(lam[b]))
            out[b] = l * x[b].astype(np.float64) + (1.0 - l) * x[perm[b]].astype(np.float64)
        else:
            d0, d1, h0, h1, w0, w1 = [int(v) for v in box[b]]
            out[b] = x[b]
            out[b, d0:d1, h0:h1, w0:w1] = x[perm[b], d0:d1, h0:h1, w0:w1]
    return out


def mixup_bound(x, lam, perm, b):
    """3.01 * 2^-24 * (|lam x_a| + |(1 - lam) x_b|) for sample b: one rounding for 1 - lam, one per product, one for the sum -- the second term
    sees three of them; the 0.01 covers the second-order terms."""
    l = np.float64(np.float32(lam[b]))
    return 3.01 * 2.0 ** -24 * (np.abs(l * x[b].astype(np.float64)) + np.abs((1.0 - l) * x[perm[b]].astype(np.float64)))
