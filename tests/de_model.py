"""
numpy model of the `de` filter (flam3-style adaptive density estimation), in scatter form and
float64: the contract the HIP kernel (cuburn_amd/csrc/de_adaptive.hip) is held to.
"""
import functools

import numpy as np


def radii16(w, R, Rmin, curve):
    """16 h per bin (an integer: h is rounded to 1/16 px), 0 where the bin has no density or R <= 0.
    R, Rmin, curve are the float32 scalars the filter is given."""
    R, curve = float(np.float32(R)), float(np.float32(curve))
    Rmin = min(max(float(np.float32(Rmin)), 0.0), R)
    w = np.asarray(w, np.float64)
    if R <= 0:
        return np.zeros(w.shape, np.int64)
    h = np.clip(R * np.maximum(w, 1.0) ** -curve, Rmin, R)
    m = np.floor(16.0 * h + 0.5).astype(np.int64)
    return np.where(w > 0, m, 0)


@functools.lru_cache(maxsize=None)
def kernel(m):
    """Weights of a bin with 16 h = m >= 16 over the offsets (j, i) in [-I, I]^2, I = m // 16: exp(-4.5 d^2 / h^2)
    on the discrete disc d^2 <= h^2 (tested in integers: 256 d^2 <= m^2), normalised by their own float64 sum."""
    I = m // 16
    j, i = np.mgrid[-I:I + 1, -I:I + 1]
    d2 = i * i + j * j
    k = np.where(256 * d2 <= m * m, np.exp(-4.5 * 256.0 * d2 / float(m * m)), 0.0)
    k /= k.sum()
    k.setflags(write=False)
    return k


def de_filter(buf, R, Rmin, curve):
    """buf: (H, W, 4) float32 accumulator (RGB, density in [..., 3]); returns the filtered (H, W, 4) float64.
    Each bin is scattered over its kernel; weight landing outside the buffer is dropped."""
    H, W = buf.shape[:2]
    src = buf.astype(np.float64)
    m = radii16(buf[..., 3], R, Rmin, curve)
    out = np.zeros((H, W, 4), np.float64)
    stay = m < 16
    out[stay] = src[stay]
    ys, xs = np.nonzero(~stay)
    for y, x in zip(ys, xs):
        mm = int(m[y, x])
        k = kernel(mm)
        I = mm // 16
        y0, y1, x0, x1 = max(y - I, 0), min(y + I + 1, H), max(x - I, 0), min(x + I + 1, W)
        out[y0:y1, x0:x1] += k[y0 - (y - I):y1 - (y - I), x0 - (x - I):x1 - (x - I), None] * src[y, x]
    return out
