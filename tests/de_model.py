"""
numpy model of the `de` filter (flam3-style adaptive density estimation), in scatter form and
float64: the contract the HIP kernel (cuburn_amd/csrc/de_adaptive.hip) is held to.  de_gather_at is a second,
independent float64 form of the same contract (gather form, written from the DESIGN.md §4.6 text), and
kernel_exponent restates the float32 arithmetic of the kernel's disc test.
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


# ---------------------------------------------------------------- gather form, from the DESIGN.md §4.6 text
MAX_RADIUS = 96                     # FL_DE_MAX_RADIUS: no disc is wider, so no source farther away reaches


def disc_norm(m):
    """S(h) for h = m / 16: exp(-4.5 d^2 / h^2) summed over the integer offsets with d^2 <= h^2.  h = m / 16 and h^2 are
    exact in float64, so the disc test is exact."""
    h = m / 16.0
    I = int(h)
    j, i = np.mgrid[-I:I + 1, -I:I + 1]
    d2 = (i * i + j * j).astype(np.float64)
    return np.exp(-4.5 * d2[d2 <= h * h] / (h * h)).sum()


def disc_weights(m):
    """The weights of one bin with 16 h = m >= 16 over the offsets [-I, I]^2, I = floor(h), normalised by disc_norm."""
    h = m / 16.0
    I = int(h)
    j, i = np.mgrid[-I:I + 1, -I:I + 1]
    d2 = (i * i + j * j).astype(np.float64)
    return np.where(d2 <= h * h, np.exp(-4.5 * d2 / (h * h)), 0.0) / disc_norm(m)


def de_gather_at(buf, R, Rmin, curve, points):
    """The filter's output at the given pixels, in float64 and gather form: out[p] is the sum, over the sources q within
    96 px of p whose own disc holds p (|p - q|^2 <= h_q^2, h_q >= 1), of in[q] exp(-4.5 |p - q|^2 / h_q^2) / S(h_q), plus
    in[p] itself when p stays where it is (w_p <= 0, R <= 0 or h_p < 1).  h_q = clamp(R max(w_q, 1)^-curve, Rmin, R)
    rounded to the nearest 1/16, in double.  buf: (H, W, 4) float32; points: (N, 2) of (y, x).  Returns (N, 4)."""
    H, W = buf.shape[:2]
    R, curve = float(np.float32(R)), float(np.float32(curve))
    Rmin = min(max(float(np.float32(Rmin)), 0.0), R)
    w = buf[..., 3].astype(np.float64)
    h = np.zeros((H, W))
    live = w > 0
    if R > 0:
        h[live] = np.floor(16.0 * np.clip(R * np.maximum(w[live], 1.0) ** -curve, Rmin, R) + 0.5) / 16.0
    spread = h >= 1.0
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    py, px = pts[:, 0], pts[:, 1]
    out = np.where(spread[py, px], 0.0, 1.0)[:, None] * buf[py, px].astype(np.float64)
    if not spread.any():
        return out
    # offsets beyond the widest disc (h <= 96), or beyond the buffer, reach nothing
    hmax = h.max()
    I = min(int(hmax), MAX_RADIUS)
    inv_s = np.zeros((H, W))
    for m in np.unique(np.rint(16.0 * h[spread]).astype(np.int64)):
        inv_s[spread & (h == m / 16.0)] = 1.0 / disc_norm(int(m))
    h2 = np.where(spread, h * h, -1.0)                     # d^2 <= h2 is the disc test, never true for a bin that stays
    coef = -4.5 / np.where(spread, h * h, 1.0)
    # padded by I with sources that stay (and are 0), so that every offset of every point indexes in bounds
    Wp = W + 2 * I
    h2p = np.pad(h2, I, constant_values=-1.0).ravel()
    coefp = np.pad(coef, I).ravel()
    invp = np.pad(inv_s, I).ravel()
    srcp = np.pad(buf.astype(np.float64), ((I, I), (I, I), (0, 0))).reshape(-1, 4)
    base = (py + I) * Wp + (px + I)
    Iy, Ix = min(I, H - 1), min(I, W - 1)
    for dy in range(-Iy, Iy + 1):
        for dx in range(-Ix, Ix + 1):
            d2 = float(dy * dy + dx * dx)
            if d2 > hmax * hmax:
                continue
            q = base + (dy * Wp + dx)
            ok = d2 <= h2p[q]
            if not ok.any():
                continue
            q = q[ok]
            out[ok] += srcp[q] * (np.exp(d2 * coefp[q]) * invp[q])[:, None]
    return out


# ---------------------------------------------------------------- the kernel's float32 arithmetic
# de_adaptive.hip: kA = (float)(-4.5 * 1.4426950408889634 * 256.0); kCut = (float)(-4.5 * 1.4426950408889634 * (1.0 + 1e-6))
KERNEL_A = np.float32(-4.5 * 1.4426950408889634 * 256.0)
KERNEL_CUT = np.float32(-4.5 * 1.4426950408889634 * (1.0 + 1e-6))


def kernel_exponent(m, dx2, dy2):
    """The exponent k_de_gather computes for a source with 16 h = m at squared offsets (dx2, dy2), in float32 as the
    kernel does it (de_adaptive.o is built without fast math and with -ffp-contract=off):
      a = kA / (float)(m * m)        IEEE division; m * m < 2^24 is exact in float32;
      t = a * (float)(dx * dx)       rounded once;
      e = fmaf(a, dy * dy, t)        the exact a * dy^2 + t, rounded once.
    fmaf is emulated by forming a * dy^2 + t in float64 and rounding that once to float32.  The float64 sum is exact:
    a has 24 significant bits and dy^2 <= 97^2 < 2^14, so a * dy^2 fits in 38 bits; t is 0 or a float32 of a's sign no
    smaller than |a|, so both terms are multiples of ulp(a), and their sum, below |a| 2^15, needs at most 40 bits.
    Rounding the exact value once is what fmaf does."""
    a = np.float32(KERNEL_A / np.float32(m * m))
    t = (a * np.asarray(dx2, np.float32)).astype(np.float32)
    return (np.float64(a) * np.asarray(dy2, np.float64) + t.astype(np.float64)).astype(np.float32)


def near_half_densities(R, curve, lo=1e-9, hi=1e-5):
    """float32 densities w >= 1 whose 16 h = 16 (R w^-curve), in float64 as radii16 computes it, lies between lo and hi
    below or above a rounding half k + 1/2, 15 <= k < 16 R: where the m a bin gets depends on h being computed in double.
    Returns (w, below), below: 16 h < k + 1/2."""
    R, curve = float(np.float32(R)), float(np.float32(curve))
    t = np.arange(15, int(16 * R)) + 0.5
    bits = np.float32((16.0 * R / t) ** (1.0 / curve)).view(np.int32)
    w = (bits[:, None] + np.arange(-512, 513, dtype=np.int32)).view(np.float32)     # float32 neighbours of each half
    d = 16.0 * (R * np.maximum(w.astype(np.float64), 1.0) ** -curve) - t[:, None]
    keep = (np.abs(d) >= lo) & (np.abs(d) <= hi) & (w >= 1)
    return w[keep], d[keep] < 0


def radii16_float(w, R, Rmin, curve):
    """16 h as a float32 pow and float32 rounding would give it: what the contract rules out (radii16 is the contract)."""
    h = np.float32(R) * np.power(np.maximum(np.asarray(w, np.float32), np.float32(1)), np.float32(-np.float32(curve)))
    h = np.clip(h, np.float32(Rmin), np.float32(R))
    m = np.floor(np.float32(16) * h + np.float32(0.5)).astype(np.int64)
    return np.where(np.asarray(w) > 0, m, 0)
