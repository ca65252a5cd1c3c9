"""
One direction of the bilateral density estimation in float64 numpy: cuburn's den_blur -> den_blur_1c -> bilateral
(cuburn/code/filters.py:106-131, 166-264; the float32 oracle's ref_den_blur -> ref_den_blur_1c -> ref_bilateral_impl is the
same thing), restated literally and vectorised over pixels.  What the device kernel (cuburn_amd/csrc/de.hip) regroups, hoists
or tabulates is written here the way the reference evaluates it, per fetch:

  * every fetch is clamped to the padded frame, the tap offset rne(slope * r) is taken per fetch and added to the pixel's
    position before the clamp;
  * the blurred density of a tap is the value of the blurred plane AT the clamped position (each blur is a plane of its own,
    computed with clamped fetches from the plane before it);
  * the centre's colour is x / (w + 1e-6), a tap's x / w; a pair with a dead member (w <= 0) has colour distance 0.5;
  * w^dpow with w^0 = 1 (also 0^0);
  * the gradient factor is left out at r = 0;
  * the result is the weighted sum times 1 / (weightsum + 1e-10).

The inputs are float32 values (images, scalars, the seven blur coefficients) taken to float64 exactly; every constant the
product computes in float32 on the host (the spatial table's sqrt2, the blur coefficients) enters with its float32 value.

Forms of an image: `raw` (x, y, z, w) as the accumulator holds it, and the kernel's normalised form N = (x / w, y / w, z / w, w)
with (0, 0, 0, w) where w <= 0 (csrc/de.hip de_in_px).  Direction 0 reads raw and writes N, directions 1..6 read and write N,
direction 7 reads N and writes raw.
"""
import numpy as np

PATTERNS = [(1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (-1.0, 1.0), (1.0, 0.5), (-0.5, 1.0), (1.0, -0.5), (0.5, 1.0)]   # cuburn/code/filters.py:8-17
RM_SQRT2 = float(np.float32(1.41421353816986))
RADIUS = 15
# Below this weighted density sum a float32 evaluation has lost terms to flush-to-zero (the reference runs with -ftz, the
# kernels and the oracle likewise): each of the 31 terms f * w that falls below 2^-126 is dropped, with w <= 64 that is a term
# below 2^-120 of the sum's own scale per dropped factor f, so a sum S misses at most 31 * 2^-120 / S of itself: 2^-25 at
# S = 2^-90.  The normalised COLOUR of such a pixel (a ratio of two such sums) is not a statement about the kernel and is NaN
# in `normalised_out`; its density is compared everywhere (it is far below the absolute term of any bar).
S_MIN = 2.0 ** -90


def gauss7(stdev=1.0):
    """The product's and the oracle's seven blur coefficients (cuburn/filters.py:11-16), in float32."""
    c = np.exp(np.arange(-3, 4, dtype=np.float32) ** 2 / np.float32(-2.0 * stdev * stdev)).astype(np.float32)
    return (c / np.float32(c.sum(dtype=np.float32))).astype(np.float32)


def tap_offsets(pattern, radii=range(-RADIUS, RADIUS + 1)):
    """[(dx, dy)] of the taps r in `radii`: each component rounded to nearest, ties to even (cvt.rni)."""
    sx, sy = PATTERNS[pattern]
    return [(int(np.rint(sx * r)), int(np.rint(sy * r))) for r in radii]


def to_normalised(raw):
    """raw (..., 4) -> N in float64: what de_in_px makes of an accumulator pixel, exactly."""
    raw = np.asarray(raw, np.float64)
    w = raw[..., 3:4]
    with np.errstate(divide='ignore', invalid='ignore'):
        n = np.where(w > 0, raw[..., :3] / w, 0.0)
    return np.concatenate([n, w], -1)


def to_raw(N):
    """N (..., 4) -> raw in float64 (exact for float32 inputs: 24 + 24 bits)."""
    N = np.asarray(N, np.float64)
    return np.concatenate([N[..., :3] * N[..., 3:4], N[..., 3:4]], -1)


def normalised_out(raw_out, S):
    """The model's result in the form directions 0..6 store: colour = sum f w n / sum f w (0 where the sum is 0, NaN where it
    is positive but below S_MIN, see there), density = raw_out's."""
    raw_out = np.asarray(raw_out, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        n = raw_out[..., :3] / raw_out[..., 3:4]
    n = np.where((S == 0)[..., None], 0.0, np.where((S < S_MIN)[..., None], np.nan, n))
    return np.concatenate([n, raw_out[..., 3:4]], -1)


def _blur(plane, pattern, step, k):
    H, W = plane.shape
    out = np.zeros_like(plane)
    ys, xs = np.arange(H), np.arange(W)
    for i, (dx, dy) in enumerate(tap_offsets(pattern, [(j - 3) * step for j in range(7)])):
        out += plane[np.ix_(np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1))] * k[i]
    return out


def blurs(raw, pattern, coefs=None):
    """(den_blur, den_blur_1c of it) of the density plane of raw (H, W, 4): 7 taps at steps 1 and 2."""
    k = np.asarray(gauss7() if coefs is None else coefs, np.float64)
    b1 = _blur(np.asarray(raw, np.float64)[..., 3], pattern, 1, k)
    return b1, _blur(b1, pattern, 2, k)


def bilateral_at(raw, pattern, scalars, ys, xs, coefs=None):
    """One pass at the pixels (ys[i], xs[i]) of raw (H, W, 4): (raw result (n, 4), S (n,) = sum f * w before the division).
    scalars = sstd, cstd, dstd, dpow, gspeed (float32 values)."""
    raw = np.asarray(raw, np.float64)
    H, W = raw.shape[:2]
    sstd, cstd, dstd, dpow, gspeed = (float(np.float32(v)) for v in scalars)
    ys, xs = np.asarray(ys), np.asarray(xs)
    _, avgp = blurs(raw, pattern, coefs)
    wp = raw[..., 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        npl = np.where(wp[..., None] > 0, raw[..., :3] / wp[..., None], 0.0)
        powp = np.where(wp > 0, np.power(np.maximum(wp, 0.0), dpow), 1.0 if dpow == 0.0 else 0.0)
    cscale, dscale = 1.0 / (-RM_SQRT2 * 3.0 * cstd), -0.5 / dstd
    cw = wp[ys, xs]
    cen = raw[ys, xs, :3] / (cw + 1.0e-6)[:, None]
    cpow = powp[ys, xs]
    clive = cw > 0
    offs = tap_offsets(pattern, range(-RADIUS - 1, RADIUS + 2))
    at = [(np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1)) for dx, dy in offs]      # r = -16 .. 16
    out = np.zeros((len(ys), 4))
    wsum = np.zeros(len(ys))
    S = np.zeros(len(ys))
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for r in range(-RADIUS, RADIUS + 1):
            py, px = at[r + RADIUS + 1]
            pw = wp[py, px]
            d = npl[py, px] - cen
            cdiff = np.where((pw > 0) & clive, (d * d).sum(-1), 0.5)
            f = np.exp(r * r / (-RM_SQRT2 * sstd)) * np.exp(cscale * cdiff) * np.exp2(dscale * np.abs(cpow - powp[py, px]))
            if r != 0:
                g = (wp[at[r + RADIUS + 2]] - wp[at[r + RADIUS]]) / (avgp[py, px] + 1.0e-6)
                f = f * np.exp2(-np.exp2(gspeed * (-g if r < 0 else g)))
            wsum += f
            S += f * pw
            out += f[:, None] * raw[py, px]
    return out / (wsum + 1e-10)[:, None], S


def bilateral_pass(raw, pattern, scalars, coefs=None):
    """One pass over the whole padded frame raw (H, W, 4): (raw result (H, W, 4), S (H, W))."""
    H, W = np.shape(raw)[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    out, S = bilateral_at(raw, pattern, scalars, ys.ravel(), xs.ravel(), coefs)
    return out.reshape(H, W, 4), S.reshape(H, W)


def ratio(x, m):
    """Per channel the worst |x - m| / (|m| + 2^-10 M_c) over the finite model values m (M_c = the channel's largest finite |m|),
    as (worst, its flat pixel index, its channel); a non-finite x where m is finite counts as infinite."""
    x, m = np.asarray(x, np.float64).reshape(-1, 4), np.asarray(m, np.float64).reshape(-1, 4)
    fin = np.isfinite(m)
    M = np.where(fin, np.abs(m), 0.0).max(0)
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.abs(x - m) / (np.abs(m) + 2.0 ** -10 * M)
    q = np.where(fin, np.where(np.isfinite(x), np.nan_to_num(q, nan=0.0), np.inf), 0.0)    # 0 / 0 (an all-zero channel): equal
    i = int(np.argmax(q))
    return float(q.flat[i]), i // 4, i % 4
