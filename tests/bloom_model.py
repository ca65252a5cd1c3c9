"""
The `bloom` filter in numpy float64, written from its definition, for tests/test_cpu_bloom.py and
tests/test_gpu_bloom.py.  It shares nothing with cuburn_amd.filters: the taps are derived here again.

A bin (r, g, b, w) of the ah x astride buffer has the excess E = f (r, g, b, w), f = (w - t) / w where w > t and 0 elsewhere
(a NaN w: 0).  E is blurred along x, then along y, with the taps exp(-i^2 / (2 sigma^2)), i = -R .. R, R = ceil(3 sigma),
normalised to sum 1 in float64 and rounded to float32 (sigma 0: the single tap 1); taps that fall outside the buffer read
zero.  The result is in + strength * blur(E) on all four channels.
"""
import numpy as np

MAX_REACH = 384


def reach(sigma):
    return int(np.ceil(3.0 * float(sigma)))


def taps(sigma):
    """The 2 R + 1 taps as float64 values of float32 numbers."""
    R = reach(sigma)
    if R == 0:
        return np.ones(1)
    i = np.arange(-R, R + 1, dtype=np.float64)
    t = np.exp(-i * i / (2.0 * float(sigma) ** 2))
    return (t / t.sum()).astype(np.float32).astype(np.float64)


def params(threshold, strength, sigma):
    """[threshold, strength, tap_0 .. tap_R]: the scalars of the fl_filter call."""
    t = taps(sigma)
    return [np.float32(threshold), np.float32(strength)] + [np.float32(v) for v in t[len(t) // 2:]]


def excess(buf, threshold):
    """E of an (ah, astride, 4) buffer, float64.  The threshold is the float32 the device receives."""
    b = np.asarray(buf, np.float32).astype(np.float64)
    w = b[..., 3]
    t = float(np.float32(threshold))
    with np.errstate(invalid='ignore', divide='ignore'):
        f = np.where(w > t, (w - t) / np.where(w > t, w, 1.0), 0.0)
    return f[..., None] * b


def blur_axis(a, t, axis):
    """Correlation with the symmetric taps t along one axis of a; beyond the array: zero."""
    R = len(t) // 2
    n = a.shape[axis]
    out = np.zeros_like(a)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    for i in range(-R, R + 1):
        if abs(i) >= n:
            continue
        # out[p] += t[i] a[p + i]
        dst[axis] = slice(max(0, -i), min(n, n - i))
        src[axis] = slice(max(0, i), min(n, n + i))
        out[tuple(dst)] += t[i + R] * a[tuple(src)]
    return out


def blur(a, sigma):
    t = taps(sigma)
    return blur_axis(blur_axis(a, t, 1), t, 0)


def bloom(buf, threshold, strength, sigma):
    """(out, blurred |E|) of an (ah, astride, 4) buffer: the model and what the device's bar is taken from."""
    b = np.asarray(buf, np.float32).astype(np.float64)
    E = excess(buf, threshold)
    s = float(np.float32(strength))
    return b + s * blur(E, sigma), blur(np.abs(E), sigma)


def bar(out, blur_abs, strength, sigma):
    """(2 ntaps + 16) 2^-24 strength blur(|E|) + 2 * 2^-24 |out|: ntaps float32 multiply-adds per pass in any order, a few
    ulp for the division in E and for the final add."""
    ntaps = 2 * reach(sigma) + 1
    return (2 * ntaps + 16) * 2.0 ** -24 * abs(float(np.float32(strength))) * blur_abs + 2 * 2.0 ** -24 * np.abs(out)
