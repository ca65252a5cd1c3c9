"""
Float64 model of the `spatial` filter (flam3's spatial filter + supersample decimation; DESIGN.md §4.7, include/flame_hip.h
fl_resample), written from the definition and independent of cuburn_amd/filters.py and csrc/resample.hip.
"""
import numpy as np

GUTTER = 12
SUPPORT = 1.5


def ntaps(radius, ss):
    fw = 2.0 * SUPPORT * ss * radius
    n = int(fw) + 1
    if (n ^ ss) & 1:
        n += 1
    return max(n, ss)


def taps(radius, ss):
    """The taps per axis in float64 (unrounded), normalised to sum 1."""
    n = ntaps(radius, ss)
    fw = 2.0 * SUPPORT * ss * radius
    adjust = SUPPORT * n / fw if fw > 0 else 1.0
    t = np.empty(n, np.float64)
    for i in range(n):
        x = ((2 * i + 1) / float(n) - 1.0) * adjust
        t[i] = np.exp(-2.0 * x * x) * np.sqrt(2.0 / np.pi)
    return t / t.sum()


def _axis(a, t, ss, nout, axis):
    """out[X] = sum_i t[i] * a[12 + ss * (X - 12) - g + i] along `axis`, zero outside a."""
    n = len(t)
    g = (n - ss) // 2
    a = np.moveaxis(a, axis, 0)
    lo = GUTTER * ss + g                                        # -(first index read by X = 0) + 12, and then some
    hi = max(0, GUTTER + ss * (nout - 1 - GUTTER) - g + n - a.shape[0])
    pad = np.zeros((lo + a.shape[0] + hi,) + a.shape[1:], np.float64)
    pad[lo:lo + a.shape[0]] = a
    out = np.zeros((nout,) + a.shape[1:], np.float64)
    for i in range(n):
        first = lo + GUTTER - ss * GUTTER - g + i                # X = 0
        out += t[i] * pad[first:first + ss * (nout - 1) + 1:ss]
    return np.moveaxis(out, 0, axis)


def resample(src, dim_in, dim_out, ss, t):
    """``src``: (ah_in * astride_in, 4) or (ah_in, astride_in, 4).  Returns ``(out, A)``, both (ah_out, astride_out, 4) float64:
    the filtered buffer and A = sum_j sum_i |t_j| |t_i| |src| per bin and channel, the scale of its float32 rounding error."""
    t = np.asarray(t, np.float64)
    assert (len(t) - ss) % 2 == 0 and len(t) >= ss
    a = np.asarray(src, np.float64).reshape(dim_in.ah, dim_in.astride, 4)
    out = _axis(_axis(a, t, ss, dim_out.astride, 1), t, ss, dim_out.ah, 0)
    A = _axis(_axis(np.abs(a), np.abs(t), ss, dim_out.astride, 1), np.abs(t), ss, dim_out.ah, 0)
    return out, A


def resample_direct(src, dim_in, dim_out, ss, t, bins):
    """The double sum of the definition, literally, for a few (X, Y) ``bins`` (checks the separable form above)."""
    t = np.asarray(t, np.float64)
    n = len(t)
    g = (n - ss) // 2
    a = np.asarray(src, np.float64).reshape(dim_in.ah, dim_in.astride, 4)
    res = []
    for X, Y in bins:
        acc = np.zeros(4)
        for j in range(n):
            sy = GUTTER + ss * (Y - GUTTER) - g + j
            for i in range(n):
                sx = GUTTER + ss * (X - GUTTER) - g + i
                if 0 <= sy < dim_in.ah and 0 <= sx < dim_in.astride:
                    acc += t[j] * t[i] * a[sy, sx]
        res.append(acc)
    return np.array(res)
