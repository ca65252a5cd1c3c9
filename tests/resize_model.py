"""
Float64 model of the Lanczos downscale, independent of cuburn_amd/filters.py and of csrc/resize.hip.

Per axis, from n_in source samples to n_out output samples, 1 <= n_in / n_out <= 8, the taps are those of Pillow's
Image.resize(..., LANCZOS) (Resample.c, precompute_coeffs): scale = n_in / n_out, support = 3 * scale; output i has its centre at
c = (i + 0.5) * scale and the window lo = max(0, int(c - support + 0.5)) .. hi = min(n_in, int(c + support + 0.5)) (exclusive), with
the weights L((x - c + 0.5) / scale), L(t) = sinc(t) sinc(t / 3) inside |t| < 3, normalised to sum 1 in float64 — a window cut by
the picture's edge is renormalised, nothing is mirrored — and then rounded to float32.

As a table: nt is the longest window of the axis; row i has nt floats and starts at first[i] = min(lo_i, n_in - nt), its window's
weights at offset lo_i - first[i] with zeros around them, so that 0 <= first[i] and first[i] + nt <= n_in.

The picture: x, then y, all four channels alike, over the picture area only; every bin of the result's padded buffer outside
its picture area is +0.  `resize` also returns A, the resample of |src| with |taps|: the scale of the rounding-error bar
    |dev - model| <= (nxt + nyt + 8) * 2^-24 * A
(nt float32 multiply-adds per pass in any order, and the rounding of the intermediate).
"""
import numpy as np

GUTTER = 12
MAX_TAPS = 50
MAX_RATIO = 8


def calc_dim(w, h):
    """(w, h, aw, ah, astride) of the padded buffer of a w x h frame."""
    aw = w + 2 * GUTTER
    return (w, h, aw, 16 * ((h + 2 * GUTTER + 15) // 16), 32 * ((aw + 31) // 32))


def lanczos(t):
    t = np.abs(np.asarray(t, np.float64))
    return np.where(t < 3.0, np.sinc(t) * np.sinc(t / 3.0), 0.0)


def windows(n_in, n_out):
    """[(lo, float64 weights summing to 1)] per output."""
    scale = float(n_in) / float(n_out)
    support = 3.0 * scale
    out = []
    for i in range(n_out):
        c = (i + 0.5) * scale
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        x = np.arange(lo, hi, dtype=np.float64)
        wt = lanczos((x - c + 0.5) / scale)
        out.append((lo, wt / wt.sum()))
    return out


def tables(n_in, n_out):
    """(first int32 [n_out], taps float32 [n_out][nt])."""
    assert n_out >= 1 and n_out <= n_in <= MAX_RATIO * n_out
    win = windows(n_in, n_out)
    nt = max(len(wt) for _, wt in win)
    first = np.zeros(n_out, np.int32)
    taps = np.zeros((n_out, nt), np.float32)
    for i, (lo, wt) in enumerate(win):
        first[i] = min(lo, n_in - nt)
        taps[i, lo - first[i]:lo - first[i] + len(wt)] = wt.astype(np.float32)
    return first, taps


def matrix(first, taps, n_in):
    """The axis as a dense float64 matrix [n_out][n_in]."""
    n_out, nt = taps.shape
    M = np.zeros((n_out, n_in), np.float64)
    for i in range(n_out):
        M[i, first[i]:first[i] + nt] = taps[i].astype(np.float64)
    return M


def resize_picture(pic, xt, yt):
    """pic float [h][w][C] -> (out, A) float64 [h2][w2][C] with the tables xt = (xfirst, xtaps), yt = (yfirst, ytaps)."""
    pic = np.asarray(pic, np.float64)
    h, w = pic.shape[:2]
    Mx, My = matrix(xt[0], xt[1], w), matrix(yt[0], yt[1], h)
    out = np.einsum('Yy,yXc->YXc', My, np.einsum('Xx,yxc->yXc', Mx, pic))
    A = np.einsum('Yy,yXc->YXc', np.abs(My), np.einsum('Xx,yxc->yXc', np.abs(Mx), np.abs(pic)))
    return out, A


def resize(src, w, h, w2, h2, xt=None, yt=None):
    """src: the padded buffer [ah][astride][4] (or flat) of a w x h frame.  Returns (out, A, nxt, nyt): the float64 padded buffers
    [ah2][astride2][4] of the w2 x h2 frame, zero outside the picture area.  Only the source's picture area is looked at."""
    _, _, _, ah, astride = calc_dim(w, h)
    _, _, _, ah2, astride2 = calc_dim(w2, h2)
    src = np.asarray(src).reshape(ah, astride, 4)
    xt = tables(w, w2) if xt is None else xt
    yt = tables(h, h2) if yt is None else yt
    pic, A = resize_picture(src[GUTTER:GUTTER + h, GUTTER:GUTTER + w], xt, yt)
    out = np.zeros((ah2, astride2, 4), np.float64)
    Aout = np.zeros_like(out)
    out[GUTTER:GUTTER + h2, GUTTER:GUTTER + w2] = pic
    Aout[GUTTER:GUTTER + h2, GUTTER:GUTTER + w2] = A
    return out, Aout, xt[1].shape[1], yt[1].shape[1]


def bar(A, nxt, nyt):
    return (nxt + nyt + 8) * 2.0 ** -24 * A
