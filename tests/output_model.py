"""
A numpy restatement of the output conversion (cuburn_amd/csrc/output.hip, cuburn/code/output.py:7-236), independent of the C
oracle and of both kernels' loops: all six formats, vectorised over the dither states.

State t of the n dither states serves pixels t, t + n, t + 2 n, ... in that order: the image is walked in blocks of n consecutive
pixels, and in block b state t meets pixel b n + t.  Every float operation is rounded to float32, left to right as written in
output.hip (both sides are compiled with -ffp-contract=off); the MWC step is done in uint64.  Nothing here carries a tolerance.
"""
import numpy as np

GUTTER = 12
F = np.float32
RGBA8, RGBA16, YUV444P, YUV444P10, YUV420P10, YUV444P12 = range(6)


class Rng(object):
    """The MWC states of one block's pixels; draws advance only the states whose mask is set."""

    def __init__(self, seeds):
        self.mul = seeds[:, 0].astype(np.uint64)
        self.state = seeds[:, 1].astype(np.uint64)
        self.carry = seeds[:, 2].astype(np.uint64)
        self.draws = np.zeros(len(seeds), np.int64)

    def next_01(self, mask):
        """mwc_next_01 where `mask`: float32(u32) * 2^-32 (exactly 1.0 for the top 128 values); 0 elsewhere."""
        t = self.mul * self.state + self.carry                 # < 2^64: (2^32 - 1)^2 + 2^32 - 1
        lo, hi = t & np.uint64(0xffffffff), t >> np.uint64(32)
        self.state = np.where(mask, lo, self.state)
        self.carry = np.where(mask, hi, self.carry)
        self.draws += mask
        return np.where(mask, lo.astype(np.uint32).astype(F) * F(2.0 ** -32), F(0))

    def store(self, seeds):
        seeds[:, 1] = self.state.astype(np.uint32)
        seeds[:, 2] = self.carry.astype(np.uint32)


def dclampf(rng, peak, v):
    """0 unless v > 0 (NaN is not); else min(peak, v * peak + 0.99 * draw).  The draw is made only where v > 0."""
    live = v > 0
    with np.errstate(over='ignore', invalid='ignore'):
        dithered = np.fmin(F(peak), v * F(peak) + F(0.99) * rng.next_01(live))
    return np.where(live, dithered, F(0))


def trunc(v, dtype):
    """Truncating convert of values that dclampf has put into [0, peak] (+ 256 for the 12-bit format)."""
    return v.astype(np.int64).astype(dtype)


def sat_u16(v):
    """65535 from there up, truncation in (0, 65535), 0 for everything else (NaN included)."""
    out = np.zeros(v.shape, np.uint16)
    with np.errstate(invalid='ignore'):
        inside = (v > 0) & (v < 65535)
        out[v >= 65535] = 65535
    out[inside] = v[inside].astype(np.int64)
    return out


def luma601(c):
    return F(0.299) * c[:, 0] + F(0.587) * c[:, 1] + F(0.114) * c[:, 2]


def cb601(c):
    return F(-0.168736) * c[:, 0] - F(0.331264) * c[:, 1] + F(0.5) * c[:, 2]


def cr601(c):
    return F(0.5) * c[:, 0] - F(0.418688) * c[:, 1] - F(0.081312) * c[:, 2]


def empty_output(w, h, fmt):
    if fmt < YUV444P:
        return np.zeros((h, w, 4), np.uint16 if fmt else np.uint8)
    if fmt == YUV420P10:
        return np.zeros(w * h * 6 // 4, np.uint16)
    return np.zeros((3, h, w), np.uint8 if fmt == YUV444P else np.uint16)


def convert(dim, buf, seeds, fmt, counts=False):
    """(pixels, seeds_after[, draws per state]) of format `fmt` for the padded float4 buffer `buf` of frame `dim` (w, h, astride)."""
    w, h, astride = int(dim.w), int(dim.h), int(dim.astride)
    assert fmt != YUV420P10 or (w % 2 == 0 and h % 2 == 0)
    n, npix = len(seeds), w * h
    src = np.asarray(buf, F).reshape(-1, astride, 4)
    seeds = np.array(seeds, np.uint32)
    draws = np.zeros(n, np.int64)
    out = empty_output(w, h, fmt)
    flat = out.reshape(-1, 4) if fmt < YUV444P else out.reshape(-1)
    for first in range(0, npix, n):
        p = np.arange(first, min(first + n, npix))
        x, y = p % w, p // w
        c = src[y + GUTTER, x + GUTTER]
        rng = Rng(seeds[:len(p)])
        with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
            if fmt < YUV444P:
                peak = 65535 if fmt else 255
                for k in range(4):
                    flat[p, k] = trunc(dclampf(rng, peak, c[:, k]), flat.dtype)
            elif fmt in (YUV444P, YUV444P10):
                peak = 255 if fmt == YUV444P else 1023
                cb = cb601(c) + F(0.5)
                fy = dclampf(rng, peak, luma601(c))
                fb = dclampf(rng, peak, cb)
                fr = dclampf(rng, peak, cr601(c) + F(0.5))
                flat[p] = trunc(fy, flat.dtype)
                flat[npix + p] = trunc(fb, flat.dtype) if fmt == YUV444P else sat_u16(F(1023) * cb)     # the reference's quirk
                flat[2 * npix + p] = trunc(fr, flat.dtype)
            elif fmt == YUV420P10:
                flat[p] = trunc(dclampf(rng, 1023, luma601(c)), np.uint16)
                quad = (x < w // 2) & (y < h // 2)
                qx, qy = 2 * x[quad] + GUTTER, 2 * y[quad] + GUTTER
                q = [src[qy, qx], src[qy, qx + 1], src[qy + 1, qx], src[qy + 1, qx + 1]]
                asum = (q[0][:, 3].astype(np.float64) + 1e-12).astype(F)
                cb, cr = q[0][:, 3] * cb601(q[0]), q[0][:, 3] * cr601(q[0])
                for k in (1, 2, 3):
                    asum = asum + q[k][:, 3]
                    cb = cb + q[k][:, 3] * cb601(q[k])
                    cr = cr + q[k][:, 3] * cr601(q[k])
                vb, vr = np.zeros(len(p), F), np.zeros(len(p), F)
                vb[quad], vr[quad] = cb / asum + F(0.5), cr / asum + F(0.5)
                fb = dclampf(rng, 1023, vb)            # (outside the quadrant the value is 0: no draw)
                fr = dclampf(rng, 1023, vr)
                ci = (w // 2) * y[quad] + x[quad]
                flat[npix + ci] = trunc(fb[quad], np.uint16)
                flat[npix + npix // 4 + ci] = trunc(fr[quad], np.uint16)
            else:
                cc = np.fmin(F(1), np.fmax(F(0), c[:, :3]))
                fy = dclampf(rng, 3504, F(0.2126) * cc[:, 0] + F(0.7152) * cc[:, 1] + F(0.0722) * cc[:, 2])
                fb = dclampf(rng, 3584, F(-0.11457) * cc[:, 0] - F(0.38543) * cc[:, 1] + F(0.5) * cc[:, 2] + F(0.5))
                fr = dclampf(rng, 3584, F(0.5) * cc[:, 0] - F(0.45416) * cc[:, 1] - F(0.04585) * cc[:, 2] + F(0.5))
                flat[p] = trunc(fy + F(256), np.uint16)
                flat[npix + p] = trunc(fb + F(256), np.uint16)
                flat[2 * npix + p] = trunc(fr + F(256), np.uint16)
        rng.store(seeds[:len(p)])
        draws[:len(p)] += rng.draws
    return (out, seeds, draws) if counts else (out, seeds)


def advance(seeds, counts):
    """The states after counts[t] steps of state t's MWC: nothing but the recurrence."""
    seeds = np.array(seeds, np.uint32)
    left = np.array(counts, np.int64)
    rng = Rng(seeds)
    while (left > 0).any():
        rng.next_01(left > 0)
        left -= 1
    rng.store(seeds)
    return seeds
