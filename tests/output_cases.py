"""
Inputs shared by tests/test_cpu_output.py and tests/test_gpu_output.py (and tools/soak_output.py): the frame sizes, named for
what they reach of the 65 536 dither states and of k_f32_to_rgba's four-pixels-in-flight unroll, and one padded float4 buffer per
size: the soak's seeded field with a deterministic sprinkle of every value the conversion treats specially.
"""
import functools

import numpy as np

from common import O
from cuburn_amd import mwc
import output_model as OM

NOUT = 65536                       # FL_NOUT: dither states; state t serves pixels t, t + NOUT, ...
F = np.float32
G = OM.GUTTER

SIZES = [
    (1, 1),                        # smallest frame
    (2, 2),                        # smallest 4:2:0 frame
    (33, 17),                      # well below one pixel per state
    (256, 256),                    # exactly one pixel per state
    (257, 255),                    # one pixel short
    (256, 257),                    # 256 states take a second pixel: first use of k = 1
    (512, 512),                    # exactly 4 per state: the unrolled group ends flush
    (720, 480),                    # 5.27 per state: second outer iteration, ragged between k = 0 and k = 1
    (701, 487),                    # the same with an odd width and a row pitch unrelated to 64; every format but 4:2:0
    (1024, 520),                   # 8.125 per state: a third outer iteration that only the first 8192 states enter
]
FORMATS = [OM.RGBA8, OM.RGBA16, OM.YUV444P, OM.YUV444P10, OM.YUV420P10, OM.YUV444P12]
STRIDED = [s for s in SIZES if s[0] * s[1] > NOUT]           # from 256 x 257 up: some state serves a second pixel
TWO_FRAMES = (720, 480)


def cases(sizes=SIZES):
    """(w, h, fmt) of every size x format; 4:2:0 cannot subsample an odd size."""
    return [(w, h, fmt) for w, h in sizes for fmt in FORMATS if not (fmt == OM.YUV420P10 and (w % 2 or h % 2))]


def case_id(case):
    return '%dx%d-fmt%d' % case


# ------------------------------------------------------------------ the values
TINY = np.finfo(F).tiny                                      # FLT_MIN
PEAKS = (255, 65535, 1023, 3504, 3584)


def _component_values():
    """[(class name, float32)]: what one component can be."""
    out = [('nan', F(np.nan)), ('+inf', F(np.inf)), ('-inf', F(-np.inf)), ('-0', F(-0.0)),
           ('denormal min', F(1.4e-45)), ('denormal max', np.nextafter(TINY, F(0))), ('FLT_MIN', TINY),
           ('1', F(1)), ('1-', np.nextafter(F(1), F(0))), ('1+', np.nextafter(F(1), F(2))),
           ('3e38', F(3e38))]                                # 3e38 * peak overflows: fminf(peak, inf)
    for peak in (255, 65535):                                # the rgba peaks: a component IS the dithered value there
        for k in (1, 100, peak - 1):
            out.append(('%d/%d' % (k, peak), F(k) / F(peak)))
            out.append(('%d.011/%d' % (k, peak), F((k + 0.011) / peak)))     # the draw alone decides between k and k + 1
    for peak in PEAKS:
        out.append(('1-.5/%d' % peak, F(1 - 0.5 / peak)))    # in (1 - 0.99 / peak, 1): fminf(peak, ...) is live
    return out


def _pixel_values():
    """[(class name, rgba)]: whole pixels, for the YUV matrices."""
    out = [('cb+.5<0', (1.4, 1.4, -0.3, 1.0)), ('cb+.5>1', (-0.3, -0.3, 1.4, 1.0)),       # 10-bit 4:4:4 stores 1023 * cb: > 1023
           ('cr+.5<0', (-0.3, 1.4, 1.4, 1.0)), ('cr+.5>1', (1.4, -0.3, -0.3, 1.0)),
           ('black', (0.0, 0.0, 0.0, 1.0))]
    for peak in (255, 1023, 3504):                           # greys: luma = v up to the rounding of the matrix row
        for k in (1, 100, peak - 1):
            for name, v in (('%d/%d' % (k, peak), F(k) / F(peak)), ('%d.011/%d' % (k, peak), F((k + 0.011) / peak))):
                out.append(('grey ' + name, (v, v, v, 1.0)))
    return out


_C = [(0.9, 0.2, 0.1), (0.1, 0.8, 0.3), (0.2, 0.3, 1.2), (0.7, 0.7, 0.1)]
_DEN = float(np.nextafter(TINY, F(0)))


def _quad_values():
    """[(class name, four rgba)]: the 2 x 2 source pixels of one 4:2:0 chroma sample, in the order (0,0) (0,1) (1,0) (1,1)."""
    def quad(alphas, colours=_C):
        return [tuple(c) + (a,) for c, a in zip(colours, alphas)]
    out = [('all alphas 0', quad((0.0, 0.0, 0.0, 0.0)))]
    for k in range(4):
        out.append(('only alpha %d' % k, quad([0.7 if j == k else 0.0 for j in range(4)])))
    out.append(('denormal alpha', quad((_DEN, 0.0, 0.0, 0.0))))
    # ... times a colour of 2e38: alpha * cb is 1.2 if the denormal is kept and 0 if it is flushed; over a sum of 1e-12
    out.append(('denormal alpha, huge colour', quad((_DEN, 0.0, 0.0, 0.0), [(0.0, 0.0, 2e38)] + _C[1:])))
    out.append(('alpha sum 0', quad((-1.0, 1.0, 0.0, 0.0))))                 # cb / 0 = +-inf
    out.append(('alpha sum 0, 0/0', quad((-1.0, 1.0, 0.0, 0.0), [_C[0]] * 4)))
    out.append(('alpha sum < 0', quad((-1.0, 0.5, 0.0, 0.0))))
    out.append(('alpha nan', quad((np.nan, 0.5, 0.5, 0.5))))
    out.append(('alpha inf', quad((np.inf, 0.5, 0.0, 0.0))))
    out.append(('alpha inf last', quad((0.5, 0.0, 0.0, np.inf))))
    return out


COMPONENT_EVERY, PIXEL_EVERY, QUAD_EVERY = 9, 17, 11


@functools.lru_cache(maxsize=None)
def frame(w, h):
    """(oracle dim, (ah * astride, 4) float32 buffer, read-only) of one size.  Field: uniform on (-0.3, 1.4), a fifth of the pixels
    zeroed, gutter included.  Over the cropped image, later layers on top of earlier ones: every COMPONENT_EVERY-th component takes
    the next component value, every PIXEL_EVERY-th pixel the next pixel value, every QUAD_EVERY-th aligned 2 x 2 quad the next
    quad: each of the 28 component values once in 252 components (0.4 %)."""
    d = O.calc_dim(w, h)
    rs = np.random.RandomState(1000 * w + h)
    buf = rs.uniform(-0.3, 1.4, (d.ah * d.astride, 4)).astype(F)
    buf[rs.uniform(size=len(buf)) < 0.2] = 0.0
    crop = np.ascontiguousarray(buf.reshape(d.ah, d.astride, 4)[G:G + h, G:G + w])

    vals = np.array([v for _, v in _component_values()], F)
    comp = crop.reshape(-1)
    j = np.arange(0, comp.size, COMPONENT_EVERY)
    comp[j] = vals[(j // COMPONENT_EVERY) % len(vals)]

    vals = np.array([v for _, v in _pixel_values()], F)
    pix = crop.reshape(-1, 4)
    j = np.arange(5, len(pix), PIXEL_EVERY)
    pix[j] = vals[(j // PIXEL_EVERY) % len(vals)]

    vals = np.array([v for _, v in _quad_values()], F)                       # (kinds, 4, 4)
    qw, qh = w // 2, h // 2
    j = np.arange(0, qw * qh, QUAD_EVERY)
    kind, qx, qy = (j // QUAD_EVERY) % len(vals), 2 * (j % max(qw, 1)), 2 * (j // max(qw, 1))
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        crop[qy + dy, qx + dx] = vals[kind, k]

    buf.reshape(d.ah, d.astride, 4)[G:G + h, G:G + w] = crop
    if w * h > 33 * 17:
        missing = [name for name, n in census(d, buf).items() if n == 0]
        assert not missing, ('%d x %d lacks' % (w, h), missing)
    buf.setflags(write=False)
    return d, buf


def census(d, buf):
    """{class name: occurrences in the CROPPED image} of every class above, from the buffer alone."""
    w, h = int(d.w), int(d.h)
    crop = np.ascontiguousarray(np.asarray(buf).reshape(d.ah, d.astride, 4)[G:G + h, G:G + w])
    bits = crop.view(np.uint32)
    out = {}
    for name, v in _component_values():
        out[name] = int((bits == np.array(v, F).view(np.uint32)).sum())
    pix = crop.reshape(-1, 4)
    with np.errstate(invalid='ignore', over='ignore'):
        cb, cr = OM.cb601(pix) + F(0.5), OM.cr601(pix) + F(0.5)
        out.update({'cb+.5<0': int((cb < 0).sum()), 'cb+.5>1': int((cb > 1).sum()), 'cr+.5<0': int((cr < 0).sum()), 'cr+.5>1': int((cr > 1).sum())})
    for name, v in _pixel_values()[4:]:
        out[name] = int((pix.view(np.uint32) == np.array(v, F).view(np.uint32)).all(1).sum())
    # alphas of the aligned quads, (quads, 4) in the order (0,0) (0,1) (1,0) (1,1)
    a = crop[:h // 2 * 2, :w // 2 * 2, 3].reshape(h // 2, 2, w // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
    b = crop[:h // 2 * 2, :w // 2 * 2, 2].reshape(h // 2, 2, w // 2, 2).transpose(0, 2, 1, 3).reshape(-1, 4)
    with np.errstate(invalid='ignore'):
        nz = a != 0
        den = (a != 0) & (np.abs(a) < TINY)
        tot = ((a[:, 0].astype(np.float64) + 1e-12).astype(F) + a[:, 1]) + a[:, 2] + a[:, 3]
        neg = (a < 0).any(1)
        out['all alphas 0'] = int((~nz).all(1).sum())
        for k in range(4):
            out['only alpha %d' % k] = int((nz[:, k] & (nz.sum(1) == 1)).sum())
        out['denormal alpha'] = int(den.any(1).sum())
        out['denormal alpha, huge colour'] = int((den[:, 0] & (b[:, 0] > 1e38)).sum())
        out['alpha sum 0'] = int((neg & (tot == 0) & (b[:, 0] != b[:, 1])).sum())
        out['alpha sum 0, 0/0'] = int((neg & (tot == 0) & (b[:, 0] == b[:, 1])).sum())
        out['alpha sum < 0'] = int((neg & (tot < 0)).sum())
        out['alpha nan'] = int(np.isnan(a).any(1).sum())
        out['alpha inf'] = int(np.isinf(a[:, 0]).sum())
        out['alpha inf last'] = int(np.isinf(a[:, 3]).sum())
    return out


@functools.lru_cache(maxsize=None)
def seeds(host_seed=11):
    """NOUT dither states for the CPU tests (the GPU tests take the device's own)."""
    s = mwc.make_seeds(NOUT, host_seed)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def oracle(w, h, fmt):
    """(pixels, states after) of the C oracle on frame(w, h) from seeds(): computed once, shared, read-only."""
    d, buf = frame(w, h)
    out, after = O.f32_to_rgba(d, buf, seeds(), fmt)
    out.setflags(write=False)
    after.setflags(write=False)
    return out, after


def served(npix, n=NOUT):
    """How many pixels each of the n states serves in a frame of npix pixels."""
    t = np.arange(n)
    return np.where(t < npix, (npix - t + n - 1) // n, 0)
