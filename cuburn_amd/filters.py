"""
Host side of the filter chain: registry, per-filter scalar derivation, launch order.

Same classes and ``apply`` contract as cuburn/filters.py:23-198 — every filter leaves its
result in the front buffer — but a filter here is one call into libflame_hip (``fl_filter``),
which owns the kernels and scratch buffers.
"""
import numpy as np
from numpy import float32 as f32

from . import _lib


class Filter(object):
    filter_map = {}
    name = ''
    full_side = False

    def apply(self, fb, gprof, params, dim, tc, stream=None):
        raise NotImplementedError()

    def scalars(self, gprof, params, dim, tc):
        """The kernel arguments derived on the host, as a float32 list."""
        return []

    def _run(self, fb, dim, vals):
        arr = np.asarray(vals, dtype=np.float32)
        _lib.check(_lib.load().fl_filter(fb.ctx, _lib.FILT[self.name], dim.w, dim.h,
                                         arr.ctypes.data, len(arr)))

    @classmethod
    def register(cls, name):
        def register_(subcls):
            cls.filter_map[name] = subcls
            subcls.name = name
            return subcls
        return register_


class _Simple(Filter):
    def apply(self, fb, gprof, params, dim, tc, stream=None):
        self._run(fb, dim, self.scalars(gprof, params, dim, tc))


@Filter.register('yuv')
class YuvFilterLib(_Simple):
    pass


@Filter.register('bilateral')
class Bilateral(_Simple):
    radius = 15
    directions = 8

    def scalars(self, gprof, params, dim, tc):
        # spatial parameter scaled so a "pixel" is a 1080p pixel (cuburn/filters.py:74-76)
        sstd = params.spatial_std(tc) * dim.w / 1920.
        return [f32(sstd), f32(params.color_std(tc)), f32(params.density_std(tc)),
                f32(params.density_pow(tc)), f32(params.gradient(tc))]


@Filter.register('de')
class DensityEstimation(_Simple):
    """flam3's adaptive density estimator: a bin's kernel radius falls from R as its density grows."""
    max_radius = 96                 # FL_DE_MAX_RADIUS: also the filter's reach (distributed.FILTER_REACH)

    def scalars(self, gprof, params, dim, tc):
        # radius in 1080p pixels, as Bilateral's spatial_std; minimum is a fraction of the radius (genome/convert.py)
        R = params.radius(tc) * dim.w / 1920.
        curve = params.curve(tc)
        if not curve > 0:
            raise ValueError('de: curve must be > 0 (got %g)' % curve)
        if R > self.max_radius:
            raise ValueError('de: radius %g px at width %d is above the %d px limit' % (R, dim.w, self.max_radius))
        minimum = min(max(params.minimum(tc), 0.0), 1.0)
        return [f32(R), f32(minimum * R), f32(curve)]


@Filter.register('logscale')
class Logscale(_Simple):
    def scalars(self, gprof, params, dim, tc):
        k1 = f32(params.brightness(tc) * 268 / 256)
        area = dim.h / (params.scale(tc) ** 2 * dim.w)       # cuburn/filters.py:103-106
        k2 = f32(1.0 / (area * gprof.spp(tc)))
        # a bin of the supersampled accumulator has 1 / ss^2 of an output pixel's area, and the spatial filter averages:
        # the same factor on either side of `spatial`
        ss = supersample_of(gprof)
        if ss != 1:
            k2 = f32(k2 * f32(ss * ss))
        return [k1, k2]


def calc_lingam(params, tc):
    """gamma / linear-range scalars shared by the clip family (cuburn/filters.py:132-136)."""
    gam = f32(1 / params.gamma(tc))
    lin = f32(params.gamma_threshold(tc))
    lingam = f32(lin ** (gam - 1.0) if lin > 0 else 0)
    return gam, lin, lingam


@Filter.register('haloclip')
class HaloClip(_Simple):
    def scalars(self, gprof, params, dim, tc):
        return [f32(1 / gprof.filters.colorclip.gamma(tc) - 1)]


@Filter.register('smearclip')
class SmearClip(_Simple):
    full_side = True

    def scalars(self, gprof, params, dim, tc):
        gam, lin, lingam = calc_lingam(gprof.filters.colorclip, tc)
        return [f32(params.width(tc)), f32(gam - 1), lin, lingam]


@Filter.register('colorclip')
class ColorClip(_Simple):
    def scalars(self, gprof, params, dim, tc):
        gam, lin, lingam = calc_lingam(params, tc)
        return [f32(params.vibrance(tc)), f32(params.highlight_power(tc)), gam, lin, lingam]


@Filter.register('plainclip')
class PlainClip(_Simple):
    def scalars(self, gprof, params, dim, tc):
        gam, lin, lingam = calc_lingam(gprof.filters.colorclip, tc)
        return [f32(gam - 1), lin, lingam, f32(gprof.filters.plainclip.brightness(tc))]


def bloom_taps(sigma):
    """
    The taps of the ``bloom`` filter's Gaussian of ``sigma`` bins, cut at R = ceil(3 sigma): exp(-i^2 / (2 sigma^2)) for
    i = -R .. R, normalised to sum 1 in float64, then float32.  sigma 0 gives the single tap 1.
    """
    sigma = float(sigma)
    if not (sigma >= 0 and np.isfinite(sigma)):
        raise ValueError('bloom: sigma must be finite and >= 0 (got %g)' % sigma)
    R = int(np.ceil(3.0 * sigma))
    if R == 0:
        return np.ones(1, np.float32)
    i = np.arange(-R, R + 1, dtype=np.float64)
    t = np.exp(-i * i / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


@Filter.register('bloom')
class Bloom(_Simple):
    """A wide Gaussian glare of the light above ``threshold``: front += strength * blur(excess)."""
    max_reach = 384                 # FL_BLOOM_MAX_REACH: taps per side, also the filter's reach (distributed.FILTER_REACH)

    def scalars(self, gprof, params, dim, tc):
        # sigma in 1080p pixels, as Bilateral's spatial_std: the same look at every size and on either side of `spatial`
        radius = params.radius(tc)
        sigma = radius * dim.w / 1920.
        if not (sigma >= 0 and np.isfinite(sigma)):
            raise ValueError('bloom: radius must be finite and >= 0 (got %g)' % radius)
        R = int(np.ceil(3.0 * sigma))
        if R > self.max_reach:
            raise ValueError('bloom: radius %g at width %d reaches %d bins per side, above the limit of %d'
                             % (radius, dim.w, R, self.max_reach))
        taps = bloom_taps(sigma)
        return [f32(params.threshold(tc)), f32(params.strength(tc))] + [f32(t) for t in taps[R:]]


@Filter.register('logencode')
class LogEncode(_Simple):
    def scalars(self, gprof, params, dim, tc):
        return [f32(params.degamma(tc))]


SPATIAL_SUPPORT = 1.5               # flam3's Gaussian: the filter is cut at 1.5 widths
MAX_SUPERSAMPLE = 4
MAX_OVERHANG = 12                   # source bins the footprint may overhang an output bin per side: the gutter


def check_supersample(ss):
    if isinstance(ss, bool) or ss != int(ss) or not 1 <= ss <= MAX_SUPERSAMPLE:
        raise ValueError('supersample must be an integer in 1..%d (got %r)' % (MAX_SUPERSAMPLE, ss))
    return int(ss)


def supersample_of(gprof):
    return check_supersample(gprof.supersample)


def spatial_taps(radius, ss):
    """
    The taps per axis of flam3's spatial filter (flam3_create_spatial_filter, Gaussian shape) of ``radius`` output pixels at
    supersample ``ss``, float32, normalised to sum 1 in float64.  Their number has the parity of ``ss``, so
    that the footprint is centred on the ss x ss source bins of an output pixel; radius 0 reaches those bins and no further.
    """
    ss, radius = check_supersample(ss), float(radius)
    if not (radius >= 0 and np.isfinite(radius)):
        raise ValueError('spatial: radius must be finite and >= 0 (got %g)' % radius)
    fw = 2.0 * SPATIAL_SUPPORT * ss * radius
    n = int(fw) + 1
    if (n ^ ss) & 1:
        n += 1
    n = max(n, ss)
    if n > ss + 2 * MAX_OVERHANG:
        raise ValueError('spatial: radius %g at supersample %d needs %d taps per axis, above the limit of %d (ss + %d: the '
                         'footprint may overhang an output pixel by the %d-bin gutter per side)'
                         % (radius, ss, n, ss + 2 * MAX_OVERHANG, 2 * MAX_OVERHANG, MAX_OVERHANG))
    adjust = SPATIAL_SUPPORT * n / fw if fw > 0 else 1.0
    x = ((2.0 * np.arange(n) + 1.0) / n - 1.0) * adjust
    t = np.exp(-2.0 * x * x) * np.sqrt(2.0 / np.pi)
    return (t / t.sum()).astype(np.float32)


@Filter.register('spatial')
class Spatial(Filter):
    """flam3's spatial filter and the supersample decimation, one kernel: takes the buffer of the ss-fold frame
    and leaves that of the output frame, whose Dimensions ``apply`` returns."""

    def apply(self, fb, gprof, params, dim, tc, stream=None):
        ss = supersample_of(gprof)
        taps = spatial_taps(params.radius(tc), ss)
        w, h = dim.w // ss, dim.h // ss
        if (w * ss, h * ss) != (dim.w, dim.h):
            raise ValueError('spatial: a %d x %d buffer is not %d times an output frame' % (dim.w, dim.h, ss))
        _lib.check(_lib.load().fl_resample(fb.ctx, w, h, ss, taps.ctypes.data, len(taps)))
        return fb.calc_dim(w, h)


RESIZE_MAX_RATIO = 8                # the library serves FL_RESIZE_MAX_TAPS = 50 taps per output: 6 * 8 + 1
RESIZE_MAX_TAPS = 50
_resize_tables = {}


def resize_tables(n_in, n_out):
    """
    One axis of the Lanczos-3 downscale from ``n_in`` to ``n_out`` samples as ``(first int32 [n_out], taps
    float32 [n_out][nt])``: output i is the sum of the nt source samples from first[i] on, weighted by taps[i].  The taps are
    Pillow's (Image.resize with LANCZOS): centre c = (i + 0.5) * n_in / n_out, support 3 * n_in / n_out, the window
    max(0, int(c - support + 0.5)) .. min(n_in, int(c + support + 0.5)), weights normalised to sum 1 in float64 and then float32;
    a window cut by the edge is renormalised.  nt is the axis's longest window; first[i] = min(lo_i, n_in - nt), so every row
    stays inside the source.  The arrays are shared between calls: read-only.
    """
    n_in, n_out = int(n_in), int(n_out)
    if n_out < 1 or not n_out <= n_in <= RESIZE_MAX_RATIO * n_out:
        raise ValueError('resize: %d -> %d samples is a ratio of %s, outside 1..%d (enlarging is not supported; for more, chain two '
                         'proxies)' % (n_in, n_out, '%.3g' % (n_in / float(n_out)) if n_out >= 1 else 'nothing', RESIZE_MAX_RATIO))
    if (n_in, n_out) in _resize_tables:
        return _resize_tables[n_in, n_out]
    scale = n_in / float(n_out)
    support = 3.0 * scale
    c = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((c - support + 0.5).astype(np.int64), 0)            # (astype truncates towards zero, as C's cast does)
    hi = np.minimum((c + support + 0.5).astype(np.int64), n_in)
    nt = int((hi - lo).max())
    first = np.minimum(lo, n_in - nt)
    x = first[:, None] + np.arange(nt)[None, :]
    t = np.abs((x - c[:, None] + 0.5) / scale)
    wt = np.where((t < 3.0) & (x >= lo[:, None]) & (x < hi[:, None]), np.sinc(t) * np.sinc(t / 3.0), 0.0)
    taps = np.ascontiguousarray((wt / wt.sum(1, keepdims=True)).astype(np.float32))
    first = np.ascontiguousarray(first.astype(np.int32))
    assert nt <= RESIZE_MAX_TAPS and first.min() >= 0 and int(first.max()) + nt <= n_in
    taps.setflags(write=False)
    first.setflags(write=False)
    if len(_resize_tables) >= 64:
        _resize_tables.clear()
    _resize_tables[n_in, n_out] = (first, taps)
    return first, taps


def resize(fb, dim, w2, h2):
    """Bring the front buffer, laid out for ``dim``, down to ``w2`` x ``h2`` with the Lanczos-3 tables above (fl_resize): the
    float frame as the filter chain left it, nothing clamped.  Returns the new Dimensions."""
    (xf, xt), (yf, yt) = resize_tables(dim.w, w2), resize_tables(dim.h, h2)
    _lib.check(_lib.load().fl_resize(fb.ctx, dim.w, dim.h, w2, h2, xf.ctypes.data, xt.ctypes.data, xt.shape[1],
                                     yf.ctypes.data, yt.ctypes.data, yt.shape[1]))
    return fb.calc_dim(w2, h2)


def create(gprof):
    """The profile's chain.  `spatial` runs where the profile lists it (["de", "logscale", "spatial", "colorclip"] is flam3's
    late clip); a supersampled profile that does not list it gets it last (tone-map at full resolution, then filter: flam3's
    early clip).  Listed at supersample 1 it is flam3's plain spatial filter."""
    order = ['yuv'] + list(gprof.filter_order)
    if order.count('spatial') > 1:
        raise ValueError("filter_order lists 'spatial' %d times: the frame is brought down to the output size once" % order.count('spatial'))
    if supersample_of(gprof) > 1 and 'spatial' not in order:
        order.append('spatial')
    return [Filter.filter_map[f]() for f in order]
