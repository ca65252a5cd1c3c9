"""
The `spatial` filter on the device (csrc/resample.hip through fl_resample) against the float64 model of tests/spatial_model.py.

Bar.  An output bin is a sum of n x n products t_j t_i src in float32, formed separably or directly: its rounding error is at
most (n * n + 2) * 2^-24 * A, A = sum |t_j| |t_i| |src| over the footprint (the model computes A beside the result, from the same
float32 taps), plus 2^-126 for a result in the denormals.  Where A is 0 the device must give exactly 0.  The taps of the
kernel tests are random, signed, asymmetric and unnormalised: a flipped or transposed tap index, which Gaussian taps would
hide, fails them.  The worst error / bar per case goes to spatial_errors.txt in the directory FLAME_TEST_REPORT_DIR names.
"""
import ctypes as C
import os

import numpy as np
import pytest

from common import O
from cuburn_amd import configs, filters, profile, render, _lib
import spatial_model as SM

pytestmark = pytest.mark.gpu

# output sizes.  A workgroup makes (256 - (n - ss)) / ss bins of 8 rows: 58 .. 256 bins wide.  The first three are several
# workgroups down and, from supersample 3 or 4 up, across, with ragged last ones; (300, 9) is 352 padded bins wide — two to seven
# workgroups across at every supersample and tap count, the last one ragged
SIZES = [(70, 40), (33, 17), (1, 1), (300, 9)]
MID = {1: 6, 2: 8, 3: 6, 4: 8}                   # the middle tap count of each supersample: ss + 6 or ss + 8


@pytest.fixture(scope='module')
def mgr(built):
    return render.RenderManager(device=0, nslots=1024, host_seed=7)


def dims(mgr, w, h, ss):
    return mgr.fb.calc_dim(ss * w, ss * h), mgr.fb.calc_dim(w, h)


def report(line):
    try:
        out = os.environ.get('FLAME_TEST_REPORT_DIR')
        if out and os.path.isdir(out):
            with open(os.path.join(out, 'spatial_errors.txt'), 'a') as fp:
                fp.write(line + '\n')
    except OSError:
        pass


def resample(mgr, w, h, ss, src, taps, expect=_lib.FL_OK):
    """front <- src (laid out for ss*w x ss*h), fl_resample, read front (laid out for w x h)."""
    lib = _lib.load()
    din, dout = dims(mgr, w, h, ss)
    _lib.check(lib.fl_reserve(mgr.fb.ctx, din.w, din.h))
    mgr.fb.write('front', np.ascontiguousarray(src, np.float32))
    t = np.ascontiguousarray(taps, np.float32)
    rc = lib.fl_resample(mgr.fb.ctx, w, h, ss, t.ctypes.data, len(t))
    assert rc == expect, (rc, lib.fl_last_error())
    return mgr.fb.read('front', (dout.ah, dout.astride, 4), np.float32)


def bar_of(A, n, extra=0.0):
    return (n * n + 2) * 2.0 ** -24 * A + 2.0 ** -126 + extra


def check(dev, model, A, n, what, extra=0.0):
    assert dev.shape == model.shape and np.isfinite(dev).all(), what
    err, bar = np.abs(dev.astype(np.float64) - model), bar_of(A, n, extra)
    ratio = float((err / bar).max())
    report('%s: worst error / bar %.4f' % (what, ratio))
    bad = err > bar
    assert not bad.any(), '%s: %d bins over the bar, worst error / bar %.3f at %s' % (
        what, bad.sum(), ratio, np.unravel_index(np.argmax(err / bar), err.shape))
    dead = (A == 0) & (np.asarray(extra) == 0)
    assert not dev[dead].any(), '%s: %d non-zero values where no source bin is in reach' % (what, np.count_nonzero(dev[dead]))


# ------------------------------------------------------------------ kernel against the model, whole padded buffer
@pytest.mark.parametrize('size', SIZES, ids=['%dx%d' % s for s in SIZES])
@pytest.mark.parametrize('ss', [1, 2, 3, 4])
def test_kernel_against_model(mgr, size, ss):
    w, h = size
    din, dout = dims(mgr, w, h, ss)
    rs = np.random.RandomState(1000 * ss + w)
    seen_dead = 0
    for n in (ss, ss + MID[ss], ss + 24):
        taps = rs.uniform(-1.0, 1.0, n).astype(np.float32)
        taps[0], taps[-1] = np.float32(0.9), np.float32(-0.6)              # the ends count, and differ
        for signed in (False, True):
            src = rs.uniform(0.0, 1.0, (din.ah * din.astride, 4)).astype(np.float32)
            if signed:
                src = (src - np.float32(0.5)) * np.float32(4.0)
            dev = resample(mgr, w, h, ss, src, taps)
            model, A = SM.resample(src, din, dout, ss, taps)
            check(dev, model, A, n, 'kernel %dx%d ss %d n %d %s' % (w, h, ss, n, 'signed' if signed else 'unsigned'))
            seen_dead += int((A == 0).sum())
            assert (A[12:12 + h, 12:12 + w] > 0).all()
    # the output gutter reaches beyond the source buffer where ss > 1 and the footprint is narrow: bins of exactly zero
    assert ss == 1 or seen_dead > 0


def test_impulses(mgr):
    """One source bin at a time — the corners of the padded source buffer and an interior bin: the output is the tap
    footprint around it and exactly zero everywhere else."""
    w, h = 33, 17
    rs = np.random.RandomState(77)
    for ss, n in ((1, 7), (2, 10), (3, 3), (3, 27), (4, 12), (4, 28)):
        din, dout = dims(mgr, w, h, ss)
        taps = rs.uniform(-1.0, 1.0, n).astype(np.float32)
        for sx, sy in ((0, 0), (din.astride - 1, din.ah - 1), (12 + ss * 16 + ss - 1, 12 + ss * 8)):
            src = np.zeros((din.ah, din.astride, 4), np.float32)
            src[sy, sx] = [1.0, -2.0, 0.5, 3.0]
            dev = resample(mgr, w, h, ss, src, taps)
            model, A = SM.resample(src, din, dout, ss, taps)
            check(dev, model, A, n, 'impulse ss %d n %d at (%d, %d)' % (ss, n, sx, sy))
            # the footprint, written out: bin (X, Y) sees the impulse through taps i = sx - (12 + ss (X - 12) - g), j likewise
            g = (n - ss) // 2
            want = np.zeros((dout.ah, dout.astride), np.float64)
            for Y in range(dout.ah):
                j = sy - (12 + ss * (Y - 12) - g)
                if 0 <= j < n:
                    for X in range(dout.astride):
                        i = sx - (12 + ss * (X - 12) - g)
                        if 0 <= i < n:
                            want[Y, X] = float(taps[j]) * float(taps[i])
            assert np.abs(model[..., 3] - 3.0 * want).max() <= 1e-12
            assert np.array_equal(dev[..., 3] != 0, want != 0) or (taps == 0).any()
            if (sx, sy) != (0, 0) or ss == 1:
                assert (want != 0).any(), (ss, n, sx, sy)


def test_argument_errors_leave_the_context_usable(mgr):
    lib = _lib.load()
    w, h = 33, 17
    din, dout = dims(mgr, w, h, 2)
    src = np.random.RandomState(3).uniform(0, 1, (din.ah * din.astride, 4)).astype(np.float32)
    ok = np.linspace(0.1, 0.8, 8).astype(np.float32)
    good = resample(mgr, w, h, 2, src, ok)
    nan = ok.copy()
    nan[5] = np.nan
    inf = ok.copy()
    inf[0] = np.inf
    cases = [(0, ok), (5, ok), (2, ok[:7]), (3, ok), (2, ok[:1]), (4, ok[:2]), (2, np.ones(28, np.float32)),
             (1, np.ones(27, np.float32)), (4, np.ones(30, np.float32)), (2, nan), (2, inf)]
    for ss, taps in cases:
        t = np.ascontiguousarray(taps, np.float32)
        assert lib.fl_resample(mgr.fb.ctx, w, h, ss, t.ctypes.data, len(t)) == _lib.FL_E_INVAL, (ss, len(t))
        assert lib.fl_last_error()
    assert lib.fl_resample(mgr.fb.ctx, w, h, 2, None, 8) == _lib.FL_E_INVAL
    assert lib.fl_resample(mgr.fb.ctx, 0, h, 2, ok.ctypes.data, 8) == _lib.FL_E_INVAL
    with pytest.raises(ValueError):
        _lib.check(lib.fl_resample(mgr.fb.ctx, w, h, 5, ok.ctypes.data, 8))
    # nothing ran, nothing moved: the same call gives the same bits as before
    again = resample(mgr, w, h, 2, src, ok)
    assert np.array_equal(good.view(np.uint32), again.view(np.uint32))
    model, A = SM.resample(src, din, dout, 2, ok)
    check(again, model, A, 8, 'after argument errors')


def test_pending_yuv_runs_first_at_the_source_size(mgr):
    """`yuv` is deferred to the next call: fl_resample must run it first, on the SOURCE's layout.  The result is the model's
    resample of the oracle's yuv_to_rgb.  The oracle's and the device's yuv are both float32 evaluations of at most five
    operations per channel on terms of magnitude M = |y| + 1.772 (|u| + |w| / 2) + 1.402 (|v| + |w| / 2): each is within
    6 * 2^-24 * M of the exact value, so they differ by at most 12 * 2^-24 * M — filtered like the data itself, that is added
    to the kernel's bar."""
    lib = _lib.load()
    w, h, ss = 33, 17, 2
    din, dout = dims(mgr, w, h, ss)
    rs = np.random.RandomState(11)
    dens = rs.poisson(rs.uniform(0, 40, (din.ah * din.astride,))).astype(np.float32)
    buf = np.zeros((din.ah * din.astride, 4), np.float32)
    buf[:, 3] = dens
    buf[:, 0] = dens * rs.uniform(0.0, 1.0, dens.shape).astype(np.float32)
    buf[:, 1] = dens * rs.uniform(0.0, 1.0, dens.shape).astype(np.float32)       # u, v about w / 2 on either side: every clamp
    buf[:, 2] = dens * rs.uniform(0.0, 1.0, dens.shape).astype(np.float32)
    taps = filters.spatial_taps(1.0, ss)
    _lib.check(lib.fl_reserve(mgr.fb.ctx, din.w, din.h))
    mgr.fb.write('front', buf)
    _lib.check(lib.fl_filter(mgr.fb.ctx, _lib.FILT['yuv'], din.w, din.h, None, 0))
    _lib.check(lib.fl_resample(mgr.fb.ctx, w, h, ss, taps.ctypes.data, len(taps)))
    dev = mgr.fb.read('front', (dout.ah, dout.astride, 4), np.float32)
    rgb = O.yuv_to_rgb(O.calc_dim(din.w, din.h), buf)
    assert (rgb[:, :3] == 0).any() and not np.array_equal(rgb, buf)
    model, A = SM.resample(rgb, din, dout, ss, taps)
    b64 = np.abs(buf.astype(np.float64))
    M = b64[:, 0] + 1.772 * (b64[:, 1] + 0.5 * b64[:, 3]) + 1.402 * (b64[:, 2] + 0.5 * b64[:, 3])
    M4 = np.stack([M, M, M, np.zeros_like(M)], 1)                                # w passes through untouched
    extra = 12 * 2.0 ** -24 * SM.resample(M4, din, dout, ss, taps)[1]
    check(dev, model, A, len(taps), 'yuv then spatial', extra=extra)
    # had the yuv been dropped, or run behind the resample, the colours would differ by far more than the bar
    wrong, _ = SM.resample(buf, din, dout, ss, taps)
    assert (np.abs(wrong - model) > 100 * bar_of(A, len(taps), extra)).any()


def test_brightness_does_not_depend_on_supersample(mgr):
    """A uniform accumulator of v per output pixel, i.e. v / ss^2 per source bin, through logscale and spatial with a
    supersample-2 profile, against the supersample-1 logscale of v: the same picture to 1e-5 relative."""
    lib = _lib.load()
    w, h, ss, tc = 33, 17, 2, 0.5
    gnm, prof = configs.cfg2()
    prof = dict(prof, width=w, height=h, filter_order=['logscale', 'spatial'])
    g1, g2 = profile.wrap(prof, gnm), profile.wrap(dict(prof, supersample=ss), gnm)
    din, dout = dims(mgr, w, h, ss)
    v = np.array([300.0, 700.0, 150.0, 1000.0], np.float32)
    # supersample 1: logscale alone
    _lib.check(lib.fl_reserve(mgr.fb.ctx, din.w, din.h))
    mgr.fb.write('front', np.tile(v, (dout.ah * dout.astride, 1)))
    assert filters.Logscale().apply(mgr.fb, g1, g1.filters.logscale, dout, tc) is None
    ref = mgr.fb.read('front', (dout.ah, dout.astride, 4), np.float32)[12:12 + h, 12:12 + w].astype(np.float64)
    assert (ref > 0).all() and np.ptp(ref[..., 3]) == 0
    # supersample 2: a quarter of the samples per bin, logscale at the source size, then the filter
    mgr.fb.write('front', np.tile(v / np.float32(ss * ss), (din.ah * din.astride, 1)))
    chain = filters.create(g2)
    assert [f.name for f in chain] == ['yuv', 'logscale', 'spatial']
    dim = din
    for filt in chain[1:]:
        dim = filt.apply(mgr.fb, g2, getattr(g2.filters, filt.name), dim, tc) or dim
    assert dim == dout
    got = mgr.fb.read('front', (dout.ah, dout.astride, 4), np.float32)[12:12 + h, 12:12 + w].astype(np.float64)
    assert np.abs(got / ref - 1).max() <= 1e-5, np.abs(got / ref - 1).max()


# ------------------------------------------------------------------ whole frames
@pytest.mark.parametrize('ss,order', [(2, None), (3, ['bilateral', 'logscale', 'spatial', 'colorclip'])], ids=['ss2-default', 'ss3-late-clip'])
def test_frame(mgr, ss, order):
    gnm, prof = configs.cfg2(samples=2 ** 21)
    prof = dict(prof, width=96, height=64, spp=2 ** 21 / (96.0 * 64.0))
    if order is not None:
        prof['filter_order'] = order
    g1 = profile.wrap(prof, gnm)
    evt, h_out = mgr.queue_frame(render.Renderer(gnm, g1), gnm, g1, 0.5)
    evt.synchronize()
    n1 = mgr.last_nsamples
    assert h_out.shape == (64, 96, 4) and n1 >= 2 ** 21
    gs = profile.wrap(dict(prof, supersample=ss), gnm)
    rdr = render.Renderer(gnm, gs)
    assert 'spatial' in [f.name for f in rdr.filts]
    evt, h_out = mgr.queue_frame(rdr, gnm, gs, 0.5)
    evt.synchronize()
    assert h_out.shape == (64, 96, 4) and h_out[..., 3].max() > 0 and evt.time() > 0
    assert mgr.last_nsamples == n1                            # the sample count is per OUTPUT pixel


def test_resample_is_timed_with_the_filters(mgr):
    lib = _lib.load()
    w, h, ss = 70, 40, 2
    din, dout = dims(mgr, w, h, ss)
    src = np.ones((din.ah * din.astride, 4), np.float32)
    taps = filters.spatial_taps(1.0, ss)
    resample(mgr, w, h, ss, src, taps)
    mgr.timings_reset()
    assert mgr.timings()['filter_ms'] == 0
    resample(mgr, w, h, ss, src, taps)
    assert mgr.timings()['filter_ms'] > 0
