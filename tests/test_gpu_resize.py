"""
The Lanczos downscale on the device (csrc/resize.hip through fl_resize) against the float64 model of tests/resize_model.py, and
the profile's `proxies` through queue_frame.

Bar, for every sample of every channel: |dev - model| <= (nxt + nyt + 8) * 2^-24 * A, A the resample of |src| with |taps| (the
model computes it beside the result): nt float32 multiply-adds per pass in any order, plus the rounding of the intermediate.
Where A is 0 the device must give exactly 0; every bin outside the result's picture area must be +0.  The worst error / bar per
case goes to resize_errors.txt in the directory FLAME_TEST_REPORT_DIR names.
"""
import ctypes as C
import os

import numpy as np
import pytest

from common import O
from cuburn_amd import _lib, configs, filters, output, profile, render
import exr_model as X
import resize_cases as RC
import resize_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mgr(built):
    return render.RenderManager(device=0, nslots=1024, host_seed=7)


def report(line):
    try:
        out = os.environ.get('FLAME_TEST_REPORT_DIR')
        if out and os.path.isdir(out):
            with open(os.path.join(out, 'resize_errors.txt'), 'a') as fp:
                fp.write(line + '\n')
    except OSError:
        pass


def call(mgr, case, xt, yt):
    w, h, w2, h2 = case
    (xf, xtaps), (yf, ytaps) = xt, yt
    xf, yf = np.ascontiguousarray(xf, np.int32), np.ascontiguousarray(yf, np.int32)
    xtaps, ytaps = np.ascontiguousarray(xtaps, np.float32), np.ascontiguousarray(ytaps, np.float32)
    return _lib.load().fl_resize(mgr.fb.ctx, w, h, w2, h2, xf.ctypes.data, xtaps.ctypes.data, xtaps.shape[1],
                                 yf.ctypes.data, ytaps.ctypes.data, ytaps.shape[1])


def resize(mgr, case, src, tables=None):
    """front <- src (laid out for w x h), fl_resize, read front (laid out for w2 x h2)."""
    lib = _lib.load()
    w, h, w2, h2 = case
    _lib.check(lib.fl_reserve(mgr.fb.ctx, w, h))
    mgr.fb.write('front', np.ascontiguousarray(src, np.float32))
    xt, yt = tables or RC.tables(*case)
    rc = call(mgr, case, xt, yt)
    assert rc == _lib.FL_OK, (rc, lib.fl_last_error())
    dout = mgr.fb.calc_dim(w2, h2)
    return mgr.fb.read('front', (dout.ah, dout.astride, 4), np.float32)


def check(dev, model, A, nxt, nyt, case, what, extra=0.0):
    w2, h2 = case[2:]
    assert dev.shape == model.shape, what
    inside = np.zeros(dev.shape[:2], bool)
    inside[M.GUTTER:M.GUTTER + h2, M.GUTTER:M.GUTTER + w2] = True
    assert np.isfinite(dev[inside]).all(), what
    assert not dev[~inside].view(np.uint32).any(), '%s: a bin outside the picture area is not +0' % what
    err, bar = np.abs(dev.astype(np.float64) - model), M.bar(A, nxt, nyt) + extra
    live = bar > 0
    ratio = float((err[live] / bar[live]).max()) if live.any() else 0.0
    report('%s: worst error / bar %.4f' % (what, ratio))
    print('%s: worst error / bar %.4f' % (what, ratio))
    bad = err > bar
    assert not bad.any(), '%s: %d samples over the bar, worst error / bar %.3f, the largest error at %s' % (
        what, bad.sum(), ratio, np.unravel_index(np.argmax(np.where(bad, err, -1.0)), err.shape))
    return ratio


# ------------------------------------------------------------------ kernels against the model
@pytest.mark.parametrize('case', RC.CASES, ids=RC.IDS)
@pytest.mark.parametrize('which', ['noisy', 'impulse'])
def test_kernel_against_model(mgr, case, which):
    src, model, A, nxt, nyt = RC.expected(case, which)
    assert nxt <= 50 and nyt <= 50
    if which == 'noisy':
        w, h = case[:2]
        outside = np.ones(src.shape[:2], bool)
        outside[M.GUTTER:M.GUTTER + h, M.GUTTER:M.GUTTER + w] = False
        assert np.isnan(src[outside]).all() and np.isfinite(src[~outside]).all() and (src[~outside] < 0).any()
    dev = resize(mgr, case, src)
    check(dev, model, A, nxt, nyt, case, 'kernel %s %s' % (RC.IDS[RC.CASES.index(case)], which))
    if which == 'impulse':
        # where no impulse is in reach the device gives exactly zero, and where one is, the footprint is there
        dead = A == 0
        assert dead.any() and not dev[dead].any()
        assert np.array_equal(dev[..., 3] != 0, model[..., 3] != 0) or (np.abs(model[..., 3][dev[..., 3] == 0]) < 1e-30).all()


def test_two_runs_give_the_same_bits(mgr):
    for case in (RC.CASES[3], RC.CASES[2]):
        src = RC.expected(case, 'noisy')[0]
        a, b = resize(mgr, case, src), resize(mgr, case, src)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_tables_of_one_size_are_told_apart_by_content(mgr):
    """The lane keeps device copies by size and content hash: other tables for the same sizes must not meet the cached ones."""
    case = RC.CASES[0]
    src, model, A, nxt, nyt = RC.expected(case, 'noisy')
    (xf, xt), (yf, yt) = RC.tables(*case)
    rs = np.random.RandomState(9)
    xt2 = (xt * rs.uniform(-1.0, 1.0, xt.shape)).astype(np.float32)
    yt2 = (yt * rs.uniform(-1.0, 1.0, yt.shape)).astype(np.float32)
    resize(mgr, case, src)
    dev = resize(mgr, case, src, ((xf, xt2), (yf, yt2)))
    model2, A2, _, _ = M.resize(src, case[0], case[1], case[2], case[3], (xf, xt2), (yf, yt2))
    check(dev, model2, A2, nxt, nyt, case, 'other tables, same sizes')
    assert (np.abs(model2 - model) > 100 * M.bar(A, nxt, nyt))[A > 0].any()
    check(resize(mgr, case, src), model, A, nxt, nyt, case, 'the first tables again')
    # more sizes than the lane keeps, then the first again
    for other in RC.CASES[1:]:
        resize(mgr, other, RC.expected(other, 'impulse')[0])
    check(resize(mgr, case, src), model, A, nxt, nyt, case, 'after every other size')


# ------------------------------------------------------------------ refusals
def test_argument_errors_leave_the_front_buffer_alone(mgr):
    lib = _lib.load()
    case = (64, 36, 24, 9)
    w, h, w2, h2 = case
    src = RC.expected(case, 'impulse')[0]
    (xf, xt), (yf, yt) = RC.tables(*case)
    nxt, nyt = xt.shape[1], yt.shape[1]
    _lib.check(lib.fl_reserve(mgr.fb.ctx, w, h))
    mgr.fb.write('front', src)
    din = mgr.fb.calc_dim(w, h)

    def raw(w=w, h=h, w2=w2, h2=h2, xf=xf, xt=xt, nxt=nxt, yf=yf, yt=yt, nyt=nyt):
        keep = [None if a is None else np.ascontiguousarray(a, t) for a, t in ((xf, np.int32), (xt, np.float32), (yf, np.int32), (yt, np.float32))]
        p = [None if a is None else a.ctypes.data for a in keep]
        return lib.fl_resize(mgr.fb.ctx, w, h, w2, h2, p[0], p[1], nxt, p[2], p[3], nyt)

    def with_value(a, idx, v):
        b = np.array(a)
        b[idx] = v
        return b

    wide = np.zeros((w2, 51), np.float32)
    bad = {
        'null xfirst': dict(xf=None), 'null xtaps': dict(xt=None), 'null yfirst': dict(yf=None), 'null ytaps': dict(yt=None),
        'w 0': dict(w=0), 'h 0': dict(h=0), 'w2 0': dict(w2=0), 'h2 0': dict(h2=0),
        'w2 > w': dict(w2=w + 1, xf=np.zeros(w + 1, np.int32), xt=np.ones((w + 1, nxt), np.float32)),
        'h2 > h': dict(h2=h + 1, yf=np.zeros(h + 1, np.int32), yt=np.ones((h + 1, nyt), np.float32)),
        'nxt 0': dict(nxt=0), 'nyt 0': dict(nyt=0), 'nxt 51': dict(xt=wide, nxt=51),
        'nyt above the source': dict(h=20, h2=9, yt=np.ones((9, 24), np.float32), nyt=24),
        'first below 0': dict(xf=with_value(xf, 3, -1)), 'first + nt past the source': dict(xf=with_value(xf, w2 - 1, w - nxt + 1)),
        'yfirst past the source': dict(yf=with_value(yf, 0, h - nyt + 1)), 'yfirst below 0': dict(yf=with_value(yf, h2 - 1, -5)),
        'NaN tap': dict(xt=with_value(xt, (5, 2), np.nan)), 'inf tap': dict(yt=with_value(yt, (h2 - 1, nyt - 1), np.inf)),
    }
    for name, over in bad.items():
        assert raw(**over) == _lib.FL_E_INVAL, name
        assert lib.fl_last_error(), name
    # x windows that are no downscale's: neighbouring outputs at either end of a 600-bin row (the first kernel stages 576 per wave)
    far = np.where(np.arange(301) % 2 == 0, 0, 600 - 12).astype(np.int32)
    assert raw(w=600, h=40, w2=301, h2=20, xf=far, xt=np.ones((301, 12), np.float32), nxt=12,
               yf=np.zeros(20, np.int32), yt=np.ones((20, 12), np.float32), nyt=12) == _lib.FL_E_INVAL
    assert lib.fl_resize(None, w, h, w2, h2, xf.ctypes.data, xt.ctypes.data, nxt, yf.ctypes.data, yt.ctypes.data, nyt) == _lib.FL_E_INVAL
    # nothing ran, nothing moved
    after = mgr.fb.read('front', (din.ah, din.astride, 4), np.float32)
    assert np.array_equal(after.view(np.uint32), np.asarray(src).view(np.uint32))
    assert raw() == _lib.FL_OK
    dout = mgr.fb.calc_dim(w2, h2)
    dev = mgr.fb.read('front', (dout.ah, dout.astride, 4), np.float32)
    _, model, A, _, _ = RC.expected(case, 'impulse')
    check(dev, model, A, nxt, nyt, case, 'after argument errors')
    with pytest.raises(ValueError):
        filters.resize(mgr.fb, mgr.fb.calc_dim(w, h), w + 1, h)


def test_pending_yuv_runs_first_at_the_source_size(mgr):
    """`yuv` is deferred to the next call: fl_resize must run it first, on the SOURCE's layout.  The result is the model's resize of
    the oracle's yuv_to_rgb.  The oracle's and the device's yuv are both float32 evaluations of at most five operations per
    channel on terms of magnitude M = |y| + 1.772 (|u| + |w| / 2) + 1.402 (|v| + |w| / 2): each is within 6 * 2^-24 * M of the
    exact value, so they differ by at most 12 * 2^-24 * M — filtered like the data itself, that is added to the kernel's bar."""
    lib = _lib.load()
    case = (64, 36, 24, 9)
    w, h, w2, h2 = case
    din, dout = mgr.fb.calc_dim(w, h), mgr.fb.calc_dim(w2, h2)
    rs = np.random.RandomState(11)
    dens = rs.poisson(rs.uniform(0, 40, (din.ah * din.astride,))).astype(np.float32)
    buf = np.zeros((din.ah * din.astride, 4), np.float32)
    buf[:, 3] = dens
    for ch in range(3):
        buf[:, ch] = dens * rs.uniform(0.0, 1.0, dens.shape).astype(np.float32)
    (xf, xt), (yf, yt) = RC.tables(*case)
    _lib.check(lib.fl_reserve(mgr.fb.ctx, w, h))
    mgr.fb.write('front', buf)
    _lib.check(lib.fl_filter(mgr.fb.ctx, _lib.FILT['yuv'], w, h, None, 0))
    assert call(mgr, case, (xf, xt), (yf, yt)) == _lib.FL_OK
    dev = mgr.fb.read('front', (dout.ah, dout.astride, 4), np.float32)
    rgb = O.yuv_to_rgb(O.calc_dim(w, h), buf)
    assert (rgb[:, :3] == 0).any() and not np.array_equal(rgb, buf)
    model, A, nxt, nyt = M.resize(rgb, w, h, w2, h2, (xf, xt), (yf, yt))
    b64 = np.abs(buf.astype(np.float64))
    Mg = b64[:, 0] + 1.772 * (b64[:, 1] + 0.5 * b64[:, 3]) + 1.402 * (b64[:, 2] + 0.5 * b64[:, 3])
    M4 = np.stack([Mg, Mg, Mg, np.zeros_like(Mg)], 1)                            # w passes through untouched
    extra = 12 * 2.0 ** -24 * M.resize(M4, w, h, w2, h2, (xf, xt), (yf, yt))[1]
    check(dev, model, A, nxt, nyt, case, 'yuv then resize', extra=extra)
    # had the yuv been dropped, or run behind the resize, the colours would differ by far more than the bar
    wrong = M.resize(buf, w, h, w2, h2, (xf, xt), (yf, yt))[0]
    assert (np.abs(wrong - model) > 100 * (M.bar(A, nxt, nyt) + extra)).any()


def test_resize_is_timed_with_the_filters(mgr):
    case = RC.CASES[0]
    src = RC.expected(case, 'impulse')[0]
    resize(mgr, case, src)
    mgr.timings_reset()
    assert mgr.timings()['filter_ms'] == 0
    resize(mgr, case, src)
    assert mgr.timings()['filter_ms'] > 0


# ------------------------------------------------------------------ whole frames
def picture(data, w, h):
    ps = X.parse(data)
    assert (ps.w, ps.h, ps.channels, ps.pixel) == (w, h, 3, X.FLOAT)
    return ps.samples.view(np.float32).reshape(h, w, 3)


def file_of(mod, buf):
    media, logs = mod.encode(buf)
    assert len(media) == 1 and logs == []
    return list(media.values())[0].read()


EXR = {'type': 'exr', 'pixel': 'float'}
# one round of the 1024 x 256 walkers: a quick frame
SAMPLES = 2 ** 18


class _ExrKeepsFront(output.DeviceEXROutput):
    """The master's module, keeping the picture area of the front buffer as the filter chain left it: read when the master is
    copied, which is before any proxy is made."""

    def copy(self, fb, dim, **kw):
        g = M.GUTTER
        self.front = fb.read('front', (dim.ah, dim.astride, 4), np.float32)[g:g + dim.h, g:g + dim.w].copy()
        return output.DeviceEXROutput.copy(self, fb, dim, **kw)


@pytest.fixture(scope='module')
def frames(built):
    """One frame of the 96x64 master with proxies 48x32 and 24x16, all float EXR; the same with a device PNG as the second proxy;
    and the same genome without proxies: [(master file, [proxy files])] of the three runs, each on a manager of its own with one
    seed."""
    runs = []
    for proxies in ([{'width': 24, 'height': 16}, {'width': 48, 'height': 32}],
                    [{'width': 48, 'height': 32}, {'width': 24, 'height': 16, 'suffix': '_s', 'output': {'type': 'png', 'encoder': 'device'}}],
                    None):
        over = {} if proxies is None else {'proxies': proxies}
        gnm, prof = configs.cfg2(samples=SAMPLES)
        gprof = profile.wrap(dict(prof, width=96, height=64, spp=SAMPLES / float(96 * 64), output=EXR, **over), gnm)
        m = render.RenderManager(device=0, nslots=1024, host_seed=7)
        try:
            rdr = render.Renderer(gnm, gprof)
            assert type(rdr.out) is output.DeviceEXROutput
            rdr.out = _ExrKeepsFront(alpha=rdr.out.alpha, pixel=rdr.out.pixel)
            evt, h_out = m.queue_frame(rdr, gnm, gprof, 0.5)
            evt.synchronize()
            assert len(evt.proxies) == len(rdr.proxies) == len(proxies or [])
            runs.append((file_of(rdr.out, h_out), [file_of(px.out, buf) for px, buf in zip(rdr.proxies, evt.proxies)],
                         [(px.width, px.height, px.suffix) for px in rdr.proxies], rdr.out.front))
        finally:
            m.fb.free()
    return runs


def padded(pic, w, h):
    _, _, _, ah, astride = M.calc_dim(w, h)
    buf = np.zeros((ah, astride, 4), np.float32)
    buf[M.GUTTER:M.GUTTER + h, M.GUTTER:M.GUTTER + w, :3] = pic
    return buf


def test_proxies_of_a_frame_are_the_models_resize_of_the_one_before(frames):
    master, proxies, names, _ = frames[0]
    assert names == [(48, 32, '_32p'), (24, 16, '_16p')]            # from the largest to the smallest
    big, mid, small = picture(master, 96, 64), picture(proxies[0], 48, 32), picture(proxies[1], 24, 16)
    assert big.max() > 0.2 and big.std() > 0.01
    for src, (w, h), got, (w2, h2), what in ((big, (96, 64), mid, (48, 32), 'proxy 48x32 of the master'),
                                             (mid, (48, 32), small, (24, 16), 'proxy 24x16 of the 48x32 proxy')):
        model, A, nxt, nyt = M.resize(padded(src, w, h), w, h, w2, h2)
        dev = padded(got, w2, h2)
        check(dev[..., :3], model[..., :3], A[..., :3], nxt, nyt, (w, h, w2, h2), what)
    # made from the 48x32 frame, not from the master again: the two differ by far more than the bar
    direct, A, nxt, nyt = M.resize(padded(big, 96, 64), 96, 64, 24, 16)
    g = M.GUTTER
    assert (np.abs(direct[g:g + 16, g:g + 24, :3] - small) > 100 * M.bar(A[g:g + 16, g:g + 24, :3], nxt, nyt)).any()


def test_a_device_png_proxy_opens_at_its_size(frames):
    Image = pytest.importorskip('PIL.Image')
    import io
    master, proxies, names, _ = frames[1]
    assert names == [(48, 32, '_32p'), (24, 16, '_s')]
    img = Image.open(io.BytesIO(proxies[1]))
    img.load()
    assert img.size == (24, 16) and img.mode == 'RGB' and np.asarray(img).max() > 0
    assert picture(proxies[0], 48, 32).shape == (32, 48, 3)


def test_the_master_is_the_encode_of_the_frame_the_chain_left(frames):
    """With proxies or without, the master's file is, byte for byte, the model's encode of the front buffer as it was when the
    master was copied: the resizes and the proxies' encodes that follow it on the lane, through the same scratch, change nothing."""
    for master, proxies, names, front in frames:
        assert front.shape == (64, 96, 4) and front[..., :3].max() > 0.2
        assert master == X.encode(front, 3, X.FLOAT), names


def fixed_accumulator(seed=21):
    """A raw YUV accumulator of a 96x64 frame: Poisson densities, colours in proportion."""
    _, _, _, ah, astride = M.calc_dim(96, 64)
    rs = np.random.RandomState(seed)
    dens = rs.poisson(rs.uniform(0, 60, (ah * astride,))).astype(np.float32)
    buf = np.zeros((ah * astride, 4), np.float32)
    buf[:, 3] = dens
    for ch in range(3):
        buf[:, ch] = dens * rs.uniform(0.0, 1.0, dens.shape).astype(np.float32)
    return buf


PROXIES = [{'width': 48, 'height': 32}, {'width': 24, 'height': 16}]


@pytest.mark.parametrize('block', [EXR, {'type': 'png', 'encoder': 'device'}, {'type': 'png'}], ids=['exr-float', 'png-device', 'png-dithered-host'])
def test_the_first_master_is_the_same_with_and_without_proxies(built, block):
    """A profile without proxies against the same profile with two, on the same genome and seed, each on a manager of its own:
    the first frame's master is byte for byte the same.  Two renders of one profile do not repeat bit for bit (the
    accumulate adds a bin's colours in an order that changes from run to run), so the comparison starts behind the iterate:
    both managers get ONE fixed accumulator written into the front buffer and run everything that follows it in queue_frame
    (RenderManager.finish_frame: the filter chain, the master's conversion with the first draw from the dither states, its
    copy, the proxies).  None of that has an atomic or an order of its own."""
    lib = _lib.load()
    acc_buf = fixed_accumulator()
    masters, nproxies = [], []
    for proxies in (None, PROXIES, None):
        gnm, prof = configs.cfg2(samples=SAMPLES)
        prof = dict(prof, width=96, height=64, spp=SAMPLES / float(96 * 64), output=block)
        if proxies:
            prof['proxies'] = proxies
        gprof = profile.wrap(prof, gnm)
        m = render.RenderManager(device=0, nslots=1024, host_seed=7)
        try:
            rdr = render.Renderer(gnm, gprof)
            acc = m.fb.set_dim(96, 64)
            fid = C.c_uint32()
            _lib.check(lib.fl_frame_begin(m.fb.ctx, C.byref(fid)))
            _lib.check(lib.fl_reserve(m.fb.ctx, 96, 64))
            m.fb.write('front', acc_buf)
            evt, h_out = m.finish_frame(rdr, gprof, acc, 0.5, fid.value)
            evt.synchronize()
            masters.append(file_of(rdr.out, h_out))
            nproxies.append(len(evt.proxies))
            for px, buf in zip(rdr.proxies, evt.proxies):
                assert len(file_of(px.out, buf)) > 0
        finally:
            m.fb.free()
    assert nproxies == [0, 2, 0]
    assert masters[0] == masters[2], 'two runs without proxies differ: the comparison does not stand on fixed ground'
    assert masters[1] == masters[0]
    if block is EXR:
        assert picture(masters[0], 96, 64).max() > 0.2
