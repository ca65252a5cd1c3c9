"""
The 4:2:0 form of the device JPEG encoder (cuburn_amd/csrc/jpeg.hip; fl_jpeg_encode_s, fl_output_jpeg_s) and the Motion-JPEG
output against the numpy model of tests/jpeg420_model.py, which tests/test_cpu_mjpeg.py holds to Pillow.  For every frame of
tests/jpeg420_cases.py the criteria of tests/test_gpu_jpeg.py:

  A. the stream parses (marker order, RST numbering, stuffing, padding), and its size, tables and restart interval are what the
     record and the model say;
  B. every coefficient c satisfies |c * q - v| <= q / 2 + EPS, v the model's float64 DCT value.  No share of outliers is allowed;
  C. the model's entropy coder, given the device's own coefficients and restart interval, reproduces the device's bytes;
  D. a second encode gives the same bytes.

EPS = 2^-8 as derived in tests/test_gpu_jpeg.py: the DCT is the same code, and its chroma input, (a + b + c + d + 2) >> 2, is an
exact integer in 0..255 like a Y sample, so the bound carries over unchanged.
"""
import ctypes as C
import io

import numpy as np
import pytest

from cuburn_amd import _lib, configs, encoders, output, profile, render
import encoder_harness as H
from encoder_harness import SENTINEL, SLACK, assert_untouched, record, upload
import jpeg420_cases as JC
import jpeg420_model as M
import jpeg_cases as JC444
import jpeg_model as J

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -8
S444, S420 = _lib.JPEG_SAMPLING['444'], _lib.JPEG_SAMPLING['420']


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
    m.fb.free()


def encode(mgr, planes, quality, sampling=S420, cap=None, buf=None):
    """fl_jpeg_encode_s into pinned memory (or `buf`) pre-filled with the sentinel; checks the sentinel at and beyond cap."""
    _, h, w = planes.shape
    if cap is None:
        cap = _lib.load().fl_jpeg_bound_s(w, h, sampling)
    return H.encode(mgr, 'fl_jpeg_encode_s', planes, w, h, (quality, sampling), cap, buf)


def stream_of(buf):
    nbytes, status, ri = record(buf)
    assert status == 0
    return bytes(buf[16:16 + nbytes])


@pytest.fixture(scope='module')
def device_ri(mgr):
    """The library's 4:2:0 restart interval, from the record of a one-MCU frame."""
    buf, _ = encode(mgr, np.zeros((3, 16, 16), np.uint8), 50)
    ri = record(buf)[2]
    assert 1 <= ri <= 10                            # six lanes per MCU, one wave per interval
    return ri


_done = {}


def encoded_case(mgr, name, ri):
    if name not in _done:
        planes, quality, check = JC.case(name, ri)
        buf, _ = encode(mgr, planes, quality)
        _done[name] = (planes, quality, check, stream_of(buf), buf)
    return _done[name]


def assert_criteria(data, planes, quality, ri):
    """A, B and C for a 4:2:0 stream; returns the parse."""
    ps = M.parse(data)                                                              # A
    qt = J.quant_tables(quality)
    assert (ps.w, ps.h) == (planes.shape[2], planes.shape[1]) and ps.restart_interval == ri
    assert np.array_equal(ps.qtables, qt)
    v = M.dct_values(planes)                                                        # B
    qz = M._qz(qt)[None].astype(np.float64)
    err = np.abs(ps.coefficients * qz - v) - qz / 2
    print('largest |c q - v| - q / 2: %.3g (EPS %.3g)' % (err.max(), EPS))
    assert (err <= EPS).all(), '%d coefficients beyond q / 2 + EPS, worst by %g' % (int((err > EPS).sum()), err.max())
    assert M.assemble(ps.w, ps.h, qt, ri, ps.coefficients) == data                  # C
    return ps


@pytest.mark.parametrize('name', JC.NAMES)
def test_cases(mgr, device_ri, name):
    planes, quality, check, data, buf = encoded_case(mgr, name, device_ri)
    assert record(buf)[2] == device_ri
    ps = assert_criteria(data, planes, quality, device_ri)
    check(ps.stats, device_ri)
    again, _ = encode(mgr, planes, quality)                                          # D
    assert stream_of(again) == data
    assert 16 + len(data) <= _lib.load().fl_jpeg_bound_s(planes.shape[2], planes.shape[1], S420)


def test_capacity(mgr, device_ri):
    planes, quality, _, data, _ = encoded_case(mgr, JC.NOISE_Q100, device_ri)
    need = len(data)
    for cap in (16 + need - 1, 16 + M.HEADER_BYTES):
        buf, cap = encode(mgr, planes, quality, cap=cap)                             # (checks the sentinel at and beyond cap)
        assert record(buf) == (need, 1, device_ri)
    buf, cap = encode(mgr, planes, quality, cap=16 + need)
    assert record(buf) == (need, 0, device_ri) and stream_of(buf) == data


def test_444_through_the_new_entry_point(mgr):
    """FL_JPEG_444 through fl_jpeg_encode_s: the bytes of fl_jpeg_encode, record included."""
    lib = _lib.load()
    for name in ('noise_17x9_q1', JC444.NOISE_Q100, 'rst_wraps'):
        planes, quality, _ = JC444.case(name, 8)
        _, h, w = planes.shape
        new, cap = encode(mgr, planes, quality, sampling=S444)
        assert cap == lib.fl_jpeg_bound(w, h)
        t = upload(mgr, planes)
        old = mgr.fb._pinned((cap + SLACK,), 'u1')
        old[:] = SENTINEL
        _lib.check(lib.fl_jpeg_encode(mgr.fb.ctx, w, h, t.data_ptr(), quality, old.ctypes.data, 0, cap))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        assert record(old)[1] == 0 and np.array_equal(old, new)
        J.parse(stream_of(new))


def test_bad_arguments(mgr, device_ri):
    lib = _lib.load()
    planes, quality, _, data, _ = encoded_case(mgr, JC.NOISE_Q100, device_ri)
    _, h, w = planes.shape
    t = upload(mgr, planes)
    cap = lib.fl_jpeg_bound_s(w, h, S420)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    ctx, src, dst = mgr.fb.ctx, t.data_ptr(), buf.ctypes.data
    bad = [(w, h, src, quality, 2, dst, 0, cap), (w, h, src, quality, -1, dst, 0, cap), (w, h, src, quality, 420, dst, 0, cap),
           (w, h, src, 0, S420, dst, 0, cap), (w, h, src, 101, S420, dst, 0, cap), (0, h, src, quality, S420, dst, 0, cap),
           (w, 65536, src, quality, S420, dst, 0, cap), (w, h, 0, quality, S420, dst, 0, cap),
           (w, h, src, quality, S420, dst, 0, 16 + M.HEADER_BYTES - 1), (w, h, src, quality, S420, None, 0, cap)]
    for args in bad:
        assert lib.fl_jpeg_encode_s(ctx, *args) == _lib.FL_E_INVAL, args
        assert lib.fl_last_error()
    for args in bad:
        if args[2]:
            assert lib.fl_output_jpeg_s(ctx, *(args[:2] + args[3:])) == _lib.FL_E_INVAL, args
    _lib.check(lib.fl_ctx_sync(ctx))
    assert (buf == SENTINEL).all()
    good, _ = encode(mgr, planes, quality)
    assert stream_of(good) == data


def test_pageable_memory(mgr, device_ri):
    """A destination that is not pinned receives a copy; the bytes are the same."""
    planes, quality, _, data, _ = encoded_case(mgr, JC.NOISE_Q100, device_ri)
    cap = _lib.load().fl_jpeg_bound_s(planes.shape[2], planes.shape[1], S420)
    buf, _ = encode(mgr, planes, quality, buf=np.empty(cap + SLACK, np.uint8))
    assert stream_of(buf) == data
    buf, _ = encode(mgr, planes, quality, cap=16 + len(data) - 1, buf=np.empty(16 + len(data) + SLACK, np.uint8))
    assert record(buf) == (len(data), 1, device_ri)


def test_device_destination(mgr, device_ri):
    import torch
    lib = _lib.load()
    planes, quality, _, data, _ = encoded_case(mgr, JC.NOISE_Q100, device_ri)
    _, h, w = planes.shape
    cap = 16 + len(data) + 7
    t = upload(mgr, planes)
    for odd in (1, 2, 3):
        out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device=t.device)
        torch.cuda.synchronize(mgr.fb.device)
        host = mgr.fb._pinned((cap + SLACK,), 'u1')
        host[:] = SENTINEL
        _lib.check(lib.fl_jpeg_encode_s(mgr.fb.ctx, w, h, t.data_ptr(), quality, S420, host.ctypes.data, out.data_ptr() + odd, cap))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        dev = out.cpu().numpy()
        assert (dev[:odd] == SENTINEL).all() and (dev[odd + cap:] == SENTINEL).all() and (host[cap:] == SENTINEL).all()
        assert stream_of(dev[odd:]) == data and stream_of(host) == data


def test_whole_path(mgr, device_ri):
    """fl_output_jpeg_s = fl_output(FL_OUT_YUV444P) + the encode: same planes, same dither states afterwards, a closed frame."""
    lib = _lib.load()
    w, h, quality = 70, 50, 90                     # partial MCUs in both axes
    dim = mgr.fb.set_dim(w, h)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(mgr.fb.ctx, C.byref(fid)))      # first: a frame chooses the lane whose buffers the calls below use
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, w, h, 0))
    rs = np.random.RandomState(11)
    front = (rs.rand(dim.ah * dim.astride, 4) * 1.3 - 0.1).astype(np.float32)
    mgr.fb.write('front', front)
    start = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    planes = np.empty((3, h, w), np.uint8)
    _lib.check(lib.fl_output(mgr.fb.ctx, w, h, _lib.OUT['yuv444p'], planes.ctypes.data, 0))
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    after_plain = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    assert not np.array_equal(start, after_plain) and planes.std() > 10

    mgr.fb.write('seeds', start)
    cap = lib.fl_jpeg_bound_s(w, h, S420)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    _lib.check(lib.fl_output_jpeg_s(mgr.fb.ctx, w, h, quality, S420, buf.ctypes.data, 0, cap))
    ms = C.c_float(-1.0)
    _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
    assert ms.value >= 0.0
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    assert_untouched(buf, cap)
    assert_criteria(stream_of(buf), planes, quality, device_ri)
    assert np.array_equal(mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32), after_plain)
    assert mgr.timings()['jpeg_ms'] > 0.0          # fl_timings_detail[5]: the encode's kernels


def _small(block):
    gnm, prof = configs.cfg2(samples=2 ** 22)
    prof = dict(prof, width=64, height=48, spp=2 ** 22 / (64.0 * 48.0), fps=24, output=block)
    return gnm, profile.wrap(prof, gnm)


def test_through_the_shim(built):
    """Three frames of a 64 x 48 config with type mjpeg: an .avi the reader accepts, whose chunks are 4:2:0 files the model parses
    and Pillow decodes at 64 x 48.  Each chunk is also the DeviceJPEGOutput(sampling='420') still of the same time from a manager
    with the same seed: a manager's frames depend on its seed and on the order of its frames only, and both managers render the
    same times in the same order."""
    times = (0.25, 0.5, 0.75)
    chunks = []
    for block in ({'type': 'mjpeg', 'quality': 85}, {'type': 'jpeg', 'device': True, 'quality': 85, 'sampling': '420'}):
        gnm, gprof = _small(block)
        m = render.RenderManager(device=0, host_seed=7)
        try:
            rdr = render.Renderer(gnm, gprof)
            got = []
            for t in times:
                evt, h_out = m.queue_frame(rdr, gnm, gprof, t)
                evt.synchronize()
                assert h_out.shape == rdr.out.shape(m.fb.calc_dim(64, 48)) and h_out.dtype == np.uint8
                media, logs = rdr.out.encode(h_out)
                got.append(media)
            if block['type'] == 'mjpeg':
                assert type(rdr.out) is encoders.MJPEGOutput and got == [{}, {}, {}]
                media, logs = rdr.out.encode(None)
                assert list(media) == ['.avi'] and logs == []
                avi = M.read_avi(media['.avi'].read())
                assert len(avi.chunks) == 3 and (avi.avih['dwWidth'], avi.avih['dwHeight']) == (64, 48)
                assert (avi.strh['dwRate'], avi.strh['dwScale']) == (24, 1)
                chunks.append(avi.chunks)
            else:
                assert type(rdr.out) is output.DeviceJPEGOutput
                chunks.append([g['.jpg'].read() for g in got])
        finally:
            m.fb.free()
    for data in chunks[0]:
        ps = M.parse(data)
        assert (ps.w, ps.h) == (64, 48) and np.array_equal(ps.qtables, J.quant_tables(85))
        planes = M.decode(data)
        assert planes.shape == (3, 48, 64) and planes[0].max() > 0
        try:
            import PIL.Image
        except ImportError:
            continue
        im = PIL.Image.open(io.BytesIO(data))
        assert im.size == (64, 48)
        im.draft('YCbCr', im.size)
        pil = np.asarray(im).transpose(2, 0, 1).astype(np.int64)
        assert np.abs(pil[0] - planes[0]).max() <= 1        # (chroma: the decoders' upsampling filters differ, see test_cpu_mjpeg.py)
    assert len(set(chunks[0])) == 3                          # three different frames
    assert chunks[0] == chunks[1]
