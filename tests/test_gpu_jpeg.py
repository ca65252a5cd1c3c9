"""
The device JPEG encoder (cuburn_amd/csrc/jpeg.hip; fl_jpeg_encode, fl_output_jpeg, DeviceJPEGOutput) against the numpy model of
tests/jpeg_model.py, which tests/test_cpu_jpeg.py holds to Pillow.  For every frame of tests/jpeg_cases.py:

  A. the stream parses (marker order, RST numbering, stuffing, padding), and its size, tables and restart interval are what the
     record and the model say;
  B. every coefficient c satisfies |c * q - v| <= q / 2 + EPS, v the model's float64 DCT value: the device quantised a value
     within EPS of the exact one to the nearest integer.  No share of outliers is allowed;
  C. the model's entropy coder, given the device's own coefficients and restart interval, reproduces the device's bytes;
  D. a second encode gives the same bytes.

EPS, the float32 DCT's error bound: a coefficient is a sum over the 64 samples of w * f with |w| <= 1/4 (the product of two
factors 0.5 * C * cos) and |f| <= 128, so the magnitudes sum to at most 64 * 32 = 2048 (the value itself stays within 1024).
Evaluated separably in float32 — two sums of eight products each — every term passes through at most 2 roundings of the
constants, 2 of the products and 2 * 7 of the additions, 18 in all, each of relative size 2^-24: the error is at most
18 * 2^-24 * 2048 (first order; the float32 division adds one more rounding of a quotient below 1024, which the bound's slack
covers).  EPS = 32 * 2^-24 * 2048 = 2^-8.
"""
import ctypes as C
import io

import numpy as np
import pytest

from cuburn_amd import _lib, configs, output, profile, render
import encoder_harness as H
from encoder_harness import SENTINEL, SLACK, record, upload, assert_jpeg_criteria as assert_criteria
import jpeg_cases as JC
import jpeg_model as J

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
    m.fb.free()


def encode(mgr, planes, quality, cap=None, buf=None):
    """fl_jpeg_encode into pinned memory (or `buf`) pre-filled with the sentinel; returns (buffer, cap)."""
    _, h, w = planes.shape
    if cap is None:
        cap = _lib.load().fl_jpeg_bound(w, h)
    return H.encode(mgr, 'fl_jpeg_encode', planes, w, h, (quality,), cap, buf)       # (checks the sentinel at and beyond cap)


def stream_of(buf):
    nbytes, status, ri = record(buf)
    assert status == 0
    return bytes(buf[16:16 + nbytes])


@pytest.fixture(scope='module')
def device_ri(mgr):
    """The library's restart interval, from the record of a one-block frame."""
    buf, _ = encode(mgr, np.zeros((3, 8, 8), np.uint8), 50)
    ri = record(buf)[2]
    assert 1 <= ri <= 65535
    return ri


_done = {}


def encoded_case(mgr, name, ri):
    """(planes, quality, check, stream, buffer) of a case, encoded once per session."""
    if name not in _done:
        planes, quality, check = JC.case(name, ri)
        buf, _ = encode(mgr, planes, quality)
        _done[name] = (planes, quality, check, stream_of(buf), buf)
    return _done[name]


@pytest.mark.parametrize('name', JC.NAMES)
def test_cases(mgr, device_ri, name):
    planes, quality, check, data, buf = encoded_case(mgr, name, device_ri)
    assert record(buf)[2] == device_ri
    ps = assert_criteria(data, planes, quality, device_ri)
    check(ps.stats, device_ri)
    again, _ = encode(mgr, planes, quality)                                          # D
    assert stream_of(again) == data
    bound = _lib.load().fl_jpeg_bound(planes.shape[2], planes.shape[1])
    assert 16 + len(data) <= bound


def test_capacity(mgr, device_ri):
    planes, quality, _, data, _ = encoded_case(mgr, JC.NOISE_Q100, device_ri)
    need = len(data)
    for cap in (16 + need - 1, 16 + J.HEADER_BYTES, 16 + need - 1000):
        buf, cap = encode(mgr, planes, quality, cap=cap)                             # (checks the sentinel at and beyond cap)
        assert record(buf) == (need, 1, device_ri)
    buf, cap = encode(mgr, planes, quality, cap=16 + need)
    assert record(buf) == (need, 0, device_ri) and stream_of(buf) == data


def test_bound(mgr):
    lib = _lib.load()
    for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        assert lib.fl_jpeg_bound(w, h) == 0
    assert lib.fl_jpeg_bound(65535, 65535) > 3 * 65535 * 65535
    assert lib.fl_jpeg_bound(1, 1) == lib.fl_jpeg_bound(8, 8) > 16 + J.HEADER_BYTES + 2


def test_bad_arguments(mgr, device_ri):
    lib = _lib.load()
    planes, quality, _, data, _ = encoded_case(mgr, JC.NOISE_Q100, device_ri)
    _, h, w = planes.shape
    t = upload(mgr, planes)
    cap = lib.fl_jpeg_bound(w, h)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    ctx, src, dst = mgr.fb.ctx, t.data_ptr(), buf.ctypes.data
    bad = [(w, h, src, 0, dst, 0, cap), (w, h, src, 101, dst, 0, cap), (w, h, src, -5, dst, 0, cap),
           (0, h, src, quality, dst, 0, cap), (w, 0, src, quality, dst, 0, cap), (65536, h, src, quality, dst, 0, cap),
           (w, 65536, src, quality, dst, 0, cap), (w, h, 0, quality, dst, 0, cap),
           (w, h, src, quality, dst, 0, 16 + J.HEADER_BYTES - 1), (w, h, src, quality, None, 0, cap)]
    for args in bad:
        assert lib.fl_jpeg_encode(ctx, *args) == _lib.FL_E_INVAL, args
        assert lib.fl_last_error()
    for args in bad:
        if args[2]:
            assert lib.fl_output_jpeg(ctx, *(args[:2] + args[3:])) == _lib.FL_E_INVAL, args
    _lib.check(lib.fl_ctx_sync(ctx))
    assert (buf == SENTINEL).all()
    good, _ = encode(mgr, planes, quality)
    assert stream_of(good) == data


def test_pageable_memory(mgr, device_ri):
    """A destination that is not pinned receives a copy; the bytes are the same."""
    planes, quality, _, data, _ = encoded_case(mgr, JC.NOISE_Q100, device_ri)
    cap = _lib.load().fl_jpeg_bound(planes.shape[2], planes.shape[1])
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
        _lib.check(lib.fl_jpeg_encode(mgr.fb.ctx, w, h, t.data_ptr(), quality, host.ctypes.data, out.data_ptr() + odd, cap))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        dev = out.cpu().numpy()
        assert (dev[:odd] == SENTINEL).all() and (dev[odd + cap:] == SENTINEL).all() and (host[cap:] == SENTINEL).all()
        assert stream_of(dev[odd:]) == data and stream_of(host) == data


def test_whole_path(mgr, device_ri):
    """fl_output_jpeg = fl_output(FL_OUT_YUV444P) + the encode: same planes, same dither states afterwards, a closed frame."""
    lib = _lib.load()
    w, h, quality = 64, 48, 90
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
    cap = lib.fl_jpeg_bound(w, h)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    _lib.check(lib.fl_output_jpeg(mgr.fb.ctx, w, h, quality, buf.ctypes.data, 0, cap))
    ms = C.c_float(-1.0)
    _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
    assert ms.value >= 0.0
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    assert (buf[cap:] == SENTINEL).all()
    assert_criteria(stream_of(buf), planes, quality, device_ri)
    assert np.array_equal(mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32), after_plain)
    assert mgr.timings()['jpeg_ms'] > 0.0          # fl_timings_detail[5]: the encode's kernels


def test_through_the_shim(built):
    gnm, prof = configs.cfg2(samples=2 ** 22)
    prof = dict(prof, width=64, height=48, spp=2 ** 22 / (64.0 * 48.0), output={'type': 'jpeg', 'device': True, 'quality': 90})
    gprof = profile.wrap(prof, gnm)
    m = render.RenderManager(device=0, host_seed=7)
    try:
        rdr = render.Renderer(gnm, gprof)
        assert isinstance(rdr.out, output.DeviceJPEGOutput)
        evt, h_out = m.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
        assert h_out.shape == rdr.out.shape(m.fb.calc_dim(64, 48)) and h_out.dtype == np.uint8
        media, logs = rdr.out.encode(h_out)
        assert list(media) == ['.jpg'] and logs == []
        data = media['.jpg'].read()
        planes = J.decode(data)
        assert planes.shape == (3, 48, 64) and planes[0].max() > 0
        try:
            import PIL.Image
        except ImportError:
            return
        im = PIL.Image.open(io.BytesIO(data))
        assert im.size == (64, 48)
        im.draft('YCbCr', im.size)
        pil = np.asarray(im).transpose(2, 0, 1).astype(np.int64)
        assert np.abs(pil - planes).max() <= 1
    finally:
        m.fb.free()
