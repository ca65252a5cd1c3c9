"""
The device JPEG encoder with optimised Huffman tables (cuburn_amd/csrc/jpeg.hip; fl_jpeg_encode_f and fl_output_jpeg_f with
FL_JPEG_OPTIMIZE) against the numpy model of tests/jpeg_opt_model.py, which tests/test_cpu_jpeg_opt.py holds to
Pillow.  For every frame of tests/jpeg_opt_cases.py, in 4:4:4 and in 4:2:0:

  A. the stream parses with the strict parser (the DHTs list the 12 / 162 legal symbols once each by (length, symbol), no
     all-ones codeword, Kraft sum 1 - 2^-Lmax; marker order, RST numbering, stuffing, padding); the header is 629 bytes; size,
     quantiser tables and restart interval are what the record and the model say;
  B. every coefficient equals that of fl_jpeg_encode_s on the same planes (the recode is lossless), and satisfies
     |c * q - v| <= q / 2 + EPS, v the model's float64 DCT value, EPS = 2^-8 as derived in tests/test_gpu_jpeg.py (the DCT is
     the same code).  No share of outliers is allowed;
  C. the model, given the device's coefficients and restart interval, reproduces the device's bytes: the counts, the DC resets,
     the table builder, the canonical order, the DHT bytes and the scan;
  D. a second encode gives the same bytes;
  E. the stream is within fl_jpeg_bound_f.
"""
import ctypes as C
import io

import numpy as np
import pytest

from cuburn_amd import _lib, configs, encoders, output, profile, render
import encoder_harness as H
from encoder_harness import SENTINEL, SLACK, assert_untouched, record, upload
import jpeg420_model as M
import jpeg_model as J
import jpeg_opt_cases as OC
import jpeg_opt_model as O

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -8
S444, S420 = OC.S444, OC.S420
OPT = _lib.JPEG_OPTIMIZE
ALL = [pytest.param(s, n, id='%s-%s' % ('420' if s else '444', n)) for s in (S444, S420) for n in OC.names(s)]
SAMPLINGS = [pytest.param(S444, id='444'), pytest.param(S420, id='420')]
NOISE_Q100 = 'noise_64x40_q100'                    # in both case modules


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
    m.fb.free()


def encode(mgr, planes, quality, sampling, flags=OPT, cap=None, buf=None):
    """fl_jpeg_encode_f into pinned memory (or `buf`) pre-filled with the sentinel; checks the sentinel at and beyond cap."""
    _, h, w = planes.shape
    if cap is None:
        cap = _lib.load().fl_jpeg_bound_f(w, h, sampling, flags)
    return H.encode(mgr, 'fl_jpeg_encode_f', planes, w, h, (quality, sampling, flags), cap, buf)


def encode_s(mgr, planes, quality, sampling):
    _, h, w = planes.shape
    cap = _lib.load().fl_jpeg_bound_s(w, h, sampling)
    return H.encode(mgr, 'fl_jpeg_encode_s', planes, w, h, (quality, sampling), cap)[0]


def stream_of(buf):
    nbytes, status, ri = record(buf)
    assert status == 0
    return bytes(buf[16:16 + nbytes])


@pytest.fixture(scope='module')
def device_ri(mgr):
    """The library's restart intervals by sampling, from the records of one-MCU frames."""
    ri = {}
    for s in (S444, S420):
        buf, _ = encode(mgr, np.zeros((3, 16 if s else 8, 16 if s else 8), np.uint8), 50, s)
        ri[s] = record(buf)[2]
        assert 1 <= ri[s] <= (10 if s else 21)
    return ri


_done = {}


def encoded_case(mgr, name, sampling, ri):
    if (name, sampling) not in _done:
        planes, quality, check = OC.case(name, ri, sampling)
        buf, _ = encode(mgr, planes, quality, sampling)
        _done[(name, sampling)] = (planes, quality, check, stream_of(buf), buf)
    return _done[(name, sampling)]


def assert_criteria(data, planes, quality, sampling, ri, standard):
    """A, B and C for an optimised stream; `standard` is the stream fl_jpeg_encode_s wrote from the same planes.  Returns the parse."""
    mod = M if sampling == S420 else J
    assert len(data) >= O.HEADER_BYTES + 2
    ps = O.parse(data)                                                              # A
    qt = J.quant_tables(quality)
    assert (ps.w, ps.h, ps.sampling) == (planes.shape[2], planes.shape[1], sampling) and ps.restart_interval == ri
    assert np.array_equal(ps.qtables, qt)
    assert np.array_equal(ps.coefficients, O.parse(standard, optimised=False).coefficients)      # B
    v = mod.dct_values(planes)
    qz = M._qz(qt)[None].astype(np.float64) if sampling == S420 else np.stack([qt[0], qt[1], qt[1]])[:, J.ZIGZAG][:, None, :].astype(np.float64)
    err = np.abs(ps.coefficients * qz - v) - qz / 2
    print('largest |c q - v| - q / 2: %.3g (EPS %.3g)' % (err.max(), EPS))
    assert (err <= EPS).all(), '%d coefficients beyond q / 2 + EPS, worst by %g' % (int((err > EPS).sum()), err.max())
    assert O.assemble(ps.w, ps.h, qt, ri, ps.coefficients, sampling) == data        # C
    return ps


@pytest.mark.parametrize('sampling,name', ALL)
def test_cases(mgr, device_ri, sampling, name):
    ri = device_ri[sampling]
    planes, quality, check, data, buf = encoded_case(mgr, name, sampling, ri)
    assert record(buf)[2] == ri
    standard = stream_of(encode_s(mgr, planes, quality, sampling))
    if name != OC.DEEP_CODE:
        (M if sampling == S420 else J).parse(standard)                              # (the parser the standard streams are held to)
    ps = assert_criteria(data, planes, quality, sampling, ri, standard)
    check(ps.stats, ri)
    print('%s: standard %d bytes, optimised %d' % (name, len(standard), len(data)))
    again, _ = encode(mgr, planes, quality, sampling)                               # D
    assert stream_of(again) == data
    assert 16 + len(data) <= _lib.load().fl_jpeg_bound_f(planes.shape[2], planes.shape[1], sampling, OPT)      # E


@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_deep_code_reaches_the_limit(mgr, device_ri, sampling):
    """Both AC tables of deep_code hold codes of 16 bits on the device, where Huffman's own would be longer."""
    ri = device_ri[sampling]
    _, _, _, data, _ = encoded_case(mgr, OC.DEEP_CODE, sampling, ri)
    ps = O.parse(data)
    cnt = O.counts(ps.coefficients, ri, sampling)
    assert O.unlimited_depth(cnt[1], 1) > 16 and O.unlimited_depth(cnt[3], 1) > 16
    assert [max(l for l in range(1, 17) if t[0][l - 1]) for t in (ps.tables[1], ps.tables[3])] == [16, 16]


@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_capacity(mgr, device_ri, sampling):
    ri = device_ri[sampling]
    planes, quality, _, data, _ = encoded_case(mgr, NOISE_Q100, sampling, ri)
    need = len(data)
    for cap in (16 + need - 1, 16 + O.HEADER_BYTES):
        buf, cap = encode(mgr, planes, quality, sampling, cap=cap)                  # (checks the sentinel at and beyond cap)
        assert record(buf) == (need, 1, ri)
    buf, cap = encode(mgr, planes, quality, sampling, cap=16 + need)
    assert record(buf) == (need, 0, ri) and stream_of(buf) == data


@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_flags_zero_is_the_entry_point_of_before(mgr, sampling):
    """flags = 0 through fl_jpeg_encode_f: the bytes of fl_jpeg_encode_s, record included."""
    lib = _lib.load()
    for name in OC.CASE_MODULE[sampling].NAMES[2:7]:
        planes, quality, _ = OC.case(name, 4, sampling)
        new, cap = encode(mgr, planes, quality, sampling, flags=0)
        assert cap == lib.fl_jpeg_bound_s(planes.shape[2], planes.shape[1], sampling)
        old = encode_s(mgr, planes, quality, sampling)
        assert record(old)[1] == 0 and np.array_equal(old, new)


@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_bad_arguments(mgr, device_ri, sampling):
    lib = _lib.load()
    planes, quality, _, data, _ = encoded_case(mgr, NOISE_Q100, sampling, device_ri[sampling])
    _, h, w = planes.shape
    t = upload(mgr, planes)
    cap = lib.fl_jpeg_bound_f(w, h, sampling, OPT)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    ctx, src, dst, s = mgr.fb.ctx, t.data_ptr(), buf.ctypes.data, sampling
    bad = [(w, h, src, quality, s, 2, dst, 0, cap), (w, h, src, quality, s, 3, dst, 0, cap), (w, h, src, quality, s, 0x80000001, dst, 0, cap),
           (w, h, src, quality, 2, OPT, dst, 0, cap), (w, h, src, quality, -1, OPT, dst, 0, cap),
           (w, h, src, 0, s, OPT, dst, 0, cap), (w, h, src, 101, s, OPT, dst, 0, cap), (0, h, src, quality, s, OPT, dst, 0, cap),
           (w, 65536, src, quality, s, OPT, dst, 0, cap), (w, h, 0, quality, s, OPT, dst, 0, cap),
           (w, h, src, quality, s, OPT, dst, 0, 16 + O.HEADER_BYTES - 1), (w, h, src, quality, s, OPT, None, 0, cap)]
    for args in bad:
        assert lib.fl_jpeg_encode_f(ctx, *args) == _lib.FL_E_INVAL, args
        assert lib.fl_last_error()
    for args in bad:
        if args[2]:
            assert lib.fl_output_jpeg_f(ctx, *(args[:2] + args[3:])) == _lib.FL_E_INVAL, args
    # more than 2^24 blocks: refused before the source is looked at or anything is queued
    assert lib.fl_jpeg_encode_f(ctx, 30000, 30000, src, quality, s, OPT, dst, 0, cap) == _lib.FL_E_UNSUPPORTED
    assert lib.fl_output_jpeg_f(ctx, 30000, 30000, quality, s, OPT, dst, 0, cap) == _lib.FL_E_UNSUPPORTED
    _lib.check(lib.fl_ctx_sync(ctx))
    assert (buf == SENTINEL).all()
    good, _ = encode(mgr, planes, quality, sampling)
    assert stream_of(good) == data


@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_pageable_memory(mgr, device_ri, sampling):
    """A destination that is not pinned receives a copy; the bytes are the same."""
    ri = device_ri[sampling]
    planes, quality, _, data, _ = encoded_case(mgr, NOISE_Q100, sampling, ri)
    cap = _lib.load().fl_jpeg_bound_f(planes.shape[2], planes.shape[1], sampling, OPT)
    buf, _ = encode(mgr, planes, quality, sampling, buf=np.empty(cap + SLACK, np.uint8))
    assert stream_of(buf) == data
    buf, _ = encode(mgr, planes, quality, sampling, cap=16 + len(data) - 1, buf=np.empty(16 + len(data) + SLACK, np.uint8))
    assert record(buf) == (len(data), 1, ri)


@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_device_destination(mgr, device_ri, sampling):
    import torch
    lib = _lib.load()
    planes, quality, _, data, _ = encoded_case(mgr, NOISE_Q100, sampling, device_ri[sampling])
    _, h, w = planes.shape
    cap = 16 + len(data) + 7
    t = upload(mgr, planes)
    for odd in (1, 2, 3):
        out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device=t.device)
        torch.cuda.synchronize(mgr.fb.device)
        host = mgr.fb._pinned((cap + SLACK,), 'u1')
        host[:] = SENTINEL
        _lib.check(lib.fl_jpeg_encode_f(mgr.fb.ctx, w, h, t.data_ptr(), quality, sampling, OPT, host.ctypes.data, out.data_ptr() + odd, cap))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        dev = out.cpu().numpy()
        assert (dev[:odd] == SENTINEL).all() and (dev[odd + cap:] == SENTINEL).all() and (host[cap:] == SENTINEL).all()
        assert stream_of(dev[odd:]) == data and stream_of(host) == data


@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_whole_path(mgr, device_ri, sampling):
    """fl_output_jpeg_f = fl_output(FL_OUT_YUV444P) + the encode: same planes, same dither states afterwards, a closed frame."""
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
    mgr.timings_reset()
    cap = lib.fl_jpeg_bound_f(w, h, sampling, OPT)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    _lib.check(lib.fl_output_jpeg_f(mgr.fb.ctx, w, h, quality, sampling, OPT, buf.ctypes.data, 0, cap))
    ms = C.c_float(-1.0)
    _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
    assert ms.value >= 0.0
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    assert_untouched(buf, cap)
    assert np.array_equal(mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32), after_plain)
    assert mgr.timings()['jpeg_ms'] > 0.0          # fl_timings_detail[5]: the encode's kernels, the new ones among them
    standard = stream_of(encode_s(mgr, planes, quality, sampling))
    assert_criteria(stream_of(buf), planes, quality, sampling, device_ri[sampling], standard)


def _small(block):
    gnm, prof = configs.cfg2(samples=2 ** 22)
    prof = dict(prof, width=64, height=48, spp=2 ** 22 / (64.0 * 48.0), fps=24, output=block)
    return gnm, profile.wrap(prof, gnm)


def test_through_the_shim(built):
    """Three frames of a 64 x 48 config with type mjpeg and optimize: an .avi the reader accepts, whose chunks are optimised
    4:2:0 files the strict parser accepts and Pillow decodes at 64 x 48.  Each chunk is also the DeviceJPEGOutput(sampling='420',
    optimize=True) still of the same time from a manager with the same seed (a manager's frames depend on its seed and on the
    order of its frames only), and holds the coefficients of the file the same output writes without `optimize`."""
    times = (0.25, 0.5, 0.75)
    chunks = []
    for block in ({'type': 'mjpeg', 'quality': 85, 'optimize': True}, {'type': 'jpeg', 'device': True, 'quality': 85, 'sampling': '420', 'optimize': True},
                  {'type': 'mjpeg', 'quality': 85}):
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
                assert type(rdr.out) is encoders.MJPEGOutput and rdr.out.optimize is bool(block.get('optimize')) and got == [{}, {}, {}]
                media, logs = rdr.out.encode(None)
                assert list(media) == ['.avi'] and logs == []
                avi = M.read_avi(media['.avi'].read())
                assert len(avi.chunks) == 3 and (avi.avih['dwWidth'], avi.avih['dwHeight']) == (64, 48)
                chunks.append(avi.chunks)
            else:
                assert type(rdr.out) is output.DeviceJPEGOutput and rdr.out.optimize is True
                chunks.append([g['.jpg'].read() for g in got])
        finally:
            m.fb.free()
    for data, plain in zip(chunks[0], chunks[2]):
        ps = O.parse(data)
        assert (ps.w, ps.h, ps.sampling) == (64, 48, S420) and np.array_equal(ps.qtables, J.quant_tables(85))
        std = M.parse(plain)
        assert np.array_equal(ps.coefficients, std.coefficients)
        assert O.assemble(64, 48, ps.qtables, ps.restart_interval, ps.coefficients, S420) == data
        print('frame: standard %d bytes, optimised %d' % (len(plain), len(data)))
        try:
            import PIL.Image
        except ImportError:
            continue
        ims = []
        for d in (data, plain):
            im = PIL.Image.open(io.BytesIO(d))
            assert im.size == (64, 48)
            im.draft('YCbCr', im.size)
            ims.append(np.asarray(im))
        assert np.array_equal(ims[0], ims[1]) and ims[0][:, :, 0].max() > 0
    assert len(set(chunks[0])) == 3                          # three different frames
    assert chunks[0] == chunks[1]
