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

What fl_jpeg_encode_s and fl_output_jpeg_s share with every encoder's entry points (the capacity rule, the destinations, refused
calls, fl_output_jpeg_s against fl_output) is the `jpeg_s420` row of tests/encoder_contract.py.
"""
import functools
import io

import numpy as np
import pytest

from cuburn_amd import _lib, encoders, output, render
import encoder_contract as EC
from encoder_harness import assert_jpeg_criteria, record
import jpeg420_cases as JC
import jpeg420_model as M
import jpeg_cases as JC444
import jpeg_model as J

pytestmark = pytest.mark.gpu

S444, S420 = _lib.JPEG_SAMPLING['444'], _lib.JPEG_SAMPLING['420']
ROW = EC.ROW['jpeg_s420']
mgr = EC.mgr_fixture()
stream_of = functools.partial(EC.file_of, ROW)
assert_criteria = functools.partial(assert_jpeg_criteria, sampling=S420)      # A, B and C for a 4:2:0 stream; returns the parse


def encode(mgr, planes, quality, sampling=S420):
    """fl_jpeg_encode_s into pinned memory pre-filled with the sentinel; checks the sentinel at and beyond cap."""
    return EC.encode(mgr, ROW, planes, (quality, sampling))


@pytest.fixture(scope='module')
def device_ri(mgr):
    """The library's 4:2:0 restart interval, from the record of a one-MCU frame."""
    return EC.param_of(mgr, ROW)


_done = {}


def encoded_case(mgr, name, ri):
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
    assert 16 + len(data) <= _lib.load().fl_jpeg_bound_s(planes.shape[2], planes.shape[1], S420)


def test_444_through_the_new_entry_point(mgr):
    """FL_JPEG_444 through fl_jpeg_encode_s: the bytes of fl_jpeg_encode, record included."""
    lib = _lib.load()
    for name in ('noise_17x9_q1', JC444.NOISE_Q100, 'rst_wraps'):
        planes, quality, _ = JC444.case(name, 8)
        _, h, w = planes.shape
        new, cap = encode(mgr, planes, quality, sampling=S444)
        assert cap == lib.fl_jpeg_bound(w, h)
        old, _ = EC.encode(mgr, EC.ROW['jpeg'], planes, (quality,), cap)
        assert record(old)[1] == 0 and np.array_equal(old, new)
        J.parse(stream_of(new))


def test_through_the_shim(built):
    """Three frames of a 64 x 48 config with type mjpeg: an .avi the reader accepts, whose chunks are 4:2:0 files the model parses
    and Pillow decodes at 64 x 48.  Each chunk is also the DeviceJPEGOutput(sampling='420') still of the same time from a manager
    with the same seed: a manager's frames depend on its seed and on the order of its frames only, and both managers render the
    same times in the same order."""
    times = (0.25, 0.5, 0.75)
    chunks = []
    for block in ({'type': 'mjpeg', 'quality': 85}, {'type': 'jpeg', 'device': True, 'quality': 85, 'sampling': '420'}):
        gnm, gprof = EC.small_profile(block, fps=24)
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
