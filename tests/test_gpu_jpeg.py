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

What fl_jpeg_encode and fl_output_jpeg share with every encoder's entry points (the capacity rule, the destinations, refused
calls, fl_output_jpeg against fl_output) is the `jpeg` row of tests/encoder_contract.py.
"""
import functools
import io

import numpy as np
import pytest

from cuburn_amd import _lib, output, render
import encoder_contract as EC
from encoder_harness import record, assert_jpeg_criteria as assert_criteria
import jpeg_cases as JC
import jpeg_model as J

pytestmark = pytest.mark.gpu
ROW = EC.ROW['jpeg']
mgr = EC.mgr_fixture()
stream_of = functools.partial(EC.file_of, ROW)


def encode(mgr, planes, quality):
    """fl_jpeg_encode into pinned memory pre-filled with the sentinel; returns (buffer, cap)."""
    return EC.encode(mgr, ROW, planes, (quality,))           # (checks the sentinel at and beyond cap)


@pytest.fixture(scope='module')
def device_ri(mgr):
    """The library's restart interval, from the record of a one-block frame."""
    return EC.param_of(mgr, ROW)


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


def test_bound(mgr):
    lib = _lib.load()
    for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        assert lib.fl_jpeg_bound(w, h) == 0
    assert lib.fl_jpeg_bound(65535, 65535) > 3 * 65535 * 65535
    assert lib.fl_jpeg_bound(1, 1) == lib.fl_jpeg_bound(8, 8) > 16 + J.HEADER_BYTES + 2


def test_through_the_shim(built):
    gnm, gprof = EC.small_profile({'type': 'jpeg', 'device': True, 'quality': 90})
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
