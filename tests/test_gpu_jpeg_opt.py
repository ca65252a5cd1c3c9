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

What fl_jpeg_encode_f and fl_output_jpeg_f share with every encoder's entry points (the capacity rule, the destinations, refused
calls, fl_output_jpeg_f against fl_output) is in the `jpeg_f444` and `jpeg_f420` rows of tests/encoder_contract.py.
"""
import functools
import io

import numpy as np
import pytest

from cuburn_amd import _lib, encoders, output, render
import encoder_contract as EC
from encoder_harness import assert_jpeg_criteria, record
import jpeg420_model as M
import jpeg_model as J
import jpeg_opt_cases as OC
import jpeg_opt_model as O

pytestmark = pytest.mark.gpu

S444, S420 = OC.S444, OC.S420
OPT = _lib.JPEG_OPTIMIZE
ALL = [pytest.param(s, n, id='%s-%s' % ('420' if s else '444', n)) for s in (S444, S420) for n in OC.names(s)]
SAMPLINGS = [pytest.param(S444, id='444'), pytest.param(S420, id='420')]
ROW = {S444: EC.ROW['jpeg_f444'], S420: EC.ROW['jpeg_f420']}
mgr = EC.mgr_fixture()
stream_of = functools.partial(EC.file_of, ROW[S444])


def encode(mgr, planes, quality, sampling, flags=OPT):
    """fl_jpeg_encode_f into pinned memory pre-filled with the sentinel; checks the sentinel at and beyond cap."""
    return EC.encode(mgr, ROW[sampling], planes, (quality, sampling, flags))


def encode_s(mgr, planes, quality, sampling):
    return EC.encode(mgr, EC.ROW['jpeg_s420'], planes, (quality, sampling))[0]


@pytest.fixture(scope='module')
def device_ri(mgr):
    """The library's restart intervals by sampling, from the records of one-MCU frames."""
    return dict((s, EC.param_of(mgr, ROW[s])) for s in (S444, S420))


_done = {}


def encoded_case(mgr, name, sampling, ri):
    if (name, sampling) not in _done:
        planes, quality, check = OC.case(name, ri, sampling)
        buf, _ = encode(mgr, planes, quality, sampling)
        _done[(name, sampling)] = (planes, quality, check, stream_of(buf), buf)
    return _done[(name, sampling)]


@pytest.mark.parametrize('sampling,name', ALL)
def test_cases(mgr, device_ri, sampling, name):
    ri = device_ri[sampling]
    planes, quality, check, data, buf = encoded_case(mgr, name, sampling, ri)
    assert record(buf)[2] == ri
    standard = stream_of(encode_s(mgr, planes, quality, sampling))
    if name != OC.DEEP_CODE:
        (M if sampling == S420 else J).parse(standard)                              # (the parser the standard streams are held to)
    ps = assert_jpeg_criteria(data, planes, quality, ri, sampling, standard)
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
def test_flags_zero_is_the_entry_point_of_before(mgr, sampling):
    """flags = 0 through fl_jpeg_encode_f: the bytes of fl_jpeg_encode_s, record included."""
    lib = _lib.load()
    for name in OC.CASE_MODULE[sampling].NAMES[2:7]:
        planes, quality, _ = OC.case(name, 4, sampling)
        new, cap = encode(mgr, planes, quality, sampling, flags=0)
        assert cap == lib.fl_jpeg_bound_s(planes.shape[2], planes.shape[1], sampling)
        old = encode_s(mgr, planes, quality, sampling)
        assert record(old)[1] == 0 and np.array_equal(old, new)


def test_through_the_shim(built):
    """Three frames of a 64 x 48 config with type mjpeg and optimize: an .avi the reader accepts, whose chunks are optimised
    4:2:0 files the strict parser accepts and Pillow decodes at 64 x 48.  Each chunk is also the DeviceJPEGOutput(sampling='420',
    optimize=True) still of the same time from a manager with the same seed (a manager's frames depend on its seed and on the
    order of its frames only), and holds the coefficients of the file the same output writes without `optimize`."""
    times = (0.25, 0.5, 0.75)
    chunks = []
    for block in ({'type': 'mjpeg', 'quality': 85, 'optimize': True}, {'type': 'jpeg', 'device': True, 'quality': 85, 'sampling': '420', 'optimize': True},
                  {'type': 'mjpeg', 'quality': 85}):
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
