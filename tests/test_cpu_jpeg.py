"""
CPU tests of the device JPEG output (no GPU): the numpy model of tests/jpeg_model.py against Pillow, the model's entropy coder
and parser against each other on every edge case of tests/jpeg_cases.py, DeviceJPEGOutput and the profile / command-line
plumbing against a stand-in library, and the C ABI's three entry points.
"""
import argparse
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, output, profile, render
import jpeg_cases as JC
import jpeg_model as J

QUALITIES = (1, 50, 75, 95, 100)


def pillow_ycc(data):
    """Pillow's decode without its colour conversion; the tests that rest on Pillow skip without it."""
    PIL_Image = pytest.importorskip('PIL.Image')
    im = PIL_Image.open(io.BytesIO(data))
    im.draft('YCbCr', im.size)
    assert im.mode == 'YCbCr'
    return im, np.asarray(im).transpose(2, 0, 1).astype(np.int64)


# ------------------------------------------------------------------ the model against Pillow
@pytest.mark.parametrize('quality', QUALITIES)
def test_model_files_open_in_pillow(quality):
    """Pillow (libjpeg's integer IDCT, accuracy class IEEE 1180: within 1 level) decodes the model's files to within 1 level of
    the model's float64 decode.  Measured maximum over these frames: 1 at every quality (0 for the 1 x 1 frame)."""
    rs = np.random.RandomState(quality)
    for w, h, ri in ((250, 37, 8), (17, 9, 2), (1, 1, 8), (64, 48, 21)):
        planes = rs.randint(0, 256, (3, h, w)).astype(np.uint8)
        smooth = np.clip(planes.astype(np.int64) // 8 + np.arange(w)[None, None, :] * 3 + np.arange(h)[None, :, None], 0, 255).astype(np.uint8)
        for p in (planes, smooth):
            data = J.encode(p, quality, ri)
            im, pil = pillow_ycc(data)
            assert im.size == (w, h)
            qt = J.quant_tables(quality)
            assert [list(im.quantization[t]) for t in (0, 1)] == [list(qt[t]) for t in (0, 1)]
            diff = np.abs(pil - J.decode(data).astype(np.int64)).max()
            print('quality %d %dx%d: Pillow vs model decode, max %d' % (quality, w, h, diff))
            assert diff <= 1


@pytest.mark.parametrize('quality', QUALITIES)
def test_tables_are_the_ones_pillow_writes(quality):
    PIL_Image = pytest.importorskip('PIL.Image')
    out = io.BytesIO()
    PIL_Image.fromarray(np.zeros((8, 8, 3), np.uint8), 'YCbCr').save(out, 'jpeg', quality=quality, subsampling=0)
    data = out.getvalue()
    theirs = PIL_Image.open(io.BytesIO(data)).quantization
    qt = J.quant_tables(quality)
    assert [list(theirs[t]) for t in (0, 1)] == [list(qt[t]) for t in (0, 1)]
    if quality == 100:
        assert (qt == 1).all()
    # ... and the four Huffman tables: libjpeg writes Annex K.3-K.6 into every file that is not optimised
    mine = J.header(8, 8, qt, 1)
    a, b = mine.index(b'\xff\xc4'), mine.index(b'\xff\xdd')
    assert data[data.index(b'\xff\xc4'):][:b - a] == mine[a:b]


# ------------------------------------------------------------------ the model against itself, on every edge case
@pytest.mark.parametrize('name', JC.NAMES)
def test_cases_contain_their_edge(name):
    planes, quality, check = JC.case(name, JC.MODEL_RI)
    data = J.encode(planes, quality, JC.MODEL_RI)
    ps = J.parse(data)
    qt = J.quant_tables(quality)
    assert (ps.w, ps.h, ps.restart_interval) == (planes.shape[2], planes.shape[1], JC.MODEL_RI)
    assert np.array_equal(ps.qtables, qt)
    assert np.array_equal(ps.coefficients, J.quantise(J.dct_values(planes), qt))
    assert J.assemble(ps.w, ps.h, ps.qtables, ps.restart_interval, ps.coefficients) == data
    assert J.header(ps.w, ps.h, qt, JC.MODEL_RI) + J.entropy_encode(ps.coefficients, JC.MODEL_RI) + b'\xff\xd9' == data
    check(ps.stats, JC.MODEL_RI)
    assert sum(ps.stats['interval_bytes']) + 2 * len(ps.stats['rst']) + 2 + J.HEADER_BYTES == len(data)
    try:
        import PIL.Image      # noqa: F401
    except ImportError:
        return
    _, pil = pillow_ycc(data)
    assert np.abs(pil - J.decode(data).astype(np.int64)).max() <= 1


@pytest.mark.parametrize('ri', (1, 3, 21))
def test_other_restart_intervals(ri):
    planes, quality, _ = JC.case('noise_250x37_q50', ri)
    data = J.encode(planes, quality, ri)
    ps = J.parse(data)
    assert ps.restart_interval == ri and ps.stats['intervals'] == -(-160 // ri)
    assert ps.stats['rst'] == [k & 7 for k in range(ps.stats['intervals'] - 1)]
    assert np.array_equal(ps.coefficients, J.parse(J.encode(planes, quality, 8)).coefficients)


def test_parser_refuses_broken_streams():
    planes, quality, _ = JC.case(JC.NOISE_Q100, 8)
    data = J.encode(planes, quality, 8)
    J.parse(data)
    rst = data.index(b'\xff\xd0', J.HEADER_BYTES)
    broken = [data[:-2], data + b'\0', data[:rst + 1] + b'\xd1' + data[rst + 2:],                  # no EOI, a trailing byte, RST1 for RST0
              data[:rst - 1] + bytes([data[rst - 1] & 0xfe]) + data[rst:],                          # a padding bit of 0
              data[:20] + b'\x02' + data[21:]]                                                      # another APP0
    stuffed = data.index(b'\xff\x00', J.HEADER_BYTES)
    broken.append(data[:stuffed + 1] + data[stuffed + 2:])                                          # an unstuffed 0xFF
    for bad in broken:
        with pytest.raises(J.JpegError):
            J.parse(bad)


# ------------------------------------------------------------------ DeviceJPEGOutput and the plumbing, against a stand-in library
class StubLib(object):
    def __init__(self, stream=b'\xff\xd8stream\xff\xd9', status=0):
        self.calls, self.stream, self.status = [], stream, status

    def fl_output_jpeg(self, ctx, w, h, quality, host, dev, cap):
        self.calls.append((ctx, w, h, quality, host, dev, cap))
        if host:
            rec = np.array([len(self.stream), self.status, 8, 0], '<u4').tobytes() + (b'' if self.status else self.stream)
            C.memmove(host, rec, len(rec))
        return 0


class StubFB(object):
    ctx = 1234

    def host_buffer(self, shape, dtype):
        self.last = np.zeros(shape, dtype)
        return self.last


def test_device_output_class(monkeypatch):
    stub = StubLib()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    out = output.DeviceJPEGOutput(quality=85)
    dim = render.Framebuffers.calc_dim(64, 48)
    cap = 16 + J.HEADER_BYTES + 2 * 3 * 64 * 48
    assert out.shape(dim) == (cap,) and np.dtype(out.dtype) == np.uint8 and out.suffix == '.jpg'
    fb = StubFB()
    buf = out.copy(fb, dim)
    assert buf is fb.last and buf.shape == (cap,)
    assert stub.calls == [(1234, 64, 48, 85, buf.ctypes.data, 0, cap)]
    media, logs = out.encode(buf)
    assert list(media) == ['.jpg'] and media['.jpg'].read() == stub.stream and logs == []
    assert out.encode(None) == ({}, [])
    assert out.copy(fb, dim, dev_out=4096, host=False) is None and stub.calls[-1][4:6] == (None, 4096)
    # status 1: the needed size is reported
    stub.status = 1
    with pytest.raises(_lib.FlameError, match=str(len(stub.stream))):
        out.encode(out.copy(fb, dim))


def test_profile_selects_the_output():
    gnm, prof = configs.cfg2()

    def out_for(block):
        return output.get_output_for_profile(profile.wrap(dict(prof, output=block), gnm))

    dev = out_for({'type': 'jpeg', 'device': True, 'quality': 70})
    assert isinstance(dev, output.DeviceJPEGOutput) and dev.quality == 70
    assert out_for({'type': 'jpeg', 'device': True}).quality == 100
    assert isinstance(out_for({'device': True}), output.DeviceJPEGOutput)            # the default type is jpeg
    for block in ({'type': 'jpeg'}, {'type': 'jpeg', 'device': False, 'quality': 70}, {}):
        plain = out_for(block)
        assert type(plain) is output.PILOutput and plain.type == 'jpeg' and plain.quality == block.get('quality', 100)
    for block in ({'type': 'jpeg', 'device': True, 'alpha': True}, {'type': 'png', 'device': True}, {'type': 'raw', 'device': True},
                  {'type': 'jpeg', 'device': True, 'quality': 0}, {'type': 'jpeg', 'device': True, 'quality': 101},
                  {'type': 'jpeg', 'device': True, 'quality': 7.5}):
        with pytest.raises(ValueError):
            out_for(block)
    assert output.get_suffix_for_profile(profile.wrap(dict(prof, output={'type': 'jpeg', 'device': True}), gnm)) == '.jpg'


def test_command_line_options():
    parser = profile.add_args(argparse.ArgumentParser())
    _, prof = profile.get_from_args(parser.parse_args(['--device-encode', '--quality', '92']))
    assert prof['output'] == {'device': True, 'quality': 92}
    _, prof = profile.get_from_args(parser.parse_args(['--codec', 'jpeg', '--quality', '80']))
    assert prof['output'] == {'type': 'jpeg', 'quality': 80}
    _, prof = profile.get_from_args(parser.parse_args([]))
    assert 'output' not in prof


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_jpeg_bound', 'fl_jpeg_encode', 'fl_output_jpeg'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert int(re.search(r'#define\s+FL_JPEG_HEADER_BYTES\s+(\d+)', code).group(1)) == J.HEADER_BYTES == _lib.JPEG_HEADER_BYTES
    # host-only entry point: usable without a GPU
    assert lib.fl_jpeg_bound(0, 8) == 0 and lib.fl_jpeg_bound(8, 65536) == 0
    assert lib.fl_jpeg_bound(1920, 1080) == 16 + J.HEADER_BYTES + 240 * 135 * 1248
    # the worst block: 22 bits of DC, 63 coefficients of 16 + 10 bits
    longest = dict((k, max(ln for _, ln in J.huff_codes(t).values())) for k, t in
                   (('dc', J.DC_CHR), ('dcl', J.DC_LUM), ('acl', J.AC_LUM), ('acc', J.AC_CHR)))
    assert longest == {'dc': 11, 'dcl': 9, 'acl': 16, 'acc': 16}
    assert 2 * -(-3 * (11 + 11 + 63 * 26) // 8) + 2 == 1248
    for bad in ((None, 8, 8, 1, 50, None, 0, 4096), (None, 8, 8, 1, 50, 1, 0, 4096)):
        assert lib.fl_jpeg_encode(*bad) == _lib.FL_E_INVAL            # (a null context or no destination: refused before the device is touched)
