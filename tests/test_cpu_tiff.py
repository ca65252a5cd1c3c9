"""
CPU tests of the device TIFF encoder's format (no GPU): the model of tests/tiff_model.py is held to Pillow (libtiff) and to its own
reader on the frames tests/test_gpu_tiff.py gives the device; the predictor is shown to be word arithmetic; the mixed frame is shown
to hold both block types and a pad byte before any device sees it; and the C ABI's three entry points, DeviceTIFFOutput, the
profile key and the command line are driven, the output against a stand-in library.
"""
import argparse
import ctypes as C
import io
import os
import re
import struct
import zlib

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, output, profile, render
import png_model as P
import tiff_cases as TC
import tiff_model as T


def roundtrip(src, ch, bits):
    """Model encode -> the model's reader; returns (file, parse)."""
    data = T.encode(src, ch, bits)
    ps = T.parse(data)
    assert (ps.w, ps.h, ps.channels, ps.bits) == (src.shape[1], src.shape[0], ch, bits)
    assert ps.samples.dtype == src.dtype and np.array_equal(ps.samples, src[:, :, :ch])
    assert 16 + len(data) <= T.bound(ps.w, ps.h, ch, bits)
    assert T.encode(src, ch, bits) == data
    return data, ps


# ------------------------------------------------------------------ the model against Pillow and against its own reader
@pytest.mark.parametrize('form', TC.FORMS, ids=TC.form_id)
def test_model_opens_in_pillow(form):
    bits, ch = form
    PIL_Image = pytest.importorskip('PIL.Image')              # (without Pillow the test shows as skipped, not as passed)
    tw = T.tile_width(bits)
    for w, h in ((1, 1), (tw + 1, 65), (7, 1)):
        src = TC.noise(w, h, bits, 5 * w + h)
        im = PIL_Image.open(io.BytesIO(T.encode(src, ch, bits)))
        assert im.size == (w, h) and im.mode == ('RGB' if ch == 3 else 'RGBA')
        got = np.asarray(im)
        assert np.array_equal(got, src[:, :, :ch] if bits == 8 else (src[:, :, :ch] >> 8).astype(np.uint8))      # Pillow keeps the high bytes of 16-bit truecolour
    src = TC.mixed(bits, TC.MIXED_SEED[form])
    got = np.asarray(PIL_Image.open(io.BytesIO(T.encode(src, ch, bits))))
    assert np.array_equal(got, src[:, :, :ch] if bits == 8 else (src[:, :, :ch] >> 8).astype(np.uint8))


@pytest.mark.parametrize('form', TC.FORMS, ids=TC.form_id)
def test_model_against_its_own_reader(form):
    bits, ch = form
    for w, h in TC.reader_shapes(bits) + TC.small_shapes() + TC.edge_shapes(bits) + ((1, 200),):
        data, ps = roundtrip(TC.noise(w, h, bits, 3 * w + h) // 5, ch, bits)
        tw, nx, ny = T.geometry(w, h, bits)
        assert ps.nt == nx * ny == len(ps.streams) and ps.tw == tw
        assert len(data) >= T.header_bytes(w, h, ch, bits) + 8 * ps.nt
        for s, d in zip(ps.streams, T.tiles(TC.noise(w, h, bits, 3 * w + h) // 5, ch, bits)):
            assert zlib.decompress(s) == d and len(d) == T.tile_bytes(ch, bits) and s[-4:] == struct.pack('>I', zlib.adler32(d))


def test_one_tile_is_inline_and_two_are_not():
    data, ps = roundtrip(TC.noise(3, 2, 8, 1), 3, 8)
    H = T.header_bytes(3, 2, 3, 8)
    assert H == 8 + 2 + 12 * 12 + 4 + 6 and ps.offsets == [H] and ps.counts == [len(data) - H]
    assert data[10 + 12 * 10:10 + 12 * 11] == struct.pack('<HHII', 324, 4, 1, H)
    assert data[10 + 12 * 11:10 + 12 * 12] == struct.pack('<HHII', 325, 4, 1, len(data) - H)
    data, ps = roundtrip(TC.noise(129, 2, 8, 1), 4, 8)
    H = T.header_bytes(129, 2, 4, 8)
    assert H == 8 + 2 + 12 * 13 + 4 + 8 + 16 and ps.offsets[0] == H and ps.nt == 2
    assert data[10 + 12 * 10:10 + 12 * 11] == struct.pack('<HHII', 324, 4, 2, H - 16)
    assert data[10 + 12 * 12:10 + 12 * 13] == struct.pack('<HHIHH', 338, 3, 1, 2, 0)


def test_reader_refuses_what_breaks_a_rule():
    src = TC.mixed(8, TC.MIXED_SEED[(8, 3)])
    data = T.encode(src, 3, 8)
    ps = T.parse(data)
    odd = [i for i, n in enumerate(ps.counts[:-1]) if n & 1][0]
    pad_at = ps.offsets[odd] + ps.counts[odd]
    assert data[pad_at] == 0
    for bad in (data + b'\0', data[:-1], data[:pad_at] + b'\1' + data[pad_at + 1:], data[:2] + b'\x2b' + data[3:],
                data[:10] + data[22:34] + data[10:22] + data[34:]):       # trailing byte, cut short, pad not zero, not 42, tags out of order
        with pytest.raises((T.TiffError, zlib.error)):
            T.parse(bad)
    # a padding sample that is not the clamped pixel
    tiles = T.tiles(src, 3, 8)
    spoiled = bytearray(tiles[-1])
    spoiled[-1] ^= 1
    streams = [T.tile_stream(d) for d in tiles[:-1]] + [T.tile_stream(bytes(spoiled))]
    with pytest.raises(T.TiffError, match='padding'):
        T.parse(T.assemble(src.shape[1], src.shape[0], 3, 8, streams))


# ------------------------------------------------------------------ the predictor, the mixed frame
@pytest.mark.parametrize('ch', (3, 4))
def test_predictor_is_word_arithmetic(ch):
    src = TC.byte_order_source()
    tile, = T.tiles(src, ch, 16)
    row = np.frombuffer(tile, '<u2').reshape(64, 64, ch)
    assert row[0, :5, 0].tolist() == [0x00ff, 0x0001, 0xfeff, 0x0001, 0x0000]
    assert tile[:2 * ch] == b'\xff\x00' * ch and tile[2 * ch:4 * ch] == b'\x01\x00' * ch and tile[4 * ch:6 * ch] == b'\xff\xfe' * ch
    assert (row[1:] == row[0]).all()                          # the rows below are the clamped row again
    # (byte arithmetic would store 0x0101, 0xffff, 0x0101: no borrow from, no carry into, the high byte)
    roundtrip(src, ch, 16)


@pytest.mark.parametrize('form', TC.FORMS, ids=TC.form_id)
def test_mixed_frame_has_what_the_device_test_needs(form):
    bits, ch = form
    src = TC.mixed(bits, TC.MIXED_SEED[form])
    assert src.shape[:2] == (70, 2 * T.tile_width(bits) + 3)
    data, ps = roundtrip(src, ch, bits)
    nt, btypes, odd = TC.mixed_properties(data)
    assert nt >= 6 and btypes == {0, 2} and odd
    assert ps.btypes[0] == 0 and ps.counts[0] == T.tile_bytes(ch, bits) + 5 + 6      # the noise tile is stored
    for s in ps.streams:                                      # one final block each: the model's own inflate finds no second one
        raw, blocks = P.zlib_inflate(s)
        assert len(blocks) == 1 and blocks[0]['final'] and all(m[1] == 1 for m in blocks[0]['matches'])


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_tiff_bound', 'fl_tiff_encode', 'fl_output_tiff'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.fl_abi_version() == 1
    for bad in ((None, 8, 8, 1, 3, 16, None, 0, 4096), (None, 8, 8, 1, 3, 16, 1, 0, 4096)):
        assert lib.fl_tiff_encode(*bad) == _lib.FL_E_INVAL          # (a null context: refused before the device is touched)
    assert lib.fl_output_tiff(None, 8, 8, 3, 16, 1, 0, 4096) == _lib.FL_E_INVAL
    assert 'tiff.hip' in open(os.path.join(REPO, 'cuburn_amd', 'csrc', 'Makefile')).read()


def test_bound(built):
    lib = _lib.load()
    for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        for ch in (3, 4):
            for bits in (8, 16):
                assert lib.fl_tiff_bound(w, h, ch, bits) == 0 == T.bound(w, h, ch, bits), (w, h)
    for ch in (0, 1, 2, 5, -3):
        assert lib.fl_tiff_bound(8, 8, ch, 16) == 0 == T.bound(8, 8, ch, 16), ch
    for bits in (0, 1, 4, 12, 24, 32, -8):
        assert lib.fl_tiff_bound(8, 8, 3, bits) == 0 == T.bound(8, 8, 3, bits), bits
    shapes = ((1, 1), (7, 3), (64, 64), (65, 64), (64, 65), (128, 64), (129, 65), (1920, 1080), (65535, 1), (1, 65535), (8000, 65535),
              (20000, 65535), (65535, 65535))
    for w, h in shapes:
        for bits, ch in TC.FORMS:
            assert lib.fl_tiff_bound(w, h, ch, bits) == T.bound(w, h, ch, bits), (w, h, ch, bits)
    assert lib.fl_tiff_bound(1, 1, 3, 8) == 16 + 164 + 24576 + 12 and lib.fl_tiff_bound(1, 1, 4, 16) == 16 + 178 + 32768 + 12
    assert lib.fl_tiff_bound(1920, 1080, 3, 16) == 16 + 164 + 8 * 510 + 510 * (24576 + 12)
    assert lib.fl_tiff_bound(65535, 65535, 3, 8) == 0 and 0 < lib.fl_tiff_bound(20000, 65535, 3, 8) < 2 ** 32      # beyond 2^32 - 1, and below


# ------------------------------------------------------------------ DeviceTIFFOutput against a stand-in library
class StubLib(object):
    def __init__(self, stream=b'II*\0tiles'):
        self.calls, self.stream, self.status = [], stream, 0

    def fl_tiff_bound(self, w, h, channels, bits):
        self.calls.append(('fl_tiff_bound', w, h, channels, bits))
        return T.bound(w, h, channels, bits)

    def fl_output_tiff(self, ctx, w, h, channels, bits, host, dev, cap):
        self.calls.append(('fl_output_tiff', ctx, w, h, channels, bits, host, dev, cap))
        if host:
            rec = np.array([len(self.stream), self.status, T.tile_bytes(channels, bits), 0], '<u4').tobytes() + self.stream
            C.memmove(host, rec, len(rec))
        return 0

    def fl_last_error(self):
        return b''


class StubFB(object):
    ctx = 1234

    def host_buffer(self, shape, dtype):
        self.last = np.zeros(shape, dtype)
        return self.last


@pytest.mark.parametrize('alpha', (False, True))
@pytest.mark.parametrize('bits', (16, 8))
def test_device_output_calls_the_library(monkeypatch, alpha, bits):
    stub = StubLib()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    ch = 4 if alpha else 3
    out = output.DeviceTIFFOutput(alpha=alpha, bits=bits) if bits != 16 else output.DeviceTIFFOutput(alpha=alpha)
    assert isinstance(out, output.DeviceEncodedOutput) and (out.suffix, out.entry, out.bits, out.channels, out.alpha) == ('.tiff', 'fl_output_tiff', bits, ch, alpha)
    dim = render.Framebuffers.calc_dim(64, 48)
    cap = T.bound(64, 48, ch, bits)
    assert out.shape(dim) == (cap,) and np.dtype(out.dtype) == np.uint8
    del stub.calls[:]
    fb = StubFB()
    buf = out.copy(fb, dim)
    assert buf is fb.last and buf.shape == (cap,)
    assert [c for c in stub.calls if c[0] == 'fl_output_tiff'] == [('fl_output_tiff', 1234, 64, 48, ch, bits, buf.ctypes.data, 0, cap)]
    assert set(c for c in stub.calls if c[0] != 'fl_output_tiff') == {('fl_tiff_bound', 64, 48, ch, bits)}
    media, logs = out.encode(buf)
    assert list(media) == ['.tiff'] and media['.tiff'].read() == stub.stream and logs == []
    assert out.encode(None) == ({}, [])
    assert out.copy(fb, dim, dev_out=4096, host=False) is None and stub.calls[-1][6:8] == (None, 4096)
    stub.status = 1                                           # status 1: the needed size is reported
    with pytest.raises(_lib.FlameError, match=str(len(stub.stream))):
        out.encode(out.copy(fb, dim))


def test_device_output_options():
    for bad in (dict(bits=True), dict(bits=12), dict(bits='16'), dict(bits=None), dict(alpha=1), dict(alpha='yes')):
        with pytest.raises(ValueError):
            output.DeviceTIFFOutput(**bad)
    for bad in (dict(quality=90), dict(compression='deflate'), dict(filter='paeth')):
        with pytest.raises(TypeError):
            output.DeviceTIFFOutput(**bad)


# ------------------------------------------------------------------ the profile key and the command line
def test_profile_key():
    gnm, prof = configs.cfg2()

    def out_for(block):
        return output.get_output_for_profile(profile.wrap(dict(prof, output=block), gnm))

    dev = out_for({'type': 'tiff', 'compression': 'deflate'})
    assert type(dev) is output.DeviceTIFFOutput and (dev.alpha, dev.channels, dev.bits, dev.entry, dev.suffix) == (False, 3, 16, 'fl_output_tiff', '.tiff')
    dev = out_for({'type': 'tiff', 'compression': 'deflate', 'alpha': True})
    assert type(dev) is output.DeviceTIFFOutput and (dev.alpha, dev.channels, dev.bits) == (True, 4, 16)
    dev = out_for({'type': 'tiff', 'compression': 'deflate', 'alpha': False})
    assert type(dev) is output.DeviceTIFFOutput and dev.alpha is False
    for block in ({'type': 'tiff'}, {'type': 'tiff', 'compression': 'none'}, {'type': 'tiff', 'alpha': True},
                  {'type': 'tiff', 'compression': 'none', 'alpha': True}):                  # the host writer, exactly as before
        host = out_for(block)
        assert type(host) is output.TiffOutput and host.alpha is bool(block.get('alpha')) and host.fmt == 1 and host.suffix == '.tiff'
    img = (np.arange(2 * 3 * 4, dtype=np.uint16) * 2731).reshape(2, 3, 4)
    for alpha in (False, True):
        with_key = out_for({'type': 'tiff', 'compression': 'none', 'alpha': alpha}).encode(img)[0]['.tiff'].read()
        assert with_key == out_for({'type': 'tiff', 'alpha': alpha}).encode(img)[0]['.tiff'].read() == output._tiff_bytes(img if alpha else img[:, :, :3])
    # any other value, and the key on any other type: refused by name
    for block in ({'type': 'tiff', 'compression': 'lzw'}, {'type': 'tiff', 'compression': True}, {'type': 'tiff', 'compression': 'Deflate'},
                  {'type': 'tiff', 'compression': 8}, {'type': 'tiff', 'compression': ''}, {'type': 'tiff', 'compression': ['deflate']},
                  {'type': 'png', 'compression': 'deflate'}, {'type': 'png', 'encoder': 'device', 'compression': 'deflate'},
                  {'type': 'jpeg', 'compression': 'none'}, {'type': 'jpeg', 'device': True, 'compression': 'deflate'}, {'compression': 'deflate'},
                  {'type': 'raw16', 'compression': 'deflate'}, {'type': 'raw', 'compression': 'none'}, {'type': 'mjpeg', 'compression': 'deflate'},
                  {'type': 'x264', 'compression': 'deflate'}):
        with pytest.raises(ValueError, match=r'output\.compression'):
            out_for(block)
    # nothing but alpha beside it
    with pytest.raises(ValueError, match=r'output\.compression.*quality'):
        out_for({'type': 'tiff', 'compression': 'deflate', 'quality': 90})
    with pytest.raises(ValueError, match=r'output\.alpha'):
        out_for({'type': 'tiff', 'compression': 'deflate', 'alpha': 1})
    # the fenced spellings stay refused, with the messages they have
    with pytest.raises(ValueError, match=r'output\.encoder: selects the device PNG encoder \("device": true is the JPEG switch\), not "tiff"'):
        out_for({'type': 'tiff', 'encoder': 'device'})
    with pytest.raises(ValueError, match=r'output\.bits: only the device PNG encoder takes it: set "encoder": "device" on a png output'):
        out_for({'type': 'tiff', 'bits': 16})
    with pytest.raises(ValueError, match=r'output\.device: only jpeg is encoded on the device, not "tiff"'):
        out_for({'type': 'tiff', 'device': True})
    for block in ({'type': 'tiff', 'compression': 'deflate', 'encoder': 'device'}, {'type': 'tiff', 'compression': 'deflate', 'bits': 16},
                  {'type': 'tiff', 'compression': 'deflate', 'device': True}, {'type': 'tiff', 'compression': 'deflate', 'bits': 8}):
        with pytest.raises(ValueError, match=r'output\.(encoder|bits|device)'):
            out_for(block)
    assert output.get_suffix_for_profile(profile.wrap(dict(prof, output={'type': 'tiff', 'compression': 'deflate'}), gnm)) == '.tiff'


def test_command_line_option():
    parser = profile.add_args(argparse.ArgumentParser())

    def out_of(*argv):
        return profile.get_from_args(parser.parse_args(list(argv)))[1].get('output')

    assert out_of('--codec', 'tiff', '--tiff-compression', 'deflate') == {'type': 'tiff', 'compression': 'deflate'}
    assert out_of('--tiff-compression', 'none', '--codec', 'tiff') == {'type': 'tiff', 'compression': 'none'}
    assert out_of('--codec', 'tiff') == {'type': 'tiff'}
    assert out_of('--tiff-compression', 'deflate') == {'compression': 'deflate'}               # (no tiff: the output factory refuses it)
    assert out_of('--codec', 'tiff', '--device-encode') == {'type': 'tiff', 'device': True}    # still the JPEG switch: refused below
    for argv in (('--tiff-compression', 'lzw'), ('--tiff-compression',), ('--tiff-compression', 'Deflate')):
        with pytest.raises(SystemExit):
            parser.parse_args(list(argv))
    text = parser.format_help()
    assert text.index('--bits') < text.index('--png-filter') < text.index('--tiff-compression') < text.index('--suffix')
    gnm, _ = configs.cfg2()

    def out_for(*argv):
        return output.get_output_for_profile(profile.wrap(profile.get_from_args(parser.parse_args(list(argv)))[1], gnm))

    dev = out_for('--codec', 'tiff', '--tiff-compression', 'deflate')
    assert type(dev) is output.DeviceTIFFOutput and (dev.bits, dev.alpha) == (16, False)
    assert type(out_for('--codec', 'tiff', '--tiff-compression', 'none')) is output.TiffOutput
    assert type(out_for('--codec', 'tiff')) is output.TiffOutput
    with pytest.raises(ValueError, match=r'output\.device: only jpeg is encoded on the device, not "tiff"'):
        out_for('--codec', 'tiff', '--device-encode')
    with pytest.raises(ValueError, match=r'output\.bits'):
        out_for('--codec', 'tiff', '--bits', '16')
    with pytest.raises(ValueError, match=r'output\.compression'):
        out_for('--codec', 'png', '--tiff-compression', 'deflate')
    with pytest.raises(ValueError, match=r'output\.compression'):
        out_for('--tiff-compression', 'deflate')               # the default type is jpeg
