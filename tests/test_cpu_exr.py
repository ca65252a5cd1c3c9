"""
CPU tests of the device OpenEXR encoder's format (no GPU).  No OpenEXR reader is installed here, so the model of tests/exr_model.py
is held to its own reader — written from the file layout, sharing nothing with the writer — on the frames tests/test_gpu_exr.py
gives the device; its half conversion to numpy's float16; its predictor to a byte-at-a-time transcription; its bound to a file of
noise; the mixed frame is shown to hold both data forms before any device sees it; and the C ABI's refusals that need no device,
DeviceEXROutput against a stand-in library, the profile keys and the command line are driven.
"""
import argparse
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, output, profile, render
import exr_cases as XC
import exr_model as X


def roundtrip(src, ch, px):
    """Model encode -> the model's reader; returns (file, parse)."""
    data = X.encode(src, ch, px)
    ps = X.parse(data)
    h, w, _ = src.shape
    assert (ps.w, ps.h, ps.channels, ps.pixel) == (w, h, ch, px)
    assert (ps.tw, ps.th) == (64, X.tile_rows(px)) and ps.header_bytes == X.header_bytes(w, h, ch, px)
    assert np.array_equal(ps.samples, X.samples_of(src, ch, px))
    assert 16 + len(data) <= X.bound(w, h, ch, px)
    assert X.encode(src, ch, px) == data
    return data, ps


# ------------------------------------------------------------------ the model against its own reader
@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_reader_returns_the_samples(form):
    px, ch = form
    for w, h in XC.small_shapes() + XC.edge_shapes(px) + ((130, 2 * X.tile_rows(px) + 3),):
        for src in (XC.noise(w, h, px, 3 * w + h), XC.ramps(w, h, w + h)):
            data, ps = roundtrip(src, ch, px)
            th, nx, ny = X.geometry(w, h, px)
            assert ps.nt == nx * ny == len(ps.datas)
            for raw, body, form_ in zip(X.raw_tiles(src, ch, px), ps.datas, ps.forms):
                if form_ == 'zip':
                    assert len(body) < len(raw) and zlib.decompress(body) == X.preprocess(raw)
                    assert body[-4:] == struct.pack('>I', zlib.adler32(X.preprocess(raw)))
                else:
                    assert body == raw
    src = XC.mixed(px, XC.MIXED_SEED[form])
    roundtrip(src, ch, px)


def test_header_is_what_the_contract_says():
    assert X.header_bytes(7, 5, 3, X.HALF) == 341 == X.header_bytes(65535, 1, 3, X.FLOAT) and X.header_bytes(7, 5, 4, X.FLOAT) == 359
    hdr = X.header(7, 5, 4, X.HALF)
    assert hdr[:8] == bytes([0x76, 0x2f, 0x31, 0x01, 0x02, 0x02, 0x00, 0x00])
    assert hdr[8:8 + 9 + 7 + 4] == b'channels\0chlist\0' + struct.pack('<i', 18 * 4 + 1)
    assert hdr[28:28 + 18] == b'A\0' + struct.pack('<i', 1) + b'\0\0\0\0' + struct.pack('<ii', 1, 1)
    ps = X.parse(X.encode(XC.ramps(7, 5, 0), 4, X.HALF))
    assert ps.order == [b'channels', b'compression', b'dataWindow', b'displayWindow', b'lineOrder', b'pixelAspectRatio',
                        b'screenWindowCenter', b'screenWindowWidth', b'tiles']
    assert ps.names == [b'A', b'B', b'G', b'R'] and ps.attrs[b'tiles'][1] == struct.pack('<IIB', 64, 64, 0)
    assert X.parse(X.encode(XC.ramps(7, 5, 0), 3, X.FLOAT)).attrs[b'tiles'][1] == struct.pack('<IIB', 64, 32, 0)


def test_tile_layout_is_planar_and_cropped():
    """A 65 x 2 frame, R = 1, G = 2, B = 3, A = 4 (+ x / 256): the second tile is one pixel wide; rows hold A, B, G, R runs."""
    src = np.empty((2, 65, 4), np.float32)
    src[:] = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    src[:, :, :] += (np.arange(65, dtype=np.float32) / 256.0)[None, :, None]
    first, second = X.raw_tiles(src, 4, X.FLOAT)
    assert len(first) == 2 * 64 * 16 and len(second) == 2 * 16
    row = np.frombuffer(first, '<f4').reshape(2, 4, 64)
    assert row[0, :, 0].tolist() == [4.0, 3.0, 2.0, 1.0] and row[1, 3, 63] == np.float32(1.0 + 63 / 256.0)
    assert np.frombuffer(second, '<f4').tolist() == [4.25, 3.25, 2.25, 1.25] * 2
    first3, _ = X.raw_tiles(src, 3, X.HALF)
    assert np.frombuffer(first3, '<f2').reshape(2, 3, 64)[0, :, 0].tolist() == [3.0, 2.0, 1.0]
    ps = X.parse(X.encode(src, 4, X.FLOAT))
    assert ps.nt == 2 and struct.unpack('<5i', X.encode(src, 4, X.FLOAT)[ps.offsets[1]:ps.offsets[1] + 20])[:4] == (1, 0, 0, 0)


def test_reader_refuses_what_breaks_the_layout():
    src = XC.mixed(X.HALF, XC.MIXED_SEED[(X.HALF, 3)])
    data = X.encode(src, 3, X.HALF)
    ps = X.parse(data)
    o1 = ps.offsets[1]
    H = ps.header_bytes
    bads = (data + b'\0', data[:-1], b'\x77' + data[1:], data[:4] + b'\x02\x00' + data[6:],
            data[:o1] + struct.pack('<i', 2) + data[o1 + 4:],                                     # a chunk with another tile's coordinates
            data[:H + 8] + struct.pack('<Q', o1 + 1) + data[H + 16:],                             # an offset that points elsewhere
            data[:o1 + 16] + struct.pack('<i', ps.sizes[1] - 1) + data[o1 + 20:],                 # a size that cuts the stream
            data.replace(b'compression\0compression\0\x01\0\0\0\x03', b'compression\0compression\0\x01\0\0\0\x02'))
    for bad in bads:
        with pytest.raises((X.ExrError, zlib.error, struct.error)):
            X.parse(bad)


# ------------------------------------------------------------------ float to half
def reference_half(a):
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(a, np.float32).astype(np.float16)


def test_to_half_is_numpy_where_numpy_is_finite():
    a = XC.half_atlas()
    assert a.size == 256 * 1024
    ref, got = reference_half(a), X.to_half(a)
    fin = np.isfinite(ref)
    assert fin.sum() > 250000 and np.array_equal(got[fin], ref.view(np.uint16)[fin])
    # every half value comes back as itself
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    wide = halves.view(np.float16).astype(np.float32)
    back = X.to_half(wide)
    finite = (halves & 0x7c00) != 0x7c00
    assert np.array_equal(back[finite], halves[finite])
    # out of range, the infinities and NaN
    over = np.isinf(ref) & ~np.isnan(a)
    assert over.sum() > 10 and np.array_equal(got[over], np.where(a[over] > 0, 0x7bff, 0xfbff))
    assert (got[np.isnan(a)] == 0).all() and np.isnan(a).sum() > 2000


def test_to_half_at_the_edges():
    def h(v):
        return int(X.to_half(np.array([v], np.float32))[0])
    assert h(65504.0) == 0x7bff and h(65519.996) == 0x7bff and h(65520.0) == 0x7bff and h(np.inf) == 0x7bff and h(3e38) == 0x7bff
    assert h(-65504.0) == 0xfbff and h(-65520.0) == 0xfbff and h(-np.inf) == 0xfbff
    assert reference_half(65519.996).view(np.uint16) == 0x7bff and np.isinf(reference_half(65520.0))      # numpy rounds the tie up, out of range
    assert h(np.nan) == 0 and h(-np.nan) == 0 and h(0.0) == 0 and h(-0.0) == 0x8000
    assert h(2.0 ** -24) == 1 and h(2.0 ** -25) == 0 and h(np.nextafter(np.float32(2.0 ** -25), np.float32(1))) == 1      # the tie goes to even
    assert h(1.5 * 2.0 ** -24) == 2 and h(2.5 * 2.0 ** -24) == 2 and h(-(2.0 ** -25)) == 0x8000
    assert h(2.0 ** -14) == 0x0400 and h(np.nextafter(np.float32(2.0 ** -14), np.float32(0))) == 0x0400 and h(1e-45) == 0
    assert h(1.0) == 0x3c00 and h(1.0 + 2.0 ** -11) == 0x3c00 and h(1.0 + 3 * 2.0 ** -11) == 0x3c02 and h(2.0 - 2.0 ** -12) == 0x4000


def test_half_denormal_range_and_below():
    k = np.arange(0, 1 << 14, dtype=np.float64)
    for scale in (2.0 ** -26, 2.0 ** -27, 3 * 2.0 ** -28):       # quarters and eighths of the smallest half denormal, up to 2^-12
        a = (k * scale).astype(np.float32)
        assert np.array_equal(X.to_half(a), reference_half(a).view(np.uint16))
        assert np.array_equal(X.to_half(-a), reference_half(-a).view(np.uint16))


# ------------------------------------------------------------------ the predictor
def slow_preprocess(raw):
    n = len(raw)
    t = bytearray(n)
    a, b = 0, (n + 1) // 2
    for i in range(0, n, 2):                                  # (the reference library's loop: one byte to each half in turn)
        t[a] = raw[i]; a += 1
        t[b] = raw[i + 1]; b += 1
    d = bytearray(n)
    d[0] = t[0]
    p = t[0]
    for i in range(1, n):
        d[i] = (t[i] - p + 128 + 256) % 256
        p = t[i]
    return bytes(d)


@pytest.mark.parametrize('n', (6, 8, 24576, 32768))
def test_preprocess_byte_by_byte(n):
    raw = np.random.RandomState(n).randint(0, 256, n).astype(np.uint8).tobytes()
    assert X.preprocess(raw) == slow_preprocess(raw)
    ramp = bytes((i * 7 // 3) & 255 for i in range(n))
    assert X.preprocess(ramp) == slow_preprocess(ramp)
    assert X.preprocess(b'\0\xff' * (n // 2)) == b'\0' + b'\x80' * (n // 2 - 1) + b'\x7f' + b'\x80' * (n // 2 - 1)


# ------------------------------------------------------------------ the bound, the mixed frame
@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_bound_is_a_file_of_noise(form):
    px, ch = form
    for w, h in ((1, 1), (65, X.tile_rows(px) + 1), (130, 3)):
        data = X.encode(XC.noise(w, h, px, w * h), ch, px)
        assert set(X.parse(data).forms) == {'raw'}
        assert 16 + len(data) == X.bound(w, h, ch, px)
    th, nx, ny = X.geometry(1920, 1080, px)
    assert X.bound(1920, 1080, ch, px) == 16 + (341 if ch == 3 else 359) + 28 * nx * ny + 1920 * 1080 * ch * X.sample_bytes(px)


@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_mixed_frame_has_what_the_device_test_needs(form):
    px, ch = form
    src = XC.mixed(px, XC.MIXED_SEED[form])
    assert src.shape[:2] == (70, 131)
    data, ps = roundtrip(src, ch, px)
    nt, forms, corner = XC.mixed_properties(data)
    assert nt == (6 if px == X.HALF else 9) and forms[0] == 'raw' and set(forms[1:]) == {'zip'}
    assert ps.sizes[0] == X.tile_bytes(ch) and ps.sizes[1] < 100           # noise: a full tile, raw; zeros: a few bytes
    assert len(X.raw_tiles(src, ch, px)[-1]) == 3 * 6 * ch * X.sample_bytes(px) and corner < 3 * 6 * ch * X.sample_bytes(px)
    s = X.samples_of(src, ch, px)
    assert not s[:X.tile_rows(px), 64:128].any() and s[:, :, :3].max() > (0x3c00 if px == X.HALF else 0x3f800000)      # above 1.0


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_exr_bound', 'fl_exr_encode', 'fl_output_exr'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert re.search(r'FL_EXR_HALF\s*=\s*1\s*,\s*FL_EXR_FLOAT\s*=\s*2', code) and _lib.EXR_PIXELS == {'half': 1, 'float': 2}
    assert lib.fl_abi_version() == 1
    for bad in ((None, 8, 8, 1, 8, 3, 1, None, 0, 4096), (None, 8, 8, 1, 8, 3, 2, 1, 0, 4096)):
        assert lib.fl_exr_encode(*bad) == _lib.FL_E_INVAL           # (a null context: refused before the device is touched)
    assert lib.fl_output_exr(None, 8, 8, 3, 1, 1, 0, 4096) == _lib.FL_E_INVAL
    assert 'exr.hip' in open(os.path.join(REPO, 'cuburn_amd', 'csrc', 'Makefile')).read()


def test_bound(built):
    lib = _lib.load()
    for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        for px, ch in XC.FORMS:
            assert lib.fl_exr_bound(w, h, ch, px) == 0 == X.bound(w, h, ch, px), (w, h)
    for ch in (0, 1, 2, 5, -3):
        assert lib.fl_exr_bound(8, 8, ch, 1) == 0 == X.bound(8, 8, ch, 1), ch
    for px in (0, 3, 16, 32, -1):
        assert lib.fl_exr_bound(8, 8, 3, px) == 0 == X.bound(8, 8, 3, px), px
    shapes = ((1, 1), (7, 3), (64, 64), (65, 64), (64, 65), (64, 32), (64, 33), (131, 70), (1920, 1080), (65535, 1), (1, 65535), (8000, 65535),
              (20000, 65535), (65535, 65535))
    for w, h in shapes:
        for px, ch in XC.FORMS:
            assert lib.fl_exr_bound(w, h, ch, px) == X.bound(w, h, ch, px), (w, h, ch, px)
    assert lib.fl_exr_bound(1, 1, 3, 1) == 16 + 341 + 28 + 6 and lib.fl_exr_bound(1, 1, 4, 2) == 16 + 359 + 28 + 16
    assert lib.fl_exr_bound(1920, 1080, 3, 1) == 16 + 341 + 28 * 510 + 1920 * 1080 * 6
    assert lib.fl_exr_bound(1920, 1080, 4, 2) == 16 + 359 + 28 * 30 * 34 + 1920 * 1080 * 16
    assert lib.fl_exr_bound(65535, 65535, 3, 1) == 0 and 0 < lib.fl_exr_bound(10000, 65535, 3, 1) < 2 ** 32      # beyond 2^32 - 1, and below


# ------------------------------------------------------------------ DeviceEXROutput against a stand-in library
class StubLib(object):
    def __init__(self, stream=X.MAGIC + b'tiles'):
        self.calls, self.stream, self.status = [], stream, 0

    def fl_exr_bound(self, w, h, channels, pixel):
        self.calls.append(('fl_exr_bound', w, h, channels, pixel))
        return X.bound(w, h, channels, pixel)

    def fl_output_exr(self, ctx, w, h, channels, pixel, host, dev, cap):
        self.calls.append(('fl_output_exr', ctx, w, h, channels, pixel, host, dev, cap))
        if host:
            rec = np.array([len(self.stream), self.status, X.tile_bytes(channels), 0], '<u4').tobytes() + self.stream
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
@pytest.mark.parametrize('pixel', ('half', 'float'))
def test_device_output_calls_the_library(monkeypatch, alpha, pixel):
    stub = StubLib()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    ch, px = 4 if alpha else 3, _lib.EXR_PIXELS[pixel]
    out = output.DeviceEXROutput(alpha=alpha, pixel=pixel) if pixel != 'half' else output.DeviceEXROutput(alpha=alpha)
    assert isinstance(out, output.DeviceEncodedOutput) and (out.suffix, out.entry, out.pixel, out.channels, out.alpha) == ('.exr', 'fl_output_exr', pixel, ch, alpha)
    dim = render.Framebuffers.calc_dim(64, 48)
    cap = X.bound(64, 48, ch, px)
    assert out.shape(dim) == (cap,) and np.dtype(out.dtype) == np.uint8
    del stub.calls[:]
    fb = StubFB()
    buf = out.copy(fb, dim)
    assert buf is fb.last and buf.shape == (cap,)
    assert [c for c in stub.calls if c[0] == 'fl_output_exr'] == [('fl_output_exr', 1234, 64, 48, ch, px, buf.ctypes.data, 0, cap)]
    assert set(c for c in stub.calls if c[0] != 'fl_output_exr') == {('fl_exr_bound', 64, 48, ch, px)}
    media, logs = out.encode(buf)
    assert list(media) == ['.exr'] and media['.exr'].read() == stub.stream and logs == []
    assert out.encode(None) == ({}, [])
    assert out.copy(fb, dim, dev_out=4096, host=False) is None and stub.calls[-1][6:8] == (None, 4096)
    stub.status = 1                                           # status 1: the needed size is reported
    with pytest.raises(_lib.FlameError, match=str(len(stub.stream))):
        out.encode(out.copy(fb, dim))


def test_device_output_options():
    for bad in (dict(pixel=True), dict(pixel=16), dict(pixel='Half'), dict(pixel=None), dict(pixel='double'), dict(alpha=1), dict(alpha='yes')):
        with pytest.raises(ValueError):
            output.DeviceEXROutput(**bad)
    for bad in (dict(quality=90), dict(bits=16), dict(compression='zip')):
        with pytest.raises(TypeError):
            output.DeviceEXROutput(**bad)


# ------------------------------------------------------------------ the profile keys and the command line
def test_profile_keys():
    gnm, prof = configs.cfg2()

    def out_for(block):
        return output.get_output_for_profile(profile.wrap(dict(prof, output=block), gnm))

    dev = out_for({'type': 'exr'})
    assert type(dev) is output.DeviceEXROutput and (dev.alpha, dev.channels, dev.pixel, dev.entry, dev.suffix) == (False, 3, 'half', 'fl_output_exr', '.exr')
    dev = out_for({'type': 'exr', 'pixel': 'float', 'alpha': True})
    assert type(dev) is output.DeviceEXROutput and (dev.alpha, dev.channels, dev.pixel) == (True, 4, 'float')
    dev = out_for({'type': 'exr', 'pixel': 'half', 'alpha': False})
    assert (dev.alpha, dev.channels, dev.pixel) == (False, 3, 'half')
    # any other key is refused by name
    for key, value in (('quality', 90), ('bits', 16), ('filter', 'paeth'), ('compression', 'deflate'), ('compression', 'none'), ('device', True),
                       ('device', False), ('encoder', 'device'), ('optimize', True), ('sampling', '420'), ('crf', 10)):
        with pytest.raises(ValueError, match=key):
            out_for({'type': 'exr', key: value})
        with pytest.raises(ValueError, match=key):
            out_for({'type': 'exr', 'pixel': 'float', 'alpha': True, key: value})
    for block in ({'type': 'exr', 'pixel': 'double'}, {'type': 'exr', 'pixel': 16}, {'type': 'exr', 'pixel': True}, {'type': 'exr', 'pixel': 'Float'},
                  {'type': 'exr', 'pixel': ''}, {'type': 'exr', 'pixel': ['half']}):
        with pytest.raises(ValueError, match=r'output\.pixel'):
            out_for(block)
    with pytest.raises(ValueError, match=r'output\.alpha'):
        out_for({'type': 'exr', 'alpha': 1})
    # pixel on any other type
    for block in ({'type': 'tiff', 'pixel': 'half'}, {'type': 'tiff', 'compression': 'deflate', 'pixel': 'half'}, {'type': 'png', 'pixel': 'float'},
                  {'type': 'png', 'encoder': 'device', 'pixel': 'half'}, {'type': 'jpeg', 'pixel': 'half'}, {'type': 'jpeg', 'device': True, 'pixel': 'half'},
                  {'pixel': 'half'}, {'type': 'raw', 'pixel': 'float'}, {'type': 'raw16', 'pixel': 'half'}, {'type': 'mjpeg', 'pixel': 'half'},
                  {'type': 'x264', 'pixel': 'half'}):
        with pytest.raises(ValueError, match=r'output\.pixel'):
            out_for(block)
    assert output.get_suffix_for_profile(profile.wrap(dict(prof, output={'type': 'exr', 'pixel': 'float'}), gnm)) == '.exr'
    assert output.get_suffix('exr') == '.exr'
    # nothing else moved
    assert type(out_for({'type': 'tiff'})) is output.TiffOutput and type(out_for({'type': 'tiff', 'compression': 'deflate'})) is output.DeviceTIFFOutput
    assert type(out_for({'type': 'png', 'encoder': 'device'})) is output.DevicePNGOutput and type(out_for({'type': 'jpeg', 'device': True})) is output.DeviceJPEGOutput
    assert not hasattr(output, 'EXROutput')                   # no host writer behind it


def test_command_line_options():
    parser = profile.add_args(argparse.ArgumentParser())

    def out_of(*argv):
        return profile.get_from_args(parser.parse_args(list(argv)))[1].get('output')

    assert out_of('--codec', 'exr') == {'type': 'exr'}
    assert out_of('--codec', 'exr', '--exr-pixel', 'float') == {'type': 'exr', 'pixel': 'float'}
    assert out_of('--exr-pixel', 'half', '--codec', 'exr') == {'type': 'exr', 'pixel': 'half'}
    assert out_of('--exr-pixel', 'half') == {'pixel': 'half'}                                  # (no exr: the output factory refuses it)
    for argv in (('--exr-pixel', 'double'), ('--exr-pixel',), ('--exr-pixel', 'Half'), ('--codec', 'openexr')):
        with pytest.raises(SystemExit):
            parser.parse_args(list(argv))
    text = parser.format_help()
    assert text.index('--tiff-compression') < text.index('--exr-pixel') < text.index('--suffix')
    gnm, _ = configs.cfg2()

    def out_for(*argv):
        return output.get_output_for_profile(profile.wrap(profile.get_from_args(parser.parse_args(list(argv)))[1], gnm))

    dev = out_for('--codec', 'exr')
    assert type(dev) is output.DeviceEXROutput and (dev.pixel, dev.alpha) == ('half', False)
    assert out_for('--codec', 'exr', '--exr-pixel', 'float').pixel == 'float'
    with pytest.raises(ValueError, match=r'output\.pixel'):
        out_for('--exr-pixel', 'half')                         # the default type is jpeg
    with pytest.raises(ValueError, match=r'output\.pixel'):
        out_for('--codec', 'tiff', '--exr-pixel', 'half')
    for extra in (('--device-encode',), ('--quality', '90'), ('--bits', '16'), ('--tiff-compression', 'deflate'), ('--png-filter', 'adaptive'), ('--optimize',)):
        with pytest.raises(ValueError, match='OpenEXR'):
            out_for('--codec', 'exr', *extra)
