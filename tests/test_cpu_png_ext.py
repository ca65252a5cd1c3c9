"""
CPU tests of the device PNG encoder's extended format (no GPU): 16-bit samples and a filter type per row.  The model of
tests/png_ext_model.py is held to zlib and Pillow on every frame tests/test_gpu_png_ext.py gives the device, the ten-band image
is shown to reach all five filter types and the tie before any device sees it, and the C ABI's three new entry points,
DevicePNGOutput, the profile keys and the command line are driven against a stand-in library.
"""
import argparse
import ctypes as C
import io
import os
import re
import zlib

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, output, profile, render
import png_cases as PC
import png_ext_cases as XC
import png_ext_model as X
import png_model as P

SEG = XC.MODEL_SEG


def roundtrip(img, ch, bits, flags, seg=SEG):
    """Model encode -> model parse, zlib and Pillow; returns the parse."""
    src = XC.source(img, ch, bits)
    data = X.encode(src, ch, bits, flags, seg)
    ps = X.parse(data, seg)
    assert (ps.w, ps.h, ps.channels, ps.bits) == (img.shape[1], img.shape[0], ch, bits)
    assert np.array_equal(ps.bytes, img) and np.array_equal(ps.pixels, src[:, :, :ch]) and ps.pixels.dtype == src.dtype
    filtered, types = X.filter_stream(img, flags)
    assert zlib.decompress(ps.zstream) == ps.filtered == filtered and ps.filters == types      # an independent inflate
    assert 16 + len(data) <= X.bound(ps.w, ps.h, ch, bits, seg)
    PIL_Image = pytest.importorskip('PIL.Image')                 # (without Pillow the test shows as skipped, not as passed)
    im = PIL_Image.open(io.BytesIO(data))
    assert im.size == (ps.w, ps.h) and im.mode == ('RGB' if ch == 3 else 'RGBA')
    got = np.asarray(im)
    assert np.array_equal(got, src[:, :, :ch] if bits == 8 else (src[:, :, :ch] >> 8).astype(np.uint8))      # Pillow keeps the high bytes of 16-bit truecolour
    return ps


# ------------------------------------------------------------------ the cost, the choice and the ten-band image
def test_cost_and_choice_rule():
    img = np.array([[[10, 250, 128]], [[12, 250, 0]]], np.uint8)      # 2 x 1 x 3
    cost = X.row_costs(img)
    assert cost[0].tolist() == [10 + 6 + 128, 12 + 6 + 0]             # None: min(r, 256 - r) of the bytes themselves
    assert cost[2].tolist() == [10 + 6 + 128, 2 + 0 + 128]            # Up: 12 - 10, 250 - 250, 0 - 128
    assert cost[1].tolist() == cost[0].tolist()                       # Sub with w = 1: a is 0
    assert cost[3, 1] == 7 + 125 + 64 and cost[4, 1] == cost[2, 1]    # Average: x - (b >> 1); Paeth with a = c = 0 predicts b
    assert cost[:, 0].tolist() == [144] * 5
    assert X.choose(img) == [0, 0]                                    # row 0: a five-way tie; row 1: None and Sub tie at 18
    assert X.choose(np.zeros((3, 4, 6), np.uint8)) == [0, 0, 0]


@pytest.mark.parametrize('w,bpp', [(40, 3), (40, 4), (37, 6), (37, 8), (5, 3), (4, 8), (33, 3), (33, 4), (33, 6), (33, 8), (5, 4), (5, 6),
                                   (5, 8), (37, 3), (37, 4), (40, 6), (40, 8), (700, 8)])
def test_ten_band_reaches_every_type(w, bpp):
    img = XC.ten_band(w, bpp)
    assert img.shape == (10, w, bpp)
    types, cost = X.choose(img), X.row_costs(img)
    assert set(types) == {0, 1, 2, 3, 4}, types
    assert len(set(cost[:, XC.ROW_TIE].tolist())) == 1 and types[XC.ROW_TIE] == 0      # the tie goes to the lowest type
    assert [types[r] for r in (XC.ROW_UP, XC.ROW_SUB, XC.ROW_AVERAGE, XC.ROW_PAETH)] == [2, 1, 3, 4]
    assert types[XC.ROW_NONE] == 0
    stream, got = X.filter_stream(img, X.ADAPTIVE)
    assert got == types and [stream[y * (1 + w * bpp)] for y in range(10)] == types
    back, filters = P.unfilter(stream, w, 10, bpp)
    assert np.array_equal(back, img) and filters == types


# ------------------------------------------------------------------ the model on every frame the device is given
@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_model_round_trip_small_frames(form):
    bits, ch, flags = form
    bpp = X.bpp_of(ch, bits)
    for w, h in ((1, 1), (1, 7), (7, 1)):
        roundtrip(XC.noise(w, h, bpp, 7 * w + h), ch, bits, flags)
    for w in XC.TEN_BAND_W:
        ps = roundtrip(XC.ten_band(w, bpp), ch, bits, flags)
        assert set(ps.filters) == ({0, 1, 2, 3, 4} if flags else {4})


def test_model_round_trip_wide_and_byte_order():
    ps = roundtrip(XC.ten_band(700, 8), 4, 16, X.ADAPTIVE)
    assert set(ps.filters) == {0, 1, 2, 3, 4}
    src = XC.byte_order_source()
    for ch in (3, 4):
        for flags in (0, X.ADAPTIVE):
            img = X.byte_image(src, ch, 16)
            assert img[0, 0].tolist()[:6] == [0x00, 0xff, 0xff, 0x00, 0x01, 0x00]      # most significant byte first
            roundtrip(img, ch, 16, flags)


def test_model_round_trip_widest_row():
    ps = roundtrip(XC.noise(65535, 2, 8, 12), 4, 16, X.ADAPTIVE)
    assert len(ps.filtered) == 2 * (1 + 65535 * 8) and all(b['type'] == 0 for b in ps.blocks)      # noise: every segment stored


@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_model_round_trip_segments(form):
    bits, ch, flags = form
    bpp = X.bpp_of(ch, bits)
    w, h = XC.soft_shape(SEG, bpp)
    ps = roundtrip(XC.soft(w, h, ch, bits, 3), ch, bits, flags)
    assert len(ps.idat) >= 3 and any(b['type'] == 2 for b in ps.blocks)


def test_default_form_is_the_existing_format():
    for name in ('7x3_rgb', 'smooth_256x96', '1x1_rgba'):
        rgba, ch, _ = PC.case(name, SEG)
        assert X.encode(rgba, ch, 8, 0, SEG) == P.encode(rgba[:, :, :ch], SEG)
    assert X.bound(1920, 1080, 3, 8, SEG) == PC.bound(1920, 1080, 3, SEG)


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_png_bound_f', 'fl_png_encode_f', 'fl_output_png_f'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert re.search(r'\bFL_PNG_ADAPTIVE\s*=\s*1\b', code) and _lib.PNG_ADAPTIVE == 1 == X.ADAPTIVE
    assert _lib.PNG_FILTERS == {'paeth': 0, 'adaptive': 1}
    assert int(re.search(r'#define\s+FL_PNG_HEADER_BYTES\s+(\d+)', code).group(1)) == 33 and lib.fl_abi_version() == 1
    for bad in ((None, 8, 8, 1, 3, 16, 0, None, 0, 4096), (None, 8, 8, 1, 3, 16, 0, 1, 0, 4096)):
        assert lib.fl_png_encode_f(*bad) == _lib.FL_E_INVAL          # (a null context: refused before the device is touched)


def test_bound_f(built):
    lib = _lib.load()
    big = ((16000, 65535, 4), (8000, 65535, 3), (1920, 1080, 3))
    seg = [s for s in range(8192, 32769, 16) if all(PC.bound(w, h, ch, s) == lib.fl_png_bound(w, h, ch) for w, h, ch in big)]
    assert len(seg) == 1                                      # the library's segment length, from the 8-bit bound of large frames
    seg = seg[0]
    for w, h, ch in ((0, 8, 3), (8, 0, 3), (65536, 8, 3), (8, 65536, 4), (8, 8, 2), (8, 8, 5), (8, 8, 0), (65535, 65535, 3)):
        for bits in (8, 16):
            for flags in (0, 1):
                assert lib.fl_png_bound(w, h, ch) == 0 and lib.fl_png_bound_f(w, h, ch, bits, flags) == 0, (w, h, ch)
    for bits in (0, 1, 4, 12, 24, 32, -8):
        assert lib.fl_png_bound_f(8, 8, 3, bits, 0) == 0, bits
    for flags in (2, 3, 4, 0x80000000, 0x101):
        assert lib.fl_png_bound_f(8, 8, 3, 8, flags) == 0 and lib.fl_png_bound_f(8, 8, 3, 16, flags) == 0, flags
    shapes = ((1, 1, 3), (1, 1, 4), (7, 3, 3), (1920, 1080, 3), (1920, 1080, 4), (8000, 65535, 4), (9000, 65535, 4), (65535, 2, 4))
    for w, h, ch in shapes:
        for flags in (0, 1):
            assert lib.fl_png_bound_f(w, h, ch, 8, flags) == lib.fl_png_bound(w, h, ch) != 0
    for w, h, ch in shapes:
        want = X.bound(w, h, ch, 16, seg)
        for flags in (0, 1):
            assert lib.fl_png_bound_f(w, h, ch, 16, flags) == (want if want < 2 ** 32 else 0), (w, h, ch)
    assert lib.fl_png_bound_f(9000, 65535, 4, 16, 0) == 0 != lib.fl_png_bound(9000, 65535, 4)      # 4.7e9 bytes at 16 bits, 2.4e9 at 8
    assert lib.fl_png_bound_f(1, 1, 4, 16, 1) == 16 + 33 + 2 + 9 + 17 + 4 + 12


# ------------------------------------------------------------------ DevicePNGOutput and the plumbing, against a stand-in library
class StubLib(object):
    """fl_png_bound / fl_output_png as tests/test_cpu_png.py's stand-in has them, and the _f forms beside them."""

    def __init__(self, stream=P.SIGNATURE + b'chunks'):
        self.calls, self.stream = [], stream

    def fl_png_bound(self, w, h, channels):
        self.calls.append(('fl_png_bound', w, h, channels))
        return PC.bound(w, h, channels, 32768)

    def fl_png_bound_f(self, w, h, channels, bits, flags):
        self.calls.append(('fl_png_bound_f', w, h, channels, bits, flags))
        return X.bound(w, h, channels, bits, 32768)

    def _write(self, host):
        if host:
            rec = np.array([len(self.stream), 0, 32768, 0], '<u4').tobytes() + self.stream
            C.memmove(host, rec, len(rec))
        return 0

    def fl_output_png(self, ctx, w, h, channels, host, dev, cap):
        self.calls.append(('fl_output_png', ctx, w, h, channels, host, dev, cap))
        return self._write(host)

    def fl_output_png_f(self, ctx, w, h, channels, bits, flags, host, dev, cap):
        self.calls.append(('fl_output_png_f', ctx, w, h, channels, bits, flags, host, dev, cap))
        return self._write(host)


class StubFB(object):
    ctx = 1234

    def host_buffer(self, shape, dtype):
        self.last = np.zeros(shape, dtype)
        return self.last


@pytest.mark.parametrize('alpha', (False, True))
def test_default_output_makes_the_calls_it_made(monkeypatch, alpha):
    stub = StubLib()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    ch = 4 if alpha else 3
    dim = render.Framebuffers.calc_dim(64, 48)
    cap = PC.bound(64, 48, ch, 32768)
    for out in (output.DevicePNGOutput(alpha=alpha), output.DevicePNGOutput(alpha=alpha, bits=8, filter='paeth')):
        assert (out.bits, out.filter, out.entry) == (8, 'paeth', 'fl_output_png')
        del stub.calls[:]
        fb = StubFB()
        buf = out.copy(fb, dim)
        assert [c[0] for c in stub.calls if c[0].endswith('_f')] == []
        assert [c for c in stub.calls if c[0] == 'fl_output_png'] == [('fl_output_png', 1234, 64, 48, ch, buf.ctypes.data, 0, cap)]
        assert set(c for c in stub.calls if c[0] != 'fl_output_png') == {('fl_png_bound', 64, 48, ch)}
        assert out.encode(buf)[0]['.png'].read() == stub.stream


@pytest.mark.parametrize('bits,filt', ((16, 'paeth'), (8, 'adaptive'), (16, 'adaptive')))
@pytest.mark.parametrize('alpha', (False, True))
def test_extended_output_calls_the_f_forms(monkeypatch, alpha, bits, filt):
    stub = StubLib()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    ch, flags = 4 if alpha else 3, 1 if filt == 'adaptive' else 0
    out = output.DevicePNGOutput(alpha=alpha, bits=bits, filter=filt)
    dim = render.Framebuffers.calc_dim(64, 48)
    cap = X.bound(64, 48, ch, bits, 32768)
    assert out.shape(dim) == (cap,) and np.dtype(out.dtype) == np.uint8 and out.suffix == '.png'
    assert (out.alpha, out.channels, out.bits, out.filter) == (alpha, ch, bits, filt)
    del stub.calls[:]
    fb = StubFB()
    buf = out.copy(fb, dim)
    assert buf.shape == (cap,)
    assert [c for c in stub.calls if c[0].startswith('fl_output')] == [('fl_output_png_f', 1234, 64, 48, ch, bits, flags, buf.ctypes.data, 0, cap)]
    assert set(c for c in stub.calls if not c[0].startswith('fl_output')) == {('fl_png_bound_f', 64, 48, ch, bits, flags)}
    media, logs = out.encode(buf)
    assert list(media) == ['.png'] and media['.png'].read() == stub.stream and logs == []
    assert out.copy(fb, dim, dev_out=4096, host=False) is None and stub.calls[-1][7:9] == (None, 4096)


def test_output_options():
    for bad in (dict(bits=True), dict(bits=12), dict(bits='16'), dict(bits=16.0), dict(bits=0), dict(bits=None), dict(filter='sub'),
                dict(filter=1), dict(filter=None), dict(filter='Adaptive'), dict(filter=True), dict(alpha=1, bits=16), dict(quality=90)):
        with pytest.raises((ValueError, TypeError)):
            output.DevicePNGOutput(**bad)
    for bad in (dict(bits=True), dict(bits=12), dict(filter='sub'), dict(filter=['paeth'])):
        with pytest.raises(ValueError):
            output.DevicePNGOutput(**bad)


def test_profile_keys():
    gnm, prof = configs.cfg2()

    def out_for(block):
        return output.get_output_for_profile(profile.wrap(dict(prof, output=block), gnm))

    dev = out_for({'type': 'png', 'encoder': 'device', 'bits': 16, 'filter': 'adaptive', 'alpha': True})
    assert type(dev) is output.DevicePNGOutput and (dev.alpha, dev.bits, dev.filter, dev.entry) == (True, 16, 'adaptive', 'fl_output_png_f')
    dev = out_for({'type': 'png', 'encoder': 'device', 'bits': 16})
    assert (dev.alpha, dev.bits, dev.filter) == (False, 16, 'paeth')
    dev = out_for({'type': 'png', 'encoder': 'device', 'filter': 'adaptive'})
    assert (dev.bits, dev.filter) == (8, 'adaptive')
    dev = out_for({'type': 'png', 'encoder': 'device'})
    assert (dev.bits, dev.filter, dev.entry) == (8, 'paeth', 'fl_output_png')
    with pytest.raises(ValueError, match='"alpha", "bits" and "filter"'):
        out_for({'type': 'png', 'encoder': 'device', 'quality': 90})
    for block in ({'type': 'png', 'encoder': 'device', 'bits': 12}, {'type': 'png', 'encoder': 'device', 'bits': True},
                  {'type': 'png', 'encoder': 'device', 'filter': 'up'}, {'type': 'png', 'encoder': 'device', 'optimize': True},
                  {'type': 'png', 'encoder': 'device', 'bits': 16, 'sampling': '420'}):
        with pytest.raises(ValueError):
            out_for(block)
    for block in ({'type': 'png', 'bits': 16}, {'type': 'png', 'filter': 'adaptive'}, {'type': 'tiff', 'bits': 16},
                  {'type': 'jpeg', 'device': True, 'bits': 8}, {'type': 'jpeg', 'filter': 'paeth'}, {'type': 'raw16', 'bits': 16},
                  {'bits': 16}, {'type': 'mjpeg', 'filter': 'adaptive'}, {'type': 'png', 'encoder': 'host', 'bits': 16}):
        with pytest.raises(ValueError, match=r'output\.(bits|filter): only the device PNG encoder'):
            out_for(block)
    assert type(out_for({'type': 'tiff'})) is output.TiffOutput and type(out_for({'type': 'png'})) is output.PILOutput


def test_command_line_options():
    parser = profile.add_args(argparse.ArgumentParser())

    def out_of(*argv):
        return profile.get_from_args(parser.parse_args(list(argv)))[1].get('output')

    assert out_of('--codec', 'png', '--device-encode', '--bits', '16') == {'type': 'png', 'encoder': 'device', 'bits': 16}
    assert out_of('--codec', 'png', '--device-encode', '--bits', '16', '--png-filter', 'adaptive') == {
        'type': 'png', 'encoder': 'device', 'bits': 16, 'filter': 'adaptive'}
    assert out_of('--png-filter', 'paeth', '--codec', 'png', '--device-encode') == {'type': 'png', 'encoder': 'device', 'filter': 'paeth'}
    assert out_of('--codec', 'png', '--device-encode') == {'type': 'png', 'encoder': 'device'}
    assert out_of('--codec', 'tiff', '--bits', '16') == {'type': 'tiff', 'bits': 16}          # the output factory refuses it
    for argv in (('--bits', '12'), ('--bits', 'x'), ('--png-filter', 'up')):
        with pytest.raises(SystemExit):
            parser.parse_args(list(argv))
    text = parser.format_help()
    assert text.index('--optimize') < text.index('--bits') < text.index('--png-filter')
    gnm, _ = configs.cfg2()
    _, prof = profile.get_from_args(parser.parse_args(['--codec', 'tiff', '--bits', '16']))
    with pytest.raises(ValueError, match=r'output\.bits'):
        output.get_output_for_profile(profile.wrap(prof, gnm))
    _, prof = profile.get_from_args(parser.parse_args(['--codec', 'png', '--device-encode', '--bits', '16', '--png-filter', 'adaptive']))
    dev = output.get_output_for_profile(profile.wrap(prof, gnm))
    assert type(dev) is output.DevicePNGOutput and (dev.bits, dev.filter) == (16, 'adaptive')
