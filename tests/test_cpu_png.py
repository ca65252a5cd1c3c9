"""
CPU tests of the device PNG output (no GPU): the parser, inflate and unfilters of tests/png_model.py against zlib and Pillow, the
model's own writer of the device's format on every edge case of tests/png_cases.py (so that a case's check is known to be
reachable before a device is asked), DevicePNGOutput and the profile / command-line plumbing against a stand-in library, and
the C ABI's three entry points.
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
import png_cases as PC
import png_model as P

SEG = 4096                    # flush distance of the zlib streams below


def _inputs():
    rs = np.random.RandomState(1)
    x = np.arange(20000)
    smooth = ((x // 7 + rs.randint(0, 2, x.size)) & 255).astype(np.uint8).tobytes()
    runs = b''.join(bytes([1 + k % 250]) + b'\0' * k for k in range(0, 301, 7)) + b'\xff' * 1000
    noise = rs.randint(0, 256, 3 * SEG + 100).astype(np.uint8).tobytes()
    text = (b'the quick brown fox jumps over the lazy dog; ' * 300)[:12345]         # matches at distances beyond 1
    return dict(smooth=smooth, runs=runs, noise=noise, text=text, empty=b'', one=b'\x07')


INPUTS = _inputs()
STRATEGIES = dict(default=(6, zlib.Z_DEFAULT_STRATEGY), rle=(6, zlib.Z_RLE), huffman_only=(6, zlib.Z_HUFFMAN_ONLY),
                  fixed=(6, zlib.Z_FIXED), level0=(0, zlib.Z_DEFAULT_STRATEGY))


# ------------------------------------------------------------------ the model against zlib and Pillow
@pytest.mark.parametrize('strategy', sorted(STRATEGIES))
@pytest.mark.parametrize('flush', (False, True))
def test_model_inflates_what_zlib_makes(strategy, flush):
    level, strat = STRATEGIES[strategy]
    types = set()
    for name, data in sorted(INPUTS.items()):
        co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strat)
        if flush:
            comp = b''.join(co.compress(data[lo:lo + SEG]) + co.flush(zlib.Z_FULL_FLUSH) for lo in range(0, len(data), SEG)) + co.flush()
        else:
            comp = co.compress(data) + co.flush()
        out, blocks = P.zlib_inflate(comp)
        assert out == data == zlib.decompress(comp), name
        assert blocks[-1]['final'] and not any(b['final'] for b in blocks[:-1])
        assert sum(b['literals'] + sum(m[0] for m in b['matches']) for b in blocks) == len(data)
        if strategy in ('rle', 'huffman_only', 'level0'):
            assert set(m[1] for b in blocks for m in b['matches']) <= {1}
        if strategy == 'huffman_only' or strategy == 'level0':
            assert not any(b['matches'] for b in blocks)
        if flush and data:                                    # a full flush ends on a byte boundary with an empty stored block
            empties = [b for b in blocks if b['type'] == 0 and b['start'] == b['end']]
            assert len(empties) >= -(-len(data) // SEG) and all(b['bit_end'] % 8 == 0 for b in empties)
        types |= set(b['type'] for b in blocks)
    assert types >= dict(default={1, 2}, rle={2}, huffman_only={2}, fixed={1}, level0={0})[strategy]


def test_model_reads_pillow_files():
    PIL_Image = pytest.importorskip('PIL.Image')
    rs = np.random.RandomState(2)
    seen = set()
    for w, h, ch in ((97, 61, 3), (64, 48, 4), (1, 1, 3), (7, 3, 4), (300, 40, 3)):
        x, y = np.arange(w)[None, :, None], np.arange(h)[:, None, None]
        pix = ((x * x // 9 + y * 3 + rs.randint(0, 2 + 60 * (y % 16 == 0), (h, w, ch))) & 255).astype(np.uint8)
        pix[h // 2:, : w // 2] = 0
        out = io.BytesIO()
        PIL_Image.fromarray(pix, 'RGB' if ch == 3 else 'RGBA').save(out, 'png')
        ps = P.parse(out.getvalue())
        assert (ps.w, ps.h, ps.channels) == (w, h, ch)
        assert np.array_equal(ps.pixels, pix) and np.array_equal(ps.pixels, np.asarray(PIL_Image.open(io.BytesIO(out.getvalue()))))
        assert ps.filtered == zlib.decompress(ps.zstream)
        seen |= set(ps.filters)
    print('filter types in Pillow\'s files:', sorted(seen))
    assert len(seen) >= 3                                     # Pillow chooses per row: the unfilters are exercised, not only type 0


@pytest.mark.parametrize('ftype', range(5))
def test_unfilters_invert_the_filters(ftype):
    rs = np.random.RandomState(ftype)
    for w, h, ch in ((1, 1, 3), (5, 4, 4), (33, 9, 3)):
        pix = rs.randint(0, 256, (h, w, ch)).astype(np.uint8)
        back, filters = P.unfilter(P.filter_rows(pix, ftype), w, h, ch)
        assert np.array_equal(back, pix) and filters == [ftype] * h
    with pytest.raises(P.PngError):
        P.unfilter(b'\x05\0\0\0', 1, 1, 3)


def test_checksums_agree_with_zlib():
    for data in INPUTS.values():
        assert P.adler32(data) == zlib.adler32(data) & 0xffffffff
        assert P.crc32(data[:3000]) == zlib.crc32(data[:3000]) & 0xffffffff
    big = b'\xff' * 300000                                    # the sum b passes 2^32 well before the end
    assert P.adler32(big) == zlib.adler32(big) & 0xffffffff


def test_model_refuses_broken_files():
    rgba, ch, _ = PC.case('smooth_256x96', PC.MODEL_SEG)
    data = P.encode(rgba[:, :, :ch], PC.MODEL_SEG)
    P.parse(data, PC.MODEL_SEG)
    idat = data.index(b'IDAT')
    n, = struct.unpack('>I', data[idat - 4:idat])
    crc_at = idat + 4 + n
    with pytest.raises(P.PngError, match='CRC'):              # a corrupted CRC
        P.parse(data[:crc_at] + bytes([data[crc_at] ^ 1]) + data[crc_at + 1:])
    with pytest.raises(P.PngError, match='CRC'):              # a corrupted byte under a good CRC's eyes
        P.parse(data[:idat + 40] + bytes([data[idat + 40] ^ 0x10]) + data[idat + 41:])
    z = b''.join(P.parse(data).idat)
    P.zlib_inflate(z)
    with pytest.raises(P.PngError, match='Adler'):            # a corrupted Adler-32
        P.zlib_inflate(z[:-1] + bytes([z[-1] ^ 1]))
    for bad in (data[:-1], data + b'\0', data[:8] + data[8 + 25:], b'\x88' + data[1:]):
        with pytest.raises(P.PngError):
            P.parse(bad)
    # an over-subscribed code-length code: four codes of one bit
    w = P._BitWriter()
    w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for _ in range(4):
        w.put(1, 3)
    w.put(0, 32)
    with pytest.raises(P.PngError, match='over-subscribed'):
        P.inflate(bytes(w.out))
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(w.out), -15)
    # ... and an incomplete one, which zlib rejects as well: two codes of two bits
    w = P._BitWriter()
    w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for ln in (2, 2, 0, 0):
        w.put(ln, 3)
    w.put(0, 32)
    with pytest.raises(P.PngError, match='incomplete'):
        P.inflate(bytes(w.out))
    with pytest.raises(zlib.error):
        zlib.decompress(bytes(w.out), -15)
    # a match that reaches before its segment's start is refused when the segment length is given
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    raw = co.compress(b'\0' * 600) + co.flush()
    assert P.inflate(raw)[0] == b'\0' * 600
    with pytest.raises(P.PngError, match='segment'):
        P.inflate(raw, seg=256)


# ------------------------------------------------------------------ the device's format, written by the model, on every edge case
@pytest.mark.parametrize('name', PC.NAMES)
def test_cases_contain_their_edge(name):
    seg = PC.MODEL_SEG
    rgba, ch, check = PC.case(name, seg)
    data = P.encode(rgba[:, :, :ch], seg)
    ps = P.parse(data, seg)
    assert (ps.w, ps.h, ps.channels) == (rgba.shape[1], rgba.shape[0], ch)
    assert np.array_equal(ps.pixels, rgba[:, :, :ch])
    assert zlib.decompress(ps.zstream) == ps.filtered == P.filter_rows(np.ascontiguousarray(rgba[:, :, :ch]))
    st = PC.stats_of(ps, seg)
    check(st, seg)
    assert st['distances'] in ([], [1]) and set(st['block_types']) <= {0, 2} and st['finals'] == [0] * (len(st['finals']) - 1) + [1]
    assert all(s['aligned'] for s in st['segments'][:-1]) and st['nidat'] == len(st['segments'])
    assert 16 + len(data) <= PC.bound(ps.w, ps.h, ch, seg)
    try:
        import PIL.Image
    except ImportError:
        return
    im = PIL.Image.open(io.BytesIO(data))
    assert im.size == (ps.w, ps.h) and im.mode == ('RGB' if ch == 3 else 'RGBA')
    assert np.array_equal(np.asarray(im), rgba[:, :, :ch])


@pytest.mark.parametrize('maxlen,n', ((15, 30), (7, 19), (15, 2), (3, 8)))
def test_length_limited_codes_are_complete(maxlen, n):
    fib = [1, 1]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    for freq in (fib[:n], [1] * n, list(range(1, n + 1)), [0, 5] * (n // 2) + [3]):
        lens = P.limited_lengths(freq, maxlen)
        used = [ln for ln in lens if ln]
        assert max(used) <= maxlen and sum(2 ** (maxlen - ln) for ln in used) == 2 ** maxlen, (freq, lens)
        assert all(bool(f) == bool(ln) for f, ln in zip(freq, lens)) or len([f for f in freq if f]) == 1
        order = sorted((f, i) for i, f in enumerate(freq) if f)
        assert [lens[i] for _, i in order] == sorted((lens[i] for _, i in order), reverse=True)      # never a longer code for a commoner symbol


def test_a_lone_symbol_gets_a_complete_code():
    assert P.limited_lengths([0, 0, 7, 0], 15) == [1, 0, 1, 0] and P.limited_lengths([7, 0, 0], 7) == [1, 1, 0]


# ------------------------------------------------------------------ DevicePNGOutput and the plumbing, against a stand-in library
class StubLib(object):
    def __init__(self, stream=P.SIGNATURE + b'chunks', status=0):
        self.calls, self.stream, self.status = [], stream, status

    def fl_png_bound(self, w, h, channels):
        return PC.bound(w, h, channels, 32768)

    def fl_output_png(self, ctx, w, h, channels, host, dev, cap):
        self.calls.append((ctx, w, h, channels, host, dev, cap))
        if host:
            rec = np.array([len(self.stream), self.status, 32768, 0], '<u4').tobytes() + (b'' if self.status else self.stream)
            C.memmove(host, rec, len(rec))
        return 0


class StubFB(object):
    ctx = 1234

    def host_buffer(self, shape, dtype):
        self.last = np.zeros(shape, dtype)
        return self.last


@pytest.mark.parametrize('alpha', (False, True))
def test_device_output_class(monkeypatch, alpha):
    stub = StubLib()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    out = output.DevicePNGOutput(alpha=alpha)
    ch = 4 if alpha else 3
    dim = render.Framebuffers.calc_dim(64, 48)
    cap = PC.bound(64, 48, ch, 32768)
    assert out.shape(dim) == (cap,) and np.dtype(out.dtype) == np.uint8 and out.suffix == '.png' and out.alpha is alpha
    fb = StubFB()
    buf = out.copy(fb, dim)
    assert buf is fb.last and buf.shape == (cap,)
    assert stub.calls == [(1234, 64, 48, ch, buf.ctypes.data, 0, cap)]
    media, logs = out.encode(buf)
    assert list(media) == ['.png'] and media['.png'].read() == stub.stream and logs == []
    assert out.encode(None) == ({}, [])
    assert out.copy(fb, dim, dev_out=4096, host=False) is None and stub.calls[-1][4:6] == (None, 4096)
    stub.status = 1                                           # status 1: the needed size is reported
    with pytest.raises(_lib.FlameError, match=str(len(stub.stream))):
        out.encode(out.copy(fb, dim))


def test_device_output_options():
    assert output.DevicePNGOutput().alpha is False
    for bad in (dict(quality=90), dict(alpha=1), dict(alpha='yes'), dict(codec='png')):
        with pytest.raises((ValueError, TypeError)):
            output.DevicePNGOutput(**bad)


def test_profile_selects_the_output():
    gnm, prof = configs.cfg2()

    def out_for(block):
        return output.get_output_for_profile(profile.wrap(dict(prof, output=block), gnm))

    dev = out_for({'type': 'png', 'encoder': 'device'})
    assert type(dev) is output.DevicePNGOutput and dev.alpha is False and dev.channels == 3
    dev = out_for({'type': 'png', 'encoder': 'device', 'alpha': True})
    assert type(dev) is output.DevicePNGOutput and dev.alpha is True and dev.channels == 4
    for block in ({'type': 'png'}, {'type': 'png', 'alpha': True}, {'type': 'png', 'device': False}):      # no `encoder`: the host path, as before
        plain = out_for(block)
        assert type(plain) is output.PILOutput and plain.type == 'png' and plain.alpha is bool(block.get('alpha'))
    for block in ({'type': 'png', 'device': True},                                        # `device` stays the JPEG switch
                  {'type': 'png', 'encoder': 'device', 'quality': 90},                      # no other option, quality included
                  {'type': 'png', 'encoder': 'device', 'device': True},
                  {'type': 'png', 'encoder': 'host'}, {'type': 'png', 'encoder': True},
                  {'type': 'jpeg', 'encoder': 'device'}, {'encoder': 'device'}, {'type': 'tiff', 'encoder': 'device'},
                  {'type': 'png', 'encoder': 'device', 'alpha': 1}):
        with pytest.raises(ValueError):
            out_for(block)
    assert isinstance(out_for({'type': 'jpeg', 'device': True, 'quality': 70}), output.DeviceJPEGOutput)
    assert output.get_suffix_for_profile(profile.wrap(dict(prof, output={'type': 'png', 'encoder': 'device'}), gnm)) == '.png'


def test_command_line_options():
    parser = profile.add_args(argparse.ArgumentParser())

    def out_of(*argv):
        return profile.get_from_args(parser.parse_args(list(argv)))[1].get('output')

    assert out_of('--codec', 'png', '--device-encode') == {'type': 'png', 'encoder': 'device'}
    assert out_of('--device-encode', '--codec', 'png') == {'type': 'png', 'encoder': 'device'}
    assert out_of('--device-encode', '--quality', '92') == {'device': True, 'quality': 92}
    assert out_of('--codec', 'jpeg', '--device-encode') == {'type': 'jpeg', 'device': True}
    assert out_of('--codec', 'png') == {'type': 'png'}
    assert out_of() is None
    assert 'png' in parser.format_help().split('--device-encode')[-1].split('--quality')[0]
    # a JSON profile whose output is png: the switch follows the type the profile ends up with
    _, prof = profile.get_from_args(argparse.Namespace(profile=None, builtin_profile='720p', device_encode=True, codec='png'))
    assert prof['output'] == {'type': 'png', 'encoder': 'device'}


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_png_bound', 'fl_png_encode', 'fl_output_png'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert int(re.search(r'#define\s+FL_PNG_HEADER_BYTES\s+(\d+)', code).group(1)) == P.HEADER_BYTES == _lib.PNG_HEADER_BYTES
    assert lib.fl_abi_version() == 1
    # host-only entry point: usable without a GPU
    for w, h, ch in ((0, 8, 3), (8, 0, 3), (65536, 8, 3), (8, 65536, 4), (8, 8, 2), (8, 8, 5), (8, 8, 0), (65535, 65535, 3)):
        assert lib.fl_png_bound(w, h, ch) == 0, (w, h, ch)
    b = lib.fl_png_bound(1920, 1080, 3)
    F = 1080 * (1 + 3 * 1920)
    nseg = (b - (16 + 33 + 2 + F + 4 + 12)) // 17
    assert b == 16 + 33 + 2 + F + 17 * nseg + 4 + 12 and nseg >= 1 and -(-F // nseg) <= 65535      # every segment one stored block
    assert lib.fl_png_bound(1, 1, 3) == 16 + 33 + 2 + 4 + 17 + 4 + 12 and lib.fl_png_bound(1, 1, 4) == lib.fl_png_bound(1, 1, 3) + 1
    assert 0 < lib.fl_png_bound(16000, 65535, 4) < 2 ** 32
    for bad in ((None, 8, 8, 1, 3, None, 0, 4096), (None, 8, 8, 1, 3, 1, 0, 4096)):
        assert lib.fl_png_encode(*bad) == _lib.FL_E_INVAL             # (a null context: refused before the device is touched)
