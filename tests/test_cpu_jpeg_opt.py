"""
CPU tests of the device JPEG encoder's optimised Huffman tables (no GPU): the numpy model of
tests/jpeg_opt_model.py against Pillow, against the models of the standard-table files and against itself on every frame of
tests/jpeg_opt_cases.py, the profile / command-line plumbing against a stand-in library, and the host side of the C ABI.

test_size asks that no optimised file be larger than the standard file of the same coefficients, for every frame of the two
case modules and deep_code.  Listing all 162 AC symbols at a frequency of at least 2 costs frames of a few dozen symbols more
than Annex K asks (EOB 7 or 8 bits instead of 4 or 2), so a table that does not save code bits is Annex K's (jpeg_opt_model):
a one-MCU frame then keeps most or all of Annex K's tables (with all four it is the standard file, byte for byte), and
test_fallback pins the rule.
"""
import argparse
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, encoders, output, profile, render
import jpeg420_model as M
import jpeg_model as J
import jpeg_opt_cases as OC
import jpeg_opt_model as O

S444, S420 = OC.S444, OC.S420
SAMPLINGS = [pytest.param(S444, id='444'), pytest.param(S420, id='420')]
ALL = [pytest.param(s, n, id='%s-%s' % ('420' if s else '444', n)) for s in (S444, S420) for n in OC.names(s)]
_files = {}


def model_files(sampling, name):
    """(planes, quality, check, ri, coefficients, the standard file, the optimised file), computed once."""
    if (sampling, name) not in _files:
        mod = M if sampling == S420 else J
        ri = OC.CASE_MODULE[sampling].MODEL_RI
        planes, quality, check = OC.case(name, ri, sampling)
        qt = J.quant_tables(quality)
        coef = mod.quantise(mod.dct_values(planes), qt)
        w, h = planes.shape[2], planes.shape[1]
        std = O.assemble(w, h, qt, ri, coef, sampling, O.STANDARD)
        if name != OC.DEEP_CODE:                               # the vectorised writer against the models' own, symbol by symbol
            assert std == mod.assemble(w, h, qt, ri, coef)
        _files[(sampling, name)] = (planes, quality, check, ri, coef, std, O.assemble(w, h, qt, ri, coef, sampling))
    return _files[(sampling, name)]


def pillow_ycc(data):
    PIL_Image = pytest.importorskip('PIL.Image')
    im = PIL_Image.open(io.BytesIO(data))
    im.draft('YCbCr', im.size)
    assert im.mode == 'YCbCr'
    return im, np.asarray(im)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize('sampling,name', ALL)
def test_pillow_decodes_the_optimised_file_to_the_same_pixels(sampling, name):
    planes, quality, _, _, _, std, opt = model_files(sampling, name)
    im, a = pillow_ycc(opt)
    _, b = pillow_ycc(std)
    assert im.size == (planes.shape[2], planes.shape[1]) and np.array_equal(a, b)


@pytest.mark.parametrize('sampling,name', ALL)
def test_model_against_itself(sampling, name):
    """The strict parser accepts the optimised file, returns the coefficients it was written from and finds the case's edge in
    it; the header differs from the standard file's in the DHT bodies only; the standard parsers refuse the file unless all four
    tables stayed Annex K's, when it is the standard file."""
    planes, quality, check, ri, coef, std, opt = model_files(sampling, name)
    ps = O.parse(opt)
    assert (ps.w, ps.h, ps.restart_interval, ps.sampling) == (planes.shape[2], planes.shape[1], ri, sampling)
    assert np.array_equal(ps.qtables, J.quant_tables(quality)) and np.array_equal(ps.coefficients, coef)
    check(ps.stats, ri)
    assert ps.tables == tuple((list(b), list(v)) for b, v in O.tables(coef, ri, sampling))
    differs = [i for i in range(O.HEADER_BYTES) if opt[i] != std[i]]
    assert all(any(off <= i < off + 16 + n for off, n in zip(O.DHT_BODY, O.DHT_SYMBOLS)) for i in differs)
    assert np.array_equal(O.parse(std, optimised=False).coefficients, coef)
    kept = [ps.tables[i] == (list(O.STANDARD[i][0]), list(O.STANDARD[i][1])) for i in range(4)]
    if all(kept):
        assert opt == std and not differs
        return
    assert differs
    with pytest.raises(J.JpegError):
        O.parse(opt, optimised=False)
    if name != OC.DEEP_CODE:
        with pytest.raises(J.JpegError):
            (M if sampling == S420 else J).parse(opt)


@pytest.mark.parametrize('sampling', SAMPLINGS)
def test_deep_code_exercises_the_limiter(sampling):
    """Huffman's own code for both AC tables of deep_code passes 16 bits; the limited code stops at 16 and uses it."""
    _, _, _, ri, coef, _, opt = model_files(sampling, OC.DEEP_CODE)
    cnt = O.counts(coef, ri, sampling)
    depth = [O.unlimited_depth(cnt[i], i & 1) for i in range(4)]
    print('unlimited depths DC lum, AC lum, DC chr, AC chr:', depth)
    assert depth[1] > 16 and depth[3] > 16
    tabs = O.parse(opt).tables
    assert [max(l for l in range(1, 17) if t[0][l - 1]) for t in (tabs[1], tabs[3])] == [16, 16]


@pytest.mark.parametrize('sampling,name', [p for p in ALL if p.values[1] != OC.ONE_MCU])
def test_size(sampling, name):
    _, _, _, _, _, std, opt = model_files(sampling, name)
    print('%s: standard %d bytes, optimised %d' % (name, len(std), len(opt)))
    assert len(opt) <= len(std)


def test_fallback():
    """A table that saves no code bits is Annex K's: all four on the one-MCU noise frame of 4:2:0, none on a frame of some size; and the
    rule is the one the model states, sum count * length against Annex K's, a tie keeping Annex K."""
    std_tabs = tuple((list(b), list(v)) for b, v in O.STANDARD)
    _, _, _, _, _, std, opt = model_files(S420, 'noise_16x16_q50')
    assert opt == std and O.parse(opt).tables == std_tabs
    kept = [t == k for t, k in zip(O.parse(model_files(S444, 'noise_8x8_q50')[6]).tables, std_tabs)]
    assert kept == [True, True, False, True]                             # table by table: here the chrominance DC table alone pays
    for sampling in (S444, S420):
        for name in ('noise_64x40_q100', 'rst_wraps', OC.DEEP_CODE):
            tabs = O.parse(model_files(sampling, name)[6]).tables
            assert all(tabs[i] != std_tabs[i] for i in range(4)), name
        _, _, _, ri, coef, _, opt = model_files(sampling, OC.ONE_MCU)
        cnt, tabs = O.counts(coef, ri, sampling), O.parse(opt).tables
        for i in range(4):
            mine, annex = J.huff_codes(tabs[i]), J.huff_codes(O.STANDARD[i])
            cost = [sum(int(cnt[i][s]) * c[s][1] for s in O.LEGAL[i & 1]) for c in (mine, annex)]
            assert cost[0] <= cost[1] and (cost[0] < cost[1]) == (tabs[i] != std_tabs[i])
    count = np.zeros(256, np.int64)
    count[0], count[1] = 5, 1                                            # DC luminance: Annex K spends 2 and 3 bits, 13 bits in all
    assert O.table_of(count, 0) == list(std_tabs[0])
    count[0] = 500                                                       # category 0 at one bit: 501 against 1003
    assert O.table_of(count, 0) != list(std_tabs[0]) and J.huff_codes(O.table_of(count, 0))[0][1] == 1


def test_strict_parser_refuses_broken_tables():
    _, _, _, _, _, _, opt = model_files(S444, 'noise_64x40_q100')
    off = O.DHT_BODY[1]
    bad = bytearray(opt)
    bad[off + 16], bad[off + 17] = bad[off + 17], bad[off + 16]          # two symbols of one length out of order
    with pytest.raises(J.JpegError):
        O.parse(bytes(bad))
    bad = bytearray(opt)
    bad[off + 16 + 161] = bad[off + 16 + 160]                            # a symbol twice, another missing
    with pytest.raises(J.JpegError):
        O.parse(bytes(bad))
    bits = list(opt[off:off + 16])
    lmax = max(l for l in range(1, 17) if bits[l - 1])
    assert lmax < 16
    bad = bytearray(opt)
    bad[off + lmax - 1] -= 1
    bad[off + lmax] += 1                                                 # a symbol moved one length down: the Kraft sum falls short
    with pytest.raises(J.JpegError):
        O.parse(bytes(bad))
    for i in range(4):
        O.check_table(O.STANDARD[i], i & 1)                              # (Annex K's tables keep the same rules)
    full = ([0, 0, 4, 8] + [0] * 12, list(range(12)))                    # a complete code: the all-ones codeword is assigned
    with pytest.raises(J.JpegError):
        O.check_table(full, 0)


# ------------------------------------------------------------------ the outputs against a stand-in library
class StubLib(object):
    def __init__(self, stream):
        self.calls, self.stream = [], stream

    def _answer(self, host):
        if host:
            rec = np.array([len(self.stream), 0, 4, 0], '<u4').tobytes() + self.stream
            C.memmove(host, rec, len(rec))
        return 0

    def fl_output_jpeg(self, ctx, w, h, quality, host, dev, cap):
        self.calls.append(('fl_output_jpeg', ctx, w, h, quality, host, dev, cap))
        return self._answer(host)

    def fl_output_jpeg_s(self, ctx, w, h, quality, sampling, host, dev, cap):
        self.calls.append(('fl_output_jpeg_s', ctx, w, h, quality, sampling, host, dev, cap))
        return self._answer(host)

    def fl_output_jpeg_f(self, ctx, w, h, quality, sampling, flags, host, dev, cap):
        self.calls.append(('fl_output_jpeg_f', ctx, w, h, quality, sampling, flags, host, dev, cap))
        return self._answer(host)


class StubFB(object):
    ctx = 1234

    def host_buffer(self, shape, dtype):
        return np.zeros(shape, dtype)


def _out_for(block, **prof_keys):
    gnm, prof = configs.cfg2()
    return output.get_output_for_profile(profile.wrap(dict(prof, output=block, **prof_keys), gnm))


def test_optimize_reaches_the_library(monkeypatch):
    stub = StubLib(M.encode(np.zeros((3, 16, 24), np.uint8), 60, 4))
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    dim, fb = render.Framebuffers.calc_dim(64, 48), StubFB()
    cap = 16 + J.HEADER_BYTES + 2 * 3 * 64 * 48
    for block, cls, sampling in (({'type': 'jpeg', 'device': True, 'quality': 85, 'optimize': True}, output.DeviceJPEGOutput, 0),
                                 ({'type': 'jpeg', 'device': True, 'quality': 85, 'sampling': '420', 'optimize': True}, output.DeviceJPEGOutput, 1),
                                 ({'type': 'mjpeg', 'quality': 85, 'optimize': True}, encoders.MJPEGOutput, 1),
                                 ({'type': 'mjpeg', 'quality': 85, 'sampling': '444', 'optimize': True}, encoders.MJPEGOutput, 0)):
        out = _out_for(block)
        assert type(out) is cls and out.optimize is True and out.capacity(dim) == cap
        buf = out.copy(fb, dim)
        assert stub.calls == [('fl_output_jpeg_f', 1234, 64, 48, 85, sampling, _lib.JPEG_OPTIMIZE, buf.ctypes.data, 0, cap)]
        del stub.calls[:]
        media, logs = out.encode(buf)
        if cls is output.DeviceJPEGOutput:
            assert list(media) == ['.jpg'] and media['.jpg'].read() == stub.stream
        else:
            assert media == {} and list(out.encode(None)[0]) == ['.avi']
    assert _lib.JPEG_OPTIMIZE == 1
    assert output.DeviceJPEGOutput(optimize=True).copy(fb, dim, dev_out=4096, host=False) is None and stub.calls[-1][7:9] == (None, 4096)


def test_without_the_key_the_calls_are_the_calls_of_before(monkeypatch):
    stub = StubLib(b'\xff\xd8stream\xff\xd9')
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    dim, fb = render.Framebuffers.calc_dim(64, 48), StubFB()
    cap = 16 + J.HEADER_BYTES + 2 * 3 * 64 * 48
    for out in (_out_for({'type': 'jpeg', 'device': True, 'quality': 85}), _out_for({'type': 'jpeg', 'device': True, 'quality': 85, 'optimize': False}),
                output.DeviceJPEGOutput(quality=85), output.DeviceJPEGOutput(quality=85, sampling='444', optimize=False)):
        assert out.optimize is False
        buf = out.copy(fb, dim)
        assert stub.calls == [('fl_output_jpeg', 1234, 64, 48, 85, buf.ctypes.data, 0, cap)]
        del stub.calls[:]
    for out in (_out_for({'type': 'jpeg', 'device': True, 'quality': 85, 'sampling': '420'}), _out_for({'type': 'mjpeg', 'quality': 85}),
                _out_for({'type': 'mjpeg', 'quality': 85, 'optimize': False}), encoders.MJPEGOutput(quality=85)):
        buf = out.copy(fb, dim)
        assert stub.calls == [('fl_output_jpeg_s', 1234, 64, 48, 85, 1, buf.ctypes.data, 0, cap)]
        del stub.calls[:]
    buf = _out_for({'type': 'mjpeg', 'quality': 85, 'sampling': '444'}).copy(fb, dim)
    assert stub.calls == [('fl_output_jpeg', 1234, 64, 48, 85, buf.ctypes.data, 0, cap)]


def test_refusals():
    for bad in (1, 0, 'yes', None):
        for block in ({'type': 'jpeg', 'device': True, 'optimize': bad}, {'type': 'mjpeg', 'optimize': bad}):
            with pytest.raises(ValueError, match='optimize'):
                _out_for(block)
    for block in ({'type': 'jpeg', 'optimize': True}, {'type': 'jpeg', 'device': False, 'optimize': True}, {'type': 'jpeg', 'optimize': False}):
        with pytest.raises(ValueError, match=r'optimize.*"device": true'):
            _out_for(block)
    for block in ({'type': 'png', 'optimize': True}, {'type': 'png', 'encoder': 'device', 'optimize': True}, {'type': 'tiff', 'optimize': True}):
        with pytest.raises(ValueError, match='optimize'):
            _out_for(block)
    with pytest.raises(ValueError, match='alpha'):
        _out_for({'type': 'jpeg', 'device': True, 'optimize': True, 'alpha': True})
    with pytest.raises(ValueError):
        _out_for({'type': 'mjpeg', 'optimize': True, 'sampling': '422'})


def test_command_line_options():
    parser = profile.add_args(argparse.ArgumentParser())
    gnm, _ = configs.cfg2()
    _, prof = profile.get_from_args(parser.parse_args(['--codec', 'mjpeg', '--optimize', '--quality', '80']))
    assert prof['output'] == {'type': 'mjpeg', 'quality': 80, 'optimize': True}
    mj = output.get_output_for_profile(profile.wrap(prof, gnm))
    assert type(mj) is encoders.MJPEGOutput and mj.optimize is True and mj.sampling == '420'
    _, prof = profile.get_from_args(parser.parse_args(['--codec', 'jpeg', '--device-encode', '--optimize']))
    assert prof['output'] == {'type': 'jpeg', 'device': True, 'optimize': True}
    assert output.get_output_for_profile(profile.wrap(prof, gnm)).optimize is True
    _, prof = profile.get_from_args(parser.parse_args(['--codec', 'jpeg', '--optimize']))
    with pytest.raises(ValueError, match='"device": true'):
        output.get_output_for_profile(profile.wrap(prof, gnm))
    _, prof = profile.get_from_args(parser.parse_args(['--codec', 'mjpeg']))
    assert prof['output'] == {'type': 'mjpeg'}


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_jpeg_bound_f', 'fl_jpeg_encode_f', 'fl_output_jpeg_f'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert re.search(r'FL_JPEG_OPTIMIZE\s*=\s*1\b', code)
    assert lib.fl_abi_version() == 1
    for flags in (0, 1, 2):
        assert lib.fl_jpeg_encode_f(None, 16, 16, 1, 50, 1, flags, None, 0, 4096) == _lib.FL_E_INVAL      # a null context: refused before the device is touched
        assert lib.fl_output_jpeg_f(None, 16, 16, 50, 1, flags, None, 0, 4096) == _lib.FL_E_INVAL


def test_bound(built):
    lib = _lib.load()
    sizes = ((1, 1), (8, 8), (16, 16), (17, 9), (1920, 1080), (65535, 65535))
    for w, h in sizes:
        for s in (0, 1):
            assert lib.fl_jpeg_bound_f(w, h, s, 0) == lib.fl_jpeg_bound_s(w, h, s) > 0
    for w, h in sizes[:-1]:
        assert lib.fl_jpeg_bound_f(w, h, 1, 1) == 16 + J.HEADER_BYTES + 2494 * ((w + 15) // 16) * ((h + 15) // 16)
        assert lib.fl_jpeg_bound_f(w, h, 0, 1) == 16 + J.HEADER_BYTES + 1248 * ((w + 7) // 8) * ((h + 7) // 8) == lib.fl_jpeg_bound(w, h)
    # the worst MCU with a frame's own tables: a DC code of 13 leaves takes up to 12 bits, an AC code up to 16
    assert 2 * -(-6 * (12 + 11 + 63 * 26) // 8) + 2 == 2494 and 2 * -(-3 * (12 + 11 + 63 * 26) // 8) + 2 == 1248
    for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        for s in (0, 1):
            for flags in (0, 1):
                assert lib.fl_jpeg_bound_f(w, h, s, flags) == 0
    for s in (-1, 2, 420):
        assert lib.fl_jpeg_bound_f(16, 16, s, 0) == lib.fl_jpeg_bound_f(16, 16, s, 1) == 0
    for flags in (2, 3, 4, 0x80000000):
        assert lib.fl_jpeg_bound_f(16, 16, 0, flags) == lib.fl_jpeg_bound_f(16, 16, 1, flags) == 0
    # more than 2^24 blocks: the counts would not fit the builder's 32-bit sums
    assert lib.fl_jpeg_bound_f(18912, 18912, 0, 1) > 0 and 3 * 2364 * 2364 <= 2 ** 24 < 3 * 2365 * 2365
    assert lib.fl_jpeg_bound_f(18913, 18913, 0, 1) == 0 and lib.fl_jpeg_bound_f(18913, 18913, 0, 0) > 0
    assert lib.fl_jpeg_bound_f(65535, 65535, 0, 1) == 0 and lib.fl_jpeg_bound_f(65535, 65535, 1, 1) == 0
    assert lib.fl_jpeg_bound_f(26752, 26752, 1, 1) > 0 and 6 * 1672 * 1672 <= 2 ** 24 < 6 * 1673 * 1673
    assert lib.fl_jpeg_bound_f(26753, 26753, 1, 1) == 0
