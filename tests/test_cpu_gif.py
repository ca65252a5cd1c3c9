"""
CPU tests of the device GIF encoder's format (no GPU).  The model of tests/gif_model.py is held to Pillow, which opens every file it
writes and returns palette[index] for every frame, and to its own strict LZW reader, which returns the indices; the quantiser's
rules are pinned on hand-made histograms; the file around the blocks (GIFOutput) is driven with model-made blocks; the output
selection, the command line and the C ABI's refusals that need no device are driven; and the definition's quality is compared with
Pillow's own median cut on a flame-like picture.
"""
import argparse
import ctypes as C
import io
import os
import re
import struct

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, encoders, output, profile, render
import gif_cases as GC
import gif_model as M

PIL_Image = pytest.importorskip('PIL.Image')


def frames_of(data):
    im = PIL_Image.open(io.BytesIO(data))
    out = []
    for k in range(im.n_frames):
        im.seek(k)
        out.append((np.asarray(im.convert('RGB')).copy(), dict(im.info)))
    return im.size, out


# ------------------------------------------------------------------ the model against Pillow and against its own reader
@pytest.mark.parametrize('name', GC.NAMES)
def test_pillow_and_the_strict_reader_return_the_model_s_pixels(name):
    frame, colors, amp = GC.cases()[name]
    h, w = frame.shape[:2]
    pal, idx, nb = GC.model(name)
    assert 1 <= nb <= colors and not pal[nb:].any() and idx.max() < nb
    block = GC.model_block(name)
    assert len(block) + 16 <= M.bound(w, h)
    w2, h2, pal2, idx2 = M.decode_block(block)
    assert (w2, h2) == (w, h) and np.array_equal(pal2, pal) and np.array_equal(idx2, idx)
    size, frames = frames_of(M.gif_file(w, h, [block, block], fps=25, loop=0))
    assert size == (w, h) and len(frames) == 2
    for got, info in frames:
        assert np.array_equal(got, pal[idx])


def test_segment_lengths():
    """Other segment lengths decode as well, and the reader is told the length: a wrong one is refused."""
    frame, colors, amp = GC.cases()['gradient_c256_a8']
    pal, idx, _ = M.quantise(frame, colors, amp)
    for seg in (256, 1000, 3584):
        block = M.block_of(96, 64, pal, idx, seg)
        assert np.array_equal(M.decode_block(block, seg)[3], idx)
        assert np.array_equal(frames_of(M.gif_file(96, 64, [block]))[1][0][0], pal[idx])
    with pytest.raises(M.GifError):
        M.decode_block(M.block_of(96, 64, pal, idx, 256), 1024)


def test_cases_are_what_the_device_test_needs():
    cases = GC.cases()
    for r, n in GC.MOD255.items():
        assert M.stream_bytes(GC.model_block('mod255_%d' % r)) % 255 == r
    assert GC.model('black')[2] == 1 and GC.model('one_bright')[2] == 2
    assert GC.gradient().shape == (64, 96, 4) and len(set(M.cells_of(GC.gradient()[:, :, :3]).ravel())) > 256
    assert len(set(M.cells_of(GC.lone_colours()))) == 256
    for n in (1023, 1024, 1025):
        f = cases['n%d' % n][0]
        assert f.shape[0] * f.shape[1] == n
    # the last segment's final code falls below, on and above both bit steps
    for L in GC.STEP_LENGTHS:
        frame, colors, amp = cases['step_%d' % L]
        pal, idx, nb = GC.model('step_%d' % L)
        assert nb == 256 and amp == 0 and np.array_equal(pal[idx], frame[:, :, :3])
        assert M.final_width(idx.ravel()[1024:]) == (9 if L < 256 else 10 if L < 768 else 11)      # a code for every pixel: the L-th code
        assert M.final_width(idx.ravel()[:1024]) == 11
    frame = cases['few_colours'][0]
    pal, idx, nb = GC.model('few_colours')
    assert np.array_equal(pal[idx], frame[:, :, :3])
    assert np.array_equal(frames_of(M.gif_file(frame.shape[1], 1, [GC.model_block('few_colours')]))[1][0][0], frame[:, :, :3])


def test_the_strict_reader_refuses():
    frame, colors, amp = GC.cases()['37x29']
    pal, idx, _ = M.quantise(frame, colors, amp)
    stream = M.lzw_stream(idx)
    assert np.array_equal(M.decode_stream(stream, idx.size), idx.ravel())
    with pytest.raises(M.GifError, match='behind END'):
        M.decode_stream(stream + b'\0', idx.size)

    def bits(codes):
        b = M._Bits()
        for code, width in codes:
            b.put(code, width)
        if b.n:
            b.put(0, 8 - b.n)
        return bytes(b.out)
    assert M.decode_stream(bits([(256, 9), (5, 9), (5, 9), (257, 9)]), 2).tolist() == [5, 5]
    assert M.decode_stream(bits([(256, 9), (5, 9), (258, 9), (257, 9)]), 3).tolist() == [5, 5, 5]      # the string just added
    with pytest.raises(M.GifError, match='above next'):
        M.decode_stream(bits([(256, 9), (5, 9), (259, 9), (257, 9)]), 3)
    assert M.decode_stream(bits([(256, 9), (5, 9), (6, 9), (7, 9), (257, 9)]), 3).tolist() == [5, 6, 7]
    with pytest.raises(M.GifError):                      # an encoder that widens too early: a width other than the expected one
        M.decode_stream(bits([(256, 9), (5, 9), (6, 10), (7, 10), (257, 10)]), 3)
    with pytest.raises(M.GifError, match='clear'):
        M.decode_stream(bits([(5, 9), (5, 9), (257, 9)]), 2)
    block = M.block_of(37, 29, pal, idx)
    assert np.array_equal(M.decode_block(block)[3], idx)
    short = bytearray(block)
    short[M.HEADER_BYTES] -= 1                           # a first sub-block that claims 254 bytes
    with pytest.raises(M.GifError):
        M.decode_block(bytes(short))
    with pytest.raises(M.GifError):
        M.decode_block(block[:-1])
    with pytest.raises(M.GifError):
        M.decode_block(block + b'\0')


# ------------------------------------------------------------------ the quantiser's rules on hand-made histograms
def hist(cells):
    count = np.zeros(32768, np.int64)
    for (r, g, b), n in cells.items():
        count[r << 10 | g << 5 | b] = n
    return count


def boxes(count, colors):
    box, nb = M.median_cut(count, colors)
    return {(c >> 10, c >> 5 & 31, c & 31): int(box[c]) for c in np.nonzero(count)[0]}, nb


def test_population_tie_goes_to_the_lowest_box():
    # the first cut leaves boxes 0 and 1 with 10 pixels and two cells each: box 0 is cut next
    got, nb = boxes(hist({(0, 0, 0): 5, (1, 0, 0): 5, (30, 0, 0): 5, (31, 0, 0): 5}), 3)
    assert nb == 3 and got == {(0, 0, 0): 0, (1, 0, 0): 2, (30, 0, 0): 1, (31, 0, 0): 1}


def test_axis_tie_goes_to_r_then_g_then_b():
    got, nb = boxes(hist({(0, 0, 0): 1, (4, 4, 4): 1}), 2)
    assert nb == 2 and got == {(0, 0, 0): 0, (4, 4, 4): 1}
    got, _ = boxes(hist({(0, 0, 9): 1, (8, 0, 0): 1, (0, 8, 0): 1, (0, 8, 9): 1}), 2)      # extents 8, 8, 9: blue
    assert got == {(0, 0, 9): 1, (8, 0, 0): 0, (0, 8, 0): 0, (0, 8, 9): 1}
    got, _ = boxes(hist({(0, 0, 0): 1, (8, 0, 8): 1, (0, 8, 0): 1, (0, 8, 8): 1}), 2)      # extents 8, 8, 8: red
    assert got == {(0, 0, 0): 0, (8, 0, 8): 1, (0, 8, 0): 0, (0, 8, 8): 0}
    got, _ = boxes(hist({(3, 0, 0): 1, (3, 8, 8): 1, (3, 8, 0): 1, (4, 0, 0): 1}), 2)      # extents 1, 8, 8: green
    assert got == {(3, 0, 0): 0, (3, 8, 8): 1, (3, 8, 0): 1, (4, 0, 0): 0}


def test_cut_is_clamped_below_the_maximum():
    # the cell at the maximum holds more than half: c would be the maximum, and the upper box empty
    got, nb = boxes(hist({(2, 0, 0): 1, (5, 0, 0): 1, (9, 0, 0): 100}), 2)
    assert nb == 2 and got == {(2, 0, 0): 0, (5, 0, 0): 0, (9, 0, 0): 1}
    # and where the minimum holds more than half, c is the minimum itself
    got, nb = boxes(hist({(2, 0, 0): 100, (5, 0, 0): 1, (9, 0, 0): 1}), 2)
    assert got == {(2, 0, 0): 0, (5, 0, 0): 1, (9, 0, 0): 1}
    # 2 * cum >= pop: exactly half stays below
    got, nb = boxes(hist({(2, 0, 0): 3, (5, 0, 0): 1, (9, 0, 0): 2}), 2)
    assert got == {(2, 0, 0): 0, (5, 0, 0): 1, (9, 0, 0): 1}


def test_cut_stops_when_no_box_can_be_split():
    count = hist({(1, 2, 3): 7, (1, 2, 4): 1, (20, 2, 3): 2})
    got, nb = boxes(count, 256)
    assert nb == 3 and sorted(got.values()) == [0, 1, 2]
    sums = np.zeros((32768, 3), np.int64)
    for c in np.nonzero(count)[0]:
        sums[c] = count[c] * np.array([8 * (c >> 10) + 1, 8 * (c >> 5 & 31) + 7, 8 * (c & 31) + 2])
    box, nb = M.median_cut(count, 256)
    pal = M.palette_of(count, sums, box, nb)
    assert not pal[3:].any() and sorted(map(tuple, pal[:3].tolist())) == [(9, 23, 26), (9, 23, 34), (161, 23, 26)]
    lut = M.lookup(count, sums, pal, nb)
    assert lut.max() < 3 and all(lut[c] == box[c] for c in np.nonzero(count)[0])
    got, nb = boxes(hist({(1, 2, 3): 7}), 256)
    assert nb == 1 and got == {(1, 2, 3): 0}


def test_palette_rounds_and_lookup_takes_the_lowest_on_a_tie():
    count = hist({(0, 0, 0): 3})
    sums = np.zeros((32768, 3), np.int64)
    sums[0] = (1 + 2 + 2, 7 + 7 + 6, 0)                   # means 5 / 3 and 20 / 3: 2 and 7
    box, nb = M.median_cut(count, 256)
    assert M.palette_of(count, sums, box, nb)[0].tolist() == [2, 7, 0]
    pal = np.zeros((256, 3), np.uint8)
    pal[0], pal[1], pal[2] = (0, 4, 4), (8, 4, 4), (200, 200, 200)
    lut = M.lookup(np.zeros(32768, np.int64), np.zeros((32768, 3), np.int64), pal, 3)
    assert lut[0] == 0 and lut[1 << 10] == 1              # the first cell's centre (4, 4, 4) is as far from entry 0 as from entry 1
    assert lut[31 << 10 | 31 << 5 | 31] == 2


def test_dither():
    grey = np.full((8, 16, 3), 128, np.uint8)
    d0 = M.dithered(grey, 0)
    assert np.array_equal(d0, grey)
    d8 = M.dithered(grey, 8)[:, :, 0] - 128
    assert d8.min() == (-63 * 8) >> 7 == -4 and d8.max() == (63 * 8) >> 7 == 3 and np.array_equal(d8[:, :8], d8[:, 8:])
    assert d8[0, 0] == (-63 * 8) >> 7 and d8[0, 1] == ((2 * 32 + 1 - 64) * 8) >> 7 and d8[7, 0] == ((2 * 63 + 1 - 64) * 8) >> 7
    assert M.dithered(np.zeros((8, 8, 3), np.uint8), 64).min() == 0 and M.dithered(np.full((8, 8, 3), 255, np.uint8), 64).max() == 255
    assert M.dithered(np.full((8, 8, 3), 100, np.uint8), 64)[0, 0, 0] == 100 + ((-63 * 64) >> 7) == 68


# ------------------------------------------------------------------ the file around the blocks
class _Record(object):
    """A host frame as the device leaves it: the record, then the block."""

    @staticmethod
    def of(block, status=0):
        return np.frombuffer(np.array([len(block), status, M.SEG, 0], '<u4').tobytes() + block + b'\xa5' * 40, np.uint8)


def some_blocks(n, w=16, h=8):
    return [M.frame_block(GC.noise(w, h, 50 + k)) for k in range(n)]


@pytest.mark.parametrize('fps', (24, 30, 50))
def test_mux_counts_loops_and_delays(fps):
    blocks = some_blocks(7)
    out = encoders.GIFOutput(fps=fps, loop=5)
    for b in blocks:
        assert out.encode(_Record.of(b)) == ({}, [])
    media, logs = out.encode(None)
    assert list(media) == ['.gif'] and logs == []
    data = media['.gif'].read()
    assert data == M.gif_file(16, 8, blocks, fps=fps, loop=5)
    assert data[:6] == b'GIF89a' and data[6:13] == struct.pack('<HH', 16, 8) + b'\x70\x00\x00' and data[-1:] == b'\x3b'
    assert data[13:32] == b'\x21\xff\x0bNETSCAPE2.0\x03\x01\x05\x00\x00' and data[32:36] == b'\x21\xf9\x04\x04'
    want = [int(round(100.0 * (k + 1) / fps)) - int(round(100.0 * k / fps)) for k in range(7)]
    assert want == encoders.gif_delays(7, fps) == M.delays(7, fps) and min(want) >= 2
    assert abs(sum(want) - 700.0 / fps) <= 0.5
    size, frames = frames_of(data)
    assert size == (16, 8) and len(frames) == 7
    for k, (got, info) in enumerate(frames):
        assert info['loop'] == 5 and info['duration'] == 10 * want[k]
        _, _, pal, idx = M.decode_block(blocks[k])
        assert np.array_equal(got, pal[idx])
    assert out.encode(None) == ({}, [])


def test_mux_refuses_rates_above_50():
    for fps in (60, 50.5, 100):
        with pytest.raises(ValueError, match='fps'):
            encoders.GIFOutput(fps=fps)
    encoders.GIFOutput(fps=50)
    with pytest.raises(ValueError, match='fps'):
        encoders.GIFOutput(fps=0)


def test_mux_starts_a_new_file_when_the_size_changes():
    a, b = some_blocks(2, 16, 8), some_blocks(2, 8, 16)
    out = encoders.GIFOutput(fps=25)
    assert out.encode(_Record.of(a[0])) == ({}, []) and out.encode(_Record.of(a[1])) == ({}, [])
    media, _ = out.encode(_Record.of(b[0]))
    assert media['.gif'].read() == M.gif_file(16, 8, a, fps=25)
    assert out.encode(_Record.of(b[1])) == ({}, [])
    media, _ = out.encode(None)
    assert media['.gif'].read() == M.gif_file(8, 16, b, fps=25)        # (the delays start over with the file)
    with pytest.raises(_lib.FlameError, match='needs'):
        out.encode(_Record.of(a[0], status=1))
    with pytest.raises(IOError):
        out.encode(_Record.of(b'\x21' + a[0][1:]))
    out.abort()
    assert out.encode(None) == ({}, [])


def test_one_frame_file():
    blk = some_blocks(1)
    out = encoders.GIFOutput()
    out.encode(_Record.of(blk[0]))
    data = out.encode(None)[0]['.gif'].read()
    assert data == M.gif_file(16, 8, blk, fps=24) and frames_of(data)[1][0][1]['duration'] == 40


class StubLib(object):
    def __init__(self):
        self.calls = []

    def fl_gif_bound(self, w, h):
        self.calls.append(('fl_gif_bound', w, h))
        return M.bound(w, h)

    def fl_output_gif(self, ctx, w, h, colors, amp, host, dev, cap):
        self.calls.append(('fl_output_gif', ctx, w, h, colors, amp, host, dev, cap))
        return 0

    def fl_last_error(self):
        return b''


class StubFB(object):
    ctx = 1234

    def host_buffer(self, shape, dtype):
        self.last = np.zeros(shape, dtype)
        return self.last


def test_output_calls_the_library(monkeypatch):
    stub = StubLib()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    dim = render.Framebuffers.calc_dim(64, 48)
    cap = M.bound(64, 48)
    for kw, args in ((dict(), (256, 8)), (dict(colors=16, dither='none'), (16, 0)), (dict(colors=2, dither='ordered', loop=3), (2, 8))):
        out = encoders.GIFOutput(**kw)
        assert isinstance(out, output.DeviceEncodedOutput) and (out.suffix, out.entry) == ('.gif', 'fl_output_gif')
        assert out.shape(dim) == (cap,) and np.dtype(out.dtype) == np.uint8
        fb = StubFB()
        buf = out.copy(fb, dim)
        assert buf is fb.last and stub.calls[-1] == ('fl_output_gif', 1234, 64, 48) + args + (buf.ctypes.data, 0, cap)


def test_output_options():
    for bad in (dict(colors=1), dict(colors=257), dict(colors=True), dict(colors=16.0), dict(colors='16'), dict(dither='bayer'), dict(dither=True),
                dict(dither=None), dict(dither=8), dict(loop=-1), dict(loop=65536), dict(loop=True), dict(loop='0')):
        with pytest.raises(ValueError):
            encoders.GIFOutput(**bad)
    for bad in (dict(alpha=True), dict(quality=90)):
        with pytest.raises(TypeError):
            encoders.GIFOutput(**bad)


# ------------------------------------------------------------------ the profile keys and the command line
def test_profile_keys():
    gnm, prof = configs.cfg2()

    def out_for(block, **over):
        return output.get_output_for_profile(profile.wrap(dict(prof, output=block, **over), gnm))

    dev = out_for({'type': 'gif'})
    assert type(dev) is encoders.GIFOutput and (dev.colors, dev.dither, dev.loop, dev.fps) == (256, 'ordered', 0, profile.wrap(prof, gnm).fps)
    dev = out_for({'type': 'gif', 'colors': 64, 'dither': 'none', 'loop': 2}, fps=30)
    assert (dev.colors, dev.dither, dev.loop, dev.fps) == (64, 'none', 2, 30)
    for key, value in (('alpha', True), ('alpha', False), ('quality', 90), ('bits', 8), ('filter', 'paeth'), ('compression', 'deflate'), ('device', True),
                       ('encoder', 'device'), ('optimize', True), ('sampling', '420'), ('crf', 10), ('pix_fmt', 'yuv420p')):
        with pytest.raises(ValueError, match=key):
            out_for({'type': 'gif', key: value})
    with pytest.raises(ValueError, match='pixel'):
        out_for({'type': 'gif', 'pixel': 'half'})
    for block in ({'type': 'gif', 'colors': 1}, {'type': 'gif', 'colors': 300}, {'type': 'gif', 'colors': '16'}):
        with pytest.raises(ValueError, match=r'output\.colors'):
            out_for(block)
    with pytest.raises(ValueError, match=r'output\.dither'):
        out_for({'type': 'gif', 'dither': 'floyd'})
    with pytest.raises(ValueError, match=r'output\.loop'):
        out_for({'type': 'gif', 'loop': 70000})
    with pytest.raises(ValueError, match='fps'):
        out_for({'type': 'gif'}, fps=60)
    # the three keys on every other type
    others = ({'type': 'jpeg'}, {}, {'type': 'jpeg', 'device': True}, {'type': 'png'}, {'type': 'png', 'encoder': 'device'}, {'type': 'tiff'},
              {'type': 'tiff', 'compression': 'deflate'}, {'type': 'exr'}, {'type': 'raw'}, {'type': 'raw16'}, {'type': 'mjpeg'}, {'type': 'x264'},
              {'type': 'vp9'}, {'type': 'vp8'}, {'type': 'prores'})
    for block in others:
        for key, value in (('colors', 256), ('dither', 'ordered'), ('loop', 0)):
            with pytest.raises(ValueError, match=key):
                out_for(dict(block, **{key: value}))
    assert output.get_suffix('gif') == '.gif' and 'gif' in output._VIDEO
    assert output.get_suffix_for_profile(profile.wrap(dict(prof, output={'type': 'gif', 'colors': 16}), gnm)) == '.gif'
    # nothing else moved
    assert type(out_for({'type': 'mjpeg'})) is encoders.MJPEGOutput and type(out_for({'type': 'exr'})) is output.DeviceEXROutput
    assert type(out_for({'type': 'png', 'encoder': 'device'})) is output.DevicePNGOutput and type(out_for({})) is output.PILOutput


def test_command_line_options():
    parser = profile.add_args(argparse.ArgumentParser())

    def out_of(*argv):
        return profile.get_from_args(parser.parse_args(list(argv)))[1].get('output')

    assert out_of('--codec', 'gif') == {'type': 'gif'}
    assert out_of('--codec', 'gif', '--gif-colors', '64', '--gif-dither', 'none') == {'type': 'gif', 'colors': 64, 'dither': 'none'}
    assert out_of('--gif-colors', '16') == {'colors': 16}                                     # (no gif: the output factory refuses it)
    for argv in (('--gif-dither', 'bayer'), ('--gif-colors', 'many'), ('--gif-colors',), ('--codec', 'GIF')):
        with pytest.raises(SystemExit):
            parser.parse_args(list(argv))
    gnm, _ = configs.cfg2()

    def out_for(*argv):
        return output.get_output_for_profile(profile.wrap(profile.get_from_args(parser.parse_args(list(argv)))[1], gnm))

    dev = out_for('--codec', 'gif', '--fps', '25')
    assert type(dev) is encoders.GIFOutput and (dev.colors, dev.dither, dev.fps) == (256, 'ordered', 25)
    assert out_for('--codec', 'gif', '--gif-colors', '32', '--still').colors == 32
    with pytest.raises(ValueError, match=r'output\.colors'):
        out_for('--gif-colors', '16')
    with pytest.raises(ValueError, match=r'output\.colors'):
        out_for('--codec', 'gif', '--gif-colors', '1000')
    with pytest.raises(ValueError, match='fps'):
        out_for('--codec', 'gif', '--fps', '60')
    for extra in (('--device-encode',), ('--quality', '90'), ('--bits', '16'), ('--tiff-compression', 'deflate'), ('--png-filter', 'adaptive'), ('--optimize',),
                  ('--exr-pixel', 'half')):
        with pytest.raises(ValueError):
            out_for('--codec', 'gif', *extra)


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_gif_bound', 'fl_gif_encode', 'fl_output_gif'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert re.search(r'#define\s+FL_GIF_HEADER_BYTES\s+779\b', code) and _lib.GIF_HEADER_BYTES == 779 == M.HEADER_BYTES
    assert _lib.GIF_DITHER == {'none': 0, 'ordered': 8}
    assert lib.fl_abi_version() == 1
    assert lib.fl_gif_encode(None, 8, 8, 1, 256, 8, 1, 0, 4096) == _lib.FL_E_INVAL      # (a null context: refused before the device is touched)
    assert lib.fl_output_gif(None, 8, 8, 256, 8, 1, 0, 4096) == _lib.FL_E_INVAL
    assert 'gif.hip' in open(os.path.join(REPO, 'cuburn_amd', 'csrc', 'Makefile')).read()


def test_bound(built):
    lib = _lib.load()
    for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536), (4097, 4096), (65535, 257), (65535, 65535)):
        assert lib.fl_gif_bound(w, h) == 0 == M.bound(w, h), (w, h)
    for w, h in ((1, 1), (7, 3), (32, 32), (41, 25), (1920, 1080), (65535, 1), (1, 65535), (65535, 256), (4096, 4096)):
        assert lib.fl_gif_bound(w, h) == M.bound(w, h) > 16 + M.HEADER_BYTES, (w, h)
    # no block is longer at any segment length: a frame of noise whose every pixel costs a code
    rs = np.random.RandomState(8)
    idx = rs.randint(0, 256, 5000).astype(np.uint8)
    pal = rs.randint(0, 256, (256, 3)).astype(np.uint8)
    for seg in (256, 1024, 3584):
        assert 16 + len(M.block_of(5000, 1, pal, idx, seg)) <= M.bound(5000, 1)


# ------------------------------------------------------------------ the definition's quality
def test_quality_against_pillow_s_median_cut():
    """On the flame-like picture the undithered mean squared error is at most 1.1 times that of Pillow's own median cut.  A
    condition on the definition, not on the device."""
    frame = GC.flame_like()
    assert frame.shape == (180, 320, 4)
    rgb = frame[:, :, :3].astype(np.int64)
    pal, idx, nb = M.quantise(frame, 256, 0)
    ours = float(((pal[idx].astype(np.int64) - rgb) ** 2).mean())
    pil = PIL_Image.fromarray(frame[:, :, :3]).quantize(256, PIL_Image.Quantize.MEDIANCUT, dither=PIL_Image.Dither.NONE).convert('RGB')
    theirs = float(((np.asarray(pil).astype(np.int64) - rgb) ** 2).mean())
    print('mean squared error: the definition %.3f, Pillow %.3f, ratio %.3f' % (ours, theirs, ours / theirs))
    assert nb == 256 and ours <= 1.1 * theirs
