"""
CPU tests of the APNG output (no GPU): the file that encoders.APNGOutput writes around the device's frame blocks, driven with
blocks made in Python (zlib.compress cut into chunks, zlib.crc32: tests/apng_cases.py).  Pillow opens the files and returns the
frames, the loop count and the exact delays; the 16-bit frames go through the reader of tests/png_ext_model.py one at a time; every
CRC-32 and the run of the sequence numbers are checked; a block out of turn is refused; then the profile keys, the command line,
and the parts of the C ABI that need no device (fl_apng_chunks, fl_apng_bound, the refusals of a null context).
"""
import argparse
import io
import os
import re
import struct
import zlib
from fractions import Fraction

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, encoders, output, profile, render
import apng_cases as A
import png_ext_model as X
import png_model as P

from PIL import Image as PIL_Image


def pixels_of(w, h, bits, k):
    """Frame k: a gradient that moves and some noise, so the stream has dynamic blocks and the frames differ."""
    rs = np.random.RandomState(31 * k + bits)
    top = 256 if bits == 8 else 65536
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 3 + 17 * k) * (top // 256), (y * 5 + x) * (top // 256), (x + y + 40 * k) * (top // 256) + 7, 200 * (top // 256) + x], axis=2)
    img = img + rs.randint(0, 4 if bits == 8 else 1000, img.shape)
    return (img % top).astype(np.uint8 if bits == 8 else np.uint16)


def stream_of(pix, ch, bits):
    return zlib.compress(P.filter_rows(X.byte_image(pix, ch, bits), 2), 6)


def write(out, frames, w, h, seg=32768, one_ahead=True):
    """Number and encode the frames as the command line's loop does — frame k + 1 is numbered before frame k is encoded — and flush;
    returns the file's bytes."""
    n = out.chunks(w, h)
    pending, media = None, {}
    for pix in frames:
        seq = out.number(w, h)
        buf = A.host_frame(A.block_from_stream(stream_of(pix, out.channels, out.bits), n, seq), seg, n, slack=9)
        if not one_ahead:
            assert out.encode(buf) == ({}, [])
            continue
        if pending is not None:
            assert out.encode(pending) == ({}, [])
        pending = buf
    if pending is not None:
        assert out.encode(pending) == ({}, [])
    media, logs = out.encode(None)
    assert list(media) == ['.apng'] and logs == []
    assert out.encode(None) == ({}, [])
    return media['.apng'].read()


# ------------------------------------------------------------------ Pillow opens the files
@pytest.mark.parametrize('alpha', (False, True))
@pytest.mark.parametrize('nframes', (1, 2, 5))
@pytest.mark.parametrize('fps, ms', ((24, Fraction(1000, 24)), (30000.0 / 1001.0, Fraction(1001, 30))))
def test_pillow_returns_frames_loop_and_delays(built, alpha, nframes, fps, ms):
    w, h, ch = 120, 100, 4 if alpha else 3                 # 36100 or 48100 filtered bytes: two chunks a frame
    out = encoders.APNGOutput(fps=fps, alpha=alpha, loop=3)
    assert out.chunks(w, h) == 2
    frames = [pixels_of(w, h, 8, k) for k in range(nframes)]
    data = write(out, frames, w, h)
    im = PIL_Image.open(io.BytesIO(data))
    assert im.format == 'PNG' and im.size == (w, h) and im.mode == ('RGBA' if alpha else 'RGB')
    assert getattr(im, 'n_frames', 1) == nframes and im.info['loop'] == 3
    for k in range(nframes):
        im.seek(k)
        assert abs(im.info['duration'] - float(ms)) < 1e-9, (k, im.info['duration'])
        assert np.array_equal(np.asarray(im), frames[k][:, :, :ch]), k
    ap = A.parse_file(data)
    assert (ap.num_frames, ap.num_plays) == (nframes, 3)
    assert all(f[5:7] == ((1, 24) if fps == 24 else (1001, 30000)) for f in ap.fctl)


def test_a_reader_without_animation_sees_frame_0(built):
    """The chunks a plain PNG reader keeps — IHDR, IDAT, IEND — are frame 0's file."""
    w, h = 120, 100
    frames = [pixels_of(w, h, 8, k) for k in range(3)]
    data = write(encoders.APNGOutput(), frames, w, h)
    keep = b''.join(A.chunk(t, b) for t, b in A.read_chunks(data, 8) if t in (b'IHDR', b'IDAT', b'IEND'))
    ps = X.parse(A.SIGNATURE + keep)
    assert np.array_equal(ps.pixels, frames[0][:, :, :3])


# ------------------------------------------------------------------ 16 bits, one frame at a time
@pytest.mark.parametrize('alpha', (False, True))
def test_16_bit_frames(built, alpha):
    w, h, ch = 64, 90, 4 if alpha else 3                   # 34650 or 46170 filtered bytes: two chunks a frame
    out = encoders.APNGOutput(bits=16, alpha=alpha, fps=25)
    assert out.chunks(w, h) == 2
    frames = [pixels_of(w, h, 16, k) for k in range(3)]
    ap = A.parse_file(write(out, frames, w, h))
    assert (ap.w, ap.h, ap.bits, ap.channels, ap.num_frames, ap.num_plays) == (w, h, 16, ch, 3, 0)
    for k in range(3):
        ps = X.parse(A.frame_as_png(ap, k))
        assert ps.bits == 16 and np.array_equal(ps.pixels, frames[k][:, :, :ch]), k
        assert ap.fctl[k][1:] == (w, h, 0, 0, 1, 25, 0, 0)


# ------------------------------------------------------------------ chunks, CRCs, numbers
@pytest.mark.parametrize('nframes', (1, 2, 5))
def test_layout_and_sequence_numbers(built, nframes):
    w, h = 120, 100
    out = encoders.APNGOutput(loop=7)
    n = out.chunks(w, h)
    frames = [pixels_of(w, h, 8, k) for k in range(nframes)]
    data = write(out, frames, w, h)
    ap = A.parse_file(data)                                # (every chunk's length and CRC-32)
    assert ap.tags == [b'IHDR', b'acTL', b'fcTL'] + [b'IDAT'] * n + ([b'fcTL'] + [b'fdAT'] * n) * (nframes - 1) + [b'IEND']
    assert ap.tags.index(b'acTL') < ap.tags.index(b'IDAT')
    assert ap.numbers == list(range(nframes + n * (nframes - 1)))
    assert [f[0] for f in ap.fctl] == [0] + [1 + (k - 1) * (n + 1) for k in range(1, nframes)]
    assert (ap.num_frames, ap.num_plays) == (nframes, 7)
    # a frame's bytes: fcTL, and the stream in n chunks, with 4 bytes of number in each fdAT
    for k in range(nframes):
        assert ap.frame_bytes[k] == 38 + len(stream_of(frames[k], 3, 8)) + 12 * n + (4 * n if k else 0)
    assert len(data) == 8 + 25 + 20 + sum(ap.frame_bytes) + 12
    assert encoders.APNGOutput.first_number(0, n) == A.IDAT_SEQ == _lib.APNG_IDAT
    assert [encoders.APNGOutput.first_number(k, 3) for k in (1, 2, 3)] == [2, 6, 10]


def test_frames_may_arrive_without_the_lookahead(built):
    w, h = 120, 100
    frames = [pixels_of(w, h, 8, k) for k in range(3)]
    assert write(encoders.APNGOutput(), frames, w, h, one_ahead=False) == write(encoders.APNGOutput(), frames, w, h)


def test_a_change_of_size_starts_a_new_file(built):
    out = encoders.APNGOutput()
    a, b = pixels_of(40, 30, 8, 0), pixels_of(30, 40, 8, 1)

    def frame(pix):
        h, w = pix.shape[:2]
        n = out.chunks(w, h)
        return A.host_frame(A.block_from_stream(stream_of(pix, 3, 8), n, out.number(w, h)), 32768, n)

    assert out.encode(frame(a)) == ({}, [])
    assert out.encode(frame(a)) == ({}, [])
    media, _ = out.encode(frame(b))                        # numbered as frame 0 of a new file: IDATs
    first = A.parse_file(media['.apng'].read())
    assert (first.w, first.h, first.num_frames, first.numbers) == (40, 30, 2, [0, 1, 2])
    media, _ = out.encode(None)
    second = A.parse_file(media['.apng'].read())
    assert (second.w, second.h, second.num_frames, second.numbers) == (30, 40, 1, [0])


# ------------------------------------------------------------------ a block out of turn
def blocks_for(out, w, h, nframes):
    n = out.chunks(w, h)
    return n, [stream_of(pixels_of(w, h, 8, k), 3, 8) for k in range(nframes)]


def test_a_wrong_first_number_is_refused(built):
    w, h = 120, 100
    out = encoders.APNGOutput()
    n, z = blocks_for(out, w, h, 2)
    assert (out.number(w, h), out.number(w, h)) == (A.IDAT_SEQ, 2)
    out.encode(A.host_frame(A.block_from_stream(z[0], n, A.IDAT_SEQ), 32768, n))
    with pytest.raises(IOError, match='frame 1 .* fdAT 2;'):
        out.encode(A.host_frame(A.block_from_stream(z[1], n, 2 + n + 1), 32768, n))      # frame 2's numbers in frame 1's place: a gap
    assert out.encode(None) == ({}, [])                    # nothing is left of the file


def test_an_idat_block_in_second_place_is_refused(built):
    w, h = 120, 100
    out = encoders.APNGOutput()
    n, z = blocks_for(out, w, h, 2)
    out.number(w, h), out.number(w, h)
    out.encode(A.host_frame(A.block_from_stream(z[0], n, A.IDAT_SEQ), 32768, n))
    with pytest.raises(IOError, match='fdAT 2'):
        out.encode(A.host_frame(A.block_from_stream(z[1], n, A.IDAT_SEQ), 32768, n))
    assert out.encode(None) == ({}, [])


def test_an_fdat_block_in_first_place_is_refused(built):
    w, h = 120, 100
    out = encoders.APNGOutput()
    n, z = blocks_for(out, w, h, 1)
    out.number(w, h)
    with pytest.raises(IOError, match='IDAT'):
        out.encode(A.host_frame(A.block_from_stream(z[0], n, 2), 32768, n))


def test_a_wrong_chunk_count_is_refused(built):
    w, h = 120, 100
    out = encoders.APNGOutput()
    n, z = blocks_for(out, w, h, 1)
    out.number(w, h)
    with pytest.raises(IOError, match='%d chunks' % n):
        out.encode(A.host_frame(A.block_from_stream(z[0], n + 1, A.IDAT_SEQ), 32768, n + 1))
    out.number(w, h)
    with pytest.raises(IOError):
        out.encode(A.host_frame(A.block_from_stream(z[0], n, A.IDAT_SEQ), 32768, n - 1))     # the chunks are right, the record is not


def test_unnumbered_missing_and_unfitting_frames(built):
    w, h = 120, 100
    out = encoders.APNGOutput()
    n, z = blocks_for(out, w, h, 2)
    good = A.host_frame(A.block_from_stream(z[0], n, A.IDAT_SEQ), 32768, n)
    with pytest.raises(IOError, match='never numbered'):
        out.encode(good)
    out.number(w, h), out.number(w, h)
    out.encode(good)
    with pytest.raises(IOError, match='still to come'):    # the flush while a numbered frame has not arrived
        out.encode(None)
    # after the failure the numbering starts again: the retried job writes a whole file
    frames = [pixels_of(w, h, 8, k) for k in range(2)]
    assert A.parse_file(write(out, frames, w, h)).numbers == list(range(2 + n))
    out.number(w, h)
    with pytest.raises(_lib.FlameError, match='APNG frame block needs'):
        out.encode(A.host_frame(b'', 32768, n, status=1))
    assert out.encode(None) == ({}, [])


def test_abort_starts_the_numbering_again(built):
    w, h = 120, 100
    out = encoders.APNGOutput()
    n, z = blocks_for(out, w, h, 1)
    assert (out.number(w, h), out.number(w, h)) == (A.IDAT_SEQ, 2)
    out.encode(A.host_frame(A.block_from_stream(z[0], n, A.IDAT_SEQ), 32768, n))
    out.abort()
    assert out.number(w, h) == A.IDAT_SEQ
    out.abort()
    assert out.encode(None) == ({}, [])


def test_the_numbers_run_out_before_the_file_does(built):
    w, h = 120, 100
    out = encoders.APNGOutput()
    n = out.chunks(w, h)
    out.number(w, h)
    last = (0xfffffffe - n - 1) // (n + 1) + 1              # the last frame whose numbers fit
    assert encoders.APNGOutput.first_number(last, n) + n - 1 <= 0xfffffffe < encoders.APNGOutput.first_number(last + 1, n) + n - 1
    out._qframes = last
    assert out.number(w, h) == 2 + (last - 1) * (n + 1)
    with pytest.raises(IOError, match='shard'):
        out.number(w, h)


# ------------------------------------------------------------------ copy: the library's call, numbered when queued
class StubLib(object):
    def __init__(self):
        self.calls = []

    def fl_apng_chunks(self, w, h, ch, bits):
        return A.chunks_of(w, h, ch, bits, 32768)

    def fl_apng_bound(self, w, h, ch, bits, flags):
        self.calls.append(('fl_apng_bound', w, h, ch, bits, flags))
        return 5000

    def fl_output_apng(self, *args):
        self.calls.append(('fl_output_apng',) + args)
        return self.rc

    def fl_last_error(self):
        return b'refused'


class StubFB(object):
    ctx = 1234

    def host_buffer(self, shape, dtype):
        self.last = np.zeros(shape, dtype)
        return self.last


def test_copy_numbers_the_frame_when_it_is_queued(monkeypatch):
    stub = StubLib()
    stub.rc = 0
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    dim = render.Framebuffers.calc_dim(120, 100)
    out = encoders.APNGOutput(alpha=True, bits=16, filter='adaptive')      # 96100 filtered bytes: three chunks
    assert isinstance(out, output.DeviceEncodedOutput) and (out.suffix, out.entry) == ('.apng', 'fl_output_apng')
    assert out.shape(dim) == (5000,) and np.dtype(out.dtype) == np.uint8
    fb = StubFB()
    seqs = []
    for _ in range(3):
        buf = out.copy(fb, dim)
        name, ctx, w, h, ch, bits, flags, seq, host, dev, cap = stub.calls[-1]
        assert (name, ctx, w, h, ch, bits, flags, host, dev, cap) == ('fl_output_apng', 1234, 120, 100, 4, 16, 1, buf.ctypes.data, 0, 5000)
        seqs.append(seq)
    assert seqs == [A.IDAT_SEQ, 2, 6]
    stub.rc = _lib.FL_E_INVAL                              # a refused call queues nothing and takes no number
    with pytest.raises(ValueError):
        out.copy(fb, dim)
    stub.rc = 0
    out.copy(fb, dim)
    assert stub.calls[-1][7] == 10 and len(out._queued) == 4
    out.copy(fb, render.Framebuffers.calc_dim(64, 48))     # another size: frame 0 of a new file
    assert stub.calls[-1][7] == A.IDAT_SEQ


# ------------------------------------------------------------------ options, profile keys, command line
def test_output_options():
    for bad in (dict(alpha=1), dict(alpha='yes'), dict(loop=-1), dict(loop=65536), dict(loop=True), dict(loop='0'), dict(loop=1.0),
                dict(bits=12), dict(bits=True), dict(bits='8'), dict(bits=16.0), dict(filter='sub'), dict(filter=None), dict(filter=1)):
        with pytest.raises(ValueError):
            encoders.APNGOutput(**bad)
    for bad in (dict(quality=90), dict(colors=16), dict(pixel='half')):
        with pytest.raises(TypeError):
            encoders.APNGOutput(**bad)


def test_delays_are_exact_fractions():
    assert encoders.apng_delay(24) == (1, 24) and encoders.apng_delay(30000.0 / 1001.0) == (1001, 30000)
    assert encoders.apng_delay(23.976023976023978) == (1001, 24000) and encoders.apng_delay(12.5) == (2, 25)
    assert encoders.apng_delay(0.1) == (10, 1) and encoders.apng_delay(90) == (1, 90)
    assert encoders.APNGOutput(fps=30000.0 / 1001.0).delay == (1001, 30000)
    for fps in (0, -24, 91, 120, 89.999):                   # 89.999 = 89999 / 1000: a delay_den above 65535
        with pytest.raises(ValueError, match='fps'):
            encoders.APNGOutput(fps=fps)
    assert Fraction(89.999).limit_denominator(1001).numerator > 65535
    with pytest.raises(ValueError, match='16 bits'):
        encoders.apng_delay(89.999)
    with pytest.raises(ValueError):
        encoders.apng_delay(0)


def test_profile_keys():
    gnm, prof = configs.cfg2()

    def out_for(block, **over):
        return output.get_output_for_profile(profile.wrap(dict(prof, output=block, **over), gnm))

    dev = out_for({'type': 'apng'})
    assert type(dev) is encoders.APNGOutput
    assert (dev.alpha, dev.channels, dev.bits, dev.filter, dev.loop, dev.fps) == (False, 3, 8, 'paeth', 0, profile.wrap(prof, gnm).fps)
    dev = out_for({'type': 'apng', 'alpha': True, 'bits': 16, 'filter': 'adaptive', 'loop': 2}, fps=60)
    assert (dev.alpha, dev.channels, dev.bits, dev.filter, dev.loop, dev.fps, dev.delay) == (True, 4, 16, 'adaptive', 2, 60, (1, 60))
    assert dev.arguments() == (4, 16, _lib.PNG_ADAPTIVE)
    for key, value in (('quality', 90), ('colors', 16), ('dither', 'none'), ('device', True), ('encoder', 'device'), ('compression', 'deflate'),
                       ('optimize', True), ('sampling', '420'), ('crf', 10), ('pix_fmt', 'yuv420p'), ('lossless', True)):
        with pytest.raises(ValueError, match=key):
            out_for({'type': 'apng', key: value})
    with pytest.raises(ValueError, match='pixel'):
        out_for({'type': 'apng', 'pixel': 'half'})
    for block, what in (({'loop': 70000}, r'output\.loop'), ({'alpha': 'yes'}, r'output\.alpha'), ({'bits': 12}, r'output\.bits'),
                        ({'filter': 'up'}, r'output\.filter')):
        with pytest.raises(ValueError, match=what):
            out_for(dict(block, type='apng'))
    for fps in (0, 91, 89.999):
        with pytest.raises(ValueError, match='fps'):
            out_for({'type': 'apng'}, fps=fps)
    assert output.get_suffix('apng') == '.apng' == output.get_suffix('apng', True) and 'apng' in output._VIDEO
    assert output.get_suffix_for_profile(profile.wrap(dict(prof, output={'type': 'apng', 'alpha': True}), gnm)) == '.apng'
    # the keys of the other types are where they were
    others = ({'type': 'jpeg'}, {}, {'type': 'jpeg', 'device': True}, {'type': 'png'}, {'type': 'png', 'encoder': 'device'}, {'type': 'tiff'},
              {'type': 'tiff', 'compression': 'deflate'}, {'type': 'exr'}, {'type': 'raw'}, {'type': 'raw16'}, {'type': 'mjpeg'}, {'type': 'x264'},
              {'type': 'vp9'}, {'type': 'vp8'}, {'type': 'prores'})
    for block in others:
        with pytest.raises(ValueError, match='loop'):
            out_for(dict(block, loop=0))
        if block != {'type': 'png', 'encoder': 'device'}:
            for key, value in (('bits', 8), ('filter', 'paeth')):
                with pytest.raises(ValueError, match=key):
                    out_for(dict(block, **{key: value}))
    for block in ({'type': 'gif'}, {'type': 'webp'}):
        assert out_for(dict(block, loop=4)).loop == 4
        for key, value in (('bits', 8), ('filter', 'paeth')):
            with pytest.raises(ValueError, match=key):
                out_for(dict(block, **{key: value}))
    dev = out_for({'type': 'png', 'encoder': 'device', 'bits': 16, 'filter': 'adaptive'})
    assert type(dev) is output.DevicePNGOutput and (dev.bits, dev.filter) == (16, 'adaptive')
    assert type(out_for({'type': 'gif'})) is encoders.GIFOutput and type(out_for({'type': 'webp'})) is encoders.WebPOutput
    assert type(out_for({})) is output.PILOutput and output.get_suffix('png', True) == '_color.png'


def test_command_line_options():
    parser = profile.add_args(argparse.ArgumentParser())

    def out_of(*argv):
        return profile.get_from_args(parser.parse_args(list(argv)))[1].get('output')

    assert out_of('--codec', 'apng') == {'type': 'apng'}
    assert out_of('--codec', 'apng', '--bits', '16', '--png-filter', 'adaptive') == {'type': 'apng', 'bits': 16, 'filter': 'adaptive'}
    with pytest.raises(SystemExit):
        parser.parse_args(['--codec', 'APNG'])
    gnm, _ = configs.cfg2()

    def out_for(*argv):
        return output.get_output_for_profile(profile.wrap(profile.get_from_args(parser.parse_args(list(argv)))[1], gnm))

    dev = out_for('--codec', 'apng', '--fps', '25', '--bits', '16', '--png-filter', 'adaptive', '--shard', '2')
    assert type(dev) is encoders.APNGOutput and (dev.alpha, dev.bits, dev.filter, dev.loop, dev.fps) == (False, 16, 'adaptive', 0, 25)
    assert type(out_for('--codec', 'apng', '--still')) is encoders.APNGOutput
    with pytest.raises(ValueError, match='fps'):
        out_for('--codec', 'apng', '--fps', '120')
    for extra in (('--device-encode',), ('--quality', '90'), ('--tiff-compression', 'deflate'), ('--optimize',), ('--exr-pixel', 'half'),
                  ('--gif-colors', '16'), ('--gif-dither', 'none')):
        with pytest.raises(ValueError):
            out_for('--codec', 'apng', *extra)


def test_the_spec_knows_the_type():
    from cuburn_amd.genome import specs
    choices = specs.profile['output']['type'].choices
    assert 'apng' in choices and 'webp' in choices and 'gif' in choices


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_apng_chunks', 'fl_apng_bound', 'fl_apng_encode', 'fl_output_apng'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert re.search(r'FL_APNG_IDAT\s*=\s*0xffffffffu', code) and _lib.APNG_IDAT == 0xffffffff
    assert lib.fl_abi_version() == 1 and re.search(r'#define\s+FL_ABI_VERSION\s+1\b', code)
    # a null context: refused before the device is touched
    assert lib.fl_apng_encode(None, 8, 8, 1, 4, 8, 0, A.IDAT_SEQ, 1, 0, 4096) == _lib.FL_E_INVAL
    assert lib.fl_output_apng(None, 8, 8, 4, 8, 0, 2, 1, 0, 4096) == _lib.FL_E_INVAL


def test_chunks_and_bound(built):
    lib = _lib.load()
    seg, env = 32768, os.environ.get('FLAME_PNG_SEG')         # (as png_segment_bytes reads it)
    if env and 8192 <= int(env) <= 32768:
        seg = int(env) & ~15
    refused = ((0, 8, 4, 8), (8, 0, 4, 8), (65536, 8, 4, 8), (8, 65536, 3, 8), (8, 8, 2, 8), (8, 8, 5, 8), (8, 8, 3, 12), (8, 8, 3, 0),
               (65535, 65535, 3, 8), (9000, 65535, 4, 16))
    for w, h, ch, bits in refused:
        assert lib.fl_png_bound_f(w, h, ch, bits, 0) == 0 == lib.fl_apng_chunks(w, h, ch, bits) == lib.fl_apng_bound(w, h, ch, bits, 0), (w, h, ch, bits)
    assert lib.fl_apng_bound(8, 8, 3, 8, 2) == 0 == lib.fl_png_bound_f(8, 8, 3, 8, 2) and lib.fl_apng_chunks(8, 8, 3, 8) == 1      # an unknown flag
    sizes = ((1, 1), (5, 3), (100, 60), (33, 70), (257, 1), (120, 100), (1920, 1080), (65535, 1), (1, 65535), (9000, 65535), (16384, 16384))
    for w, h in sizes:
        for ch in (3, 4):
            for bits in (8, 16):
                png = lib.fl_png_bound_f(w, h, ch, bits, 0)
                n = lib.fl_apng_chunks(w, h, ch, bits)
                if not png:
                    assert n == 0 == lib.fl_apng_bound(w, h, ch, bits, 0)
                    continue
                assert n == A.chunks_of(w, h, ch, bits, seg) >= 1, (w, h, ch, bits)
                for flags in (0, 1):
                    assert lib.fl_png_bound_f(w, h, ch, bits, flags) == png
                    assert lib.fl_apng_bound(w, h, ch, bits, flags) == png - 33 - 12 + 4 * n, (w, h, ch, bits)
    assert lib.fl_apng_chunks(1920, 1080, 3, 8) == -(-1080 * 5761 // seg)
