"""
CPU tests of the 4:2:0 form of the device JPEG output and of the Motion-JPEG output (no GPU): the numpy model of
tests/jpeg420_model.py against Pillow and against itself on every case of tests/jpeg420_cases.py, MJPEGOutput's AVI files against
the model's reader with a stand-in library, the profile / command-line plumbing, and the host side of the C ABI.
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
import jpeg420_cases as JC
import jpeg420_model as M
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
    """Pillow reads the model's files as 4:2:0 with the model's tables, and its Y plane is within 1 level of the model's float64
    decode (libjpeg's integer IDCT, IEEE 1180: the tolerance tests/test_cpu_jpeg.py uses).  Chroma is compared only on frames
    whose Cb and Cr planes are flat: libjpeg upsamples chroma with a triangle filter and the model replicates, so on any other
    frame the two decodes differ by what the filters differ, which says nothing about the stream.  A flat plane is the same
    under both."""
    JpegImagePlugin = pytest.importorskip('PIL.JpegImagePlugin')
    rs = np.random.RandomState(quality)
    for w, h, ri in ((250, 37, 4), (17, 9, 2), (1, 1, 4), (64, 48, 10)):
        planes = rs.randint(0, 256, (3, h, w)).astype(np.uint8)
        smooth = np.clip(planes.astype(np.int64) // 8 + np.arange(w)[None, None, :] * 3 + np.arange(h)[None, :, None], 0, 255).astype(np.uint8)
        flat = planes.copy()
        flat[1], flat[2] = 90, 171
        for p, chroma_too in ((planes, False), (smooth, False), (flat, True)):
            data = M.encode(p, quality, ri)
            im, pil = pillow_ycc(data)
            assert im.size == (w, h)
            assert JpegImagePlugin.get_sampling(im) == 2 and [tuple(l[:3]) for l in im.layer] == [(1, 2, 2), (2, 1, 1), (3, 1, 1)]
            qt = J.quant_tables(quality)
            assert [list(im.quantization[t]) for t in (0, 1)] == [list(qt[t]) for t in (0, 1)]
            mine = M.decode(data).astype(np.int64)
            diff = np.abs(pil[0] - mine[0]).max()
            print('quality %d %dx%d: Pillow vs model decode, Y max %d' % (quality, w, h, diff))
            assert diff <= 1
            if chroma_too:
                assert np.abs(pil[1:] - mine[1:]).max() <= 1


# ------------------------------------------------------------------ the model against itself, on every case
@pytest.mark.parametrize('name', JC.NAMES)
def test_cases_contain_their_edge(name):
    planes, quality, check = JC.case(name, JC.MODEL_RI)
    data = M.encode(planes, quality, JC.MODEL_RI)
    ps = M.parse(data)
    qt = J.quant_tables(quality)
    assert (ps.w, ps.h, ps.restart_interval) == (planes.shape[2], planes.shape[1], JC.MODEL_RI)
    assert np.array_equal(ps.qtables, qt)
    assert np.array_equal(ps.coefficients, M.quantise(M.dct_values(planes), qt))
    assert M.assemble(ps.w, ps.h, ps.qtables, ps.restart_interval, ps.coefficients) == data
    check(ps.stats, JC.MODEL_RI)
    assert sum(ps.stats['interval_bytes']) + 2 * len(ps.stats['rst']) + 2 + M.HEADER_BYTES == len(data)
    with pytest.raises(J.JpegError):
        J.parse(data)                              # the 4:4:4 parser refuses the sampling
    with pytest.raises(J.JpegError):
        M.parse(J.encode(planes, quality, JC.MODEL_RI))


def test_downsample_clamps_before_it_averages():
    p = np.zeros((3, 3, 3), np.uint8)
    p[1] = [[10, 20, 31], [40, 50, 61], [70, 80, 93]]
    y, c = M.downsample(p)
    assert y.shape == (16, 16) and c.shape == (2, 8, 8)
    # the last column and row are replicated first: (31 + 31 + 61 + 61 + 2) >> 2, (70 + 80 + 70 + 80 + 2) >> 2, 93
    assert c[0, 0, 0] == (10 + 20 + 40 + 50 + 2) >> 2 and c[0, 0, 1] == 46 and c[0, 1, 0] == 75 and c[0, 1, 1] == 93
    assert (c[0, 2:, :] == c[0, 1:2, :]).all() and (c[0, :, 2:] == c[0, :, 1:2]).all()


# ------------------------------------------------------------------ MJPEGOutput against a stand-in library
class StubLib(object):
    """Records the calls and hands out the streams it was given, one per call."""

    def __init__(self, streams, status=0):
        self.calls, self.streams, self.status, self.k = [], list(streams), status, 0

    def _answer(self, host):
        if host:
            stream = self.streams[self.k % len(self.streams)]
            self.k += 1
            rec = np.array([len(stream), self.status, 4, 0], '<u4').tobytes() + (b'' if self.status else stream)
            C.memmove(host, rec, len(rec))
        return 0

    def fl_output_jpeg(self, ctx, w, h, quality, host, dev, cap):
        self.calls.append(('fl_output_jpeg', ctx, w, h, quality, host, dev, cap))
        return self._answer(host)

    def fl_output_jpeg_s(self, ctx, w, h, quality, sampling, host, dev, cap):
        self.calls.append(('fl_output_jpeg_s', ctx, w, h, quality, sampling, host, dev, cap))
        return self._answer(host)


class StubFB(object):
    ctx = 1234

    def host_buffer(self, shape, dtype):
        self.last = np.zeros(shape, dtype)         # one buffer per frame here; the real ring reuses them
        return self.last


@pytest.fixture(scope='module')
def frames():
    """Five 24 x 16 files of the model, at least one of odd and one of even length."""
    out = [M.encode(np.random.RandomState(s).randint(0, 256, (3, 16, 24)).astype(np.uint8), 60, 4) for s in range(5)]
    if len(out[0]) % 2 == 0:                       # the one-frame file is the odd one
        out.sort(key=lambda d: -(len(d) % 2))
    assert len(out[0]) % 2 == 1 and any(len(d) % 2 == 0 for d in out)
    return out


@pytest.mark.parametrize('fps,rate,scale', [(24, 24, 1), (29.97, 2997, 100)])
@pytest.mark.parametrize('nframes', (1, 2, 5))
def test_avi_writer(monkeypatch, frames, nframes, fps, rate, scale):
    stub = StubLib(frames[:nframes])
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    out = encoders.MJPEGOutput(fps=fps, quality=60)
    dim = render.Framebuffers.calc_dim(24, 16)
    fb = StubFB()
    for k in range(nframes):
        buf = out.copy(fb, dim)
        assert stub.calls[-1] == ('fl_output_jpeg_s', 1234, 24, 16, 60, 1, buf.ctypes.data, 0, out.capacity(dim))
        assert out.encode(buf) == ({}, [])
        buf[:] = 0xEE                              # the frame buffer is reused: the writer must have copied the bytes out
    media, logs = out.encode(None)
    assert list(media) == ['.avi'] and logs == []
    data = media['.avi'].read()
    avi = M.read_avi(data)
    assert avi.chunks == frames[:nframes]
    assert avi.avih['dwTotalFrames'] == avi.strh['dwLength'] == nframes
    assert (avi.strh['dwRate'], avi.strh['dwScale']) == (rate, scale)
    assert avi.avih['dwMicroSecPerFrame'] == int(round(1e6 / fps))
    assert (avi.avih['dwWidth'], avi.avih['dwHeight']) == (24, 16) and avi.strf['biSizeImage'] == 24 * 16 * 3
    assert avi.avih['dwSuggestedBufferSize'] == avi.strh['dwSuggestedBufferSize'] == max(len(d) for d in frames[:nframes])
    off = 4
    for (o, n), d in zip(avi.index, frames[:nframes]):
        assert (o, n) == (off, len(d)) and data[220 + o:220 + o + 8] == b'00dc' + len(d).to_bytes(4, 'little')
        off += 8 + len(d) + len(d) % 2
    assert len(data) == 224 + off - 4 + 8 + 16 * nframes and len(data) % 2 == 0
    assert out.encode(None) == ({}, [])            # nothing is left


def test_avi_reader_refuses_broken_files(monkeypatch, frames):
    stub = StubLib(frames[:2])
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    out, fb, dim = encoders.MJPEGOutput(fps=24), StubFB(), render.Framebuffers.calc_dim(24, 16)
    for _ in range(2):
        out.encode(out.copy(fb, dim))
    data = out.encode(None)[0]['.avi'].read()
    M.read_avi(data)
    n0 = len(frames[0])
    for bad in (data[:-1], data + b'\0', data[:48] + b'\x03' + data[49:], data[:224 + 4] + (n0 + 1).to_bytes(4, 'little') + data[232:],
                data[:-8] + (5).to_bytes(4, 'little') + data[-4:], data[:224 + 8 + n0] + b'\x01' + data[224 + 9 + n0:]):
        with pytest.raises(M.AviError):
            M.read_avi(bad)


def test_avi_writer_refuses_a_frame_that_did_not_fit(monkeypatch, frames):
    stub = StubLib(frames[:1], status=1)
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    out, fb, dim = encoders.MJPEGOutput(fps=24), StubFB(), render.Framebuffers.calc_dim(24, 16)
    with pytest.raises(_lib.FlameError, match=str(len(frames[0]))):
        out.encode(out.copy(fb, dim))
    assert out.encode(None) == ({}, [])


def test_avi_writer_two_gib_rule(monkeypatch, frames):
    """The limit patched down to what two frames need less one byte: the second frame raises before anything of it is written,
    and the message names `shard`."""
    stub = StubLib(frames[:2])
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    pad = lambda n: n + n % 2
    two = 224 + sum(8 + pad(len(d)) for d in frames[:2]) + 8 + 32
    monkeypatch.setattr(encoders, 'AVI_MAX_BYTES', two - 1)
    opened = []
    real = encoders.tempfile.TemporaryFile
    monkeypatch.setattr(encoders.tempfile, 'TemporaryFile', lambda *a, **k: opened.append(real(*a, **k)) or opened[-1])
    out, fb, dim = encoders.MJPEGOutput(fps=24), StubFB(), render.Framebuffers.calc_dim(24, 16)
    out.encode(out.copy(fb, dim))
    size = opened[0].tell()
    with pytest.raises(IOError, match='shard'):
        out.encode(out.copy(fb, dim))
    assert len(opened) == 1 and opened[0].tell() == size
    # ... and a first frame that is too large alone opens no file
    out.abort()
    assert opened[0].closed
    monkeypatch.setattr(encoders, 'AVI_MAX_BYTES', 224 + 8 + pad(len(frames[0])) + 8 + 16 - 1)
    with pytest.raises(IOError, match='shard'):
        out.encode(out.copy(fb, dim))
    assert len(opened) == 1
    monkeypatch.setattr(encoders, 'AVI_MAX_BYTES', 224 + 8 + pad(len(frames[0])) + 8 + 16)
    stub.k = 0
    out.encode(out.copy(fb, dim))
    assert len(M.read_avi(out.encode(None)[0]['.avi'].read()).chunks) == 1


def test_avi_writer_abort_and_size_change(monkeypatch, frames):
    other = M.encode(np.zeros((3, 8, 40), np.uint8), 60, 4)
    stub = StubLib([frames[0], frames[1], other])
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    opened = []
    real = encoders.tempfile.TemporaryFile
    monkeypatch.setattr(encoders.tempfile, 'TemporaryFile', lambda *a, **k: opened.append(real(*a, **k)) or opened[-1])
    out, fb, dim = encoders.MJPEGOutput(fps=24), StubFB(), render.Framebuffers.calc_dim(24, 16)
    assert out.encode(out.copy(fb, dim)) == ({}, []) and out.encode(out.copy(fb, dim)) == ({}, [])
    media, _ = out.encode(out.copy(fb, dim))       # a frame of another size: the file so far comes back, a new one starts
    first = M.read_avi(media['.avi'].read())
    assert first.chunks == frames[:2] and first.avih['dwWidth'] == 24
    out.abort()                                    # drops the second file
    assert len(opened) == 2 and opened[1].closed
    assert out.encode(None) == ({}, [])
    out.abort()                                    # (and may be called with nothing open)


# ------------------------------------------------------------------ profile and command line
def _out_for(block, **prof_keys):
    gnm, prof = configs.cfg2()
    return output.get_output_for_profile(profile.wrap(dict(prof, output=block, **prof_keys), gnm))


def test_profile_selects_the_outputs():
    mj = _out_for({'type': 'mjpeg'}, fps=30)
    assert type(mj) is encoders.MJPEGOutput and isinstance(mj, output.DeviceEncodedOutput)
    assert (mj.fps, mj.quality, mj.sampling, mj.suffix) == (30, 90, '420', '.avi')
    mj = _out_for({'type': 'mjpeg', 'quality': 70, 'sampling': '444'})
    assert (mj.quality, mj.sampling) == (70, '444')
    with pytest.raises(ValueError, match='alpha'):
        _out_for({'type': 'mjpeg', 'alpha': True})
    for block in ({'type': 'mjpeg', 'sampling': '422'}, {'type': 'mjpeg', 'quality': 0}, {'type': 'jpeg', 'device': True, 'sampling': '411'}):
        with pytest.raises(ValueError):
            _out_for(block)
    still = _out_for({'type': 'jpeg', 'device': True, 'sampling': '420', 'quality': 80})
    assert type(still) is output.DeviceJPEGOutput and (still.sampling, still.quality, still.suffix) == ('420', 80, '.jpg')
    assert _out_for({'type': 'jpeg', 'device': True}).sampling == '444'
    gnm, prof = configs.cfg2()
    assert output.get_suffix_for_profile(profile.wrap(dict(prof, output={'type': 'mjpeg'}), gnm)) == '.avi'
    assert output.get_suffix('mjpeg') == '.avi'


def test_sampling_reaches_the_library(monkeypatch):
    stub = StubLib([b'\xff\xd8stream\xff\xd9'])
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    dim, fb = render.Framebuffers.calc_dim(64, 48), StubFB()
    cap = 16 + J.HEADER_BYTES + 2 * 3 * 64 * 48
    # without `sampling`, and with 444: the calls of before, on the entry point of before
    for out in (_out_for({'type': 'jpeg', 'device': True, 'quality': 85}), output.DeviceJPEGOutput(quality=85),
                output.DeviceJPEGOutput(quality=85, sampling='444')):
        buf = out.copy(fb, dim)
        assert stub.calls == [('fl_output_jpeg', 1234, 64, 48, 85, buf.ctypes.data, 0, cap)]
        del stub.calls[:]
    out = _out_for({'type': 'jpeg', 'device': True, 'quality': 85, 'sampling': '420'})
    buf = out.copy(fb, dim)
    assert stub.calls == [('fl_output_jpeg_s', 1234, 64, 48, 85, 1, buf.ctypes.data, 0, cap)]
    media, logs = out.encode(buf)
    assert list(media) == ['.jpg'] and media['.jpg'].read() == stub.streams[0]
    assert out.copy(fb, dim, dev_out=4096, host=False) is None and stub.calls[-1][6:8] == (None, 4096)


def test_command_line_options():
    parser = profile.add_args(argparse.ArgumentParser())
    _, prof = profile.get_from_args(parser.parse_args(['--codec', 'mjpeg', '--quality', '80', '--shard', '10']))
    assert prof['output'] == {'type': 'mjpeg', 'quality': 80} and prof['shard'] == 10
    gnm, _ = configs.cfg2()
    mj = output.get_output_for_profile(profile.wrap(prof, gnm))
    assert type(mj) is encoders.MJPEGOutput and mj.quality == 80
    _, prof = profile.get_from_args(parser.parse_args(['--codec', 'mjpeg']))
    assert prof['output'] == {'type': 'mjpeg'}


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_jpeg_bound_s', 'fl_jpeg_encode_s', 'fl_output_jpeg_s'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert re.search(r'FL_JPEG_444\s*=\s*0\b', code) and re.search(r'FL_JPEG_420\s*=\s*1\b', code)
    assert _lib.JPEG_SAMPLING == {'444': 0, '420': 1}
    assert lib.fl_abi_version() == 1
    for bad in ((None, 16, 16, 1, 50, 1, None, 0, 4096), (None, 16, 16, 1, 50, 1, 1, 0, 4096)):
        assert lib.fl_jpeg_encode_s(*bad) == _lib.FL_E_INVAL          # (a null context: refused before the device is touched)


def test_bound(built):
    lib = _lib.load()
    for w, h in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        assert lib.fl_jpeg_bound(w, h) == 0
        for s in (0, 1):
            assert lib.fl_jpeg_bound_s(w, h, s) == 0
    for s in (-1, 2, 420):
        assert lib.fl_jpeg_bound_s(16, 16, s) == 0
    assert lib.fl_jpeg_bound_s(1, 1, 1) == lib.fl_jpeg_bound_s(16, 16, 1) == 16 + J.HEADER_BYTES + 2492
    assert lib.fl_jpeg_bound_s(17, 16, 1) == 16 + J.HEADER_BYTES + 2 * 2492
    assert lib.fl_jpeg_bound_s(1920, 1080, 1) == 16 + J.HEADER_BYTES + 120 * 68 * 2492
    for w, h in ((1, 1), (8, 8), (17, 9), (1920, 1080), (65535, 65535)):
        assert lib.fl_jpeg_bound_s(w, h, 0) == lib.fl_jpeg_bound(w, h)
    # the worst MCU: six blocks of 22 bits of DC and 63 coefficients of 16 + 10 bits, every byte stuffed, a marker behind it
    assert 2 * -(-6 * (11 + 11 + 63 * 26) // 8) + 2 == 2492
