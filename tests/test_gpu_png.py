"""
The device PNG encoder (cuburn_amd/csrc/png.hip; fl_png_encode, fl_output_png, DevicePNGOutput) read back by the model of
tests/png_model.py, which tests/test_cpu_png.py holds to zlib and Pillow.  For every frame of tests/png_cases.py:

  A. the file parses — chunk order, every CRC-32, the zlib header, the Adler-32 — and the model's pixels and Pillow's equal the
     source at the chosen channel count, every one of them: the format is lossless.  zlib inflates the concatenated IDATs to the
     same filtered bytes;
  B. the case's own check passes with the record's segment length; every match has distance 1 and lies inside its segment; every
     segment is one IDAT, starts on a byte boundary and, but for the last, ends on one; only the last block is final; a dynamic
     segment is smaller than its stored form; no code is longer than 15 bits (7 in the code-length code);
  C. a second encode gives the same bytes, record + file stay within fl_png_bound, and the bytes are the ones the model's own
     writer of the format produces (the same tokens, the same tie-breaks in the length-limited codes).

Then the capacity rule, bad arguments, pageable and device destinations, fl_output_png against fl_output(FL_OUT_RGBA8), and the
path through the shim.
"""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

from cuburn_amd import _lib, configs, output, profile, render
import encoder_harness as H
from encoder_harness import SENTINEL, SLACK, record, upload
import png_cases as PC
import png_model as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
    m.fb.free()


def encode(mgr, rgba, ch, cap=None, buf=None):
    """fl_png_encode into pinned memory (or `buf`) pre-filled with the sentinel; returns (buffer, cap)."""
    h, w, _ = rgba.shape
    if cap is None:
        cap = _lib.load().fl_png_bound(w, h, ch)
    return H.encode(mgr, 'fl_png_encode', rgba, w, h, (ch,), cap, buf)              # (checks the sentinel at and beyond cap)


def file_of(buf):
    nbytes, status, seg = record(buf)
    assert status == 0
    return bytes(buf[16:16 + nbytes])


@pytest.fixture(scope='module')
def device_seg(mgr):
    """The library's segment length, from the record of a one-pixel frame."""
    buf, _ = encode(mgr, np.zeros((1, 1, 4), np.uint8), 3)
    seg = record(buf)[2]
    assert 256 <= seg <= 65535
    return seg


_done = {}


def encoded_case(mgr, name, seg):
    """(rgba, channels, check, file, buffer) of a case, encoded once per session."""
    if name not in _done:
        rgba, ch, check = PC.case(name, seg)
        buf, _ = encode(mgr, rgba, ch)
        _done[name] = (rgba, ch, check, file_of(buf), buf)
    return _done[name]


def assert_criteria(data, rgba, ch, seg):
    """A and B for a file; returns the parse and its statistics."""
    want = rgba[:, :, :ch]
    ps = P.parse(data, seg)                                                         # A
    assert (ps.w, ps.h, ps.channels) == (rgba.shape[1], rgba.shape[0], ch)
    assert np.array_equal(ps.pixels, want), '%d pixels differ' % int((ps.pixels != want).any(axis=2).sum())
    assert zlib.decompress(ps.zstream) == ps.filtered
    try:
        import PIL.Image
    except ImportError:
        pass
    else:
        im = PIL.Image.open(io.BytesIO(data))
        assert im.size == (ps.w, ps.h) and im.mode == ('RGB' if ch == 3 else 'RGBA')
        assert np.array_equal(np.asarray(im), want)
    st = PC.stats_of(ps, seg)                                                       # B
    assert all(0 <= f <= 4 for f in st['filters'])
    assert st['distances'] in ([], [1]) and set(st['block_types']) <= {0, 2}
    assert st['finals'] == [0] * (len(st['finals']) - 1) + [1]
    assert st['nidat'] == len(st['segments']) == -(-st['nfiltered'] // seg)
    for k, (s, body) in enumerate(zip(st['segments'], ps.idat)):
        last = k + 1 == len(st['segments'])
        assert s['start_aligned'] and (last or s['aligned'])
        coded = len(body) - (2 if k == 0 else 0) - (4 if last else 0)
        assert 8 * coded == (s['bits'] + 7) // 8 * 8                                # one IDAT per segment: its bytes are the segment's
        assert s['stored'] or (s['dynamic'] and coded < s['nbytes'] + 5)
        assert not s['stored'] or coded == s['nbytes'] + 5
    for b in st['blocks']:
        if b['type'] == 2:
            assert b['max_lit_len'] <= 15 and b['max_dist_len'] <= 1 and b['max_cl_len'] <= 7 and b['lit_complete'] and b['cl_complete']
    return ps, st


@pytest.mark.parametrize('name', PC.NAMES)
def test_cases(mgr, device_seg, name):
    rgba, ch, check, data, buf = encoded_case(mgr, name, device_seg)
    assert record(buf)[2] == device_seg
    ps, st = assert_criteria(data, rgba, ch, device_seg)
    print('%s: %d x %d x %d, file %d bytes of %d raw, blocks %s' % (name, ps.w, ps.h, ch, len(data), st['raw_bytes'], st['block_types']))
    check(st, device_seg)
    again, _ = encode(mgr, rgba, ch)                                                 # C
    assert file_of(again) == data
    assert 16 + len(data) <= _lib.load().fl_png_bound(ps.w, ps.h, ch) == PC.bound(ps.w, ps.h, ch, device_seg)
    assert P.encode(rgba[:, :, :ch], device_seg) == data


def test_capacity(mgr, device_seg):
    rgba, ch, _, data, _ = encoded_case(mgr, PC.NOISE, device_seg)
    need = len(data)
    for cap in (16 + need - 1, 16 + P.HEADER_BYTES, 16 + need - 1000):
        buf, cap = encode(mgr, rgba, ch, cap=cap)                                    # (checks the sentinel at and beyond cap)
        assert record(buf) == (need, 1, device_seg)
    buf, cap = encode(mgr, rgba, ch, cap=16 + need)
    assert record(buf) == (need, 0, device_seg) and file_of(buf) == data


def test_bound(mgr, device_seg):
    lib = _lib.load()
    for w, h, ch in ((0, 8, 3), (8, 0, 3), (65536, 8, 3), (8, 65536, 3), (8, 8, 1), (8, 8, 5), (65535, 65535, 4)):
        assert lib.fl_png_bound(w, h, ch) == 0
    for w, h, ch in ((1, 1, 3), (1920, 1080, 3), (1920, 1080, 4), (8000, 65535, 4)):
        assert lib.fl_png_bound(w, h, ch) == PC.bound(w, h, ch, device_seg)


def test_bad_arguments(mgr, device_seg):
    lib = _lib.load()
    rgba, ch, _, data, _ = encoded_case(mgr, PC.NOISE, device_seg)
    h, w, _ = rgba.shape
    t = upload(mgr, rgba)
    cap = lib.fl_png_bound(w, h, ch)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    ctx, src, dst = mgr.fb.ctx, t.data_ptr(), buf.ctypes.data
    bad = [(w, h, src, 0, dst, 0, cap), (w, h, src, 2, dst, 0, cap), (w, h, src, 5, dst, 0, cap), (w, h, src, -3, dst, 0, cap),
           (0, h, src, ch, dst, 0, cap), (w, 0, src, ch, dst, 0, cap), (65536, h, src, ch, dst, 0, cap),
           (w, 65536, src, ch, dst, 0, cap), (65535, 65535, src, ch, dst, 0, cap), (w, h, 0, ch, dst, 0, cap),
           (w, h, src, ch, dst, 0, 16 + P.HEADER_BYTES - 1), (w, h, src, ch, None, 0, cap)]
    for args in bad:
        assert lib.fl_png_encode(ctx, *args) == _lib.FL_E_INVAL, args
        assert lib.fl_last_error()
    for args in bad:
        if args[2]:
            assert lib.fl_output_png(ctx, *(args[:2] + args[3:])) == _lib.FL_E_INVAL, args
    _lib.check(lib.fl_ctx_sync(ctx))
    assert (buf == SENTINEL).all()
    good, _ = encode(mgr, rgba, ch)
    assert file_of(good) == data


def test_pageable_memory(mgr, device_seg):
    """A destination that is not pinned receives a copy; the bytes are the same."""
    rgba, ch, _, data, _ = encoded_case(mgr, PC.NOISE, device_seg)
    cap = _lib.load().fl_png_bound(rgba.shape[1], rgba.shape[0], ch)
    buf, _ = encode(mgr, rgba, ch, buf=np.empty(cap + SLACK, np.uint8))
    assert file_of(buf) == data
    buf, _ = encode(mgr, rgba, ch, cap=16 + len(data) - 1, buf=np.empty(16 + len(data) + SLACK, np.uint8))
    assert record(buf) == (len(data), 1, device_seg)


def test_device_destination(mgr, device_seg):
    import torch
    lib = _lib.load()
    rgba, ch, _, data, _ = encoded_case(mgr, 'smooth_256x96', device_seg)
    h, w, _ = rgba.shape
    cap = 16 + len(data) + 7
    t = upload(mgr, rgba)
    for odd in (1, 2, 3):
        out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device=t.device)
        torch.cuda.synchronize(mgr.fb.device)
        host = mgr.fb._pinned((cap + SLACK,), 'u1')
        host[:] = SENTINEL
        _lib.check(lib.fl_png_encode(mgr.fb.ctx, w, h, t.data_ptr(), ch, host.ctypes.data, out.data_ptr() + odd, cap))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        dev = out.cpu().numpy()
        assert (dev[:odd] == SENTINEL).all() and (dev[odd + cap:] == SENTINEL).all() and (host[cap:] == SENTINEL).all()
        assert file_of(dev[odd:]) == data and file_of(host) == data


def test_whole_path(mgr, device_seg):
    """fl_output_png = fl_output(FL_OUT_RGBA8) + the encode: same pixels, same dither states afterwards, a closed frame."""
    lib = _lib.load()
    w, h = 64, 48
    dim = mgr.fb.set_dim(w, h)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(mgr.fb.ctx, C.byref(fid)))      # first: a frame chooses the lane whose buffers the calls below use
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, w, h, 0))
    rs = np.random.RandomState(11)
    front = (rs.rand(dim.ah * dim.astride, 4) * 1.3 - 0.1).astype(np.float32)
    mgr.fb.write('front', front)
    start = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    plain = np.empty((h, w, 4), np.uint8)
    _lib.check(lib.fl_output(mgr.fb.ctx, w, h, _lib.OUT['rgba8'], plain.ctypes.data, 0))
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    after_plain = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    assert not np.array_equal(start, after_plain) and plain.std() > 10

    for ch in (3, 4):
        mgr.fb.write('seeds', start)                          # (the frame stays open: the same lane, the same framebuffer)
        _lib.check(lib.fl_timings_reset(mgr.fb.ctx))
        cap = lib.fl_png_bound(w, h, ch)
        buf = mgr.fb._pinned((cap + SLACK,), 'u1')
        buf[:] = SENTINEL
        _lib.check(lib.fl_output_png(mgr.fb.ctx, w, h, ch, buf.ctypes.data, 0, cap))
        ms = C.c_float(-1.0)
        _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
        assert ms.value >= 0.0
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        assert (buf[cap:] == SENTINEL).all()
        assert_criteria(file_of(buf), plain, ch, device_seg)      # the decoded pixels are the plain call's bytes
        assert np.array_equal(mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32), after_plain)
        tm = mgr.timings()
        assert tm['encode_ms'] > 0.0 and tm['jpeg_ms'] == tm['encode_ms']      # fl_timings_detail[5]: the kernels of both device encoders


@pytest.mark.parametrize('alpha', (False, True))
def test_through_the_shim(built, alpha):
    PIL_Image = pytest.importorskip('PIL.Image')
    gnm, prof = configs.cfg2(samples=2 ** 22)
    block = {'type': 'png', 'encoder': 'device'}
    if alpha:
        block['alpha'] = True
    prof = dict(prof, width=64, height=48, spp=2 ** 22 / (64.0 * 48.0), output=block)
    gprof = profile.wrap(prof, gnm)
    m = render.RenderManager(device=0, host_seed=7)
    try:
        rdr = render.Renderer(gnm, gprof)
        assert type(rdr.out) is output.DevicePNGOutput and rdr.out.alpha is alpha
        evt, h_out = m.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
        assert h_out.shape == rdr.out.shape(m.fb.calc_dim(64, 48)) and h_out.dtype == np.uint8
        media, logs = rdr.out.encode(h_out)
        assert list(media) == ['.png'] and logs == []
        data = media['.png'].read()
        ps = P.parse(data, record(h_out)[2])
        assert (ps.w, ps.h, ps.channels) == (64, 48, 4 if alpha else 3) and ps.pixels[:, :, :3].max() > 0
        im = PIL_Image.open(io.BytesIO(data))
        assert im.size == (64, 48) and im.mode == ('RGBA' if alpha else 'RGB')
        assert np.array_equal(np.asarray(im), ps.pixels)
    finally:
        m.fb.free()


def test_command_line(built, tmp_path):
    """python -m cuburn_amd FLAME --still --codec png --device-encode writes the device's file: Paeth rows in one IDAT per segment."""
    import json, os, subprocess, sys
    PIL_Image = pytest.importorskip('PIL.Image')
    here = os.path.dirname(os.path.abspath(__file__))
    gold = json.load(open(os.path.join(here, 'golden', 'genome_front.json')))
    (tmp_path / 'B.json').write_text(json.dumps(gold['db']['B']))
    out = subprocess.run([sys.executable, '-m', 'cuburn_amd', 'B', '-d', str(tmp_path), '--still', '-P', 'preview', '--codec', 'png',
                          '--device-encode', '-o', str(tmp_path), '--width', '320', '--height', '180', '--spp', '200'],
                         cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.png'))
    assert len(files) == 1, (os.listdir(str(tmp_path)), out.stderr[-500:])
    data = open(os.path.join(str(tmp_path), files[0]), 'rb').read()
    ps = P.parse(data)
    assert (ps.w, ps.h, ps.channels) == (320, 180, 3) and ps.filters == [4] * 180 and ps.stats['distances'] in ([], [1])
    assert len(ps.idat) == -(-len(ps.filtered) // 32768) or len(ps.idat) > 1
    im = PIL_Image.open(io.BytesIO(data))
    assert im.size == (320, 180) and im.mode == 'RGB' and np.array_equal(np.asarray(im), ps.pixels) and ps.pixels.max() > 60
