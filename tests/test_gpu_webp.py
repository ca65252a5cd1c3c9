"""
The device WebP encoder (cuburn_amd/csrc/webp.hip; fl_webp_encode, fl_output_webp) and the WebP output against the Python model of
tests/webp_model.py, which tests/test_cpu_webp.py holds to Pillow's libwebp and to its own strict reader: for every frame of
tests/webp_cases.py the device's frame block equals the model's byte for byte — every tile's mode, every code's lengths and header,
every pixel's bits and the padding — and the record says so.  All arithmetic on both sides is integer arithmetic, so there is no
tolerance anywhere.
"""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cuburn_amd import _lib, configs, encoders, output, profile, render
import encoder_harness as H
from encoder_harness import SENTINEL, SLACK, assert_untouched, record, upload
import webp_cases as WC
import webp_model as M

pytestmark = pytest.mark.gpu
PARAM = _lib.WEBP_PB | _lib.WEBP_EB << 8


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
    m.fb.free()


def encode(mgr, frame, channels, cap=None, buf=None):
    """fl_webp_encode into pinned memory (or `buf`) pre-filled with the sentinel; checks the sentinel at and beyond cap."""
    h, w = frame.shape[:2]
    if cap is None:
        cap = _lib.load().fl_webp_bound(w, h, channels)
    return H.encode(mgr, 'fl_webp_encode', frame, w, h, (channels,), cap, buf)


def block_of(buf):
    nbytes, status, param = record(buf)
    assert (status, param) == (0, PARAM)
    return bytes(buf[16:16 + nbytes])


def first_difference(a, b):
    """Where two blocks part: the bit offset in the payload (the chunk header is 8 bytes)."""
    n = min(len(a), len(b))
    x = np.frombuffer(a[:n], np.uint8) ^ np.frombuffer(b[:n], np.uint8)
    d = np.nonzero(x)[0]
    if not len(d):
        return 'lengths %d and %d, no difference below %d' % (len(a), len(b), n)
    bit = int(d[0]) * 8 + int(np.nonzero(np.unpackbits(x[d[0]:d[0] + 1], bitorder='little'))[0][0])
    return 'lengths %d and %d, first differing bit %d of the block, bit %d of the payload' % (len(a), len(b), bit, bit - 64)


@pytest.mark.parametrize('name', WC.NAMES)
def test_cases(mgr, name):
    frame, channels = WC.cases()[name]
    want = WC.model_block(name)
    buf, cap = encode(mgr, frame, channels)
    got = block_of(buf)
    assert got == want, first_difference(got, want)
    assert 16 + len(got) <= cap == M.bound(frame.shape[1], frame.shape[0], channels)
    assert (buf[16 + len(got):cap] == SENTINEL).all()           # nothing behind the block
    again, _ = encode(mgr, frame, channels)
    assert block_of(again) == got


def test_capacity(mgr):
    for name in ('plasma_17x17', 'plasma_65x64'):
        frame, channels = WC.cases()[name]
        need = len(WC.model_block(name))
        for cap in (16 + need - 1, 16 + 8):
            buf, cap = encode(mgr, frame, channels, cap=cap)
            assert record(buf) == (need, 1, PARAM)
            assert (buf[16:] == SENTINEL).all()                 # nothing behind the record
        buf, cap = encode(mgr, frame, channels, cap=16 + need)
        assert record(buf) == (need, 0, PARAM) and block_of(buf) == WC.model_block(name)


def test_bad_arguments(mgr):
    lib = _lib.load()
    frame, channels = WC.cases()['plasma_17x17']
    h, w = frame.shape[:2]
    t = upload(mgr, frame)
    cap = lib.fl_webp_bound(w, h, channels)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    ctx, src, dst = mgr.fb.ctx, t.data_ptr(), buf.ctypes.data
    bad = [(w, h, src, 2, dst, 0, cap), (w, h, src, 5, dst, 0, cap), (w, h, src, 0, dst, 0, cap), (w, h, src, 1, dst, 0, cap),
           (0, h, src, 4, dst, 0, cap), (w, 0, src, 4, dst, 0, cap), (16385, 1, src, 4, dst, 0, 1 << 30), (1, 16385, src, 4, dst, 0, 1 << 30),
           (65536, 1, src, 4, dst, 0, 1 << 30), (w, h, 0, 4, dst, 0, cap), (w, h, src, 4, None, 0, cap), (w, h, src, 4, dst, 0, 16 + 8 - 1)]
    for args in bad:
        assert lib.fl_webp_encode(ctx, *args) == _lib.FL_E_INVAL, args
        assert lib.fl_last_error()
    for args in bad:
        if args[2]:
            assert lib.fl_output_webp(ctx, *(args[:2] + args[3:])) == _lib.FL_E_INVAL, args
    _lib.check(lib.fl_ctx_sync(ctx))
    assert (buf == SENTINEL).all()
    good, _ = encode(mgr, frame, channels)
    assert block_of(good) == WC.model_block('plasma_17x17')


def test_pageable_memory_and_device_destinations(mgr):
    """A destination that is not pinned receives a copy; a device destination of any alignment receives the same bytes."""
    import torch
    lib = _lib.load()
    frame, channels = WC.cases()['plasma_130x70']
    want = WC.model_block('plasma_130x70')
    h, w = frame.shape[:2]
    cap = lib.fl_webp_bound(w, h, channels)
    buf, _ = encode(mgr, frame, channels, buf=np.empty(cap + SLACK, np.uint8))
    assert block_of(buf) == want
    buf, _ = encode(mgr, frame, channels, cap=16 + len(want) - 1, buf=np.empty(16 + len(want) + SLACK, np.uint8))
    assert record(buf) == (len(want), 1, PARAM)
    cap = 16 + len(want) + 7
    t = upload(mgr, frame)
    for odd in (1, 2, 3):
        out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device=t.device)
        torch.cuda.synchronize(mgr.fb.device)
        host = mgr.fb._pinned((cap + SLACK,), 'u1')
        host[:] = SENTINEL
        _lib.check(lib.fl_webp_encode(mgr.fb.ctx, w, h, t.data_ptr(), channels, host.ctypes.data, out.data_ptr() + odd, cap))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        dev = out.cpu().numpy()
        assert (dev[:odd] == SENTINEL).all() and (dev[odd + cap:] == SENTINEL).all() and (host[cap:] == SENTINEL).all()
        assert block_of(dev[odd:]) == want and block_of(host) == want


def test_whole_path(mgr):
    """fl_output_webp = fl_output(FL_OUT_RGBA8) + the encode: same pixels, same dither states afterwards, a closed frame."""
    lib = _lib.load()
    w, h = 70, 50
    dim = mgr.fb.set_dim(w, h)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(mgr.fb.ctx, C.byref(fid)))      # first: a frame chooses the lane whose buffers the calls below use
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, w, h, 0))
    rs = np.random.RandomState(11)
    front = (rs.rand(dim.ah * dim.astride, 4) * 1.3 - 0.1).astype(np.float32)
    mgr.fb.write('front', front)
    start = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    pixels = np.empty((h, w, 4), np.uint8)
    _lib.check(lib.fl_output(mgr.fb.ctx, w, h, _lib.OUT['rgba8'], pixels.ctypes.data, 0))
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    after_plain = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    assert not np.array_equal(start, after_plain) and pixels[:, :, :3].std() > 10

    channels = 4
    mgr.fb.write('seeds', start)
    cap = lib.fl_webp_bound(w, h, channels)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    _lib.check(lib.fl_output_webp(mgr.fb.ctx, w, h, channels, buf.ctypes.data, 0, cap))
    ms = C.c_float(-1.0)
    _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
    assert ms.value >= 0.0
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    assert_untouched(buf, cap)
    assert np.array_equal(mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32), after_plain)
    direct, _ = encode(mgr, pixels, channels)
    assert block_of(buf) == block_of(direct) == M.encode(pixels, channels)
    assert mgr.timings()['encode_ms'] > 0.0          # fl_timings_detail[5]: the encode's kernels


def _small(block):
    gnm, prof = configs.cfg2(samples=2 ** 22)
    prof = dict(prof, width=96, height=64, spp=2 ** 22 / (96.0 * 64.0), fps=24, output=block)
    return gnm, profile.wrap(prof, gnm)


def test_through_the_shim(built):
    """Three frames of a 96 x 64 config with type webp: a .webp that the model's container reader parses and whose frames, by the
    strict reader and by Pillow, are the `raw` frames of the same times from a manager with the same seed (a manager's frames depend
    on its seed and on the order of its frames only)."""
    times = (0.25, 0.5, 0.75)
    got = {}
    for block in ({'type': 'webp', 'alpha': True, 'loop': 2}, {'type': 'raw'}):
        gnm, gprof = _small(block)
        m = render.RenderManager(device=0, host_seed=7)
        try:
            rdr = render.Renderer(gnm, gprof)
            frames = []
            for t in times:
                evt, h_out = m.queue_frame(rdr, gnm, gprof, t)
                evt.synchronize()
                assert h_out.shape == rdr.out.shape(m.fb.calc_dim(96, 64)) and h_out.dtype == np.uint8
                if block['type'] == 'webp':
                    assert rdr.out.encode(h_out) == ({}, [])
                else:
                    frames.append(np.array(h_out))
            if block['type'] == 'webp':
                assert type(rdr.out) is encoders.WebPOutput
                media, logs = rdr.out.encode(None)
                assert list(media) == ['.webp'] and logs == []
                got['webp'] = media['.webp'].read()
            else:
                assert type(rdr.out) is output.RawOutput
                got['raw'] = frames
        finally:
            m.fb.free()
    assert len(got['raw']) == 3 and got['raw'][0][:, :, :3].max() > 0 and not np.array_equal(got['raw'][0], got['raw'][1])
    parsed = M.read_file(got['webp'])
    assert parsed['animated'] and (parsed['w'], parsed['h'], parsed['alpha'], parsed['loop']) == (96, 64, True, 2)
    assert parsed['durations'] == M.durations(3, 24)
    for blk, raw in zip(parsed['blocks'], got['raw']):
        pixels, info = M.decode(blk)
        assert np.array_equal(pixels, raw) and info['alpha_is_used'] == 1
        assert blk == M.encode(raw, 4)
    assert got['webp'] == M.write_animation(parsed['blocks'], 96, 64, True, 2, M.durations(3, 24))
    try:
        from PIL import Image, features
    except ImportError:
        return
    if features.check('webp'):
        im = Image.open(io.BytesIO(got['webp']))
        assert im.size == (96, 64) and im.n_frames == 3
        for k, raw in enumerate(got['raw']):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert('RGBA')), raw)


def test_command_line_writes_a_webp(built, tmp_path):
    """python -m cuburn_amd FLAME --codec webp at 64 x 48 with three frames in the file, and --still, end to end: the container reader
    parses the files and the strict reader decodes every frame."""
    here = os.path.dirname(os.path.abspath(__file__))
    gold = json.load(open(os.path.join(here, 'golden', 'genome_front.json')))
    (tmp_path / 'B.json').write_text(json.dumps(gold['db']['B']))
    out = subprocess.run([sys.executable, '-m', 'cuburn_amd', 'B', '-d', str(tmp_path), '-P', 'preview', '--codec', 'webp',
                          '-o', str(tmp_path), '--width', '64', '--height', '48', '--spp', '200', '--fps', '24', '--duration', '0.125',
                          '--shard', '0.125'],
                         cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.webp'))
    assert len(files) == 1, (os.listdir(str(tmp_path)), out.stderr[-500:])
    parsed = M.read_file(open(os.path.join(str(tmp_path), files[0]), 'rb').read())
    assert parsed['animated'] and (parsed['w'], parsed['h'], parsed['alpha'], parsed['loop']) == (64, 48, False, 0)
    assert parsed['durations'] == M.durations(3, 24)
    seen = [M.decode(blk)[0] for blk in parsed['blocks']]
    assert len(seen) == 3 and seen[0][..., :3].max() > 0 and not np.array_equal(seen[0], seen[1]) and (seen[0][..., 3] == 255).all()
    for blk, pixels in zip(parsed['blocks'], seen):
        assert blk == M.encode(pixels, 3)
    out = subprocess.run([sys.executable, '-m', 'cuburn_amd', 'B', '-d', str(tmp_path), '-P', 'preview', '--codec', 'webp', '--still', '-n', 'one',
                          '-o', str(tmp_path), '--width', '64', '--height', '48', '--spp', '200'],
                         cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    stills = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.webp') and f not in files)
    assert len(stills) == 1, (os.listdir(str(tmp_path)), out.stderr[-500:])
    parsed = M.read_file(open(os.path.join(str(tmp_path), stills[0]), 'rb').read())
    assert not parsed['animated'] and M.decode(parsed['blocks'][0])[0].shape == (48, 64, 4)
