"""
The device GIF encoder (cuburn_amd/csrc/gif.hip; fl_gif_encode, fl_output_gif) and the GIF output against the Python model of
tests/gif_model.py, which tests/test_cpu_gif.py holds to Pillow and to its own strict reader: for every frame of tests/gif_cases.py
the device's frame block equals the model's byte for byte — histogram, cut, palette, lookup, dither, every LZW code and width, the
segments' padding, the sub-blocks — and the record says so.  All arithmetic on both sides is integer arithmetic, so there is no
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
import gif_cases as GC
import gif_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
    m.fb.free()


def encode(mgr, frame, colors, amp, cap=None, buf=None):
    """fl_gif_encode into pinned memory (or `buf`) pre-filled with the sentinel; checks the sentinel at and beyond cap."""
    h, w = frame.shape[:2]
    if cap is None:
        cap = _lib.load().fl_gif_bound(w, h)
    return H.encode(mgr, 'fl_gif_encode', frame, w, h, (colors, amp), cap, buf)


def block_of(buf, seg=M.SEG):
    nbytes, status, param = record(buf)
    assert (status, param) == (0, seg)
    return bytes(buf[16:16 + nbytes])


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return 'lengths %d and %d, first difference at %s' % (len(a), len(b), int(d[0]) if len(d) else 'none below %d' % n)


@pytest.mark.parametrize('name', GC.NAMES)
def test_cases(mgr, name):
    frame, colors, amp = GC.cases()[name]
    want = GC.model_block(name)
    buf, cap = encode(mgr, frame, colors, amp)
    got = block_of(buf)
    assert got == want, first_difference(got, want)
    assert (buf[16 + len(got):cap] == SENTINEL).all()           # nothing behind the block
    again, _ = encode(mgr, frame, colors, amp)
    assert block_of(again) == got


def test_few_colours_come_back_exactly(mgr):
    PIL_Image = pytest.importorskip('PIL.Image')
    frame, colors, amp = GC.cases()['few_colours']
    buf, _ = encode(mgr, frame, colors, amp)
    im = PIL_Image.open(io.BytesIO(M.gif_file(frame.shape[1], frame.shape[0], [block_of(buf)])))
    assert np.array_equal(np.asarray(im.convert('RGB')), frame[:, :, :3])


def test_capacity(mgr):
    frame, colors, amp = GC.cases()['37x29']
    need = len(GC.model_block('37x29'))
    for cap in (16 + need - 1, 16 + M.HEADER_BYTES):
        buf, cap = encode(mgr, frame, colors, amp, cap=cap)
        assert record(buf) == (need, 1, M.SEG)
        assert (buf[16:] == SENTINEL).all()                     # nothing behind the record
    buf, cap = encode(mgr, frame, colors, amp, cap=16 + need)
    assert record(buf) == (need, 0, M.SEG) and block_of(buf) == GC.model_block('37x29')


def test_bad_arguments(mgr):
    lib = _lib.load()
    frame, colors, amp = GC.cases()['37x29']
    h, w = frame.shape[:2]
    t = upload(mgr, frame)
    cap = lib.fl_gif_bound(w, h)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    ctx, src, dst = mgr.fb.ctx, t.data_ptr(), buf.ctypes.data
    bad = [(w, h, src, 1, 8, dst, 0, cap), (w, h, src, 257, 8, dst, 0, cap), (w, h, src, 0, 8, dst, 0, cap), (w, h, src, -4, 8, dst, 0, cap),
           (w, h, src, 256, -1, dst, 0, cap), (w, h, src, 256, 65, dst, 0, cap),
           (0, h, src, 256, 8, dst, 0, cap), (w, 0, src, 256, 8, dst, 0, cap), (65536, 1, src, 256, 8, dst, 0, cap), (4097, 4096, src, 256, 8, dst, 0, 1 << 30),
           (w, h, 0, 256, 8, dst, 0, cap), (w, h, src, 256, 8, None, 0, cap), (w, h, src, 256, 8, dst, 0, 16 + M.HEADER_BYTES - 1)]
    for args in bad:
        assert lib.fl_gif_encode(ctx, *args) == _lib.FL_E_INVAL, args
        assert lib.fl_last_error()
    for args in bad:
        if args[2]:
            assert lib.fl_output_gif(ctx, *(args[:2] + args[3:])) == _lib.FL_E_INVAL, args
    _lib.check(lib.fl_ctx_sync(ctx))
    assert (buf == SENTINEL).all()
    good, _ = encode(mgr, frame, colors, amp)
    assert block_of(good) == GC.model_block('37x29')


def test_pageable_memory_and_device_destinations(mgr):
    """A destination that is not pinned receives a copy; a device destination of any alignment receives the same bytes."""
    import torch
    lib = _lib.load()
    frame, colors, amp = GC.cases()['gradient_c256_a8']
    want = GC.model_block('gradient_c256_a8')
    h, w = frame.shape[:2]
    cap = lib.fl_gif_bound(w, h)
    buf, _ = encode(mgr, frame, colors, amp, buf=np.empty(cap + SLACK, np.uint8))
    assert block_of(buf) == want
    buf, _ = encode(mgr, frame, colors, amp, cap=16 + len(want) - 1, buf=np.empty(16 + len(want) + SLACK, np.uint8))
    assert record(buf) == (len(want), 1, M.SEG)
    cap = 16 + len(want) + 7
    t = upload(mgr, frame)
    for odd in (1, 2, 3):
        out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device=t.device)
        torch.cuda.synchronize(mgr.fb.device)
        host = mgr.fb._pinned((cap + SLACK,), 'u1')
        host[:] = SENTINEL
        _lib.check(lib.fl_gif_encode(mgr.fb.ctx, w, h, t.data_ptr(), colors, amp, host.ctypes.data, out.data_ptr() + odd, cap))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        dev = out.cpu().numpy()
        assert (dev[:odd] == SENTINEL).all() and (dev[odd + cap:] == SENTINEL).all() and (host[cap:] == SENTINEL).all()
        assert block_of(dev[odd:]) == want and block_of(host) == want


def test_whole_path(mgr):
    """fl_output_gif = fl_output(FL_OUT_RGBA8) + the encode: same pixels, same dither states afterwards, a closed frame."""
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

    mgr.fb.write('seeds', start)
    cap = lib.fl_gif_bound(w, h)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    _lib.check(lib.fl_output_gif(mgr.fb.ctx, w, h, 64, 8, buf.ctypes.data, 0, cap))
    ms = C.c_float(-1.0)
    _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
    assert ms.value >= 0.0
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    assert_untouched(buf, cap)
    assert np.array_equal(mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32), after_plain)
    direct, _ = encode(mgr, pixels, 64, 8)
    assert block_of(buf) == block_of(direct) == M.frame_block(pixels, 64, 8)
    assert mgr.timings()['encode_ms'] > 0.0          # fl_timings_detail[5]: the encode's kernels


def test_segment_length_from_the_environment(built, monkeypatch):
    """FLAME_GIF_SEG is read when a context is created: 256 gives the model's bytes for segments of 256 pixels."""
    monkeypatch.setenv('FLAME_GIF_SEG', '256')
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    try:
        for name in ('gradient_c256_a8', 'step_256', '1x1'):
            frame, colors, amp = GC.cases()[name]
            buf, _ = encode(m, frame, colors, amp)
            assert record(buf)[1:] == (0, 256)
            got, want = block_of(buf, 256), GC.model_block(name, 256)
            assert got == want, first_difference(got, want)
            assert want != GC.model_block(name) or name == '1x1'
    finally:
        _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
        m.fb.free()


def _small(block):
    gnm, prof = configs.cfg2(samples=2 ** 22)
    prof = dict(prof, width=64, height=48, spp=2 ** 22 / (64.0 * 48.0), fps=24, output=block)
    return gnm, profile.wrap(prof, gnm)


def test_through_the_shim(built):
    """Three frames of a 64 x 48 config with type gif: a .gif whose blocks are the model's blocks of the `raw` frames of the same
    times from a manager with the same seed (a manager's frames depend on its seed and on the order of its frames only)."""
    times = (0.25, 0.5, 0.75)
    got = {}
    for block in ({'type': 'gif', 'colors': 32, 'loop': 2}, {'type': 'raw'}):
        gnm, gprof = _small(block)
        m = render.RenderManager(device=0, host_seed=7)
        try:
            rdr = render.Renderer(gnm, gprof)
            frames = []
            for t in times:
                evt, h_out = m.queue_frame(rdr, gnm, gprof, t)
                evt.synchronize()
                assert h_out.shape == rdr.out.shape(m.fb.calc_dim(64, 48)) and h_out.dtype == np.uint8
                if block['type'] == 'gif':
                    assert rdr.out.encode(h_out) == ({}, [])
                else:
                    frames.append(np.array(h_out))
            if block['type'] == 'gif':
                assert type(rdr.out) is encoders.GIFOutput
                media, logs = rdr.out.encode(None)
                assert list(media) == ['.gif'] and logs == []
                got['gif'] = media['.gif'].read()
            else:
                assert type(rdr.out) is output.RawOutput
                got['raw'] = frames
        finally:
            m.fb.free()
    assert len(got['raw']) == 3 and got['raw'][0][:, :, :3].max() > 0 and not np.array_equal(got['raw'][0], got['raw'][1])
    assert got['gif'] == M.gif_file(64, 48, [M.frame_block(f, 32, 8) for f in got['raw']], fps=24, loop=2)


def test_command_line_writes_a_gif(built, tmp_path):
    """python -m cuburn_amd FLAME --codec gif at 64 x 48 with three frames in the file, end to end: Pillow opens it and returns
    what the model's strict reader returns."""
    PIL_Image = pytest.importorskip('PIL.Image')
    here = os.path.dirname(os.path.abspath(__file__))
    gold = json.load(open(os.path.join(here, 'golden', 'genome_front.json')))
    (tmp_path / 'B.json').write_text(json.dumps(gold['db']['B']))
    out = subprocess.run([sys.executable, '-m', 'cuburn_amd', 'B', '-d', str(tmp_path), '-P', 'preview', '--codec', 'gif', '--gif-colors', '64',
                          '-o', str(tmp_path), '--width', '64', '--height', '48', '--spp', '200', '--fps', '24', '--duration', '0.125',
                          '--shard', '0.125'],
                         cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.gif'))
    assert len(files) == 1, (os.listdir(str(tmp_path)), out.stderr[-500:])
    data = open(os.path.join(str(tmp_path), files[0]), 'rb').read()
    im = PIL_Image.open(io.BytesIO(data))
    assert im.size == (64, 48) and im.n_frames == 3 and im.info['loop'] == 0
    at, blocks = 13 + 19, []
    for k in range(3):
        assert data[at:at + 4] == b'\x21\xf9\x04\x04' and data[at + 4:at + 8] == bytes([M.delays(3, 24)[k], 0, 0, 0])
        at += 8
        n = M.HEADER_BYTES
        while data[at + n]:
            n += 1 + data[at + n]
        blocks.append(data[at:at + n + 1])
        at += n + 1
    assert data[at:] == b'\x3b'
    seen = []
    for k, blk in enumerate(blocks):
        w, h, pal, idx = M.decode_block(blk)
        assert (w, h) == (64, 48) and idx.max() < 64 and not pal[64:].any()
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert('RGB')), pal[idx])
        assert M.block_of(w, h, pal, idx) == blk                 # the LZW and the sub-blocks are the model's
        seen.append(pal[idx])
    assert seen[0].max() > 0 and not np.array_equal(seen[0], seen[1])
