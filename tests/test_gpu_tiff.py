"""
The device TIFF encoder (cuburn_amd/csrc/tiff.hip; fl_tiff_encode, fl_output_tiff, DeviceTIFFOutput) against the model of
tests/tiff_model.py, which tests/test_cpu_tiff.py holds to Pillow and to its own reader.  Every file is compared byte for byte with
the file the model writes for the same samples; the frames are those of tests/tiff_cases.py, the smallest at which the tiling, the
predictor, the padding and the placement can go wrong.  Then the capacity rule, the destinations, bad arguments, fl_output_tiff
against fl_output, and the path through the shim.
"""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

from cuburn_amd import _lib, configs, output, profile, render
import encoder_harness as H
from encoder_harness import SENTINEL, SLACK, record, upload
import tiff_cases as TC
import tiff_model as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
    m.fb.free()


def encode(mgr, src, ch, bits, cap=None, buf=None):
    """fl_tiff_encode from u8 / u16 [h][w][4] into pinned memory (or `buf`) pre-filled with the sentinel; waits, checks the sentinel
    at and beyond cap; returns the buffer."""
    lib = _lib.load()
    h, w, _ = src.shape
    assert src.shape[2] == 4 and src.dtype == TC.dtype_of(bits)
    if cap is None:
        cap = lib.fl_tiff_bound(w, h, ch, bits)
        assert cap
    return H.encode(mgr, 'fl_tiff_encode', np.ascontiguousarray(src).view(np.uint8), w, h, (ch, bits), cap, buf)[0]


def file_of(buf, ch, bits):
    nbytes, status, param = record(buf)
    assert status == 0 and param == T.tile_bytes(ch, bits)
    return bytes(buf[16:16 + nbytes])


def assert_is_model(mgr, src, ch, bits):
    """The device's file for the samples is the model's, byte for byte, and within the bound; returns it."""
    data = file_of(encode(mgr, src, ch, bits), ch, bits)
    want = T.encode(src, ch, bits)
    if data != want:                                          # say where before failing
        ps = T.parse(data)
        assert (ps.w, ps.h, ps.channels, ps.bits) == (src.shape[1], src.shape[0], ch, bits)
        assert np.array_equal(ps.samples, src[:, :, :ch]), '%d samples differ' % int((ps.samples != src[:, :, :ch]).sum())
    assert data == want
    assert 16 + len(data) <= _lib.load().fl_tiff_bound(src.shape[1], src.shape[0], ch, bits) == T.bound(src.shape[1], src.shape[0], ch, bits)
    return data


def pillow_agrees(data, src, ch, bits):
    PIL_Image = pytest.importorskip('PIL.Image')
    im = PIL_Image.open(io.BytesIO(data))
    assert im.size == (src.shape[1], src.shape[0]) and im.mode == ('RGB' if ch == 3 else 'RGBA')
    assert np.array_equal(np.asarray(im), src[:, :, :ch] if bits == 8 else (src[:, :, :ch] >> 8).astype(np.uint8))


# ------------------------------------------------------------------ byte for byte with the model
@pytest.mark.parametrize('form', TC.FORMS, ids=TC.form_id)
def test_small_frames(mgr, form):
    """1 x 1: one tile, inline offsets, padding everywhere; a column; a row."""
    bits, ch = form
    for w, h in TC.small_shapes():
        data = assert_is_model(mgr, TC.noise(w, h, bits, 7 * w + h), ch, bits)
        assert T.parse(data).nt == 1


@pytest.mark.parametrize('form', TC.FORMS, ids=TC.form_id)
def test_tile_edges(mgr, form):
    """Exactly one full tile; two tiles, one of them almost all padding."""
    bits, ch = form
    for (w, h), nt in zip(TC.edge_shapes(bits), (1, 2, 2)):
        data = assert_is_model(mgr, TC.noise(w, h, bits, 3 * w + h) // 5, ch, bits)
        assert T.parse(data).nt == nt


@pytest.mark.parametrize('form', TC.FORMS, ids=TC.form_id)
def test_mixed_tiles(mgr, form):
    """Six tiles: dynamic and stored blocks, a pad byte; the same bytes again; Pillow reads them."""
    bits, ch = form
    src = TC.mixed(bits, TC.MIXED_SEED[form])
    nt, btypes, odd = TC.mixed_properties(T.encode(src, ch, bits))
    assert nt >= 6 and btypes == {0, 2} and odd               # (the model alone: the seed was chosen on the CPU)
    data = assert_is_model(mgr, src, ch, bits)
    assert file_of(encode(mgr, src, ch, bits), ch, bits) == data
    pillow_agrees(data, src, ch, bits)


@pytest.mark.parametrize('ch', (3, 4))
def test_byte_order_row(mgr, ch):
    src = TC.byte_order_source()
    data = assert_is_model(mgr, src, ch, 16)
    ps = T.parse(data)
    assert np.array_equal(ps.samples, src[:, :, :ch])
    tile = np.frombuffer(zlib.decompress(ps.streams[0]), '<u2').reshape(64, 64, ch)
    assert tile[0, :5, 0].tolist() == [0x00ff, 0x0001, 0xfeff, 0x0001, 0x0000]


def test_widest_frame(mgr):
    """65535 x 1 RGBA16 of noise: 1024 tiles, every thread of the placement kernel has one; the first and the last tile against the
    model (the pure-Python coder is too slow for all of them), every sample through the reader."""
    src = TC.noise(65535, 1, 16, 12)
    data = file_of(encode(mgr, src, 4, 16), 4, 16)
    ps = T.parse(data)
    assert ps.nt == 1024 and (ps.w, ps.h, ps.channels, ps.bits) == (65535, 1, 4, 16)
    assert np.array_equal(ps.samples, src)
    tiles = T.tiles(src, 4, 16)
    assert ps.streams[0] == T.tile_stream(tiles[0]) and ps.streams[-1] == T.tile_stream(tiles[-1])
    assert ps.offsets[0] == T.header_bytes(65535, 1, 4, 16) == 178 + 8 * 1024


def test_tall_frame(mgr):
    for bits, ch in ((16, 3), (8, 4)):
        data = assert_is_model(mgr, TC.noise(1, 200, bits, 9) // 3, ch, bits)
        assert T.parse(data).nt == 4


# ------------------------------------------------------------------ capacity, destinations, bad arguments
def test_capacity(mgr):
    src = TC.mixed(16, TC.MIXED_SEED[(16, 4)])
    h, w, _ = src.shape
    data = file_of(encode(mgr, src, 4, 16), 4, 16)
    need, tb = len(data), T.tile_bytes(4, 16)
    buf = encode(mgr, src, 4, 16, cap=16 + need)              # (encode checks the sentinel at and beyond cap)
    assert record(buf) == (need, 0, tb) and file_of(buf, 4, 16) == data
    for cap in (16 + need - 1, 16 + T.header_bytes(w, h, 4, 16)):
        buf = encode(mgr, src, 4, 16, cap=cap)
        assert record(buf) == (need, 1, tb)


def test_pageable_memory(mgr):
    src = TC.mixed(16, TC.MIXED_SEED[(16, 3)])
    cap = _lib.load().fl_tiff_bound(src.shape[1], src.shape[0], 3, 16)
    buf = encode(mgr, src, 3, 16, buf=np.empty(cap + SLACK, np.uint8))
    assert file_of(buf, 3, 16) == T.encode(src, 3, 16)


def test_device_destination_at_an_odd_address(mgr):
    import torch
    lib = _lib.load()
    src = TC.mixed(8, TC.MIXED_SEED[(8, 4)])
    h, w, _ = src.shape
    want = T.encode(src, 4, 8)
    cap = 16 + len(want) + 7
    t = upload(mgr, src)
    out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device=t.device)
    torch.cuda.synchronize(mgr.fb.device)
    _lib.check(lib.fl_tiff_encode(mgr.fb.ctx, w, h, t.data_ptr(), 4, 8, None, out.data_ptr() + 1, cap))
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    dev = out.cpu().numpy()
    assert dev[0] == SENTINEL and (dev[1 + cap:] == SENTINEL).all() and file_of(dev[1:], 4, 8) == want


def test_bad_arguments(mgr):
    lib = _lib.load()
    src = TC.noise(37, 10, 16, 4) // 7
    want = T.encode(src, 4, 16)
    h, w = 10, 37
    t = upload(mgr, src.view(np.uint8))
    cap = lib.fl_tiff_bound(w, h, 4, 16)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    ctx, sp, dst = mgr.fb.ctx, t.data_ptr(), buf.ctypes.data
    assert lib.fl_tiff_bound(20000, 65535, 4, 8) == 0 == lib.fl_tiff_bound(20000, 65535, 3, 16)
    bad = [(0, h, sp, 4, 16, dst, 0, cap), (w, 0, sp, 4, 16, dst, 0, cap), (65536, h, sp, 4, 16, dst, 0, cap), (w, 65536, sp, 4, 16, dst, 0, cap),
           (w, h, sp, 2, 16, dst, 0, cap), (w, h, sp, 5, 16, dst, 0, cap), (w, h, sp, 0, 16, dst, 0, cap),
           (w, h, sp, 4, 0, dst, 0, cap), (w, h, sp, 4, 12, dst, 0, cap), (w, h, sp, 4, 32, dst, 0, cap),
           (20000, 65535, sp, 4, 8, dst, 0, cap),                          # a frame whose fl_tiff_bound is 0: beyond 2^32 - 1
           (w, h, 0, 4, 16, dst, 0, cap), (w, h, sp, 4, 16, None, 0, cap), (w, h, sp, 4, 16, dst, 0, 16 + T.header_bytes(w, h, 4, 16) - 1)]
    for args in bad:
        buf[:] = SENTINEL
        assert lib.fl_tiff_encode(ctx, *args) == _lib.FL_E_INVAL, args
        assert lib.fl_last_error()
        if args[2]:
            assert lib.fl_output_tiff(ctx, *(args[:2] + args[3:])) == _lib.FL_E_INVAL, args
        _lib.check(lib.fl_ctx_sync(ctx))
        assert (buf == SENTINEL).all()
        _lib.check(lib.fl_tiff_encode(ctx, w, h, sp, 4, 16, dst, 0, cap))      # ... and the next frame is still right
        _lib.check(lib.fl_ctx_sync(ctx))
        assert file_of(buf, 4, 16) == want and (buf[cap:] == SENTINEL).all()


# ------------------------------------------------------------------ the whole path
@pytest.mark.parametrize('bits', (16, 8))
def test_whole_path(mgr, bits):
    """fl_output_tiff = fl_output(FL_OUT_RGBA16 / RGBA8) + the encode: same samples, same dither states afterwards, a closed frame."""
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
    plain = np.empty((h, w, 4), TC.dtype_of(bits))
    _lib.check(lib.fl_output(mgr.fb.ctx, w, h, _lib.OUT['rgba16' if bits == 16 else 'rgba8'], plain.ctypes.data, 0))
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    after_plain = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    assert not np.array_equal(start, after_plain) and plain.std() > (1000 if bits == 16 else 4)

    for ch in (3, 4):
        mgr.fb.write('seeds', start)                          # (the frame stays open: the same lane, the same framebuffer)
        cap = lib.fl_tiff_bound(w, h, ch, bits)
        buf = mgr.fb._pinned((cap + SLACK,), 'u1')
        buf[:] = SENTINEL
        _lib.check(lib.fl_output_tiff(mgr.fb.ctx, w, h, ch, bits, buf.ctypes.data, 0, cap))
        ms = C.c_float(-1.0)
        _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
        assert ms.value >= 0.0
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        assert (buf[cap:] == SENTINEL).all()
        data = file_of(buf, ch, bits)
        ps = T.parse(data)
        assert (ps.w, ps.h, ps.channels, ps.bits) == (w, h, ch, bits)
        assert np.array_equal(ps.samples, plain[:, :, :ch])   # the decoded samples are the plain call's
        assert data == T.encode(plain, ch, bits)
        assert np.array_equal(mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32), after_plain)


def test_encode_is_timed(mgr):
    """The encode's kernels are in slot 5 of fl_timings_detail, like the other encoders'."""
    _lib.check(_lib.load().fl_timings_reset(mgr.fb.ctx))
    assert mgr.timings()['encode_ms'] == 0.0
    encode(mgr, TC.noise(70, 70, 16, 2), 3, 16)
    assert mgr.timings()['encode_ms'] > 0.0


# ------------------------------------------------------------------ through the shim
class _TiffWithRaw16(output.DeviceTIFFOutput):
    """The output the profile chose, which also takes the raw16 output of the same frame from the same seeds: fl_output(FL_OUT_RGBA16)
    first, the dither states put back, then the device TIFF.  (Two managers of one seed do not serve: the accumulator's float sums
    depend on the order of its atomic adds.)"""

    def copy(self, fb, dim, **kw):
        lib = _lib.load()
        _lib.check(lib.fl_ctx_sync(fb.ctx))
        seeds = fb.read('seeds', (fb.nwalkers, 3), np.uint32)
        raw = output.Raw16Output().copy(fb, dim)
        _lib.check(lib.fl_ctx_sync(fb.ctx))
        self.raw16 = np.array(raw)
        assert not np.array_equal(fb.read('seeds', (fb.nwalkers, 3), np.uint32), seeds)
        fb.write('seeds', seeds)
        return output.DeviceTIFFOutput.copy(self, fb, dim, **kw)


@pytest.mark.parametrize('alpha', (False, True))
def test_through_the_shim(built, alpha):
    """output: {"type": "tiff", "compression": "deflate"} through profile, Renderer and queue_frame: the file decodes to exactly the
    raw16 output of the same frame and seeds, and is the file the model writes for it."""
    block = {'type': 'tiff', 'compression': 'deflate'}
    if alpha:
        block['alpha'] = True
    gnm, prof = configs.cfg2(samples=2 ** 22)
    prof = dict(prof, width=64, height=48, spp=2 ** 22 / (64.0 * 48.0), output=block)
    gprof = profile.wrap(prof, gnm)
    m = render.RenderManager(device=0, host_seed=7)
    try:
        rdr = render.Renderer(gnm, gprof)
        assert type(rdr.out) is output.DeviceTIFFOutput
        assert (rdr.out.alpha, rdr.out.bits, rdr.out.entry) == (alpha, 16, 'fl_output_tiff')
        rdr.out = _TiffWithRaw16(alpha=rdr.out.alpha, bits=rdr.out.bits)
        evt, h_out = m.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
        assert h_out.shape == rdr.out.shape(m.fb.calc_dim(64, 48)) and h_out.dtype == np.uint8
        media, logs = rdr.out.encode(h_out)
        assert list(media) == ['.tiff'] and logs == []
        data, raw = media['.tiff'].read(), rdr.out.raw16
    finally:
        m.fb.free()
    ch = 4 if alpha else 3
    ps = T.parse(data)
    assert (ps.w, ps.h, ps.channels, ps.bits) == (64, 48, ch, 16) and ps.samples[:, :, :3].max() > 255
    assert raw.shape == (48, 64, 4) and raw.dtype == np.uint16 and (raw & 255).std() > 10
    assert np.array_equal(ps.samples, raw[:, :, :ch])
    assert data == T.encode(raw, ch, 16)
    pillow_agrees(data, raw, ch, 16)


def test_command_line_writes_a_file_pillow_opens(built, tmp_path):
    """python -m cuburn_amd FLAME --still --codec tiff --tiff-compression deflate, end to end."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    gold = json.load(open(os.path.join(here, 'golden', 'genome_front.json')))
    (tmp_path / 'B.json').write_text(json.dumps(gold['db']['B']))
    out = subprocess.run([sys.executable, '-m', 'cuburn_amd', 'B', '-d', str(tmp_path), '--still', '-P', 'preview', '--codec', 'tiff',
                          '--tiff-compression', 'deflate', '-o', str(tmp_path), '--width', '320', '--height', '180', '--spp', '200'],
                         cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.tiff'))
    assert len(files) == 1, (os.listdir(str(tmp_path)), out.stderr[-500:])
    data = open(os.path.join(str(tmp_path), files[0]), 'rb').read()
    ps = T.parse(data)
    assert (ps.w, ps.h, ps.channels, ps.bits, ps.nt) == (320, 180, 3, 16, 15) and ps.samples.max() > 60 * 257
    assert len(data) < 320 * 180 * 6                          # smaller than the uncompressed samples
    pillow_agrees(data, ps.samples, 3, 16)
