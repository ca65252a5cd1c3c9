"""
The device OpenEXR encoder (cuburn_amd/csrc/exr.hip; fl_exr_encode, fl_output_exr, DeviceEXROutput) against the model of
tests/exr_model.py, which tests/test_cpu_exr.py holds to numpy's float16 and to its own reader.  Every file is compared byte for
byte with the file the model writes for the same samples; the frames are those of tests/exr_cases.py, the smallest at which the
conversion, the cropped tiles, the two data forms and the placement can go wrong.  Then the source's stride, the capacity rule, the
destinations, bad arguments, fl_output_exr on the front buffer in place, and the path through the shim.
"""
import ctypes as C

import numpy as np
import pytest

from cuburn_amd import _lib, configs, output, profile, render
import encoder_harness as H
from encoder_harness import SENTINEL, SLACK, record, upload
import exr_cases as XC
import exr_model as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
    m.fb.free()


def encode(mgr, src, ch, px, cap=None, buf=None, stride=None):
    """fl_exr_encode from f32 [h][stride][4] into pinned memory (or `buf`) pre-filled with the sentinel; waits, checks the sentinel
    at and beyond cap; returns the buffer.  `src` is [h][w][4] unless `stride` says its rows are longer than the frame's."""
    lib = _lib.load()
    h, sw, _ = src.shape
    w = sw if stride is None else stride[0]
    assert src.shape[2] == 4 and src.dtype == np.float32
    if cap is None:
        cap = lib.fl_exr_bound(w, h, ch, px)
        assert cap
    return H.encode(mgr, 'fl_exr_encode', np.ascontiguousarray(src).view(np.uint8), w, h, (sw, ch, px), cap, buf)[0]


def file_of(buf, ch):
    nbytes, status, param = record(buf)
    assert status == 0 and param == X.tile_bytes(ch)
    return bytes(buf[16:16 + nbytes])


def explain(data, want, src, ch, px):
    """Say where a file differs from the model's before the comparison fails."""
    if data != want:
        ps = X.parse(data)
        assert (ps.w, ps.h, ps.channels, ps.pixel) == (src.shape[1], src.shape[0], ch, px)
        ref = X.samples_of(src, ch, px)
        assert np.array_equal(ps.samples, ref), '%d samples differ' % int((ps.samples != ref).sum())
        assert ps.forms == X.parse(want).forms and ps.sizes == X.parse(want).sizes


def assert_is_model(mgr, src, ch, px):
    """The device's file for the samples is the model's, byte for byte, and within the bound; returns it."""
    data = file_of(encode(mgr, src, ch, px), ch)
    want = X.encode(src, ch, px)
    explain(data, want, src, ch, px)
    assert data == want
    assert 16 + len(data) <= _lib.load().fl_exr_bound(src.shape[1], src.shape[0], ch, px) == X.bound(src.shape[1], src.shape[0], ch, px)
    return data


# ------------------------------------------------------------------ byte for byte with the model
@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_small_frames(mgr, form):
    """1 x 1, a column, a row: one cropped tile, of noise (raw) and of ramps."""
    px, ch = form
    for w, h in XC.small_shapes():
        data = assert_is_model(mgr, XC.noise(w, h, px, 7 * w + h), ch, px)
        assert X.parse(data).nt == 1 and 16 + len(data) == X.bound(w, h, ch, px)
        assert_is_model(mgr, XC.ramps(w, h, w + h), ch, px)


@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_tile_edges(mgr, form):
    """Exactly one full tile; a second tile one pixel wide; a second tile one row high."""
    px, ch = form
    for (w, h), nt in zip(XC.edge_shapes(px), (1, 2, 2)):
        data = assert_is_model(mgr, XC.ramps(w, h, 3 * w + h), ch, px)
        ps = X.parse(data)
        assert ps.nt == nt and 'zip' in ps.forms
        assert X.parse(assert_is_model(mgr, XC.noise(w, h, px, 3 * w + h), ch, px)).forms == ['raw'] * nt


@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_mixed_tiles(mgr, form):
    """131 x 70: a raw tile of noise, compressed ramps, a tile of zeros, a corner tile of 3 x 6 pixels; the same bytes again."""
    px, ch = form
    src = XC.mixed(px, XC.MIXED_SEED[form])
    nt, forms, corner = XC.mixed_properties(X.encode(src, ch, px))
    assert nt == (6 if px == X.HALF else 9) and forms[0] == 'raw' and set(forms[1:]) == {'zip'}      # (the model alone: the seed was chosen on the CPU)
    data = assert_is_model(mgr, src, ch, px)
    assert file_of(encode(mgr, src, ch, px), ch) == data
    ps = X.parse(data)
    assert ps.forms == forms and (ps.tw, ps.th) == (64, X.tile_rows(px))


def test_widest_frame(mgr):
    """65535 x 1 float RGBA: 1024 tiles, every thread of the placement kernel has one; the first and the last tile against the
    model, every sample through the reader."""
    src = XC.ramps(65535, 1, 12)
    src[:, :6400] = XC.noise(6400, 1, X.FLOAT, 12)
    data = file_of(encode(mgr, src, 4, X.FLOAT), 4)
    ps = X.parse(data)
    assert ps.nt == 1024 and (ps.w, ps.h, ps.channels, ps.pixel) == (65535, 1, 4, X.FLOAT)
    assert np.array_equal(ps.samples, X.samples_of(src, 4, X.FLOAT))
    assert ps.forms[:100] == ['raw'] * 100 and set(ps.forms[100:]) == {'zip'}
    raws = X.raw_tiles(src, 4, X.FLOAT)
    assert ps.datas[0] == X.tile_data(raws[0]) and ps.datas[-1] == X.tile_data(raws[-1]) and len(raws[-1]) == 63 * 16
    assert ps.offsets[0] == X.header_bytes(65535, 1, 4, X.FLOAT) + 8 * 1024 == 359 + 8192


def test_tall_frame(mgr):
    for px, ch in ((X.HALF, 3), (X.FLOAT, 4)):
        data = assert_is_model(mgr, XC.ramps(1, 200, 9), ch, px)
        assert X.parse(data).nt == -(-200 // X.tile_rows(px))


@pytest.mark.parametrize('ch', (3, 4))
def test_half_atlas(mgr, ch):
    """Every half value, every midpoint between two of them and the floats beside it, the edges of the range, NaN, the denormals:
    the device's conversion gives the bits of the model's (which the CPU test holds to numpy's)."""
    src = XC.atlas_frame()
    data = file_of(encode(mgr, src, ch, X.HALF), ch)
    ps = X.parse(data)
    assert (ps.w, ps.h, ps.nt) == (256, 1024, 64)
    want = X.to_half(src[:, :, :ch])
    bad = ps.samples != want
    assert not bad.any(), [(float(v), hex(int(g)), hex(int(r))) for v, g, r in zip(src[:, :, :ch][bad][:8], ps.samples[bad][:8], want[bad][:8])]
    assert data == X.encode(src, ch, X.HALF)


@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_source_stride(mgr, form):
    """Rows longer than the frame, sentinels between them: only the frame's pixels reach the file."""
    px, ch = form
    w, h, stride = 70, X.tile_rows(px) + 5, 83
    src = np.full((h, stride, 4), -7777.0, np.float32)
    src[:, :w] = XC.ramps(w, h, 5)
    src[:3, :w] = XC.noise(w, 3, px, 5)
    data = file_of(encode(mgr, src, ch, px, stride=(w,)), ch)
    want = X.encode(np.ascontiguousarray(src[:, :w]), ch, px)
    explain(data, want, np.ascontiguousarray(src[:, :w]), ch, px)
    assert data == want


# ------------------------------------------------------------------ capacity, destinations, bad arguments
def test_capacity(mgr):
    src = XC.mixed(X.HALF, XC.MIXED_SEED[(X.HALF, 4)])
    h, w, _ = src.shape
    data = file_of(encode(mgr, src, 4, X.HALF), 4)
    need, tb = len(data), X.tile_bytes(4)
    buf = encode(mgr, src, 4, X.HALF, cap=16 + need)          # (encode checks the sentinel at and beyond cap)
    assert record(buf) == (need, 0, tb) and file_of(buf, 4) == data
    for cap in (16 + need - 1, 16 + X.header_bytes(w, h, 4, X.HALF) + 8 * 6):
        buf = encode(mgr, src, 4, X.HALF, cap=cap)
        assert record(buf) == (need, 1, tb)
        assert (buf[16:] == SENTINEL).all()                   # nothing behind the record


def test_pageable_memory(mgr):
    src = XC.mixed(X.FLOAT, XC.MIXED_SEED[(X.FLOAT, 3)])
    cap = _lib.load().fl_exr_bound(src.shape[1], src.shape[0], 3, X.FLOAT)
    buf = encode(mgr, src, 3, X.FLOAT, buf=np.empty(cap + SLACK, np.uint8))
    assert file_of(buf, 3) == X.encode(src, 3, X.FLOAT)


def test_device_destination_at_an_odd_address(mgr):
    import torch
    lib = _lib.load()
    src = XC.mixed(X.HALF, XC.MIXED_SEED[(X.HALF, 3)])
    h, w, _ = src.shape
    want = X.encode(src, 3, X.HALF)
    cap = 16 + len(want) + 7
    t = upload(mgr, src.view(np.uint8))
    out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device=t.device)
    host = mgr.fb._pinned((cap,), 'u1')
    host[:] = SENTINEL
    torch.cuda.synchronize(mgr.fb.device)
    _lib.check(lib.fl_exr_encode(mgr.fb.ctx, w, h, t.data_ptr(), w, 3, X.HALF, host.ctypes.data, out.data_ptr() + 1, cap))      # both destinations
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    dev = out.cpu().numpy()
    assert dev[0] == SENTINEL and (dev[1 + cap:] == SENTINEL).all() and file_of(dev[1:], 3) == want
    assert file_of(host, 3) == want


def test_bad_arguments(mgr):
    lib = _lib.load()
    w, h = 37, 10
    src = XC.ramps(w, h, 4)
    want = X.encode(src, 4, X.HALF)
    t = upload(mgr, src.view(np.uint8))
    cap = lib.fl_exr_bound(w, h, 4, X.HALF)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    ctx, sp, dst = mgr.fb.ctx, t.data_ptr(), buf.ctypes.data
    assert lib.fl_exr_bound(20000, 65535, 4, X.HALF) == 0 == lib.fl_exr_bound(20000, 65535, 3, X.FLOAT)
    # (w, h, src, stride, channels, pixel, host, dev, cap)
    bad = [(0, h, sp, w, 4, 1, dst, 0, cap), (w, 0, sp, w, 4, 1, dst, 0, cap), (65536, h, sp, 65536, 4, 1, dst, 0, cap), (w, 65536, sp, w, 4, 1, dst, 0, cap),
           (w, h, sp, w, 2, 1, dst, 0, cap), (w, h, sp, w, 5, 1, dst, 0, cap), (w, h, sp, w, 0, 1, dst, 0, cap),
           (w, h, sp, w, 4, 0, dst, 0, cap), (w, h, sp, w, 4, 3, dst, 0, cap), (w, h, sp, w, 4, 16, dst, 0, cap),
           (20000, 65535, sp, 20000, 4, 1, dst, 0, cap),                   # a frame whose fl_exr_bound is 0: beyond 2^32 - 1
           (w, h, 0, w, 4, 1, dst, 0, cap), (w, h, sp, w - 1, 4, 1, dst, 0, cap), (w, h, sp, 0, 4, 1, dst, 0, cap), (w, h, sp, w, 4, 1, None, 0, cap),
           (w, h, sp, w, 4, 1, dst, 0, 16 + X.header_bytes(w, h, 4, X.HALF) + 8 - 1)]
    for args in bad:
        buf[:] = SENTINEL
        assert lib.fl_exr_encode(ctx, *args) == _lib.FL_E_INVAL, args
        assert lib.fl_last_error()
        if args[2] and args[3] >= args[0]:
            assert lib.fl_output_exr(ctx, *(args[:2] + args[4:])) == _lib.FL_E_INVAL, args
        _lib.check(lib.fl_ctx_sync(ctx))
        assert (buf == SENTINEL).all()
        _lib.check(lib.fl_exr_encode(ctx, w, h, sp, w, 4, 1, dst, 0, cap))      # ... and the next frame is still right
        _lib.check(lib.fl_ctx_sync(ctx))
        assert file_of(buf, 4) == want and (buf[cap:] == SENTINEL).all()


def test_encode_is_timed(mgr):
    """The encode's kernels are in slot 5 of fl_timings_detail, like the other encoders'."""
    _lib.check(_lib.load().fl_timings_reset(mgr.fb.ctx))
    assert mgr.timings()['encode_ms'] == 0.0
    encode(mgr, XC.ramps(70, 70, 2), 3, X.HALF)
    assert mgr.timings()['encode_ms'] > 0.0


# ------------------------------------------------------------------ the front buffer in place
def read_seeds(mgr):
    return mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)


def crop(front, dim):
    g = render.Framebuffers.gutter
    return np.ascontiguousarray(front.reshape(dim.ah, dim.astride, 4)[g:g + dim.h, g:g + dim.w])


def output_exr(mgr, w, h, ch, px):
    lib = _lib.load()
    cap = lib.fl_exr_bound(w, h, ch, px)
    buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    _lib.check(lib.fl_output_exr(mgr.fb.ctx, w, h, ch, px, buf.ctypes.data, 0, cap))
    return buf, cap


@pytest.mark.parametrize('size', ((40, 8), (200, 120)), ids=('40x8', '200x120'))
def test_output_reads_the_front_buffer_in_place(mgr, size):
    """fl_output_exr: the crop of the front buffer bit for bit at float, to_half of it at half; values below 0 and above 1, a NaN
    and an infinity arrive; the gutter never does; no dither draw; the frame is closed."""
    lib = _lib.load()
    w, h = size
    dim = mgr.fb.set_dim(w, h)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(mgr.fb.ctx, C.byref(fid)))      # first: a frame chooses the lane whose buffers the calls below use
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, w, h, 0))
    rs = np.random.RandomState(w)
    front = np.full((dim.ah, dim.astride, 4), -31337.0, np.float32)      # the gutter: a value the picture does not hold
    pic = (rs.rand(h, w, 4) * 6.0 - 2.0).astype(np.float32)
    pic[1, 2, 0], pic[2, 3, 1], pic[3, 4, 2], pic[0, 0, 3] = np.nan, np.inf, -np.inf, 70000.0
    g = render.Framebuffers.gutter
    front[g:g + h, g:g + w] = pic
    import torch
    from cuburn_amd import distributed
    acc = distributed.accumulator_tensor(mgr.fb, mgr.fb.device, dim)      # fl_buffer_ptr(FL_BUF_FRONT): the buffer itself, as a tensor
    assert acc.numel() == front.size
    acc.copy_(torch.from_numpy(front.reshape(-1)))
    torch.cuda.synchronize(mgr.fb.device)
    assert np.nanmin(pic) < -1.0 and pic[np.isfinite(pic)].max() > 3.0
    before = read_seeds(mgr)
    for px in (X.FLOAT, X.HALF):
        for ch in (3, 4):
            buf, cap = output_exr(mgr, w, h, ch, px)
            ms = C.c_float(-1.0)
            _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
            assert ms.value >= 0.0
            _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
            assert (buf[cap:] == SENTINEL).all()
            data = file_of(buf, ch)
            ps = X.parse(data)
            assert (ps.w, ps.h, ps.channels, ps.pixel) == (w, h, ch, px)
            if px == X.FLOAT:
                assert np.array_equal(ps.samples, pic[:, :, :ch].view(np.uint32))
            else:
                assert np.array_equal(ps.samples, X.to_half(pic[:, :, :ch]))
                assert ps.samples[1, 2, 0] == 0 and ps.samples[2, 3, 1] == 0x7bff and ps.samples[3, 4, 2] == 0xfbff
            gutter = np.float32(-31337.0)
            assert not (ps.samples == (gutter.view(np.uint32) if px == X.FLOAT else X.to_half(np.array([gutter]))[0])).any()
            assert data == X.encode(pic, ch, px)
            assert np.array_equal(read_seeds(mgr), before)    # no dither draw
    assert np.array_equal(crop(mgr.fb.read('front', (dim.ah * dim.astride, 4), np.float32), dim).view(np.uint32), pic.view(np.uint32))      # read, not changed


def test_output_flushes_a_deferred_filter_tail(mgr):
    """`bilateral` is deferred until something looks at the buffer: fl_output_exr runs it first."""
    lib = _lib.load()
    w, h = 200, 120
    dim = mgr.fb.set_dim(w, h)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(mgr.fb.ctx, C.byref(fid)))
    rs = np.random.RandomState(3)
    front = (rs.rand(dim.ah * dim.astride, 4) * 3.0 + 0.01).astype(np.float32)
    bil = np.asarray([6.0 * w / 1920., 0.05, 1.5, 0.8, 4.0], np.float32)

    def start():
        _lib.check(lib.fl_debug_clear(mgr.fb.ctx, w, h, 0))
        mgr.fb.write('front', front)
        _lib.check(lib.fl_filter(mgr.fb.ctx, _lib.FILT['bilateral'], dim.w, dim.h, bil.ctypes.data, len(bil)))

    start()
    want = crop(mgr.fb.read('front', front.shape, np.float32), dim)      # (the read flushes, as every look at the buffer does)
    assert np.isfinite(want).all() and not np.array_equal(want, crop(front, dim))
    start()
    buf, cap = output_exr(mgr, w, h, 4, X.FLOAT)
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    ps = X.parse(file_of(buf, 4))
    assert np.array_equal(ps.samples, want.view(np.uint32))


# ------------------------------------------------------------------ through the shim
class _ExrWithFront(output.DeviceEXROutput):
    """The output the profile chose, which first keeps the accumulator the `raw` path would hand on: the front buffer behind the
    filter chain, cropped."""

    def copy(self, fb, dim, **kw):
        _lib.check(_lib.load().fl_ctx_sync(fb.ctx))
        self.front = crop(fb.read('front', (dim.ah * dim.astride, 4), np.float32), dim)
        return output.DeviceEXROutput.copy(self, fb, dim, **kw)


@pytest.mark.parametrize('block', ({'type': 'exr'}, {'type': 'exr', 'pixel': 'float', 'alpha': True}), ids=('half', 'float-alpha'))
def test_through_the_shim(built, block):
    """output: {"type": "exr"} through profile, Renderer and queue_frame: the file decodes to the accumulator's crop."""
    gnm, prof = configs.cfg2(samples=2 ** 22)
    W, Hh = 320, 180
    prof = dict(prof, width=W, height=Hh, spp=2 ** 22 / float(W * Hh), output=block)
    gprof = profile.wrap(prof, gnm)
    m = render.RenderManager(device=0, host_seed=7)
    try:
        rdr = render.Renderer(gnm, gprof)
        assert type(rdr.out) is output.DeviceEXROutput
        assert (rdr.out.alpha, rdr.out.pixel, rdr.out.entry) == (bool(block.get('alpha')), block.get('pixel', 'half'), 'fl_output_exr')
        rdr.out = _ExrWithFront(alpha=rdr.out.alpha, pixel=rdr.out.pixel)
        evt, h_out = m.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
        assert h_out.shape == rdr.out.shape(m.fb.calc_dim(W, Hh)) and h_out.dtype == np.uint8
        media, logs = rdr.out.encode(h_out)
        assert list(media) == ['.exr'] and logs == []
        data, front = media['.exr'].read(), rdr.out.front
    finally:
        m.fb.free()
    ch, px = (4 if block.get('alpha') else 3), _lib.EXR_PIXELS[block.get('pixel', 'half')]
    ps = X.parse(data)
    assert (ps.w, ps.h, ps.channels, ps.pixel) == (W, Hh, ch, px)
    assert front.shape == (Hh, W, 4) and front[:, :, :3].max() > 0.2 and front.std() > 0.01
    assert np.array_equal(ps.samples, X.samples_of(front, ch, px))
    assert data == X.encode(front, ch, px)
    assert 'zip' in ps.forms and len(data) < W * Hh * ch * X.sample_bytes(px)


def test_command_line_writes_an_exr(built, tmp_path):
    """python -m cuburn_amd FLAME --still --codec exr --exr-pixel float, end to end."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    gold = json.load(open(os.path.join(here, 'golden', 'genome_front.json')))
    (tmp_path / 'B.json').write_text(json.dumps(gold['db']['B']))
    out = subprocess.run([sys.executable, '-m', 'cuburn_amd', 'B', '-d', str(tmp_path), '--still', '-P', 'preview', '--codec', 'exr',
                          '--exr-pixel', 'float', '-o', str(tmp_path), '--width', '320', '--height', '180', '--spp', '200'],
                         cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    files = sorted(f for f in os.listdir(str(tmp_path)) if f.endswith('.exr'))
    assert len(files) == 1, (os.listdir(str(tmp_path)), out.stderr[-500:])
    data = open(os.path.join(str(tmp_path), files[0]), 'rb').read()
    ps = X.parse(data)
    assert (ps.w, ps.h, ps.channels, ps.pixel, ps.nt) == (320, 180, 3, X.FLOAT, 5 * 6)
    pic = ps.samples.view(np.float32)
    assert np.isfinite(pic).all() and pic.max() > 0.2 and pic.std() > 0.01
