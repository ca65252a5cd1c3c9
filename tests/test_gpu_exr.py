"""
The device OpenEXR encoder (cuburn_amd/csrc/exr.hip; fl_exr_encode, fl_output_exr, DeviceEXROutput) against the model of
tests/exr_model.py, which tests/test_cpu_exr.py holds to numpy's float16 and to its own reader.  Every file is compared byte for
byte with the file the model writes for the same samples; the frames are those of tests/exr_cases.py, the smallest at which the
conversion, the cropped tiles, the two data forms and the placement can go wrong.  Then the source's stride, fl_output_exr on the
front buffer in place, and the path through the shim.  What fl_exr_encode and fl_output_exr share with every encoder's entry points
(the capacity rule, the destinations, refused calls, the timing slot) is the `exr` row of tests/encoder_contract.py.
"""
import ctypes as C

import numpy as np
import pytest

from cuburn_amd import _lib, output, render
import encoder_contract as EC
import encoder_harness as H
from encoder_harness import SENTINEL, SLACK
import exr_cases as XC
import exr_model as X

pytestmark = pytest.mark.gpu
ROW = EC.ROW['exr']
mgr = EC.mgr_fixture()


def encode(mgr, src, ch, px, stride=None):
    """fl_exr_encode from f32 [h][stride][4] into pinned memory pre-filled with the sentinel; waits, checks the sentinel at and beyond
    cap; returns the buffer.  `src` is [h][w][4] unless `stride` says its rows are longer than the frame's."""
    h, sw, _ = src.shape
    w = sw if stride is None else stride[0]
    assert src.shape[2] == 4 and src.dtype == np.float32
    cap = _lib.load().fl_exr_bound(w, h, ch, px)
    assert cap
    return H.encode(mgr, 'fl_exr_encode', np.ascontiguousarray(src).view(np.uint8), w, h, (sw, ch, px), cap)[0]


def file_of(buf, ch):
    return EC.file_of(ROW, buf, (0, ch, 0))                  # (status 0, and the record's parameter is the channel count's tile)


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
    W, Hh = 320, 180
    gnm, gprof = EC.small_profile(block, W, Hh)
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
    files = [f for f in EC.run_cli(tmp_path, '--still', '-P', 'preview', '--codec', 'exr', '--exr-pixel', 'float', '--width', '320', '--height', '180',
                                   '--spp', '200') if f.endswith('.exr')]
    assert len(files) == 1, files
    data = open(files[0], 'rb').read()
    ps = X.parse(data)
    assert (ps.w, ps.h, ps.channels, ps.pixel, ps.nt) == (320, 180, 3, X.FLOAT, 5 * 6)
    pic = ps.samples.view(np.float32)
    assert np.isfinite(pic).all() and pic.max() > 0.2 and pic.std() > 0.01
