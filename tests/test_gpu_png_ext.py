"""
The device PNG encoder's extended forms (cuburn_amd/csrc/png.hip; fl_png_encode_f, fl_output_png_f, DevicePNGOutput with bits /
filter) against the model of tests/png_ext_model.py, which tests/test_cpu_png_ext.py holds to zlib and Pillow: 16-bit samples and a
filter type per row.  Every file is compared byte for byte with the file the model writes for the same pixels, with the segment
length the device's record reports; the frames are those of tests/png_ext_cases.py, the smallest at which the filter stage can go
wrong.  Then the default form against fl_png_encode, and the path through the shim.  What fl_png_encode_f and fl_output_png_f
share with every encoder's entry points (the capacity rule, the destinations, refused calls, fl_output_png_f against
fl_output(FL_OUT_RGBA16)) is in the `png_f_paeth` and `png_f_adaptive` rows of tests/encoder_contract.py.
"""
import functools
import io

import numpy as np
import pytest

from cuburn_amd import _lib, output, render
import encoder_contract as EC
from encoder_harness import record
import png_ext_cases as XC
import png_ext_model as X
import png_model as P

pytestmark = pytest.mark.gpu
ROW = EC.ROW['png_f_adaptive']
mgr = EC.mgr_fixture()
file_of = functools.partial(EC.file_of, ROW)


def encode_f(mgr, src, ch, bits, flags):
    """fl_png_encode_f from u8 / u16 [h][w][4] into pinned memory pre-filled with the sentinel; waits, checks the sentinel at and
    beyond cap; returns the buffer."""
    assert src.shape[2] == 4 and src.dtype == (np.uint8 if bits == 8 else np.uint16)
    return EC.encode(mgr, ROW, src, (ch, bits, flags))[0]


@pytest.fixture(scope='module')
def device_seg(mgr):
    """The library's segment length, from the record of a one-pixel frame."""
    return EC.param_of(mgr, ROW)


def assert_is_model(mgr, img, ch, bits, flags, seg):
    """The device's file for the byte image is the model's, byte for byte, and within the bound; returns it."""
    src = XC.source(img, ch, bits)
    buf = encode_f(mgr, src, ch, bits, flags)
    assert record(buf)[2] == seg
    data = file_of(buf)
    want = X.encode(src, ch, bits, flags, seg)
    if data != want:                                          # say where before failing
        ps = X.parse(data, seg)
        _, types = X.filter_stream(img, flags)
        assert (ps.bits, ps.channels, ps.w, ps.h) == (bits, ch, img.shape[1], img.shape[0])
        assert ps.filters == types, 'filter types %r, the model chooses %r' % (ps.filters, types)
        assert np.array_equal(ps.bytes, img), '%d bytes differ' % int((ps.bytes != img).sum())
    assert data == want
    assert 16 + len(data) <= _lib.load().fl_png_bound_f(img.shape[1], img.shape[0], ch, bits, flags) == X.bound(img.shape[1], img.shape[0], ch, bits, seg)
    return data


# ------------------------------------------------------------------ byte for byte with the model
@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_small_frames(mgr, device_seg, form):
    """1 x 1; w = 1 (a and c are always 0); h = 1 (no row above)."""
    bits, ch, flags = form
    for w, h in ((1, 1), (1, 7), (7, 1)):
        assert_is_model(mgr, XC.noise(w, h, X.bpp_of(ch, bits), 7 * w + h), ch, bits, flags, device_seg)


@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_ten_band(mgr, device_seg, form):
    """Every filter type and the five-way tie, at every rowlen mod 4."""
    bits, ch, flags = form
    for w in XC.TEN_BAND_W:
        data = assert_is_model(mgr, XC.ten_band(w, X.bpp_of(ch, bits)), ch, bits, flags, device_seg)
        ps = X.parse(data, device_seg)
        assert set(ps.filters) == ({0, 1, 2, 3, 4} if flags else {4}) and (not flags or ps.filters[XC.ROW_TIE] == 0)
        if form == XC.FORMS[-1] and w == 40:
            assert file_of(encode_f(mgr, XC.source(XC.ten_band(w, 8), ch, bits), ch, bits, flags)) == data      # the same bytes again


def test_ten_band_wide(mgr, device_seg):
    """700 pixels: the choice kernel's loop runs more than once and its sums cross waves."""
    data = assert_is_model(mgr, XC.ten_band(700, 8), 4, 16, X.ADAPTIVE, device_seg)
    assert set(X.parse(data, device_seg).filters) == {0, 1, 2, 3, 4}


def test_widest_row(mgr, device_seg):
    """65535 x 2 RGBA16 of noise: the longest row there is; 32-bit costs and addresses."""
    img = XC.noise(65535, 2, 8, 12)
    src = XC.source(img, 4, 16)
    buf = encode_f(mgr, src, 4, 16, X.ADAPTIVE)
    assert file_of(buf) == X.encode(src, 4, 16, X.ADAPTIVE, device_seg)


@pytest.mark.parametrize('form', XC.FORMS, ids=XC.form_id)
def test_segments(mgr, device_seg, form):
    """At least three segments whose boundaries fall inside rows, dynamic blocks among them."""
    bits, ch, flags = form
    w, h = XC.soft_shape(device_seg, X.bpp_of(ch, bits))
    data = assert_is_model(mgr, XC.soft(w, h, ch, bits, 3), ch, bits, flags, device_seg)
    ps = X.parse(data, device_seg)
    assert len(ps.idat) >= 3 and any(b['type'] == 2 for b in ps.blocks)
    PIL_Image = pytest.importorskip('PIL.Image')
    im = np.asarray(PIL_Image.open(io.BytesIO(data)))
    assert np.array_equal(im, ps.pixels if bits == 8 else (ps.pixels >> 8).astype(np.uint8))


@pytest.mark.parametrize('ch', (3, 4))
@pytest.mark.parametrize('flags', (0, X.ADAPTIVE))
def test_byte_order(mgr, device_seg, ch, flags):
    src = XC.byte_order_source()
    buf = encode_f(mgr, src, ch, 16, flags)
    data = file_of(buf)
    assert data == X.encode(src, ch, 16, flags, device_seg)
    ps = X.parse(data, device_seg)
    assert np.array_equal(ps.pixels, src[:, :, :ch]) and ps.bytes[0, 0].tolist()[:6] == [0x00, 0xff, 0xff, 0x00, 0x01, 0x00]


def test_default_form_is_fl_png_encode(mgr, device_seg):
    img = XC.ten_band(37, 4)
    for ch in (3, 4):
        src = XC.source(img[:, :, :ch], ch, 8)
        old, _ = EC.encode(mgr, EC.ROW['png'], src, (ch,))
        new = encode_f(mgr, src, ch, 8, 0)
        assert file_of(new) == file_of(old) == P.encode(src[:, :, :ch], device_seg) and record(new) == record(old)


# ------------------------------------------------------------------ through the shim
class _WithRaw16(output.DevicePNGOutput):
    """The output the profile chose, which also takes the raw16 output of the same frame from the same seeds: fl_output(FL_OUT_RGBA16)
    first, the dither states put back, then the device PNG.  (Two managers of one seed do not serve: the accumulator's float sums
    depend on the order of its atomic adds, and two renders of one frame differ by one unit in about a thousandth of the 16-bit
    samples, raw16 against raw16 included.)"""

    def copy(self, fb, dim, **kw):
        lib = _lib.load()
        _lib.check(lib.fl_ctx_sync(fb.ctx))
        seeds = fb.read('seeds', (fb.nwalkers, 3), np.uint32)
        raw = output.Raw16Output().copy(fb, dim)
        _lib.check(lib.fl_ctx_sync(fb.ctx))
        self.raw16 = np.array(raw)
        assert not np.array_equal(fb.read('seeds', (fb.nwalkers, 3), np.uint32), seeds)
        fb.write('seeds', seeds)
        return output.DevicePNGOutput.copy(self, fb, dim, **kw)


@pytest.mark.parametrize('alpha', (False, True))
def test_through_the_shim(built, alpha):
    """output: {"type": "png", "encoder": "device", "bits": 16, "filter": "adaptive"} through profile, Renderer and queue_frame: the
    file decodes to exactly the raw16 output of the same frame and seeds, and is the file the model writes for it."""
    block = {'type': 'png', 'encoder': 'device', 'bits': 16, 'filter': 'adaptive'}
    if alpha:
        block['alpha'] = True
    gnm, gprof = EC.small_profile(block)
    m = render.RenderManager(device=0, host_seed=7)
    try:
        rdr = render.Renderer(gnm, gprof)
        assert type(rdr.out) is output.DevicePNGOutput
        assert (rdr.out.alpha, rdr.out.bits, rdr.out.filter, rdr.out.entry) == (alpha, 16, 'adaptive', 'fl_output_png_f')
        rdr.out = _WithRaw16(alpha=rdr.out.alpha, bits=rdr.out.bits, filter=rdr.out.filter)
        evt, h_out = m.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
        assert h_out.shape == rdr.out.shape(m.fb.calc_dim(64, 48)) and h_out.dtype == np.uint8
        media, logs = rdr.out.encode(h_out)
        assert list(media) == ['.png'] and logs == []
        data, seg, raw = media['.png'].read(), record(h_out)[2], rdr.out.raw16
    finally:
        m.fb.free()
    ch = 4 if alpha else 3
    ps = X.parse(data, seg)
    assert (ps.w, ps.h, ps.channels, ps.bits) == (64, 48, ch, 16) and ps.pixels[:, :, :3].max() > 255
    assert raw.shape == (48, 64, 4) and raw.dtype == np.uint16 and (raw & 255).std() > 10
    assert np.array_equal(ps.pixels, raw[:, :, :ch])
    assert data == X.encode(raw, ch, 16, X.ADAPTIVE, seg)
    PIL_Image = pytest.importorskip('PIL.Image')
    im = PIL_Image.open(io.BytesIO(data))
    assert im.size == (64, 48) and im.mode == ('RGBA' if alpha else 'RGB')
    assert np.array_equal(np.asarray(im), (ps.pixels >> 8).astype(np.uint8))
