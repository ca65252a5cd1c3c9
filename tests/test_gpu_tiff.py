"""
The device TIFF encoder (cuburn_amd/csrc/tiff.hip; fl_tiff_encode, fl_output_tiff, DeviceTIFFOutput) against the model of
tests/tiff_model.py, which tests/test_cpu_tiff.py holds to Pillow and to its own reader.  Every file is compared byte for byte with
the file the model writes for the same samples; the frames are those of tests/tiff_cases.py, the smallest at which the tiling, the
predictor, the padding and the placement can go wrong.  Then the path through the shim and the command line.  What
fl_tiff_encode and fl_output_tiff share with every encoder's entry points (the capacity rule, the destinations, refused calls,
fl_output_tiff against fl_output, the timing slot) is in the `tiff` and `tiff_8` rows of tests/encoder_contract.py.
"""
import io
import zlib

import numpy as np
import pytest

from cuburn_amd import _lib, output, render
import encoder_contract as EC
import tiff_cases as TC
import tiff_model as T

pytestmark = pytest.mark.gpu
ROW = EC.ROW['tiff']
mgr = EC.mgr_fixture()


def encode(mgr, src, ch, bits):
    """fl_tiff_encode from u8 / u16 [h][w][4] into pinned memory pre-filled with the sentinel; waits, checks the sentinel at and
    beyond cap; returns the buffer."""
    assert src.shape[2] == 4 and src.dtype == TC.dtype_of(bits)
    return EC.encode(mgr, ROW, src, (ch, bits))[0]


def file_of(buf, ch, bits):
    return EC.file_of(ROW, buf, (ch, bits))                  # (status 0, and the record's parameter is the form's tile)


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
    gnm, gprof = EC.small_profile(block)
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
    files = [f for f in EC.run_cli(tmp_path, '--still', '-P', 'preview', '--codec', 'tiff', '--tiff-compression', 'deflate', '--width', '320',
                                   '--height', '180', '--spp', '200') if f.endswith('.tiff')]
    assert len(files) == 1, files
    data = open(files[0], 'rb').read()
    ps = T.parse(data)
    assert (ps.w, ps.h, ps.channels, ps.bits, ps.nt) == (320, 180, 3, 16, 15) and ps.samples.max() > 60 * 257
    assert len(data) < 320 * 180 * 6                          # smaller than the uncompressed samples
    pillow_agrees(data, ps.samples, 3, 16)
