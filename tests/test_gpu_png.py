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

Then the path through the shim and the command line.  What fl_png_encode and fl_output_png share with every encoder's entry
points (the capacity rule, refused calls, pageable and device destinations, fl_output_png against fl_output(FL_OUT_RGBA8)) is the
`png` row of tests/encoder_contract.py.
"""
import functools
import io

import numpy as np
import pytest

from cuburn_amd import _lib, output, render
import encoder_contract as EC
from encoder_harness import assert_png_criteria as assert_criteria, record
import png_cases as PC
import png_model as P

pytestmark = pytest.mark.gpu
ROW = EC.ROW['png']
mgr = EC.mgr_fixture()
file_of = functools.partial(EC.file_of, ROW)


def encode(mgr, rgba, ch):
    """fl_png_encode into pinned memory pre-filled with the sentinel; returns (buffer, cap)."""
    return EC.encode(mgr, ROW, rgba, (ch,))                  # (checks the sentinel at and beyond cap)


@pytest.fixture(scope='module')
def device_seg(mgr):
    """The library's segment length, from the record of a one-pixel frame."""
    return EC.param_of(mgr, ROW)


_done = {}


def encoded_case(mgr, name, seg):
    """(rgba, channels, check, file, buffer) of a case, encoded once per session."""
    if name not in _done:
        rgba, ch, check = PC.case(name, seg)
        buf, _ = encode(mgr, rgba, ch)
        _done[name] = (rgba, ch, check, file_of(buf), buf)
    return _done[name]


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


def test_bound(mgr, device_seg):
    lib = _lib.load()
    for w, h, ch in ((0, 8, 3), (8, 0, 3), (65536, 8, 3), (8, 65536, 3), (8, 8, 1), (8, 8, 5), (65535, 65535, 4)):
        assert lib.fl_png_bound(w, h, ch) == 0
    for w, h, ch in ((1, 1, 3), (1920, 1080, 3), (1920, 1080, 4), (8000, 65535, 4)):
        assert lib.fl_png_bound(w, h, ch) == PC.bound(w, h, ch, device_seg)


@pytest.mark.parametrize('alpha', (False, True))
def test_through_the_shim(built, alpha):
    PIL_Image = pytest.importorskip('PIL.Image')
    block = {'type': 'png', 'encoder': 'device'}
    if alpha:
        block['alpha'] = True
    gnm, gprof = EC.small_profile(block)
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
    PIL_Image = pytest.importorskip('PIL.Image')
    files = [f for f in EC.run_cli(tmp_path, '--still', '-P', 'preview', '--codec', 'png', '--device-encode', '--width', '320', '--height', '180',
                                   '--spp', '200') if f.endswith('.png')]
    assert len(files) == 1, files
    data = open(files[0], 'rb').read()
    ps = P.parse(data)
    assert (ps.w, ps.h, ps.channels) == (320, 180, 3) and ps.filters == [4] * 180 and ps.stats['distances'] in ([], [1])
    assert len(ps.idat) == -(-len(ps.filtered) // 32768) or len(ps.idat) > 1
    im = PIL_Image.open(io.BytesIO(data))
    assert im.size == (320, 180) and im.mode == 'RGB' and np.array_equal(np.asarray(im), ps.pixels) and ps.pixels.max() > 60
