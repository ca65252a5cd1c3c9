"""
The device GIF encoder (cuburn_amd/csrc/gif.hip; fl_gif_encode, fl_output_gif) and the GIF output against the Python model of
tests/gif_model.py, which tests/test_cpu_gif.py holds to Pillow and to its own strict reader: for every frame of tests/gif_cases.py
the device's frame block equals the model's byte for byte — histogram, cut, palette, lookup, dither, every LZW code and width, the
segments' padding, the sub-blocks — and the record says so.  All arithmetic on both sides is integer arithmetic, so there is no
tolerance anywhere.  What fl_gif_encode and fl_output_gif share with every encoder's entry points (the capacity rule, the
destinations, refused calls, fl_output_gif against fl_output(FL_OUT_RGBA8)) is the `gif` row of tests/encoder_contract.py.
"""
import io

import numpy as np
import pytest

from cuburn_amd import _lib, encoders, output, render
import encoder_contract as EC
from encoder_harness import SENTINEL, first_difference, record
import gif_cases as GC
import gif_model as M

pytestmark = pytest.mark.gpu
ROW = EC.ROW['gif']
mgr = EC.mgr_fixture()


def encode(mgr, frame, colors, amp):
    """fl_gif_encode into pinned memory pre-filled with the sentinel; checks the sentinel at and beyond cap."""
    return EC.encode(mgr, ROW, frame, (colors, amp))


def block_of(buf, seg=M.SEG):
    return EC.file_of(ROW, buf, param=seg)                   # (status 0, and the record's parameter is the segment)


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


def test_through_the_shim(built):
    """Three frames of a 64 x 48 config with type gif: a .gif whose blocks are the model's blocks of the `raw` frames of the same
    times from a manager with the same seed (a manager's frames depend on its seed and on the order of its frames only)."""
    times = (0.25, 0.5, 0.75)
    got = {}
    for block in ({'type': 'gif', 'colors': 32, 'loop': 2}, {'type': 'raw'}):
        gnm, gprof = EC.small_profile(block, fps=24)
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
    files = [f for f in EC.run_cli(tmp_path, '-P', 'preview', '--codec', 'gif', '--gif-colors', '64', '--width', '64', '--height', '48', '--spp', '200',
                                   '--fps', '24', '--duration', '0.125', '--shard', '0.125') if f.endswith('.gif')]
    assert len(files) == 1, files
    data = open(files[0], 'rb').read()
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
