"""
The device WebP encoder (cuburn_amd/csrc/webp.hip; fl_webp_encode, fl_output_webp) and the WebP output against the Python model of
tests/webp_model.py, which tests/test_cpu_webp.py holds to Pillow's libwebp and to its own strict reader: for every frame of
tests/webp_cases.py the device's frame block equals the model's byte for byte — every tile's mode, every code's lengths and header,
every pixel's bits and the padding — and the record says so.  All arithmetic on both sides is integer arithmetic, so there is no
tolerance anywhere.  What fl_webp_encode and fl_output_webp share with every encoder's entry points (the capacity rule, the
destinations, refused calls, fl_output_webp against fl_output(FL_OUT_RGBA8)) is the `webp` row of tests/encoder_contract.py.
"""
import io

import numpy as np
import pytest

from cuburn_amd import encoders, output, render
import encoder_contract as EC
from encoder_harness import SENTINEL, first_difference
import webp_cases as WC
import webp_model as M

pytestmark = pytest.mark.gpu
ROW = EC.ROW['webp']
mgr = EC.mgr_fixture()


def encode(mgr, frame, channels):
    """fl_webp_encode into pinned memory pre-filled with the sentinel; checks the sentinel at and beyond cap."""
    return EC.encode(mgr, ROW, frame, (channels,))


def block_of(buf):
    return EC.file_of(ROW, buf, (4,))                        # (status 0, and the record's parameter is the tile sizes')


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


def test_through_the_shim(built):
    """Three frames of a 96 x 64 config with type webp: a .webp that the model's container reader parses and whose frames, by the
    strict reader and by Pillow, are the `raw` frames of the same times from a manager with the same seed (a manager's frames depend
    on its seed and on the order of its frames only)."""
    times = (0.25, 0.5, 0.75)
    got = {}
    for block in ({'type': 'webp', 'alpha': True, 'loop': 2}, {'type': 'raw'}):
        gnm, gprof = EC.small_profile(block, 96, 64, fps=24)
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
    files = [f for f in EC.run_cli(tmp_path, '-P', 'preview', '--codec', 'webp', '--width', '64', '--height', '48', '--spp', '200', '--fps', '24',
                                   '--duration', '0.125', '--shard', '0.125') if f.endswith('.webp')]
    assert len(files) == 1, files
    parsed = M.read_file(open(files[0], 'rb').read())
    assert parsed['animated'] and (parsed['w'], parsed['h'], parsed['alpha'], parsed['loop']) == (64, 48, False, 0)
    assert parsed['durations'] == M.durations(3, 24)
    seen = [M.decode(blk)[0] for blk in parsed['blocks']]
    assert len(seen) == 3 and seen[0][..., :3].max() > 0 and not np.array_equal(seen[0], seen[1]) and (seen[0][..., 3] == 255).all()
    for blk, pixels in zip(parsed['blocks'], seen):
        assert blk == M.encode(pixels, 3)
    stills = [f for f in EC.run_cli(tmp_path, '-P', 'preview', '--codec', 'webp', '--still', '-n', 'one', '--width', '64', '--height', '48', '--spp', '200')
              if f.endswith('.webp')]
    assert len(stills) == 1, stills
    parsed = M.read_file(open(stills[0], 'rb').read())
    assert not parsed['animated'] and M.decode(parsed['blocks'][0])[0].shape == (48, 64, 4)
