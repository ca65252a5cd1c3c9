"""
The two device encoders on one lane: they share the lane's scratch and staging buffers (cuburn_amd/csrc/flame_abi.hip,
encode_on), so a JPEG, a PNG that needs about ten times the JPEG's scratch, and the JPEG again are queued back to back with no
wait in between.  The second call regrows the shared buffer while the first's work is queued, the third runs in the larger
one.  Both tests use one context and begin no frame, so every call stays on one lane.  64x40 and 256x96x3 are the smallest
cases of the encoders' own tests for which the regrow and the reuse both happen.
"""
import numpy as np
import pytest

from cuburn_amd import _lib
import encoder_contract as EC
import encoder_harness as H
import jpeg_cases as JC
import png_cases as PC
import png_model as P
from encoder_harness import assert_jpeg_criteria

pytestmark = pytest.mark.gpu


mgr = EC.mgr_fixture()


@pytest.fixture(scope='module')
def inputs(mgr):
    """The two frames (neither depends on the restart interval or the segment length), on the device."""
    planes, quality, _ = JC.case(JC.NOISE_Q100, None)
    rgba, ch, _ = PC.case('smooth_256x96', None)
    assert planes.shape == (3, 40, 64) and rgba.shape == (96, 256, 4) and ch == 3
    return planes, quality, H.upload(mgr, planes), rgba, ch, H.upload(mgr, rgba)


def jpeg_png_jpeg(mgr, inputs, pinned, extra=None):
    """Queue JPEG, PNG, JPEG (and extra(queue_png), if given) into sentinel-filled buffers of their own; one wait at the end.
    Returns the buffers, each checked at and beyond its cap."""
    lib = _lib.load()
    planes, quality, tj, rgba, ch, tp = inputs
    jcap, pcap = lib.fl_jpeg_bound(64, 40), lib.fl_png_bound(256, 96, ch)
    make = (lambda cap: None) if pinned else (lambda cap: np.empty(cap + H.SLACK, np.uint8))
    queue_jpeg = lambda: (H.queue(mgr, 'fl_jpeg_encode', tj, 64, 40, (quality,), jcap, make(jcap)), jcap)
    queue_png = lambda cap=pcap: (H.queue(mgr, 'fl_png_encode', tp, 256, 96, (ch,), cap, make(cap)), cap)
    done = [queue_jpeg(), queue_png(), queue_jpeg()]
    if extra:
        done.append(extra(queue_png))
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    for buf, cap in done:
        H.assert_untouched(buf, cap)
    return [buf for buf, _ in done]


def files_of(bufs):
    out = []
    for buf in bufs:
        nbytes, status, _ = H.record(buf)
        assert status == 0
        out.append(bytes(buf[16:16 + nbytes]))
    return out


@pytest.fixture(scope='module')
def pinned_files(mgr, inputs):
    """The first calls on the context's lane: (JPEG, PNG, JPEG) into pinned memory, and the records' parameters."""
    bufs = jpeg_png_jpeg(mgr, inputs, pinned=True)
    return files_of(bufs), H.record(bufs[0])[2], H.record(bufs[1])[2]


def test_shared_scratch(inputs, pinned_files):
    planes, quality, _, rgba, ch, _ = inputs
    (jpeg_a, png, jpeg_b), ri, seg = pinned_files
    assert png == P.encode(rgba[:, :, :ch], seg)
    assert jpeg_a == jpeg_b
    assert_jpeg_criteria(jpeg_a, planes, quality, ri)


def test_shared_staging(mgr, inputs, pinned_files):
    """Destinations that are not pinned go through the lane's staging buffer: the same regrow and reuse, and the same bytes."""
    want, _, seg = pinned_files
    short = 16 + len(want[1]) - 1
    bufs = jpeg_png_jpeg(mgr, inputs, pinned=False, extra=lambda queue_png: queue_png(short))
    assert files_of(bufs[:3]) == want
    assert H.record(bufs[3]) == (len(want[1]), 1, seg)
