"""
The output conversion kernels (cuburn_amd/csrc/output.hip: k_f32_to_rgba, k_f32_to_yuv) against the C oracle, bit for bit, at the
sizes of tests/output_cases.py: frames in which a dither state serves up to nine pixels, so that the stride of the pixel loops,
every lane of k_f32_to_rgba's four-deep unroll and the order in which a state's draws go to its pixels are all observed — the
two bit-exact tests of tests/test_gpu_parity.py run at 200 x 120, where every state serves at most one pixel.  Compared each
time: the pixels, the dither states afterwards, and the walker and palette states in front of them, which the kernel must not
touch.  The oracle is held to the numpy model of tests/output_model.py by tests/test_cpu_output.py.  No tolerance anywhere.
"""
import numpy as np
import pytest

from common import O
from cuburn_amd import encoders, output, render, _lib
import output_cases as OC
import output_model as OM

pytestmark = pytest.mark.gpu

NSLOTS = 1024
RESTORE = (200, 120)                 # the size tests/test_gpu_parity.py leaves its manager at
POISON = 0xA5                        # what a destination holds before the call


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=NSLOTS, host_seed=42)
    assert m.fb.nout == OC.NOUT
    yield m
    m.fb.set_dim(*RESTORE)
    _lib.check(_lib.load().fl_debug_clear(m.fb.ctx, RESTORE[0], RESTORE[1], 0))
    _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))


def first_dither_state(mgr):
    """The seed table is walkers | 64 palette rows of 256 | NOUT dither states."""
    first = mgr.fb.nslots * mgr.fb.nthreads + 64 * 256
    assert mgr.fb.nwalkers - first == OC.NOUT
    return first


def read_seeds(mgr):
    return mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)


def load_frame(mgr, w, h):
    """Size the context for w x h and put the case's buffer into `front`; returns (dim, oracle dim, buffer)."""
    d, buf = OC.frame(w, h)
    dim = mgr.fb.set_dim(w, h)
    assert (dim.w, dim.h, dim.ah, dim.astride) == (d.w, d.h, d.ah, d.astride)
    _lib.check(_lib.load().fl_debug_clear(mgr.fb.ctx, dim.w, dim.h, 0))
    mgr.fb.write('front', buf)
    return dim, d, buf


def poisoned(w, h, fmt):
    out = OM.empty_output(w, h, fmt)
    out.view(np.uint8)[...] = POISON
    return out


def convert(mgr, w, h, fmt, host=True, dev=None):
    """fl_output into a poisoned host array (and / or the device tensor `dev`), synchronised; returns the host array."""
    lib = _lib.load()
    out = poisoned(w, h, fmt) if host else None
    assert lib.fl_output_bytes(w, h, fmt) == OM.empty_output(w, h, fmt).nbytes
    _lib.check(lib.fl_output(mgr.fb.ctx, w, h, fmt, out.ctypes.data if host else None, dev.data_ptr() if dev is not None else 0))
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    return out


def assert_states(before, after, ref_after, first, what):
    assert np.array_equal(after[first:], ref_after), '%s: %d dither states differ' % (what, int((after[first:] != ref_after).any(1).sum()))
    assert np.array_equal(after[:first], before[:first]), '%s: walker / palette states changed' % (what,)


# ------------------------------------------------------------------ 1. every size x format
@pytest.mark.parametrize('case', OC.cases(), ids=OC.case_id)
def test_output_equals_oracle(mgr, case):
    w, h, fmt = case
    dim, d, buf = load_frame(mgr, w, h)
    first = first_dither_state(mgr)
    before = read_seeds(mgr)
    out = convert(mgr, w, h, fmt)
    after = read_seeds(mgr)
    ref, ref_after = O.f32_to_rgba(d, buf, before[first:], fmt)
    assert out.shape == ref.shape and out.dtype == ref.dtype
    assert np.array_equal(out, ref), '%d of %d values differ' % (int((out != ref).sum()), ref.size)
    assert_states(before, after, ref_after, first, OC.case_id(case))


# ------------------------------------------------------------------ 2. two frames in a row
def test_second_frame_continues_from_the_first(mgr):
    """rgba8, then 4:2:0 with nothing in between: the second call starts from the states the first left."""
    w, h = OC.TWO_FRAMES
    dim, d, buf = load_frame(mgr, w, h)
    first = first_dither_state(mgr)
    before = read_seeds(mgr)
    out_a = convert(mgr, w, h, OM.RGBA8)
    mid = read_seeds(mgr)
    out_b = convert(mgr, w, h, OM.YUV420P10)
    after = read_seeds(mgr)
    ref_a, rng_a = O.f32_to_rgba(d, buf, before[first:], OM.RGBA8)
    ref_b, rng_b = O.f32_to_rgba(d, buf, rng_a, OM.YUV420P10)
    assert np.array_equal(out_a, ref_a)
    assert_states(before, mid, rng_a, first, 'first frame')
    assert np.array_equal(out_b, ref_b)
    assert_states(before, after, rng_b, first, 'second frame')
    assert not np.array_equal(rng_a, rng_b)


# ------------------------------------------------------------------ 3. the dev_out path
@pytest.mark.parametrize('fmt', [OM.RGBA8, OM.YUV420P10])
def test_device_destination(mgr, fmt):
    """The frame straight into a device tensor of the caller: with host_out = NULL the tensor holds the oracle's frame, with both
    destinations both do; all three calls start from the same states."""
    import torch
    w, h = OC.TWO_FRAMES
    dim, d, buf = load_frame(mgr, w, h)
    first = first_dither_state(mgr)
    start = read_seeds(mgr)
    ref, ref_after = O.f32_to_rgba(d, buf, start[first:], fmt)

    def tensor():
        t = torch.full((ref.nbytes,), POISON, dtype=torch.uint8, device='cuda:%d' % mgr.fb.device)
        torch.cuda.synchronize(mgr.fb.device)                # torch's stream is not the context's
        return t

    def frame_of(t):
        return t.cpu().numpy().view(ref.dtype).reshape(ref.shape)

    own = convert(mgr, w, h, fmt)                             # the context's own pixel buffer, for comparison
    assert np.array_equal(own, ref)
    assert_states(start, read_seeds(mgr), ref_after, first, 'host only')

    mgr.fb.write('seeds', start)
    t = tensor()
    assert convert(mgr, w, h, fmt, host=False, dev=t) is None
    assert np.array_equal(frame_of(t), ref)
    assert_states(start, read_seeds(mgr), ref_after, first, 'device only')

    mgr.fb.write('seeds', start)
    t = tensor()
    both = convert(mgr, w, h, fmt, host=True, dev=t)
    assert np.array_equal(frame_of(t), ref) and np.array_equal(both, ref)
    assert_states(start, read_seeds(mgr), ref_after, first, 'host and device')


# ------------------------------------------------------------------ 4. the Output classes
OUTPUTS = [
    ('Output', lambda: output.Output(), OM.RGBA8),
    ('TiffOutput', lambda: output.TiffOutput(), OM.RGBA16),
    ('VPxOutput yuv444p', lambda: encoders.VPxOutput(codec='vp9', pix_fmt='yuv444p'), OM.YUV444P),
    ('VPxOutput yuv444p10', lambda: encoders.VPxOutput(codec='vp9', pix_fmt='yuv444p10'), OM.YUV444P10),
    ('VPxOutput yuv420p10', lambda: encoders.VPxOutput(codec='vp9', pix_fmt='yuv420p10'), OM.YUV420P10),
    ('ProResOutput', lambda: encoders.ProResOutput(), OM.YUV444P12),
]


@pytest.mark.parametrize('name,make,fmt', OUTPUTS, ids=[o[0] for o in OUTPUTS])
def test_output_classes(mgr, name, make, fmt):
    """out.copy(fb, dim) returns an array of out.shape(dim) and out.dtype that holds the oracle's frame for out.fmt."""
    w, h = OC.TWO_FRAMES
    dim, d, buf = load_frame(mgr, w, h)
    first = first_dither_state(mgr)
    before = read_seeds(mgr)
    out = make()
    assert out.fmt == fmt
    h_out = out.copy(mgr.fb, dim)
    _lib.check(_lib.load().fl_ctx_sync(mgr.fb.ctx))
    after = read_seeds(mgr)
    ref, ref_after = O.f32_to_rgba(d, buf, before[first:], out.fmt)
    assert h_out.shape == tuple(out.shape(dim)) == ref.shape and h_out.dtype == np.dtype(out.dtype) == ref.dtype
    assert np.array_equal(h_out, ref)
    assert_states(before, after, ref_after, first, name)
