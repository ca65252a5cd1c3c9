"""
What the GPU tests of the device encoders share (test_gpu_jpeg.py, test_gpu_jpeg_opt.py, test_gpu_mjpeg.py, test_gpu_png.py,
test_gpu_png_ext.py, test_gpu_tiff.py, test_gpu_exr.py, test_gpu_gif.py, test_gpu_webp.py, test_gpu_encoders_shared.py):
destinations pre-filled with a sentinel, the call of an encoder's fl_X_encode, and the 16-byte record in front of the file.
"""
import numpy as np

from cuburn_amd import _lib
import jpeg_model as J

SENTINEL = 0xA5
SLACK = 4096                  # sentinel bytes the tests keep behind a capacity
EPS = 2.0 ** -8               # the float32 DCT's error bound, derived in tests/test_gpu_jpeg.py


def upload(mgr, arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).to('cuda:%d' % mgr.fb.device)
    torch.cuda.synchronize(mgr.fb.device)
    return t


def record(buf):
    """(nbytes, status, param) of the record; param is the restart interval (JPEG) or the segment's bytes (PNG)."""
    nbytes, status, param, zero = (int(v) for v in np.frombuffer(buf[:16], '<u4'))
    assert zero == 0
    return nbytes, status, param


def queue(mgr, entry, t, w, h, args, cap, buf=None):
    """Queue the library's `entry`, fl_X_encode(ctx, w, h, src, *args, host_out, dev_out, cap), from the device tensor `t` into
    pinned memory (or `buf`) pre-filled with the sentinel; no wait.  `args` is the tuple of the entry point's middle arguments
    (exr's src_stride is its first).  Returns the buffer, which holds cap + SLACK bytes unless the caller brought it."""
    if buf is None:
        buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    _lib.check(getattr(_lib.load(), entry)(mgr.fb.ctx, w, h, t.data_ptr(), *args, buf.ctypes.data, 0, cap))
    return buf


def assert_untouched(buf, cap):
    assert (buf[cap:] == SENTINEL).all(), 'bytes at or beyond cap were written'


def encode(mgr, entry, src, w, h, args, cap, buf=None):
    """Upload `src`, queue(), wait, and check the sentinel at and beyond cap; returns (buffer, cap)."""
    t = upload(mgr, src)
    buf = queue(mgr, entry, t, w, h, args, cap, buf)
    _lib.check(_lib.load().fl_ctx_sync(mgr.fb.ctx))
    assert_untouched(buf, cap)
    return buf, cap


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return 'lengths %d and %d, first difference at %s' % (len(a), len(b), int(d[0]) if len(d) else 'none below %d' % n)


def assert_jpeg_criteria(data, planes, quality, ri):
    """A, B and C of tests/test_gpu_jpeg.py for a stream; returns the parse."""
    ps = J.parse(data)                                                              # A
    qt = J.quant_tables(quality)
    assert (ps.w, ps.h) == (planes.shape[2], planes.shape[1]) and ps.restart_interval == ri, (ps.w, ps.h, ps.restart_interval, planes.shape, ri)
    assert np.array_equal(ps.qtables, qt), (ps.qtables, qt)
    v = J.dct_values(planes)                                                        # B
    qz = np.stack([qt[0], qt[1], qt[1]])[:, J.ZIGZAG][:, None, :].astype(np.float64)
    err = np.abs(ps.coefficients * qz - v) - qz / 2
    print('largest |c q - v| - q / 2: %.3g (EPS %.3g)' % (err.max(), EPS))
    assert (err <= EPS).all(), '%d coefficients beyond q / 2 + EPS, worst by %g' % (int((err > EPS).sum()), err.max())
    again = J.assemble(ps.w, ps.h, qt, ri, ps.coefficients)                         # C
    assert again == data, first_difference(again, data)
    return ps
