"""
What the GPU tests of the device encoders share (test_gpu_jpeg.py, test_gpu_jpeg_opt.py, test_gpu_mjpeg.py, test_gpu_png.py,
test_gpu_png_ext.py, test_gpu_tiff.py, test_gpu_exr.py, test_gpu_gif.py, test_gpu_webp.py, test_gpu_encoders_shared.py):
destinations pre-filled with a sentinel, the call of an encoder's fl_X_encode, and the 16-byte record in front of the file.
"""
import numpy as np

from cuburn_amd import _lib

SENTINEL = 0xA5
SLACK = 4096                  # sentinel bytes the tests keep behind a capacity


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


def queue(mgr, entry, t, w, h, arg, cap, buf=None):
    """Queue the library's `entry` (fl_jpeg_encode / fl_png_encode) from the device tensor `t` into pinned memory (or `buf`)
    pre-filled with the sentinel; no wait.  Returns the buffer, which holds cap + SLACK bytes unless the caller brought it."""
    if buf is None:
        buf = mgr.fb._pinned((cap + SLACK,), 'u1')
    buf[:] = SENTINEL
    _lib.check(getattr(_lib.load(), entry)(mgr.fb.ctx, w, h, t.data_ptr(), arg, buf.ctypes.data, 0, cap))
    return buf


def assert_untouched(buf, cap):
    assert (buf[cap:] == SENTINEL).all(), 'bytes at or beyond cap were written'


def encode(mgr, entry, src, w, h, arg, cap, buf=None):
    """Upload `src`, queue(), wait, and check the sentinel at and beyond cap; returns (buffer, cap)."""
    t = upload(mgr, src)
    buf = queue(mgr, entry, t, w, h, arg, cap, buf)
    _lib.check(_lib.load().fl_ctx_sync(mgr.fb.ctx))
    assert_untouched(buf, cap)
    return buf, cap
