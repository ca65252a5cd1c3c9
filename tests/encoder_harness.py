"""
What the GPU tests of the device encoders share (test_gpu_jpeg.py, test_gpu_jpeg_opt.py, test_gpu_mjpeg.py, test_gpu_png.py,
test_gpu_png_ext.py, test_gpu_tiff.py, test_gpu_exr.py, test_gpu_gif.py, test_gpu_webp.py, test_gpu_apng.py,
test_gpu_encoders_shared.py, test_gpu_encoder_contract.py): destinations pre-filled with a sentinel, the call of an encoder's
fl_X_encode, the 16-byte record in front of the file, and the criteria a JPEG stream and a PNG file are held to where they are not
compared byte for byte.  This module knows no encoder by name but those two; what the entry points of all of them promise —
capacity, destinations, refusals, the whole path, the timing slot — is stated once in tests/encoder_contract.py, over one row per
entry point, on top of what is here.
"""
import io
import zlib

import numpy as np

from cuburn_amd import _lib
import jpeg420_model as M
import jpeg_model as J
import jpeg_opt_model as O
import png_cases as PC
import png_model as P

SENTINEL = 0xA5
SLACK = 4096                  # sentinel bytes the tests keep behind a capacity
EPS = 2.0 ** -8               # the float32 DCT's error bound, derived in tests/test_gpu_jpeg.py


def upload(mgr, arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).to('cuda:%d' % mgr.fb.device)
    torch.cuda.synchronize(mgr.fb.device)
    return t


def record(buf, chunks=False):
    """(nbytes, status, param) of the record; param is the restart interval (JPEG), the segment's bytes (PNG), ...  The fourth word
    is 0, but for an APNG frame block, where it counts the chunks: `chunks` returns it as well."""
    nbytes, status, param, fourth = (int(v) for v in np.frombuffer(bytes(buf[:16]), '<u4'))
    if chunks:
        return nbytes, status, param, fourth
    assert fourth == 0
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


def assert_untouched(buf, cap, what=''):
    assert len(buf) > cap and (buf[cap:] == SENTINEL).all(), '%sbytes at or beyond cap %d were written' % (what and what + ': ', cap)


def encode(mgr, entry, src, w, h, args, cap, buf=None, what=''):
    """Upload `src`, queue(), wait, and check the sentinel at and beyond cap; returns (buffer, cap)."""
    t = upload(mgr, src)
    buf = queue(mgr, entry, t, w, h, args, cap, buf)
    _lib.check(_lib.load().fl_ctx_sync(mgr.fb.ctx))
    assert_untouched(buf, cap, what)
    return buf, cap


def first_difference(a, b):
    """Where two files part: the byte, and the bit of the whole (the least significant bit of a byte first, as deflate, LZW and VP8L
    fill them)."""
    n = min(len(a), len(b))
    x = np.frombuffer(a[:n], np.uint8) ^ np.frombuffer(b[:n], np.uint8)
    d = np.nonzero(x)[0]
    if not len(d):
        return 'lengths %d and %d, first difference at none below %d' % (len(a), len(b), n)
    bit = int(d[0]) * 8 + int(np.nonzero(np.unpackbits(x[d[0]:d[0] + 1], bitorder='little'))[0][0])
    return 'lengths %d and %d, first difference at %d (bit %d)' % (len(a), len(b), int(d[0]), bit)


def assert_jpeg_criteria(data, planes, quality, ri, sampling=0, standard=None):
    """A, B and C of tests/test_gpu_jpeg.py for a stream of either sampling (0: 4:4:4, 1: 4:2:0); with `standard`, the stream
    fl_jpeg_encode_s wrote from the same planes, A, B and C of tests/test_gpu_jpeg_opt.py for an optimised one.  Returns the parse."""
    mod = M if sampling else J
    qt = J.quant_tables(quality)
    if standard is None:
        ps = mod.parse(data)                                                        # A
        again = mod.assemble(ps.w, ps.h, qt, ri, ps.coefficients)
    else:
        assert len(data) >= O.HEADER_BYTES + 2
        ps = O.parse(data)
        assert ps.sampling == sampling
        assert np.array_equal(ps.coefficients, O.parse(standard, optimised=False).coefficients)      # B: the recode is lossless
        again = O.assemble(ps.w, ps.h, qt, ri, ps.coefficients, sampling)
    assert (ps.w, ps.h) == (planes.shape[2], planes.shape[1]) and ps.restart_interval == ri, (ps.w, ps.h, ps.restart_interval, planes.shape, ri)
    assert np.array_equal(ps.qtables, qt), (ps.qtables, qt)
    v = mod.dct_values(planes)                                                      # B
    qz = (M._qz(qt)[None] if sampling else np.stack([qt[0], qt[1], qt[1]])[:, J.ZIGZAG][:, None, :]).astype(np.float64)
    err = np.abs(ps.coefficients * qz - v) - qz / 2
    print('largest |c q - v| - q / 2: %.3g (EPS %.3g)' % (err.max(), EPS))
    assert (err <= EPS).all(), '%d coefficients beyond q / 2 + EPS, worst by %g' % (int((err > EPS).sum()), err.max())
    assert again == data, first_difference(again, data)                             # C
    return ps


def assert_png_criteria(data, rgba, ch, seg):
    """A and B of tests/test_gpu_png.py for a file; returns the parse and its statistics."""
    want = rgba[:, :, :ch]
    ps = P.parse(data, seg)                                                         # A
    assert (ps.w, ps.h, ps.channels) == (rgba.shape[1], rgba.shape[0], ch)
    assert np.array_equal(ps.pixels, want), '%d pixels differ' % int((ps.pixels != want).any(axis=2).sum())
    assert zlib.decompress(ps.zstream) == ps.filtered
    try:
        import PIL.Image
    except ImportError:
        pass
    else:
        im = PIL.Image.open(io.BytesIO(data))
        assert im.size == (ps.w, ps.h) and im.mode == ('RGB' if ch == 3 else 'RGBA')
        assert np.array_equal(np.asarray(im), want)
    st = PC.stats_of(ps, seg)                                                       # B
    assert all(0 <= f <= 4 for f in st['filters'])
    assert st['distances'] in ([], [1]) and set(st['block_types']) <= {0, 2}
    assert st['finals'] == [0] * (len(st['finals']) - 1) + [1]
    assert st['nidat'] == len(st['segments']) == -(-st['nfiltered'] // seg)
    for k, (s, body) in enumerate(zip(st['segments'], ps.idat)):
        last = k + 1 == len(st['segments'])
        assert s['start_aligned'] and (last or s['aligned'])
        coded = len(body) - (2 if k == 0 else 0) - (4 if last else 0)
        assert 8 * coded == (s['bits'] + 7) // 8 * 8                                # one IDAT per segment: its bytes are the segment's
        assert s['stored'] or (s['dynamic'] and coded < s['nbytes'] + 5)
        assert not s['stored'] or coded == s['nbytes'] + 5
    for b in st['blocks']:
        if b['type'] == 2:
            assert b['max_lit_len'] <= 15 and b['max_dist_len'] <= 1 and b['max_cl_len'] <= 7 and b['lit_complete'] and b['cl_complete']
    return ps, st
