"""
The device PNG encoder's extended format (include/flame_hip.h, fl_png_encode_f) written out in Python on top of tests/png_model.py:
a sample depth of 8 or 16 bits and, per row, the filter type of least cost.  A 16-bit frame is handled as the u8 [h][w][bpp] image
of its bytes in file order (every sample most significant byte first), which png_model's filters and unfilters take as they take
any channel count.  tests/test_cpu_png_ext.py holds this model to zlib and Pillow; tests/test_gpu_png_ext.py holds the device to it.
"""
import struct

import numpy as np

import png_model as P

ADAPTIVE = 1                      # FL_PNG_ADAPTIVE


def bpp_of(channels, bits):
    return channels * bits // 8


def byte_image(samples, channels, bits):
    """u8 [h][w][bpp]: the bytes the file holds for the first `channels` samples of u8 or u16 [h][w][>= channels] pixels."""
    s = np.ascontiguousarray(samples[:, :, :channels])
    if bits == 8:
        assert s.dtype == np.uint8
        return s
    assert bits == 16 and s.dtype == np.uint16
    h, w, _ = s.shape
    return np.ascontiguousarray(s.astype('>u2').view(np.uint8).reshape(h, w, 2 * channels))


def samples_of(bytes_img, bits):
    """The inverse of byte_image: u8 [h][w][channels] or u16 [h][w][channels] in native order."""
    if bits == 8:
        return bytes_img
    h, w, bpp = bytes_img.shape
    return np.ascontiguousarray(bytes_img).view('>u2').reshape(h, w, bpp // 2).astype(np.uint16)


def row_costs(bytes_img):
    """int64 [5][h]: for every filter type and row, the sum over the row's residual bytes r of min(r, 256 - r)."""
    h, w, bpp = bytes_img.shape
    out = np.empty((5, h), np.int64)
    for t in range(5):
        r = np.frombuffer(P.filter_rows(bytes_img, t), np.uint8).reshape(h, 1 + w * bpp)[:, 1:].astype(np.int64)
        out[t] = np.minimum(r, 256 - r).sum(axis=1)
    return out


def choose(bytes_img):
    """The filter type of every row: the smallest type whose cost is minimal (np.argmin returns the first minimum)."""
    return [int(t) for t in np.argmin(row_costs(bytes_img), axis=0)]


def filter_stream(bytes_img, flags=0):
    """(the filtered stream, the rows' types) of a byte image: all Paeth, or with ADAPTIVE each row the type of least cost."""
    h, w, bpp = bytes_img.shape
    if not flags & ADAPTIVE:
        return P.filter_rows(bytes_img, 4), [4] * h
    types = choose(bytes_img)
    by_type = dict((t, np.frombuffer(P.filter_rows(bytes_img, t), np.uint8).reshape(h, 1 + w * bpp)) for t in set(types))
    return b''.join(by_type[t][y].tobytes() for y, t in enumerate(types)), types


def encode(samples, channels, bits, flags, seg):
    """The file the device writes for u8 / u16 [h][w][>= channels] pixels with segments of `seg` filtered bytes."""
    img = byte_image(samples, channels, bits)
    h, w, _ = img.shape
    filtered, _ = filter_stream(img, flags)
    los = list(range(0, len(filtered), seg))
    parts = [P.deflate_segment(filtered[lo:lo + seg], lo == los[-1]) for lo in los]
    parts[0] = b'\x78\x01' + parts[0]
    parts[-1] += struct.pack('>I', P.adler32(filtered))

    def chunk(tag, body):
        return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', P.crc32(tag + body))
    return (P.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, bits, 2 if channels == 3 else 6, 0, 0, 0))
            + b''.join(chunk(b'IDAT', p) for p in parts) + chunk(b'IEND', b''))


def parse(data, seg=None):
    """png_model.parse for depth 8 or 16: an object with w, h, channels, bits, idat, zstream, filtered, blocks, filters, `bytes`
    (u8 [h][w][bpp], the unfiltered bytes in file order) and `pixels` (u8 or u16 [h][w][channels]).  Every checksum is verified."""
    ck = P.chunks(data)
    if ck[0][0] != b'IHDR' or len(ck[0][1]) != 13:
        raise P.PngError('IHDR is not the first chunk')
    ps = P.Parsed()
    ps.w, ps.h, ps.bits, ctype, comp, filt, lace = struct.unpack('>IIBBBBB', ck[0][1])
    if ps.bits not in (8, 16) or ctype not in (2, 6) or comp or filt or lace:
        raise P.PngError('not a truecolour, non-interlaced PNG of 8 or 16 bits')
    ps.channels = 3 if ctype == 2 else 4
    ps.tags = [tag for tag, _ in ck]
    ps.idat = [body for tag, body in ck if tag == b'IDAT']
    if ps.tags != [b'IHDR'] + [b'IDAT'] * len(ps.idat) + [b'IEND'] or not ps.idat:
        raise P.PngError('chunks %r' % ps.tags)
    ps.zstream = b''.join(ps.idat)
    ps.filtered, ps.blocks = P.zlib_inflate(ps.zstream, seg)
    ps.bytes, ps.filters = P.unfilter(ps.filtered, ps.w, ps.h, bpp_of(ps.channels, ps.bits))
    ps.pixels = samples_of(ps.bytes, ps.bits)
    return ps


def bound(w, h, channels, bits, seg):
    """fl_png_bound_f for a frame it does not refuse: the all-stored worst case with rows of 1 + w * bpp bytes."""
    F = h * (1 + w * bpp_of(channels, bits))
    return 16 + P.HEADER_BYTES + 2 + F + 17 * -(-F // seg) + 4 + 12
