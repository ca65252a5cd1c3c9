"""
A model of the OpenEXR file the device writes (cuburn_amd/csrc/exr.hip; include/flame_hip.h, fl_exr_encode), in Python and numpy:
the float to half conversion in integer arithmetic, the cropped tiles and their channel-planar rows, OpenEXR's byte split and delta
predictor, the tile's data built on png_model's coder of a last segment and its Adler-32, the header, the bound, and a reader.
No OpenEXR reader is installed where these tests run, so `parse` is the only decoder: it is written from the published file layout
and shares nothing with the writer above it but `struct` and `zlib` — it walks the attributes by name, type and size, takes the
tile geometry from `tiles` and `dataWindow`, finds the chunks through the offset table, tells compressed from raw by the size and
undoes the predictor and the split itself.  tests/test_cpu_exr.py holds the model to numpy's float16 and to its own reader;
tests/test_gpu_exr.py compares the device's files with it byte for byte.
"""
import struct
import zlib

import numpy as np

import png_model as P

HALF, FLOAT = 1, 2
TILE_WIDTH = 64
MAGIC = b'\x76\x2f\x31\x01'


class ExrError(ValueError):
    pass


def tile_rows(pixel):
    return 32 if pixel == FLOAT else 64


def sample_bytes(pixel):
    return 4 if pixel == FLOAT else 2


def tile_bytes(channels):
    """A full tile, at either depth: the record's parameter."""
    return 8192 * channels


def geometry(w, h, pixel):
    """(tile rows, tiles per row, tiles per column)."""
    th = tile_rows(pixel)
    return th, -(-w // TILE_WIDTH), -(-h // th)


# ------------------------------------------------------------------ samples
def to_half(x):
    """The half bits (uint16) of float32 values: round to nearest, ties to even, gradual underflow, in integer arithmetic on the
    float's bits; what would be infinite is +-65504, NaN is 0."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7fffffff
    e, m = a >> 23, a & 0x7fffff
    # normal halves: exponent e - 112 and the top 10 mantissa bits; a carry out of the mantissa runs into the exponent
    hn = ((e - 112) << 10) | (m >> 13)
    rem = m & 0x1fff
    hn = hn + ((rem > 0x1000) | ((rem == 0x1000) & ((hn & 1) == 1)))
    # below 2^-14: the mantissa with its leading one, shifted to units of 2^-24
    sh = np.minimum(126 - e, 31)
    sh = np.where(e < 113, sh, 14)
    mant = np.where(e > 0, m | 0x800000, m)
    hs = mant >> sh
    rem = mant & ((1 << sh) - 1)
    halfway = 1 << (sh - 1)
    hs = hs + ((rem > halfway) | ((rem == halfway) & ((hs & 1) == 1)))
    hb = np.where(e >= 113, hn, hs)
    hb = np.where(hb >= 0x7c00, 0x7bff, hb) | sign
    hb = np.where(a > 0x7f800000, 0, hb)
    return hb.astype(np.uint16)


def samples_of(x, channels, pixel):
    """[h][w][channels] of the file's sample bits (uint16 / uint32), channels in R, G, B, A order."""
    x = np.asarray(x)
    assert x.ndim == 3 and x.dtype == np.float32 and x.shape[2] >= channels and channels in (3, 4) and pixel in (HALF, FLOAT)
    x = np.ascontiguousarray(x[:, :, :channels])
    return x.view(np.uint32) if pixel == FLOAT else to_half(x)


def file_order(channels):
    """The chlist's order — alphabetical — as indices into R, G, B, A."""
    return [3, 2, 1, 0] if channels == 4 else [2, 1, 0]


# ------------------------------------------------------------------ tiles
def raw_tiles(x, channels, pixel):
    """The raw bytes of every tile, ty-major: the tile cropped to the image; row by row, within a row channel by channel in the
    chlist's order, within a channel the samples low byte first."""
    s = samples_of(x, channels, pixel)
    h, w, _ = s.shape
    th, nx, ny = geometry(w, h, pixel)
    dt = '<u4' if pixel == FLOAT else '<u2'
    out = []
    for ty in range(ny):
        for tx in range(nx):
            t = s[ty * th:(ty + 1) * th, tx * TILE_WIDTH:(tx + 1) * TILE_WIDTH][:, :, file_order(channels)]
            out.append(np.ascontiguousarray(t.transpose(0, 2, 1)).astype(dt).tobytes())
    return out


def preprocess(raw):
    """OpenEXR's two steps in front of zlib: the even-indexed bytes, then the odd-indexed ones; then every byte but the first as the
    difference to the one before it, plus 128."""
    b = np.frombuffer(raw, np.uint8)
    assert b.size and b.size % 2 == 0
    t = np.concatenate([b[0::2], b[1::2]]).astype(np.int64)
    d = t.copy()
    d[1:] = (t[1:] - t[:-1] + 128) & 255
    return d.astype(np.uint8).tobytes()


def tile_data(raw):
    """What a chunk holds for the tile: the zlib stream where it is smaller than the raw bytes, else those."""
    d = preprocess(raw)
    z = b'\x78\x01' + P.deflate_segment(d, True) + struct.pack('>I', P.adler32(d))
    return z if len(z) < len(raw) else raw


# ------------------------------------------------------------------ the file
def _attr(name, typ, value):
    return name + b'\0' + typ + b'\0' + struct.pack('<i', len(value)) + value


def header(w, h, channels, pixel):
    chlist = b''.join(n + b'\0' + struct.pack('<iB3xii', pixel, 0, 1, 1) for n in ((b'A', b'B', b'G', b'R') if channels == 4 else (b'B', b'G', b'R'))) + b'\0'
    box = struct.pack('<4i', 0, 0, w - 1, h - 1)
    return (MAGIC + struct.pack('<I', 0x00000202)
            + _attr(b'channels', b'chlist', chlist)
            + _attr(b'compression', b'compression', b'\x03')
            + _attr(b'dataWindow', b'box2i', box)
            + _attr(b'displayWindow', b'box2i', box)
            + _attr(b'lineOrder', b'lineOrder', b'\x00')
            + _attr(b'pixelAspectRatio', b'float', struct.pack('<f', 1.0))
            + _attr(b'screenWindowCenter', b'v2f', struct.pack('<2f', 0.0, 0.0))
            + _attr(b'screenWindowWidth', b'float', struct.pack('<f', 1.0))
            + _attr(b'tiles', b'tiledesc', struct.pack('<IIB', TILE_WIDTH, tile_rows(pixel), 0))
            + b'\0')


def header_bytes(w, h, channels, pixel):
    """H: magic, version and the attributes (the offset table follows)."""
    return len(header(w, h, channels, pixel))


def bound(w, h, channels, pixel):
    """fl_exr_bound."""
    if not (1 <= w <= 65535 and 1 <= h <= 65535) or channels not in (3, 4) or pixel not in (HALF, FLOAT):
        return 0
    th, nx, ny = geometry(w, h, pixel)
    n = 16 + header_bytes(w, h, channels, pixel) + 28 * nx * ny + w * h * channels * sample_bytes(pixel)
    return 0 if n > 0xffffffff else n


def assemble(w, h, channels, pixel, datas):
    """The file around the tiles' data."""
    th, nx, ny = geometry(w, h, pixel)
    assert len(datas) == nx * ny
    hdr = header(w, h, channels, pixel)
    p = len(hdr) + 8 * len(datas)
    offs, body = [], bytearray()
    for i, d in enumerate(datas):
        offs.append(p)
        body += struct.pack('<5i', i % nx, i // nx, 0, 0, len(d)) + d
        p += 20 + len(d)
    return hdr + struct.pack('<%dQ' % len(offs), *offs) + bytes(body)


def encode(x, channels, pixel, only=None):
    """The file the device writes for f32 [h][w][>= channels].  `only`: the tiles to run through the (slow) coder — the others are
    stored raw, which gives a file of the same layout but not the device's bytes."""
    raws = raw_tiles(x, channels, pixel)
    datas = [tile_data(r) if only is None or i in only else r for i, r in enumerate(raws)]
    return assemble(x.shape[1], x.shape[0], channels, pixel, datas)


# ------------------------------------------------------------------ the reader
class Parsed(object):
    pass


def _cstr(data, p, what):
    q = data.find(b'\0', p)
    if q < 0 or q - p > 255:
        raise ExrError('%s at %d does not end' % (what, p))
    return data[p:q], q + 1


def parse(data):
    """
    A tiled, single-part, one-level OpenEXR file with ZIP compression, read from the published layout.  Returns an object with w, h,
    channels, pixel, names, th, nx, ny, nt, attrs (name -> (type, value bytes)), header_bytes, offsets, sizes (each chunk's
    dataSize), forms ('zip' / 'raw' per tile), datas and samples: the sample bits, uint16 / uint32 [h][w][channels] in R, G, B, A
    order.  Raises ExrError where the file breaks the layout or holds what this reader does not know.
    """
    data = bytes(data)
    if data[:4] != MAGIC:
        raise ExrError('no magic number')
    version, = struct.unpack('<I', data[4:8])
    if version & 0xff != 2 or version >> 8 != 0x2:
        raise ExrError('version word %#x: not version 2 with only the tiled bit' % version)
    ps = Parsed()
    ps.attrs, order, p = {}, [], 8
    while True:
        if p >= len(data):
            raise ExrError('the header does not end')
        if data[p] == 0:
            p += 1
            break
        name, p = _cstr(data, p, 'attribute name')
        typ, p = _cstr(data, p, 'attribute type')
        size, = struct.unpack('<i', data[p:p + 4])
        if size < 0 or p + 4 + size > len(data):
            raise ExrError('attribute %r has size %d' % (name, size))
        if name in ps.attrs:
            raise ExrError('attribute %r twice' % name)
        ps.attrs[name] = (typ, data[p + 4:p + 4 + size])
        order.append(name)
        p += 4 + size
    ps.header_bytes, ps.order = p, order

    def need(name, typ, size=None):
        if name not in ps.attrs or ps.attrs[name][0] != typ or (size is not None and len(ps.attrs[name][1]) != size):
            raise ExrError('attribute %r / %r is missing or has another type or size' % (name, typ))
        return ps.attrs[name][1]
    # channels
    cl, q, chans = need(b'channels', b'chlist'), 0, []
    while True:
        if q >= len(cl):
            raise ExrError('the channel list does not end')
        if cl[q] == 0:
            if q + 1 != len(cl):
                raise ExrError('bytes behind the channel list')
            break
        name, q = _cstr(cl, q, 'channel name')
        ptype, plinear, xs, ys = struct.unpack('<iB3xii', cl[q:q + 16])
        if cl[q + 5:q + 8] != b'\0\0\0' or (xs, ys) != (1, 1) or ptype not in (HALF, FLOAT):
            raise ExrError('channel %r: type %d, sampling %d x %d' % (name, ptype, xs, ys))
        chans.append((name, ptype))
        q += 16
    ps.names = [c[0] for c in chans]
    if ps.names != sorted(ps.names) or sorted(ps.names) not in ([b'B', b'G', b'R'], [b'A', b'B', b'G', b'R']) or len(set(c[1] for c in chans)) != 1:
        raise ExrError('channels %r' % (chans,))
    ps.channels, ps.pixel = len(chans), chans[0][1]
    if need(b'compression', b'compression', 1) != b'\x03':
        raise ExrError('compression %d is not ZIP' % need(b'compression', b'compression', 1)[0])
    x0, y0, x1, y1 = struct.unpack('<4i', need(b'dataWindow', b'box2i', 16))
    if (x0, y0) != (0, 0) or x1 < 0 or y1 < 0 or need(b'displayWindow', b'box2i', 16) != ps.attrs[b'dataWindow'][1]:
        raise ExrError('data window %r' % ((x0, y0, x1, y1),))
    ps.w, ps.h = x1 + 1, y1 + 1
    if need(b'lineOrder', b'lineOrder', 1) != b'\0':
        raise ExrError('line order')
    if struct.unpack('<f', need(b'pixelAspectRatio', b'float', 4))[0] != 1.0 or struct.unpack('<f', need(b'screenWindowWidth', b'float', 4))[0] != 1.0:
        raise ExrError('pixel aspect ratio or screen window width')
    if struct.unpack('<2f', need(b'screenWindowCenter', b'v2f', 8)) != (0.0, 0.0):
        raise ExrError('screen window centre')
    xsize, ysize, mode = struct.unpack('<IIB', need(b'tiles', b'tiledesc', 9))
    if mode != 0 or not xsize or not ysize:
        raise ExrError('tiles of %d x %d, mode %d' % (xsize, ysize, mode))
    ps.tw, ps.th = xsize, ysize
    ps.nx, ps.ny = -(-ps.w // xsize), -(-ps.h // ysize)
    ps.nt = ps.nx * ps.ny
    if p + 8 * ps.nt > len(data):
        raise ExrError('the offset table is cut short')
    ps.offsets = list(struct.unpack('<%dQ' % ps.nt, data[p:p + 8 * ps.nt]))
    p += 8 * ps.nt
    bps = 4 if ps.pixel == FLOAT else 2
    bits = np.zeros((ps.h, ps.w, ps.channels), np.uint32 if ps.pixel == FLOAT else np.uint16)
    slot = [ps.names.index(n) for n in ((b'R', b'G', b'B', b'A')[:ps.channels])]      # where R, G, B, A sit in a row of the file
    ps.sizes, ps.forms, ps.datas = [], [], []
    for i, o in enumerate(ps.offsets):
        if o != p:
            raise ExrError('chunk %d at %d, expected at %d' % (i, o, p))
        if o + 20 > len(data):
            raise ExrError('chunk %d is cut short' % i)
        tx, ty, lx, ly, size = struct.unpack('<5i', data[o:o + 20])
        if (tx, ty, lx, ly) != (i % ps.nx, i // ps.nx, 0, 0):
            raise ExrError('chunk %d is tile (%d, %d) of level (%d, %d)' % (i, tx, ty, lx, ly))
        tw, th = min(xsize, ps.w - tx * xsize), min(ysize, ps.h - ty * ysize)
        n = tw * th * ps.channels * bps
        if size <= 0 or size > n or o + 20 + size > len(data):
            raise ExrError('chunk %d holds %d bytes for a tile of %d' % (i, size, n))
        body = data[o + 20:o + 20 + size]
        if size < n:
            z = zlib.decompressobj()
            t = z.decompress(body)
            if not z.eof or z.unused_data or len(t) != n:
                raise ExrError('chunk %d: %d bytes inflated for a tile of %d, %d unused' % (i, len(t), n, len(z.unused_data)))
            t = np.cumsum(np.frombuffer(t, np.uint8).astype(np.int64) - 128) + 128      # t[i] = t[i-1] + d[i] - 128, t[0] = d[0]
            t = (t & 255).astype(np.uint8)
            raw = np.empty(n, np.uint8)
            raw[0::2], raw[1::2] = t[:n // 2], t[n // 2:]
            raw = raw.tobytes()
        else:
            raw = body
        ps.sizes.append(size)
        ps.forms.append('zip' if size < n else 'raw')
        ps.datas.append(body)
        rows = np.frombuffer(raw, '<u%d' % bps).reshape(th, ps.channels, tw)
        bits[ty * ysize:ty * ysize + th, tx * xsize:tx * xsize + tw] = rows[:, slot, :].transpose(0, 2, 1)
        p = o + 20 + size
    if p != len(data):
        raise ExrError('%d bytes behind the last chunk' % (len(data) - p))
    ps.samples = bits
    return ps
