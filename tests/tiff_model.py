"""
A model of the TIFF file the device writes (cuburn_amd/csrc/tiff.hip; include/flame_hip.h, fl_tiff_encode), in Python and numpy:
the tiling and the horizontal predictor, the file built on png_model's coder of a last segment and its Adler-32, the header's size
and the bound, and a reader that walks the IFD, checks every rule of the layout and inflates each tile with zlib.
tests/test_cpu_tiff.py holds the model to Pillow and to its own reader; tests/test_gpu_tiff.py compares the device's files with it
byte for byte.
"""
import struct
import zlib

import numpy as np

import png_model as P

TILE_LENGTH = 64
SHORT, LONG = 3, 4


class TiffError(ValueError):
    pass


def tile_width(bits):
    return 128 if bits == 8 else 64


def tile_bytes(channels, bits):
    return tile_width(bits) * TILE_LENGTH * channels * bits // 8


def geometry(w, h, bits):
    """(tile width, tiles per row, tiles per column)."""
    tw = tile_width(bits)
    return tw, -(-w // tw), -(-h // TILE_LENGTH)


def _check(samples, channels, bits):
    samples = np.asarray(samples)
    assert samples.ndim == 3 and samples.shape[2] >= channels and channels in (3, 4) and bits in (8, 16)
    assert samples.dtype == (np.uint8 if bits == 8 else np.uint16)
    return samples[:, :, :channels]


def tiles(samples, channels, bits):
    """The predicted bytes of every tile, row-major: samples outside the image are the clamped pixel's; within a tile row every
    sample but the first pixel's is the difference to the pixel on its left, mod 2^bits; 16-bit values low byte first."""
    s = _check(samples, channels, bits)
    h, w, _ = s.shape
    tw, nx, ny = geometry(w, h, bits)
    ys = np.minimum(np.arange(ny * TILE_LENGTH), h - 1)
    xs = np.minimum(np.arange(nx * tw), w - 1)
    padded = s[ys][:, xs].astype(np.int64)
    out = []
    for ty in range(ny):
        for tx in range(nx):
            t = padded[ty * TILE_LENGTH:(ty + 1) * TILE_LENGTH, tx * tw:(tx + 1) * tw]
            d = t.copy()
            d[:, 1:] -= t[:, :-1]
            out.append((d & ((1 << bits) - 1)).astype('<u%d' % (bits // 8)).tobytes())
    return out


def entries_of(channels):
    return 13 if channels == 4 else 12


def header_bytes(w, h, channels, bits):
    """H: everything in front of the first tile."""
    tw, nx, ny = geometry(w, h, bits)
    nt = nx * ny
    return 8 + 2 + 12 * entries_of(channels) + 4 + 2 * channels + (8 * nt if nt > 1 else 0)


def bound(w, h, channels, bits):
    """fl_tiff_bound."""
    if not (1 <= w <= 65535 and 1 <= h <= 65535) or channels not in (3, 4) or bits not in (8, 16):
        return 0
    tw, nx, ny = geometry(w, h, bits)
    n = 16 + header_bytes(w, h, channels, bits) + nx * ny * (tile_bytes(channels, bits) + 5 + 6 + 1)
    return 0 if n > 0xffffffff else n


def tile_stream(d):
    """One tile's data: a zlib stream of one final block."""
    return b'\x78\x01' + P.deflate_segment(d, True) + struct.pack('>I', P.adler32(d))


def assemble(w, h, channels, bits, streams):
    """The file around the tiles' zlib streams."""
    tw, nx, ny = geometry(w, h, bits)
    nt = nx * ny
    assert len(streams) == nt
    ne = entries_of(channels)
    fixed = 8 + 2 + 12 * ne + 4 + 2 * channels
    H = header_bytes(w, h, channels, bits)
    offs, p = [], H
    for i, s in enumerate(streams):
        offs.append(p)
        p += len(s) + (len(s) & 1 if i + 1 < nt else 0)
    counts = [len(s) for s in streams]

    def entry(tag, typ, count, value):
        if typ == SHORT and count == 1:
            return struct.pack('<HHIHH', tag, typ, count, value, 0)
        return struct.pack('<HHII', tag, typ, count, value)
    ifd = [entry(256, LONG, 1, w), entry(257, LONG, 1, h), entry(258, SHORT, channels, fixed - 2 * channels), entry(259, SHORT, 1, 8),
           entry(262, SHORT, 1, 2), entry(277, SHORT, 1, channels), entry(284, SHORT, 1, 1), entry(317, SHORT, 1, 2),
           entry(322, LONG, 1, tw), entry(323, LONG, 1, TILE_LENGTH),
           entry(324, LONG, nt, offs[0] if nt == 1 else fixed), entry(325, LONG, nt, counts[0] if nt == 1 else fixed + 4 * nt)]
    if channels == 4:
        ifd.append(entry(338, SHORT, 1, 2))
    out = b'II' + struct.pack('<HI', 42, 8) + struct.pack('<H', ne) + b''.join(ifd) + struct.pack('<I', 0)
    out += struct.pack('<%dH' % channels, *([bits] * channels))
    if nt > 1:
        out += struct.pack('<%dI' % nt, *offs) + struct.pack('<%dI' % nt, *counts)
    assert len(out) == H
    body = bytearray()
    for i, s in enumerate(streams):
        body += s
        if len(s) & 1 and i + 1 < nt:
            body.append(0)
    return out + bytes(body)


def encode(samples, channels, bits):
    """The file the device writes for u8 / u16 [h][w][>= channels] samples."""
    s = _check(samples, channels, bits)
    return assemble(s.shape[1], s.shape[0], channels, bits, [tile_stream(d) for d in tiles(s, channels, bits)])


class Parsed(object):
    pass


def parse(data):
    """
    A file of the form the device writes, with every rule of the layout checked: the header, tag order, types and counts, inline
    values with one tile, even offsets, zero pad bytes, tiles that fill the file exactly with nothing trailing, each tile one zlib
    stream of its size, padding samples equal to the clamped pixels.  Returns an object with w, h, channels, bits, tw, nt, offsets,
    counts, streams (the tiles' data), btypes (0 stored, 2 dynamic) and samples (u8 / u16 [h][w][channels], the predictor undone).
    """
    data = bytes(data)
    if len(data) < 8 or data[:8] != b'II' + struct.pack('<HI', 42, 8):
        raise TiffError('bytes 0..7 are not II, 42, 8')
    ne, = struct.unpack('<H', data[8:10])
    if ne not in (12, 13):
        raise TiffError('%d entries' % ne)
    ents = [struct.unpack('<HHI', data[10 + 12 * i:18 + 12 * i]) + (data[18 + 12 * i:22 + 12 * i],) for i in range(ne)]
    if struct.unpack('<I', data[10 + 12 * ne:14 + 12 * ne])[0] != 0:
        raise TiffError('a second IFD')
    tags = [e[0] for e in ents]
    want = [256, 257, 258, 259, 262, 277, 284, 317, 322, 323, 324, 325] + ([338] if ne == 13 else [])
    if tags != want:
        raise TiffError('tags %r' % tags)
    types = dict((e[0], e[1]) for e in ents)
    for tag in want:
        if types[tag] != (LONG if tag in (256, 257, 322, 323, 324, 325) else SHORT):
            raise TiffError('tag %d has type %d' % (tag, types[tag]))
    ent = dict((e[0], e) for e in ents)

    def one(tag):
        _, typ, count, raw = ent[tag]
        if count != 1:
            raise TiffError('tag %d has count %d' % (tag, count))
        if typ == SHORT:
            v, z = struct.unpack('<HH', raw)
            if z:
                raise TiffError('tag %d: bytes behind its SHORT' % tag)
            return v
        return struct.unpack('<I', raw)[0]
    ps = Parsed()
    ps.w, ps.h, ps.channels = one(256), one(257), one(277)
    if ps.channels != (4 if ne == 13 else 3) or not ps.w or not ps.h:
        raise TiffError('%d x %d, %d samples per pixel with %d entries' % (ps.w, ps.h, ps.channels, ne))
    if (one(259), one(262), one(284), one(317)) != (8, 2, 1, 2) or (ne == 13 and one(338) != 2):
        raise TiffError('compression, photometric, planar configuration, predictor or extra samples')
    fixed = 10 + 12 * ne + 4 + 2 * ps.channels
    _, _, count, raw = ent[258]
    if count != ps.channels or struct.unpack('<I', raw)[0] != fixed - 2 * ps.channels:
        raise TiffError('BitsPerSample: count %d at %d' % (count, struct.unpack('<I', raw)[0]))
    bps = struct.unpack('<%dH' % ps.channels, data[fixed - 2 * ps.channels:fixed])
    if len(set(bps)) != 1 or bps[0] not in (8, 16):
        raise TiffError('BitsPerSample %r' % (bps,))
    ps.bits = bps[0]
    ps.tw, nx, ny = geometry(ps.w, ps.h, ps.bits)
    ps.nt = nx * ny
    if (one(322), one(323)) != (ps.tw, TILE_LENGTH):
        raise TiffError('tiles of %d x %d' % (one(322), one(323)))
    if ent[324][2] != ps.nt or ent[325][2] != ps.nt:
        raise TiffError('%d offsets and %d counts for %d tiles' % (ent[324][2], ent[325][2], ps.nt))
    H = header_bytes(ps.w, ps.h, ps.channels, ps.bits)
    if ps.nt == 1:
        ps.offsets, ps.counts = [struct.unpack('<I', ent[324][3])[0]], [struct.unpack('<I', ent[325][3])[0]]      # inline
    else:
        if (struct.unpack('<I', ent[324][3])[0], struct.unpack('<I', ent[325][3])[0]) != (fixed, fixed + 4 * ps.nt):
            raise TiffError('the arrays are not behind BitsPerSample')
        ps.offsets = list(struct.unpack('<%dI' % ps.nt, data[fixed:fixed + 4 * ps.nt]))
        ps.counts = list(struct.unpack('<%dI' % ps.nt, data[fixed + 4 * ps.nt:H]))
    p = H
    ps.streams, ps.btypes = [], []
    tb = tile_bytes(ps.channels, ps.bits)
    raw_tiles = []
    for i, (o, n) in enumerate(zip(ps.offsets, ps.counts)):
        if o != p or o & 1:
            raise TiffError('tile %d at %d, expected at %d (even)' % (i, o, p))
        s = data[o:o + n]
        if len(s) != n or n < 8 or s[:2] != b'\x78\x01':
            raise TiffError('tile %d is cut short or has no zlib header' % i)
        p = o + n
        if n & 1 and i + 1 < ps.nt:
            if data[p:p + 1] != b'\0':
                raise TiffError('the pad byte behind tile %d is not zero' % i)
            p += 1
        bfinal, btype = s[2] & 1, s[2] >> 1 & 3
        if not bfinal or btype not in (0, 2):
            raise TiffError('tile %d: first block has BFINAL %d, BTYPE %d' % (i, bfinal, btype))
        d = zlib.decompressobj()
        raw = d.decompress(s)
        if not d.eof or d.unused_data or len(raw) != tb:
            raise TiffError('tile %d: %d bytes inflated, %d unused, end of stream %r' % (i, len(raw), len(d.unused_data), d.eof))
        ps.streams.append(s)
        ps.btypes.append(btype)
        raw_tiles.append(raw)
    if p != len(data):
        raise TiffError('%d bytes behind the last tile' % (len(data) - p))
    dt = '<u%d' % (ps.bits // 8)
    full = np.zeros((ny * TILE_LENGTH, nx * ps.tw, ps.channels), np.uint8 if ps.bits == 8 else np.uint16)
    for i, raw in enumerate(raw_tiles):
        d = np.frombuffer(raw, dt).reshape(TILE_LENGTH, ps.tw, ps.channels).astype(np.uint64)
        t = np.cumsum(d, axis=1, dtype=np.uint64) & np.uint64((1 << ps.bits) - 1)
        ty, tx = divmod(i, nx)
        full[ty * TILE_LENGTH:(ty + 1) * TILE_LENGTH, tx * ps.tw:(tx + 1) * ps.tw] = t.astype(full.dtype)
    ps.samples = np.ascontiguousarray(full[:ps.h, :ps.w])
    ys, xs = np.minimum(np.arange(full.shape[0]), ps.h - 1), np.minimum(np.arange(full.shape[1]), ps.w - 1)
    if not np.array_equal(full, ps.samples[ys][:, xs]):
        raise TiffError('padding samples are not the clamped pixels')
    return ps
