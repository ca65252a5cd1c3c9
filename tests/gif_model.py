"""
The GIF frame block of the device encoder (include/flame_hip.h, fl_gif_encode; cuburn_amd/csrc/gif.hip) and the file around it,
written in Python straight from the definition: histogram of 32768 cells, median cut by population, inverse colour map, ordered
dither, LZW in segments that each begin with a clear code.  All arithmetic is integer arithmetic.

`decode_block` is a strict reader of its own: it raises on a code above `next`, a code of a width other than the expected one,
data behind END, and a sub-block length that does not match.  Pillow is lenient about such things; it is the third-party witness
for the pixels (tests/test_cpu_gif.py), not for strictness.
"""
import struct

import numpy as np

SEG = 1024                    # FL_GIF_SEG
HEADER_BYTES = 779            # FL_GIF_HEADER_BYTES: 2C, the descriptor, the table, 08
CLEAR, END = 256, 257

BAYER = np.array([[0, 32, 8, 40, 2, 34, 10, 42], [48, 16, 56, 24, 50, 18, 58, 26], [12, 44, 4, 36, 14, 46, 6, 38],
                  [60, 28, 52, 20, 62, 30, 54, 22], [3, 35, 11, 43, 1, 33, 9, 41], [51, 19, 59, 27, 49, 17, 57, 25],
                  [15, 47, 7, 39, 13, 45, 5, 37], [63, 31, 55, 23, 61, 29, 53, 21]], np.int64)


def cells_of(rgb):
    rgb = rgb.astype(np.int64)
    return (rgb[..., 0] >> 3) << 10 | (rgb[..., 1] >> 3) << 5 | rgb[..., 2] >> 3


def histogram(rgb):
    """(count, sums[3]) over the 32768 cells of an [..., 3] array of u8."""
    cell = cells_of(rgb).ravel()
    flat = rgb.reshape(-1, 3).astype(np.int64)
    count = np.bincount(cell, minlength=32768).astype(np.int64)
    sums = np.stack([np.bincount(cell, weights=flat[:, k], minlength=32768).astype(np.int64) for k in range(3)], 1)
    return count, sums


def median_cut(count, colors=256):
    """box[cell] for every non-empty cell (-1 elsewhere) and nb, the number of boxes."""
    box = np.where(count > 0, 0, -1)
    cells = np.nonzero(count)[0]
    coords = np.stack([cells >> 10, cells >> 5 & 31, cells & 31], 1)
    cnt = count[cells]
    of = np.zeros(len(cells), np.int64)             # the box of every non-empty cell
    nb = 1
    pops, ncs = [int(cnt.sum())], [len(cells)]      # every box's pixels and non-empty cells
    while nb < colors:
        best, bpop = -1, -1
        for b in range(nb):
            if ncs[b] > 1 and pops[b] > bpop:        # (a tie stays with the lower index)
                best, bpop = b, pops[b]
        if best < 0:
            break
        m = of == best
        ext = [int(coords[m, a].max() - coords[m, a].min()) for a in range(3)]
        axis = ext.index(max(ext))                   # (the first of the largest: R, then G, then B)
        lo, hi = int(coords[m, axis].min()), int(coords[m, axis].max())
        cum, c = 0, None
        for k in range(32):
            cum += int(cnt[m & (coords[:, axis] == k)].sum())
            if 2 * cum >= bpop:
                c = k
                break
        c = min(max(c, lo), hi - 1)
        up = m & (coords[:, axis] > c)
        of[up] = nb
        pops.append(int(cnt[up].sum())); ncs.append(int(up.sum()))
        pops[best] -= pops[nb]; ncs[best] -= ncs[nb]
        nb += 1
    box[cells] = of
    return box, nb


def palette_of(count, sums, box, nb):
    pal = np.zeros((256, 3), np.int64)
    for b in range(nb):
        m = box == b
        n = int(count[m].sum())
        pal[b] = (sums[m].sum(0) + n // 2) // n
    return pal.astype(np.uint8)


def lookup(count, sums, pal, nb):
    """The palette entry of every cell."""
    cell = np.arange(32768)
    centre = np.stack([8 * (cell >> 10) + 4, 8 * (cell >> 5 & 31) + 4, 8 * (cell & 31) + 4], 1)
    n = np.maximum(count, 1)[:, None]
    point = np.where(count[:, None] > 0, (sums + n // 2) // n, centre)
    point, ents = point.astype(np.int32), pal[:nb].astype(np.int32)
    d = sum((point[:, None, k] - ents[None, :, k]) ** 2 for k in range(3))
    return d.argmin(1).astype(np.uint8)              # (argmin: the first of the least)


def dithered(rgb, amp):
    h, w = rgb.shape[:2]
    d = 2 * BAYER[np.arange(h)[:, None] & 7, np.arange(w)[None, :] & 7] + 1 - 64
    return np.clip(rgb.astype(np.int64) + ((d * amp) >> 7)[:, :, None], 0, 255)


def quantise(rgba, colors=256, amp=8):
    """(palette u8 [256][3], indices u8 [h][w], nb) of a u8 [h][w][>=3] frame."""
    rgb = np.asarray(rgba)[:, :, :3]
    count, sums = histogram(rgb)
    box, nb = median_cut(count, colors)
    pal = palette_of(count, sums, box, nb)
    lut = lookup(count, sums, pal, nb)
    return pal, lut[cells_of(dithered(rgb, amp))], nb


class _Bits(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc |= code << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def bits(self):
        return 8 * len(self.out) + self.n


def _step(nxt, width):
    nxt += 1
    if nxt > (1 << width) and width < 12:
        width += 1
    return nxt, width


def lzw_segment(idx, last):
    """The bytes of one segment of indices."""
    b = _Bits()
    width, nxt = 9, 258
    b.put(CLEAR, 9)
    table = {}
    p = int(idx[0])
    for c in idx[1:]:
        c = int(c)
        code = table.get((p, c))
        if code is not None:
            p = code
            continue
        b.put(p, width)
        table[(p, c)] = nxt
        nxt, width = _step(nxt, width)
        p = c
    b.put(p, width)
    nxt, width = _step(nxt, width)                   # the entry the decoder adds
    if last:
        b.put(END, width)
        if b.n:
            b.put(0, 8 - b.n)
    else:
        b.put(CLEAR, width)
        while b.n:
            b.put(CLEAR, 9)
    assert b.n == 0 and nxt <= 4096
    return bytes(b.out)


def final_width(idx):
    """The width in which a segment of these indices emits its last string's code."""
    width, nxt, table, p = 9, 258, {}, int(idx[0])
    for c in idx[1:]:
        c = int(c)
        if (p, c) in table:
            p = table[(p, c)]
            continue
        table[(p, c)] = nxt
        nxt, width = _step(nxt, width)
        p = c
    return width


def lzw_stream(indices, seg=SEG):
    flat = np.asarray(indices).ravel()
    nseg = (len(flat) + seg - 1) // seg
    return b''.join(lzw_segment(flat[i * seg:(i + 1) * seg], i + 1 == nseg) for i in range(nseg))


def sub_blocks(stream):
    out = bytearray()
    for g in range(0, len(stream), 255):
        piece = stream[g:g + 255]
        out.append(len(piece))
        out += piece
    out.append(0)
    return bytes(out)


def block_of(w, h, pal, indices, seg=SEG):
    """The frame block from a palette and indices."""
    assert np.asarray(pal).shape == (256, 3) and np.asarray(indices).size == w * h
    return (b'\x2c' + struct.pack('<4H', 0, 0, w, h) + b'\x87' + np.asarray(pal, np.uint8).tobytes() + b'\x08'
            + sub_blocks(lzw_stream(indices, seg)))


def frame_block(rgba, colors=256, amp=8, seg=SEG):
    """What fl_gif_encode puts behind the record."""
    h, w = rgba.shape[:2]
    pal, idx, _ = quantise(rgba, colors, amp)
    return block_of(w, h, pal, idx, seg)


def stream_bytes(block):
    """The length of the data stream of a block (the sub-blocks' bytes without their length bytes)."""
    n, at = 0, HEADER_BYTES
    while block[at]:
        n += block[at]
        at += 1 + block[at]
    return n


def bound(w, h):
    """fl_gif_bound: twelve bits a pixel and 84 bits of framing a segment at the shortest segment length."""
    if not (1 <= w <= 65535 and 1 <= h <= 65535) or w * h > 1 << 24:
        return 0
    n = w * h
    t = (3 * n + 1) // 2 + 11 * ((n + 255) // 256)
    return 16 + HEADER_BYTES + t + (t + 254) // 255 + 1


def delays(nframes, fps):
    """Centiseconds of every frame: the file keeps the rate on average."""
    return [int(round(100.0 * (k + 1) / fps)) - int(round(100.0 * k / fps)) for k in range(nframes)]


def gif_file(w, h, blocks, fps=24, loop=0):
    out = bytearray(b'GIF89a' + struct.pack('<HH', w, h) + b'\x70\x00\x00')
    out += b'\x21\xff\x0bNETSCAPE2.0\x03\x01' + struct.pack('<H', loop) + b'\x00'
    for blk, d in zip(blocks, delays(len(blocks), fps)):
        out += b'\x21\xf9\x04\x04' + struct.pack('<H', d) + b'\x00\x00' + blk
    out += b'\x3b'
    return bytes(out)


# ---- the strict reader -------------------------------------------------------------------------------------------------
class GifError(ValueError):
    pass


def _unblock(data, at):
    """(stream, offset behind the terminator): every sub-block but the last holds 255 bytes."""
    stream = bytearray()
    short = False
    while True:
        if at >= len(data):
            raise GifError('the sub-blocks run past the end')
        n = data[at]
        at += 1
        if n == 0:
            return bytes(stream), at
        if short:
            raise GifError('a sub-block behind one of fewer than 255 bytes')
        if at + n > len(data):
            raise GifError('a sub-block length that does not match')
        short = n < 255
        stream += data[at:at + n]
        at += n


def decode_stream(stream, npix, seg=SEG):
    """Indices of a data stream written in segments of `seg` pixels.  Strict: the widths are the definition's, no code is above
    `next`, CLEAR stands exactly where a segment ends, the padding is what the definition says, nothing follows END."""
    pos = 0

    def get(width):
        nonlocal pos
        if pos + width > 8 * len(stream):
            raise GifError('the stream ends inside a code')
        v = 0
        for k in range(width):
            v |= (stream[(pos + k) >> 3] >> ((pos + k) & 7) & 1) << k
        pos += width
        return v
    out = []
    nseg = (npix + seg - 1) // seg
    for s in range(nseg):
        n = min(seg, npix - s * seg)
        if pos & 7:
            raise GifError('a segment that does not begin on a byte boundary')
        if get(9) != CLEAR:
            raise GifError('a segment without its clear code')
        table = {}
        width, nxt = 9, 258
        got = []
        prev = None
        while len(got) < n:
            code = get(width)
            if code in (CLEAR, END):
                raise GifError('code %d inside a segment' % code)
            if prev is None:
                if code > 255:
                    raise GifError('a first code that is no index')
                entry = [code]
            else:
                if code > nxt - 1:                   # (next - 1 is the string the encoder added behind the code before this one)
                    raise GifError('code %d above next %d' % (code, nxt - 1))
                entry = table[code] if code in table else [code] if code < 256 else prev + [prev[0]]
                table[nxt - 1] = prev + [entry[0]]
            nxt, width = _step(nxt, width)           # what the encoder did behind this code, the last one included
            got += entry
            prev = entry
        if len(got) != n:
            raise GifError('a string runs over the end of its segment')
        closing = get(width)
        if s + 1 == nseg:
            if closing != END:
                raise GifError('no END behind the last segment (read %d in %d bits)' % (closing, width))
            while pos & 7:
                if get(1):
                    raise GifError('padding that is not zero')
            if pos != 8 * len(stream):
                raise GifError('data behind END')
        else:
            if closing != CLEAR:
                raise GifError('no CLEAR behind a segment (read %d in %d bits)' % (closing, width))
            while pos & 7:
                if get(9) != CLEAR:
                    raise GifError('padding that is no clear code')
        out += got
    return np.array(out, np.uint8)


def decode_block(block, seg=SEG):
    """(w, h, palette, indices [h][w]) of a frame block."""
    if block[0] != 0x2c or block[9] != 0x87 or block[HEADER_BYTES - 1] != 8:
        raise GifError('not a frame block of this encoder')
    left, top, w, h = struct.unpack('<4H', block[1:9])
    if left or top:
        raise GifError('a frame that does not start at 0, 0')
    pal = np.frombuffer(block[10:778], np.uint8).reshape(256, 3)
    stream, at = _unblock(block, HEADER_BYTES)
    if at != len(block):
        raise GifError('bytes behind the block terminator')
    return w, h, pal, decode_stream(stream, w * h, seg).reshape(h, w)
