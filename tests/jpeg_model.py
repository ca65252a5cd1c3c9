"""
Model of the device JPEG encoder (include/flame_hip.h, fl_jpeg_encode): numpy only, float64.

Baseline sequential JPEG (ITU T.81, JFIF 1.01): 8 bit, three components Y, Cb, Cr all sampled 1x1, one interleaved scan, the
Huffman tables of Annex K.3-K.6, the quantisation tables of Annex K.1 / K.2 scaled the libjpeg way, restart intervals.

  encode(planes, quality, restart_interval) -> bytes      the whole file
  parse(data) -> Parsed                                   a strict entropy decoder: marker order, RST numbering, stuffing, padding
  entropy_encode(coefficients, restart_interval) -> bytes the scan's data, RSTm markers included (what lies between SOS and EOI)
  decode(data) -> planes                                  float64 IDCT, round, clamp

Coefficients are int arrays [3][blocks][64]: component, block in raster order, zigzag position.
"""
import collections

import numpy as np

HEADER_BYTES = 629            # SOI, APP0, DQT x2, SOF0, DHT x4, DRI, SOS

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.1 / K.2, row-major
Q_BASE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
    + [99] * 32])

# Annex K.3-K.6: (BITS, HUFFVAL)
DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
# DHT order in the file: (class << 4 | id, table)
DHT_ORDER = ((0x00, DC_LUM), (0x10, AC_LUM), (0x01, DC_CHR), (0x11, AC_CHR))


class JpegError(ValueError):
    pass


def quant_tables(quality):
    """[2][64] row-major: Annex K.1 / K.2 scaled as libjpeg's jpeg_set_quality does (baseline: entries 1..255)."""
    if not 1 <= quality <= 100:
        raise ValueError('quality must be 1..100')
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((Q_BASE * s + 50) // 100, 1, 255)


def huff_codes(table):
    """symbol -> (code, length), T.81 Annex C."""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


_ENC = dict(dc=(huff_codes(DC_LUM), huff_codes(DC_CHR)), ac=(huff_codes(AC_LUM), huff_codes(AC_CHR)))
_DEC = dict((kind, tuple(dict(((ln, code), sym) for sym, (code, ln) in t.items()) for t in tabs)) for kind, tabs in _ENC.items())

# C[u][x] = 0.5 * C(u) * cos((2x + 1) u pi / 16): the 1-D factor of the T.81 DCT
_C = np.array([[0.5 * (np.sqrt(0.5) if u == 0 else 1.0) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def blocks_of(planes):
    """u8 [3][h][w] -> float64 [3][blocks][8][8], level shifted; the last column / row replicated into partial blocks."""
    planes = np.asarray(planes)
    _, h, w = planes.shape
    bh, bw = (h + 7) // 8, (w + 7) // 8
    p = np.pad(planes.astype(np.float64) - 128.0, ((0, 0), (0, 8 * bh - h), (0, 8 * bw - w)), mode='edge')
    return p.reshape(3, bh, 8, bw, 8).transpose(0, 1, 3, 2, 4).reshape(3, bh * bw, 8, 8)


def dct_values(planes):
    """float64 DCT values [3][blocks][64] in zigzag order, before quantisation."""
    b = blocks_of(planes)
    F = np.einsum('vy,cbyx,ux->cbvu', _C, b, _C)
    return F.reshape(3, -1, 64)[:, :, ZIGZAG]


def quantise(values, qt):
    """values [3][blocks][64] zigzag, qt [2][64] row-major -> int coefficients."""
    qz = np.stack([qt[0], qt[1], qt[1]])[:, ZIGZAG]
    return np.rint(values / qz[:, None, :]).astype(np.int64)


def _cat(v):
    return int(abs(int(v))).bit_length()


class _BitWriter(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xff
            self.out.append(byte)
            if byte == 0xff:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _value_bits(v, s):
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


def entropy_encode(coefficients, restart_interval):
    """The scan's data: MCUs of three blocks, intervals padded with 1-bits and followed by RST(k mod 8) except the last."""
    coefficients = np.asarray(coefficients)
    nmcu = coefficients.shape[1]
    out = bytearray()
    nint = (nmcu + restart_interval - 1) // restart_interval
    for it in range(nint):
        bw, pred = _BitWriter(), [0, 0, 0]
        for m in range(it * restart_interval, min(nmcu, (it + 1) * restart_interval)):
            for c in range(3):
                z = coefficients[c, m]
                dc_tab, ac_tab = _ENC['dc'][min(c, 1)], _ENC['ac'][min(c, 1)]
                diff = int(z[0]) - pred[c]
                pred[c] = int(z[0])
                s = _cat(diff)
                bw.put(*dc_tab[s])
                if s:
                    bw.put(_value_bits(diff, s), s)
                run = 0
                for k in range(1, 64):
                    v = int(z[k])
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bw.put(*ac_tab[0xf0])
                        run -= 16
                    s = _cat(v)
                    bw.put(*ac_tab[run << 4 | s])
                    bw.put(_value_bits(v, s), s)
                    run = 0
                if run:
                    bw.put(*ac_tab[0])
        bw.pad()
        out += bw.out
        if it + 1 < nint:
            out += bytes([0xff, 0xd0 + (it & 7)])
    return bytes(out)


def header(w, h, qt, restart_interval):
    def seg(marker, body):
        return bytes([0xff, marker]) + (len(body) + 2).to_bytes(2, 'big') + bytes(body)
    out = b'\xff\xd8' + seg(0xe0, b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for t in range(2):
        out += seg(0xdb, bytes([t]) + bytes(int(v) for v in np.asarray(qt[t])[ZIGZAG]))
    out += seg(0xc0, bytes([8]) + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for ident, (bits, vals) in DHT_ORDER:
        out += seg(0xc4, bytes([ident]) + bytes(bits) + bytes(vals))
    out += seg(0xdd, restart_interval.to_bytes(2, 'big'))
    out += seg(0xda, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEADER_BYTES
    return out


def assemble(w, h, qt, restart_interval, coefficients):
    return header(w, h, qt, restart_interval) + entropy_encode(coefficients, restart_interval) + b'\xff\xd9'


def encode(planes, quality, restart_interval):
    planes = np.asarray(planes)
    qt = quant_tables(quality)
    return assemble(planes.shape[2], planes.shape[1], qt, restart_interval, quantise(dct_values(planes), qt))


Parsed = collections.namedtuple('Parsed', 'w h qtables restart_interval coefficients stats')


class _BitReader(object):
    """Bits of one restart interval; un-stuffs FF 00 and stops at a marker."""

    def __init__(self, data, pos, stats):
        self.d, self.pos, self.acc, self.n, self.stats = data, pos, 0, 0, stats

    def _fill(self):
        if self.pos >= len(self.d):
            raise JpegError('entropy-coded data runs past the end of the file')
        byte = self.d[self.pos]
        if byte == 0xff:
            if self.pos + 1 >= len(self.d) or self.d[self.pos + 1] != 0:
                raise JpegError('marker inside an interval at byte %d' % self.pos)
            self.pos += 1
            self.stats['stuffed'] += 1
        self.pos += 1
        self.acc = (self.acc << 8) | byte
        self.n += 8

    def bit(self):
        if not self.n:
            self._fill()
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, count):
        v = 0
        for _ in range(count):
            v = v << 1 | self.bit()
        return v

    def symbol(self, dec):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.bit()
            sym = dec.get((length, code))
            if sym is not None:
                return sym
        raise JpegError('no Huffman code matches at byte %d' % self.pos)

    def end(self):
        """The rest of the last byte must be 1-bits; returns the position behind the interval."""
        n = self.n                  # (at most 7: a byte is fetched only when none is left)
        if n and self.bits(n) != (1 << n) - 1:
            raise JpegError('padding bits are not ones before byte %d' % self.pos)
        return self.pos


def _extend(v, s):
    return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def parse(data):
    """Strict parse of a file the device (or ``encode``) wrote.  Raises JpegError on anything the format in
    include/flame_hip.h does not allow.  ``stats``: what the entropy-coded data contained."""
    data = bytes(data)
    pos = [0]

    def take(n):
        if pos[0] + n > len(data):
            raise JpegError('truncated header')
        pos[0] += n
        return data[pos[0] - n:pos[0]]

    def segment(marker):
        if take(2) != bytes([0xff, marker]):
            raise JpegError('expected marker FF%02X at byte %d' % (marker, pos[0] - 2))
        n = int.from_bytes(take(2), 'big')
        return take(n - 2)

    if take(2) != b'\xff\xd8':
        raise JpegError('no SOI')
    if segment(0xe0) != b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]):
        raise JpegError('APP0 is not JFIF 1.01, units 0, density 1:1, no thumbnail')
    qt = np.zeros((2, 64), np.int64)
    for t in range(2):
        body = segment(0xdb)
        if len(body) != 65 or body[0] != t:
            raise JpegError('DQT %d is not one 8-bit table with id %d' % (t, t))
        qt[t, ZIGZAG] = list(body[1:])
    if (qt < 1).any():
        raise JpegError('zero quantiser')
    sof = segment(0xc0)
    if len(sof) != 15 or sof[0] != 8 or sof[5:] != bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]):
        raise JpegError('SOF0 is not 8 bit, components 1, 2, 3 sampled 1x1 with tables 0, 1, 1')
    h, w = int.from_bytes(sof[1:3], 'big'), int.from_bytes(sof[3:5], 'big')
    if not w or not h:
        raise JpegError('empty frame')
    for ident, (bits, vals) in DHT_ORDER:
        if segment(0xc4) != bytes([ident]) + bytes(bits) + bytes(vals):
            raise JpegError('DHT %02x is not the Annex K table' % ident)
    dri = segment(0xdd)
    if len(dri) != 2:
        raise JpegError('bad DRI')
    ri = int.from_bytes(dri, 'big')
    if ri < 1:
        raise JpegError('restart interval 0')
    if segment(0xda) != bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]):
        raise JpegError('SOS is not one interleaved baseline scan of the three components')
    if pos[0] != HEADER_BYTES:
        raise JpegError('header of %d bytes' % pos[0])

    nmcu = ((w + 7) // 8) * ((h + 7) // 8)
    nint = (nmcu + ri - 1) // ri
    coef = np.zeros((3, nmcu, 64), np.int64)
    stats = dict(stuffed=0, zrl=0, eob=0, blocks=0, blocks_without_eob=0, eob_only_blocks=0, dc_zero_diffs=0, max_zero_run=0,
                 dc_categories=[0] * 12, ac_categories=[0] * 11, intervals=nint, rst=[], last_interval_mcus=nmcu - (nint - 1) * ri,
                 interval_bytes=[])
    p = pos[0]
    for it in range(nint):
        br, pred = _BitReader(data, p, stats), [0, 0, 0]
        for m in range(it * ri, min(nmcu, (it + 1) * ri)):
            for c in range(3):
                s = br.symbol(_DEC['dc'][min(c, 1)])
                if s > 11:
                    raise JpegError('DC category %d' % s)
                diff = _extend(br.bits(s), s) if s else 0
                stats['dc_categories'][s] += 1
                stats['dc_zero_diffs'] += diff == 0
                pred[c] += diff
                coef[c, m, 0] = pred[c]
                k, eob, nsym, zeros = 1, False, 0, 0
                while k < 64:
                    sym = br.symbol(_DEC['ac'][min(c, 1)])
                    nsym += 1
                    run, s = sym >> 4, sym & 15
                    if s == 0:
                        if run == 15:
                            stats['zrl'] += 1
                            k += 16
                            zeros += 16
                            if k > 63:
                                raise JpegError('ZRL runs past the block')
                            continue
                        if run != 0:
                            raise JpegError('AC symbol %02x' % sym)
                        stats['eob'] += 1
                        eob = True
                        break
                    if s > 10:
                        raise JpegError('AC category %d' % s)
                    k += run
                    if k > 63:
                        raise JpegError('run past the block')
                    stats['max_zero_run'] = max(stats['max_zero_run'], zeros + run)
                    zeros = 0
                    coef[c, m, k] = _extend(br.bits(s), s)
                    if coef[c, m, k] == 0:
                        raise JpegError('coded zero')
                    stats['ac_categories'][s] += 1
                    k += 1
                stats['blocks'] += 1
                stats['blocks_without_eob'] += not eob
                stats['eob_only_blocks'] += eob and nsym == 1
        q = br.end()
        stats['interval_bytes'].append(q - p)
        p = q
        if it + 1 < nint:
            if data[p:p + 2] != bytes([0xff, 0xd0 + (it & 7)]):
                raise JpegError('expected RST%d behind interval %d' % (it & 7, it))
            stats['rst'].append(it & 7)
            p += 2
    if data[p:] != b'\xff\xd9':
        raise JpegError('expected EOI and the end of the file at byte %d' % p)
    return Parsed(w, h, qt, ri, coef, stats)


def idct_planes(coefficients, qt, w, h):
    """float64 planes (before rounding) from coefficients [3][blocks][64] zigzag."""
    qz = np.stack([qt[0], qt[1], qt[1]])[:, ZIGZAG]
    F = np.zeros(coefficients.shape, np.float64)
    F[:, :, ZIGZAG] = coefficients * qz[:, None, :]
    bh, bw = (h + 7) // 8, (w + 7) // 8
    b = np.einsum('vy,cbvu,ux->cbyx', _C, F.reshape(3, -1, 8, 8), _C)
    p = b.reshape(3, bh, bw, 8, 8).transpose(0, 1, 3, 2, 4).reshape(3, 8 * bh, 8 * bw)
    return p[:, :h, :w] + 128.0


def decode(data):
    """u8 [3][h][w] Y, Cb, Cr."""
    ps = parse(data)
    return np.clip(np.rint(idct_planes(ps.coefficients, ps.qtables, ps.w, ps.h)), 0, 255).astype(np.uint8)
