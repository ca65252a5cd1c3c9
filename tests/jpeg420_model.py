"""
Model of the device JPEG encoder's 4:2:0 form (include/flame_hip.h, fl_jpeg_encode_s with FL_JPEG_420) and of the AVI files
MJPEGOutput writes: numpy only, float64.  The tables, the DCT factors and the bit reader and writer are jpeg_model's.

The stream is jpeg_model's with these differences: SOF0 declares Y as 2x2 and Cb, Cr as 1x1; an MCU covers 16 x 16 pixels and
holds six blocks Y00, Y01, Y10, Y11, Cb, Cr; each chroma sample is (a + b + c + d + 2) >> 2 over the 2 x 2 full-resolution
samples, whose coordinates are clamped to w - 1, h - 1 first; the Y predictor runs through the four Y blocks of an MCU and on
into the next MCU, Cb and Cr run MCU to MCU, all three restart at 0 in every interval.

  downsample(planes) -> (Y [16 mh][16 mw], C [2][8 mh][8 mw])   integers, padded to whole MCUs
  dct_values(planes) -> float64 [mcus][6][64]                   zigzag, before quantisation
  encode / assemble / entropy_encode / header / parse / decode  as in jpeg_model, coefficients [mcus][6][64]
  read_avi(data) -> Avi                                         a strict reader of AVI 1.0 with one MJPG stream

`decode` upsamples chroma by replication: it is the model's own convention, not a decoder's (libjpeg interpolates).
"""
import collections
import struct

import numpy as np

import jpeg_model as J

HEADER_BYTES = J.HEADER_BYTES
SOF0_SAMPLING = 158 + 11          # the byte 0x22 / 0x11 of component 1: SOI 2, APP0 18, DQT 2 x 69, then FFC0 len(2) P Y(2) X(2) Nf C1
TABLE_OF_SLOT = (0, 0, 0, 0, 1, 1)
COMP_OF_SLOT = (0, 0, 0, 0, 1, 2)


def mcus(w, h):
    return (w + 15) // 16, (h + 15) // 16


def downsample(planes):
    """u8 [3][h][w] -> (Y, C): int64, padded to whole MCUs by replicating the last column / row (= clamping the coordinates)
    before the chroma average."""
    planes = np.asarray(planes)
    _, h, w = planes.shape
    mw, mh = mcus(w, h)
    p = np.pad(planes.astype(np.int64), ((0, 0), (0, 16 * mh - h), (0, 16 * mw - w)), mode='edge')
    c = p[1:]
    return p[0], (c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + 2) >> 2


def blocks_of(planes):
    """float64 [mcus][6][8][8], level shifted, in the order of the scan."""
    y, c = downsample(planes)
    mh, mw = y.shape[0] // 16, y.shape[1] // 16
    yb = y.reshape(mh, 2, 8, mw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mh * mw, 4, 8, 8)       # [mcu][2 v + u][8][8]
    cb = c.reshape(2, mh, 8, mw, 8).transpose(1, 3, 0, 2, 4).reshape(mh * mw, 2, 8, 8)
    return np.concatenate([yb, cb], axis=1).astype(np.float64) - 128.0


def dct_values(planes):
    F = np.einsum('vy,msyx,ux->msvu', J._C, blocks_of(planes), J._C)
    return F.reshape(F.shape[0], 6, 64)[:, :, J.ZIGZAG]


def _qz(qt):
    return np.asarray(qt)[list(TABLE_OF_SLOT)][:, J.ZIGZAG]             # [6][64], zigzag


def quantise(values, qt):
    return np.rint(values / _qz(qt)[None]).astype(np.int64)


def entropy_encode(coefficients, restart_interval):
    coefficients = np.asarray(coefficients)
    nmcu = coefficients.shape[0]
    out = bytearray()
    nint = (nmcu + restart_interval - 1) // restart_interval
    for it in range(nint):
        bw, pred = J._BitWriter(), [0, 0, 0]
        for m in range(it * restart_interval, min(nmcu, (it + 1) * restart_interval)):
            for slot in range(6):
                z, c, t = coefficients[m, slot], COMP_OF_SLOT[slot], TABLE_OF_SLOT[slot]
                dc_tab, ac_tab = J._ENC['dc'][t], J._ENC['ac'][t]
                diff = int(z[0]) - pred[c]
                pred[c] = int(z[0])
                s = J._cat(diff)
                bw.put(*dc_tab[s])
                if s:
                    bw.put(J._value_bits(diff, s), s)
                run = 0
                for k in range(1, 64):
                    v = int(z[k])
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bw.put(*ac_tab[0xf0])
                        run -= 16
                    s = J._cat(v)
                    bw.put(*ac_tab[run << 4 | s])
                    bw.put(J._value_bits(v, s), s)
                    run = 0
                if run:
                    bw.put(*ac_tab[0])
        bw.pad()
        out += bw.out
        if it + 1 < nint:
            out += bytes([0xff, 0xd0 + (it & 7)])
    return bytes(out)


def header(w, h, qt, restart_interval):
    """jpeg_model's header with Y declared 2x2: only the sampling byte differs."""
    out = bytearray(J.header(w, h, qt, restart_interval))
    assert out[SOF0_SAMPLING - 1:SOF0_SAMPLING + 2] == bytes([1, 0x11, 0])
    out[SOF0_SAMPLING] = 0x22
    return bytes(out)


def assemble(w, h, qt, restart_interval, coefficients):
    return header(w, h, qt, restart_interval) + entropy_encode(coefficients, restart_interval) + b'\xff\xd9'


def encode(planes, quality, restart_interval):
    planes = np.asarray(planes)
    qt = J.quant_tables(quality)
    return assemble(planes.shape[2], planes.shape[1], qt, restart_interval, quantise(dct_values(planes), qt))


Parsed = collections.namedtuple('Parsed', 'w h qtables restart_interval coefficients stats')


def parse(data):
    """Strict parse of a 4:2:0 file: the header must be, byte for byte, the one `header` writes for the size, tables and restart
    interval it declares; the entropy-coded data is decoded as jpeg_model.parse does.  Raises jpeg_model.JpegError."""
    data = bytes(data)
    if len(data) < HEADER_BYTES + 2:
        raise J.JpegError('truncated header')
    qt = np.zeros((2, 64), np.int64)
    for t in range(2):
        qt[t, J.ZIGZAG] = list(data[20 + 69 * t + 5:20 + 69 * t + 69])
    h, w = struct.unpack('>HH', data[163:167])
    ri = struct.unpack('>H', data[HEADER_BYTES - 14 - 2:HEADER_BYTES - 14])[0]
    if not w or not h or ri < 1 or (qt < 1).any():
        raise J.JpegError('empty frame, restart interval 0 or zero quantiser')
    if data[SOF0_SAMPLING] != 0x22:
        raise J.JpegError('SOF0 does not sample Y 2x2')
    if data[:HEADER_BYTES] != header(w, h, qt, ri):
        raise J.JpegError('the header is not SOI, APP0, DQT x2, SOF0 (2x2, 1x1, 1x1), DHT x4 (Annex K), DRI, SOS')

    mw, mh = mcus(w, h)
    nmcu = mw * mh
    nint = (nmcu + ri - 1) // ri
    coef = np.zeros((nmcu, 6, 64), np.int64)
    stats = dict(stuffed=0, zrl=0, eob=0, blocks=0, blocks_without_eob=0, eob_only_blocks=0, dc_zero_diffs=0, max_zero_run=0,
                 dc_categories=[0] * 12, dc11_by_component=[0, 0, 0], ac_categories=[0] * 11, intervals=nint, rst=[],
                 last_interval_mcus=nmcu - (nint - 1) * ri, interval_bytes=[])
    p = HEADER_BYTES
    for it in range(nint):
        br, pred = J._BitReader(data, p, stats), [0, 0, 0]
        for m in range(it * ri, min(nmcu, (it + 1) * ri)):
            for slot in range(6):
                c, t = COMP_OF_SLOT[slot], TABLE_OF_SLOT[slot]
                s = br.symbol(J._DEC['dc'][t])
                if s > 11:
                    raise J.JpegError('DC category %d' % s)
                diff = J._extend(br.bits(s), s) if s else 0
                stats['dc_categories'][s] += 1
                stats['dc11_by_component'][c] += s == 11
                stats['dc_zero_diffs'] += diff == 0
                pred[c] += diff
                coef[m, slot, 0] = pred[c]
                k, eob, nsym, zeros = 1, False, 0, 0
                while k < 64:
                    sym = br.symbol(J._DEC['ac'][t])
                    nsym += 1
                    run, s = sym >> 4, sym & 15
                    if s == 0:
                        if run == 15:
                            stats['zrl'] += 1
                            k += 16
                            zeros += 16
                            if k > 63:
                                raise J.JpegError('ZRL runs past the block')
                            continue
                        if run != 0:
                            raise J.JpegError('AC symbol %02x' % sym)
                        stats['eob'] += 1
                        eob = True
                        break
                    if s > 10:
                        raise J.JpegError('AC category %d' % s)
                    k += run
                    if k > 63:
                        raise J.JpegError('run past the block')
                    stats['max_zero_run'] = max(stats['max_zero_run'], zeros + run)
                    zeros = 0
                    coef[m, slot, k] = J._extend(br.bits(s), s)
                    if coef[m, slot, k] == 0:
                        raise J.JpegError('coded zero')
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
                raise J.JpegError('expected RST%d behind interval %d' % (it & 7, it))
            stats['rst'].append(it & 7)
            p += 2
    if data[p:] != b'\xff\xd9':
        raise J.JpegError('expected EOI and the end of the file at byte %d' % p)
    return Parsed(w, h, qt, ri, coef, stats)


def idct_planes(coefficients, qt, w, h):
    """(Y float64 [h][w], C float64 [2][ceil(h / 2)][ceil(w / 2)]) before rounding."""
    mw, mh = mcus(w, h)
    F = np.zeros(coefficients.shape, np.float64)
    F[:, :, J.ZIGZAG] = coefficients * _qz(qt)[None]
    b = np.einsum('vy,msvu,ux->msyx', J._C, F.reshape(-1, 6, 8, 8), J._C) + 128.0
    y = b[:, :4].reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(16 * mh, 16 * mw)
    c = b[:, 4:].reshape(mh, mw, 2, 8, 8).transpose(2, 0, 3, 1, 4).reshape(2, 8 * mh, 8 * mw)
    return y[:h, :w], c[:, :(h + 1) // 2, :(w + 1) // 2]


def decode(data):
    """u8 [3][h][w] Y, Cb, Cr; chroma upsampled by replication."""
    ps = parse(data)
    y, c = idct_planes(ps.coefficients, ps.qtables, ps.w, ps.h)
    y, c = (np.clip(np.rint(a), 0, 255).astype(np.uint8) for a in (y, c))
    up = np.repeat(np.repeat(c, 2, axis=1), 2, axis=2)[:, :ps.h, :ps.w]
    return np.concatenate([y[None], up])


# ---------------------------------------------------------------------------------------------------------------- AVI
class AviError(ValueError):
    pass


Avi = collections.namedtuple('Avi', 'avih strh strf index chunks')
_AVIH = ('dwMicroSecPerFrame dwMaxBytesPerSec dwPaddingGranularity dwFlags dwTotalFrames dwInitialFrames dwStreams '
         'dwSuggestedBufferSize dwWidth dwHeight r0 r1 r2 r3').split()
_STRH = ('fccType fccHandler dwFlags wPriority wLanguage dwInitialFrames dwScale dwRate dwStart dwLength dwSuggestedBufferSize '
         'dwQuality dwSampleSize left top right bottom').split()
_STRF = 'biSize biWidth biHeight biPlanes biBitCount biCompression biSizeImage biXPelsPerMeter biYPelsPerMeter biClrUsed biClrImportant'.split()


def read_avi(data):
    """AVI 1.0, little-endian, one MJPG video stream:
      RIFF 'AVI ' { LIST 'hdrl' { avih (56) LIST 'strl' { strh (56) strf (40) } } LIST 'movi' { 00dc ... } idx1 }
    Chunks are padded to an even length; an idx1 entry is 00dc, 0x10, the offset of the chunk's header from the 'movi' fourcc,
    the unpadded size.  Returns the three headers as dicts, the index as [(offset, size)] and the chunks' bytes; raises
    AviError on anything that does not agree with anything else."""
    data = bytes(data)

    def need(cond, what):
        if not cond:
            raise AviError(what)

    def head(pos, tag):
        need(pos + 8 <= len(data) and data[pos:pos + 4] == tag, 'expected %r at byte %d' % (tag, pos))
        return struct.unpack('<I', data[pos + 4:pos + 8])[0]

    def lst(pos, kind):
        size = head(pos, b'LIST')
        need(data[pos + 8:pos + 12] == kind and size >= 4, 'expected LIST %r at byte %d' % (kind, pos))
        return size

    need(head(0, b'RIFF') == len(data) - 8, 'the RIFF size is not the size of the file less 8')
    need(len(data) <= 2 ** 31 - 1, 'the file passes 2^31 - 1 bytes')
    need(data[8:12] == b'AVI ', 'not an AVI file')
    need(lst(12, b'hdrl') == 4 + 64 + 8 + 4 + 64 + 48, 'hdrl is not avih and one strl of strh and strf')
    need(head(24, b'avih') == 56, 'avih is not 56 bytes')
    avih = dict(zip(_AVIH, struct.unpack('<14I', data[32:88])))
    need(lst(88, b'strl') == 4 + 64 + 48, 'strl is not strh and strf')
    need(head(100, b'strh') == 56, 'strh is not 56 bytes')
    strh = dict(zip(_STRH, struct.unpack('<4s4sIHHIIIIIIII4H', data[108:164])))
    need(head(164, b'strf') == 40, 'strf is not 40 bytes')
    strf = dict(zip(_STRF, struct.unpack('<IiiHH4sIiiII', data[172:212])))
    movi = lst(212, b'movi')
    movi_fourcc, end = 220, 220 + movi
    need(end + 8 <= len(data), 'movi runs past the file')
    chunks, offsets, pos = [], [], 224
    while pos < end:
        n = head(pos, b'00dc')
        need(pos + 8 + n + (n & 1) <= end, 'a chunk runs past movi')
        need(not (n & 1) or data[pos + 8 + n] == 0, 'a padding byte is not 0')
        chunks.append(data[pos + 8:pos + 8 + n])
        offsets.append(pos - movi_fourcc)
        pos += 8 + n + (n & 1)
    need(pos == end, 'movi does not end with a chunk')
    nidx = head(end, b'idx1')
    need(end + 8 + nidx == len(data) and nidx == 16 * len(chunks), 'idx1 is not 16 bytes per chunk up to the end of the file')
    index = []
    for k in range(len(chunks)):
        tag, flags, off, size = struct.unpack('<4sIII', data[end + 8 + 16 * k:end + 24 + 16 * k])
        need(tag == b'00dc' and flags == 0x10, 'index entry %d is not a key frame of stream 0' % k)
        need((off, size) == (offsets[k], len(chunks[k])), 'index entry %d does not point at chunk %d' % (k, k))
        index.append((off, size))
    n, largest = len(chunks), max([len(c) for c in chunks] + [0])
    need(avih['dwTotalFrames'] == n and strh['dwLength'] == n, 'frame counts')
    need(avih['dwFlags'] == 0x10 and avih['dwStreams'] == 1, 'avih flags / streams')
    need(avih['dwSuggestedBufferSize'] == largest, 'dwSuggestedBufferSize is not the largest chunk')
    need(strh['fccType'] == b'vids' and strh['fccHandler'] == b'MJPG', 'strh is not a vids / MJPG stream')
    need(strh['dwScale'] >= 1 and strh['dwRate'] >= 1 and np.gcd(strh['dwScale'], strh['dwRate']) == 1, 'dwScale / dwRate is not a reduced fraction')
    need(avih['dwMicroSecPerFrame'] == int(round(1e6 * strh['dwScale'] / strh['dwRate'])), 'dwMicroSecPerFrame is not dwScale / dwRate')
    w, h = avih['dwWidth'], avih['dwHeight']
    need(w >= 1 and h >= 1 and (strf['biWidth'], strf['biHeight']) == (w, h), 'sizes of avih and strf')
    need((strf['biSize'], strf['biPlanes'], strf['biBitCount'], strf['biCompression'], strf['biSizeImage']) == (40, 1, 24, b'MJPG', w * h * 3),
         'strf is not a 24-bit MJPG BITMAPINFOHEADER')
    for c in chunks:
        need(c[:2] == b'\xff\xd8' and c[-2:] == b'\xff\xd9', 'a chunk is not a JPEG file')
        need(struct.unpack('>HH', c[163:167]) == (h, w), 'a frame is not of the size the headers give')
    return Avi(avih, strh, strf, index, chunks)
