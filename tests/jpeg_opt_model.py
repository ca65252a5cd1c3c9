"""
Model of the device JPEG encoder's optimised Huffman tables (include/flame_hip.h, FL_JPEG_OPTIMIZE): numpy only.
The DCT, the quantiser, the header and the Annex K tables are jpeg_model's and jpeg420_model's; the length-limited Huffman
construction is png_model.limited_lengths.

The file is the one those models write but for BITS / HUFFVAL of the four DHT segments and the bits of the scan.  For each table
(DC luminance, AC luminance, DC chrominance, AC chrominance, the order of the file) count[s] is how often the scan emits s;
freq[s] = 2 * count[s] + 2 for every legal symbol and 1 for a pseudo-symbol behind the alphabet (index 12 / 256); the lengths are
limited_lengths(freq, 16); BITS[l] counts the legal symbols of length l, HUFFVAL orders them by (length, symbol), the codes
follow T.81 Annex C.  A table whose lengths do not cost the frame fewer code bits (sum count * length) than Annex K's table of
the same kind is Annex K's table instead, which obeys the same rules of order: with all four kept the file is the standard file.

  symbols(coefficients, ri, sampling) -> Symbols           what the scan emits, as arrays
  counts(coefficients, ri, sampling) -> [4][256]
  table_of(count, index) -> (BITS, HUFFVAL);  tables(coefficients, ri, sampling) -> four of them
  assemble(w, h, qt, ri, coefficients, sampling, tabs=None) -> bytes      tabs None: the optimised tables; STANDARD: Annex K's
  parse(data, optimised=True) -> Parsed                    a strict decoder that reads its tables from the file
  unlimited_depth(count, ac) -> the longest code Huffman's construction gives those frequencies with no limit

Coefficients are laid out as the sampling's own model has them: 4:4:4 [3][blocks][64], 4:2:0 [mcus][6][64].
"""
import collections
import re

import numpy as np

import jpeg_model as J
import jpeg420_model as M
import png_model

S444, S420 = 0, 1
HEADER_BYTES = J.HEADER_BYTES
DHT_BODY = (182, 215, 398, 431)           # where BITS starts in the header: SOI 2, APP0 18, DQT 2 x 69, SOF0 19, then FFC4 len(2) Tc|Th
DHT_SYMBOLS = (12, 162, 12, 162)
LEGAL = (list(range(12)), sorted([0x00, 0xf0] + [r << 4 | s for r in range(16) for s in range(1, 11)]))      # DC, AC
STANDARD = tuple(t for _, t in J.DHT_ORDER)
MAX_CODE = 16
_CAT = np.array([int(v).bit_length() for v in range(4096)])

Symbols = collections.namedtuple('Symbols', 'nblk table interval dcat diff blk k v nzrl sym eob')
Parsed = collections.namedtuple('Parsed', 'w h qtables restart_interval coefficients stats sampling tables')


def scan_order(coefficients, sampling):
    """-> blocks [n][64] in the order of the scan, and per block its table (0, 1), component and MCU."""
    c = np.asarray(coefficients).astype(np.int64)
    if sampling == S420:
        nmcu = c.shape[0]
        return c.reshape(-1, 64), np.tile(M.TABLE_OF_SLOT, nmcu), np.tile(M.COMP_OF_SLOT, nmcu), np.repeat(np.arange(nmcu), 6)
    nmcu = c.shape[1]
    return c.transpose(1, 0, 2).reshape(-1, 64), np.tile([0, 1, 1], nmcu), np.tile([0, 1, 2], nmcu), np.repeat(np.arange(nmcu), 3)


def symbols(coefficients, ri, sampling):
    B, table, comp, mcu = scan_order(coefficients, sampling)
    nblk, interval = len(B), mcu // ri
    diff = np.zeros(nblk, np.int64)
    for c in range(3):                                        # the predictor: the component's previous block, 0 at an interval's start
        idx = np.flatnonzero(comp == c)
        dc, iv = B[idx, 0], interval[idx]
        prev = np.concatenate([[0], dc[:-1]])
        same = np.concatenate([[False], iv[1:] == iv[:-1]])
        diff[idx] = dc - np.where(same, prev, 0)
    blk, k = np.nonzero(B[:, 1:])
    k = k + 1
    v = B[blk, k]
    first = np.concatenate([[True], blk[1:] != blk[:-1]])
    run = k - np.where(first, 0, np.concatenate([[0], k[:-1]])) - 1
    lastk = np.zeros(nblk, np.int64)
    np.maximum.at(lastk, blk, k)
    return Symbols(nblk, table, interval, _CAT[np.abs(diff)], diff, blk, k, v, run >> 4, (run & 15) << 4 | _CAT[np.abs(v)], lastk < 63)


def counts(coefficients, ri, sampling):
    """[4][256] in the order of the file; a DC table uses the first 12."""
    s = symbols(coefficients, ri, sampling)
    out = np.zeros((4, 256), np.int64)
    for t in range(2):
        out[2 * t] = np.bincount(s.dcat[s.table == t], minlength=256)
        mine = s.table[s.blk] == t
        out[2 * t + 1] = np.bincount(s.sym[mine], minlength=256)
        out[2 * t + 1, 0xf0] += s.nzrl[mine].sum()
        out[2 * t + 1, 0x00] += s.eob[s.table == t].sum()
    return out


def _freq(count, ac):
    n = 256 if ac else 12
    freq = [0] * (n + 1)
    for s in LEGAL[ac]:
        freq[s] = 2 * int(count[s]) + 2
    freq[n] = 1                                               # the pseudo-symbol: strictly the rarest, so it takes a longest code
    return freq


def table_of(count, index):
    """index: 0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance."""
    ac = index & 1
    lens = png_model.limited_lengths(_freq(count, ac), MAX_CODE)
    annex = J.huff_codes(STANDARD[index])
    if sum(int(count[s]) * lens[s] for s in LEGAL[ac]) >= sum(int(count[s]) * annex[s][1] for s in LEGAL[ac]):
        return [list(v) for v in STANDARD[index]]
    vals = sorted(LEGAL[ac], key=lambda s: (lens[s], s))
    return [sum(1 for s in LEGAL[ac] if lens[s] == l) for l in range(1, 17)], vals


def unlimited_depth(count, ac):
    freq = _freq(count, ac)
    return max(png_model.limited_lengths(freq, len(freq)))


def tables(coefficients, ri, sampling):
    cnt = counts(coefficients, ri, sampling)
    return tuple(table_of(cnt[i], i) for i in range(4))


def _lookup(tab):
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for sym, (c, l) in J.huff_codes(tab).items():
        code[sym], length[sym] = c, l
    return code, length


def _value_bits(v, s):
    return np.where(v >= 0, v, v - 1) & ((1 << s) - 1)


def entropy_encode(coefficients, ri, sampling, tabs):
    """The scan's data with the tables `tabs` (four (BITS, HUFFVAL) in the order of the file), RSTm markers included."""
    s = symbols(coefficients, ri, sampling)
    lut = [_lookup(t) for t in tabs]
    dcc, dcl = (np.stack([lut[0][i], lut[2][i]]) for i in range(2))
    acc, acl = (np.stack([lut[1][i], lut[3][i]]) for i in range(2))
    allb = np.arange(s.nblk)
    tnz = s.table[s.blk]
    hasv = s.dcat > 0
    zb, zk = np.repeat(s.blk, s.nzrl), np.repeat(s.k, s.nzrl)
    eb = allb[s.eob]
    # tokens (block, position, order within the position, code, length): DC code, DC value, ZRLs, AC code, AC value, EOB
    parts = [(allb, 0, 0, dcc[s.table, s.dcat], dcl[s.table, s.dcat]),
             (allb[hasv], 0, 1, _value_bits(s.diff[hasv], s.dcat[hasv]), s.dcat[hasv]),
             (zb, zk, 0, acc[s.table[zb], 0xf0], acl[s.table[zb], 0xf0]),
             (s.blk, s.k, 1, acc[tnz, s.sym], acl[tnz, s.sym]),
             (s.blk, s.k, 2, _value_bits(s.v, s.sym & 15), s.sym & 15),
             (eb, 64, 0, acc[s.table[eb], 0], acl[s.table[eb], 0])]
    if any((p[4] < 1).any() for p in parts):
        raise ValueError('a table has no code for a symbol the scan emits')
    blk = np.concatenate([p[0] for p in parts])
    key = blk * 198 + np.concatenate([np.broadcast_to(p[1], p[0].shape) for p in parts]) * 3 + np.concatenate([np.full(p[0].shape, p[2]) for p in parts])
    code, length = np.concatenate([p[3] for p in parts]), np.concatenate([p[4] for p in parts])
    nint = int(s.interval[-1]) + 1
    ibits = np.bincount(s.interval[blk], weights=length, minlength=nint).astype(np.int64)
    pad = (-ibits) % 8                                        # an interval is padded to a byte with 1-bits
    lastblk = np.flatnonzero(np.concatenate([s.interval[1:] != s.interval[:-1], [True]]))
    padded = pad > 0
    key = np.concatenate([key, lastblk[padded] * 198 + 65 * 3])
    code, length = np.concatenate([code, (1 << pad[padded]) - 1]), np.concatenate([length, pad[padded]])
    order = np.argsort(key, kind='stable')
    code, length = code[order], length[order]
    start = np.cumsum(length) - length
    j = np.arange(int(length.sum())) - np.repeat(start, length)
    bits = (np.repeat(code, length) >> (np.repeat(length, length) - 1 - j)) & 1
    raw = np.packbits(bits.astype(np.uint8)).tobytes()
    ends = np.cumsum((ibits + pad) // 8)
    out, p = bytearray(), 0
    for it in range(nint):
        out += raw[p:ends[it]].replace(b'\xff', b'\xff\x00')
        p = ends[it]
        if it + 1 < nint:
            out += bytes([0xff, 0xd0 + (it & 7)])
    return bytes(out)


def header(w, h, qt, ri, sampling, tabs):
    out = bytearray((M.header if sampling == S420 else J.header)(w, h, qt, ri))
    for off, n, (bits, vals) in zip(DHT_BODY, DHT_SYMBOLS, tabs):
        assert len(bits) == 16 and len(vals) == n
        out[off:off + 16 + n] = bytes(bits) + bytes(vals)
    return bytes(out)


def assemble(w, h, qt, ri, coefficients, sampling, tabs=None):
    if tabs is None:
        tabs = tables(coefficients, ri, sampling)
    return header(w, h, qt, ri, sampling, tabs) + entropy_encode(coefficients, ri, sampling, tabs) + b'\xff\xd9'


def encode(planes, quality, ri, sampling, tabs=None):
    planes = np.asarray(planes)
    mod = M if sampling == S420 else J
    qt = J.quant_tables(quality)
    return assemble(planes.shape[2], planes.shape[1], qt, ri, mod.quantise(mod.dct_values(planes), qt), sampling, tabs)


def check_table(tab, ac):
    """What the format asks of a DHT: all the legal symbols, each once, by (length, symbol); a code that is complete but for the
    one all-ones codeword of the longest length, which stays unassigned."""
    bits, vals = tab
    if sorted(vals) != LEGAL[ac]:
        raise J.JpegError('HUFFVAL is not the %d legal symbols, each once' % len(LEGAL[ac]))
    if sum(bits) != len(vals) or len(bits) != MAX_CODE:
        raise J.JpegError('BITS does not count HUFFVAL in lengths 1..16')
    lmax = max(l for l in range(1, 17) if bits[l - 1])
    if sum(bits[l - 1] << (16 - l) for l in range(1, 17)) != (1 << 16) - (1 << (16 - lmax)):
        raise J.JpegError('the Kraft sum is not 1 - 2^-Lmax')
    codes = J.huff_codes(tab)
    if any(c == (1 << l) - 1 for c, l in codes.values()):
        raise J.JpegError('an all-ones codeword')
    if vals != sorted(vals, key=lambda s: (codes[s][1], s)):
        raise J.JpegError('HUFFVAL is not ordered by (length, symbol)')


def _decoder(tab):
    sym, length = [0] * 65536, [0] * 65536
    for s, (c, l) in J.huff_codes(tab).items():
        lo, hi = c << (16 - l), (c + 1) << (16 - l)
        sym[lo:hi] = [s] * (hi - lo)
        length[lo:hi] = [l] * (hi - lo)
    return sym, length


def parse(data, optimised=True):
    """Strict parse of a 4:4:4 or 4:2:0 file.  The header must be the one the sampling's model writes for the size, quantiser
    tables and restart interval it declares, but for BITS / HUFFVAL, which must pass check_table (optimised) or be Annex K's
    (not optimised); the entropy-coded data is decoded with the file's tables and held to what jpeg_model.parse asks of it:
    RST numbering, stuffing, 1-padding, legal symbols, no coded zero, EOI and the end of the file."""
    data = bytes(data)
    if len(data) < HEADER_BYTES + 2:
        raise J.JpegError('truncated header')
    qt = np.zeros((2, 64), np.int64)
    for t in range(2):
        qt[t, J.ZIGZAG] = list(data[20 + 69 * t + 5:20 + 69 * t + 69])
    h, w = int.from_bytes(data[163:165], 'big'), int.from_bytes(data[165:167], 'big')
    ri = int.from_bytes(data[HEADER_BYTES - 16:HEADER_BYTES - 14], 'big')
    if not w or not h or ri < 1 or (qt < 1).any():
        raise J.JpegError('empty frame, restart interval 0 or zero quantiser')
    if data[M.SOF0_SAMPLING] not in (0x11, 0x22):
        raise J.JpegError('SOF0 samples Y neither 1x1 nor 2x2')
    sampling = S420 if data[M.SOF0_SAMPLING] == 0x22 else S444
    tabs = tuple((list(data[off:off + 16]), list(data[off + 16:off + 16 + n])) for off, n in zip(DHT_BODY, DHT_SYMBOLS))
    if data[:HEADER_BYTES] != header(w, h, qt, ri, sampling, tabs):
        raise J.JpegError('the header is not SOI, APP0, DQT x2, SOF0, DHT x4 (12, 162, 12, 162 symbols), DRI, SOS')
    if optimised:
        for i, tab in enumerate(tabs):
            check_table(tab, i & 1)
    elif tabs != tuple((list(b), list(v)) for b, v in STANDARD):
        raise J.JpegError('the tables are not Annex K')
    dec = [_decoder(t) for t in tabs]

    if sampling == S420:
        mw, mh = M.mcus(w, h)
        order = [(M.COMP_OF_SLOT[s], M.TABLE_OF_SLOT[s]) for s in range(6)]
    else:
        mw, mh = (w + 7) // 8, (h + 7) // 8
        order = [(0, 0), (1, 1), (2, 1)]
    nmcu = mw * mh
    nint = (nmcu + ri - 1) // ri
    body = data[HEADER_BYTES:]
    marks = [(m.start(), body[m.start() + 1]) for m in re.finditer(b'\xff[^\x00]', body, re.S)]
    if len(marks) != nint or marks[-1] != (len(body) - 2, 0xd9):
        raise J.JpegError('%d markers behind the header, not %d of which the last is EOI at the end of the file' % (len(marks), nint))
    coef = np.zeros((nmcu, len(order), 64), np.int64)
    stats = dict(stuffed=0, zrl=0, eob=0, blocks=0, blocks_without_eob=0, eob_only_blocks=0, dc_zero_diffs=0, max_zero_run=0,
                 dc_categories=[0] * 12, dc11_by_component=[0, 0, 0], ac_categories=[0] * 11, intervals=nint, rst=[],
                 last_interval_mcus=nmcu - (nint - 1) * ri, interval_bytes=[])
    p = 0
    for it, (at, marker) in enumerate(marks):
        if it + 1 < nint:
            if marker != 0xd0 + (it & 7):
                raise J.JpegError('expected RST%d behind interval %d' % (it & 7, it))
            stats['rst'].append(it & 7)
        seg = body[p:at]
        p = at + 2
        stats['interval_bytes'].append(len(seg))
        stats['stuffed'] += seg.count(b'\xff')
        raw = seg.replace(b'\xff\x00', b'\xff')
        nbits, top = 8 * len(raw), 8 * len(raw) + 32
        val, pos = int.from_bytes(raw + b'\xff\xff\xff\xff', 'big'), 0
        pred = [0, 0, 0]
        for m in range(it * ri, min(nmcu, (it + 1) * ri)):
            for slot, (c, t) in enumerate(order):
                dsym, dlen = dec[2 * t]
                asym, alen = dec[2 * t + 1]
                if pos > nbits:
                    raise J.JpegError('interval %d runs past its bytes' % it)
                win =(val >> (top - pos - 16)) & 0xffff
                s = dsym[win]
                if not dlen[win]:
                    raise J.JpegError('no Huffman code matches in interval %d' % it)
                pos += dlen[win]
                diff = 0
                if s:
                    diff = (val >> (top - pos - s)) & ((1 << s) - 1)
                    pos += s
                    diff = J._extend(diff, s)
                stats['dc_categories'][s] += 1
                stats['dc11_by_component'][c] += s == 11
                stats['dc_zero_diffs'] += diff == 0
                pred[c] += diff
                z = coef[m, slot]
                z[0] = pred[c]
                k, eob, nsym, zeros = 1, False, 0, 0
                while k < 64:
                    if pos > nbits:
                        raise J.JpegError('interval %d runs past its bytes' % it)
                    win = (val >> (top - pos - 16)) & 0xffff
                    sym = asym[win]
                    if not alen[win]:
                        raise J.JpegError('no Huffman code matches in interval %d' % it)
                    pos += alen[win]
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
                        stats['eob'] += 1
                        eob = True
                        break
                    k += run
                    if k > 63:
                        raise J.JpegError('run past the block')
                    if zeros + run > stats['max_zero_run']:
                        stats['max_zero_run'] = zeros + run
                    zeros = 0
                    v = J._extend((val >> (top - pos - s)) & ((1 << s) - 1), s)
                    pos += s
                    if v == 0:
                        raise J.JpegError('coded zero')
                    z[k] = v
                    stats['ac_categories'][s] += 1
                    k += 1
                stats['blocks'] += 1
                stats['blocks_without_eob'] += not eob
                stats['eob_only_blocks'] += eob and nsym == 1
        left = nbits - pos
        if left < 0 or left > 7:
            raise J.JpegError('interval %d ends %d bits before its marker' % (it, left))
        if left and (val >> 32) & ((1 << left) - 1) != (1 << left) - 1:
            raise J.JpegError('padding bits are not ones in interval %d' % it)
    if sampling == S444:
        coef = np.ascontiguousarray(coef.transpose(1, 0, 2))
    return Parsed(w, h, qt, ri, coef, stats, sampling, tabs)
