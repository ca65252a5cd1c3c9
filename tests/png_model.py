"""
A model of what a PNG file holds, in pure Python and numpy (no device, no zlib, no Pillow): a chunk parser that checks every
CRC-32 itself, an inflate (RFC 1950 / 1951) that returns the bytes together with statistics per block and per segment, the five
unfilters of the PNG specification and an Adler-32.  tests/test_cpu_png.py holds it to zlib and Pillow; tests/test_gpu_png.py
reads the device encoder's files with it.
"""
import struct

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
HEADER_BYTES = 33                 # signature + IHDR
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class PngError(ValueError):
    pass


def _crc_table():
    t = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ 0xedb88320 if c & 1 else c >> 1
        t.append(c)
    return t


_CRC = _crc_table()


def crc32(data, crc=0):
    c = crc ^ 0xffffffff
    for b in data:
        c = _CRC[(c ^ b) & 0xff] ^ (c >> 8)
    return c ^ 0xffffffff


def adler32(data):
    """Adler-32 of bytes (RFC 1950), in exact integer arithmetic."""
    d = np.frombuffer(bytes(data), np.uint8).astype(np.uint64)
    n = len(d)
    a = (1 + int(d.sum())) % 65521
    b = (n + sum(int(((np.uint64(n) - np.arange(lo, min(lo + 65536, n), dtype=np.uint64)) * d[lo:lo + 65536]).sum())
                 for lo in range(0, n, 65536))) % 65521
    return b << 16 | a


def chunks(data):
    """[(tag, body)] of a PNG file; every length and CRC-32 is checked, and nothing may follow IEND."""
    if data[:8] != SIGNATURE:
        raise PngError('no PNG signature')
    out, p = [], 8
    while p < len(data):
        if p + 12 > len(data):
            raise PngError('a chunk is cut short')
        n, = struct.unpack('>I', data[p:p + 4])
        tag, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        if p + 12 + n > len(data):
            raise PngError('chunk %r passes the end of the file' % tag)
        if struct.unpack('>I', data[p + 8 + n:p + 12 + n])[0] != crc32(tag + body):
            raise PngError('CRC-32 of chunk %r at %d is wrong' % (tag, p))
        out.append((tag, body))
        p += 12 + n
        if tag == b'IEND':
            break
    if not out or out[-1][0] != b'IEND' or p != len(data):
        raise PngError('the file does not end with IEND')
    return out


class _Huff(object):
    """A canonical prefix code (RFC 1951 3.2.2) from code lengths; `complete`, and an error when over-subscribed."""

    def __init__(self, lengths, what):
        self.lengths = list(lengths)
        self.maxlen = max(self.lengths) if self.lengths else 0
        count = [0] * (self.maxlen + 1)
        for ln in self.lengths:
            count[ln] += 1
        count[0] = 0
        kraft = sum(c << (self.maxlen - ln) for ln, c in enumerate(count) if ln)
        if self.maxlen and kraft > 1 << self.maxlen:
            raise PngError('over-subscribed %s code' % what)
        self.complete = self.maxlen > 0 and kraft == 1 << self.maxlen
        self.used = sum(count)
        code, nxt = 0, [0] * (self.maxlen + 2)
        for bits in range(1, self.maxlen + 1):
            code = (code + count[bits - 1]) << 1
            nxt[bits] = code
        self.table = {}
        for sym, ln in enumerate(self.lengths):
            if ln:
                self.table[(ln, nxt[ln])] = sym
                nxt[ln] += 1


class _BitReader(object):
    def __init__(self, data):
        self.data, self.pos = data, 0            # pos in bits

    def bits(self, n):
        v = 0
        for i in range(n):
            byte = self.pos >> 3
            if byte >= len(self.data):
                raise PngError('the deflate stream is cut short')
            v |= (self.data[byte] >> (self.pos & 7) & 1) << i
            self.pos += 1
        return v

    def symbol(self, huff):
        code = 0
        for ln in range(1, huff.maxlen + 1):
            code = code << 1 | self.bits(1)
            sym = huff.table.get((ln, code))
            if sym is not None:
                return sym
        raise PngError('a code that the table does not hold')


_FIXED_LIT = _Huff([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, 'fixed')
_FIXED_DIST = _Huff([5] * 30, 'fixed distance')


def inflate(data, seg=None):
    """
    (bytes, blocks, end position in bytes) of a raw deflate stream.  blocks: one dict per block with `type` (0 stored, 1 fixed,
    2 dynamic), `final`, `start` / `end` (output offsets), `bit_start` / `bit_end` (bit positions in the stream), `literals`,
    `matches` = [(length, distance, output offset)], and for dynamic blocks `max_lit_len`, `max_dist_len`, `max_cl_len`,
    `lit_complete`, `dist_complete`, `cl_complete`, `dist_codes_used` (number of distance codes of non-zero length),
    `dist_lengths`.  With `seg`, a match that reaches before the start of its segment of `seg` output bytes, or past its end, is an error.
    """
    rd, out, blocks = _BitReader(data), bytearray(), []
    while True:
        blk = dict(bit_start=rd.pos, start=len(out), literals=0, matches=[])
        blk['final'], blk['type'] = rd.bits(1), rd.bits(2)
        if blk['type'] == 0:
            rd.pos = (rd.pos + 7) & ~7
            n, nn = rd.bits(16), rd.bits(16)
            if n ^ nn != 0xffff:
                raise PngError('stored block: LEN and NLEN disagree')
            byte = rd.pos >> 3
            if byte + n > len(data):
                raise PngError('the deflate stream is cut short')
            out += data[byte:byte + n]
            rd.pos += 8 * n
            blk['literals'] = n
        elif blk['type'] in (1, 2):
            if blk['type'] == 1:
                lit, dist = _FIXED_LIT, _FIXED_DIST
            else:
                hlit, hdist, hclen = rd.bits(5) + 257, rd.bits(5) + 1, rd.bits(4) + 4
                if hlit > 286 or hdist > 30:
                    raise PngError('too many codes')
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = rd.bits(3)
                clh = _Huff(cl, 'code-length')
                if not clh.complete:
                    raise PngError('incomplete code-length code')
                lens = []
                while len(lens) < hlit + hdist:
                    s = rd.symbol(clh)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise PngError('repeat with nothing before it')
                        lens += [lens[-1]] * (3 + rd.bits(2))
                    else:
                        lens += [0] * (3 + rd.bits(3) if s == 17 else 11 + rd.bits(7))
                if len(lens) != hlit + hdist:
                    raise PngError('code lengths run past their count')
                if lens[256] == 0:
                    raise PngError('no end-of-block code')
                lit, dist = _Huff(lens[:hlit], 'literal/length'), _Huff(lens[hlit:], 'distance')
                if not lit.complete:
                    raise PngError('incomplete literal/length code')
                if not dist.complete and not (dist.used <= 1 and dist.maxlen <= 1):      # zlib: a lone distance code of length 1, or none at all
                    raise PngError('incomplete distance code')
                blk.update(max_lit_len=lit.maxlen, max_dist_len=dist.maxlen, max_cl_len=clh.maxlen, lit_complete=lit.complete,
                           dist_complete=dist.complete, cl_complete=clh.complete, dist_codes_used=dist.used, dist_lengths=list(lens[hlit:]),
                           lit_lengths=list(lens[:hlit]))
            while True:
                s = rd.symbol(lit)
                if s < 256:
                    out.append(s)
                    blk['literals'] += 1
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise PngError('length symbol %d' % s)
                    length = LEN_BASE[s - 257] + rd.bits(LEN_EXTRA[s - 257])
                    if dist.maxlen == 0:
                        raise PngError('a match in a block without distance codes')
                    d = rd.symbol(dist)
                    if d > 29:
                        raise PngError('distance symbol %d' % d)
                    distance = DIST_BASE[d] + rd.bits(DIST_EXTRA[d])
                    at = len(out)
                    if distance > at or (seg and distance > at % seg):
                        raise PngError('a match at %d reaches %d back: before the start of the %s' % (at, distance, 'segment' if seg else 'stream'))
                    if seg and at // seg != (at + length - 1) // seg:
                        raise PngError('a match of %d at %d crosses the end of its segment' % (length, at))
                    blk['matches'].append((length, distance, at))
                    if distance == 1:
                        out += out[-1:] * length
                    else:
                        for _ in range(length):
                            out.append(out[-distance])
        else:
            raise PngError('block type 3')
        blk['end'], blk['bit_end'] = len(out), rd.pos
        blocks.append(blk)
        if blk['final']:
            break
    return bytes(out), blocks, (rd.pos + 7) >> 3


def zlib_inflate(data, seg=None):
    """(bytes, blocks) of a zlib stream: header, deflate blocks, Adler-32 (all checked; nothing may follow)."""
    if len(data) < 6:
        raise PngError('a zlib stream has at least 6 bytes')
    cmf, flg = data[0], data[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31 or flg & 0x20:
        raise PngError('zlib header %02x %02x' % (cmf, flg))
    out, blocks, end = inflate(data[2:], seg)
    if len(data) != 2 + end + 4:
        raise PngError('%d bytes behind the last block, where the Adler-32 takes 4' % (len(data) - 2 - end))
    if struct.unpack('>I', data[2 + end:])[0] != adler32(out):
        raise PngError('Adler-32 is wrong')
    return out, blocks


def _paeth(a, b, c):
    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter(filtered, w, h, ch):
    """(pixels u8 [h][w][ch], filter bytes) from the filtered stream of an 8-bit image (PNG specification, section 9)."""
    row = 1 + w * ch
    if len(filtered) != h * row:
        raise PngError('%d filtered bytes for %d rows of %d' % (len(filtered), h, row))
    f = np.frombuffer(filtered, np.uint8).reshape(h, row)
    out = np.zeros((h, w * ch), np.uint8)
    zero = np.zeros(w * ch, np.uint8)
    for y in range(h):
        ft, line, up = int(f[y, 0]), f[y, 1:], out[y - 1] if y else zero
        if ft == 0:
            out[y] = line
        elif ft == 2:
            out[y] = line + up
        elif ft == 1:
            for c in range(ch):
                out[y, c::ch] = np.cumsum(line[c::ch], dtype=np.uint64).astype(np.uint8)
        elif ft in (3, 4):
            cur, upl, res = [0] * (w * ch), [int(v) for v in up], [int(v) for v in line]
            for x in range(w * ch):
                a = cur[x - ch] if x >= ch else 0
                c = upl[x - ch] if x >= ch else 0
                pred = (a + upl[x]) >> 1 if ft == 3 else _paeth(a, upl[x], c)
                cur[x] = (res[x] + pred) & 255
            out[y] = cur
        else:
            raise PngError('filter byte %d in row %d' % (ft, y))
    return out.reshape(h, w, ch), [int(v) for v in f[:, 0]]


def filter_rows(pixels, ftype=4):
    """The filtered stream of u8 [h][w][ch] pixels with one filter type on every row (vectorised)."""
    h, w, ch = pixels.shape
    x = pixels.reshape(h, w * ch).astype(np.int64)
    a = np.zeros_like(x); a[:, ch:] = x[:, :-ch]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, ch:] = x[:-1, :-ch]
    if ftype == 0:
        pred = 0
    elif ftype == 1:
        pred = a
    elif ftype == 2:
        pred = b
    elif ftype == 3:
        pred = (a + b) >> 1
    else:
        pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    out = np.empty((h, 1 + w * ch), np.uint8)
    out[:, 0] = ftype
    out[:, 1:] = ((x - pred) & 255).astype(np.uint8)
    return out.tobytes()


class Parsed(object):
    pass


def parse(data, seg=None):
    """
    A PNG file of the form the device writes — signature, IHDR, IDATs, IEND; 8 bit, colour type 2 or 6, not interlaced — with every
    checksum verified.  Returns an object with w, h, channels, idat (the bodies), filtered, pixels, filters, blocks and `stats`:
    with `seg`, stats['segments'] lists per segment of `seg` filtered bytes its blocks, whether it is dynamic, its bytes in the
    stream and whether it ends on a byte boundary.
    """
    ck = chunks(data)
    if ck[0][0] != b'IHDR' or len(ck[0][1]) != 13:
        raise PngError('IHDR is not the first chunk')
    ps = Parsed()
    ps.w, ps.h, depth, ctype, comp, filt, lace = struct.unpack('>IIBBBBB', ck[0][1])
    if depth != 8 or ctype not in (2, 6) or comp or filt or lace:
        raise PngError('not an 8-bit truecolour, non-interlaced PNG')
    ps.channels = 3 if ctype == 2 else 4
    ps.tags = [tag for tag, _ in ck]
    ps.idat = [body for tag, body in ck if tag == b'IDAT']
    if ps.tags != [b'IHDR'] + [b'IDAT'] * len(ps.idat) + [b'IEND'] or not ps.idat:
        raise PngError('chunks %r' % ps.tags)
    ps.zstream = b''.join(ps.idat)
    ps.filtered, ps.blocks = zlib_inflate(ps.zstream, seg)
    ps.pixels, ps.filters = unfilter(ps.filtered, ps.w, ps.h, ps.channels)
    matches = [m for b in ps.blocks for m in b['matches']]
    ps.stats = dict(blocks=ps.blocks, block_types=[b['type'] for b in ps.blocks], literals=sum(b['literals'] for b in ps.blocks),
                    matches=matches, match_lengths=sorted(set(m[0] for m in matches)), distances=sorted(set(m[1] for m in matches)),
                    finals=[b['final'] for b in ps.blocks], nidat=len(ps.idat), filters=ps.filters, nfiltered=len(ps.filtered),
                    file_bytes=len(data), raw_bytes=ps.w * ps.h * ps.channels)
    if seg:
        segs, bi = [], 0
        for lo in range(0, len(ps.filtered), seg):
            hi, mine = min(lo + seg, len(ps.filtered)), []
            while bi < len(ps.blocks) and ps.blocks[bi]['start'] < hi:
                mine.append(ps.blocks[bi])
                bi += 1
            while bi < len(ps.blocks) and ps.blocks[bi]['start'] == ps.blocks[bi]['end'] == hi:      # an empty block closes the segment before it
                mine.append(ps.blocks[bi])
                bi += 1
            if not mine or mine[0]['start'] != lo or mine[-1]['end'] != hi:
                raise PngError('no block boundary at the segment boundaries %d, %d' % (lo, hi))
            coded = [b for b in mine if b['end'] > b['start']]
            segs.append(dict(blocks=mine, dynamic=any(b['type'] == 2 for b in coded), stored=all(b['type'] == 0 for b in coded),
                             bits=mine[-1]['bit_end'] - mine[0]['bit_start'], aligned=mine[-1]['bit_end'] % 8 == 0,
                             start_aligned=mine[0]['bit_start'] % 8 == 0, nbytes=hi - lo))
        ps.stats['segments'] = segs
    return ps


# ------------------------------------------------------------------ the device encoder's format, written out in Python
def _len_symbol(length):
    for i in range(28, -1, -1):
        if LEN_BASE[i] <= length:
            return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def tokens(d):
    """[byte] or [(length,)] per token of a segment: a literal for the head of every group of equal bytes, and for its r repeats
    matches of distance 1 and length min(r, 258) while r >= 3, then literals."""
    d = np.frombuffer(bytes(d), np.uint8)
    heads = np.flatnonzero(np.concatenate(([True], d[1:] != d[:-1])))
    out = []
    for at, nxt in zip(heads, np.concatenate((heads[1:], [len(d)]))):
        b, r = int(d[at]), int(nxt - at - 1)
        out.append(b)
        while r >= 3:
            out.append((min(r, 258),))
            r -= min(r, 258)
        out += [b] * r
    return out


def limited_lengths(freq, maxlen):
    """Code lengths of a complete prefix code with none above maxlen: Huffman's (ties: the lower frequency, then the lower symbol,
    leaves before inner nodes), depths cut at maxlen, and the Kraft sum repaired by lengthening the deepest code that can be."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    lens, n = [0] * len(freq), len(used)
    if n == 1:
        s = used[0][1]
        lens[s] = lens[0 if s else 1] = 1
        return lens
    if n == 0:
        return lens
    nfreq, lpar, npar, leaf, node = [], [0] * n, [0] * n, 0, 0
    for k in range(n - 1):
        f = 0
        for _ in range(2):
            if leaf < n and (node >= k or used[leaf][0] <= nfreq[node]):
                f += used[leaf][0]; lpar[leaf] = k; leaf += 1
            else:
                f += nfreq[node]; npar[node] = k; node += 1
        nfreq.append(f)
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[npar[k]] + 1
    cnt = [0] * (maxlen + 1)
    for i in range(n):
        cnt[min(depth[lpar[i]] + 1, maxlen)] += 1
    total = sum(cnt[ln] << (maxlen - ln) for ln in range(1, maxlen + 1))
    while total > 1 << maxlen:
        cnt[maxlen] -= 1
        for ln in range(maxlen - 1, 0, -1):
            if cnt[ln]:
                cnt[ln] -= 1; cnt[ln + 1] += 2
                break
        total -= 1
    i = 0
    for ln in range(maxlen, 0, -1):
        for _ in range(cnt[ln]):
            lens[used[i][1]] = ln
            i += 1
    return lens


def canonical_codes(lens):
    """{symbol: (code as sent — most significant bit first, so bit-reversed for the writer —, length)}."""
    h = _Huff(lens, 'model')
    return dict((sym, (int(format(code, '0%db' % ln)[::-1], 2), ln)) for (ln, code), sym in h.table.items())


class _BitWriter(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def deflate_segment(d, last):
    """One segment as the device codes it: a dynamic block (and, unless it is the last, an empty stored block that ends it on a
    byte boundary), or a stored block when that is no smaller."""
    n = len(d)
    stored = bytes([1 if last else 0]) + struct.pack('<HH', n, n ^ 0xffff) + bytes(d)
    toks = tokens(d)
    freq, nmatch = [0] * 286, 0
    freq[256] = 1
    for t in toks:
        if isinstance(t, tuple):
            freq[_len_symbol(t[0])[0]] += 1
            nmatch += 1
        else:
            freq[t] += 1
    lens = limited_lengths(freq, 15)
    hlit = 286
    while hlit > 257 and lens[hlit - 1] == 0:
        hlit -= 1
    seq_in, seq, i = lens[:hlit] + [1 if nmatch else 0], [], 0
    while i < len(seq_in):
        v, r = seq_in[i], 1
        while i + r < len(seq_in) and seq_in[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138); seq.append((18, k - 11, 7)); r -= k
            if r >= 3:
                seq.append((17, r - 3, 3)); r = 0
            seq += [(0, 0, 0)] * r
        else:
            seq.append((v, 0, 0)); r -= 1
            while r >= 3:
                k = min(r, 6); seq.append((16, k - 3, 2)); r -= k
            seq += [(v, 0, 0)] * r
    clfreq = [0] * 19
    for s, _, _ in seq:
        clfreq[s] += 1
    cllens = limited_lengths(clfreq, 7)
    hclen = 19
    while hclen > 4 and cllens[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    code, clcode = canonical_codes(lens), canonical_codes(cllens)
    w = _BitWriter()
    w.put(1 if last else 0, 1); w.put(2, 2); w.put(hlit - 257, 5); w.put(0, 5); w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cllens[CL_ORDER[k]], 3)
    for s, extra, nb in seq:
        w.put(*clcode[s])
        if nb:
            w.put(extra, nb)
    for t in toks:
        if isinstance(t, tuple):
            sym, eb, ev = _len_symbol(t[0])
            w.put(*code[sym])
            w.put(ev, eb + 1)                  # the extra bits, then the lone distance code: one bit, 0
        else:
            w.put(*code[t])
    w.put(*code[256])
    if not last:
        w.put(0, 3)
        w.align()
        w.out += b'\x00\x00\xff\xff'
    else:
        w.align()
    return bytes(w.out) if len(w.out) < len(stored) else stored


def encode(pixels, seg):
    """The file the device encoder writes for u8 [h][w][3 or 4] pixels with segments of `seg` filtered bytes."""
    h, w, ch = pixels.shape
    filtered = filter_rows(np.ascontiguousarray(pixels), 4)
    los = list(range(0, len(filtered), seg))
    parts = [deflate_segment(filtered[lo:lo + seg], lo == los[-1]) for lo in los]
    parts[0] = b'\x78\x01' + parts[0]
    parts[-1] += struct.pack('>I', adler32(filtered))

    def chunk(tag, body):
        return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', crc32(tag + body))
    return (SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2 if ch == 3 else 6, 0, 0, 0))
            + b''.join(chunk(b'IDAT', p) for p in parts) + chunk(b'IEND', b''))
