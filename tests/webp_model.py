"""
A Python model of the device WebP encoder (csrc/webp.hip; the format is fixed in include/flame_hip.h): `encode` writes the bytes
the device must write, `decode` is a strict reader written from the format that refuses what the encoder never writes, and the
two container writers and readers are the files encoders.WebPOutput makes.  PB and EB are the predictor's and the entropy tiles'
size bits (the device: 4 and 6).
"""
import struct

import numpy as np

from png_model import canonical_codes, limited_lengths

MODES = (1, 2, 7, 10, 11, 12)
CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
ALPHABETS = (280, 256, 256, 256, 40)          # green, red, blue, alpha, distance


class WebPError(ValueError):
    pass


# ---- the encoder ------------------------------------------------------------------------------------------------------
class Bits(object):
    """Values of n bits each, least significant bit first."""

    def __init__(self):
        self.parts = []
        self.vals, self.lens, self.nbits = [], [], 0

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        self.vals.append(v)
        self.lens.append(n)
        self.nbits += n

    def extend(self, vals, lens):
        self._close()
        self.parts.append((np.asarray(vals, np.uint64), np.asarray(lens, np.int64)))
        self.nbits += int(np.sum(lens))

    def _close(self):
        if self.vals:
            self.parts.append((np.array(self.vals, np.uint64), np.array(self.lens, np.int64)))
            self.vals, self.lens = [], []

    def tobytes(self):
        self._close()
        if not self.parts:
            return b''
        vals = np.concatenate([p[0] for p in self.parts])
        lens = np.concatenate([p[1] for p in self.parts])
        keep = lens > 0
        vals, lens = vals[keep], lens[keep]
        total = int(lens.sum())
        starts = np.cumsum(lens) - lens
        within = (np.arange(total, dtype=np.int64) - np.repeat(starts, lens)).astype(np.uint64)
        bits = ((np.repeat(vals, lens) >> within) & np.uint64(1)).astype(np.uint8)
        return np.packbits(bits, bitorder='little').tobytes()


def green_subtracted(pixels, channels):
    """int [h][w][4] (r - g, g, b - g, a) mod 256; channels 3 reads every alpha as 255."""
    p = np.asarray(pixels).astype(np.int64)
    out = p.copy()
    out[..., 0] = (p[..., 0] - p[..., 1]) & 255
    out[..., 2] = (p[..., 2] - p[..., 1]) & 255
    if channels == 3:
        out[..., 3] = 255
    return out


def _avg2(a, b):
    return (a + b) >> 1


def predict(mode, L, T, TL, TR):
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 7:
        return _avg2(L, T)
    if mode == 10:
        return _avg2(_avg2(L, TL), _avg2(T, TR))
    if mode == 11:
        e = L + T - TL
        dl = np.abs(e - L).sum(axis=-1, keepdims=True)
        dt = np.abs(e - T).sum(axis=-1, keepdims=True)
        return np.where(dl < dt, L, T)
    if mode == 12:
        return np.clip(L + T - TL, 0, 255)
    raise WebPError('mode %d is not one of the six' % mode)


def neighbours(P):
    """L, T, TL, TR of every pixel (zeros where the fixed rules apply anyway); TR of the last column is pixel (0, y)."""
    L, T, TL, TR = (np.zeros_like(P) for _ in range(4))
    L[:, 1:] = P[:, :-1]
    T[1:] = P[:-1]
    TL[1:, 1:] = P[:-1, :-1]
    TR[1:, :-1] = P[:-1, 1:]
    TR[1:, -1] = P[1:, 0]
    return L, T, TL, TR


def fixed_rules(pred, P):
    pred = pred.copy()
    pred[1:, 0] = P[:-1, 0]
    pred[0, 1:] = P[0, :-1]
    pred[0, 0] = (0, 0, 0, 255)
    return pred


def mode_residuals(P):
    """{mode: residual [h][w][4]} with the fixed rules applied."""
    nb = neighbours(P)
    return dict((m, (P - fixed_rules(predict(m, *nb), P)) & 255) for m in MODES)


def _tile_sums(a, bits):
    h, w = a.shape
    t = 1 << bits
    ty, tx = -(-h // t), -(-w // t)
    pad = np.zeros((ty * t, tx * t), a.dtype)
    pad[:h, :w] = a
    return pad.reshape(ty, t, tx, t).sum(axis=(1, 3))


def choose_modes(P, PB=4):
    """(mode map [ty][tx], residual [h][w][4]): per tile the mode of least sum of min(r, 256 - r), the lowest on a tie."""
    res = mode_residuals(P)
    costs = np.stack([_tile_sums(np.minimum(res[m], 256 - res[m]).sum(axis=-1), PB) for m in MODES])
    pick = np.argmin(costs, axis=0)
    modes = np.array(MODES)[pick]
    h, w = P.shape[:2]
    full = np.repeat(np.repeat(pick, 1 << PB, axis=0), 1 << PB, axis=1)[:h, :w]
    stack = np.stack([res[m] for m in MODES])
    out = np.take_along_axis(stack, full[None, :, :, None], axis=0)[0]
    return modes, out


def code_length_tokens(lens):
    """[(kind, extra value, extra bits)] for lens[0 .. last used]: zeros in runs of 18 while at least 11 remain, then 17, then
    literal zeros; 16 is never used."""
    out, i, n = [], 0, len(lens)
    while i < n:
        if lens[i]:
            out.append((lens[i], 0, 0))
            i += 1
            continue
        run = 0
        while i + run < n and lens[i + run] == 0:
            run += 1
        i += run
        while run >= 11:
            m = min(run, 138)
            out.append((18, m - 11, 7))
            run -= m
        if run >= 3:
            out.append((17, run - 3, 3))
            run = 0
        out.extend([(0, 0, 0)] * run)
    return out


def write_code(bw, freq):
    """One prefix code from the counts; returns {symbol: (code as written, length)}, empty when the code emits no bits."""
    used = [s for s, f in enumerate(freq) if f]
    if len(used) <= 1:
        s = used[0] if used else 0
        bw.put(1, 1)
        bw.put(0, 1)
        bw.put(1 if s > 1 else 0, 1)
        bw.put(s, 8 if s > 1 else 1)
        return {}
    bw.put(0, 1)
    lens = limited_lengths(list(freq), 15)
    toks = code_length_tokens(lens[:used[-1] + 1])
    tf = [0] * 19
    for k, _, _ in toks:
        tf[k] += 1
    cl = limited_lengths(tf, 7)
    clcodes = canonical_codes(cl)
    ncl = max(4, 1 + max(i for i, k in enumerate(CL_ORDER) if cl[k]))
    bw.put(ncl - 4, 4)
    for k in CL_ORDER[:ncl]:
        bw.put(cl[k], 3)
    ntok = len(toks)
    k = max(1, -(-(ntok - 2).bit_length() // 2))
    bw.put(1, 1)
    bw.put(k - 1, 3)
    bw.put(ntok - 2, 2 * k)
    for kind, ev, eb in toks:
        c, n = clcodes[kind]
        bw.put(c, n)
        if eb:
            bw.put(ev, eb)
    return canonical_codes(lens)


def _tables(codes):
    c, n = np.zeros(256, np.uint64), np.zeros(256, np.int64)
    for s, (code, ln) in codes.items():
        if s < 256:
            c[s], n[s] = code, ln
    return c, n


def write_group(bw, hists):
    """Five codes (the distance code from no counts); returns the four (codes, lengths) tables."""
    tabs = [_tables(write_code(bw, list(hists[c]) + [0] * (ALPHABETS[c] - 256))) for c in range(4)]
    write_code(bw, [0] * 40)
    return tabs


def write_subimage(bw, green, red, alpha=255):
    """An entropy-coded image of its own: no cache, one group from its own counts, its pixels (blue 0)."""
    green, red = np.asarray(green).ravel(), np.asarray(red).ravel()
    bw.put(0, 1)
    hists = [np.bincount(green, minlength=256), np.bincount(red, minlength=256), np.bincount([0], minlength=256),
             np.bincount([alpha], minlength=256)]
    tabs = write_group(bw, hists)
    syms = np.stack([green, red, np.zeros_like(green), np.full_like(green, alpha)], axis=1)
    vals = np.stack([tabs[c][0][syms[:, c]] for c in range(4)], axis=1)
    lens = np.stack([tabs[c][1][syms[:, c]] for c in range(4)], axis=1)
    bw.extend(vals.ravel(), lens.ravel())


def payload_bits(pixels, channels, PB=4, EB=6):
    """(Bits, info) of one frame; info: modes, residual, and the bit counts of the stream's parts."""
    pixels = np.asarray(pixels)
    h, w = pixels.shape[:2]
    assert pixels.shape == (h, w, 4) and 1 <= w <= 16384 and 1 <= h <= 16384 and channels in (3, 4)
    P = green_subtracted(pixels, channels)
    modes, res = choose_modes(P, PB)
    bw = Bits()
    bw.put(0x2f, 8)
    bw.put(w - 1, 14)
    bw.put(h - 1, 14)
    bw.put(1 if channels == 4 else 0, 1)
    bw.put(0, 3)
    bw.put(1, 1); bw.put(2, 2)                    # subtract green
    bw.put(1, 1); bw.put(0, 2); bw.put(PB - 2, 3)        # predictor
    write_subimage(bw, modes, np.zeros_like(modes))
    bw.put(0, 1)                                  # no further transform
    bw.put(0, 1)                                  # no colour cache
    bw.put(1, 1); bw.put(EB - 2, 3)               # meta prefix codes
    t = 1 << EB
    gy, gx = -(-h // t), -(-w // t)
    gi = np.arange(gy * gx)
    write_subimage(bw, gi & 255, gi >> 8)
    sub_end = bw.nbits
    # order of the symbols of a pixel: green, red, blue, alpha; the residual's channels are r, g, b, a
    sym = res[..., (1, 0, 2, 3)]
    vals, lens = np.zeros((h, w, 4), np.uint64), np.zeros((h, w, 4), np.int64)
    for ty in range(gy):
        for tx in range(gx):
            tile = sym[ty * t:(ty + 1) * t, tx * t:(tx + 1) * t]
            hists = [np.bincount(tile[..., c].ravel(), minlength=256) for c in range(4)]
            tabs = write_group(bw, hists)
            for c in range(4):
                vals[ty * t:(ty + 1) * t, tx * t:(tx + 1) * t, c] = tabs[c][0][tile[..., c]]
                lens[ty * t:(ty + 1) * t, tx * t:(tx + 1) * t, c] = tabs[c][1][tile[..., c]]
    head_end = bw.nbits
    bw.extend(vals.ravel(), lens.ravel())
    info = dict(modes=modes, residual=res, sub_bits=sub_end, header_bits=head_end - sub_end, pixel_bits=bw.nbits - head_end,
                bits=bw.nbits)
    return bw, info


def chunk(fourcc, payload):
    return fourcc + struct.pack('<I', len(payload)) + payload + (b'\0' if len(payload) & 1 else b'')


def encode(pixels, channels, PB=4, EB=6):
    """The frame block: a complete `VP8L` chunk."""
    bw, _ = payload_bits(pixels, channels, PB, EB)
    return chunk(b'VP8L', bw.tobytes())


def bound(w, h, channels):
    """fl_webp_bound."""
    if not (1 <= w <= 16384 and 1 <= h <= 16384 and channels in (3, 4)):
        return 0
    code = 76 + 256 * 14
    group = 4 * code + 4
    pt = -(-w // 16) * -(-h // 16)
    g = -(-w // 64) * -(-h // 64)
    bits = 49 + (1 + group + 60 * pt) + 6 + (1 + group + 60 * g) + g * group + 60 * w * h
    n = 16 + 8 + (bits + 7) // 8 + 1
    return 0 if n > 0xffffffff else n


# ---- the strict reader ------------------------------------------------------------------------------------------------
class _Reader(object):
    def __init__(self, data):
        self.d = bytes(data)
        self.bits = np.unpackbits(np.frombuffer(self.d, np.uint8), bitorder='little').tolist()
        self.pos = 0

    def get(self, n):
        p = self.pos
        if p + n > len(self.bits):
            raise WebPError('the payload ends inside a value')
        v = 0
        for i, b in enumerate(self.bits[p:p + n]):
            v |= b << i
        self.pos = p + n
        return v


class _Code(object):
    """A prefix code from its lengths: complete, or one symbol that takes no bits."""

    def __init__(self, lens):
        used = [(n, s) for s, n in enumerate(lens) if n]
        self.single = None
        if not used:
            raise WebPError('a code without symbols')
        if len(used) == 1:
            self.single = used[0][1]
            return
        if sum(1 << (15 - n) for n, _ in used) != 1 << 15:
            raise WebPError('a code that is not complete')
        self.table, code, prev = {}, 0, 0
        for n, s in sorted(used):
            code <<= n - prev
            self.table[(n, code)] = s
            code += 1
            prev = n

    def read(self, r):
        if self.single is not None:
            return self.single
        code = 0
        for n in range(1, 16):
            code = code << 1 | r.get(1)
            if (n, code) in self.table:
                return self.table[(n, code)]
        raise WebPError('no such code')


def _read_code(r, nsym):
    if r.get(1):
        if r.get(1):
            raise WebPError('a simple code of two symbols')
        s = r.get(8 if r.get(1) else 1)
        if s >= nsym:
            raise WebPError('symbol beyond the alphabet')
        lens = [0] * nsym
        lens[s] = 1
        return _Code(lens)
    ncl = r.get(4) + 4
    cl = [0] * 19
    for k in CL_ORDER[:ncl]:
        cl[k] = r.get(3)
    if cl[16]:
        raise WebPError('symbol 16 has a code')
    clcode = _Code(cl)
    if clcode.single is not None:
        raise WebPError('a code-length code of one symbol is not complete')
    if not r.get(1):
        raise WebPError('the token count is not written')
    ntok = 2 + r.get(2 + 2 * r.get(3))
    lens = []
    for _ in range(ntok):
        k = clcode.read(r)
        if k == 16:
            raise WebPError('symbol 16')
        if k == 17:
            lens += [0] * (3 + r.get(3))
        elif k == 18:
            lens += [0] * (11 + r.get(7))
        else:
            lens.append(k)
    if len(lens) > nsym:
        raise WebPError('more code lengths than symbols')
    if not lens or lens[-1] == 0:
        raise WebPError('trailing zero lengths')
    code = _Code(lens + [0] * (nsym - len(lens)))
    if code.single is not None:
        raise WebPError('a normal code of one symbol')
    return code


def _read_group(r):
    return [_read_code(r, n) for n in ALPHABETS]


def _read_pixels(r, w, h, groups, group_of):
    out = np.zeros((h, w, 4), np.int64)                # r, g, b, a
    for y in range(h):
        for x in range(w):
            g = groups[group_of(x, y)]
            green = g[0].read(r)
            if green >= 256:
                raise WebPError('a green symbol of 256 or more (a back reference)')
            out[y, x] = (g[1].read(r), green, g[2].read(r), g[3].read(r))
    return out


def _read_subimage(r, w, h):
    if r.get(1):
        raise WebPError('a colour cache')
    g = _read_group(r)
    return _read_pixels(r, w, h, [g], lambda x, y: 0)


def _predict_pixel(mode, L, T, TL, TR):
    """The reader's own predictor on four-tuples of integers."""
    if mode == 1:
        return L
    if mode == 2:
        return T
    if mode == 7:
        return tuple((a + b) >> 1 for a, b in zip(L, T))
    if mode == 10:
        return tuple((((a + c) >> 1) + ((b + d) >> 1)) >> 1 for a, b, c, d in zip(L, T, TL, TR))
    if mode == 11:
        dl = sum(abs(b - c) for b, c in zip(T, TL))             # |e - L| with e = L + T - TL
        dt = sum(abs(a - c) for a, c in zip(L, TL))
        return L if dl < dt else T
    if mode == 12:
        return tuple(min(max(a + b - c, 0), 255) for a, b, c in zip(L, T, TL))
    raise WebPError('mode %d is not one of the six' % mode)


def decode_payload(data):
    """(pixels u8 [h][w][4], info) of a VP8L payload; info: alpha_is_used, PB, EB, modes, groups."""
    r = _Reader(data)
    if r.get(8) != 0x2f:
        raise WebPError('no VP8L signature')
    w, h = r.get(14) + 1, r.get(14) + 1
    alpha_used = r.get(1)
    if r.get(3):
        raise WebPError('version is not 0')
    if (r.get(1), r.get(2)) != (1, 2):
        raise WebPError('the first transform is not subtract green')
    if (r.get(1), r.get(2)) != (1, 0):
        raise WebPError('the second transform is not the predictor')
    PB = r.get(3) + 2
    tw, th = -(-w >> PB), -(-h >> PB)
    sub = _read_subimage(r, tw, th)
    if (sub[..., 0] != 0).any() or (sub[..., 2] != 0).any() or (sub[..., 3] != 255).any():
        raise WebPError('the mode image holds more than modes')
    modes = sub[..., 1]
    for m in np.unique(modes):
        if int(m) not in MODES:
            raise WebPError('mode %d is not one of the six' % m)
    if r.get(1):
        raise WebPError('a third transform')
    if r.get(1):
        raise WebPError('a colour cache')
    if not r.get(1):
        raise WebPError('no meta prefix codes')
    EB = r.get(3) + 2
    gw, gh = -(-w >> EB), -(-h >> EB)
    ent = _read_subimage(r, gw, gh)
    gi = (ent[..., 0] << 8 | ent[..., 1]).ravel()
    if (gi != np.arange(gw * gh)).any() or (ent[..., 2] != 0).any() or (ent[..., 3] != 255).any():
        raise WebPError('the entropy image does not name group i at pixel i')
    groups = [_read_group(r) for _ in range(gw * gh)]
    res = _read_pixels(r, w, h, groups, lambda x, y: (y >> EB) * gw + (x >> EB))
    while r.pos & 7:
        if r.get(1):
            raise WebPError('a set bit in the padding')
    if r.pos >> 3 != len(r.d):
        raise WebPError('bytes behind the padding')
    # the inverse predictor, then the green comes back (plain integers: a pixel at a time is the format's own order)
    res, rows = res.tolist(), []
    for y in range(h):
        row, up = [], rows[y - 1] if y else None
        for x in range(w):
            if x == 0 and y == 0:
                pred = (0, 0, 0, 255)
            elif y == 0:
                pred = row[x - 1]
            elif x == 0:
                pred = up[0]
            else:
                pred = _predict_pixel(int(modes[y >> PB, x >> PB]), row[x - 1], up[x], up[x - 1], up[x + 1] if x + 1 < w else row[0])
            row.append(tuple((r + p) & 255 for r, p in zip(res[y][x], pred)))
        rows.append(row)
    P = np.array(rows, np.int64).reshape(h, w, 4)
    out = P.copy()
    out[..., 0] = (P[..., 0] + P[..., 1]) & 255
    out[..., 2] = (P[..., 2] + P[..., 1]) & 255
    if not alpha_used and (out[..., 3] != 255).any():
        raise WebPError('alpha_is_used is 0 but an alpha is not 255')
    return out.astype(np.uint8), dict(alpha_is_used=alpha_used, PB=PB, EB=EB, modes=modes, groups=gw * gh, w=w, h=h)


def read_chunk(data, at=0):
    """(fourcc, payload, next offset) of the chunk at `at`; the pad byte of an odd payload must be 0."""
    if at + 8 > len(data):
        raise WebPError('a chunk header runs off the end')
    fourcc = bytes(data[at:at + 4])
    n, = struct.unpack('<I', bytes(data[at + 4:at + 8]))
    end = at + 8 + n + (n & 1)
    if end > len(data):
        raise WebPError('chunk length %d runs off the end' % n)
    if n & 1 and data[end - 1] != 0:
        raise WebPError('the pad byte is not 0')
    return fourcc, bytes(data[at + 8:at + 8 + n]), end


def decode(block):
    """The frame block — one whole `VP8L` chunk and nothing else — to (pixels, info)."""
    fourcc, payload, end = read_chunk(block)
    if fourcc != b'VP8L':
        raise WebPError('not a VP8L chunk')
    if end != len(block):
        raise WebPError('wrong chunk length: bytes behind the chunk')
    return decode_payload(payload)


# ---- the containers ---------------------------------------------------------------------------------------------------
def _u24(v):
    return struct.pack('<I', v)[:3]


def _g24(b):
    return struct.unpack('<I', bytes(b) + b'\0')[0]


def durations(nframes, fps):
    return [int(round(1000.0 * (k + 1) / fps)) - int(round(1000.0 * k / fps)) for k in range(nframes)]


def write_still(block):
    return b'RIFF' + struct.pack('<I', 4 + len(block)) + b'WEBP' + bytes(block)


def write_animation(blocks, w, h, alpha, loop, durs):
    body = chunk(b'VP8X', bytes([0x12 if alpha else 0x02, 0, 0, 0]) + _u24(w - 1) + _u24(h - 1))
    body += chunk(b'ANIM', struct.pack('<IH', 0, loop))
    for blk, d in zip(blocks, durs):
        body += chunk(b'ANMF', _u24(0) + _u24(0) + _u24(w - 1) + _u24(h - 1) + _u24(d) + b'\x02' + bytes(blk))
    return b'RIFF' + struct.pack('<I', 4 + len(body)) + b'WEBP' + body


def read_file(data):
    """dict(animated, w, h, alpha, loop, durations, blocks) of either container, strictly."""
    data = bytes(data)
    if data[:4] != b'RIFF' or data[8:12] != b'WEBP':
        raise WebPError('not a RIFF WEBP file')
    if struct.unpack('<I', data[4:8])[0] != len(data) - 8:
        raise WebPError('wrong RIFF length')
    fourcc, payload, at = read_chunk(data, 12)
    if fourcc == b'VP8L':
        if at != len(data):
            raise WebPError('bytes behind the only frame')
        return dict(animated=False, blocks=[data[12:]], durations=[], loop=None)
    if fourcc != b'VP8X' or len(payload) != 10 or payload[0] not in (0x02, 0x12) or payload[1:4] != b'\0\0\0':
        raise WebPError('bad VP8X chunk')
    out = dict(animated=True, alpha=payload[0] == 0x12, w=_g24(payload[4:7]) + 1, h=_g24(payload[7:10]) + 1, blocks=[], durations=[])
    fourcc, payload, at = read_chunk(data, at)
    if fourcc != b'ANIM' or len(payload) != 6 or payload[:4] != b'\0\0\0\0':
        raise WebPError('bad ANIM chunk')
    out['loop'], = struct.unpack('<H', payload[4:])
    while at < len(data):
        fourcc, payload, at = read_chunk(data, at)
        if fourcc != b'ANMF' or len(payload) < 16 + 8:
            raise WebPError('bad ANMF chunk')
        if _g24(payload[0:3]) or _g24(payload[3:6]) or _g24(payload[6:9]) + 1 != out['w'] or _g24(payload[9:12]) + 1 != out['h']:
            raise WebPError('a frame that does not cover the canvas')
        if payload[15] != 0x02:
            raise WebPError('ANMF flags are not "do not blend, do not dispose"')
        out['durations'].append(_g24(payload[12:15]))
        out['blocks'].append(payload[16:])
    if len(out['blocks']) < 2:
        raise WebPError('an animation of fewer than two frames')
    return out
