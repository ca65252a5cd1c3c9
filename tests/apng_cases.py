"""
What the APNG tests share (tests/test_cpu_apng.py, tests/test_gpu_apng.py, tests/apng_child.py): the frames, a reader of frame
blocks and of whole files that checks every length, CRC-32 and sequence number with zlib's CRC, and a writer of blocks in Python
(zlib.compress cut into chunks) that stands in for the device where there is none.
"""
import struct
import zlib

import numpy as np

IDAT_SEQ = 0xffffffff                 # FL_APNG_IDAT
ADAPTIVE = 1                          # FL_PNG_ADAPTIVE
SIGNATURE = b'\x89PNG\r\n\x1a\n'
SENTINEL = 0xA5
SLACK = 256                           # sentinel bytes kept behind a capacity
SMALL_SEG = 8192                      # FLAME_PNG_SEG of the child process: the smallest the library takes

# (w, h, channels, bits): one chunk that is first and last at once; 18060 filtered bytes, three chunks of 8192 with a short last
# one; 16-bit samples with alpha (18550 bytes, three chunks); a single row
SHAPES = ((5, 3, 3, 8), (100, 60, 3, 8), (33, 70, 4, 16), (257, 1, 3, 8))
PATTERNS = ('random', 'zero_runs')
FLAGS = (0, ADAPTIVE)


def filtered_bytes(w, h, ch, bits):
    return h * (1 + w * ch * bits // 8)


def chunks_of(w, h, ch, bits, seg):
    return -(-filtered_bytes(w, h, ch, bits) // seg)


def seqs_for(n):
    """First numbers whose low bytes carry from chunk to chunk, and the largest a frame of n chunks can start with."""
    return (1, 254, 65534, 0x00fffffe, 0xfffffffe - (n - 1))


def overflowing_seqs(n):
    """Every first number whose last, seq + n - 1, would pass 0xfffffffe (0xffffffff itself asks for IDATs): n - 1 of them, from
    0xffffffff - (n - 1) up."""
    return list(range(0xffffffff - (n - 1), 0xffffffff))


def source(w, h, bits, pattern, seed=0):
    """u8 or u16 [h][w][4] pixels as the device converts them: noise, or zeros with a few samples set (long runs of one byte)."""
    rs = np.random.RandomState(1000 * w + h + bits + seed)
    dt, top = (np.uint8, 256) if bits == 8 else (np.uint16, 65536)
    if pattern == 'random':
        return rs.randint(0, top, (h, w, 4)).astype(dt)
    out = np.zeros((h, w, 4), dt)
    for _ in range(max(2, w * h // 200)):
        out[rs.randint(h), rs.randint(w)] = rs.randint(0, top, 4)
    return out


def case_id(shape, pattern, flags):
    return '%dx%d_ch%d_b%d_%s_%s' % (shape + (pattern, 'adaptive' if flags else 'paeth'))


def read_chunks(data, start=0):
    """[(tag, body)] of the chunks that fill data[start:] exactly; every length and CRC-32 is checked (zlib.crc32)."""
    data = bytes(data)
    out, p = [], start
    while p < len(data):
        assert p + 12 <= len(data), 'a chunk is cut short at %d' % p
        n, = struct.unpack('>I', data[p:p + 4])
        assert p + 12 + n <= len(data), 'the chunk at %d passes the end' % p
        tag, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        crc, = struct.unpack('>I', data[p + 8 + n:p + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, 'CRC-32 of chunk %r at %d' % (tag, p)
        out.append((tag, body))
        p += 12 + n
    return out


def chunk(tag, body):
    return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xffffffff)


def retag(block, seq):
    """The IDAT block of an fdAT block that starts at `seq`: every tag, length, number and CRC checked, the numbers stripped."""
    out = b''
    for i, (tag, body) in enumerate(read_chunks(block)):
        assert tag == b'fdAT' and len(body) >= 4 and struct.unpack('>I', body[:4])[0] == seq + i, (i, tag, body[:4])
        out += chunk(b'IDAT', body[4:])
    return out


def block_from_stream(z, n, seq):
    """A frame block of n chunks that hold the zlib stream z in pieces of about equal length."""
    assert len(z) >= n
    cuts = [len(z) * i // n for i in range(n + 1)]
    parts = [z[cuts[i]:cuts[i + 1]] for i in range(n)]
    if seq == IDAT_SEQ:
        return b''.join(chunk(b'IDAT', p) for p in parts)
    return b''.join(chunk(b'fdAT', struct.pack('>I', seq + i) + p) for i, p in enumerate(parts))


def host_frame(block, seg, n, status=0, slack=0):
    """The host frame of a block: the 16-byte record and the block behind it, as the device leaves them."""
    rec = np.array([len(block), status, seg, n], '<u4').view(np.uint8)
    return np.concatenate([rec, np.frombuffer(block, np.uint8), np.zeros(slack, np.uint8)])


class Apng(object):
    """A parsed APNG file: w, h, bits, channels, num_frames, num_plays, tags, and per frame `fctl` (the thirteen fields of the
    fcTL as a tuple behind its sequence number) and `stream` (the frame's zlib stream, reassembled from its chunks); `numbers`
    are the sequence numbers in file order."""


def parse_file(data):
    data = bytes(data)
    assert data[:8] == SIGNATURE
    ck = read_chunks(data, 8)
    ap = Apng()
    ap.tags = [t for t, _ in ck]
    assert ap.tags[0] == b'IHDR' and ap.tags[1] == b'acTL' and ap.tags[-1] == b'IEND' and ap.tags.count(b'IEND') == 1
    ap.w, ap.h, ap.bits, ctype, comp, filt, lace = struct.unpack('>IIBBBBB', ck[0][1])
    assert ctype in (2, 6) and (comp, filt, lace) == (0, 0, 0)
    ap.channels = 3 if ctype == 2 else 4
    ap.num_frames, ap.num_plays = struct.unpack('>II', ck[1][1])
    ap.numbers, ap.fctl, ap.stream, ap.frame_bytes = [], [], [], []
    for tag, body in ck[2:-1]:
        if tag == b'fcTL':
            assert len(body) == 26
            f = struct.unpack('>IIIIIHHBB', body)
            ap.numbers.append(f[0]); ap.fctl.append(f); ap.stream.append(b''); ap.frame_bytes.append(38)
        elif tag == b'IDAT':
            assert len(ap.fctl) == 1, 'IDAT outside frame 0'
            ap.stream[-1] += body; ap.frame_bytes[-1] += 12 + len(body)
        else:
            assert tag == b'fdAT' and len(ap.fctl) >= 2, (tag, len(ap.fctl))
            ap.numbers.append(struct.unpack('>I', body[:4])[0])
            ap.stream[-1] += body[4:]; ap.frame_bytes[-1] += 12 + len(body)
    return ap


def frame_as_png(ap, k):
    """Frame k as a PNG file of its own: the reassembled stream in one IDAT."""
    ihdr = struct.pack('>IIBBBBB', ap.w, ap.h, ap.bits, 2 if ap.channels == 3 else 6, 0, 0, 0)
    return SIGNATURE + chunk(b'IHDR', ihdr) + chunk(b'IDAT', ap.stream[k]) + chunk(b'IEND', b'')
