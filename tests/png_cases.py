"""
The frames tests/test_cpu_png.py and tests/test_gpu_png.py encode: the smallest shapes at which each part of the PNG encoder can
go wrong.  A case is (name, build(seg) -> (rgba u8 [h][w][4], channels), check(stats, seg)): `check` asserts, from the statistics
png_model.parse gathered, that the file contains what the case is named for, so that a case that stops reaching its edge fails.
`seg` is the encoder's segment length in filtered bytes; sizes that depend on it are built from it.

Several frames are built from the residuals they should filter to.  In a frame one pixel high Paeth predicts the pixel to the
left (the row above is zero), so a wanted residual stream is integrated per channel; those cases assert the filter byte 4.
"""
import numpy as np

import png_model as P

MODEL_SEG = 32768             # the length the CPU tests use; the GPU tests take the device's from its record


def bound(w, h, ch, seg):
    """fl_png_bound: record, header, zlib header, every segment stored in an IDAT of its own, Adler-32, IEND."""
    F = h * (1 + w * ch)
    return 16 + P.HEADER_BYTES + 2 + F + 17 * -(-F // seg) + 4 + 12


def _rgba(pix, ch):
    """u8 [h][w][4] from [h][w][ch]; an alpha the file leaves out is set to a value that would show if it were coded."""
    h, w, _ = pix.shape
    out = np.full((h, w, 4), 0x5a, np.uint8)
    out[:, :, :ch] = pix
    return out


def _row_from_residuals(res, ch):
    """A frame one pixel high whose Paeth-filtered stream is [4] + res (len(res) a multiple of ch)."""
    res = np.asarray(res, np.uint64).reshape(-1, ch)
    return _rgba((np.cumsum(res, axis=0) & 255).astype(np.uint8)[None], ch), ch


def _shape_for(total):
    """(w, h, channels) of a frame whose filtered stream has exactly `total` bytes."""
    for ch in (3, 4):
        if (total - 1) % ch == 0 and 1 <= (total - 1) // ch <= 65535:
            return (total - 1) // ch, 1, ch
    for row in range(total, 1, -1):
        if total % row == 0 and total // row <= 65535:
            for ch in (3, 4):
                if (row - 1) % ch == 0 and 1 <= (row - 1) // ch <= 65535:
                    return (row - 1) // ch, total // row, ch
    raise ValueError('no frame filters to %d bytes' % total)


def _soft(w, h, ch, seed):
    """A ramp with a little noise: compressible, and no two rows alike."""
    rs = np.random.RandomState(seed)
    x, y = np.arange(w)[None, :, None], np.arange(h)[:, None, None]
    return ((x * 3 + y * 5 + np.arange(ch)[None, None, :] * 40 + rs.randint(0, 3, (h, w, ch))) & 255).astype(np.uint8)


def _tiny(ch):
    def build(seg):
        return _rgba(np.array([[[201, 17, 96, 33][:ch]]], np.uint8), ch), ch

    def check(st, seg):
        assert st['nfiltered'] == 1 + ch and len(st['segments']) == 1 and st['finals'][-1] == 1
        assert st['segments'][0]['stored']                    # five bytes cannot pay for a dynamic header
    return build, check


def _build_7x3(seg):
    return _rgba(np.random.RandomState(3).randint(0, 256, (3, 7, 3)).astype(np.uint8), 3), 3


def _check_7x3(st, seg):
    assert st['nfiltered'] == 3 * 22 and len(st['segments']) == 1


def _around_seg(delta):
    def build(seg):
        w, h, ch = _shape_for(seg + delta)
        return _rgba(_soft(w, h, ch, 20 + delta), ch), ch

    def check(st, seg):
        assert st['nfiltered'] == seg + delta
        sizes = [s['nbytes'] for s in st['segments']]
        assert sizes == ([seg, 1] if delta == 1 else [seg + delta]), sizes
        assert st['segments'][0]['dynamic']
    return build, check


def _build_noise(seg):
    w, h, ch = _shape_for(3 * seg + 100)
    return _rgba(np.random.RandomState(9).randint(0, 256, (h, w, ch)).astype(np.uint8), ch), ch


def _check_noise(st, seg):
    assert st['nfiltered'] == 3 * seg + 100 and [s['nbytes'] for s in st['segments']] == [seg, seg, seg, 100]
    assert all(s['stored'] for s in st['segments']) and st['matches'] == []
    assert st['adler_b_unreduced'] >= 1 << 32                 # the sums leave 32 bits unless they are reduced on the way
    assert st['file_bytes'] + 16 <= st['bound']


def _zeros_shape(seg):
    w = 400
    return w, (5 * seg // 2) // (1 + 3 * w)


def _build_zeros(seg):
    w, h = _zeros_shape(seg)
    return _rgba(np.zeros((h, w, 3), np.uint8), 3), 3


def _check_zeros(st, seg):
    w, h = _zeros_shape(seg)
    row = 1 + 3 * w
    assert len(st['segments']) == 3 and all(s['dynamic'] for s in st['segments'])
    assert st['distances'] == [1] and 258 in st['match_lengths']
    for b in st['blocks']:
        if b['type'] == 2:
            assert b['dist_codes_used'] == 1 and b['dist_lengths'] == [1]      # only distance code 0
    ends = set(at + length for length, _, at in st['matches'])
    for cut in (seg, 2 * seg):
        assert cut % row > 4                                  # the cut falls inside a row's run of zeros ...
        assert cut in ends                                    # ... which a match ends at, and none crosses (the parser refuses one that reaches back)
    assert st['literals'] < 3 * h + 6                         # the filter byte, the first zero, a leftover; the first zero behind each cut


def _runs_stream(seg):
    """Residuals (the filter byte in front counted): a non-zero byte, then L zeros, for L = 3 .. 300; filler in front of a run that a
    segment boundary would cut, so that every run is coded whole."""
    out = [4]
    for L in range(3, 301):
        if len(out) // seg != (len(out) + L + 1) // seg:
            out += [1 + (k & 1) for k in range(seg - len(out) % seg)]
        out += [7 + (L & 1)] + [0] * L
    while (len(out) - 1) % 3:
        out.append(1 + (len(out) & 1))
    return out


def _build_runs(seg):
    return _row_from_residuals(_runs_stream(seg)[1:], 3)


def _check_runs(st, seg):
    assert st['filters'] == [4]
    assert st['match_lengths'] == list(range(3, 259))         # L zeros: a literal and L - 1 repeats; 259 and 260 repeats leave one and two literals
    assert st['distances'] == [1]
    assert len(st['matches']) == 297 + 39             # one match per run of 4 and more, a second one from 262 zeros on
    assert all(s['dynamic'] for s in st['segments'])


def _build_ramp(seg):
    return _row_from_residuals([1 + k % 3 for k in range(2999)][:2997], 3)


def _check_ramp(st, seg):
    assert st['filters'] == [4] and st['block_types'] == [2] and st['matches'] == []
    b = st['blocks'][0]
    assert b['dist_codes_used'] == 0 and b['dist_lengths'] == [0]      # a single distance code of length zero


def _fib_counts(seg):
    """How often each residual value occurs.  The row's filter byte (once) and the end-of-block symbol (once) are F1 and F2, the
    residual values F3 .. F21: 28 656 symbols, whose unrestricted Huffman code is a single chain 20 deep."""
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    k = 21
    while 1 + sum(fib[2:k]) + 2 > seg:
        k -= 1
    assert k >= 18                                            # (F1 .. F18: 17 deep unrestricted)
    counts = fib[2:k]
    counts[-1] += -sum(counts) % 3                            # whole pixels: up to two more of the commonest value, which stays at one bit
    return counts


def _build_fib(seg):
    counts = _fib_counts(seg)
    syms = [10 + i for i, c in sorted(enumerate(counts), key=lambda ic: -ic[1]) for _ in range(c)]
    n = len(syms)
    res = [0] * n
    res[0::2] = syms[:(n + 1) // 2]                           # the commonest value fills every other place: no two neighbours are equal
    res[1::2] = syms[(n + 1) // 2:]
    assert all(a != b for a, b in zip(res, res[1:]))
    return _row_from_residuals(res, 3)


def _check_fib(st, seg):
    counts = _fib_counts(seg)
    assert st['filters'] == [4] and st['block_types'] == [2] and st['matches'] == []
    assert st['literals'] == 1 + sum(counts) and (len(counts) < 19 or st['literals'] == 28655 + 2)
    b = st['blocks'][0]
    assert b['max_lit_len'] == 15 and b['lit_complete']
    lens = b['lit_lengths']
    assert lens[4] == lens[256] == lens[10] == 15 and lens[10 + len(counts) - 1] == 1      # the rarest cut to 15 bits, the commonest at one


def _build_smooth(seg):
    w, h = 256, 96
    x, y = np.arange(w)[None, :, None], np.arange(h)[:, None, None]
    c = np.arange(3)[None, None, :]
    v = 128 + 100 * np.sin(x / (20.0 + 3 * c)) * np.cos(y / (15.0 + 2 * c))
    pix = np.rint(v).astype(np.uint8)
    pix[:12], pix[-12:], pix[:, :16], pix[:, -16:] = 0, 0, 0, 0
    return _rgba(pix, 3), 3


def _check_smooth(st, seg):
    assert st['nfiltered'] == 96 * 769 and all(s['dynamic'] for s in st['segments'])
    assert 2 * st['file_bytes'] < st['raw_bytes']
    assert st['distances'] == [1]


CASES = [('1x1_rgb',) + _tiny(3), ('1x1_rgba',) + _tiny(4), ('7x3_rgb', _build_7x3, _check_7x3),
         ('exactly_seg',) + _around_seg(0), ('seg_minus_1',) + _around_seg(-1), ('seg_plus_1',) + _around_seg(1),
         ('noise_3seg_100', _build_noise, _check_noise), ('zeros_3seg', _build_zeros, _check_zeros),
         ('runs_3_to_300', _build_runs, _check_runs), ('ramp_no_match', _build_ramp, _check_ramp),
         ('fibonacci_15', _build_fib, _check_fib), ('smooth_256x96', _build_smooth, _check_smooth)]
NAMES = [c[0] for c in CASES]
NOISE = 'noise_3seg_100'


def case(name, seg):
    """(rgba, channels, check) of a case."""
    _, build, check = CASES[NAMES.index(name)]
    rgba, ch = build(seg)
    return rgba, ch, check


def stats_of(ps, seg):
    """png_model.parse's statistics with what the checks need beside them."""
    st = dict(ps.stats)
    d = np.frombuffer(ps.filtered, np.uint8).astype(object)
    n = len(d)
    st['adler_b_unreduced'] = int(n + sum((n - i) * int(v) for i, v in enumerate(d))) if n <= 4 * seg + 1000 else 0
    st['bound'] = bound(ps.w, ps.h, ps.channels, seg)
    return st
