"""
CPU tests of the device WebP encoder's format (no GPU).  The model of tests/webp_model.py is held to Pillow's libwebp, which decodes
every file it writes to the source pixels, and to its own strict reader, which refuses what the encoder never writes; the predictor's
rules and ties and the code-length tokens are pinned on hand-made inputs; the files around the blocks (WebPOutput) are driven with
model-made blocks; the output selection, the command line and the C ABI's refusals that need no device are driven.
"""
import argparse
import io
import os
import re
import struct

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, encoders, output, profile, render
from png_model import limited_lengths
import webp_cases as WC
import webp_model as M

from PIL import Image as PIL_Image, features

needs_webp = pytest.mark.skipif(not features.check('webp'), reason='this Pillow has no WebP decoder')


def frames_of(data):
    im = PIL_Image.open(io.BytesIO(data))
    out = []
    for k in range(getattr(im, 'n_frames', 1)):
        im.seek(k)
        out.append((np.asarray(im.convert('RGBA')).copy(), dict(im.info)))
    return im.size, out


# ------------------------------------------------------------------ the model against Pillow and against its own reader
@needs_webp
@pytest.mark.parametrize('name', WC.NAMES)
def test_pillow_returns_the_source_pixels(name):
    frame, channels = WC.cases()[name]
    h, w = frame.shape[:2]
    block = WC.model_block(name)
    assert block[:4] == b'VP8L' and len(block) % 2 == 0 and 16 + len(block) <= M.bound(w, h, channels)
    size, frames = frames_of(M.write_still(block))
    assert size == (w, h) and len(frames) == 1
    assert np.array_equal(frames[0][0], WC.expected(name))
    assert M.encode(frame, channels) == block                   # the same pixels give the same bytes


@pytest.mark.parametrize('name', WC.NAMES)
def test_the_strict_reader_returns_the_source_pixels(name):
    frame, channels = WC.cases()[name]
    pixels, info = M.decode(WC.model_block(name))
    assert np.array_equal(pixels, WC.expected(name))
    assert (info['PB'], info['EB'], info['alpha_is_used']) == (4, 6, int(channels == 4))
    assert info['groups'] == -(-frame.shape[1] // 64) * -(-frame.shape[0] // 64)


@needs_webp
def test_other_tile_sizes_decode():
    frame, channels = WC.cases()['plasma_130x70']
    for PB, EB in ((2, 2), (3, 5), (5, 4), (9, 9)):
        block = M.encode(frame, channels, PB, EB)
        assert np.array_equal(frames_of(M.write_still(block))[1][0][0], frame)
    pixels, info = M.decode(M.encode(frame[:20, :30], 4, 3, 3))
    assert np.array_equal(pixels, frame[:20, :30]) and (info['PB'], info['EB'], info['groups']) == (3, 3, 12)


def test_cases_are_what_the_device_test_needs():
    cases = WC.cases()
    assert set(WC.NAMES) == set(cases)
    info = dict((n, M.payload_bits(*cases[n])[1]) for n in WC.NAMES if n != 'wide_1088x1024')
    assert set(info['six_modes']['modes'].ravel().tolist()) == set(M.MODES)         # every mode wins somewhere
    assert info['flat_130x70']['pixel_bits'] == 0                                   # every code one symbol
    assert info['flat_130x70']['header_bits'] == 6 * 5 * 4                          # six groups of five simple codes of symbol 0
    assert info['cost_ties']['modes'][:, 0].tolist() == [1, 1] and info['cost_ties']['modes'][0, 1] == 2      # all six tie; 1, 11, 12 tie; 2, 11, 12 tie
    res = M.mode_residuals(M.green_subtracted(*cases['cost_ties']))
    cost = lambda m, sl: int(np.minimum(res[m], 256 - res[m])[sl].sum())
    flat, rows, cols = (slice(0, 16), slice(0, 16)), (slice(16, 32), slice(0, 16)), (slice(0, 16), slice(16, 32))
    assert len(set(cost(m, flat) for m in M.MODES)) == 1
    assert cost(1, rows) == cost(11, rows) == cost(12, rows) < min(cost(m, rows) for m in (2, 7, 10))
    assert cost(2, cols) == cost(11, cols) == cost(12, cols) < min(cost(m, cols) for m in (1, 7, 10))
    # the noise meets the bound with room, and stays above 7 bits a symbol
    assert 16 + len(WC.model_block('noise_128x128')) <= M.bound(128, 128, 4) and info['noise_128x128']['pixel_bits'] > 7 * 4 * 128 * 128
    # the ladder: green's tree is 16 deep and the limit of 15 cuts it; alpha's token kinds make a code that limit 7 cuts
    lad = info['ladder']
    assert (lad['modes'] == 1).all()
    green = np.bincount(lad['residual'][..., 1].ravel(), minlength=256).tolist()
    assert max(limited_lengths(green, 40)) == 16 and sorted(n for n in limited_lengths(green, 15) if n) == list(range(1, 14)) + [15] * 4
    alpha = np.bincount(lad['residual'][..., 3].ravel(), minlength=256).tolist()
    lens = limited_lengths(alpha, 15)
    assert dict((n, lens.count(n)) for n in set(lens) if n) == WC.LADDER_LENGTHS
    tf = [0] * 19
    for kind, _, _ in M.code_length_tokens(lens[:129]):
        tf[kind] += 1
    assert max(limited_lengths(tf, 15)) == 8 and max(limited_lengths(tf, 7)) == 7
    # 272 groups: the entropy sub-image needs red
    assert -(-1088 // 64) * (1024 // 64) == 272
    # the same source with and without alpha
    assert np.array_equal(cases['alpha_rgba'][0], cases['alpha_rgb'][0]) and WC.model_block('alpha_rgba') != WC.model_block('alpha_rgb')
    assert len(set(cases['alpha_rgba'][0][..., 3].ravel().tolist())) > 8


# ------------------------------------------------------------------ what the strict reader refuses
def test_the_strict_reader_refuses(monkeypatch):
    frame, channels = WC.cases()['plasma_17x17']
    good = WC.model_block('plasma_17x17')
    assert np.array_equal(M.decode(good)[0], frame)
    payload = good[8:8 + struct.unpack('<I', good[4:8])[0]]

    def flip(bit, data=payload):
        d = bytearray(data)
        d[bit >> 3] ^= 1 << (bit & 7)
        return bytes(d)

    with pytest.raises(M.WebPError, match='subtract green'):            # a transform other than the two named: type 3 in front
        M.decode_payload(flip(41))
    with pytest.raises(M.WebPError, match='predictor'):                 # ... and type 1 (cross-colour) in second place
        M.decode_payload(flip(44))
    with pytest.raises(M.WebPError, match='cache'):                     # the mode sub-image's cache bit
        M.decode_payload(flip(49))
    with pytest.raises(M.WebPError, match='signature'):
        M.decode_payload(b'\x2e' + payload[1:])
    with pytest.raises(M.WebPError, match='version'):
        M.decode_payload(flip(37))
    # a wrong chunk length, and bytes behind the chunk
    with pytest.raises(M.WebPError, match='chunk length'):
        M.decode(good[:4] + struct.pack('<I', len(payload) + 2) + good[8:])
    with pytest.raises(M.WebPError, match='chunk length'):
        M.decode(good + b'\0\0')
    with pytest.raises(M.WebPError):
        M.decode(good[:4] + struct.pack('<I', len(payload) - 2) + good[8:])
    with pytest.raises(M.WebPError, match='VP8L'):
        M.decode(b'VP8 ' + good[4:])
    # bits behind the padding: a set padding bit, and a whole byte more
    info = M.payload_bits(frame, channels)[1]
    assert info['bits'] % 8, 'the case needs padding bits'
    with pytest.raises(M.WebPError, match='padding'):
        M.decode_payload(flip(info['bits']))
    with pytest.raises(M.WebPError, match='behind the padding'):
        M.decode_payload(payload + b'\0')
    with pytest.raises(M.WebPError, match='ends inside'):
        M.decode_payload(payload[:-3])


def _rewritten(monkeypatch, frame, channels, **bend):
    """The block of `frame` from the model with one of its functions replaced."""
    for name, fn in bend.items():
        monkeypatch.setattr(M, name, fn)
    return M.encode(frame, channels)


@needs_webp
def test_the_strict_reader_refuses_a_seventh_mode(monkeypatch):
    frame, channels = WC.cases()['plasma_16x16']
    real = M.choose_modes

    def choose(P, PB=4):                                                # mode 0 (black) everywhere: a valid stream that libwebp decodes
        modes, res = real(P, PB)
        pred = M.fixed_rules(np.broadcast_to(np.array((0, 0, 0, 255)), P.shape), P)
        return np.zeros_like(modes), (P - pred) & 255
    block = _rewritten(monkeypatch, frame, channels, choose_modes=choose)
    assert np.array_equal(frames_of(M.write_still(block))[1][0][0], frame)
    with pytest.raises(M.WebPError, match='mode 0 is not one of the six'):
        M.decode(block)


@needs_webp
def test_the_strict_reader_refuses_symbol_16(monkeypatch):
    frame, channels = WC.cases()['plasma_16x16']
    real = M.code_length_tokens

    def tokens(lens):                                                   # VP8L's 16: repeat the previous non-zero length 3..6 times
        out, i = [], 0
        while i < len(lens):
            run = 1
            while i + run < len(lens) and lens[i + run] == lens[i]:
                run += 1
            if lens[i] and run >= 4:
                m = min(run - 1, 6)
                out += [(lens[i], 0, 0), (16, m - 3, 2)]
                i += 1 + m
            else:
                out += real(lens[i:i + run])
                i += run
        return out
    block = _rewritten(monkeypatch, frame, channels, code_length_tokens=tokens)
    assert block != WC.model_block('plasma_16x16')
    assert np.array_equal(frames_of(M.write_still(block))[1][0][0], frame)       # libwebp takes it
    with pytest.raises(M.WebPError, match='16'):
        M.decode(block)


def test_the_strict_reader_refuses_a_back_reference_and_a_cache():
    """Hand-written streams of one 4 x 1 picture: green 256 (a length prefix) as the second symbol; and the main image's cache bit."""
    def stream(cache, green_syms):
        bw = M.Bits()
        bw.put(0x2f, 8); bw.put(3, 14); bw.put(0, 14); bw.put(0, 1); bw.put(0, 3)
        bw.put(1, 1); bw.put(2, 2)
        bw.put(1, 1); bw.put(0, 2); bw.put(2, 3)
        M.write_subimage(bw, np.array([1]), np.array([0]))
        bw.put(0, 1)
        bw.put(cache, 1)
        if cache:
            bw.put(1, 4)
        bw.put(1, 1); bw.put(4, 3)
        M.write_subimage(bw, np.array([0]), np.array([0]))
        freq = [0] * 280
        for s in green_syms:
            freq[s] += 1
        codes = M.write_code(bw, freq)
        M.write_code(bw, [1] + [0] * 255)
        M.write_code(bw, [1] + [0] * 255)
        M.write_code(bw, [1] + [0] * 255)
        M.write_code(bw, [0] * 40)
        for s in green_syms:
            bw.put(*codes[s])
        return bw.tobytes()
    pixels, _ = M.decode_payload(stream(0, [5, 0, 0, 1]))
    assert pixels[0, :, 1].tolist() == [5, 5, 5, 6]
    with pytest.raises(M.WebPError, match='256 or more'):
        M.decode_payload(stream(0, [5, 256, 0, 1]))
    with pytest.raises(M.WebPError, match='cache'):
        M.decode_payload(stream(1, [5, 0, 0, 1]))


# ------------------------------------------------------------------ the predictor's rules and ties
def _px(g, a=255):
    return np.array((0, g, 0, a))


def test_predictor_rules():
    L, T, TL, TR = (np.array(v) for v in ((10, 200, 30, 255), (13, 100, 31, 0), (40, 50, 90, 128), (1, 2, 3, 4)))
    assert M.predict(1, L, T, TL, TR).tolist() == L.tolist() and M.predict(2, L, T, TL, TR).tolist() == T.tolist()
    assert M.predict(7, L, T, TL, TR).tolist() == [11, 150, 30, 127]                                    # floors
    assert M.predict(10, L, T, TL, TR).tolist() == [(25 + 7) // 2, (125 + 51) // 2, (60 + 17) // 2, (191 + 2) // 2]
    assert M.predict(12, L, T, TL, TR).tolist() == [0, 250, 0, 127]                                     # clamped per channel
    assert M.predict(12, np.array((250,) * 4), np.array((250,) * 4), np.array((10,) * 4), TR).tolist() == [255] * 4
    # select: e = L + T - TL; dL = sum |e - L| = sum |T - TL|; L if dL < dT, else T — so T on dL == dT
    L, T, TL = np.array((10, 10, 10, 10)), np.array((30, 30, 30, 30)), np.array((20, 20, 20, 20))
    assert M.predict(11, L, T, TL, TR).tolist() == T.tolist()                                           # dL == dT == 40
    assert M.predict(11, L, T, TL + np.array((1, 0, 0, 0)), TR).tolist() == L.tolist()                  # dL 39 < dT 41
    assert M.predict(11, L, T, TL - np.array((1, 0, 0, 0)), TR).tolist() == T.tolist()
    with pytest.raises(M.WebPError):
        M.predict(13, L, T, TL, TR)


@needs_webp
def test_fixed_rules_and_the_last_column_s_top_right():
    rs = np.random.RandomState(3)
    frame = rs.randint(0, 256, (5, 6, 4)).astype(np.uint8)
    P = M.green_subtracted(frame, 4)
    L, T, TL, TR = M.neighbours(P)
    assert np.array_equal(TR[2, 5], P[2, 0]) and np.array_equal(TR[2, 4], P[1, 5]) and np.array_equal(TL[3, 2], P[2, 1])
    res = M.mode_residuals(P)
    for m in M.MODES:                                           # whatever the mode: (0, 0) from 0, 0, 0, 255; row 0 from L; column 0 from T
        assert np.array_equal(res[m][0, 0], (P[0, 0] - (0, 0, 0, 255)) & 255)
        assert np.array_equal(res[m][0, 1:], (P[0, 1:] - P[0, :-1]) & 255)
        assert np.array_equal(res[m][1:, 0], (P[1:, 0] - P[:-1, 0]) & 255)
    want = (P[2, 5] - ((((P[2, 4] + P[1, 4]) >> 1) + ((P[1, 5] + P[2, 0]) >> 1)) >> 1)) & 255
    assert np.array_equal(res[10][2, 5], want)
    # green is subtracted before the predictor sees anything, and three channels read alpha as 255
    assert np.array_equal(P[..., 0], (frame[..., 0].astype(int) - frame[..., 1]) & 255) and (M.green_subtracted(frame, 3)[..., 3] == 255).all()
    # a 6 x 5 picture that only mode 10 with that top right predicts exactly is decoded by Pillow
    assert np.array_equal(frames_of(M.write_still(M.encode(frame, 4)))[1][0][0], frame)


def test_a_mode_tie_goes_to_the_lowest():
    flat = np.full((16, 16, 4), 200, np.uint8)
    modes, res = M.choose_modes(M.green_subtracted(flat, 4))
    assert modes.tolist() == [[1]]
    frame = WC.cases()['cost_ties'][0]
    assert M.choose_modes(M.green_subtracted(frame, 3))[0].tolist()[0] == [1, 2]
    # pixels outside the image do not count: a 17 x 17 frame's edge tiles are one pixel wide
    modes, _ = M.choose_modes(M.green_subtracted(WC.cases()['plasma_17x17'][0], 4))
    assert modes.shape == (2, 2)


# ------------------------------------------------------------------ the code-length tokens
@pytest.mark.parametrize('run,want', ((2, [(0, 0, 0)] * 2), (3, [(17, 0, 3)]), (10, [(17, 7, 3)]), (11, [(18, 0, 7)]), (138, [(18, 127, 7)]),
                                      (139, [(18, 127, 7), (0, 0, 0)]), (149, [(18, 127, 7), (18, 0, 7)]), (141, [(18, 127, 7), (17, 0, 3)]),
                                      (1, [(0, 0, 0)]), (150, [(18, 127, 7), (18, 1, 7)])))
@needs_webp
def test_zero_runs(run, want):
    lens = [3] + [0] * run + [5]
    assert M.code_length_tokens(lens) == [(3, 0, 0)] + want + [(5, 0, 0)]
    # ... and a code with such a run goes through Pillow and the reader
    freq = [0] * 256
    freq[0], freq[run + 1], freq[255] = 5, 3, 2
    rs = np.random.RandomState(run)
    g = rs.permutation(np.repeat(np.arange(256), freq))
    frame = np.zeros((1, 10, 4), np.uint8)
    frame[0, :, 1] = np.cumsum(g)
    frame[0, :, 0] = frame[0, :, 2] = frame[0, :, 1]
    frame[..., 3] = 255
    block = M.encode(frame, 3)
    assert np.array_equal(M.decode(block)[0], frame) and np.array_equal(frames_of(M.write_still(block))[1][0][0], frame)


def test_no_sixteen_and_no_trailing_zeros():
    lens = [4] * 40 + [0] * 5 + [7] * 9
    toks = M.code_length_tokens(lens)
    assert all(k != 16 for k, _, _ in toks) and len(toks) == 40 + 1 + 9
    bw = M.Bits()
    codes = M.write_code(bw, [1, 1] + [0] * 254)                # two used symbols: lengths 1, 1 and nothing behind them
    assert codes == {0: (0, 1), 1: (1, 1)}
    # normal form, 4 code-length lengths at least, token count 2 in k = 1: 1 + 4 + 3 * 4 + 1 + 3 + 2 + 2 tokens of one bit
    assert bw.nbits == 1 + 4 + 12 + 1 + 3 + 2 + 2


@needs_webp
def test_a_lone_token_kind():
    """256 symbols used equally: every length is 8, the only token kind is 8; it gets one bit and so does kind 0."""
    frame = np.zeros((16, 16, 4), np.uint8)
    frame[..., 1] = np.cumsum(np.random.RandomState(2).permutation(256)).reshape(16, 16)
    frame[..., 0] = frame[..., 2] = frame[..., 1]
    frame[..., 3] = 255
    block = M.encode(frame, 3)
    assert np.array_equal(M.decode(block)[0], frame) and np.array_equal(frames_of(M.write_still(block))[1][0][0], frame)
    bw = M.Bits()
    codes = M.write_code(bw, [16] * 256)
    assert set(n for _, n in codes.values()) == {8}
    # 1 + 4 + 3 * 12 (the order reaches kind 8 at its twelfth place) + 1 + 3 + 8 (254 tokens more than 2: k = 4) + 256 tokens of one bit
    assert M.CL_ORDER.index(8) == 11 and bw.nbits == 1 + 4 + 36 + 1 + 3 + 8 + 256
    assert limited_lengths([0] * 8 + [256] + [0] * 10, 7) == [1] + [0] * 7 + [1] + [0] * 10
    assert limited_lengths([256] + [0] * 18, 7)[:2] == [1, 1]                    # the lone kind 0 takes kind 1 along


def test_simple_codes():
    for s, bits in ((0, [1, 0, 0, 0]), (1, [1, 0, 0, 1]), (2, [1, 0, 1] + [0, 1, 0, 0, 0, 0, 0, 0]), (255, [1, 0, 1] + [1] * 8)):
        bw = M.Bits()
        freq = [0] * 256
        freq[s] = 9
        assert M.write_code(bw, freq) == {}
        assert list(np.unpackbits(np.frombuffer(bw.tobytes(), np.uint8), bitorder='little')[:bw.nbits]) == bits
    bw = M.Bits()
    assert M.write_code(bw, [0] * 40) == {} and bw.nbits == 4


# ------------------------------------------------------------------ the files around the blocks
class _Record(object):
    """A host frame as the device leaves it: the record, then the block."""

    @staticmethod
    def of(block, status=0):
        return np.frombuffer(np.array([len(block), status, 4 | 6 << 8, 0], '<u4').tobytes() + block + b'\xa5' * 40, np.uint8)


def some_frames(n, w=16, h=8):
    return [WC.noise(w, h, 50 + k) for k in range(n)]


def some_blocks(n, w=16, h=8, channels=4):
    return [M.encode(f, channels) for f in some_frames(n, w, h)]


@needs_webp
@pytest.mark.parametrize('fps,alpha', ((24, True), (30, False), (90, True), (7.5, False)))
def test_mux_counts_loops_and_durations(fps, alpha):
    frames = some_frames(7)
    blocks = [M.encode(f, 4 if alpha else 3) for f in frames]
    out = encoders.WebPOutput(fps=fps, loop=5, alpha=alpha)
    for b in blocks:
        assert out.encode(_Record.of(b)) == ({}, [])
    media, logs = out.encode(None)
    assert list(media) == ['.webp'] and logs == []
    data = media['.webp'].read()
    want = [int(round(1000.0 * (k + 1) / fps)) - int(round(1000.0 * k / fps)) for k in range(7)]
    assert want == encoders.webp_durations(7, fps) == M.durations(7, fps) and min(want) >= 11
    assert abs(sum(want) - 7000.0 / fps) <= 0.5
    assert data == M.write_animation(blocks, 16, 8, alpha, 5, want)
    assert data[:4] == b'RIFF' and struct.unpack('<I', data[4:8])[0] == len(data) - 8 and data[8:16] == b'WEBPVP8X'
    assert data[20] == (0x12 if alpha else 0x02) and data[30:34] == b'ANIM' and data[42:44] == struct.pack('<H', 5)
    parsed = M.read_file(data)
    assert parsed['animated'] and parsed['blocks'] == blocks and parsed['durations'] == want and parsed['loop'] == 5
    assert (parsed['w'], parsed['h'], parsed['alpha']) == (16, 8, alpha)
    im = PIL_Image.open(io.BytesIO(data))
    assert im.size == (16, 8) and im.n_frames == 7 and im.info['loop'] == 5
    for k, f in enumerate(frames):
        im.seek(k)
        im.load()
        assert im.info['duration'] == want[k]
        got = np.asarray(im.convert('RGBA'))
        assert np.array_equal(got[..., :3], f[..., :3]) and np.array_equal(got[..., 3], f[..., 3] if alpha else np.full((8, 16), 255))
    assert out.encode(None) == ({}, [])


def test_mux_refuses_rates_above_90():
    for fps in (91, 90.5, 100, 120):
        with pytest.raises(ValueError, match='fps'):
            encoders.WebPOutput(fps=fps)
    encoders.WebPOutput(fps=90)
    for fps in (0, -1):
        with pytest.raises(ValueError, match='fps'):
            encoders.WebPOutput(fps=fps)


@needs_webp
def test_one_frame_file_is_the_simple_format():
    frame = some_frames(1)[0]
    blk = M.encode(frame, 4)
    out = encoders.WebPOutput(alpha=True)
    assert out.encode(_Record.of(blk)) == ({}, [])
    data = out.encode(None)[0]['.webp'].read()
    assert data == M.write_still(blk) == b'RIFF' + struct.pack('<I', 4 + len(blk)) + b'WEBP' + blk
    parsed = M.read_file(data)
    assert not parsed['animated'] and parsed['blocks'] == [blk]
    size, frames = frames_of(data)
    assert size == (16, 8) and len(frames) == 1 and np.array_equal(frames[0][0], frame)
    # two frames of the same pixels: another container around the same block
    out.encode(_Record.of(blk))
    out.encode(_Record.of(blk))
    two = out.encode(None)[0]['.webp'].read()
    assert two == M.write_animation([blk, blk], 16, 8, True, 0, M.durations(2, 24)) and two[12:16] == b'VP8X'
    assert out.encode(None) == ({}, [])


def test_mux_starts_a_new_file_when_the_size_changes():
    a, b = some_blocks(2, 16, 8, 3), some_blocks(2, 8, 16, 3)
    out = encoders.WebPOutput(fps=25)
    assert out.encode(_Record.of(a[0])) == ({}, []) and out.encode(_Record.of(a[1])) == ({}, [])
    media, _ = out.encode(_Record.of(b[0]))
    assert media['.webp'].read() == M.write_animation(a, 16, 8, False, 0, M.durations(2, 25))
    media, _ = out.encode(_Record.of(a[0]))                    # one frame of the other size: a simple file
    assert media['.webp'].read() == M.write_still(b[0])
    assert out.encode(_Record.of(a[1])) == ({}, [])
    media, _ = out.encode(None)
    assert media['.webp'].read() == M.write_animation(a, 16, 8, False, 0, M.durations(2, 25))       # (the durations start over with the file)
    with pytest.raises(_lib.FlameError, match='needs'):
        out.encode(_Record.of(a[0], status=1))
    with pytest.raises(IOError):
        out.encode(_Record.of(b'VP8 ' + a[0][4:]))
    out.encode(_Record.of(a[0]))
    out.abort()
    assert out.encode(None) == ({}, [])


def test_a_file_that_would_pass_4_gib_names_shard(monkeypatch):
    blocks = some_blocks(3)
    out = encoders.WebPOutput()
    assert out.LIMIT == encoders.WebPOutput.LIMIT == (1 << 32) - 10
    monkeypatch.setattr(encoders.WebPOutput, 'LIMIT', 12 + 18 + 14 + 2 * (24 + len(blocks[0])) + 10)
    out.encode(_Record.of(blocks[0]))
    out.encode(_Record.of(blocks[1]))
    with pytest.raises(IOError, match='shard'):
        out.encode(_Record.of(blocks[2]))
    assert out.encode(None) == ({}, [])


def test_container_reader_refuses():
    blocks = some_blocks(2)
    good = M.write_animation(blocks, 16, 8, True, 0, [40, 40])
    assert M.read_file(good)['blocks'] == blocks
    for bad in (good[:4] + struct.pack('<I', len(good)) + good[8:], good[:20] + b'\x10' + good[21:], good[:-1], b'RIFX' + good[4:],
                M.write_animation(blocks[:1], 16, 8, True, 0, [40]), good.replace(b'ANMF', b'ANMG', 1),
                M.write_still(blocks[0]) + b'\0\0'):
        with pytest.raises(M.WebPError):
            M.read_file(bad)


class StubLib(object):
    def __init__(self):
        self.calls = []

    def fl_webp_bound(self, w, h, channels):
        self.calls.append(('fl_webp_bound', w, h, channels))
        return M.bound(w, h, channels)

    def fl_output_webp(self, ctx, w, h, channels, host, dev, cap):
        self.calls.append(('fl_output_webp', ctx, w, h, channels, host, dev, cap))
        return 0

    def fl_last_error(self):
        return b''


class StubFB(object):
    ctx = 1234

    def host_buffer(self, shape, dtype):
        self.last = np.zeros(shape, dtype)
        return self.last


def test_output_calls_the_library(monkeypatch):
    stub = StubLib()
    monkeypatch.setattr(_lib, 'load', lambda: stub)
    dim = render.Framebuffers.calc_dim(64, 48)
    for kw, channels in ((dict(), 3), (dict(alpha=True, loop=3), 4), (dict(alpha=False), 3)):
        out = encoders.WebPOutput(**kw)
        cap = M.bound(64, 48, channels)
        assert isinstance(out, output.DeviceEncodedOutput) and (out.suffix, out.entry) == ('.webp', 'fl_output_webp')
        assert out.shape(dim) == (cap,) and np.dtype(out.dtype) == np.uint8
        fb = StubFB()
        buf = out.copy(fb, dim)
        assert buf is fb.last and stub.calls[-1] == ('fl_output_webp', 1234, 64, 48, channels, buf.ctypes.data, 0, cap)
    assert set(c[0] for c in stub.calls) == {'fl_webp_bound', 'fl_output_webp'}


def test_output_options():
    for bad in (dict(alpha=1), dict(alpha='yes'), dict(alpha=None), dict(loop=-1), dict(loop=65536), dict(loop=True), dict(loop='0'), dict(loop=1.0)):
        with pytest.raises(ValueError):
            encoders.WebPOutput(**bad)
    for bad in (dict(quality=90), dict(colors=16), dict(lossless=True)):
        with pytest.raises(TypeError):
            encoders.WebPOutput(**bad)


# ------------------------------------------------------------------ the profile keys and the command line
def test_profile_keys():
    gnm, prof = configs.cfg2()

    def out_for(block, **over):
        return output.get_output_for_profile(profile.wrap(dict(prof, output=block, **over), gnm))

    dev = out_for({'type': 'webp'})
    assert type(dev) is encoders.WebPOutput and (dev.alpha, dev.channels, dev.loop, dev.fps) == (False, 3, 0, profile.wrap(prof, gnm).fps)
    dev = out_for({'type': 'webp', 'alpha': True, 'loop': 2}, fps=60)
    assert (dev.alpha, dev.channels, dev.loop, dev.fps) == (True, 4, 2, 60)
    for key, value in (('quality', 90), ('bits', 8), ('filter', 'paeth'), ('compression', 'deflate'), ('device', True), ('encoder', 'device'),
                       ('optimize', True), ('sampling', '420'), ('crf', 10), ('pix_fmt', 'yuv420p'), ('colors', 16), ('dither', 'none'), ('lossless', True)):
        with pytest.raises(ValueError, match=key):
            out_for({'type': 'webp', key: value})
    with pytest.raises(ValueError, match='pixel'):
        out_for({'type': 'webp', 'pixel': 'half'})
    with pytest.raises(ValueError, match=r'output\.loop'):
        out_for({'type': 'webp', 'loop': 70000})
    with pytest.raises(ValueError, match=r'output\.alpha'):
        out_for({'type': 'webp', 'alpha': 'yes'})
    with pytest.raises(ValueError, match='fps'):
        out_for({'type': 'webp'}, fps=120)
    # loop on every type but gif and webp
    others = ({'type': 'jpeg'}, {}, {'type': 'jpeg', 'device': True}, {'type': 'png'}, {'type': 'png', 'encoder': 'device'}, {'type': 'tiff'},
              {'type': 'tiff', 'compression': 'deflate'}, {'type': 'exr'}, {'type': 'raw'}, {'type': 'raw16'}, {'type': 'mjpeg'}, {'type': 'x264'},
              {'type': 'vp9'}, {'type': 'vp8'}, {'type': 'prores'})
    for block in others:
        with pytest.raises(ValueError, match='loop'):
            out_for(dict(block, loop=0))
    assert out_for({'type': 'gif', 'loop': 4}).loop == 4
    assert output.get_suffix('webp') == '.webp' == output.get_suffix('webp', True) and 'webp' in output._VIDEO
    assert output.get_suffix_for_profile(profile.wrap(dict(prof, output={'type': 'webp', 'alpha': True}), gnm)) == '.webp'
    # nothing else moved
    assert type(out_for({'type': 'gif'})) is encoders.GIFOutput and type(out_for({'type': 'exr'})) is output.DeviceEXROutput
    assert type(out_for({'type': 'png', 'encoder': 'device'})) is output.DevicePNGOutput and type(out_for({})) is output.PILOutput
    assert output.get_suffix('png', True) == '_color.png' and output.get_suffix('gif') == '.gif'


def test_command_line_options():
    parser = profile.add_args(argparse.ArgumentParser())

    def out_of(*argv):
        return profile.get_from_args(parser.parse_args(list(argv)))[1].get('output')

    assert out_of('--codec', 'webp') == {'type': 'webp'}
    with pytest.raises(SystemExit):
        parser.parse_args(['--codec', 'WEBP'])
    gnm, _ = configs.cfg2()

    def out_for(*argv):
        return output.get_output_for_profile(profile.wrap(profile.get_from_args(parser.parse_args(list(argv)))[1], gnm))

    dev = out_for('--codec', 'webp', '--fps', '25')
    assert type(dev) is encoders.WebPOutput and (dev.alpha, dev.loop, dev.fps) == (False, 0, 25)
    assert type(out_for('--codec', 'webp', '--still')) is encoders.WebPOutput
    with pytest.raises(ValueError, match='fps'):
        out_for('--codec', 'webp', '--fps', '120')
    for extra in (('--device-encode',), ('--quality', '90'), ('--bits', '16'), ('--tiff-compression', 'deflate'), ('--png-filter', 'adaptive'), ('--optimize',),
                  ('--exr-pixel', 'half'), ('--gif-colors', '16'), ('--gif-dither', 'none')):
        with pytest.raises(ValueError):
            out_for('--codec', 'webp', *extra)


def test_the_spec_knows_the_type():
    from cuburn_amd.genome import specs
    assert 'webp' in specs.profile['output']['type'].choices and 'gif' in specs.profile['output']['type'].choices


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_entry_points(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('fl_webp_bound', 'fl_webp_encode', 'fl_output_webp'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert re.search(r'#define\s+FL_WEBP_PB\s+4\b', code) and re.search(r'#define\s+FL_WEBP_EB\s+6\b', code)
    assert (_lib.WEBP_PB, _lib.WEBP_EB) == (4, 6)
    assert lib.fl_abi_version() == 1
    assert lib.fl_webp_encode(None, 8, 8, 1, 4, 1, 0, 4096) == _lib.FL_E_INVAL      # (a null context: refused before the device is touched)
    assert lib.fl_output_webp(None, 8, 8, 4, 1, 0, 4096) == _lib.FL_E_INVAL
    mk = open(os.path.join(REPO, 'cuburn_amd', 'csrc', 'Makefile')).read()
    assert 'webp.hip' in mk and re.search(r'webp\.o:\s*encode_device\.h', mk)


def test_bound(built):
    lib = _lib.load()
    for w, h, ch in ((0, 8, 4), (8, 0, 4), (16385, 8, 4), (8, 16385, 3), (65535, 65535, 4), (8, 8, 2), (8, 8, 5), (8, 8, 0), (8, 8, 1)):
        assert lib.fl_webp_bound(w, h, ch) == 0 == M.bound(w, h, ch), (w, h, ch)
    for w, h in ((1, 1), (7, 3), (16, 16), (17, 17), (64, 64), (65, 65), (1920, 1080), (16384, 1), (1, 16384), (16384, 16384)):
        for ch in (3, 4):
            assert lib.fl_webp_bound(w, h, ch) == M.bound(w, h, ch) > 24, (w, h, ch)
    assert M.bound(16384, 16384, 4) < 1 << 32
    # 60 bits a pixel, 14644 a group and sub-image: the terms of the proof
    assert M.bound(1, 1, 4) == 16 + 8 + (49 + (1 + 14644 + 60) + 6 + (1 + 14644 + 60) + 14644 + 60 + 7) // 8 + 1
    # noise, whose every symbol costs about 8 bits, and every case are inside it
    for name in WC.NAMES:
        frame, ch = WC.cases()[name]
        assert 16 + len(WC.model_block(name)) <= M.bound(frame.shape[1], frame.shape[0], ch)
