"""
Named frames for the WebP suites (test_cpu_webp.py, test_gpu_webp.py): name -> (u8 [h][w][4], channels).  The model's block of
every case is computed once and shared.
"""
import functools

import numpy as np

import webp_model as M


def plasma(w, h, seed):
    """Smooth colour with a little noise and an alpha that varies."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    px = np.stack([xx * 3 + yy, xx + yy * 2, (xx * yy) >> 3, 255 - ((xx + 3 * yy) >> 1)], -1)
    return ((px + rs.randint(0, 4, px.shape)) & 255).astype(np.uint8)


def noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 4)).astype(np.uint8)


def six_modes():
    """96 x 32: 16 x 16 tiles of textures that each suit another predictor (test_cpu_webp.py checks that all six modes win)."""
    rs = np.random.RandomState(5)
    yy, xx = np.mgrid[0:16, 0:16]
    one = lambda v: np.repeat(np.asarray(v)[..., None], 4, axis=-1)
    tiles = [
        one(np.repeat(rs.randint(0, 256, (16, 1)), 16, axis=1)),                 # rows of one value: L
        one(np.repeat(rs.randint(0, 256, (1, 16)), 16, axis=0)),                 # columns of one value: T
        one(60 + 3 * xx + 2 * yy + rs.randint(0, 9, (16, 16))),                  # a noisy slope: an average
        one(100 + ((xx * xx + yy * yy) >> 3) + rs.randint(0, 3, (16, 16))),      # a curved surface
        one(np.where((xx > 6) ^ (yy > 9), 200, 30) + np.where(xx + yy > 17, 20, 0)),      # flat regions with edges: select
        one(7 * xx + 5 * yy),                                                    # a plane: L + T - TL
    ]
    row = np.concatenate(tiles, axis=1)
    frame = np.concatenate([row, np.roll(row, 16, axis=1)[::-1]], axis=0) & 255
    frame[..., 3] = 255 - frame[..., 3] // 2
    return frame.astype(np.uint8)


def cost_ties():
    """32 x 32, four tiles.  Top left: flat, and column 16 holds the same value, so all six modes predict every pixel and tie.  Top
    right: columns of one value each, so 2, 11 and 12 tie (a flat column to the left is such a column too).  Bottom: rows of one value
    each below the flat tile, so 1, 11 and 12 tie in the left one."""
    rs = np.random.RandomState(6)
    g = np.full((32, 32), 90)
    g[:16, 17:] = rs.randint(0, 256, (1, 15))
    g[16:, :] = rs.randint(0, 256, (16, 1))
    return np.stack([g, g, g, np.full_like(g, 255)], -1).astype(np.uint8)


def _walk(rs, counts):
    """[64][64] values whose steps along every row (column 0 holds 0 everywhere) take value v counts[v] times, 4032 in all."""
    steps = np.concatenate([np.full(n, v) for v, n in counts.items()])
    assert len(steps) == 64 * 63
    rs.shuffle(steps)
    return np.concatenate([np.zeros((64, 1), np.int64), np.cumsum(steps.reshape(64, 63), axis=1)], axis=1)


LADDER_LENGTHS = {2: 1, 3: 1, 4: 1, 5: 3, 6: 10, 7: 18, 8: 21, 9: 30, 10: 23, 11: 15, 12: 6}      # symbols per code length: Kraft's sum is 1


def ladder():
    """64 x 64, one entropy tile, every row a walk from its left neighbour, so that mode 1 wins and the steps are the residuals.
    Green's seventeen step values are counted 1, 1, 1, 3, 4, 7, 11, ... 843 and the rest: each count is one more than the sum of all
    but the last before it, the steepest ladder under build_lengths' rule that a tie takes the leaf, so Huffman's tree is a chain of
    depth 16 (3570 pixels suffice) and the limit of 15 has to cut it.
    Alpha's 129 step values are counted 2^(12 - length) with LADDER_LENGTHS symbols per length, which is the code they get; the
    counts of those lengths as token kinds — 1, 1, 1, 3, 10, 18, 21, 30, 23, 15, 6 — make a code of depth 8 that the limit of 7
    has to cut (test_cpu_webp.py checks both properties on the model's residuals)."""
    rs = np.random.RandomState(7)
    rungs = [1, 1, 1]
    while len(rungs) < 16:
        rungs.append(sum(rungs[:-1]) + 1)
    counts = dict(zip(range(16, 0, -1), rungs))
    counts[0] = 64 * 63 - sum(rungs)
    g = _walk(rs, counts)
    lens = [ln for ln, n in sorted(LADDER_LENGTHS.items()) for _ in range(n)]
    counts = dict((i, 1 << (12 - ln)) for i, ln in enumerate(lens))        # values 0 .. 128: no zero run among the lengths
    counts[0] -= 64                                                        # column 0 brings 64 residuals of 0
    a = 255 + _walk(rs, counts)
    out = np.stack([g, g, g, a], -1)
    return (out & 255).astype(np.uint8)


def wide():
    """1088 x 1024: 272 groups, so the entropy sub-image's red is not 0; smooth, so that the model is quick."""
    yy, xx = np.mgrid[0:1024, 0:1088]
    return np.stack([(xx >> 3) + (yy >> 4), (xx >> 2) & 255, ((xx + yy) >> 3) & 255, np.full_like(xx, 255)], -1).astype(np.uint8) & 255


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for w, h in ((1, 1), (1, 70), (70, 1), (16, 16), (17, 17), (64, 64), (65, 64), (64, 65), (130, 70)):
        out['plasma_%dx%d' % (w, h)] = (plasma(w, h, 10 + w + h), 4)
    out['flat_130x70'] = (np.zeros((70, 130, 4), np.uint8), 3)         # every code one symbol: no pixel emits a bit
    out['noise_128x128'] = (noise(128, 128, 3), 4)
    out['six_modes'] = (six_modes(), 4)
    out['cost_ties'] = (cost_ties(), 3)
    out['alpha_rgba'] = (plasma(50, 40, 4), 4)
    out['alpha_rgb'] = (plasma(50, 40, 4), 3)                          # the same source, alpha read as 255
    out['ladder'] = (ladder(), 4)
    out['wide_1088x1024'] = (wide(), 3)
    return out


NAMES = ('plasma_1x1', 'plasma_1x70', 'plasma_70x1', 'plasma_16x16', 'plasma_17x17', 'plasma_64x64', 'plasma_65x64', 'plasma_64x65', 'plasma_130x70',
         'flat_130x70', 'noise_128x128', 'six_modes', 'cost_ties', 'alpha_rgba', 'alpha_rgb', 'ladder', 'wide_1088x1024')


@functools.lru_cache(maxsize=None)
def model_block(name):
    frame, channels = cases()[name]
    return M.encode(frame, channels)


def expected(name):
    frame, channels = cases()[name]
    want = frame.copy()
    if channels == 3:
        want[..., 3] = 255
    return want
