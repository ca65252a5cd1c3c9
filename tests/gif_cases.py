"""
The frames tests/test_cpu_gif.py and tests/test_gpu_gif.py give the GIF model and the device's GIF encoder: the smallest at which
the histogram, the cut, the lookup, the dither, the segments' ends, the code widths and the sub-blocks can go wrong.  Sources are
u8 [h][w][4] as FL_OUT_RGBA8 writes them; the alpha byte is noise, since the encoder must ignore it.
"""
import numpy as np

import gif_model as M


def _rgba(rgb, seed=0):
    rgb = np.asarray(rgb, np.uint8)
    a = np.random.RandomState(77 + seed).randint(0, 256, rgb.shape[:2] + (1,)).astype(np.uint8)
    return np.ascontiguousarray(np.concatenate([rgb, a], 2))


def noise(w, h, seed):
    return _rgba(np.random.RandomState(seed).randint(0, 256, (h, w, 3)), seed)


def lone_colours():
    """256 colours, each alone in its cell: cell coordinates (k & 31, k >> 5, 12), with low bits that differ."""
    k = np.arange(256)
    return np.stack([8 * (k & 31) + k % 7, 8 * (k >> 5) + 2 + k % 5, np.full(256, 100)], 1).astype(np.uint8)


def lone_noise(n, seed):
    """One row of n pixels drawn from lone_colours, no pair of neighbours twice: with 256 entries every pixel comes back exactly,
    no string is ever found in the dictionary, and every pixel costs a code."""
    rs = np.random.RandomState(seed)
    pick = list(rs.permutation(256))                  # every colour is there
    seen = set(zip(pick[:-1], pick[1:]))
    while len(pick) < n:
        c = int(rs.randint(0, 256))
        if (pick[-1], c) not in seen:
            seen.add((pick[-1], c))
            pick.append(c)
    return _rgba(lone_colours()[np.array(pick[:n])][None], seed)


def black(w, h):
    return _rgba(np.zeros((h, w, 3), np.uint8))


def one_bright(w, h):
    img = np.zeros((h, w, 3), np.uint8)
    img[h // 3, w // 5] = (250, 200, 30)
    return _rgba(img)


def gradient(w=96, h=64):
    """Red along x and green along y over the whole range, blue fixed: 32 x 32 cells at this size, far more than 256."""
    y, x = np.mgrid[0:h, 0:w]
    return _rgba(np.stack([x * 255 // (w - 1), y * 255 // (h - 1), np.full((h, w), 77)], 2))


def flame_like(w=320, h=180, seed=5):
    """A black ground with six soft coloured blobs, gamma 2.2 and half a level of noise."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    lin = np.zeros((h, w, 3))
    for _ in range(6):
        cx, cy, rad = rs.uniform(0.1, 0.9) * w, rs.uniform(0.1, 0.9) * h, rs.uniform(0.08, 0.25) * h
        col = rs.uniform(0.1, 1.0, 3)
        lin += np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * rad * rad))[:, :, None] * col[None, None, :]
    img = 255.0 * np.clip(lin, 0, 1) ** (1 / 2.2) + rs.uniform(-0.5, 0.5, (h, w, 3))
    return _rgba(np.clip(np.rint(img), 0, 255), seed)


GRADIENT_FORMS = tuple((c, a) for c in (2, 16, 256) for a in (0, 8, 64))
STEP_LENGTHS = tuple(range(250, 261)) + tuple(range(762, 771))      # the last segment's pixels: its final code falls on and around the 9 -> 10 and 10 -> 11 bit steps
MOD255 = {0: 1661, 1: 1250, 254: 1239}      # one-row noise frames (seed = the width) whose data stream's length mod 255 is the key: test_cpu_gif.py checks it


_cases = {}


def cases():
    """name -> (frame, colors, amp); built once, never changed."""
    if _cases:
        return _cases
    out = {'1x1': (noise(1, 1, 1), 256, 8),
           'n1023': (noise(1023, 1, 2), 256, 8), 'n1024': (noise(32, 32, 3), 256, 8), 'n1025': (noise(41, 25, 4), 256, 8),
           '37x29': (noise(37, 29, 5), 256, 8), '37x29_flame': (flame_like(37, 29, 6), 256, 8),
           'black': (black(64, 64), 256, 8), 'one_bright': (one_bright(64, 64), 256, 8),
           'few_colours': (lone_noise(1024 + 300, 9), 256, 0),
           'flame_wide': (flame_like(700, 200, 7), 256, 8)}      # above 512 * 256 pixels: the histogram's waves take more than one step
    for L in STEP_LENGTHS:
        out['step_%d' % L] = (lone_noise(1024 + L, 100 + L), 256, 0)
    for colors, amp in GRADIENT_FORMS:
        out['gradient_c%d_a%d' % (colors, amp)] = (gradient(), colors, amp)
    for r, n in sorted(MOD255.items()):
        out['mod255_%d' % r] = (noise(n, 1, n), 256, 8)
    _cases.update(out)
    return _cases


NAMES = tuple(cases())
_models = {}


def model(name):
    """(palette, indices, nb) of a case by the model, computed once."""
    if name not in _models:
        _models[name] = M.quantise(*cases()[name])
    return _models[name]


_blocks = {}


def model_block(name, seg=M.SEG):
    """The model's frame block of a case, computed once."""
    if (name, seg) not in _blocks:
        frame = cases()[name][0]
        pal, idx, _ = model(name)
        _blocks[(name, seg)] = M.block_of(frame.shape[1], frame.shape[0], pal, idx, seg)
    return _blocks[(name, seg)]
