"""
The frames tests/test_cpu_tiff.py and tests/test_gpu_tiff.py give the TIFF model and the device's TIFF encoder: the smallest at which
the tiling, the predictor, the padding and the placement can go wrong.  Sources are u8 / u16 [h][w][4], as the device takes them.
"""
import numpy as np

import tiff_model as T

FORMS = ((8, 3), (8, 4), (16, 3), (16, 4))                    # (bits, channels)


def form_id(form):
    return '%dbit-%dch' % form


def dtype_of(bits):
    return np.uint8 if bits == 8 else np.uint16


def noise(w, h, bits, seed):
    return np.random.RandomState(seed).randint(0, 1 << bits, (h, w, 4)).astype(dtype_of(bits))


def small_shapes():
    """1 x 1: one tile, inline offsets, padding everywhere; a column; a row."""
    return ((1, 1), (1, 7), (7, 1))


def edge_shapes(bits):
    """Exactly one full tile; two tiles of which the second is almost all padding, to the right and below."""
    tw = T.tile_width(bits)
    return ((tw, 64), (tw + 1, 64), (tw, 65))


def reader_shapes(bits):
    tw = T.tile_width(bits)
    return ((1, 1), (tw, 64), (tw + 1, 65), (2 * tw + 3, 70))


MIXED_SEED = {(8, 3): 0, (8, 4): 0, (16, 3): 0, (16, 4): 0}   # chosen on the CPU (test_cpu_tiff.py checks what they give)


def mixed(bits, seed):
    """(2 TW + 3) x 70: six tiles.  Smooth ramps with a little texture, which code as dynamic blocks, and noise over the whole of the
    first tile, which is stored."""
    tw = T.tile_width(bits)
    w, h = 2 * tw + 3, 70
    rs = np.random.RandomState(1000 + seed)
    y, x = np.mgrid[0:h, 0:w]
    top = (1 << bits) - 1
    img = np.empty((h, w, 4), np.int64)
    for c in range(4):
        a, b = rs.randint(1, 5, 2)
        img[:, :, c] = (x * a * (top // 1024 + 1) + y * b * (top // 512 + 1) + c * 37 + rs.randint(0, 3, (h, w))) % (top + 1)
    img[:64, :tw] = rs.randint(0, top + 1, (64, tw, 4))
    return img.astype(dtype_of(bits))


def mixed_properties(data):
    """What the mixed frame must show in the model's file: (tiles, block types, an odd tile before the last)."""
    ps = T.parse(data)
    return ps.nt, set(ps.btypes), any(n & 1 for n in ps.counts[:-1])


def byte_order_source():
    """One row 0x00ff, 0x0100, 0xffff, 0x0000 in every channel: differences that carry and borrow across the byte boundary."""
    src = np.empty((1, 4, 4), np.uint16)
    src[0, :, :] = np.array([0x00ff, 0x0100, 0xffff, 0x0000], np.uint16)[:, None]
    return src
