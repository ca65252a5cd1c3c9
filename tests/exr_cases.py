"""
The frames tests/test_cpu_exr.py and tests/test_gpu_exr.py give the OpenEXR model and the device's OpenEXR encoder: the smallest at
which the conversion, the cropped tiles, the planar rows, the predictor, the choice between the two data forms and the placement can
go wrong.  Sources are f32 [h][w][4], as the device takes them.
"""
import numpy as np

import exr_model as X

FORMS = ((X.HALF, 3), (X.HALF, 4), (X.FLOAT, 3), (X.FLOAT, 4))      # (pixel, channels)
NAMES = {X.HALF: 'half', X.FLOAT: 'float'}


def form_id(form):
    return '%s-%dch' % (NAMES[form[0]], form[1])


def noise(w, h, pixel, seed):
    """Samples whose file bytes are noise: at float any 32 bits (NaN, infinities and denormals among them), at half the widened
    values of random finite half bits."""
    rs = np.random.RandomState(seed)
    if pixel == X.FLOAT:
        return rs.randint(0, 1 << 32, (h, w, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    hb = rs.randint(0, 1 << 16, (h, w, 4)).astype(np.uint16)
    hb[(hb & 0x7c00) == 0x7c00] &= 0x83ff
    return hb.view(np.float16).astype(np.float32)


def ramps(w, h, seed):
    """Smooth, a little textured, below 0 and above 1: multiples of 1 / 64, so the low bytes of a float are zero."""
    rs = np.random.RandomState(2000 + seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.empty((h, w, 4), np.float32)
    for c in range(4):
        a, b = rs.randint(1, 5, 2)
        img[:, :, c] = (x * a + y * b + c * 37 + rs.randint(0, 2, (h, w)) - 100) / 64.0
    return img


def small_shapes():
    """One pixel; a column; a row: one cropped tile each."""
    return ((1, 1), (1, 7), (7, 1))


def edge_shapes(pixel):
    """Exactly one tile; a second tile one pixel wide; a second tile one row high."""
    th = X.tile_rows(pixel)
    return ((64, th), (65, th), (64, th + 1))


MIXED_SEED = {(X.HALF, 3): 0, (X.HALF, 4): 0, (X.FLOAT, 3): 0, (X.FLOAT, 4): 0}      # chosen on the CPU (test_cpu_exr.py checks what they give)
MIXED_SHAPE = (131, 70)


def mixed(pixel, seed):
    """131 x 70: three tiles a row, two rows of them at half (64 + 6) and three at float (32 + 32 + 6), so the corner tile is 3 x 6
    pixels at either depth.  Ramps, which compress; noise over the whole of the first tile, which is stored raw; zeros over the second."""
    w, h = MIXED_SHAPE
    th = X.tile_rows(pixel)
    img = ramps(w, h, seed)
    img[:th, :64] = noise(64, th, pixel, 1000 + seed)
    img[:th, 64:128] = 0.0
    return img


def mixed_properties(data):
    """What the mixed frame must show in the model's file: (tiles, forms in order, the corner tile's bytes)."""
    ps = X.parse(data)
    return ps.nt, ps.forms, ps.sizes[-1]


def _widen(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


def half_atlas():
    """Every float the conversion can get wrong, 256 * 1024 of them: all 65536 half values widened; the midpoint of every pair of
    neighbouring halves of one sign (65520, the midpoint to the first value out of range, among them) with the floats next to it on
    either side; the edges of the range; the half denormals' range and below, down into the float denormals."""
    allh = _widen(np.arange(65536, dtype=np.uint32))
    with np.errstate(invalid='ignore'):
        lo = _widen(np.arange(0, 0x7c00, dtype=np.uint32)).astype(np.float64)
        hi = np.concatenate([lo[1:], [65536.0]])
        mid = ((lo + hi) / 2).astype(np.float32)                  # exact: a half has 11 significant bits, a float 24
    assert np.array_equal(mid.astype(np.float64), (lo + hi) / 2)
    below, above = np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))
    mids = np.concatenate([mid, below, above])
    special = np.array([65504.0, 65519.996, 65520.0, 65536.0, 1e9, np.inf, -np.inf, np.nan, 0.0, -0.0, 3.4028235e38, -3.4028235e38], np.float32)
    special = np.concatenate([special, -special[:5], np.array([0x7fc00001, 0xffc00000, 0x7f800001, 0xff800001], np.uint32).view(np.float32)])
    tiny = np.concatenate([np.ldexp(np.float32(1), -np.arange(14, 60)).astype(np.float32),
                           np.ldexp(np.float32(1.5), -np.arange(14, 60)).astype(np.float32),
                           np.arange(1, 64, dtype=np.uint32).view(np.float32),                        # float denormals
                           (np.uint32(0x33000000) + np.arange(-8, 9).astype(np.uint32)).view(np.float32),      # around 2^-25: the tie to zero
                           np.array([0x007fffff, 0x00800000, 0x00000001], np.uint32).view(np.float32)])
    vals = np.concatenate([allh, mids, -mids, special, tiny, -tiny]).astype(np.float32)
    assert vals.size <= 256 * 1024
    out = np.zeros(256 * 1024, np.float32)
    out[:vals.size] = vals
    return out


def atlas_frame():
    """The atlas as a 256 x 1024 frame: R holds it, G holds it backwards, B negated, A is 1."""
    a = half_atlas().reshape(1024, 256)
    img = np.empty((1024, 256, 4), np.float32)
    img[:, :, 0], img[:, :, 1], img[:, :, 2], img[:, :, 3] = a, a[::-1, ::-1], -a, 1.0
    return img


def front_values(n, seed):
    """n float4 for a front buffer: below 0 and above 1, a NaN and an infinity among them."""
    rs = np.random.RandomState(seed)
    v = (rs.rand(n, 4) * 6.0 - 2.0).astype(np.float32)
    return v
