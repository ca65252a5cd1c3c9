"""
The frames tests/test_cpu_png_ext.py and tests/test_gpu_png_ext.py encode with the extended device PNG format (a depth of 16 bits,
a filter type per row): the smallest shapes at which the filter stage can go wrong.  Frames are built as byte images, u8 [h][w][bpp]
in file order (png_ext_model), and handed to the device as the u8 or u16 [h][w][4] source that holds them (`source`).
"""
import numpy as np

import png_ext_model as X

FORMS = [(bits, ch, flags) for bits in (8, 16) for ch in (3, 4) for flags in (0, X.ADAPTIVE)]
MODEL_SEG = 32768
TEN_BAND_W = (5, 33, 37, 40)          # with bpp 3, 4, 6, 8: rowlen mod 4 takes every value
# the rows of ten_band (0-based) that are built for one filter type each, and the tie
ROW_TIE, ROW_UP, ROW_NONE, ROW_SUB, ROW_AVERAGE, ROW_PAETH = 0, 2, 3, 5, 7, 9


def form_id(form):
    bits, ch, flags = form
    return '%s%d_%s' % ('rgb' if ch == 3 else 'rgba', bits, 'adaptive' if flags else 'paeth')


def source(bytes_img, channels, bits):
    """u8 / u16 [h][w][4] in native byte order whose first `channels` samples are the byte image's; an alpha the file leaves out is
    set to a value that would show if it were coded."""
    h, w, _ = bytes_img.shape
    s = X.samples_of(np.ascontiguousarray(bytes_img), bits)
    out = np.full((h, w, 4), 0x5a if bits == 8 else 0x5aa5, s.dtype)
    out[:, :, :channels] = s
    return out


def ten_band(w, bpp, seed=5):
    """u8 [10][w][bpp]: ten rows, one for each thing the choice of a filter type can meet.  Row 0 is a five-way tie (type 0); rows
    2, 3, 5, 7 and 9 are built so that Up, None, Sub, Average and Paeth leave nothing or next to nothing; the rest is noise."""
    rs = np.random.RandomState(seed + 131 * w + bpp)
    n = w * bpp
    px, k = np.arange(n) // bpp, np.arange(n) % bpp
    rows = np.zeros((10, n), np.uint8)
    rows[1] = rs.randint(0, 256, n)
    rows[2] = rows[1]
    rows[3] = px & 1
    rows[4] = rs.randint(0, 256, n)
    rows[5] = (100 + 3 * px + 17 * k) & 255
    rows[6] = rs.randint(0, 256, n)
    for i in range(n):
        rows[7, i] = ((int(rows[7, i - bpp]) if i >= bpp else 0) + int(rows[6, i])) >> 1
    half = (w // 2) * bpp
    rows[8, :half] = rs.randint(0, 256, half)
    rows[8, half:] = 200
    rows[9, :half] = rows[8, :half]
    rows[9, half:] = 90
    return rows.reshape(10, w, bpp)


def noise(w, h, bpp, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, bpp)).astype(np.uint8)


def soft(w, h, channels, bits, seed):
    """A gradient with a little noise in the low bits: compressible, and no two rows alike."""
    rs = np.random.RandomState(seed)
    x, y, c = np.arange(w)[None, :, None], np.arange(h)[:, None, None], np.arange(channels)[None, None, :]
    if bits == 8:
        return ((x * 3 + y * 5 + c * 40 + rs.randint(0, 3, (h, w, channels))) & 255).astype(np.uint8)
    v = ((x * 700 + y * 1100 + c * 9000 + rs.randint(0, 48, (h, w, channels))) & 65535).astype(np.uint16)
    return X.byte_image(v, channels, 16)


def soft_shape(seg, bpp):
    """(w, h) of a frame of at least three segments whose boundaries fall inside rows."""
    w = 211
    rowlen = 1 + w * bpp
    h = -(-(2 * seg + seg // 3) // rowlen)
    assert h * rowlen > 2 * seg and seg % rowlen and (2 * seg) % rowlen
    return w, h


def byte_order_source():
    """u16 [5][6][4]: the samples 0x00FF, 0xFF00, 0x0100, 0x0001 in turn, shifted from pixel to pixel and row to row."""
    pat = np.array([0x00ff, 0xff00, 0x0100, 0x0001], np.uint16)
    y, x, s = np.arange(5)[:, None, None], np.arange(6)[None, :, None], np.arange(4)[None, None, :]
    return pat[(y + x + s) % 4]
