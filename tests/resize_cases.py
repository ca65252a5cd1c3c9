"""
The cases of the Lanczos downscale's tests: the shapes, the two inputs each runs on, and the shared model
results.  Used by tests/test_cpu_resize.py and tests/test_gpu_resize.py; nothing here touches the device.
"""
import functools

import numpy as np

import resize_model as M

# (w, h, w2, h2): the smallest shapes at which the kernels can go wrong.  k_resize_rows takes 64 output columns by 16 source rows
# per workgroup, k_resize_cols 64 padded columns by 16 padded rows with source bands of 16 rows.
CASES = [
    (64, 36, 24, 9),        # non-integer ratios 2.67 and 4; astride 96 > aw 88
    (40, 24, 40, 24),       # ratio 1
    (400, 264, 50, 33),     # ratio 8: the widest tables
    (333, 131, 167, 47),    # odd sizes across tile seams
    (600, 40, 301, 20),     # more than one row segment
    (40, 400, 20, 57),      # a tall source window
]
IDS = ['%dx%d-%dx%d' % c for c in CASES]


@functools.lru_cache(maxsize=None)
def tables(w, h, w2, h2):
    return M.tables(w, w2), M.tables(h, h2)


def noisy_source(case, seed=0):
    """Gamma-distributed values with negative ones mixed in over the picture area; NaN in every gutter and padding bin."""
    w, h = case[:2]
    _, _, _, ah, astride = M.calc_dim(w, h)
    rs = np.random.RandomState(1000 + 7 * w + h + seed)
    src = np.full((ah, astride, 4), np.nan, np.float32)
    pic = rs.gamma(0.7, 1.5, (h, w, 4)).astype(np.float32)
    pic *= np.where(rs.uniform(size=pic.shape) < 0.25, np.float32(-1.0), np.float32(1.0))
    src[M.GUTTER:M.GUTTER + h, M.GUTTER:M.GUTTER + w] = pic
    return src


def impulse_positions(case):
    """Source bins (x, y) of the picture area: the four corners, the seams of the kernels' tiles and an interior bin."""
    w, h, w2, h2 = case
    (xf, xt), (yf, yt) = tables(*case)
    pos = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2 + 1, h // 2 - 1)]
    if w2 > 64:                                      # the last source bin of output column 63's window and the first of column 64's
        pos += [(int(xf[63]) + xt.shape[1] - 1, h // 3), (int(xf[64]), h // 3)]
    if w2 + M.GUTTER > 64:                           # the padded columns 63 | 64 of the second kernel's strips
        pos += [(int(xf[63 - M.GUTTER]) + xt.shape[1] // 2, 2), (int(xf[64 - M.GUTTER]) + xt.shape[1] // 2, 2)]
    if h > 16:                                       # source rows 15 | 16: two workgroups of the first kernel
        pos += [(w // 3, 15), (w // 3, 16)]
    if h2 + M.GUTTER > 16:                           # padded rows 15 | 16 of the result: output rows 3 | 4
        pos += [(1, int(yf[3]) + yt.shape[1] - 1), (1, int(yf[4]))]
        lo = int(min(yf[4:20].min(), h - 1)) if h2 > 4 else 0
        if lo + 16 < h:                              # the seam of the second kernel's first two source bands
            pos += [(w - 2, lo + 15), (w - 2, lo + 16)]
    return sorted(set((min(max(x, 0), w - 1), min(max(y, 0), h - 1)) for x, y in pos))


def impulse_source(case):
    """Lone impulses, far enough apart in value to tell them apart, zero elsewhere (gutter included)."""
    w, h = case[:2]
    _, _, _, ah, astride = M.calc_dim(w, h)
    src = np.zeros((ah, astride, 4), np.float32)
    for k, (x, y) in enumerate(impulse_positions(case)):
        src[M.GUTTER + y, M.GUTTER + x] = np.array([1.0, -2.0, 0.5, 3.0], np.float32) * np.float32(1 + k)
    return src


@functools.lru_cache(maxsize=None)
def expected(case, which):
    """(src, model, A, nxt, nyt) of a case on the 'noisy' or the 'impulse' input: computed once, shared, read-only."""
    src = noisy_source(case) if which == 'noisy' else impulse_source(case)
    xt, yt = tables(*case)
    out, A, nxt, nyt = M.resize(src, case[0], case[1], case[2], case[3], xt, yt)      # (the model looks at the picture area only)
    for a in (src, out, A):
        a.setflags(write=False)
    return src, out, A, nxt, nyt
