"""
The frames tests/test_cpu_mjpeg.py and tests/test_gpu_mjpeg.py encode in 4:2:0: the smallest shapes at which each part of that
form can go wrong.  As in jpeg_cases.py a case is (name, build(ri) -> (planes u8 [3][h][w], quality), check(stats, ri)), `check`
asserting from the statistics of jpeg420_model.parse that the stream contains what the case is named for.
"""
import numpy as np

MODEL_RI = 4              # the interval the CPU tests use; the GPU tests take the device's from its record


def _noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (3, h, w)).astype(np.uint8)


def _size(w, h):
    def check(st, ri):
        assert st['blocks'] == 6 * ((w + 15) // 16) * ((h + 15) // 16)
    return check


def _short_last(ri):          # 2 ri + 1 MCUs in a row, the last column partial: three intervals, the last of one MCU
    return _noise(16 * (2 * ri + 1) - 5, 9, 5), 50


def _check_short_last(st, ri):
    assert st['intervals'] == 3 and st['rst'] == [0, 1]
    assert st['last_interval_mcus'] == 1 and (ri == 1 or st['last_interval_mcus'] < ri)


def _wrap(ri):                # 9 ri + 1 MCUs: ten intervals
    return _noise(16 * (9 * ri + 1), 16, 6), 50


def _check_wrap(st, ri):
    assert st['intervals'] == 10 and st['rst'] == [0, 1, 2, 3, 4, 5, 6, 7, 0], st['rst']


def _check_stuffed(st, ri):
    assert st['stuffed'] >= 1


def _flat(ri):
    p = np.empty((3, 32, 48), np.uint8)
    p[0], p[1], p[2] = 77, 128, 200
    return p, 75


def _check_flat(st, ri):
    assert st['eob_only_blocks'] == st['blocks'] == 36 and st['dc_zero_diffs'] >= 24


def _dc_extremes(ri):
    """Y in columns of 8 pixels 0, 255, 0, 255, ...: inside an MCU Y00 -> Y01 -> Y10 -> Y11 is 0, 255, 0, 255 and the next MCU's
    Y00 is 0 again, so the Y predictor steps by 2040 (category 11) on both of its paths.  Chroma is 0, 255, 0 by MCU."""
    p = np.zeros((3, 16, 48), np.uint8)
    p[0][:, (np.arange(48) // 8) % 2 == 1] = 255
    p[1:, :, 16:32] = 255
    return p, 100


def _check_dc_extremes(st, ri):
    assert ri >= 2
    y, cb, cr = st['dc11_by_component']
    # Y: -1024 at an interval's start, +-2040 at every other block; chroma: -1024 first, +2040 into MCU 1 where the interval goes on
    assert y == 12 and cb >= 2 and cr >= 2, st['dc11_by_component']


def rounding_planes():
    """64 x 16, four MCUs.  In MCU m every 2 x 2 cell of Cb is (k, k, k, k + m) and of Cr (k, k + (m + 2) % 4, k, k): all sums of
    a chroma block have the same residue mod 4, so a rounding other than (sum + 2) >> 2 moves a whole block's DC by 8 at
    quality 100, far beyond criterion B."""
    rs = np.random.RandomState(9)
    p = rs.randint(0, 256, (3, 16, 64)).astype(np.uint8)
    k = rs.randint(0, 250, (2, 8, 32))
    for c in range(2):
        cells = np.repeat(np.repeat(k[c], 2, axis=0), 2, axis=1)
        for m in range(4):
            r = m if c == 0 else (m + 2) % 4
            ys, xs = (1, 1) if c == 0 else (0, 1)
            cells[ys::2, 16 * m + xs:16 * (m + 1):2] += r
        p[1 + c] = cells
    return p


def _check_rounding(st, ri):
    p = rounding_planes().astype(np.int64)
    for c in (1, 2):
        sums = p[c, 0::2, 0::2] + p[c, 0::2, 1::2] + p[c, 1::2, 0::2] + p[c, 1::2, 1::2]
        per_mcu = [set((sums[:, 8 * m:8 * m + 8] % 4).ravel()) for m in range(4)]
        assert all(len(s) == 1 for s in per_mcu) and set.union(*per_mcu) == {0, 1, 2, 3}, per_mcu


NOISE_Q100 = 'noise_64x40_q100'
CASES = [
    ('noise_1x1_q50', lambda ri: (_noise(1, 1, 1), 50), _size(1, 1)),
    ('noise_16x16_q50', lambda ri: (_noise(16, 16, 2), 50), _size(16, 16)),
    ('noise_17x17_q1', lambda ri: (_noise(17, 17, 3), 1), _size(17, 17)),
    ('noise_15x9_q95', lambda ri: (_noise(15, 9, 4), 95), _size(15, 9)),
    ('short_last_interval', _short_last, _check_short_last),
    ('rst_wraps', _wrap, _check_wrap),
    (NOISE_Q100, lambda ri: (_noise(64, 40, 7), 100), _check_stuffed),
    ('dc_extremes_q100', _dc_extremes, _check_dc_extremes),
    ('chroma_rounding_q100', lambda ri: (rounding_planes(), 100), _check_rounding),
    ('flat_q75', _flat, _check_flat),
]
NAMES = [c[0] for c in CASES]


def case(name, ri):
    _, build, check = CASES[NAMES.index(name)]
    planes, quality = build(ri)
    return planes, quality, check
