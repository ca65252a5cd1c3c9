"""
The frames tests/test_cpu_jpeg.py and tests/test_gpu_jpeg.py encode: the smallest shapes at which each part of the JPEG encoder
can go wrong.  A case is (name, build(ri) -> (planes u8 [3][h][w], quality), check(stats, ri)): `check` asserts, from the
statistics jpeg_model.parse gathered, that the stream contains what the case is named for, so that a case that stops exercising
its edge fails.  Sizes that depend on the restart interval `ri` (MCUs per interval) are built from it.
"""
import numpy as np

MODEL_RI = 8              # the interval the CPU tests use; the GPU tests take the device's from its record


def _noise(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (3, h, w)).astype(np.uint8)


def _size(w, h):
    def check(st, ri):
        assert st['blocks'] == 3 * ((w + 7) // 8) * ((h + 7) // 8)
    return check


def _short_last(ri):          # 2 ri + 1 MCUs in a row, the last column partial: three intervals, the last of one MCU
    return _noise(8 * (2 * ri + 1) - 3, 5, 5), 50


def _check_short_last(st, ri):
    assert st['intervals'] == 3 and st['rst'] == [0, 1]
    assert st['last_interval_mcus'] == 1 and (ri == 1 or st['last_interval_mcus'] < ri)


def _wrap(ri):                # 9 ri + 1 MCUs: ten intervals
    return _noise(8 * (9 * ri + 1), 8, 6), 50


def _check_wrap(st, ri):
    assert st['intervals'] == 10 and st['rst'] == [0, 1, 2, 3, 4, 5, 6, 7, 0], st['rst']


def _check_single(st, ri):
    assert st['intervals'] == 1 and st['rst'] == []


def _check_stuffed(st, ri):
    assert st['stuffed'] >= 1


def _flat(ri):
    p = np.empty((3, 16, 24), np.uint8)
    p[0], p[1], p[2] = 77, 128, 200
    return p, 75


def _check_flat(st, ri):
    assert st['eob_only_blocks'] == st['blocks'] == 18 and st['dc_zero_diffs'] >= 6


def _dc11(ri):                # blocks of 0 beside blocks of 255: DC -1024 next to 1016
    p = np.zeros((3, 8, 32), np.uint8)
    p[:, :, 8:16] = 255
    p[:, :, 24:32] = 255
    return p, 100


def _check_dc11(st, ri):
    assert ri >= 2 and st['dc_categories'][11] >= 1, st['dc_categories']


def _ac10(ri):                # left half 0, right half 255: the first horizontal frequency is about -924
    p = np.zeros((3, 8, 8), np.uint8)
    p[:, :, 4:] = 255
    return p, 100


def _check_ac10(st, ri):
    assert st['ac_categories'][10] >= 1, st['ac_categories']


def _basis77(ri):             # only the last zigzag position survives quality 50: 62 zeros in front of it
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    block = np.rint(128 + 100 * np.outer(c, c)).astype(np.uint8)
    return np.tile(block, (3, 1, 2)), 50


def _check_basis77(st, ri):
    assert st['max_zero_run'] == 62 and st['zrl'] == 3 * st['blocks'] and st['blocks_without_eob'] == st['blocks'] == 6
    assert st['eob'] == 0


NOISE_Q100 = 'noise_64x40_q100'
CASES = [
    ('noise_1x1_q50', lambda ri: (_noise(1, 1, 1), 50), _size(1, 1)),
    ('noise_8x8_q50', lambda ri: (_noise(8, 8, 2), 50), _check_single),
    ('noise_17x9_q1', lambda ri: (_noise(17, 9, 3), 1), _size(17, 9)),
    ('noise_250x37_q50', lambda ri: (_noise(250, 37, 4), 50), _size(250, 37)),
    ('short_last_interval', _short_last, _check_short_last),
    ('rst_wraps', _wrap, _check_wrap),
    (NOISE_Q100, lambda ri: (_noise(64, 40, 7), 100), _check_stuffed),
    ('flat_q75', _flat, _check_flat),
    ('dc_category_11', _dc11, _check_dc11),
    ('ac_category_10', _ac10, _check_ac10),
    ('basis_7_7_q50', _basis77, _check_basis77),
]
NAMES = [c[0] for c in CASES]


def case(name, ri):
    _, build, check = CASES[NAMES.index(name)]
    planes, quality = build(ri)
    return planes, quality, check
