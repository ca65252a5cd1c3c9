"""
The frames tests/test_cpu_jpeg_opt.py and tests/test_gpu_jpeg_opt.py encode with optimised Huffman tables: every frame of
jpeg_cases.py (4:4:4) and jpeg420_cases.py (4:2:0), whose checks keep saying that the stream contains the edge the case is named
for (short last interval, RST wrap, stuffing, flat frames, DC extremes), and two of this module's own:

  deep_code   uniform noise at 512 x 512, quality 90: the rarest AC symbols sit so far below the commonest that Huffman's code
              for them passes 16 bits, so the limiter works.  The CPU test asserts that from the model, for both AC tables of
              both samplings (seed 15: 19, 20 in 4:4:4 and 19, 17 in 4:2:0, whose chrominance table counts a quarter of the blocks).
  one_mcu     a flat frame of one MCU (8 x 8 in 4:4:4, 16 x 16 in 4:2:0): a symbol is emitted once or twice or never, so all but
              a few sit at the floor frequency and the builder's ranking and merge meet little but ties; only the luminance DC
              table saves code bits here, so this is also a frame on which Annex K's tables are kept.
"""
import numpy as np

import jpeg420_cases
import jpeg_cases

S444, S420 = 0, 1
CASE_MODULE = {S444: jpeg_cases, S420: jpeg420_cases}
DEEP_CODE, ONE_MCU = 'deep_code', 'one_mcu'
DEEP_SEED, DEEP_QUALITY = 15, 90


def names(sampling):
    return CASE_MODULE[sampling].NAMES + [DEEP_CODE, ONE_MCU]


def _check_deep(st, ri):
    assert st['blocks'] in (3 * 64 * 64, 6 * 32 * 32) and st['stuffed'] >= 1 and len(st['rst']) > 8


def _check_one_mcu(st, ri):
    assert st['intervals'] == 1 and st['rst'] == [] and st['eob_only_blocks'] == st['blocks'] and st['blocks'] in (3, 6)


def case(name, ri, sampling):
    """-> (planes u8 [3][h][w], quality, check(stats, ri))."""
    if name == DEEP_CODE:
        return np.random.RandomState(DEEP_SEED).randint(0, 256, (3, 512, 512)).astype(np.uint8), DEEP_QUALITY, _check_deep
    if name == ONE_MCU:
        side = 16 if sampling == S420 else 8
        p = np.empty((3, side, side), np.uint8)
        p[0], p[1], p[2] = 31, 128, 140
        return p, 75, _check_one_mcu
    return CASE_MODULE[sampling].case(name, ri)
