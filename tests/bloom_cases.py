"""
Inputs and cases shared by tests/test_cpu_bloom.py and tests/test_gpu_bloom.py (numpy only).

The frame sizes are the smallest at which the two kernels of csrc/bloom.hip can go wrong: k_bloom_rows takes segments of 256
bins of a row, k_bloom_cols strips of 64 columns by 32 rows, fed in bands of 16 rows.
"""
import numpy as np

THRESHOLD = 1.0
STRENGTH = 0.25

# (frame size, sigma): R = ceil(3 sigma)
CASES = [
    ((40, 24), 16.0),       # padded 64 x 48, R = 48: every window crosses both edges in both axes
    ((70, 40), 5.0),        # astride 96 > aw 94: the last strip of columns is half empty; 64 rows
    ((200, 120), 0.0),      # 224 x 144: four strips by five tiles of rows; one tap
    ((200, 120), 1.0),
    ((200, 120), 5.0),
    ((200, 120), 20.0),
    ((90, 70), 128.0),      # R = 384, the limit: the window is far larger than the frame
    ((300, 20), 5.0),       # astride above 256: two segments per row, a seam inside the picture
    ((300, 20), 100.0),     # R = 300: a halo wider than a segment
]


def case_id(case):
    return '%dx%d-sigma%g' % (case[0] + (case[1],))


def gamma_buffer(ah, astride, seed=1, threshold=THRESHOLD):
    """(ah, astride, 4) float32, all values >= 0: gamma-distributed densities of which about 30 % lie above the threshold,
    colours a random share of the density; some bins with w = 0 (colour kept) and w = threshold exactly."""
    rs = np.random.RandomState(seed)
    w = rs.gamma(2.0, 1.0, (ah, astride))
    w *= threshold / np.percentile(w, 70.0)
    buf = np.zeros((ah, astride, 4), np.float32)
    buf[..., 3] = w
    buf[..., :3] = w[..., None] * rs.uniform(0.1, 1.5, (ah, astride, 3))
    zero = rs.uniform(size=(ah, astride)) < 0.03
    at = rs.uniform(size=(ah, astride)) < 0.03
    buf[zero, 3] = 0.0
    buf[at & ~zero, 3] = np.float32(threshold)
    return buf


def impulse_bins(ah, astride):
    """(y, x) of the single impulses: interior, on the seams of the tiles of both kernels, and the two far corners."""
    pts = [(ah // 2 + 3, astride // 2 + 5), (0, 0), (ah - 1, astride - 1)]
    pts += [(y, x) for y in (31, 32) for x in (63, 64) if y < ah and x < astride]
    pts += [(ah // 3, x) for x in (255, 256) if x < astride]
    return pts


def impulse_buffer(ah, astride, threshold=THRESHOLD):
    """Mostly empty: one bright bin at each of impulse_bins, a bin with w = 0 and one with w = threshold beside the first."""
    buf = np.zeros((ah, astride, 4), np.float32)
    for n, (y, x) in enumerate(impulse_bins(ah, astride)):
        buf[y, x] = (3.0 + n, 2.0, 0.5 * n, 4.0 + n)
    y, x = impulse_bins(ah, astride)[0]
    buf[y, x + 1] = (5.0, 6.0, 7.0, 0.0)
    buf[y + 1, x] = (5.0, 6.0, 7.0, threshold)
    return buf
