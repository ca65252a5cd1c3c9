"""
The encoders' placement helper alone (csrc/encode_device.h: place_pieces and store_offsets, through fl_debug_place's
one-workgroup kernel) against numpy's exclusive cumulative sum in uint64, exactly.

The piece counts sit on both sides of every multiple of the workgroup's 1024 threads at which a thread's range grows by a piece
(1024 -> 1025, 2048 -> 2049), at ranges that leave the last threads empty (1, 2, 1023, 2047) and at one count far above them with a
ragged last range (100 003).  Every length set holds lengths near 2^32, so that the sums carry into the high word — inside a
thread's own range, across the workgroup's scan, and in `front` + the scan.
"""
import numpy as np
import pytest

from cuburn_amd import render, _lib

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 100003)
FRONTS = (0, 33)


@pytest.fixture(scope='module')
def mgr(built):
    return render.RenderManager(device=0, nslots=1024, host_seed=7)


def lengths(n):
    """Seeded: small lengths as an encoder's pieces have, every seventh within 2^16 of 2^32, the first and last the largest u32."""
    rng = np.random.RandomState(n)
    lens = rng.randint(0, 70000, n).astype(np.uint32)
    big = np.arange(n) % 7 == 3
    lens[big] = (2 ** 32 - 1 - rng.randint(0, 2 ** 16, int(big.sum()))).astype(np.uint32)
    lens[0] = lens[-1] = 2 ** 32 - 1
    return lens


@pytest.mark.parametrize('front', FRONTS)
@pytest.mark.parametrize('n', COUNTS)
def test_offsets_and_total_are_the_exclusive_cumsum(mgr, n, front):
    lens = lengths(n)
    offs = np.full(n, 0xA5A5A5A5A5A5A5A5, np.uint64)
    total = np.zeros(1, np.uint64)
    _lib.check(_lib.load().fl_debug_place(mgr.fb.ctx, lens.ctypes.data, n, front, offs.ctypes.data, total.ctypes.data))
    incl = np.cumsum(lens.astype(np.uint64), dtype=np.uint64)
    want = np.uint64(front) + np.concatenate([np.zeros(1, np.uint64), incl[:-1]])
    assert n == 1 or int(incl[-1]) >> 32, 'the case must carry into the high word'
    assert int(total[0]) == int(incl[-1])
    bad = np.flatnonzero(offs != want)
    assert bad.size == 0, (bad[:4], offs[bad[:4]], want[bad[:4]])
