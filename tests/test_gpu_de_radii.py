"""
The `de` filter's kernel (cuburn_amd/csrc/de_adaptive.hip) at every quantised radius, tile edge and frame
size, through the public ABI (fl_debug_clear, Framebuffers.write, fl_filter(FL_FILT_DE), read) against the float64 forms
of tests/de_model.py:

  * lone bins of every 16 h = 16 .. 1536, and bins that stay, at every kind of position within a 64 x 16 tile;
  * lone bins on the padded edges of the 200 x 120, 1080p and 4K accumulators (gutter, half-width last tile column);
  * the reach of a 64 x 16 output tile over its 5 x 13 neighbourhood, at the smallest reaching radius and one below;
  * the rounding of h to 1/16 in double, on densities within 1e-5 of a rounding half;
  * cfg2 frames at 1080p and 4K against the gather form de_gather_at;
  * scratch reuse across frame sizes and other filters, and `de` after `yuv`.

Lone-bin bound, LONE_RTOL = 2e-6.  For one source the kernel writes fma(c * sinv[m], 2^e, 0): sinv is the double 1 / S
rounded to float (2^-24 relative), c * sinv is rounded (2^-24), and so is the fma into the zero accumulator (2^-24).  The
exponent e = fma(a, dy^2, t), t = a dx^2, a = kA / m^2: kA is rounded from double and the quotient once more (2^-24 of e
each), t and e are rounded once each (2^-24 |e| at most); inside the cut |e| <= 6.5, so e is off by at most
4 * 2^-24 * 6.5 = 1.55e-6 and 2^e by 1.55e-6 ln 2 = 1.07e-6 relative; v_exp_f32 adds 1 ulp (2^-23 = 1.2e-7).  Total
1.07e-6 + 1.2e-7 + 3 * 6e-8 = 1.37e-6 < 2e-6, per pixel and so for a disc's sum.  The bound is derived; the tests print
the worst error they measure.
"""
import ctypes as C
import math

import numpy as np
import pytest

from common import O, frame_times
from de_model import de_filter, de_gather_at, disc_weights, near_half_densities, radii16
from accum_inputs import fractional_band_accum as accum, synth_accum
from cuburn_amd import _lib, configs, filters, profile, render

pytestmark = pytest.mark.gpu

TW, TH = 64, 16                                     # k_de_gather's output tile
XRES, YRES = (0, 1, 31, 62, 63), (0, 1, 7, 14, 15)  # where within its tile a lone bin sits: column, row
LONE = (96.0, 0.0, 1.0)                             # R, Rmin, curve: 16 h = 1536 / max(w, 1)
BIG = (4072, 2024)                                  # the frame of a 4096 x 2048 accumulator
LONE_RTOL = 2e-6
BAR = 2e-5                                          # whole frames: 2e-5 |ref| + 1e-6 max |ref| (test_gpu_de_adaptive)


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    m.fb.free()


def padded(size):
    dim = render.Framebuffers.calc_dim(*size)
    return dim.ah, dim.astride


def run_filters(mgr, size, buf, chain):
    """Write `buf` ((ah, astride, 4) float32) to the front buffer of a `size` frame, run the [(name, scalars)] chain
    through fl_filter and read the front buffer back."""
    lib = _lib.load()
    w, h = size
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, w, h, 0))
    mgr.fb.write('front', buf)
    for name, vals in chain:
        arr = np.asarray(vals, np.float32)
        _lib.check(lib.fl_filter(mgr.fb.ctx, _lib.FILT[name], w, h, arr.ctypes.data, len(arr)))
    return mgr.fb.read('front', buf.shape, np.float32)


def run_de(mgr, size, buf, vals):
    return run_filters(mgr, size, buf, [('de', vals)])


def lone_density(m, frac=0.0):
    """A float32 density whose 16 h under LONE is m + frac, |frac| <= 0.35, so at least 0.1 from a rounding half (m = 1536:
    a density in (0, 1))."""
    w = np.float32(0.5) if m == 1536 else np.float32(1536.0 / (m + frac))
    s = 1536.0 / max(float(w), 1.0)
    assert int(radii16(w, *LONE)) == m and abs(s - math.floor(s) - 0.5) >= 0.1, (m, frac)
    return w


def expected(m, col):
    """The float64 output of one lone bin over its box [-I, I]^2, I = m // 16 (a bin that stays: itself)."""
    col = np.asarray(col, np.float64)
    return col.reshape(1, 1, 4) if m < 16 else disc_weights(m)[..., None] * col


def fitted_m(dev, y, x, col, m):
    """Which of m - 1, m, m + 1 the device's spread of the lone bin at (y, x) is closest to (for failure messages)."""
    I = (m + 1) // 16
    got = dev[max(y - I, 0):y + I + 1, max(x - I, 0):x + I + 1].astype(np.float64)
    oy, ox = y - max(y - I, 0), x - max(x - I, 0)

    def err(k):
        ref = np.zeros((2 * I + 1, 2 * I + 1, 4))
        J = k // 16
        ref[I - J:I + J + 1, I - J:I + J + 1] = expected(k, col)
        return np.abs(got - ref[I - oy:I - oy + got.shape[0], I - ox:I - ox + got.shape[1]]).max()
    return min((m - 1, m, m + 1), key=err)


def check_bins(dev, placed, rtol=LONE_RTOL):
    """placed: [(m, y, x, colour)] of lone bins with disjoint boxes.  Each box (clipped to the buffer) against `expected`:
    disc pixels to rtol, pixels outside the disc exactly 0, a bin that stays to the bit; each spreading bin's kept sum
    against the model's to rtol in all four channels.  Returns (failures, worst relative error, nonzero values outside
    every box)."""
    H, W = dev.shape[:2]
    mask = np.zeros((H, W), bool)
    bad, worst = [], 0.0
    for m, y, x, col in placed:
        I = m // 16
        y0, y1, x0, x1 = max(y - I, 0), min(y + I + 1, H), max(x - I, 0), min(x + I + 1, W)
        assert not mask[y0:y1, x0:x1].any(), 'boxes overlap'
        mask[y0:y1, x0:x1] = True
        if m < 16:
            if not np.array_equal(dev[y, x].view(np.uint32), np.asarray(col, np.float32).view(np.uint32)):
                bad.append((m, y, x, 'moved'))
            continue
        got = dev[y0:y1, x0:x1].astype(np.float64)
        ref = expected(m, col)[y0 - (y - I):y1 - (y - I), x0 - (x - I):x1 - (x - I)]
        disc = ref != 0
        rel = (np.abs(got - ref)[disc] / np.abs(ref[disc])).max()
        srel = (np.abs(got.sum((0, 1)) - ref.sum((0, 1))) / np.abs(ref.sum((0, 1)))).max()
        worst = max(worst, rel, srel)
        if rel > rtol or srel > rtol or (got[~disc] != 0).any():
            bad.append((m, y, x, float(rel), float(srel), int((got[~disc] != 0).sum()), fitted_m(dev, y, x, col, m)))
    return bad, worst, int(np.count_nonzero(dev[~mask]))


def lay_out(bins, size):
    """bins: [(m, colour)] -> accumulators of a `size` frame holding them as lone bins: boxes [-I, I]^2 shelf-packed,
    largest first, the centres cycling over the columns XRES x rows YRES of their tiles.  Returns [(buf, placed)]."""
    H, W = padded(size)
    frames = []
    y0, shelf, cur = H, 0, W
    for n, k in enumerate(sorted(range(len(bins)), key=lambda k: -bins[k][0])):
        m, col = bins[k]
        I = m // 16
        xr, yr = XRES[n % 5], YRES[n // 5 % 5]
        cx = cur + I + (xr - cur - I) % TW
        if cx + I >= W:                              # a new shelf: its tallest (first) box + room to align the rows
            y0, shelf, cur = y0 + shelf, 2 * I + TH, 0
            if y0 + shelf > H:
                y0 = 0
                frames.append((np.zeros((H, W, 4), np.float32), []))
            cx = I + (xr - I) % TW
        cy = y0 + I + (yr - y0 - I) % TH
        assert cy + I < H and cx + I < W
        frames[-1][0][cy, cx] = col
        frames[-1][1].append((m, cy, cx, col))
        cur = cx + I + 1
    return frames


def colour(rs, w):
    return np.append(rs.uniform(1, 1e3, 3), w).astype(np.float32)


def test_de_every_radius_as_lone_bins(mgr):
    """Every quantised radius 16 h = 16 .. 1536 as a lone bin (R = 96, Rmin = 0, curve = 1; 16 h at least 0.1 from a
    rounding half), and bins that stay (w = 0, w < 0, 16 h < 15.5), at every combination of the tile columns XRES and tile
    rows YRES: each disc pixel against the model to LONE_RTOL (module docstring), every other pixel exactly 0, each disc's
    sum equal to the bin's input to LONE_RTOL in all four channels.  One wrong entry of the normaliser table, a disc one
    offset too wide or too narrow, or an m off by one fails here."""
    rs = np.random.RandomState(5)
    bins = [(m, colour(rs, lone_density(m, (-0.35, 0.0, 0.35)[m % 3]))) for m in range(16, 1537)]
    stay = [np.float32(v) for v in (0.0, -1.0, 1536 / 15.3, 1e3, 1e6)]
    for w in stay:
        m = int(radii16(w, *LONE))
        assert m < 16
        bins.append((m, colour(rs, w)))
    frames = lay_out(bins, BIG)
    placed, failures, worst = [], [], 0.0
    for buf, pl in frames:
        dev = run_de(mgr, BIG, buf, LONE)
        bad, wst, n_out = check_bins(dev, pl)
        assert n_out == 0, '%d nonzero values outside every disc' % n_out
        failures += bad
        worst = max(worst, wst)
        placed += pl
    radii = sorted({m for m, *_ in placed if m >= 16})
    spots = {(x % TW, y % TH) for _, y, x, _ in placed}
    print('lone bins: %d spreading radii (%d..%d), %d bins, %d that stay, %d tile positions, %d accumulators of %d x %d; '
          'worst relative error %.3g' % (len(radii), radii[0], radii[-1], len(placed), len(stay), len(spots), len(frames),
                                         padded(BIG)[1], padded(BIG)[0], worst))
    assert radii == list(range(16, 1537)) and len(spots) == 25
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize('size', [(200, 120), (1920, 1080), (3840, 2160)])
def test_de_lone_bins_on_padded_edges(mgr, size):
    """Lone bins on the corners and edges of the padded accumulator, inside its 12-pixel gutter, in the first column of
    the half-width last tile column (astride is an odd multiple of 32 at these widths) and in the last column before it:
    the weight that falls outside the accumulator is dropped exactly as the model drops it, the rest matches the model to
    LONE_RTOL, and nothing else changes."""
    H, W = padded(size)
    assert W % TW == TW // 2
    big, mid = (400, 160) if H < 400 else (1536, 800)
    spots = [(0, 0, big), (0, W - 1, big), (H - 1, 0, big), (H - 1, W - 1, big),
             (0, W // 2, mid), (H - 1, W // 2, mid), (H // 2, 0, mid), (H // 2, W - 1, mid),
             (H // 4, W - 32, 48), (3 * H // 4, W - 33, 48),
             (5, W // 4, 32), (H - 6, 3 * W // 4, 32), (H // 4, 5, 32), (3 * H // 4, W - 8, 32)]
    rs = np.random.RandomState(size[0])
    buf = np.zeros((H, W, 4), np.float32)
    placed = []
    for y, x, m in spots:
        buf[y, x] = col = colour(rs, lone_density(m))
        placed.append((m, y, x, col))
    bad, worst, n_out = check_bins(run_de(mgr, size, buf, LONE), placed)
    print('edges %dx%d: %d lone bins, worst relative error %.3g' % (W, H, len(placed), worst))
    assert n_out == 0 and not bad, (n_out, bad)


REACH = (300, 184)             # 352 x 208 bins: 5.5 x 13 tiles, tile (2, 6) has its whole 5 x 13 neighbourhood
PYTHAGOREAN = [(3, 4), (5, 12), (8, 15), (20, 21), (12, 35), (33, 56), (60, 63), (0, 96)]


def test_de_tile_reach_at_its_boundary(mgr):
    """k_de_gather leaves a 64 x 16 output tile untouched unless a tile of its 5 x 13 neighbourhood (rx = 2, ry = 6)
    holds a bin whose disc covers the gap between the two tiles' nearest bins, gx = 64 |ox| - 63, gy = 16 |oy| - 15.

    For every offset (ox, oy) != (0, 0) around tile (2, 6): one bin at the corner of tile (2 + ox, 6 + oy) nearest to it,
    at the smallest m with m^2 >= 256 (gx^2 + gy^2).  The nearest pixel of tile (2, 6) receives the model's non-zero
    value; at m - 1 the tile is not touched at all.  It holds -0.0 there, which a gathered tile would turn into +0.0 (its
    sums start from +0), so bit equality shows that the tile was skipped.  Where the gap is beyond 96 px, (+-2, +-6), no
    radius reaches, and m = 1536 leaves the tile bit-identical.  Then exact-edge Pythagorean offsets (dx, dy) from the
    tile's corners, m = 16 sqrt(dx^2 + dy^2): the corner pixel is reached at m and exactly 0 at m - 1."""
    H, W = padded(REACH)
    tx0, ty0 = 2 * TW, 6 * TH
    tile = (slice(ty0, ty0 + TH), slice(tx0, tx0 + TW))
    rgb = np.float32([300.0, 200.0, 100.0])

    def run(src, m, fill):
        buf = np.zeros((H, W, 4), np.float32)
        buf[tile] = fill
        buf[src] = np.append(rgb, lone_density(m))
        dev = run_de(mgr, REACH, buf, LONE)
        ref = de_filter(buf, *LONE)
        err = np.abs(dev - ref) - LONE_RTOL * np.abs(ref)
        assert not (err > 0).any(), (src, m, int((err > 0).sum()))
        return buf, dev

    def untouched(buf, dev):
        return np.array_equal(dev[tile].view(np.uint32), buf[tile].view(np.uint32))

    reached, unreachable = [], []
    for oy in range(-6, 7):
        for ox in range(-2, 3):
            if ox == oy == 0:
                continue
            sx, sy = tx0 + TW * ox + (TW - 1 if ox < 0 else 0), ty0 + TH * oy + (TH - 1 if oy < 0 else 0)
            px, py = tx0 + (TW - 1 if ox > 0 else 0), ty0 + (TH - 1 if oy > 0 else 0)
            gx, gy = abs(sx - px), abs(sy - py)
            assert (gx, gy) == (TW * abs(ox) - TW + 1 if ox else 0, TH * abs(oy) - TH + 1 if oy else 0)
            m = max(16, math.isqrt(256 * (gx * gx + gy * gy) - 1) + 1)
            if m > 1536:
                assert untouched(*run((sy, sx), 1536, -0.0)), (ox, oy)
                unreachable.append((ox, oy))
                continue
            _, dev = run((sy, sx), m, -0.0)
            assert (dev[py, px] > 0).all(), (ox, oy, m)
            assert untouched(*run((sy, sx), m - 1, -0.0)), (ox, oy, m - 1)
            reached.append((ox, oy, m))
    edges = 0
    for dx, dy in PYTHAGOREAN:
        m = 16 * math.isqrt(dx * dx + dy * dy)
        assert 256 * (dx * dx + dy * dy) == m * m
        for s, (py, px) in ((1, (ty0 + TH - 1, tx0 + TW - 1)), (-1, (ty0, tx0))):
            src = (py + s * dy, px + s * dx)
            assert (run(src, m, 0.0)[1][py, px] > 0).all(), (dx, dy, m)
            assert (run(src, m - 1, 0.0)[1][py, px] == 0).all(), (dx, dy, m - 1)
            edges += 1
    print('tile reach: %d neighbour offsets (%d reached, m %d..%d; %d beyond 96 px), %d exact-edge cases' % (
        len(reached) + len(unreachable), len(reached), min(r[2] for r in reached), max(r[2] for r in reached),
        len(unreachable), edges))
    assert len(reached) + len(unreachable) == 64 and sorted(unreachable) == [(-2, -6), (-2, 6), (2, -6), (2, 6)]
    assert {(ox, m) for ox, oy, m in reached if oy == 0 and abs(ox) == 2} == {(-2, 1040), (2, 1040)}
    assert {(oy, m) for ox, oy, m in reached if ox == 0 and abs(oy) == 6} == {(-6, 1296), (6, 1296)}


@pytest.mark.parametrize('curve', [1.0, 0.6])
def test_de_rounds_h_in_double(mgr, curve):
    """Densities whose 16 h, in float64, lies within 1e-5 of a rounding half, on both sides but no closer than 1e-9
    (de_model.near_half_densities): the device picks the m of radii16, which rounds h computed in double.  Each bin's m
    is identified from its spread: the weights at a disc's edge move by about 1 % per unit of m, far beyond LONE_RTOL.
    A float32 pow would pick the other m for about 30 % of them (test_cpu_de_adaptive)."""
    vals = (96.0, 0.0, curve)
    w, below = near_half_densities(96.0, curve)
    rs = np.random.RandomState(int(10 * curve))
    pick = np.concatenate([rs.choice(np.flatnonzero(side), min(150, side.sum()), replace=False)
                           for side in (below, ~below)])
    ms = radii16(w[pick], *vals)
    frames = lay_out([(int(m), colour(rs, x)) for m, x in zip(ms, w[pick])], BIG)
    wrong = []
    for buf, placed in frames:
        bad, _, n_out = check_bins(run_de(mgr, BIG, buf, vals), placed)
        assert n_out == 0
        wrong += bad
    print('rounding, curve %g: %d densities within 1e-5 of a half (%d below, %d above), m %d..%d' % (
        curve, len(pick), below[pick].sum(), (~below[pick]).sum(), ms.min(), ms.max()))
    assert not wrong, (len(wrong), wrong[:8])


def cfg2_accumulator(size, samples, seed=7):
    """A cfg2 accumulator of `samples` at `size` after `yuv` (what `de` sees in its chain), the manager that holds it and
    the default `de` scalars."""
    lib = _lib.load()
    gnm, prof = configs.cfg2(samples=samples)
    gprof = profile.wrap(dict(prof, width=size[0], height=size[1], filter_order=['de']), gnm)
    m = render.RenderManager(device=0, host_seed=seed)
    rdr = render.Renderer(gnm, gprof)
    tc = 0.5
    dim = m.fb.set_dim(*size, nsamples=samples)
    ts, td = frame_times(gprof, tc)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(m.fb.ctx, C.byref(fid)))
    m._copy(rdr, gnm)
    g = rdr._handle(m.fb)
    _lib.check(lib.fl_interp(m.fb.ctx, g, dim.w, dim.h, ts, td))
    run = C.c_uint64()
    _lib.check(lib.fl_iterate(m.fb.ctx, g, dim.w, dim.h, float(samples), m.fuse, m.resolve_accum_mode(dim), C.byref(run)))
    none = np.zeros(0, np.float32)
    _lib.check(lib.fl_filter(m.fb.ctx, _lib.FILT['yuv'], dim.w, dim.h, none.ctypes.data, 0))
    acc = m.fb.read('front', (dim.ah, dim.astride, 4), np.float32)
    return m, acc, filters.DensityEstimation().scalars(gprof, gprof.filters.de, dim, tc)


def sample_points(acc, vals, nrand, seed):
    """Every pixel of the first and last tile rows, of the half-width last tile column and of four interior tiles whose
    largest radius differs most from a neighbour's, and nrand random pixels: (N, 2) of (y, x)."""
    H, W = acc.shape[:2]
    ntx, nty = (W + TW - 1) // TW, H // TH
    m = np.zeros((H, ntx * TW), np.int64)
    m[:, :W] = radii16(acc[..., 3], *vals)
    t = m.reshape(nty, TH, ntx, TW).max((1, 3))
    c = t[1:-1, 1:-1]
    d = np.zeros_like(t)
    d[1:-1, 1:-1] = np.max([np.abs(c - t[:-2, 1:-1]), np.abs(c - t[2:, 1:-1]), np.abs(c - t[1:-1, :-2]),
                            np.abs(c - t[1:-1, 2:])], 0)
    inner = np.argsort(d.ravel(), kind='stable')[::-1][:4]
    assert (d.ravel()[inner] > 0).all()
    sel = np.zeros((H, W), bool)
    sel[:TH] = sel[-TH:] = True
    sel[:, (ntx - 1) * TW:] = True
    for k in inner:
        ty, tx = divmod(int(k), ntx)
        sel[ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW] = True
    rs = np.random.RandomState(seed)
    sel[rs.randint(0, H, nrand), rs.randint(0, W, nrand)] = True
    return np.argwhere(sel)


@pytest.mark.parametrize('size,samples', [((1920, 1080), 2 ** 24), ((1920, 1080), 2 ** 28), ((3840, 2160), 2 ** 26)])
def test_de_real_frames_match_gather_form(built, size, samples):
    """cfg2's post-`yuv` accumulator at full size (2^24 samples: sparse, nearly every bin spreads) through `de` with the
    default scalars (R = 11 at 1080p, 22 at 4K), against de_gather_at at the pixels of sample_points, within the
    whole-frame bar; and the energy of a copy whose 96-pixel border is zeroed is conserved."""
    mgr, acc, vals = cfg2_accumulator(size, samples)
    try:
        dev = run_de(mgr, size, acc, vals)
        zacc = acc.copy()
        zacc[:96] = zacc[-96:] = zacc[:, :96] = zacc[:, -96:] = 0
        zdev = run_de(mgr, size, zacc, vals)
    finally:
        mgr.fb.free()
    assert vals[0] == np.float32(11.0 * size[0] / 1920)
    live = acc[..., 3] > 0
    pts = sample_points(acc, vals, 16384, samples % 997)
    ref = de_gather_at(acc, *vals, pts)
    got = dev[pts[:, 0], pts[:, 1]].astype(np.float64)
    print('%dx%d, 2^%d samples: %.3f of the bins with density spread, %d pixels sampled' % (
        size[0], size[1], int(math.log2(samples)), (radii16(acc[..., 3], *vals)[live] >= 16).mean(), len(pts)))
    assert np.isfinite(got).all()
    for ch in range(4):
        err = np.abs(got[:, ch] - ref[:, ch]) - (BAR * np.abs(ref[:, ch]) + 1e-6 * np.abs(ref[:, ch]).max())
        assert not (err > 0).any(), (ch, int((err > 0).sum()), pts[np.argmax(err)], got[np.argmax(err), ch],
                                     ref[np.argmax(err), ch])
    s0, s1 = zacc.astype(np.float64).sum((0, 1)), zdev.astype(np.float64).sum((0, 1))
    assert (np.abs(s1 - s0) <= 1e-5 * np.abs(zacc.astype(np.float64)).sum((0, 1))).all(), (s0, s1)


OTHERS = [('yuv', []), ('bilateral', [6.0 * 3840 / 1920., 0.05, 1.5, 0.8, 4.0]), ('logscale', [4.1875, 0.002]),
          ('colorclip', [1.0, -1.0, 0.25, 0.01, 0.01 ** (0.25 - 1)])]
REUSE = [((3840, 2160), (22.0, 0.0, 0.6)), ((200, 120), (23.0, 2.3, 1.0)), ((1920, 1080), (11.0, 0.0, 0.6))]


def test_de_scratch_reuse_is_bit_identical(built):
    """`de` stages its sources in d_back / d_blur and its tile maxima in d_de_tmax: grow-only scratch that the other
    filters share.  In one context, `de` at 4K, at 200 x 120 and at 1080p, then again in the reverse order after a
    bilateral chain, a smearclip and a haloclip at 4K (which write d_back, d_side and d_blur): every result is
    bit-identical to `de` in a fresh context."""
    inputs = {size: accum(render.Framebuffers.calc_dim(*size), seed=5) for size, _ in REUSE}
    fresh = {}
    for size, vals in REUSE:
        m = render.RenderManager(device=0, nslots=1024, host_seed=1)
        try:
            fresh[size] = run_de(m, size, inputs[size], vals)
        finally:
            m.fb.free()
    big = REUSE[0][0]
    m = render.RenderManager(device=0, nslots=1024, host_seed=1)
    try:
        got = [(size, run_de(m, size, inputs[size], vals)) for size, vals in REUSE]
        run_filters(m, big, inputs[big], OTHERS)
        run_filters(m, big, inputs[big], [('smearclip', [0.7, 0.25 - 1, 0.01, 0.01 ** (0.25 - 1)])])
        run_filters(m, big, inputs[big], [('haloclip', [0.25 - 1])])
        got += [(size, run_de(m, size, inputs[size], vals)) for size, vals in REUSE[::-1]]
    finally:
        m.fb.free()
    for size, g in got:
        assert np.array_equal(g.view(np.uint32), fresh[size].view(np.uint32)), size
        assert not np.array_equal(g, inputs[size])


def test_de_after_yuv_matches_oracle_then_model(mgr):
    """['yuv', 'de'] through fl_filter (`yuv` is deferred; `de` runs it first) against the oracle's yuv_to_rgb followed by
    de_gather_at at every pixel, within the whole-frame bar; the model applied to the buffer before `yuv` is not."""
    size, vals = (200, 120), (9.0, 0.9, 0.6)
    H, W = padded(size)
    buf = synth_accum(render.Framebuffers.calc_dim(*size), 6).reshape(H, W, 4)
    got = run_filters(mgr, size, buf, [('yuv', []), ('de', vals)]).reshape(-1, 4).astype(np.float64)
    rgb = O.yuv_to_rgb(O.calc_dim(*size), buf.reshape(-1, 4)).reshape(H, W, 4)
    pts = np.argwhere(np.ones((H, W), bool))

    def within(ref):
        return np.abs(got - ref) <= BAR * np.abs(ref) + 1e-6 * np.abs(ref).max(0)
    assert np.isfinite(got).all()
    assert within(de_gather_at(rgb, *vals, pts)).all()
    assert not within(de_gather_at(buf, *vals, pts)).all()
