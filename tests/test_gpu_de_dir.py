"""
The bilateral DE one direction at a time: k_de_dir (cuburn_amd/csrc/de.hip) through fl_debug_de_dir, in the instantiations the
chain uses, against the float64 model of tests/de_dir_model.py on the cases of tests/de_dir_cases.py (tests/test_cpu_de_dir.py is
their CPU side).  A failure names the direction, frame, pixel, its tile and the tile's kind.

  A  every direction, frame, input kind and parameter set against the model, in the direction's own output form: every finite
     model value obeys |x - m| <= B (|m| + 2^-10 M_c), M_c the channel's largest |m| in the frame; no share of outliers.
     B per class (direction family x input kind x parameter set) = max(4 e_oracle + T_pow, 4 * 2^-24): e_oracle is the float32
     oracle's own worst ratio against the model on the same inputs, 4 is test_gpu_interp.py's margin for hardware
     exp2 / rcp / log2 (1-2 ulp where libm is 0.5), T_pow = 2 ln2 |0.5 / dstd| max_w w^dpow (ln2 dpow |log2 w| + 1) 2^-22 is the
     density factor's sensitivity to the 2-ulp bars of v_log_f32 / v_exp_f32, derived, not measured.
     Every B is at most 1e-4 (asserted on the CPU side).  Measured on an MI355X, device worst ratio / B per class:
     horizontal 8.3e-7 / 3.1e-6 (dense, dpow 0) .. 5.9e-6 / 4.4e-5 (sparse, default); integer steps 1.4e-6 / 5.1e-6 ..
     4.2e-5 / 5.9e-5 (sparse, dpow 0; sparse, sstd 24: 3.9e-5 / 6.7e-5); half slopes 1.1e-6 / 4.2e-6 .. 1.1e-5 / 4.7e-5;
     lone bins 4.1e-7 / 1.6e-6.
  B  lone bins: nonzero exactly on the support the tap geometry gives (away from the edges the 31 pixels q - t(r)), exactly 0
     elsewhere, values at the bar of A; every wave has a dead centre, so this pins de_tap_loop_slow.
  C  a picture shifted through every column and row residue of the direction's tile: interior results equal bit for bit.
  D  the three tile orders give the same bits on every frame, and no NaN of the entry's prefill is left in the padded frame.
  E  direction 0 from the raw accumulator (in_mode 1) and from YUV (in_mode 2, with colours that clamp), direction 7 to raw pixels.
  F  what the entry refuses, and that a chain through fl_filter right after gives the bits it gave before.

The device's worst ratio of every class is printed beside its B (run with -s).
"""
import numpy as np
import pytest

import de_dir_cases as Cs
import de_dir_model as M
from cuburn_amd import _lib, render

pytestmark = pytest.mark.gpu

CLASSES = [(f, k, p) for f in Cs.FAMILIES for k in Cs.KINDS for p in Cs.PSETS]


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    m.fb.free()


def run_dir(mgr, size, buf, P, sc, in_mode=1, order=-1):
    """`buf` ((ah, astride, 4) float32) into the front buffer of a `size` frame, one direction, the front buffer back."""
    lib = _lib.load()
    w, h = size
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, w, h, 0))
    mgr.fb.write('front', buf)
    arr = np.asarray(sc, np.float32)
    _lib.check(lib.fl_debug_de_dir(mgr.fb.ctx, w, h, P, arr.ctypes.data, in_mode, order))
    return mgr.fb.read('front', buf.shape, np.float32)


def where(P, shape, y, x):
    """'pixel (x, y), tile (tx, ty) border|interior' for a failure message."""
    H, W = shape[:2]
    TW, TH = Cs.tile_shape(P)
    ty = y // TH
    tx = (x - Cs.shear(P, y - ty * TH) + (Cs.span(P) if Cs.K[P] > 0 else 0)) // TW
    return 'pixel (%d, %d) of %d x %d, tile (%d, %d) row %d of it, %s' % (
        x, y, W, H, tx, ty, y - ty * TH, 'border' if Cs.border(P, tx, ty, H, W) else 'interior')


def held(P, dev, want, B, what):
    """The bar of A on one result; returns the worst ratio."""
    q, i, ch = M.ratio(dev, want)
    y, x = divmod(i, want.shape[1]) if want.ndim == 3 else (0, i)
    assert q <= B, '%s: ratio %.3g > B %.3g at %s, channel %d: device %r, model %r' % (
        what, q, B, where(P, want.shape, y, x) if want.ndim == 3 else 'support pixel %d' % i, ch,
        dev.reshape(-1, 4)[i, ch], want.reshape(-1, 4)[i, ch])
    return q


@pytest.mark.parametrize('fam,kind,pset', CLASSES)
def test_direction_against_model(mgr, fam, kind, pset):
    """A: every direction of the family on every frame."""
    B, e, t = Cs.bound(fam, kind, pset)
    worst = 0.0
    for P in Cs.FAMILIES[fam]:
        for size in Cs.FRAMES:
            dev_in, want, _, _ = Cs.case_a(P, size, kind, pset)
            dev = run_dir(mgr, size, dev_in, P, Cs.scalars(pset, size))
            worst = max(worst, held(P, dev, want, B, 'direction %d, %d x %d, %s, %s' % ((P,) + size + (kind, pset))))
    print('%-10s %-6s %-10s device %.3g   B %.3g (e_oracle %.3g, T_pow %.3g)' % (fam, kind, pset, worst, B, e, t))


@pytest.mark.parametrize('P', range(8))
def test_lone_bins(mgr, P):
    """B: lone bins (0.3, 0.5, 0.2, 1.0) on every column and row of the direction's tile, on the corners and the edge midpoints
    of every frame, at sstd 24 and 6."""
    B, e, t = Cs.bound(Cs.family(P), 'lone', None)
    worst, nbins = 0.0, 0
    for size in Cs.FRAMES:
        for sstd in Cs.LONE_SSTD:
            for n, (dev_in, sup, want, pts) in enumerate(Cs.lone_case(P, size, sstd)[0]):
                what = 'direction %d, %d x %d, sstd %g, accumulator %d' % ((P,) + size + (sstd, n))
                dev = run_dir(mgr, size, dev_in, P, Cs.lone_scalars(sstd))
                off = np.argwhere((dev != 0).any(-1) & ~sup)          # (NaN != 0: an unwritten pixel shows here too)
                assert not len(off), '%s: %d nonzero pixels off the support, first %s = %r; bins (y, x) %r' % (
                    what, len(off), where(P, dev.shape, *off[0]), dev[tuple(off[0])], pts)
                ys, xs = np.nonzero(sup)
                got = dev[ys, xs]
                dead = np.flatnonzero((want[:, 3] > 1e-30) & ~(got[:, 3] > 0))
                assert not len(dead), '%s: no density at %s, model %r' % (what, where(P, dev.shape, ys[dead[0]], xs[dead[0]]), want[dead[0]])
                worst = max(worst, held(P, got, want, B, what))
                nbins += len(pts)
    print('direction %d: %d lone bins, device %.3g   B %.3g (e_oracle %.3g, T_pow %.3g)' % (P, nbins, worst, B, e, t))


@pytest.mark.parametrize('kind', Cs.KINDS)
@pytest.mark.parametrize('P', range(8))
def test_shifted_picture_is_bit_identical(mgr, P, kind):
    """C: the arithmetic of an interior pixel does not depend on which tile, wave, lane or row parity computes it."""
    sc = Cs.scalars('sstd24', Cs.SHIFT_FRAME)
    r0, r1, c0, c1 = Cs.SHIFT_RECT
    base = run_dir(mgr, Cs.SHIFT_FRAME, Cs.shift_input(P, kind, 0, 0), P, sc)
    assert np.isfinite(base).all() and (base[r0:r1, c0:c1, 3] > 0).mean() > 0.02
    for sx, sy in Cs.shifts(P):
        out = run_dir(mgr, Cs.SHIFT_FRAME, Cs.shift_input(P, kind, sx, sy), P, sc)
        a, b = base[r0:r1 - sy, c0:c1 - sx].view(np.uint32), out[r0 + sy:r1, c0 + sx:c1].view(np.uint32)
        diff = np.argwhere((a != b).any(-1))
        assert not len(diff), 'direction %d, %s, shift (%d, %d): %d pixels differ, first at %s: %r against %r unshifted at %s' % (
            P, kind, sx, sy, len(diff), where(P, out.shape, r0 + sy + diff[0][0], c0 + sx + diff[0][1]),
            out[r0 + sy + diff[0][0], c0 + sx + diff[0][1]], base[r0 + diff[0][0], c0 + diff[0][1]],
            where(P, out.shape, r0 + diff[0][0], c0 + diff[0][1]))


@pytest.mark.parametrize('P', range(8))
def test_tile_orders_are_bit_identical(mgr, P):
    """D: orders 0, 1, 2 and the table's own give the same bits on every frame and input kind; the padded frame holds no NaN."""
    for size in Cs.FRAMES:
        for kind in Cs.KINDS:
            dev_in = Cs.case_a(P, size, kind, 'sstd24')[0]
            sc = Cs.scalars('sstd24', size)
            outs = [run_dir(mgr, size, dev_in, P, sc, order=o) for o in (0, 1, 2, -1)]
            for o, out in zip((0, 1, 2, -1), outs):
                bad = np.argwhere(~np.isfinite(out).all(-1))
                assert not len(bad), 'direction %d, %d x %d, %s, order %d: %d pixels not written or not finite, first %s' % (
                    (P,) + size + (kind, o, len(bad), where(P, out.shape, *bad[0])))
                diff = np.argwhere((out.view(np.uint32) != outs[0].view(np.uint32)).any(-1))
                assert not len(diff), 'direction %d, %d x %d, %s: order %d differs from order 0 at %d pixels, first %s' % (
                    (P,) + size + (kind, o, len(diff), where(P, out.shape, *diff[0])))


@pytest.mark.parametrize('kind', Cs.KINDS)
@pytest.mark.parametrize('size', [(33, 17), (200, 120)])
def test_first_and_last_direction_forms(mgr, size, kind):
    """E: direction 0 normalises the raw accumulator (in_mode 1) or yuv_to_rgb of it (in_mode 2, with colours that clamp at 0)
    as it stages it; direction 7 returns raw pixels."""
    for pset in ('default', 'sstd24'):
        sc = Cs.scalars(pset, size)
        what = '%d x %d, %s, %s' % (size + (kind, pset))
        for P, in_mode in ((0, 1), (0, 2), (7, 1)):
            B = Cs.bound(Cs.family(P), kind, pset)[0]
            dev_in, want, e, _ = Cs.case_a(P, size, kind, pset, in_mode)
            assert 4 * e <= B
            dev = run_dir(mgr, size, dev_in, P, sc, in_mode)
            q = held(P, dev, want, B, 'direction %d in_mode %d, %s' % (P, in_mode, what))
            print('direction %d in_mode %d, %s: device %.3g   B %.3g' % (P, in_mode, what, q, B))
            if in_mode == 2:                    # the same buffer read as RGB is another picture
                assert M.ratio(run_dir(mgr, size, dev_in, 0, sc, 1), want)[0] > 100 * B
            if P == 7:                          # raw, not normalised
                assert M.ratio(dev, M.to_normalised(want))[0] > 100 * B


def test_refusals_leave_the_context_usable(mgr):
    """F: bad patterns, orders and in_mode are refused with FL_E_INVAL and queue nothing: the chain through fl_filter right after
    gives the bits it gave before, and so does a direction."""
    lib = _lib.load()
    size = (200, 120)
    sc = np.asarray(Cs.scalars('default', size), np.float32)
    raw = Cs.accumulator('dense', size)

    def chain():
        _lib.check(lib.fl_debug_clear(mgr.fb.ctx, size[0], size[1], 0))
        mgr.fb.write('front', raw)
        _lib.check(lib.fl_filter(mgr.fb.ctx, _lib.FILT['bilateral'], size[0], size[1], sc.ctypes.data, 5))
        return mgr.fb.read('front', raw.shape, np.float32)
    before = chain()
    one = run_dir(mgr, size, raw, 0, sc, 2, 1)
    for P, in_mode, order in ((-1, 1, -1), (8, 1, -1), (1 << 20, 1, 0), (0, 0, -1), (0, 3, -1), (0, -1, 2), (3, 1, -2), (3, 1, 3), (7, 1, 77)):
        rc = lib.fl_debug_de_dir(mgr.fb.ctx, size[0], size[1], P, sc.ctypes.data, in_mode, order)
        assert rc == _lib.FL_E_INVAL, (P, in_mode, order, rc)
        with pytest.raises(ValueError):
            _lib.check(rc)
    assert lib.fl_debug_de_dir(mgr.fb.ctx, size[0], size[1], 0, None, 1, -1) == _lib.FL_E_INVAL
    assert lib.fl_debug_de_dir(None, size[0], size[1], 0, sc.ctypes.data, 1, -1) == _lib.FL_E_INVAL
    after = chain()
    assert np.isfinite(before).all() and np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert np.array_equal(run_dir(mgr, size, raw, 0, sc, 2, 1).view(np.uint32), one.view(np.uint32))
    # in_mode is ignored by directions 1..7; a deferred `yuv` in front of the entry runs first
    n = Cs.case_a(3, size, 'dense', 'default')[0]
    assert np.array_equal(run_dir(mgr, size, n, 3, sc, 77).view(np.uint32), run_dir(mgr, size, n, 3, sc, 1).view(np.uint32))
