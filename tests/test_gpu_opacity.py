"""
Xform opacity on the device (include/flame_hip.h (5) words 14 / 15, (6) FL_OP_OPACITY), through the C ABI.

The CPU oracle knows nothing of opacity.  The tests rest on the "three boxes" flame of tests/flames.py instead: the
images of its three xforms are disjoint, so a plotted sample lies in box k exactly when xform k produced it, and what an
opacity must do to each box is known in closed form; exact identities (opacity 1 == no key, opacity 0 == the keyless render
minus one box, every kernel form == every other) anchor the new code to everything the oracle already pins.
"""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from common import O, prepare, frame_times
from cuburn_amd import configs, profile, render, _lib
from cuburn_amd.genome.use import SplineEval
from cuburn_amd.packer import GenomePacker, OP_CONST, OP_OPACITY
from flames import (three_boxes, with_opacity, plot_probability, BOX_TOP, BOX_LOW_LEFT, BOX_LOW_RIGHT, BOX_WEIGHTS)
import gpu_harness as H
from gpu_harness import same_bits, setup_frame

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSE = 256
N26 = 2 ** 26


@pytest.fixture(scope='module')
def mgr(built):
    return render.RenderManager(device=0, nslots=1024, host_seed=42)


def _as_pinned_here(r, *drop):
    """A harness launch reduced to what these tests hold: three point words (the fourth belongs to the chaos tests)."""
    return dict(((k, v) for k, v in r.items() if k not in ('params', 'prog') + drop), pts=r['pts'][:, :3].copy())


def launch(*a, **kw):
    return _as_pinned_here(H.launch(*a, **kw))


def snapshot(*a, **kw):
    return _as_pinned_here(H.snapshot(*a, **kw), 'rdr', 'g')


def box(front, dim, rect, chan=3):
    r0, r1, c0, c1 = rect
    return front[:, chan].reshape(dim)[r0:r1 + 1, c0:c1 + 1].astype(np.float64)


def box_order(front, dim):
    """Rectangles of xforms 0, 1, 2 — which lower box is xform 0 is read off the keyless render's masses (0.5 against 0.3)."""
    left, right = box(front, dim, BOX_LOW_LEFT).sum(), box(front, dim, BOX_LOW_RIGHT).sum()
    tot = front[:, 3].astype(np.float64).sum()
    assert abs(max(left, right) / tot - 0.5) < 0.01 and abs(min(left, right) / tot - 0.3) < 0.01
    assert abs(box(front, dim, BOX_TOP).sum() / tot - 0.2) < 0.01
    return (BOX_LOW_LEFT, BOX_LOW_RIGHT, BOX_TOP) if left > right else (BOX_LOW_RIGHT, BOX_LOW_LEFT, BOX_TOP)


def mag_spline64(value, t, scale=1.0):
    """A magnitude-domain spline of the genome in float64: the packer's knots (SplineEval.normalize) through the device's
    Catmull-Rom in the lin-log domain (csrc/interp.hip catmull_rom, cuburn/code/interp.py:299-355).  SplineEval's own
    __call__ is linear-domain whatever the spline (as in the reference), which is not what the device evaluates for a
    magnitude spline such as `opacity` between its knots."""
    kt, kv = SplineEval.normalize(value, scale)
    n = kt.size
    times = np.full(32, 1e9)
    knots = np.zeros(32)
    times[:n], knots[:n] = np.float32(kt), np.float32(kv)
    idx = max(int(np.searchsorted(times, t, side='left')) - 1, 1)
    t1, t2 = times[idx], times[idx + 1] - times[idx]
    t0, t3 = (times[idx - 1] - t1) / t2, (times[idx + 2] - t1) / t2
    u = (t - t1) / t2
    k0, k1, k2, k3 = knots[idx - 1: idx + 3]
    m1, m2 = (k2 - k0) / (1.0 - t0), (k3 - k1) / t3
    E = 0.0625
    slope = lambda x, m: m / x if x >= E else m / -x if x <= -E else m / E
    linlog = lambda x: np.log2(x) + 5.0 if x > E else -(np.log2(-x) + 5.0) if x < -E else x / E
    linexp = lambda v: 2.0 ** (v - 5.0) if v >= 1.0 else -2.0 ** (-v - 5.0) if v <= -1.0 else v * E
    m1, m2, k1, k2 = slope(k1, m1), slope(k2, m2), linlog(k1), linlog(k2)
    uu, uuu = u * u, u * u * u
    r = m1 * (uuu - 2 * uu + u) + k1 * (2 * uuu - 3 * uu + 1) + m2 * (uuu - uu) + k2 * (-2 * uuu + 3 * uu)
    return linexp(r)


def test_mag_spline_restatement_agrees_with_the_oracle_at_knots_and_between():
    """(no GPU needed, but lives with its users) The float64 restatement above against the oracle's own spline evaluation
    of a magnitude spline the oracle does know: camera.scale."""
    gnm, prof = three_boxes()
    gnm['camera']['scale'] = [0.25, 0.0, 0.5, 0.1, 0.3, 0.9]
    G = O._Genome(gnm, 0.37)
    mine = mag_spline64(gnm['camera']['scale'], np.float32(0.37))
    assert abs(float(G.val(('camera', 'scale'), 1.0, 'mag')) - mine) <= 2e-5 * mine


# ------------------------------------------------------------------ 5. the ABI refuses malformed opacity structure
def test_genome_create_rejects_bad_opacity_structure(mgr):
    lib = _lib.load()
    gnm = three_boxes((0.5, None, 1.0))[0]
    gnm['final_xform'] = copy.deepcopy(gnm['xforms']['1'])
    pk = GenomePacker(gnm)
    prog = np.ascontiguousarray(pk.prog, np.int32)
    rec0, xs = int(prog[5]), int(prog[6])

    def create(ops):
        ops = np.ascontiguousarray(ops, np.int32)
        g = C.c_void_p()
        rc = lib.fl_genome_create(mgr.fb.ctx, prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), pk.nrows, C.byref(g))
        if rc == 0:
            lib.fl_genome_destroy(g)
        return rc
    assert create(pk.ops_array) == 0
    i14 = [i for i, o in enumerate(pk.ops_array) if o[0] == OP_CONST and o[1] == rec0 + 14][0]
    iop = [i for i, o in enumerate(pk.ops_array) if o[0] == OP_OPACITY and o[1] == rec0 + 15][0]
    bad = pk.ops_array.copy(); bad[i14, 2] |= 1 << 10
    assert create(bad) == _lib.FL_E_INVAL                                   # bits >= 10 of word 14 stay refused
    for dst in (rec0 + 14, rec0 + 13, rec0 + 16, rec0 + xs + 15 - 1, rec0 + 3 * xs + 15, 3):
        bad = pk.ops_array.copy(); bad[iop, 1] = dst
        assert create(bad) == _lib.FL_E_INVAL, dst                          # only word 15 of a SELECTABLE record
    for row in (-1, pk.nrows, pk.nrows + 7):
        bad = pk.ops_array.copy(); bad[iop, 2] = row
        assert create(bad) == _lib.FL_E_INVAL, row
    bad = np.delete(pk.ops_array, iop, axis=0)
    assert create(bad) == _lib.FL_E_INVAL                                   # the flag without its op: word 15 would be 0


# ------------------------------------------------------------------ 6. fl_interp
def test_interp_writes_plot_probability_per_temporal_sample(mgr):
    """An opacity animated 1 -> 0.2 -> 0 across the frame window: word 15 of every temporal sample against the float64
    formula on the float64 magnitude-domain spline, 2e-5 relative (the project's fl_interp bar), exact at the snaps."""
    gnm, prof = three_boxes((None, [1.0, 0.0, 0.0, 0.0, 0.5, 0.2], 0.7))
    gnm['time'] = {'duration': 1, 'frame_width': 1.0}
    prof = dict(prof, frame_width=1.0)
    rdr, gprof, dim, g, ts, td = setup_frame(mgr, gnm, prof, 0.5)
    assert td > 0.9
    pk = rdr.packer
    dev = mgr.fb.read('params', (1024, pk.pstride), np.float32, g)
    xo, xs = int(pk.prog[5]), int(pk.prog[6])
    w14 = dev[:, [xo + 14, xo + xs + 14, xo + 2 * xs + 14]].view(np.int32)
    assert (w14 == np.array([1, 1 | 0x200, 1 | 0x200])).all()
    assert (dev[:, xo + 15] == 0).all()                                   # no key: the word stays padding
    tstep = np.float32(np.float32(td) / np.float32(1024))
    worst, n_frac, n_one, n_zero = 0.0, 0, 0, 0
    snap1 = float(np.float32(1) - np.float32(1e-6))
    for s in range(1024):
        t = np.float32(ts) + np.float32(s) * tstep
        p = min(max(mag_spline64(gnm['xforms']['1']['opacity'], t), 0.0), 1.0)
        q, d = plot_probability(p), float(dev[s, xo + xs + 15])
        qf = 10.0 ** np.log2(p) if p > 0 else 0.0
        # the device's float32 spline value may fall on the other side of a threshold it is within the fl_interp bar of
        near_snap = abs(p - snap1) <= 2e-5 * snap1 or abs(qf - 2.0 ** -32) <= 1e-4 * 2.0 ** -32
        if q in (0.0, 1.0):
            assert d == q or (near_snap and abs(d - qf) <= 1e-4 * qf), (s, p, d)
            n_one += d == 1.0; n_zero += d == 0.0
        elif not (near_snap and d in (0.0, 1.0)):
            worst = max(worst, abs(d - q) / q); n_frac += 1
            assert 0.0 < d < 1.0
    print('plot probability: %d fractional samples, worst relative error %.3g; %d at 1, %d at 0' % (n_frac, worst, n_one, n_zero))
    assert n_frac > 500 and n_one >= 1 and n_zero >= 1
    assert worst <= 2e-5, worst
    q2 = dev[:, xo + 2 * xs + 15]
    assert (np.abs(q2.astype(np.float64) - plot_probability(0.7)) <= 2e-5 * plot_probability(0.7)).all()      # a constant opacity


# ------------------------------------------------------------------ 7. opacity 1 is the keyless genome, bit for bit
@pytest.mark.parametrize('which', ['three_boxes', 'cfg2'])
def test_opacity_one_is_bit_identical_to_no_opacity(built, which):
    if which == 'three_boxes':
        keyless, prof = three_boxes()
        ones = three_boxes((1.0, 1.0, 1.0))[0]
    else:
        keyless, prof = configs.cfg2(samples=2 ** 24)
        keyless['camera']['scale'] = 1.0          # zoomed in at 1080p: no pixel comes near a full cell, the packed cells are comparable
        ones = with_opacity(keyless, ['0', '1', '2'], 1.0)
    assert GenomePacker(ones).nrows == GenomePacker(keyless).nrows + 3
    for nw, nslots in ((4, 1024), (16, 256)):
        for rtc in ('1', '0'):
            ref = None
            for mode in (1, 0):                     # binned first: its density is the atomic comparison's reference for hot flames
                a = snapshot(keyless, prof, mode, nw, nslots, FLAME_RTC=rtc)
                b = snapshot(ones, prof, mode, nw, nslots, seeds_in=a['seeds0'], FLAME_RTC=rtc)
                assert int(a['ctr'][0]) > 0.15 * a['samples'] and int(b['ctr'][2]) == 0
                assert int(a['ctr'][0]) + int(a['ctr'][1]) == a['samples']
                if mode == 1:
                    ref, ref_seeds = a['front'][:, 3].copy(), a['seeds0']
                else:
                    assert np.array_equal(a['seeds0'], ref_seeds)
                did = same_bits(a, b, (which, nw, rtc, mode), atomic=mode == 0, ref=ref, min_lit=20)
                want = 'every cell, packed cells too' if which == 'cfg2' else 'every cell' if mode == 1 else 'cells below the drain threshold'
                assert did.startswith(want), (which, nw, rtc, mode, did)


# ------------------------------------------------------------------ 8. opacity 0 removes one box and nothing else
def test_opacity_zero_removes_exactly_that_xform(mgr):
    """Box 1 empty in all four channels; in the other boxes the density bit for bit that of the keyless render from the same
    seeds (no draw is spent on q = 0, so every other sample is the same sample) and the colour sums to rtol 2e-6.  The frame
    is 2^22 samples: the colour sums are float32 accumulators that take a pixel's full cells one float add per ~512 hits, each
    add rounding by up to half an ulp (3e-8 relative), in an order that changes once box 1's records leave the log; the boxes'
    fixed-point pixels take 1.5 % of all samples, so at 2^22 that is ~125 adds — a few ulp between two groupings, inside the
    33 ulp of 2e-6 — where a 2^26 frame's ~2000 adds per hot pixel would use up most of that.
    The frame is rendered twice: through fl_iterate (zeros, densities), and as the one counted launch at round 0 that such a
    frame is (counters; colour sums).  Two fl_iterate frames of ONE keyless genome from the same seeds in one context
    already differ in their Y sums by palette steps (measured: density identical, Y up to 1.1e-2 relative at single-sample
    pixels, U and V to 3e-7; the context's round counter runs on from frame to frame); launches at round 0 repeat to 6e-7."""
    lib = _lib.load()
    N = 2 ** 22
    keyless, prof = three_boxes()
    gone = three_boxes((None, 0.0, None))[0]
    seeds0 = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    fronts = {}
    for tag, gnm in (('keyless', keyless), ('gone', gone)):
        mgr.fb.write('seeds', seeds0)
        rdr, gprof, dim, g, ts, td = setup_frame(mgr, gnm, prof)
        run = C.c_uint64()
        _lib.check(lib.fl_iterate(mgr.fb.ctx, g, dim.w, dim.h, float(N), FUSE, _lib.ACCUM_BINNED, C.byref(run)))
        assert run.value == N
        fronts[tag] = mgr.fb.read('front', (dim.ah * dim.astride, 4), np.float32)
    dim = (dim.ah, dim.astride)
    assert dim == (272, 352)                                               # (344 columns in use)
    rects = box_order(fronts['keyless'], dim)
    assert fronts['keyless'][:, 3].astype(np.float64).sum() == N         # every sample of this flame is in frame
    for ch in range(4):
        assert (box(fronts['gone'], dim, rects[1], ch) == 0).all(), ch
    for k in (0, 2):
        assert np.array_equal(box(fronts['gone'], dim, rects[k]), box(fronts['keyless'], dim, rects[k])), k
    in1 = box(fronts['keyless'], dim, rects[1]).sum()
    assert fronts['gone'][:, 3].astype(np.float64).sum() == N - in1
    # the counters, from the same frame as one counted launch (16 rounds of 1024 x 256 walkers)
    a = launch(mgr, keyless, prof, 1, N // (1024 * 256), FUSE, seeds0)
    b = launch(mgr, gone, prof, 1, N // (1024 * 256), FUSE, seeds0)
    assert np.array_equal(a['front'][:, 3], fronts['keyless'][:, 3]) and np.array_equal(b['front'][:, 3], fronts['gone'][:, 3])
    assert a['ctr'].tolist() == [N, 0, 0, 0]
    assert b['ctr'].tolist() == [N - int(in1), 0, int(in1), 0]
    assert np.array_equal(a['rng'], b['rng']) and np.array_equal(a['pts'], b['pts'])       # no draw is spent on q = 0
    for ch in range(4):
        assert (box(b['front'], dim, rects[1], ch) == 0).all(), ch
    for k in (0, 2):
        for ch in range(3):
            got, want = box(b['front'], dim, rects[k], ch), box(a['front'], dim, rects[k], ch)
            print('box %d channel %d: worst relative difference %.3g' % (k, ch, (np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max()))
            np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-4)


# ------------------------------------------------------------------ 9. fractional opacities: the distribution
def _fraction_checks(r, rects, qs, what):
    """Box fractions and the dropped share against their analytic expectations, 5-sigma bars with the wave-round as the
    independent trial (the xform choice is per wave)."""
    w = np.array(BOX_WEIGHTS)
    qs = np.array(qs, np.float64)
    acc, oob, drop = int(r['ctr'][0]), int(r['ctr'][1]), int(r['ctr'][2])
    N = r['samples']
    assert acc + oob + drop == N and oob == 0, (what, r['ctr'], N)
    dens = [box(r['front'], r['dim'], rc).sum() for rc in rects]
    assert sum(dens) == acc == r['front'][:, 3].astype(np.float64).sum()
    M = N / 64.0
    Mp = M * (qs * w).sum()
    f = qs * w / (qs * w).sum()
    for k in range(3):
        got, bar = dens[k] / acc, 5 * np.sqrt(f[k] * (1 - f[k]) / Mp)
        print('%s box %d: fraction %.6f expected %.6f bar %.2g' % (what, k, got, f[k], bar))
        assert abs(got - f[k]) <= bar, (what, k, got, f[k], bar)
    hid = (w * (1 - qs)).sum()
    var = (w * (1 - qs) ** 2).sum() - hid ** 2
    bar = 5 * np.sqrt(var / M + (w * qs * (1 - qs)).sum() / N)
    print('%s dropped %.6f expected %.6f bar %.2g' % (what, drop / N, hid, bar))
    assert abs(drop / N - hid) <= bar, (what, drop / N, hid, bar)
    return dens


@pytest.fixture(scope='module')
def keyless_reference():
    gnm, prof = three_boxes()
    F = prepare(gnm, prof)
    ref, _, _ = O.flam3_render(F['dim'], F['packer'].prog, F['params'], F['palette'], F['seeds'], N26, 8)
    return ref


@pytest.mark.parametrize('opac', [(0.5, 1.0, 0.25), (0.9, 0.7, 1.0)])
def test_fractional_opacity_distribution(mgr, keyless_reference, opac):
    keyless, prof = three_boxes()
    k0 = launch(mgr, keyless, prof, 1, 256, FUSE)
    rects = box_order(k0['front'], k0['dim'])
    qs = [plot_probability(p) for p in opac]
    assert qs[:2] == pytest.approx([0.1, 1.0]) or qs[2] == 1.0
    r = launch(mgr, three_boxes(opac)[0], prof, 1, 256, FUSE)
    dens = _fraction_checks(r, rects, qs, str(opac))
    # inside each box: the keyless flam3-style render's box (any scale: both are normalised), on 8 x 8 blocks
    ref = keyless_reference
    for k, (r0, r1, c0, c1) in enumerate(rects):
        pad = (r0, r0 + 39, c0, c0 + 55)                                   # 40 x 56: whole blocks; the margin is empty gap
        assert box(r['front'], r['dim'], pad).sum() == dens[k]
        bg = box(r['front'], r['dim'], pad).reshape(5, 8, 7, 8).sum((1, 3))
        br = box(ref, r['dim'], pad).reshape(5, 8, 7, 8).sum((1, 3))
        ng, nr = bg.sum(), br.sum()
        pg, pr = bg / ng, br / nr
        l1 = np.abs(pg - pr).sum()
        floor = (np.sqrt(2 / np.pi) * np.sqrt(pr * (1 - pr) * (1 / ng + 1 / nr))).sum()     # E|difference| of two multinomials
        print('%s box %d: %d samples, block L1 %.5f, shot-noise floor %.5f' % (opac, k, ng, l1, floor))
        assert l1 <= floor + 0.02, (opac, k, l1, floor)
        cg = np.array([box(r['front'], r['dim'], pad, ch).sum() for ch in range(3)]) / ng
        cr = np.array([box(ref, r['dim'], pad, ch).sum() for ch in range(3)]) / nr
        assert np.abs(cg - cr).max() < 1.0 / 255, (opac, k, cg, cr)


# ------------------------------------------------------------------ 10. every kernel form renders the same samples
FRACTIONAL_OPACITY = (0.5, 1.0, 0.25)

CHILD = r'''
import sys
sys.path[:0] = [%(repo)r, %(repo)r + '/tests']
import numpy as np
import flames
import gpu_harness
gnm, prof = flames.three_boxes(%(opacity)r)
seeds = np.load(%(seeds)r)
out = {}
for mode in (0, 1):
    r = gpu_harness.snapshot(gnm, prof, mode, seeds_in=seeds)
    r['pts'] = r['pts'][:, :3].copy()
    for k in ('ctr', 'atom', 'rng', 'pts', 'front'):
        out['%%s%%d' %% (k, mode)] = r[k]
np.savez(%(out)r, **out)
'''


def test_fractional_opacity_same_on_every_path(built, tmp_path, capfd):
    gnm, prof = three_boxes(FRACTIONAL_OPACITY)
    base = {}
    for mode in (0, 1):
        base[mode] = snapshot(gnm, prof, mode, seeds_in=None if mode == 0 else base[0]['seeds0'])
        assert 0 < int(base[mode]['ctr'][2]) < base[mode]['samples']
    seeds = base[0]['seeds0']
    ref = base[1]['front'][:, 3]
    assert same_bits(base[0], base[1], 'binned == atomic (hot flags clear)', colour_exact=False, atomic=True, ref=ref, min_lit=20).startswith('cells below')
    for mode in (0, 1):
        assert same_bits(base[mode], snapshot(gnm, prof, mode, seeds_in=seeds, FLAME_RTC='0'), ('interpreter', mode), atomic=mode == 0, ref=ref, min_lit=20)
        assert same_bits(base[mode], snapshot(gnm, prof, mode, 16, 256, seeds_in=seeds), ('16-wave quarters', mode), colour_exact=False,
                         atomic=mode == 0, ref=ref, min_lit=20)
        assert same_bits(base[mode], snapshot(gnm, prof, mode, 16, 256, seeds_in=seeds, FLAME_RTC='0'), ('16-wave quarters, interpreter', mode),
                         colour_exact=False, atomic=mode == 0, ref=ref, min_lit=20)
    same_bits(base[1], snapshot(gnm, prof, 1, seeds_in=seeds, FLAME_BIN_WIDE='1'), 'wide tiles', colour_exact=False)
    same_bits(base[1], snapshot(gnm, prof, 1, seeds_in=seeds, FLAME_BIN_WIDE='1', FLAME_RTC='0'), 'wide tiles, interpreter', colour_exact=False)
    assert 'interpreter kernel' not in capfd.readouterr().err, 'the per-genome kernel was not used'
    # the plot of a round inside the next round's xform block (the default for this flame) or behind its own walk: a code
    # generation switch of the per-genome kernel, so a process of its own (the module cache does not key on the flags)
    np.save(str(tmp_path / 'seeds.npy'), seeds)
    out = str(tmp_path / 'nomerge.npz')
    r = subprocess.run([sys.executable, '-c', CHILD % dict(repo=REPO, opacity=FRACTIONAL_OPACITY, seeds=str(tmp_path / 'seeds.npy'), out=out)], capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, FLAME_RTC_FLAGS='-DFL_ITER_MERGE_MAX_XF=0'))
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'interpreter kernel' not in r.stderr
    z = np.load(out)
    for mode in (0, 1):
        same_bits(base[mode], dict((k, z['%s%d' % (k, mode)]) for k in ('ctr', 'atom', 'rng', 'pts', 'front')), ('no MERGE', mode), atomic=mode == 0, ref=ref, min_lit=20)


def test_fractional_opacity_atomic_histogram_where_cells_are_comparable(built, capfd):
    """cfg2 zoomed in at 1080p (no pixel comes near a full cell, asserted) with fractional opacities on all three xforms: the
    packed histogram of direct atomics — hidden samples: no add, no roulette draw — against the binned accumulate's, the
    interpreter's and the 16-wave quarters', densities and packed cells exact, colour sums to 2e-6 across accumulate modes
    and bit for bit within one."""
    gnm, prof = configs.cfg2(samples=2 ** 24)
    gnm['camera']['scale'] = 1.0
    for k, p in zip('012', (0.5, 0.9, 0.25)):
        gnm['xforms'][k]['opacity'] = p
    base = {}
    for mode in (0, 1):
        base[mode] = snapshot(gnm, prof, mode, seeds_in=None if mode == 0 else base[0]['seeds0'])
        c = base[mode]['ctr']
        assert int(c[0]) > 100000 and int(c[2]) > 0.3 * base[mode]['samples'] and int(c[0] + c[1] + c[2]) == base[mode]['samples']
        assert float(base[mode]['front'][:, 3].astype(np.float64).sum()) == int(c[0])
    seeds = base[0]['seeds0']
    full = 'every cell, packed cells too'
    assert same_bits(base[0], base[1], 'binned == atomic', colour_exact=False) == full
    for mode in (0, 1):
        assert same_bits(base[mode], snapshot(gnm, prof, mode, seeds_in=seeds, FLAME_RTC='0'), ('interpreter', mode)) == full
        assert same_bits(base[mode], snapshot(gnm, prof, mode, 16, 256, seeds_in=seeds), ('16-wave quarters', mode), colour_exact=mode == 0) == full
    assert same_bits(base[0], snapshot(gnm, prof, 1, seeds_in=seeds, FLAME_BIN_WIDE='1'), 'atomic == wide tiles', colour_exact=False) == full
    assert 'interpreter kernel' not in capfd.readouterr().err, 'the per-genome kernel was not used'


def test_fractional_opacity_many_xforms_per_genome_equals_interpreter(built, capfd):
    """cfg3 (8 xforms + final: records fetched per round, operand table in LDS, no MERGE) and cfg5 (12 xforms: the single-copy
    loop) with two fractional xforms."""
    for cfg, keys in (('cfg3', ['2', '5']), ('cfg5', ['03', '10'])):
        gnm, prof = configs.CONFIGS[cfg](samples=2 ** 24)
        prof = dict(prof, width=640, height=360)
        gnm['camera']['scale'] = 0.9
        gnm = with_opacity(gnm, keys[:1], 0.5)
        gnm = with_opacity(gnm, keys[1:], [0.9, 0.3])
        seeds = ref = None
        for mode in (1, 0):                         # binned first: the reference density of the atomic comparison
            a = snapshot(gnm, prof, mode, seeds_in=seeds)
            seeds = a['seeds0']
            b = snapshot(gnm, prof, mode, seeds_in=seeds, FLAME_RTC='0')
            assert 1000 < int(a['ctr'][2]) and int(a['ctr'][0]) > 100000, a['ctr']
            if mode == 1:
                ref = a['front'][:, 3].copy()
            did = same_bits(a, b, (cfg, mode), colour_exact=mode == 1 or int(a['ctr'][3]) == 0, atomic=mode == 0, ref=ref)
            print(cfg, 'mode', mode, 'compared:', did)
            assert did
    assert 'interpreter kernel' not in capfd.readouterr().err, 'the per-genome kernel was not used'


# ------------------------------------------------------------------ 11. an animated opacity
def test_animated_opacity_uses_each_samples_own_probability(mgr):
    keyless, prof = three_boxes()
    k0 = launch(mgr, keyless, prof, 1, 256, FUSE)
    rects = box_order(k0['front'], k0['dim'])
    gnm, prof = three_boxes((None, [1.0, 0.0], None))
    gnm['time'] = {'duration': 1, 'frame_width': 1.0}
    prof = dict(prof, frame_width=1.0)
    r = launch(mgr, gnm, prof, 1, 256, FUSE)
    gprof = profile.wrap(prof, gnm)
    ts, td = frame_times(gprof, 0.5)
    tstep = np.float32(np.float32(td) / np.float32(1024))
    q1 = np.array([plot_probability(mag_spline64([1.0, 0.0], np.float32(ts) + np.float32(s) * tstep)) for s in range(1024)])
    assert q1.max() == 1.0 and q1.min() == 0.0 and 0.05 < q1.mean() < 0.95
    # every temporal sample runs the same number of samples: the frame is the equal-weight mixture of its 1024 samples
    w = np.array(BOX_WEIGHTS)
    plotted = np.stack([np.full(1024, w[0]), w[1] * q1, np.full(1024, w[2])])        # per sample, per box
    f = plotted.sum(1) / plotted.sum()
    acc, oob, drop = (int(x) for x in r['ctr'][:3])
    assert acc + oob + drop == r['samples'] and oob == 0
    Mp = r['samples'] / 64.0 * plotted.sum() / 1024
    got = box(r['front'], r['dim'], rects[1]).sum() / acc
    bar = 5 * np.sqrt(f[1] * (1 - f[1]) / Mp)
    print('animated: box 1 fraction %.6f expected %.6f bar %.2g; mean q %.4f' % (got, f[1], bar, q1.mean()))
    assert abs(got - f[1]) <= bar, (got, f[1], bar)
    assert abs(f[1] - w[1]) > 20 * bar                                     # (a test that could tell)


# ------------------------------------------------------------------ 12. end to end
def test_flam3_file_with_opacity_renders_differently_without_it(mgr, tmp_path):
    from cuburn_amd.genome import store
    gold = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'genome_front.json')))
    src = gold['xml']['rich'].replace(' chaos="1 0.5 2"', '')
    assert src.count(' opacity="0.5"') == 1
    frames = {}
    for tag, text in (('with', src), ('without', src.replace(' opacity="0.5"', ''))):
        d = tmp_path / tag
        d.mkdir()
        (d / 'rich.flam3').write_text(text)
        with pytest.warns(UserWarning):
            gnm, base = store.connect(str(d)).animation(str(d / 'rich.flam3'))
        has = [k for k, xf in gnm['xforms'].items() if 'opacity' in xf]
        assert (len(has) >= 1) == (tag == 'with')
        prof = dict(configs.cfg2()[1], width=320, height=240)
        gprof = profile.wrap(prof, gnm)
        rdr = render.Renderer(gnm, gprof)
        assert bool((rdr.packer.ops_array[:, 0] == OP_OPACITY).any()) == (tag == 'with')
        mgr.fb.write('seeds', mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32) if 'seeds' not in frames else frames['seeds'])
        frames.setdefault('seeds', mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32))
        evt, h = mgr.queue_frame(rdr, gnm, gprof, 0.1)
        evt.synchronize()
        frames[tag] = np.array(h).astype(np.int32)
        assert frames[tag].shape == (240, 320, 4) and (frames[tag][..., 3] > 0).mean() > 0.05
    mad = np.abs(frames['with'] - frames['without']).mean()
    print('rich.flam3 with / without opacity: mean absolute difference %.3f' % mad)
    assert mad > 0.5, mad
