"""
Xform chaos (flam3 xaos) on the device, through the C ABI: FL_OP_CHAOS_CDF against the model of tests/chaos_model.py, and the
CHAOS form of the walk (include/flame_hip.h (5) "Contract of a chaos kernel"; DESIGN.md §4.1 "Xaos").

The CPU oracle knows nothing of chaos.  The iterate tests rest on the nine-boxes flame of tests/chaos_model.py: a sample plotted
in second-level box (p, n) was produced by xform n after xform p, so the picture shows the transition counts — exactly (forbidden
pairs hold 0 hits, a cycle splits the samples in thirds), and statistically (pair masses pi_p M_pn at 6 sigma, the binomial
widened by the chain's autocorrelation bound).  Exact identities — every kernel form equals every other, an all-ones table is
the keyless genome — anchor the new form of the walk to everything the oracle already pins.
"""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from common import O
from cuburn_amd import configs, profile, render, _lib
from cuburn_amd.packer import GenomePacker, OP_CDF, OP_CHAOS_CDF
import chaos_model as X
import interp_model as M
from flames import FRACTIONAL, FORBIDDEN, ZERO_DIAGONAL, CYCLE, many_xforms, rich_xml, spread_flame
from gpu_harness import env, same_bits, setup_frame, launch, snapshot, check_against_cpu_game

pytestmark = pytest.mark.gpu
FUSE = 256
U = 2.0 ** -24


@pytest.fixture(scope='module')
def mgr(built):
    return render.RenderManager(device=0, nslots=1024, host_seed=43)


def density(r):
    return r['front'][:, 3].reshape(r['dim']).astype(np.float64)


def rects_of(r):
    cam, aff = X.affines_of(r['params'][0], r['prog'])
    return X.box_rects(cam, aff)


def frame(m, gnm, prof, nsamples, mode=_lib.ACCUM_BINNED):
    """A frame through fl_iterate; the flushed accumulator."""
    rdr, gprof, dim, g, ts, td = setup_frame(m, gnm, prof)
    run = C.c_uint64()
    _lib.check(_lib.load().fl_iterate(m.fb.ctx, g, dim.w, dim.h, float(nsamples), FUSE, mode, C.byref(run)))
    assert run.value == nsamples
    front = m.fb.read('front', (dim.ah * dim.astride, 4), np.float32)
    params = m.fb.read('params', (1024, rdr.packer.pstride), np.float32, g)
    return dict(front=front, dim=(dim.ah, dim.astride), params=params, prog=rdr.packer.prog)


# ------------------------------------------------------------------ fl_genome_create
def test_genome_create_rejects_malformed_chaos_programs(mgr):
    lib = _lib.load()
    pk = GenomePacker(X.nine_boxes(FRACTIONAL)[0])
    co, ps, xo, xs = int(pk.prog[8]), int(pk.prog[3]), int(pk.prog[5]), int(pk.prog[6])

    def create(prog, ops, nrows=pk.nrows):
        prog, ops = np.ascontiguousarray(prog, np.int32), np.ascontiguousarray(ops, np.int32)
        g = C.c_void_p()
        rc = lib.fl_genome_create(mgr.fb.ctx, prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), nrows, C.byref(g))
        if rc == 0:
            lib.fl_genome_destroy(g)
        return rc
    assert create(pk.prog, pk.ops_array) == 0
    # 1. a chaos_off that is out of range or overlaps the records
    for off in (-1, 0, 6, xo, xo + 3 * xs - 1, co - 1, ps - 8, ps, ps + 1, 1 << 30):
        bad = pk.prog.copy(); bad[8] = off
        assert create(bad, pk.ops_array) == _lib.FL_E_INVAL, off
    # 2. more than 32 xforms together with chaos (and 33 keyless xforms, or 32 with chaos, are fine)
    g33 = many_xforms(33, False)[0]
    p33 = GenomePacker(g33)
    assert create(p33.prog, p33.ops_array, p33.nrows) == 0
    p32 = GenomePacker(many_xforms(32, True)[0])
    assert len(p32.prog) == 9 and create(p32.prog, p32.ops_array, p32.nrows) == 0
    n = 33
    prog = np.concatenate([p33.prog, [p33.pstride]]).astype(np.int32)
    prog[3] = p33.pstride + n * n
    rows = np.arange(n) * 0
    ops = np.concatenate([p33.ops_array, [[OP_CHAOS_CDF, p33.pstride + p * n, int(rows[p]), n] for p in range(n)]]).astype(np.int32)
    assert prog[3] <= 4096 and create(prog, ops, p33.nrows) == _lib.FL_E_INVAL
    # 3. a chaos op whose dst is not a row of the matrix; a row without its op; a chaos op in a keyless program
    ich = [i for i, o in enumerate(pk.ops_array) if o[0] == OP_CHAOS_CDF]
    assert len(ich) == 3
    for dst in (co + 1, co - 3, co + 9, xo, 6, 0):
        bad = pk.ops_array.copy(); bad[ich[1], 1] = dst
        assert create(pk.prog, bad) == _lib.FL_E_INVAL, dst
    bad = pk.ops_array.copy(); bad[ich[1], 1] = co                          # two ops for row 0, none for row 1
    assert create(pk.prog, bad) == _lib.FL_E_INVAL
    assert create(pk.prog, np.delete(pk.ops_array, ich[2], axis=0)) == _lib.FL_E_INVAL
    for b in (2, 4, 3 | (pk.nrows << 8), 3 | ((pk.nrows - 2) << 8), -1):
        bad = pk.ops_array.copy(); bad[ich[0], 3] = b
        assert create(pk.prog, bad) == _lib.FL_E_INVAL, b                   # the row length, and the rows it reads
    bad = pk.ops_array.copy(); bad[ich[0], 2] = pk.nrows - 1
    assert create(pk.prog, bad) == _lib.FL_E_INVAL
    assert create(pk.prog[:8], pk.ops_array) == _lib.FL_E_INVAL


# ------------------------------------------------------------------ fl_interp
def _genome_n(n, seed):
    rng = np.random.default_rng(seed)
    gnm, prof = many_xforms(n, False)
    keys = sorted(gnm['xforms'])
    for i, k in enumerate(keys):
        gnm['xforms'][k]['weight'] = float(np.round(rng.uniform(0.1, 2.0), 3))
        tab = dict((t, float(np.round(rng.uniform(0.0, 3.0), 3))) for t in keys if rng.uniform() < 0.8)
        gnm['xforms'][k]['chaos'] = tab or {keys[0]: 0.5}
    return gnm, prof


def interp_cases():
    anim = [[1.0, [1.0, 0.0], 1.0], [[0.0, 2.0], 1.0, [1.0, 0.0, 0.0, 0.0, 0.5, 0.2]], [1.0, 1.0, 1.0]]
    cases = {
        'nxf2': _genome_n(2, 2), 'nxf3': X.nine_boxes(FRACTIONAL), 'nxf32': _genome_n(32, 32),
        'zero-row': X.nine_boxes([[0.0, 0.0, 0.0], [1.0, 2.0, 0.5], [1.0, 1.0, 1.0]]),
        'zero-column': X.nine_boxes([[1.0, 0.0, 2.0], [0.5, 0.0, 1.0], [2.0, 0.0, 1.0]]),
        'negative': X.nine_boxes([[-1.0, 1.0, 2.0], [1.0, -0.5, -3.0], [-2.0, -2.0, -0.125]]),
        'zero-weight': X.nine_boxes(FRACTIONAL, weights=(0.5, 0.0, 0.2)),
        'animated': X.nine_boxes(anim),
    }
    return cases


@pytest.mark.parametrize('case', ['nxf2', 'nxf3', 'nxf32', 'zero-row', 'zero-column', 'negative', 'zero-weight', 'animated'])
def test_interp_writes_the_chaos_matrix(mgr, case):
    """Every row of every temporal sample against the float64 model; the bar is 4 x the float32 restatement's own deviation on
    the same input, at least 4 x 2^-24.  The last word of every row is exactly 2.0; the keyless words of the block
    are bit-equal to the keyless genome's."""
    gnm, prof = interp_cases()[case]
    if case == 'animated':
        gnm['time'] = {'duration': 1, 'frame_width': 1.0}
        prof = dict(prof, frame_width=1.0)
    rdr, gprof, dim, g, ts, td = setup_frame(mgr, gnm, prof, 0.5)
    assert (td > 0.9) == (case == 'animated')
    pk = rdr.packer
    n, co = int(pk.prog[1]), int(pk.prog[8])
    dev = mgr.fb.read('params', (1024, pk.pstride), np.float32, g)
    times, knots = pk.pack(gnm)
    T, K = M.flat_table(times, knots)
    t = M.sample_times(ts, td, 1024)
    ut, inv = np.unique(t, return_inverse=True)
    fn = O.lib().ref_catmull_rom

    def row64(r):
        return M.spline(T, K, r, t, False).value

    def row32(r):
        return np.array([fn(T.ctypes.data + 128 * r, K.ctypes.data + 128 * r, float(x), 0) for x in ut], np.float32)[inv]
    cdf_op = [o for o in pk.ops_array if o[0] == OP_CDF][0]
    ch_ops = [o for o in pk.ops_array if o[0] == OP_CHAOS_CDF]
    assert len(ch_ops) == n and [int(o[1]) for o in ch_ops] == [co + p * n for p in range(n)]
    w64 = np.stack([row64(int(cdf_op[2]) + k) for k in range(n)], 1)
    w32 = np.stack([row32(int(cdf_op[2]) + k) for k in range(n)], 1)
    c64 = np.stack([np.stack([row64((int(o[3]) >> 8) + k) for k in range(n)], 1) for o in ch_ops], 1)
    c32 = np.stack([np.stack([row32((int(o[3]) >> 8) + k) for k in range(n)], 1) for o in ch_ops], 1)
    model, own = X.cdf64(w64, c64), X.cdf32(w32, c32)
    got = dev[:, co:co + n * n].reshape(1024, n, n)
    assert (got[..., n - 1] == 2.0).all()
    own_dev = float(np.abs(own[..., :n - 1] - model[..., :n - 1]).max())
    dev_dev = float(np.abs(got[..., :n - 1] - model[..., :n - 1]).max())
    bar = 4.0 * max(own_dev, U)
    print('chaos matrix %s: device %.3f bar %.3f float32 restatement %.3f (x 2^-24)' % (case, dev_dev / U, bar / U, own_dev / U))
    out = os.environ.get('FLAME_TEST_REPORT_DIR')
    if out and os.path.isdir(out):
        with open(os.path.join(out, 'interp_errors.txt'), 'a') as fp:
            fp.write('chaos matrix %s: device %.3f bar %.3f oracle %.3f (x 2^-24 of scale)\n' % (case, dev_dev / U, bar / U, own_dev / U))
    assert dev_dev <= bar, (case, dev_dev / U, bar / U)
    if case == 'zero-row':
        assert np.array_equal(got[:, 0, :], dev[:, 6:6 + n])               # the fallback: FL_OP_CDF's own row, bit for bit
    if case == 'zero-column':
        assert np.array_equal(got[:, :, 1], got[:, :, 0])
    if case == 'negative':
        assert (got[:, 1, 0] >= 1.0).all()                                 # only xform 0 may follow xform 1
        assert np.array_equal(got[:, 2, :], dev[:, 6:6 + n])               # every entry negative: the fallback
    if case == 'zero-weight':
        assert np.array_equal(got[:, :, 1], got[:, :, 0])
    if case == 'animated':
        assert len(np.unique(got[:, 0, 0])) > 500 and got[0, 0, 0] < got[-1, 0, 0]
    # the keyless words: what the same genome without its tables gets
    plain = copy.deepcopy(gnm)
    for xf in plain['xforms'].values():
        xf.pop('chaos', None)
    rdr0, _, _, g0, _, _ = setup_frame(mgr, plain, prof, 0.5)
    assert rdr0.packer.pstride == co and len(rdr0.packer.prog) == 8
    dev0 = mgr.fb.read('params', (1024, co), np.float32, g0)
    assert np.array_equal(dev0.view(np.uint32), dev[:, :co].view(np.uint32))


# ------------------------------------------------------------------ iterate, exact
@pytest.mark.parametrize('table', ['forbidden', 'zero-diagonal'])
def test_forbidden_transitions_hold_exactly_zero_hits(built, table):
    """Every second-level box of a forbidden pair holds exactly 0 hits, every permitted one is lit — across four launches per
    frame (FLAME_LAUNCH_ROUNDS=16: the walker's next xform persists in points[].w between them) and two frames in a row, with
    both kernels."""
    tab = FORBIDDEN if table == 'forbidden' else ZERO_DIAGONAL
    gnm, prof = X.nine_boxes(tab)
    N = 2 ** 24
    for rtc in ('1', '0'):
        with env(FLAME_LAUNCH_ROUNDS='16', FLAME_RTC=rtc):
            m = render.RenderManager(device=0, nslots=1024, host_seed=45)
            try:
                for k in range(2):
                    r = frame(m, gnm, prof, N)
                    first, second = rects_of(r)
                    d = density(r)
                    assert d.sum() == N
                    lit = 0
                    for (p, n), rect in second.items():
                        got = X.in_rect(d, rect).sum()
                        lit += got
                        if tab[p][n] == 0:
                            assert got == 0, (rtc, k, p, n, got)
                            assert (X.in_rect(np.abs(r['front'][:, :3]).sum(1).reshape(r['dim']), rect) == 0).all()
                        else:
                            assert got > 1000, (rtc, k, p, n, got)
                    assert lit == N
                st = m.timings()
                assert (st['spec_launches'] > 0) == (rtc == '1') and (st['interp_launches'] > 0) == (rtc == '0')
            finally:
                m.fb.free()


def test_cyclic_table_splits_the_samples_in_exact_thirds(mgr):
    """0 -> 1 -> 2 -> 0 only, binned, write-enabled rounds a multiple of 3, everything in frame: each first-level box holds
    exactly a third of the plotted samples."""
    gnm, prof = X.nine_boxes(CYCLE)
    r = launch(mgr, gnm, prof, 1, 48, FUSE)
    N = r['samples']
    assert r['ctr'].tolist()[:3] == [N, 0, 0]
    first, second = rects_of(r)
    d = density(r)
    assert [X.in_rect(d, rc).sum() for rc in first] == [N // 3] * 3
    for (p, n), rect in second.items():
        assert X.in_rect(d, rect).sum() == (N // 3 if n == (p + 1) % 3 else 0), (p, n)


def _forms_agree(gnm, prof, what, min_lit=200):
    base = {}
    for mode in (1, 0):
        base[mode] = snapshot(gnm, prof, mode, seeds_in=None if mode == 1 else base[1]['seeds0'])
    seeds, ref = base[1]['seeds0'], base[1]['front'][:, 3]
    nxf = int(base[1]['prog'][1])
    w = base[1]['pts'][:, 3].view(np.float32)
    assert set(np.unique(w)) == set(np.arange(nxf, dtype=np.float32)), what      # the walkers carry their next xform
    same_bits(base[0], base[1], (what, 'binned == atomic'), colour_exact=False, atomic=True, ref=ref, min_lit=min_lit)
    forms = [((4, 1024), {'FLAME_RTC': '0'}), ((8, 512), {}), ((8, 512), {'FLAME_RTC': '0'}), ((16, 256), {}), ((16, 256), {'FLAME_RTC': '0'})]
    for (nw, nslots), sw in forms:
        for mode in (1, 0):
            r = snapshot(gnm, prof, mode, nw, nslots, seeds_in=seeds, **sw)
            same_bits(base[mode], r, (what, nw, sw, mode), colour_exact=nw == 4, atomic=mode == 0, ref=ref, min_lit=min_lit)
    for sw in ({}, {'FLAME_RTC': '0'}):
        r = snapshot(gnm, prof, 1, seeds_in=seeds, FLAME_BIN_WIDE='1', **sw)
        same_bits(base[1], r, (what, 'wide', sw), colour_exact=False)
    return base


def test_every_kernel_form_equals_every_other(built, capfd):
    """Per-genome kernel and interpreter; 4-wave slots, 8-wave halves and 16-wave quarters; narrow tiles, wide tiles and direct
    atomics: counters, RNG states and walkers (w included) bit-identical, densities bit-identical (atomic: the cells below the
    drain threshold), colour sums to 2e-6."""
    gnm, prof = spread_flame(FRACTIONAL)
    base = _forms_agree(gnm, prof, 'fractional table')
    c = base[1]['ctr']
    assert int(c[0]) + int(c[1]) == base[1]['samples'] and int(c[2]) == 0 and int(c[0]) > 0.2 * base[1]['samples']
    assert 'interpreter kernel' not in capfd.readouterr().err, 'the per-genome kernel was not used'


def test_every_kernel_form_with_opacity_and_a_final_xform(built, capfd):
    gnm, prof = spread_flame(FRACTIONAL)
    gnm['xforms']['1']['opacity'] = 0.5
    gnm['final_xform'] = {'color': 0.0, 'color_speed': 0.0, 'pre_affine': configs._affine(10, 0.9, 0.02, -0.03),
                          'variations': {'linear': {'weight': 0.9}, 'spherical': {'weight': 0.02}}}
    base = _forms_agree(gnm, prof, 'chaos + opacity + final')
    c = base[1]['ctr']
    assert 0 < int(c[2]) < base[1]['samples'] and int(c[0]) + int(c[1]) + int(c[2]) == base[1]['samples']
    assert 'interpreter kernel' not in capfd.readouterr().err, 'the per-genome kernel was not used'


def test_all_ones_table_renders_the_keyless_genome_bit_for_bit(built):
    keyless, prof = X.nine_boxes()
    ones = X.nine_boxes([[1.0, [1.0, 1.0], None]] * 3)[0]
    for rtc in ('1', '0'):
        a = snapshot(keyless, prof, 1, FLAME_RTC=rtc)
        b = snapshot(ones, prof, 1, seeds_in=a['seeds0'], FLAME_RTC=rtc)
        assert len(b['prog']) == 8
        same_bits(a, b, ('all ones', rtc))
        assert (a['pts'][:, 3] == 0).all()                                  # keyless kernels keep writing 0


def test_stale_next_index_is_clamped(mgr):
    """points[].w = 40 (and NaN, inf, negative) in front of a 3-xform chaos genome, as if the buffer had last served a genome
    with more xforms: on load the index is clamped to nxf - 1 (not finite, negative: 0) — include/flame_hip.h (5).  The launch
    completes, the counters add up, and the walkers that carried 40 were moved by xform 2, the others by xform 0."""
    gnm, prof = X.nine_boxes(FRACTIONAL)
    a = launch(mgr, gnm, prof, 1, 16, 16)
    pts = a['pts'].view(np.float32).copy()
    assert np.isfinite(pts[:, :2]).all()
    stale = np.array([40.0, np.nan, np.inf, -3.0, 2.5, 1e30], np.float32)
    pts[:, 3] = stale[np.arange(len(pts)) % len(stale)]
    for rtc in ('1', '0'):
        with env(FLAME_RTC=rtc):
            m = render.RenderManager(device=0, nslots=1024, host_seed=46)
            try:
                r = launch(m, gnm, prof, 1, 1, 0, points_in=pts)
            finally:
                m.fb.free()
        c = [int(v) for v in r['ctr']]
        assert c[0] + c[1] + c[2] == r['samples'] == len(pts) and c[0] == r['samples']
        first, second = rects_of(r)
        d = density(r)
        want = [0, 0, 0]
        for v in stale[np.arange(len(pts)) % len(stale)]:
            want[int(min(max(v, 0.0), 2.0)) if np.isfinite(v) else 0] += 1
        assert [int(X.in_rect(d, rc).sum()) for rc in first] == want, rtc
        w = r['pts'][:, 3].view(np.float32)
        assert set(np.unique(w)) <= {0.0, 1.0, 2.0}


# ------------------------------------------------------------------ iterate, statistical
def test_pair_masses_against_the_exact_ones(mgr):
    """2^24 samples: the nine second-level boxes against pi_p M_pn at 6 sigma per box, sigma^2 = N r (1 - r) (1 + lambda) /
    (1 - lambda) — the binomial widened by the chain's autocorrelation bound (derived, not measured; the same bar holds the
    model in tests/test_cpu_chaos.py)."""
    for tab in (FORBIDDEN, FRACTIONAL):
        gnm, prof = X.nine_boxes(tab)
        N = 2 ** 24
        r = frame(mgr, gnm, prof, N)
        rows = r['params'][0][int(r['prog'][8]):].reshape(3, 3).astype(np.float64)
        Mx = X.transition(X.cdf64(np.array([X.WEIGHTS], np.float32), np.array([tab], np.float32))[0])
        assert np.abs(X.transition(rows) - Mx).max() < 1e-6
        lam = X.lambda2(Mx)
        assert lam <= 0.5, lam
        exact = X.pair_masses(Mx)
        first, second = rects_of(r)
        d = density(r)
        assert d.sum() == N
        for (p, n), rect in second.items():
            got, want, bar = X.in_rect(d, rect).sum(), N * exact[p, n], 6 * X.sigma(N, exact[p, n], lam)
            print('pair %d -> %d: %d hits, exact %.1f, bar %.1f (lambda %.3f)' % (p, n, got, want, bar, lam))
            assert abs(got - want) <= bar, (p, n, got, want, bar)
        keyless = np.outer(X.WEIGHTS, X.WEIGHTS)
        assert np.abs(exact - keyless).max() * N > 10 * 6 * X.sigma(N, 0.25, lam)      # (a test that could tell)


def test_equal_rows_are_the_reweighted_keyless_genome(mgr):
    """c_pn = c_n: distributionally the keyless genome with weights w_n c_n — cfg2 at 256 x 256 against the oracle's flam3-style
    render of that reweighted genome at the bars of the full-size tests (block L1: noise + 2 %, colour 1 / 255)."""
    gnm, prof = configs.cfg2(samples=2 ** 24)
    prof = dict(prof, width=256, height=256, spp=2 ** 24 / 65536.0)
    col = {'0': 0.5, '1': 2.0, '2': 1.25}
    chaos, plain = copy.deepcopy(gnm), copy.deepcopy(gnm)
    for k in chaos['xforms']:
        chaos['xforms'][k]['chaos'] = dict(col)
        plain['xforms'][k]['weight'] = gnm['xforms'][k]['weight'] * col[k]
    rdr, gprof, dim, g, ts, td = setup_frame(mgr, chaos, prof)
    assert len(rdr.packer.prog) == 9
    run = C.c_uint64()
    _lib.check(_lib.load().fl_iterate(mgr.fb.ctx, g, dim.w, dim.h, float(2 ** 24), FUSE, _lib.ACCUM_BINNED, C.byref(run)))
    front = mgr.fb.read('front', (dim.ah * dim.astride, 4), np.float32)
    l1, noise, fg, fr = check_against_cpu_game(plain, prof, 0.5, 1024, dim, front, run.value, 2 ** 24, 16, 0.02, 2e-3, 1.0 / 255)
    print('equal rows: block L1 %.4f (noise %.4f), in-frame %.4f / %.4f' % (l1, noise, fg, fr))
    # ... and not the unweighted one
    front0 = frame(mgr, gnm, prof, 2 ** 24)['front']
    b = lambda f: f[:, 3].reshape(dim.ah, dim.astride)[:dim.ah // 16 * 16, :dim.astride // 16 * 16].reshape(dim.ah // 16, 16, -1, 16).sum((1, 3))
    assert np.abs(b(front) / b(front).sum() - b(front0) / b(front0).sum()).sum() > 2 * (0.02 + 1.5 * noise)


# ------------------------------------------------------------------ end to end
def test_flam3_file_with_chaos_renders_differently_without_it(mgr, tmp_path):
    from cuburn_amd.genome import store
    src = rich_xml()
    frames = {}
    for tag, text in (('with', src), ('without', src.replace(' chaos="1 0.5 2"', ''))):
        d = tmp_path / tag
        d.mkdir()
        (d / 'rich.flam3').write_text(text)
        with pytest.warns(UserWarning):
            gnm, base = store.connect(str(d)).animation(str(d / 'rich.flam3'))
        assert any('chaos' in xf for xf in gnm['xforms'].values()) == (tag == 'with')
        prof = dict(configs.cfg2()[1], width=320, height=240)
        gprof = profile.wrap(prof, gnm)
        rdr = render.Renderer(gnm, gprof)
        assert bool((rdr.packer.ops_array[:, 0] == OP_CHAOS_CDF).any()) == (tag == 'with')
        mgr.fb.write('seeds', mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32) if 'seeds' not in frames else frames['seeds'])
        frames.setdefault('seeds', mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32))
        evt, h = mgr.queue_frame(rdr, gnm, gprof, 0.1)
        evt.synchronize()
        frames[tag] = np.array(h).astype(np.int32)
        assert frames[tag].shape == (240, 320, 4) and (frames[tag][..., 3] > 0).mean() > 0.05
    mad = np.abs(frames['with'] - frames['without']).mean()
    print('rich.flam3 with / without chaos: mean absolute difference %.3f' % mad)
    assert mad > 0.5, mad
