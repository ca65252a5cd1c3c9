"""
The two kernels at the head of every frame (cuburn_amd/csrc/interp.hip: k_interp_params, k_interp_palette) against the float64
model of tests/interp_model.py, on every branch: the atlas of tests/interp_cases.py, which tests/test_cpu_interp.py ties to the
float32 oracle and to the reference's own kernel output.  Every test is one fl_genome_create + fl_genome_upload + fl_interp and a
read of the parameter blocks / the packed palette / the RNG states: no frames, no iterate.

Bars.  All deviations are device against model, in units of the model's scale.  Per class the device may deviate by
FACTOR = 4 x what the float32 evaluation of the same expression deviates ON THE SAME INPUT (the oracle for the splines, the float32
numpy restatement of the op formulas over the oracle's splines for the other op kinds; computed here at run time, pinned in
tests/test_cpu_interp.py's table), and at least by 4 x 2^-24.  Why 4: kernel and oracle evaluate the same float32 expression in
the same order without contraction, and float division is correctly rounded on both sides; they can differ only in log2f / exp2f
(and sinf / cosf for the op kinds), the device library against libm at about an ulp each, so a doubled error with a factor of
two over it.  Exact words (FL_OP_CONST, the last CDF word, the opacity outcomes 0 and 1) and the packed palette are bit-equal.
The device's worst deviation per class is appended to interp_errors.txt in the directory the environment variable
FLAME_TEST_REPORT_DIR names, when it is set.
"""
import ctypes as C
import os

import numpy as np
import pytest

from common import O
from cuburn_amd import configs, profile, render, _lib
import interp_model as M
import interp_cases as T

pytestmark = pytest.mark.gpu

FACTOR = 4.0
U = 2.0 ** -24


@pytest.fixture(scope='module')
def mgrs(built):
    prod = render.RenderManager(device=0, host_seed=7)
    assert prod.fb.nslots == 1536
    return {1024: render.RenderManager(device=0, nslots=1024, host_seed=7), 1536: prod}


def report(test, worst):
    try:
        out = os.environ.get('FLAME_TEST_REPORT_DIR')
        if out and os.path.isdir(out):
            with open(os.path.join(out, 'interp_errors.txt'), 'a') as fp:
                for key, (dev, bar, own) in sorted(worst.items(), key=str):
                    fp.write('%s: %s / %s: device %.3f bar %.3f oracle %.3f (x 2^-24 of scale)\n' % (test, key[0], key[1], dev / U, bar / U, own / U))
    except OSError:
        pass


def check(worst, got, own, what):
    """Device against model per class under FACTOR x the float32 evaluation's own deviation (and the floor)."""
    assert set(got) == set(own), sorted(set(got) ^ set(own), key=str)
    for k, v in got.items():
        bar = FACTOR * max(own[k], U)
        old = worst.get(k, (0.0, 0.0, 0.0))
        worst[k] = (max(old[0], v), max(old[1], bar), max(old[2], own[k]))
    for k, v in got.items():
        assert v <= FACTOR * max(own[k], U), '%s, class %s: device deviates %.2f x 2^-24 of scale from the model, bar %.2f (float32 evaluation %.2f)' % (
            what, k, v / U, FACTOR * max(own[k], U) / U, own[k] / U)


GREY = (np.full((1, 256, 4), 0.5, np.float32), [0.0])


class Device(object):
    """A synthetic genome on the device: created, uploaded, destroyed with the block."""

    def __init__(self, mgr, g, pal=GREY):
        self.mgr, self.g, self.lib = mgr, g, _lib.load()
        self.h = C.c_void_p()
        ops = np.ascontiguousarray(g.ops, np.int32)
        _lib.check(self.lib.fl_genome_create(mgr.fb.ctx, g.prog.ctypes.data, len(g.prog), ops.ctypes.data, len(ops), g.nrows, C.byref(self.h)))
        pals = np.ascontiguousarray(pal[0], np.float32)
        pt = np.full(32, M.PAD_TIME, np.float32)
        pt[:len(pal[1])] = pal[1]
        times, knots = np.ascontiguousarray(g.times), np.ascontiguousarray(g.knots)
        _lib.check(self.lib.fl_genome_upload(mgr.fb.ctx, self.h, times.ctypes.data, knots.ctypes.data, pals.ctypes.data, pt.ctypes.data, len(pals)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lib.fl_ctx_sync(self.mgr.fb.ctx)
        self.lib.fl_genome_destroy(self.h)

    def interp(self, window, size=(200, 120)):
        """fl_interp for the window; the parameter blocks (samples, pstride) float32."""
        _lib.check(self.lib.fl_interp(self.mgr.fb.ctx, self.h, size[0], size[1], window[0], window[1]))
        return self.mgr.fb.read('params', (self.mgr.fb.ntemporal, self.g.pstride), np.float32, self.h)


def blocks(mgr, g, window, size=(200, 120)):
    with Device(mgr, g) as d:
        return d.interp(window, size)


# ------------------------------------------------------------------ splines
@pytest.mark.parametrize('slots', T.SLOTS)
@pytest.mark.parametrize('window', T.WINDOWS, ids=T.WINDOW_IDS)
def test_splines_on_every_branch(mgrs, window, slots):
    g = T.spline_genome()
    t = T.times_of(window, slots)
    dev = blocks(mgrs[slots], g, window)
    worst = {}
    try:
        check(worst, T.spline_deviations(g, dev, t), T.spline_deviations(g, T.f32_blocks(g, t), t), 'window %r, %d samples' % (window, slots))
    finally:
        report('splines %r %d' % (window, slots), worst)
    assert len(worst) >= 10


def test_last_row_of_32_knots_past_its_last_knot(mgrs):
    """The 32-knot row is the LAST of its table and the frame runs past its 31st knot: the fourth support point is the padding row
    the library keeps behind the table (include/flame_hip.h (4)), as in the model's table."""
    g = T.spline_genome(last32=True)
    assert g.nrows == 2 and (g.times[1] < 1e8).all()
    window = T.WINDOWS[4]
    worst = {}
    for slots in T.SLOTS:
        t = T.times_of(window, slots)
        dev = blocks(mgrs[slots], g, window)
        got = T.spline_deviations(g, dev, t)
        assert ('lin', 'next-row') in got and ('mag', 'next-row') in got
        try:
            check(worst, got, T.spline_deviations(g, T.f32_blocks(g, t), t), '32 knots, last row, %d samples' % slots)
        finally:
            report('last row of 32 knots %d' % slots, worst)


# ------------------------------------------------------------------ the other op kinds
@pytest.mark.parametrize('window', T.WINDOWS, ids=T.WINDOW_IDS)
def test_precalc_ops_at_their_edges(mgrs, window):
    """Camera (two frame sizes), affine, CDF, ratio, the two inverse squares, perspective and opacity at ordinary values and at
    their clamps.  FL_OP_CONST words bit-equal, the last CDF word 2.0, opacity outcomes exactly 0 / 1 where the model's class
    says so: asserted inside op_deviations."""
    t = T.times_of(window, 1024)
    worst = {}
    try:
        for g in (T.precalc_genome(), T.opacity_genome()):
            with Device(mgrs[1024], g) as d:
                for size in T.FRAMES:
                    dim = T.frame_dim(*size)
                    dev = d.interp(window, size)
                    check(worst, T.op_deviations(g, dev, t, dim), T.op_deviations(g, T.f32_blocks(g, t, dim), t, dim),
                          'window %r, frame %r' % (window, size))
    finally:
        report('precalc %r' % (window,), worst)
    assert len(worst) == 8


def test_blocks_hold_only_what_their_ops_write(mgrs, built):
    """launch_interp_params zeroes a lane's blocks only when the lane last held another genome.  A and B have the same pstride,
    B writes a strict subset of A's words; A, B, A, B on each of the context's lanes: after every call every word the current
    genome does not write is 0.0, and the written ones are those of a manager that never held anything else, bit for bit."""
    lib = _lib.load()
    mgr = mgrs[1024]
    A = T.spline_genome()
    B = T.Genome()
    for name, t, k in T.spline_rows()[:3]:
        B.add(M.OP_SPLINE_MAG, B.row(t, k), 0, name)
    B.next += 7                                            # (not the first words behind the record either)
    B.add(M.OP_SPLINE, 1, 0, 'late')
    B.finish(pstride=A.pstride)
    window = T.WINDOWS[0]
    t = T.times_of(window, 1024)
    fresh, mask = {}, {}
    for name, g in (('A', A), ('B', B)):
        m = render.RenderManager(device=0, nslots=1024, host_seed=9)
        fresh[name] = blocks(m, g, window)
        m.fb.free()
        mask[name] = M.blocks(g.T, g.K, g.ops, t[:1], (1, 1, 1), g.pstride)[2]
    assert (mask['A'] | ~mask['B']).all() and mask['B'].sum() < mask['A'].sum() and not mask['A'].all()
    assert fresh['A'][:, mask['A'] & ~mask['B']].any()
    with Device(mgr, A) as da, Device(mgr, B) as db:
        lanes = set()
        for step, name in enumerate('AABBAABB'):
            fid = C.c_uint32()
            _lib.check(lib.fl_frame_begin(mgr.fb.ctx, C.byref(fid)))
            lanes.add(fid.value % 2)
            got = (da if name == 'A' else db).interp(window)
            assert not got[:, ~mask[name]].view(np.uint32).any(), 'step %d (%s): words no op writes are not zero' % (step, name)
            assert np.array_equal(got.view(np.uint32), fresh[name].view(np.uint32)), 'step %d (%s)' % (step, name)
        assert lanes == {0, 1}


# ------------------------------------------------------------------ palette
@pytest.mark.parametrize('case', range(len(T.palette_cases())), ids=[c[0] for c in T.palette_cases()])
def test_palette_edges(mgrs, case):
    """Packed cells and the RNG states afterwards bit-equal to the oracle's; against the model every value that differs lies
    where the model's value before truncation is within 2^-12 of an integer, and at most 0.2 % of the values lie there."""
    name, pals, times, (ts, td), seed = T.palette_cases()[case]
    mgr = mgrs[1024]
    nwalk = mgr.fb.nslots * mgr.fb.nthreads
    seeds = mgr.fb.read('seeds', (nwalk + 64 * 256, 3), np.uint32)
    seeds[nwalk:] = T.palette_seeds(seed)
    mgr.fb.write('seeds', seeds)
    g = T.Genome().finish()
    with Device(mgr, g, (pals, times)) as d:
        d.interp((ts, td))
        dev = mgr.fb.read('palette', (64, 256), np.uint64)
        after = mgr.fb.read('seeds', (nwalk + 64 * 256, 3), np.uint32)[nwalk:]
    ref, rng = O.interp_palette(pals, np.array(times, np.float32), ts, td, T.palette_seeds(seed))
    assert np.array_equal(dev, ref), '%s: %d cells differ from the oracle' % (name, (dev != ref).sum())
    assert np.array_equal(after, rng.reshape(-1, 3))
    pre, cells, model_after = T.palette_model(case)
    ndiff, far, near = M.palette_condition(dev, pre, cells)
    assert far == 0 and near <= 0.002, (name, ndiff, far, near)
    assert np.array_equal(after, model_after)


# ------------------------------------------------------------------ a real genome through the packer
def test_packer_rows_reach_the_kernel(mgrs):
    """A stepped colour, pre-affine angles of 29 and 30 interior knots (rows of 31 and 32) and an animated weight through
    GenomePacker and Renderer: the uploaded rows are oracle.normalize's, and the device blocks meet the bars, for a frame
    straddling the step and for one that runs past t = 1."""
    gnm, prof = configs.cfg2()
    xf = gnm['xforms']
    xf['0']['color'] = [0.2, 0.0, 0.8, 0.0, 0.5, 0.3, 0.5, 0.7]
    xf['0']['weight'] = [0.5, 0.0, 1.5, 0.0]

    def angle(n):
        k = [70.0, 0.0, 110.0, 0.0]
        for i in range(1, n - 1):
            k += [i / 32.0, 70.0 + 25.0 * np.sin(0.9 * i)]
        return k
    xf['1']['pre_affine']['angle'] = angle(29)
    xf['2']['pre_affine']['angle'] = angle(30)
    gprof = profile.wrap(dict(prof, width=200, height=120), gnm)
    mgr = mgrs[1024]
    rdr = render.Renderer(gnm, gprof)
    h = rdr._handle(mgr.fb)
    mgr._copy(rdr, gnm)
    g = T.Packed(rdr.packer, gnm)
    paths = [p for p, _ in rdr.packer.rows]
    for path, n in ((('xforms', '0', 'color'), 6), (('xforms', '0', 'weight'), 4), (('xforms', '1', 'pre_affine', 'angle'), 31),
                    (('xforms', '2', 'pre_affine', 'angle'), 32)):
        node = gnm
        for p in path:
            node = node[p]
        rt, rk = [np.float32(x) for x in O.normalize(node, 1)]
        for r in [i for i, p in enumerate(paths) if p == path]:
            assert len(rt) == n and np.array_equal(g.times[r, :n], rt) and np.array_equal(g.knots[r, :n], rk)
            assert (g.times[r, n:] == M.PAD_TIME).all() and not g.knots[r, n:].any()
    dim = T.frame_dim(200, 120)
    worst = {}
    try:
        for window in ((0.4375, 0.125), (0.9375, 0.125)):
            t = T.times_of(window, 1024)
            _lib.check(_lib.load().fl_interp(mgr.fb.ctx, h, 200, 120, window[0], window[1]))
            dev = mgr.fb.read('params', (1024, g.pstride), np.float32, h)
            ref = T.f32_blocks(g, t, dim)
            got = T.spline_deviations(g, dev, t)
            got.update(T.op_deviations(g, dev, t, dim))
            own = T.spline_deviations(g, ref, t)
            own.update(T.op_deviations(g, ref, t, dim))
            check(worst, got, own, 'packed genome, window %r' % (window,))
    finally:
        report('packed genome', worst)
    assert ('affine', 'all') in worst and ('cdf', 'all') in worst and ('lin', 'by-step') in worst
