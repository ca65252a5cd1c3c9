"""
The binned accumulate and the sample log, each alone against the integer model of tests/accum_model.py.

(a) fl_debug_accum runs k_accum_tiles_p3 / k_accum_tiles<8> (csrc/binned.hip) on the hand-built logs of tests/accum_cases.py —
    every run alignment, group total, empty group, hot-cell and fill threshold, palette chunk and the ragged last gang placed on
    purpose (tests/test_cpu_accum_model.py asserts that they are there) — and compares every cell with the model, exactly.
(b) FL_BUF_LOG / FL_BUF_DIR show what k_iter (binned) wrote: the log must pass the model's `validate`, own as many records as the
    kernel counted, and decode to the histogram that the accumulate, and a launch with direct atomics, then produce.
(c) What fl_debug_accum must refuse never reaches the device.
"""
import ctypes as C

import numpy as np
import pytest

import accum_cases as AC
import accum_model as M
from common import frame_times
from cuburn_amd import configs, profile, render, _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                  # unit roundoff of float32
FL_INV255 = np.float32(0.003921568859368562698)


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    m.fb.free()


def accum(fb, g, log, dirw):
    log, dirw = np.ascontiguousarray(log, np.uint32), np.ascontiguousarray(dirw, np.uint32)
    return _lib.load().fl_debug_accum(fb.ctx, g.w, g.h, log.ctypes.data, log.size, dirw.ctypes.data, dirw.size, *g.args())


# ---- (a) -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', AC.NAMES)
def test_accumulate_equals_the_model(mgr, name):
    """Counts are integers below 2^24 and must be exact, before the flush (packed count + float count) and after it.

    Colour channels, after the flush, against the float64 value T = S / 255 of the model's integer field sum S.  The device
    adds K non-negative terms into the cell's float: a spill adds fl(s * c) for the integer sum s < 2^18 (exact) of the hits it
    carries, c = FL_INV255 = (1 + d) / 255 with |d| <= 2^-24 (asserted below); the flush adds its s * c fused (one rounding for
    product and add).  With u = 2^-24: a term is s / 255 * (1 + d)(1 + e), |e| <= u, and goes through at most K roundings of
    the running sum, each a factor (1 + e'), |e'| <= u, all terms >= 0.  Hence |result - T| <= T * ((1 + u)^(K + 2) - 1).
    K per cell, from the model's hits h of each part (workgroup) that touches it: a hot group carries >= 16 hits, so at most
    h // 16 of them; an LDS drain is the exchange of an add that found >= 256 hits in the cell, and a cell is back at zero after
    an exchange, so at most h - 256 adds find that many; hits that go one way do not go the other, and g // 16 +
    max(0, h - g - 256) is largest at g = 0 or g = h: max(h // 16, h - 256, 0) spills; at most two more at the tile add (the
    direct spill of a chunk of big_thr hits, the drain of a packed cell found full), and one for the flush.  The reference's own
    arithmetic (one float64 division) is allowed 2^-50 T."""
    c = AC.case(name)
    log, dirw = AC.encoded(name)
    g, fb, lib = c.g, mgr.fb, _lib.load()
    model = M.accumulate(c.runs, g, c.palette, c.preload)
    before = np.zeros(g.ncells, np.uint64) if c.preload is None else c.preload
    _lib.check(lib.fl_debug_clear(fb.ctx, g.w, g.h, 0))
    fb.write('palette', c.palette)
    if c.preload is not None:
        fb.write('atom', c.preload)
    _lib.check(accum(fb, g, log, dirw))
    atom = fb.read('atom', (g.ncells,), np.uint64)
    front = fb.read('front', (g.ncells, 4), np.float32)
    _lib.check(lib.fl_debug_flush(fb.ctx, g.w, g.h))
    front2 = fb.read('front', (g.ncells, 4), np.float32)
    atom2 = fb.read('atom', (g.ncells,), np.uint64)

    hit = np.zeros(g.ncells, bool)
    hit[g.cell_of(c.runs.tile, c.runs.rec)[0]] = True
    n_atom = M.unpack_cells(atom)[0]
    count = n_atom + front[:, 3].astype(np.int64)
    print('%s: %d records, %d cells hit, %d in the floats before the flush, largest cell %d' %
          (name, len(c.runs.rec), hit.sum(), int(front[:, 3].sum()), model[0].max(initial=0)))
    assert (front[:, 3] == np.floor(front[:, 3])).all()
    bad = np.nonzero(count != model[0])[0]
    assert bad.size == 0, ('count before the flush', bad[:8], count[bad[:8]], model[0][bad[:8]])
    assert np.array_equal(atom[~hit], before[~hit]) and not front[~hit].any(), 'a cell outside every run was touched'
    if M.is_plain(c.runs, log, dirw, g, c.preload):
        assert not front.any(), 'nothing fills, nothing is hot: the float accumulator stays empty'
        bad = np.nonzero(atom != M.pack_cells(*model))[0]
        assert bad.size == 0, ('packed cells', bad[:8], atom[bad[:8]], M.pack_cells(*model)[bad[:8]])
    bad = np.nonzero(front2[:, 3].astype(np.int64) != model[0])[0]
    assert bad.size == 0, ('count after the flush', bad[:8], front2[bad[:8], 3], model[0][bad[:8]])
    assert not atom2.any()

    assert abs(float(FL_INV255) * 255.0 - 1.0) <= U
    k = M.float_adds_bound(c.runs, g)
    for ch in range(3):
        t = model[1 + ch] / 255.0
        bound = t * ((1.0 + U) ** (k + 2) - 1.0) + t * 2.0 ** -50
        err = np.abs(front2[:, ch].astype(np.float64) - t)
        worst = int(np.argmax(np.where(t > 0, err / np.maximum(bound, 1e-300), err)))
        print('  channel %d: error %.3g of a bound of %.3g where it comes closest (cell %d: %d hits, K = %d)' %
              (ch, err[worst], bound[worst], worst, model[0][worst], k[worst]))
        assert (err <= bound).all(), (ch, worst, front2[worst, ch], t[worst], err[worst], bound[worst])


# ---- (b) -------------------------------------------------------------------------------------------------------------------------
def linear_flame():
    """The parity tests' flame without transcendentals: three linear + bent xforms, a post affine, a final xform."""
    gnm, prof = configs.cfg2()
    for k in gnm['xforms']:
        gnm['xforms'][k]['variations'] = {'linear': {'weight': 0.8}, 'bent': {'weight': 0.2}}
    gnm['xforms']['1']['post_affine'] = configs._affine(10.0, 0.9, 0.05, -0.1)
    gnm['final_xform'] = {'color': 0.3, 'color_speed': 0.25, 'pre_affine': configs._affine(-8.0, 0.97, 0.02, 0.01),
                          'variations': {'linear': {'weight': 1.0}}}
    return gnm, prof


WRITERS = {}


@pytest.fixture(scope='module', autouse=True)
def free_writers():
    yield
    for m in [w[0] for w in WRITERS.values()]:
        m.fb.free()
    WRITERS.clear()


def writer(layout, monkeypatch):
    """(manager, renderer, genome, frame) of a layout, made once: narrow and wide with 1024 slots of four waves, `sub` with 256
    slots of sixteen waves (four temporal samples per workgroup)."""
    if layout not in WRITERS:
        if layout == 'wide':
            monkeypatch.setenv('FLAME_BIN_WIDE', '1')          # (read when the context is created)
        if layout == 'sub':
            monkeypatch.setenv('FLAME_NW', '16')
        m = render.RenderManager(device=0, nslots=256 if layout == 'sub' else 1024, host_seed=42)
        gnm, prof = linear_flame()
        w, h, wide = AC.FRAMES['wide' if layout == 'wide' else 'narrow']
        gprof = profile.wrap(dict(prof, width=w, height=h), gnm)
        WRITERS[layout] = (m, render.Renderer(gnm, gprof), gnm, gprof, wide)
    return WRITERS[layout]


@pytest.mark.parametrize('layout,write_rounds', [('narrow', 32), ('narrow', 21), ('wide', 32), ('wide', 21), ('sub', 21)])
def test_iterate_writes_the_log_the_model_reads(layout, write_rounds, monkeypatch, built):
    """One binned launch (5 fuse rounds, then 32 write-enabled ones — two full batches per slot — or 21: a short last batch)."""
    lib = _lib.load()
    m, rdr, gnm, gprof, wide = writer(layout, monkeypatch)
    fb, fuse = m.fb, 5
    nt = fb.nthreads
    g = M.Geometry(gprof.width, gprof.height, wide, fb.nslots, (write_rounds + 15) // 16, 16 * nt, 16)
    h = rdr._handle(fb)
    m._copy(rdr, gnm)
    ts, td = frame_times(gprof, 0.5)
    _lib.check(lib.fl_interp(fb.ctx, h, g.w, g.h, ts, td))
    nwalk = fb.nslots * nt
    seeds = fb.read('seeds', (nwalk + 64 * 256, 3), np.uint32)
    palette = fb.read('palette', (64, 256), np.uint64)

    def launch(mode):
        fb.write('seeds', seeds)
        _lib.check(lib.fl_debug_clear(fb.ctx, g.w, g.h, 1))
        _lib.check(lib.fl_debug_iter_launch(fb.ctx, h, g.w, g.h, 0, write_rounds + fuse, fuse, mode))
        ctr = np.zeros(4, np.uint64)
        _lib.check(lib.fl_debug_counters(fb.ctx, ctr.ctypes.data))
        return ctr

    ctr = launch(_lib.ACCUM_BINNED)
    log = fb.read('log', (g.log_words,), np.uint32)
    dirw = fb.read('dir', (g.dir_words,), np.uint32)
    _lib.check(lib.fl_debug_flush(fb.ctx, g.w, g.h))
    dens = fb.read('front', (g.ncells, 4), np.float32)[:, 3]

    assert M.validate(g.w, g.h, log, dirw, *g.args()) is None
    cnt = (dirw & 0xffff).reshape(g.nbins, g.nbatch).astype(np.int64)
    first = (dirw >> 16).reshape(g.nbins, g.nbatch)
    assert not first[0].any()
    per_batch = cnt.sum(0).reshape(fb.nslots, g.per_slot)
    rounds_of = np.minimum(16, write_rounds - 16 * np.arange(g.per_slot))
    print('%s %d rounds: %d records in %d batches, fullest batch %d of %d' %
          (layout, write_rounds, cnt.sum(), g.nbatch, per_batch.max(), 16 * nt))
    assert (per_batch <= rounds_of[None, :] * nt).all() and per_batch.min() > 0
    assert cnt.sum() == int(ctr[0]) > 0
    runs = M.decode_log(log, dirw, g)
    model = M.accumulate(runs, g, palette)
    assert model[0].max() < 2 ** 24
    bad = np.nonzero(dens.astype(np.int64) != model[0])[0]
    assert bad.size == 0, (bad[:8], dens[bad[:8]], model[0][bad[:8]])

    ctr_a = launch(_lib.ACCUM_ATOMIC)
    _lib.check(lib.fl_debug_flush(fb.ctx, g.w, g.h))
    dens_a = fb.read('front', (g.ncells, 4), np.float32)[:, 3]
    assert int(ctr_a[2]) == 0 and np.array_equal(ctr_a[:2], ctr[:2])
    assert np.array_equal(dens_a, dens)


# ---- (c) -------------------------------------------------------------------------------------------------------------------------
def test_invalid_logs_never_reach_the_device(mgr):
    lib, fb = _lib.load(), mgr.fb
    name = 'align/wide/256-3-256-3'
    c = AC.case(name)
    log, dirw = AC.encoded(name)
    g = c.g
    _lib.check(lib.fl_debug_clear(fb.ctx, g.w, g.h, 0))
    fb.write('palette', c.palette)
    _lib.check(accum(fb, g, log, dirw))

    def state():
        return [fb.read(which, shape, dtype) for which, shape, dtype in
                (('log', (g.log_words,), np.uint32), ('dir', (g.dir_words,), np.uint32), ('atom', (g.ncells,), np.uint64),
                 ('front', (g.ncells, 4), np.float32), ('palette', (64, 256), np.uint64))]

    before = state()
    assert np.array_equal(before[0], log) and np.array_equal(before[1], dirw) and before[2].any()
    for what, (w, h, blog, bdir, nbatch, records, nslots, nparts, wide) in AC.invalid_examples():
        blog, bdir = np.ascontiguousarray(blog, np.uint32), np.ascontiguousarray(bdir, np.uint32)
        rc = lib.fl_debug_accum(fb.ctx, w, h, blog.ctypes.data, blog.size, bdir.ctypes.data, bdir.size, nbatch, records, nslots, nparts, wide)
        assert rc == _lib.FL_E_INVAL, what
    for a, b in zip(before, state()):
        assert np.array_equal(a, b)


def test_log_taps_before_the_first_binned_launch(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=7)
    word = np.zeros(1, np.uint32)
    for which in ('log', 'dir'):
        rc = _lib.load().fl_read_buffer(m.fb.ctx, None, _lib.BUF[which], word.ctypes.data, 4)
        assert rc == _lib.FL_E_INVAL and b'not allocated' in _lib.load().fl_last_error()
    m.fb.free()
