"""
What the GPU tests and tools/ share to drive the library through its C ABI and to judge what it returned: frames set up and
launched on a RenderManager, the oracle's device model beside them, single filters, and the comparisons.
Importing this module creates no context (the per-genome compile check at the end needs none at all).
"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from common import O, prepare, frame_times
from cuburn_amd import profile, render, _lib
from cuburn_amd.packer import GenomePacker
from flames import random_genome


def walkers(mgr):
    """(slots, threads per slot, walker count, oracle geometry) of a manager's current context."""
    ns, nt = mgr.fb.nslots, mgr.fb.nthreads
    return ns, nt, ns * nt, {256: O.GEOM_4x64, 512: O.GEOM_8x64, 1024: O.GEOM_16x64}[nt]


def setup_frame(mgr, gnm, prof, tc=0.5):
    """Upload + interp on the GPU; returns (rdr, gprof, dim, handle) and device params/palette."""
    gprof = profile.wrap(prof, gnm)
    rdr = render.Renderer(gnm, gprof)
    g = rdr._handle(mgr.fb)
    mgr._copy(rdr, gnm)
    dim = mgr.fb.calc_dim(gprof.width, gprof.height)
    ts, td = frame_times(gprof, tc)
    _lib.check(_lib.load().fl_interp(mgr.fb.ctx, g, dim.w, dim.h, ts, td))
    return rdr, gprof, dim, g, ts, td


def run_device_model(mgr, gnm, prof, nrounds, fuse, launches=1, mode=0, seeds_in=None, tc=0.5):
    """GPU and oracle from the same device params / palette / seeds / points; returns both states.
    mode 0 = packed global atomics (hot flags + roulette live), 1 = binned (no sample thinning)."""
    lib = _lib.load()
    ns, nt, nwalk, geom = walkers(mgr)
    if seeds_in is not None:                # before interp: the palette kernel draws from these too
        mgr.fb.write('seeds', seeds_in)
    seeds0 = mgr.fb.read('seeds', (nwalk + 64 * 256, 3), np.uint32)
    rdr, gprof, dim, g, ts, td = setup_frame(mgr, gnm, prof, tc)
    d = O.calc_dim(dim.w, dim.h)
    nbins = dim.ah * dim.astride
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, dim.w, dim.h, 1))
    params = mgr.fb.read('params', (ns, rdr.packer.pstride), np.float32, g)
    palette = mgr.fb.read('palette', (64, 256), np.uint64)
    seeds = mgr.fb.read('seeds', (nwalk + 64 * 256, 3), np.uint32)
    rng = seeds[:nwalk].copy()
    points = np.full((nwalk, 4), np.nan, np.float32)
    hot = np.zeros(nbins // 16, np.uint32)
    atom = np.zeros(nbins, np.uint64)
    out4 = np.zeros((nbins, 4), np.float32)
    res = []
    r0 = 0
    for k in range(launches):
        f = fuse if k == 0 else 0
        _lib.check(lib.fl_debug_iter_launch(mgr.fb.ctx, g, dim.w, dim.h, r0, nrounds + f, f, mode))
        ctr_ref = O.iter_launch(geom, d, rdr.packer.prog, params, palette, rng, points, ns,
                                hot, atom, out4, r0, nrounds + f, f)
        ctr_dev = np.zeros(4, np.uint64)
        _lib.check(lib.fl_debug_counters(mgr.fb.ctx, ctr_dev.ctypes.data))
        dev_atom = mgr.fb.read('atom', (nbins,), np.uint64)
        res.append(dict(ctr_ref=ctr_ref.copy(), ctr_dev=ctr_dev, atom_ref=atom.copy(), atom_dev=dev_atom))
        if mode == 1:                       # binned mode never thins: flags are neither read nor kept
            _lib.check(lib.fl_debug_clear_hot(mgr.fb.ctx, dim.w, dim.h))
            hot[:] = 0
        _lib.check(lib.fl_debug_flush(mgr.fb.ctx, dim.w, dim.h))
        O.flush(d, atom, out4, hot)
        if mode == 1:
            _lib.check(lib.fl_debug_clear_hot(mgr.fb.ctx, dim.w, dim.h))
            hot[:] = 0
        res[-1].update(front_dev=mgr.fb.read('front', (nbins, 4), np.float32), front_ref=out4.copy(),
                       hot_dev=mgr.fb.read('hot', (nbins // 16,), np.uint32), hot_ref=hot.copy())
        r0 += nrounds + f
    dev_rng = mgr.fb.read('seeds', (nwalk + 64 * 256, 3), np.uint32)[:nwalk]
    dev_pts = mgr.fb.read('points', (nwalk, 4), np.float32)
    return res, (rng, points), (dev_rng, dev_pts), dim, seeds0


def run_device_model_gpu_only(mgr, gnm, prof, nrounds, fuse, mode, seeds_in=None):
    lib = _lib.load()
    if seeds_in is not None:
        mgr.fb.write('seeds', seeds_in)
    seeds0 = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    rdr, gprof, dim, g, ts, td = setup_frame(mgr, gnm, prof)
    nbins = dim.ah * dim.astride
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, dim.w, dim.h, 1))
    _lib.check(lib.fl_debug_iter_launch(mgr.fb.ctx, g, dim.w, dim.h, 0, nrounds + fuse, fuse, mode))
    ctr = np.zeros(4, np.uint64)
    _lib.check(lib.fl_debug_counters(mgr.fb.ctx, ctr.ctypes.data))
    atom = mgr.fb.read('atom', (nbins,), np.uint64)
    rng = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)[:walkers(mgr)[2]]
    return dict(ctr=ctr, atom=atom), None, rng, dim, seeds0


def density(front, dim):
    return front[:, 3].reshape(dim.ah, dim.astride).astype(np.float64)


def run_filter(mgr, name, dim, buf, vals):
    lib = _lib.load()
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, dim.w, dim.h, 0))
    mgr.fb.write('front', buf)
    arr = np.asarray(vals, np.float32)
    _lib.check(lib.fl_filter(mgr.fb.ctx, _lib.FILT[name], dim.w, dim.h, arr.ctypes.data, len(arr)))
    return mgr.fb.read('front', buf.shape, np.float32)


def assert_close(dev, ref, rtol, atol, what):
    assert np.isfinite(dev[np.isfinite(ref)]).all(), '%s: %d non-finite device values where the oracle is finite' % (
        what, (~np.isfinite(dev[np.isfinite(ref)])).sum())
    err = np.abs(dev - ref) - (atol + rtol * np.abs(ref))
    bad = err > 0
    assert not bad.any(), '%s: %d / %d out of tolerance, worst dev=%r ref=%r' % (
        what, bad.sum(), bad.size, dev.flat[np.argmax(err)], ref.flat[np.argmax(err)])


class env(object):
    """FLAME_* switches are read when a context is created (FLAME_RTC_FLAGS: when a kernel is compiled)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = dict((k, os.environ.get(k)) for k in self.kw)
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def same_bits(a, b, what, colour_exact=True, atomic=False, ref=None, min_lit=1000):
    """Counters, RNG states, walker points and the flushed density channel bit for bit.  The packed cells (FL_BUF_ATOM after the
    launch) and the colour sums are compared bit for bit too where no cell can have been drained on the way (fewer than 128
    hits in every pixel); a flame with hotter pixels — the fixed points of the three boxes hold 1e5 hits — drains full cells into
    the float accumulator in an order that is not reproducible between two runs of ONE kernel (see
    test_paired_halves_are_the_walkers_of_1024_four_wave_slots): there the colour sums are held to DESIGN §2's 2e-6.
    With direct atomics (``atomic``) a pixel that takes more than 512 hits in ONE round — the boxes' fixed points take thousands —
    can pass the cell's 10-bit count before the drain that a returning add asks for has run (iter.hip, "Every add returns the
    previous cell value"), with or without opacity.  ``ref`` is then the flushed density of the BINNED launch of the same genome
    from the same seeds (the binned accumulate keeps every sample, and the walk is the same walk): a cell that holds fewer than
    512 hits there never reaches the drain threshold, so on all those cells both atomic histograms must equal it exactly, and
    their colour sums each other to 2e-6 — at least ``min_lit`` lit cells of them (the three boxes' attractor lights only ~800
    cells in all, most of them hot: its callers ask for 20, and the atomic histogram with hidden samples is held cell for cell
    on zoomed cfg2 in test_fractional_opacity_atomic_histogram_where_cells_are_comparable).  Returns what was compared."""
    assert np.array_equal(a['ctr'][:3], b['ctr'][:3]), (what, a['ctr'], b['ctr'])
    assert np.array_equal(a['rng'], b['rng']), what
    assert np.array_equal(a['pts'], b['pts']), what
    nodrain = float(a['front'][:, 3].max()) < 128.0 and float(b['front'][:, 3].max()) < 128.0
    if atomic and not nodrain:
        assert ref is not None, what
        safe = ref < 512.0
        lit = int((ref[safe] > 0).sum())
        assert lit >= min_lit, (what, lit)
        for r in (a, b):
            assert np.array_equal(r['front'][safe, 3], ref[safe]), what
        np.testing.assert_allclose(a['front'][safe, :3], b['front'][safe, :3], rtol=2e-6, atol=1e-4, err_msg=str(what))
        return 'cells below the drain threshold: %d' % lit
    assert np.array_equal(a['front'][:, 3], b['front'][:, 3]), what
    if nodrain:
        assert int(a['ctr'][3]) == 0 and int(b['ctr'][3]) == 0, (what, a['ctr'], b['ctr'])
        assert np.array_equal(a['atom'], b['atom']), what
    if nodrain and colour_exact:
        assert np.array_equal(a['front'].view(np.uint32), b['front'].view(np.uint32)), what
    else:       # (records grouped differently: the order of float additions may move, DESIGN §2 "binned == atomic")
        np.testing.assert_allclose(a['front'][:, :3], b['front'][:, :3], rtol=2e-6, atol=1e-4, err_msg=str(what))
    return 'every cell, packed cells too' if nodrain else 'every cell'


def launch(m, gnm, prof, mode, nrounds, fuse, seeds_in=None, points_in=None):
    """One counted iterate launch from cleared buffers — and NaN points, or ``points_in`` — then the flush: everything the
    launch left behind (walkers with their fourth word; `rdr` and `g` are only good while `m` lives)."""
    lib = _lib.load()
    if seeds_in is not None:
        m.fb.write('seeds', seeds_in)
    seeds0 = m.fb.read('seeds', (m.fb.nwalkers, 3), np.uint32)
    rdr, gprof, dim, g, ts, td = setup_frame(m, gnm, prof)
    nbins = dim.ah * dim.astride
    nwalk = m.fb.nslots * m.fb.nthreads
    _lib.check(lib.fl_debug_clear(m.fb.ctx, dim.w, dim.h, 1 if points_in is None else 0))
    if points_in is not None:
        m.fb.write('points', points_in)
    _lib.check(lib.fl_debug_iter_launch(m.fb.ctx, g, dim.w, dim.h, 0, nrounds + fuse, fuse, mode))
    ctr = np.zeros(4, np.uint64)
    _lib.check(lib.fl_debug_counters(m.fb.ctx, ctr.ctypes.data))
    atom = m.fb.read('atom', (nbins,), np.uint64)
    rng = m.fb.read('seeds', (m.fb.nwalkers, 3), np.uint32)[:nwalk]
    pts = m.fb.read('points', (nwalk, 4), np.float32).view(np.uint32).copy()
    params = m.fb.read('params', (1024, rdr.packer.pstride), np.float32, g)
    _lib.check(lib.fl_debug_flush(m.fb.ctx, dim.w, dim.h))
    front = m.fb.read('front', (nbins, 4), np.float32)
    return dict(ctr=ctr, atom=atom, rng=rng, pts=pts, front=front, seeds0=seeds0, dim=(dim.ah, dim.astride),
                samples=nrounds * nwalk, params=params, prog=rdr.packer.prog, rdr=rdr, g=g)


def snapshot(gnm, prof, mode, nw=4, nslots=1024, nrounds=29, fuse=5, seeds_in=None, **switches):
    """A launch in a context of its own geometry and switches."""
    with env(FLAME_NW=None if nw == 4 else str(nw), **switches):
        m = render.RenderManager(device=0, nslots=nslots, host_seed=44)
        assert (m.fb.nw, m.fb.nslots) == (nw, nslots), ((m.fb.nw, m.fb.nslots), (nw, nslots))
        try:
            return launch(m, gnm, prof, mode, nrounds, fuse, seeds_in)
        finally:
            m.fb.free()


def iterate_frame(m, gnm, prof, tc, nsamples, geometry_by_samples=False):
    lib = _lib.load()
    gprof = profile.wrap(prof, gnm)
    rdr = render.Renderer(gnm, gprof)
    dim = m.fb.set_dim(gprof.width, gprof.height, nsamples=nsamples if geometry_by_samples else None)
    g = rdr._handle(m.fb)
    ts, td = frame_times(gprof, tc)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(m.fb.ctx, C.byref(fid)))
    m._copy(rdr, gnm)
    _lib.check(lib.fl_interp(m.fb.ctx, g, dim.w, dim.h, ts, td))
    run = C.c_uint64()
    mode = m.resolve_accum_mode(dim)
    assert mode == _lib.ACCUM_BINNED, mode
    _lib.check(lib.fl_iterate(m.fb.ctx, g, dim.w, dim.h, float(nsamples), m.fuse, mode, C.byref(run)))
    front = m.fb.read('front', (dim.ah * dim.astride, 4), np.float32)
    return rdr, gprof, dim, td, run.value, front


def blocks(dens, bs):
    H, W = dens.shape[0] // bs * bs, dens.shape[1] // bs * bs
    return dens[:H, :W].reshape(H // bs, bs, W // bs, bs).sum((1, 3))


def check_against_cpu_game(gnm, prof, tc, nslots, dim, front, nrun, ncpu, bs, l1_max, frac_tol, col_tol, nthreads=16):
    dens = front[:, 3].reshape(dim.ah, dim.astride).astype(np.float64)
    assert np.array_equal(dens, np.rint(dens)) and dens.min() >= 0, 'density must hold integer counts'
    assert dens.sum() <= nrun, (dens.sum(), nrun)
    F = prepare(gnm, prof, tc, nslots=nslots)
    ref, secs, acc = O.flam3_render(F['dim'], F['packer'].prog, F['params'], F['palette'], F['seeds'], ncpu, nthreads)    # one private float4 histogram per thread
    dr = ref[:, 3].reshape(dim.ah, dim.astride).astype(np.float64)
    fg, fr = dens.sum() / nrun, dr.sum() / ncpu
    assert abs(fg - fr) < frac_tol, ('in-frame fraction', fg, fr)
    bg, br = blocks(dens, bs), blocks(dr, bs)
    l1 = np.abs(bg / bg.sum() - br / br.sum()).sum()
    # shot noise of the smaller (CPU) sample alone contributes ~ sum_b sqrt(2 p_b / (pi n)) to the L1
    p = br / br.sum()
    noise = np.sqrt(2.0 * p / (np.pi * max(dr.sum(), 1.0))).sum()
    assert l1 < l1_max + 1.5 * noise, ('block L1', l1, 'shot-noise floor', noise)
    cg = front[:, :3].sum(0, dtype=np.float64) / dens.sum()
    cr = ref[:, :3].sum(0, dtype=np.float64) / dr.sum()
    assert np.abs(cg - cr).max() < col_tol, ('mean colour', cg, cr)
    return l1, noise, fg, fr


# Bars of the full-size filter chain (tone-mapped values in [0, 1]).  Measured (gpurun_out/fullsize_chain_errors.txt,
# tools/diag_chain_error.py): cfg2 / cfg3 whole 1080p frames max 2.2e-5 / 2.3e-5, 99.9 % below 1.2e-6, mean 4e-8; the
# 4K / 8K windows max 1.7e-6 / 6.4e-6.  The maximum sits at single-hit pixels at the rim of the flame, where
# colorclip's linear segment below `gamma_threshold` multiplies differences by lin^(gamma - 1) = 31.6; above a DE
# density of 10 the relative error of the DE output itself is 3e-6.  The bars are ~4x the worst measured values
# (round 2 asked for max < 2e-2): hardware exp / log / rcp on one side, libm on the other.
CHAIN_MAX, CHAIN_P999, CHAIN_MEAN = 1e-4, 5e-6, 5e-7


def check_chain_error(err, what):
    stats = (float(err.max()), float(np.percentile(err, 99.9)), float(err.mean()))
    try:
        import os
        if os.path.isdir('gpurun_out'):
            with open('gpurun_out/fullsize_chain_errors.txt', 'a') as fp:
                fp.write('%s: max %.3e p99.9 %.3e mean %.3e\n' % ((what,) + stats))
    except OSError:
        pass
    assert stats[0] < CHAIN_MAX and stats[1] < CHAIN_P999 and stats[2] < CHAIN_MEAN, (what,) + stats
    return stats


def filter_chain_on_device(m, rdr, gprof, dim, tc):
    vals = {}
    for filt in rdr.filts:
        vals[filt.name] = [float(v) for v in filt.scalars(gprof, getattr(gprof.filters, filt.name), dim, tc)]
        filt.apply(m.fb, gprof, getattr(gprof.filters, filt.name), dim, tc)
    assert [f.name for f in rdr.filts] == ['yuv', 'bilateral', 'logscale', 'colorclip'], [f.name for f in rdr.filts]
    dev = m.fb.read('front', (dim.ah * dim.astride, 4), np.float32)
    assert np.isfinite(dev).all(), '%d non-finite values after the chain' % (~np.isfinite(dev)).sum()
    return vals, dev


def oracle_chain(d, buf, vals):
    cur = O.yuv_to_rgb(d, np.ascontiguousarray(buf))
    cur = O.bilateral_chain(d, cur, *vals['bilateral'])
    cur = O.logscale(d, cur, *vals['logscale'])
    return O.colorclip(d, cur, *vals['colorclip'])


def pack_digest(pk):
    import hashlib
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(pk.prog, np.int32).tobytes())
    h.update(np.ascontiguousarray(pk.ops_array, np.int32).tobytes())
    h.update(json.dumps([['.'.join(p), bool(m)] for p, m in pk.rows]).encode())
    h.update(json.dumps(['.'.join(p) for p in pk.packed]).encode())
    return h.hexdigest()[:32]


def compile_check(gnm, nw, count, acc):
    pk = GenomePacker(gnm)
    prog = np.ascontiguousarray(pk.prog, np.int32)
    ops = np.ascontiguousarray(pk.ops_array, np.int32)
    log = C.create_string_buffer(8192)
    rc = _lib.load().fl_rtc_compile_check(prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), nw, count, acc, log, len(log))
    if rc == _lib.FL_E_UNSUPPORTED:
        pytest.skip('libhiprtc is not installed')
    return rc, log.value.decode()


def kernel_resources(tmp_path):
    readelf = '/opt/rocm/lib/llvm/bin/llvm-readelf'
    if not os.path.exists(readelf):
        pytest.skip('no llvm-readelf')
    co = str(tmp_path / 'k_iter_spec.co')
    notes = subprocess.run([readelf, '--notes', co], capture_output=True, text=True, timeout=60).stdout
    num = lambda key: int(re.search(r'\.' + key + r':\s+(\d+)', notes).group(1))
    sect = subprocess.run([readelf, '-S', co], capture_output=True, text=True, timeout=60).stdout
    text = int(re.search(r'\.text\s+PROGBITS\s+\S+\s+\S+\s+([0-9a-f]+)', sect).group(1), 16)
    return dict(vgpr=num('vgpr_count'), sgpr=num('sgpr_count'), spill=num('vgpr_spill_count'), sgpr_spill=num('sgpr_spill_count'),
                scratch=num('private_segment_fixed_size'), lds=num('group_segment_fixed_size'), text=text)


def check_random_genome(mgr, mgr_prod, seed):
    """The body of test_gpu_random_genomes.test_random_genome_parity, for the test and for tools/soak_random_genomes.py."""
    lib = _lib.load()
    gnm, prof = random_genome(seed)
    if seed % 2 == 1:                       # animated genomes run in the geometry that ships
        mgr = mgr_prod
        assert mgr.fb.nslots == 1536, mgr.fb.nslots
    gprof = profile.wrap(prof, gnm)
    rdr = render.Renderer(gnm, gprof)
    g = rdr._handle(mgr.fb)
    mgr._copy(rdr, gnm)
    dim = mgr.fb.calc_dim(gprof.width, gprof.height)
    tc = 0.37
    ts, td = frame_times(gprof, tc)
    _lib.check(lib.fl_interp(mgr.fb.ctx, g, dim.w, dim.h, ts, td))
    dev = mgr.fb.read('params', (mgr.fb.nslots, rdr.packer.pstride), np.float32, g)
    F = prepare(gnm, prof, tc, nslots=mgr.fb.nslots)
    ref = F['params']
    names = ['.'.join(n) for n in rdr.packer.packed]
    lastden = names.index('den.' + rdr.packer.xform_keys[-1])
    assert np.all(dev[:, lastden] >= 1.0), dev[:, lastden].min()
    dev[:, lastden] = ref[:, lastden]
    structural = np.array([n.split('.')[-1].startswith('#') or n.startswith('pad') for n in names])
    assert np.array_equal(dev[:, structural].view(np.uint32), ref[:, structural].view(np.uint32)), 'structure words'
    err = np.abs(dev - ref)[:, ~structural] / (np.abs(ref[:, ~structural]) + 1.0)
    i = np.unravel_index(np.argmax(err), err.shape)
    assert err.max() < 5e-5, (np.array(names)[~structural][i[1]], err.max())

    # short iterate vs the flam3-style game on the oracle's blocks
    n = 2 ** 24
    run = C.c_uint64()
    _lib.check(lib.fl_iterate(mgr.fb.ctx, g, dim.w, dim.h, float(n), mgr.fuse, 1, C.byref(run)))     # the default schedule (fuse 256)
    nbins = dim.ah * dim.astride
    front = mgr.fb.read('front', (nbins, 4), np.float32).astype(np.float64)
    assert np.isfinite(front).all(), '%d non-finite accumulator values' % (~np.isfinite(front)).sum()
    refh, _, _ = O.flam3_render(F['dim'], F['packer'].prog, F['params'], F['palette'], F['seeds'], n, 8)
    refh = refh.astype(np.float64)
    fg, fr = front[:, 3].sum() / run.value, refh[:, 3].sum() / n
    assert abs(fg - fr) < 0.01 + 0.02 * fr, (fg, fr)
    if fr > 0.02:
        cg, cr = front[:, :3].sum(0) / front[:, 3].sum(), refh[:, :3].sum(0) / refh[:, 3].sum()
        assert np.abs(cg - cr).max() < 2.5 / 255, (cg, cr)
        H, W = dim.ah // 16 * 16, dim.astride // 16 * 16
        def blocks(a):
            return a[:, 3].reshape(dim.ah, dim.astride)[:H, :W].reshape(H // 16, 16, W // 16, 16).sum((1, 3))
        bg, br = blocks(front), blocks(refh)
        l1 = np.abs(bg / bg.sum() - br / br.sum()).sum()
        # the bar is the shot-noise floor of the two samples, sum over blocks of sqrt(2 / pi * p * (1/Ng + 1/Nr)), times 3
        # (wave-coherent xform choice and the CPU game's eight long trajectories are both clustered samples: block z-scores
        # of 1.0-1.2 against an independent game) plus 2 % — as tests/test_gpu_fullsize.py; round 3: 5 % flat
        p = br / br.sum()
        floor = np.sqrt(2 / np.pi * p * (1.0 / bg.sum() + 1.0 / br.sum())).sum()
        assert l1 < 0.02 + 3 * floor, (l1, floor)
