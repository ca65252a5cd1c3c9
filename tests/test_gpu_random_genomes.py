    # (seed 226 — handkerchief + perspective + rings2, from the soak of seeds 221-260: block L1 0.20 against 8
    # trajectories, 0.049 against 64, 0.033 against 512, 0.0235 against 4096 and below the bar against 65536 trajectories
    # of 1024 iterations)
"""
Randomised genomes through the C ABI: the structure of the genome is data here (one precompiled
interpreter kernel), so parity must hold for ANY structure, not just the BASELINE configs.
A seeded generator draws xform counts, variation sets (with parameters), post affines, final
xforms, animated ([p0, v0, p1, v1] + extra knots) splines and two palettes; for each genome:
  * the interpolated parameter blocks (one per walker slot) agree with the oracle's by-name float64 restatement;
  * every word of the block that is not a spline / precalc value is exactly the structure the
    program says (variation numbers, counts, zero padding);
  * a short iterate lands the same fraction of samples in frame as the oracle's flam3-style game
    driven by the ORACLE's parameter blocks, with matching mean colour (distributional, since
    random variations use hardware transcendentals).
48 seeds are committed; seeds 17-336 were run once by hand (tools/diag_random_seed.py, DESIGN.md §5 'Fuse'):
that run found the point-attractor overflow of the tile accumulate (fixed; test_gpu_parity.py
test_binned_point_attractor_keeps_every_sample) and six single-xform genomes that are not a fair
comparison (a lone map does not mix: eight CPU trajectories are not a distribution).
"""
import numpy as np
import pytest

from common import O, prepare
from cuburn_amd import configs, profile, render, _lib
from cuburn_amd.genome import variations as V
from flames import random_genome
from gpu_harness import check_random_genome

pytestmark = pytest.mark.gpu
NSLOTS = 1024


@pytest.fixture(scope='module')
def mgr():
    from __graft_entry__ import build
    build()
    return render.RenderManager(device=0, nslots=NSLOTS, host_seed=23)


@pytest.fixture(scope='module')
def mgr_prod(mgr):
    """Production geometry (RenderManager() defaults: 1536 slots): used for the animated genomes."""
    return render.RenderManager(device=0, host_seed=23)


def _seeds():
    """1 .. 48 by default; FLAME_SOAK_SEEDS=a-b widens the range for a soak run (profiles/r06_soak_random_genomes.txt: 49-248)."""
    import os
    e = os.environ.get('FLAME_SOAK_SEEDS')
    if e:
        a, b = e.split('-')
        return list(range(int(a), int(b) + 1))
    return list(range(1, 49))


@pytest.mark.parametrize('seed', _seeds())
def test_random_genome_parity(mgr, mgr_prod, seed):
    check_random_genome(mgr, mgr_prod, seed)


def _blocks16(a, dim):
    H, W = dim.ah // 16 * 16, dim.astride // 16 * 16
    return a.reshape(dim.ah, dim.astride)[:H, :W].reshape(H // 16, 16, W // 16, 16).sum((1, 3))


# Genomes of ONE xform: a lone map converges to its orbit at its own contraction rate, with no averaging
# over xform choices — the class for which a fuse of 64 was measurably too short (seed 209: cross + fan2 +
# linear, block L1 0.11 at fuse 64, 0.010 at 256).  Everything here runs at RenderManager's DEFAULTS,
# through queue_frame: no explicit fuse, production slots (1024 of them for these sample counts).  The CPU sample
# uses 4096 trajectories (eight trajectories of a map that does not mix are not a distribution, and 64 are a poor
# one: seed 176, cell + julian, is 0.046 from a 64-trajectory sample and 0.021 from 4096 — the error of the CPU
# sample's basin weights); the two seeds that mix least get 65536 short trajectories, a sample made like the GPU's.
@pytest.mark.parametrize('seed', [209, 41, 48, 50, 102, 110, 176, 226, 270, 278, 295])
def test_single_xform_genome_default_schedule(seed):
    gnm, prof = random_genome(seed)
    assert len(gnm['xforms']) == 1
    prof = dict(prof, filter_order=[])                       # the accumulator itself is compared
    gprof = profile.wrap(prof, gnm)
    m = render.RenderManager(device=0, host_seed=23)
    assert m.fuse == 256 and m.fb.nslots == 1536             # cuburn/render.py:215 (1536 until the first frame's sample count is known)
    rdr = render.Renderer(gnm, gprof)
    tc = 0.37
    evt, _ = m.queue_frame(rdr, gnm, gprof, tc)
    evt.synchronize()
    dim = m.fb.calc_dim(gprof.width, gprof.height)
    dens = m.fb.read('front', (dim.ah * dim.astride, 4), np.float32).astype(np.float64)[:, 3]
    nrun = m.last_nsamples
    F = prepare(gnm, prof, tc, nslots=m.fb.nslots)
    n = 2 ** 26
    # (seed 226 — handkerchief + perspective + rings2, from the soak of seeds 221-260 — mixes even less: block L1 0.20
    # against 8 trajectories, 0.049 against 64, 0.033 against 512, 0.0235 against 4096 and below the bar against 65536
    # trajectories of 1024 iterations, i.e. against a CPU sample made the way the GPU's is: many short orbits)
    refh, _, _ = O.flam3_render(F['dim'], F['packer'].prog, F['params'], F['palette'], F['seeds'], n, 65536 if seed in (226, 176) else 4096)
    refd = refh.astype(np.float64)[:, 3]
    fg, fr = dens.sum() / nrun, refd.sum() / n
    assert abs(fg - fr) < 0.005 + 0.01 * fr, (fg, fr)
    if fr > 0.02:
        bg, br = _blocks16(dens, dim), _blocks16(refd, dim)
        l1 = np.abs(bg / bg.sum() - br / br.sum()).sum()
        # shot noise of both samples: sum over blocks of sqrt(2 / pi * p * (1/Ng + 1/Nr))
        p = br / br.sum()
        floor = np.sqrt(2 / np.pi * p * (1.0 / dens.sum() + 1.0 / refd.sum())).sum()
        assert l1 < 0.02 + 3 * floor, (l1, floor)
    m.fb.free()


def _variation_genome(names):
    """One xform per variation (plus a little linear so that points keep moving), default parameters."""
    xforms = {}
    for i, n in enumerate(names):
        var = {n: dict([(k, dv if dv else 0.6) for k, (dv, _) in V.var_params[n].items()], weight=0.6)}
        if n != 'linear':
            var['linear'] = {'weight': 0.4}
        xforms['%02d' % i] = {'weight': 1.0, 'color': i / max(len(names) - 1, 1), 'color_speed': 0.5,
                              'pre_affine': configs._affine(17.0 * i, 0.7, 0.3 * np.cos(i), 0.3 * np.sin(i)),
                              'variations': var}
    gnm = {'type': 'animation', 'name': 'vars', 'camera': {'center': {'x': 0.0, 'y': 0.0}, 'rotation': 0.0, 'scale': 0.25},
           'time': {'duration': 1, 'frame_width': 0.0}, 'palette': [[0.0] + configs.palette_encode(configs.grey_ramp())],
           'xforms': xforms}
    prof = {'width': 384, 'height': 216, 'spp': 100.0, 'fps': 1, 'duration': 1, 'frame_width': 0.0,
            'output': {'type': 'raw'}, 'filter_order': ['bilateral', 'logscale', 'colorclip']}
    return gnm, prof


ALL_VARS = sorted(V.var_ids, key=lambda n: V.var_ids[n])


@pytest.mark.parametrize('chunk', list(range(0, len(ALL_VARS), 8)))
def test_every_variation_per_genome_kernel_equals_interpreter(chunk, monkeypatch):
    """All 95 variations, eight per genome: the kernel compiled for the genome's structure (hipRTC)
    and the precompiled interpreter kernel (FLAME_RTC=0) leave identical RNG states, walker points,
    sample counters and per-cell densities — the specialisation inlines every variation body with a constant
    id where the interpreter calls one out-of-line function, and must not change a single bit."""
    lib = _lib.load()
    names = ALL_VARS[chunk:chunk + 8]
    gnm, prof = _variation_genome(names)
    gprof = profile.wrap(prof, gnm)
    out = {}
    for rtc in ('0', '1'):
        monkeypatch.setenv('FLAME_RTC', rtc)
        m = render.RenderManager(device=0, nslots=NSLOTS, host_seed=5)
        rdr = render.Renderer(gnm, gprof)
        g = rdr._handle(m.fb)
        m._copy(rdr, gnm)
        dim = m.fb.calc_dim(gprof.width, gprof.height)
        _lib.check(lib.fl_interp(m.fb.ctx, g, dim.w, dim.h, 0.5, 0.0))
        _lib.check(lib.fl_debug_clear(m.fb.ctx, dim.w, dim.h, 1))
        _lib.check(lib.fl_debug_iter_launch(m.fb.ctx, g, dim.w, dim.h, 0, 20, 4, 1))
        ctr = np.zeros(4, np.uint64)
        _lib.check(lib.fl_debug_counters(m.fb.ctx, ctr.ctypes.data))
        _lib.check(lib.fl_debug_flush(m.fb.ctx, dim.w, dim.h))
        out[rtc] = (ctr, m.fb.read('seeds', (m.fb.nwalkers, 3), np.uint32),
                    m.fb.read('points', (NSLOTS * 256, 4), np.float32),
                    m.fb.read('front', (dim.ah * dim.astride, 4), np.float32))
        m.fb.free()
    (ca, ra, pa, fa), (cb, rb, pb, fb) = out['0'], out['1']
    assert np.array_equal(ca, cb), (names, ca, cb)
    assert np.array_equal(ra, rb), names
    both_nan = np.isnan(pa) & np.isnan(pb)
    assert np.array_equal(pa.view(np.uint32)[~both_nan], pb.view(np.uint32)[~both_nan]), names
    # densities are integers (exact); colour sums are float atomics whose order varies run to run
    assert np.array_equal(fa[:, 3], fb[:, 3]), names
    assert np.allclose(fa[:, :3], fb[:, :3], rtol=1e-5, atol=1e-5), names
