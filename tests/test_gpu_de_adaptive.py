"""
The `de` filter (flam3-style adaptive density estimation) on the GPU: the HIP kernel through
fl_filter against the numpy model of tests/de_model.py, its energy and pass-through properties, determinism,
whole frames through RenderManager.queue_frame, and the reach the sample-sharded band path relies on.
"""
import ctypes as C

import numpy as np
import pytest

from common import frame_times
from de_model import de_filter
from cuburn_amd import _lib, configs, profile, render
from accum_inputs import fractional_band_accum as accum
from gpu_harness import run_filter

pytestmark = pytest.mark.gpu

FW, FH = 200, 120
DE_ORDER = ['de', 'logscale', 'smearclip']


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    yield m
    m.fb.free()


@pytest.mark.parametrize('R,minimum,curve', [(11, 0, 0.6), (4.5, 0.5, 0.4), (23, 0.1, 1.0), (96, 0, 0.6)])
def test_de_matches_model(mgr, R, minimum, curve):
    dim = mgr.fb.calc_dim(FW, FH)
    buf = accum(dim)
    vals = [np.float32(R), np.float32(minimum * R), np.float32(curve)]
    dev = run_filter(mgr, 'de', dim, buf.reshape(-1, 4), vals).reshape(buf.shape).astype(np.float64)
    ref = de_filter(buf, *vals)
    assert np.isfinite(dev).all()
    for ch in range(4):
        err = np.abs(dev[..., ch] - ref[..., ch]) - (2e-5 * np.abs(ref[..., ch]) + 1e-6 * ref[..., ch].max())
        assert not (err > 0).any(), (ch, (err > 0).sum(), dev[..., ch].flat[np.argmax(err)], ref[..., ch].flat[np.argmax(err)])


@pytest.mark.parametrize('R,minimum,curve', [(11, 0, 0.6), (23, 0.1, 1.0)])
def test_de_conserves_energy(mgr, R, minimum, curve):
    dim = mgr.fb.calc_dim(FW, FH)
    buf = accum(dim, seed=2)
    edge = int(np.ceil(R))
    buf[:edge] = 0; buf[-edge:] = 0; buf[:, :edge] = 0; buf[:, -edge:] = 0
    dev = run_filter(mgr, 'de', dim, buf.reshape(-1, 4), [R, minimum * R, curve]).reshape(buf.shape)
    assert not np.array_equal(dev, buf)
    s0, s1 = buf.astype(np.float64).sum((0, 1)), dev.astype(np.float64).sum((0, 1))
    assert np.allclose(s1, s0, rtol=1e-5, atol=0), (s0, s1)


def test_de_copies_when_nothing_spreads(mgr):
    dim = mgr.fb.calc_dim(FW, FH)
    buf = accum(dim, seed=3)
    flat = buf.reshape(-1, 4)
    assert np.array_equal(run_filter(mgr, 'de', dim, flat, [0.0, 0.0, 0.6]), flat)           # R <= 0
    dense = buf.copy()
    dense[..., 3] += 300.0                                   # 11 * 300^-0.6 < 1: every h < 1
    flat = dense.reshape(-1, 4)
    assert np.array_equal(run_filter(mgr, 'de', dim, flat, [11.0, 0.0, 0.6]), flat)


def test_de_deterministic(mgr):
    dim = mgr.fb.calc_dim(FW, FH)
    flat = accum(dim, seed=4).reshape(-1, 4)
    a = run_filter(mgr, 'de', dim, flat, [23.0, 0.0, 0.6])
    b = run_filter(mgr, 'de', dim, flat, [23.0, 0.0, 0.6])
    assert np.array_equal(a, b) and not np.array_equal(a, flat)


def test_de_rejects_bad_parameters(mgr):
    dim = mgr.fb.calc_dim(FW, FH)
    flat = accum(dim).reshape(-1, 4)
    with pytest.raises(ValueError, match='curve'):
        run_filter(mgr, 'de', dim, flat, [11.0, 0.0, 0.0])
    with pytest.raises(ValueError, match='96'):
        run_filter(mgr, 'de', dim, flat, [97.0, 0.0, 0.6])


def render_small(order, seed):
    gnm, prof = configs.cfg2(samples=2 ** 22)
    gprof = profile.wrap(dict(prof, width=320, height=240, filter_order=order), gnm)
    m = render.RenderManager(device=0, host_seed=seed)
    try:
        evt, h = m.queue_frame(render.Renderer(gnm, gprof), gnm, gprof, 0.5)
        evt.synchronize()
        return np.array(h)
    finally:
        m.fb.free()


def test_de_whole_frame():
    a = render_small(DE_ORDER, 7)
    assert a.shape[:2] == (240, 320)
    f = a.astype(np.float64)
    assert np.isfinite(f).all() and f[..., :3].max() > 0
    assert not np.array_equal(a, render_small(['logscale', 'smearclip'], 7))
    assert np.array_equal(a, render_small(DE_ORDER, 7))


def test_de_band_filtering_matches_whole_frame(built):
    """As test_gpu_parity.test_band_filtering_matches_whole_frame, with the `de` chain at a radius near the cap: the
    halo (224 rows) covers the chain's reach (96 + 9), so the stitched bands are the whole frame."""
    import torch
    from cuburn_amd import distributed as D
    gnm, prof = configs.cfg2()
    prof = dict(prof, spp=2 ** 26 / (1920.0 * 1080.0), filter_order=DE_ORDER, filters={'de': {'radius': 90 / 11.}})
    gprof = profile.wrap(prof, gnm)
    m = render.RenderManager(device=0, host_seed=9)
    rdr = render.Renderer(gnm, gprof)
    lib = _lib.load()
    tc = 0.5
    dim = m.fb.set_dim(gprof.width, gprof.height)
    R = rdr.filts[1].scalars(gprof, gprof.filters.de, dim, tc)[0]
    assert 89 < R <= 96
    ts, td = frame_times(gprof, tc)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(m.fb.ctx, C.byref(fid)))
    m._copy(rdr, gnm)
    g = rdr._handle(m.fb)
    _lib.check(lib.fl_interp(m.fb.ctx, g, dim.w, dim.h, ts, td))
    run = C.c_uint64()
    _lib.check(lib.fl_iterate(m.fb.ctx, g, dim.w, dim.h, float(2 ** 26), m.fuse, m.resolve_accum_mode(dim), C.byref(run)))
    acc = m.fb.read('front', (dim.ah, dim.astride * 4), np.float32)
    for filt in rdr.filts:
        filt.apply(m.fb, gprof, getattr(gprof.filters, filt.name), dim, tc)
    whole = m.fb.read('front', (dim.ah, dim.astride * 4), np.float32)
    assert whole.max() > 0.5

    assert D.band_path_ok(rdr.out, dim, [f.name for f in rdr.filts])
    plan = D.band_plan(dim.ah, 2)
    stitched = np.zeros_like(whole)
    for r0, r1 in plan[1]:
        top = D.BAND_HALO if r0 > 0 else 0
        band = torch.from_numpy(acc[r0 - top:min(r1 + D.BAND_HALO, dim.ah)].copy()).cuda()
        _, bdim = D.filter_band(m, rdr, gprof, dim, band, tc, 0, convert=False)
        res = m.fb.read('front', (bdim.ah, dim.astride * 4), np.float32)
        stitched[r0:r1] = res[top:top + (r1 - r0)]
    err = np.abs(stitched - whole)
    assert err.max() < 2e-5, (err.max(), err.mean())
    m.fb.free()
