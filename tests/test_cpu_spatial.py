"""
CPU tests (no GPU) of the `spatial` filter's host side: the taps against the float64 model of tests/spatial_model.py, the
chain's placement rules, the supersample bookkeeping of logscale, the schema / profile / command-line plumbing and the ABI
declaration.  The kernel itself: tests/test_gpu_spatial.py.
"""
import argparse
import os
import re

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, filters, profile, render
from cuburn_amd.genome import specs
import spatial_model as SM

# (supersample, radius) -> taps per axis, worked out by hand from the definition
TABLE = {(1, 0.5): 3, (2, 0.5): 4, (2, 1): 8, (3, 1): 11, (4, 1): 14, (4, 2): 26}


def wrapped(**prof_kw):
    gnm, prof = configs.cfg2()
    return gnm, profile.wrap(dict(prof, **prof_kw), gnm)


@pytest.mark.parametrize('ss,radius', sorted(TABLE))
def test_taps_equal_the_model(ss, radius):
    t = filters.spatial_taps(radius, ss)
    m = SM.taps(radius, ss)
    assert t.dtype == np.float32 and len(t) == TABLE[(ss, radius)] == len(m) == SM.ntaps(radius, ss)
    assert np.array_equal(t, m.astype(np.float32))
    assert np.array_equal(t, t[::-1]) and (t > 0).all()                     # symmetric
    assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 4 * 2.0 ** -24 * len(t)
    assert (len(t) - ss) % 2 == 0 and t.argmax() in (len(t) // 2, (len(t) - 1) // 2)


def test_model_separable_form_is_the_double_sum():
    rs = np.random.RandomState(5)
    ss, t = 3, rs.uniform(-1, 1, 9)
    din, dout = render.Framebuffers.calc_dim(3 * 5, 3 * 3), render.Framebuffers.calc_dim(5, 3)
    src = rs.uniform(-1, 1, (din.ah * din.astride, 4))
    out, A = SM.resample(src, din, dout, ss, t)
    bins = [(0, 0), (dout.astride - 1, dout.ah - 1), (12, 12), (16, 14), (31, 0), (3, 20), (20, 31)]
    ref = SM.resample_direct(src, din, dout, ss, t, bins)
    for (X, Y), r in zip(bins, ref):
        assert np.abs(out[Y, X] - r).max() <= 1e-13 * max(A[Y, X].max(), 1e-300), (X, Y)
    assert (A >= np.abs(out) - 1e-13).all()


def test_tap_limits():
    for ss in (1, 2, 3, 4):
        t = filters.spatial_taps(0, ss)                                     # radius 0: the pixel's own ss x ss bins and no more
        assert len(t) == ss and np.array_equal(t, SM.taps(0, ss).astype(np.float32)) and np.array_equal(t, t[::-1])
    assert filters.spatial_taps(0, 1)[0] == 1 and np.array_equal(filters.spatial_taps(0, 2), [0.5, 0.5])
    # the footprint may overhang an output pixel by the 12-bin gutter per side: n <= ss + 24
    with pytest.raises(ValueError) as e:
        filters.spatial_taps(3, 4)
    assert '38' in str(e.value) and '28' in str(e.value) and 'radius 3' in str(e.value) and 'supersample 4' in str(e.value)
    # radius 2.3 at supersample 4: fw = 27.6, n = 28 = ss + 24 taps — the limit itself, the widest filter there is;
    # the first radius past it (12 r >= 28) is refused
    assert len(filters.spatial_taps(2.3, 4)) == 28 == SM.ntaps(2.3, 4)
    for radius in (2.34, 2.5):
        with pytest.raises(ValueError):
            filters.spatial_taps(radius, 4)
    assert len(filters.spatial_taps(8.3, 1)) == 25 and len(filters.spatial_taps(4.16, 2)) == 26
    with pytest.raises(ValueError):
        filters.spatial_taps(8.4, 1)
    for bad in (0, 5, 1.5, True):
        with pytest.raises(ValueError):
            filters.spatial_taps(1.0, bad)
    for bad in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            filters.spatial_taps(bad, 2)
    # supersample 1: flam3's plain filter — 3 taps at radius 0.5, 5 at the default camera.dither_width of 1
    assert len(filters.spatial_taps(0.5, 1)) == 3 and len(filters.spatial_taps(1.0, 1)) == 5


def names(gprof):
    return [f.name for f in filters.create(gprof)]


def test_create_placement():
    base = ['yuv', 'bilateral', 'logscale', 'colorclip']
    assert names(wrapped()[1]) == base                                       # supersample 1, not listed: today's chain
    assert names(wrapped(supersample=1)[1]) == base
    assert names(wrapped(supersample=2)[1]) == base + ['spatial']            # appended last: flam3's early clip
    late = ['de', 'logscale', 'spatial', 'colorclip']
    assert names(wrapped(supersample=3, filter_order=late)[1]) == ['yuv'] + late      # runs where it is listed
    assert names(wrapped(filter_order=late)[1]) == ['yuv'] + late            # supersample 1, listed: the plain spatial filter
    with pytest.raises(ValueError):
        filters.create(wrapped(supersample=2, filter_order=['spatial', 'logscale', 'spatial'])[1])
    for bad in (0, 5, 2.5):
        with pytest.raises(ValueError):
            filters.create(wrapped(supersample=bad)[1])
    assert isinstance(filters.create(wrapped(supersample=2)[1])[-1], filters.Spatial)
    assert filters.Filter.filter_map['spatial'] is filters.Spatial and filters.Spatial.name == 'spatial'


def test_logscale_counts_the_bins_of_a_pixel():
    tc = 0.3
    gnm, g1 = wrapped()
    dim = render.Framebuffers.calc_dim(g1.width, g1.height)
    lf = filters.Logscale()
    k1, k2 = lf.scalars(g1, g1.filters.logscale, dim, tc)
    # today's value, restated
    area = dim.h / (g1.filters.logscale.scale(tc) ** 2 * dim.w)
    assert k2 == np.float32(1.0 / (area * g1.spp(tc))) and k1 == np.float32(g1.filters.logscale.brightness(tc) * 268 / 256)
    assert lf.scalars(wrapped(supersample=1)[1], g1.filters.logscale, dim, tc) == [k1, k2]
    for ss in (2, 3, 4):
        gs = wrapped(supersample=ss)[1]
        for d in (dim, render.Framebuffers.calc_dim(ss * g1.width, ss * g1.height)):       # either side of `spatial`
            s1, s2 = lf.scalars(gs, gs.filters.logscale, d, tc)
            assert s1 == k1 and type(s2) is np.float32 and s2 == k2 * np.float32(ss * ss), ss


def test_schema_profile_and_command_line():
    assert specs.filters['spatial'] == {} and 'spatial' in specs.profile['filter_order'].type.choices
    rad = specs.prof_filters['spatial']['radius']
    assert rad.ref == 'camera.dither_width' and rad.default == 1 and specs.profile['supersample'].default == 1
    gnm, gprof = wrapped(supersample=3, filters={'spatial': {'radius': 0.5}}, filter_order=['logscale', 'spatial'])
    assert gprof.supersample == 3 and list(gprof.filter_order) == ['logscale', 'spatial']
    assert wrapped()[1].supersample == 1
    # the profile's factor times the genome's camera.dither_width (flam3's `filter`)
    gnm = dict(gnm, camera=dict(gnm.get('camera', {}), dither_width=[0.8, 0, 1.6, 0]))
    gp = profile.wrap({'filters': {'spatial': {'radius': 0.5}}}, gnm)
    assert abs(gp.filters.spatial.radius(0.0) - 0.4) < 1e-12 and abs(gp.filters.spatial.radius(1.0) - 0.8) < 1e-12
    assert abs(profile.wrap({}, gnm).filters.spatial.radius(0.0) - 0.8) < 1e-12
    assert abs(profile.wrap({}, configs.cfg2()[0]).filters.spatial.radius(0.5) - 1.0) < 1e-12      # the schema's default width
    # --supersample reaches the profile
    parser = profile.add_args(argparse.ArgumentParser())
    name, prof = profile.get_from_args(parser.parse_args(['--supersample', '2', '-P', '1080p']))
    assert prof['supersample'] == 2 and prof['width'] == 1920
    name, prof = profile.get_from_args(parser.parse_args(['-P', '1080p']))
    assert 'supersample' not in prof
    opts = [a for grp in parser._action_groups if grp.title == 'Spatial options' for a in grp._group_actions]
    assert '--supersample' in [s for a in opts for s in a.option_strings]


def test_renderer_carries_the_chain():
    gnm, gprof = wrapped(supersample=2)
    rdr = render.Renderer(gnm, gprof)
    assert [f.name for f in rdr.filts] == ['yuv', 'bilateral', 'logscale', 'colorclip', 'spatial']


def test_abi_declares_and_exports_fl_resample(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'int\s+fl_resample\s*\(\s*fl_ctx\s*\*\s*ctx,\s*uint32_t w,\s*uint32_t h,\s*uint32_t ss,\s*const float\s*\*\s*taps,'
                     r'\s*uint32_t ntaps\)', code)
    assert 'fl_resample' in _lib.EXPORTS and hasattr(_lib.load(), 'fl_resample')
    assert _lib.load().fl_abi_version() == 1
    mk = open(os.path.join(REPO, 'cuburn_amd', 'csrc', 'Makefile')).read()
    assert 'resample.hip' in mk


def test_spatial_fails_loudly_without_gpu(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(_lib.FlameError):
        render.RenderManager(device=0)
    # argument errors are found before any device is touched; a null context is an error, not a crash
    lib = _lib.load()
    t = np.ones(3, np.float32)
    assert lib.fl_resample(None, 8, 8, 1, t.ctypes.data, 3) == _lib.FL_E_INVAL
    assert b'null' in lib.fl_last_error()


def test_sharded_path_refuses_to_resample():
    """Before any device call: the generator raises on its first step, with no manager at all."""
    from cuburn_amd import distributed
    for kw in (dict(supersample=2), dict(filter_order=['logscale', 'spatial', 'colorclip'])):
        gnm, gprof = wrapped(**kw)
        rdr = render.Renderer(gnm, gprof)
        with pytest.raises(ValueError) as e:
            next(distributed.sharded_frame_steps(None, rdr, gnm, gprof, 0.5, 0, 2, device=0))
        assert 'resample' in str(e.value) and 'halo' in str(e.value)
