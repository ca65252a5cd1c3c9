"""
The `de` filter (flam3-style adaptive density estimation) on the host: the filter chain and its
scalars, the parameter limits, the reach the sample-sharded band path relies on, and the numpy model
(tests/de_model.py) that the GPU tests hold the kernel to.
"""
import json
import os
import re

import numpy as np
import pytest

from common import REPO
from de_model import (KERNEL_CUT, de_filter, de_gather_at, kernel, kernel_exponent, near_half_densities, radii16,
                      radii16_float)
from cuburn_amd import _lib, configs, distributed, filters, output, profile, render
from cuburn_amd.genome import convert

DE_ORDER = ['de', 'logscale', 'smearclip']


def gprof_for(w=1920, h=1080, gnm=None, **prof_kw):
    g, prof = configs.cfg2()
    gnm = g if gnm is None else gnm
    prof = dict(prof, width=w, height=h, filter_order=DE_ORDER, **prof_kw)
    return profile.wrap(prof, gnm)


def de_scalars(gp, tc=0.5):
    dim = render.Framebuffers.calc_dim(gp.width, gp.height)
    return filters.DensityEstimation().scalars(gp, gp.filters.de, dim, tc)


def test_chain_and_filter_id():
    """A profile whose filter_order lists `de` builds a chain (it raised KeyError before the filter existed), and the
    Python id is the header's."""
    assert [f.name for f in filters.create(gprof_for())] == ['yuv'] + DE_ORDER
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    m = re.search(r'\bFL_FILT_DE\s*=\s*(\d+)', hdr)
    assert m and _lib.FILT['de'] == int(m.group(1))


def test_scalars_scale_with_width():
    R, Rmin, curve = de_scalars(gprof_for())
    assert (R, Rmin, curve) == (np.float32(11.0), np.float32(0.0), np.float32(0.6))
    assert de_scalars(gprof_for(3840, 2160))[0] == np.float32(22.0)
    assert de_scalars(gprof_for(960, 540))[0] == np.float32(5.5)


def test_scalars_minimum_and_profile_multipliers():
    g, _ = configs.cfg2()
    g = json.loads(json.dumps(g))
    g.setdefault('filters', {})['de'] = {'radius': 10.0, 'minimum': 0.25, 'curve': 0.5}
    R, Rmin, curve = de_scalars(gprof_for(gnm=g))
    assert (R, Rmin, curve) == (np.float32(10.0), np.float32(2.5), np.float32(0.5))
    # profile-side filter parameters multiply the genome's
    R, Rmin, curve = de_scalars(gprof_for(gnm=g, filters={'de': {'radius': 2.0, 'curve': 3.0}}))
    assert (R, Rmin, curve) == (np.float32(20.0), np.float32(5.0), np.float32(1.5))


def test_scalars_from_flam3_estimator():
    gold = json.load(open(os.path.join(REPO, 'tests', 'golden', 'genome_front.json')))
    xml = gold['xml']['ref_test'].replace(
        '<flame time="0"', '<flame time="0" estimator_radius="9" estimator_minimum="3" estimator_curve="0.4"')
    node = convert.flam3_to_node(convert.XMLGenomeParser.parse(xml)[0])
    for w in (1920, 1280):
        R, Rmin, curve = de_scalars(gprof_for(w, 720, gnm=node))
        assert R == np.float32(9.0 * w / 1920)
        assert Rmin == np.float32(9.0 * w / 1920 / 3)
        assert curve == np.float32(0.4)


@pytest.mark.parametrize('de,w,what', [({'curve': 0.0}, 1920, 'curve'), ({'radius': 97.0}, 1920, 'radius'),
                                       ({'radius': 48.5}, 3840, 'radius')])
def test_scalars_limits(de, w, what):
    g, _ = configs.cfg2()
    g = json.loads(json.dumps(g))
    g.setdefault('filters', {})['de'] = de
    with pytest.raises(ValueError, match=what):
        de_scalars(gprof_for(w, 1080, gnm=g))
    ok = dict(de, radius=96.0 * 1920 / w) if 'radius' in de else dict(de, curve=1e-3)
    g['filters']['de'] = ok
    de_scalars(gprof_for(w, 1080, gnm=g))


def test_minimum_is_clamped():
    g, _ = configs.cfg2()
    g = json.loads(json.dumps(g))
    g.setdefault('filters', {})['de'] = {'radius': 8.0, 'minimum': 0.5}
    # the profile multiplier takes the fraction beyond 1: the filter clamps it
    R, Rmin, _ = de_scalars(gprof_for(gnm=g, filters={'de': {'minimum': 3.0}}))
    assert Rmin == R == np.float32(8.0)


@pytest.mark.parametrize('m', [16, 17, 24, 33, 72, 176, 255, 1000, 1535, 1536])
def test_model_kernel_normalised_and_symmetric(m):
    k = kernel(m)
    assert abs(k.sum() - 1.0) < 1e-12
    assert np.array_equal(k, k[::-1]) and np.array_equal(k, k[:, ::-1]) and np.array_equal(k, k.T)
    I = m // 16
    assert k[I, I] == k.max() and (k > 0).sum() == sum(1 for i in range(-I, I + 1) for j in range(-I, I + 1)
                                                      if 256 * (i * i + j * j) <= m * m)


def test_model_radii():
    w = np.array([0.0, -1.0, 0.25, 1.0, 2.0, 1e6], np.float32)
    m = radii16(w, 11.0, 0.0, 0.6)
    assert list(m[:4]) == [0, 0, 176, 176]                  # 0 < w < 1 counts as 1
    assert m[4] == int(np.floor(16 * 11 * 2 ** -0.6 + 0.5)) and m[5] == 0
    assert list(radii16(w, 11.0, 5.5, 0.6)[3:]) == [176, int(np.floor(16 * 11 * 2 ** -0.6 + 0.5)), 88]
    assert not radii16(w, 0.0, 0.0, 0.6).any()


def test_model_pass_through_bit_identical():
    """Bins with h < 1 and bins with w <= 0 come out as they went in, to the bit."""
    rs = np.random.RandomState(3)
    buf = np.zeros((40, 64, 4), np.float32)
    buf[..., :3] = rs.uniform(0, 1e4, (40, 64, 3)).astype(np.float32)
    buf[..., 3] = rs.uniform(200, 1e5, (40, 64)).astype(np.float32)        # h = 11 w^-0.6 < 1
    buf[5:9, 5:9, 3] = 0.0
    buf[10:12, 20:30, 3] = -2.0
    assert (radii16(buf[..., 3], 11.0, 0.0, 0.6) < 16).all()
    assert np.array_equal(de_filter(buf, 11.0, 0.0, 0.6).astype(np.float32), buf)


def test_model_conserves_and_spreads():
    buf = np.zeros((64, 64, 4), np.float32)
    buf[32, 32] = (3.0, 2.0, 1.0, 1.0)                     # h = R
    buf[10, 50] = (5.0, 5.0, 5.0, 8.0)                     # h = R 8^-0.6
    out = de_filter(buf, 6.0, 0.0, 0.6)
    assert np.allclose(out.sum((0, 1)), buf.astype(np.float64).sum((0, 1)), rtol=1e-12)
    assert out[32, 32, 3] < 1 and out[32, 38, 3] > 0 and out[32, 39, 3] == 0
    assert np.allclose(out[32 - 6:33 + 6, 32 - 6:33 + 6, 3], kernel(96))
    # weight beyond the buffer's edge is dropped
    edge = np.zeros((16, 16, 4), np.float32)
    edge[0, 0] = (1, 1, 1, 1)
    assert 0.25 < de_filter(edge, 6.0, 0.0, 0.6)[..., 3].sum() < 0.5


def sparse_accum(H, W, seed):
    """Sparse bins for the two model forms: densities in (0, 1) (h = R), spreading bins of many radii, bins that stay
    (w = 0, w < 0, or so dense that h < 1) beside spreading ones, and bins on every edge and corner."""
    rs = np.random.RandomState(seed)
    w = np.where(rs.uniform(size=(H, W)) < 0.08, rs.choice([0.3, 0.9, 1.0, 2.5, 7.0, 40.0, 1e3, 1e5], (H, W)), 0.0)
    w *= rs.uniform(0.8, 1.2, (H, W))
    edge = np.zeros((H, W), bool)
    edge[0, ::7] = edge[-1, 3::7] = edge[::5, 0] = edge[2::5, -1] = True
    edge[0, 0] = edge[0, -1] = edge[-1, 0] = edge[-1, -1] = True
    w[edge] = rs.uniform(0.2, 6.0, edge.sum())
    w[H // 2, W // 2 - 1:W // 2 + 2] = (0.0, 0.5, -2.0)             # stays (w = 0), spreads at h = R, stays (w < 0)
    w[H // 3, W // 3:W // 3 + 2] = (5e4, 0.7)                        # h < 1 (unless Rmin says otherwise) beside h = R
    buf = np.zeros((H, W, 4), np.float32)
    buf[..., 3] = w
    lit = (w != 0) | (rs.uniform(size=(H, W)) < 0.05)                 # some colour without density: it stays
    buf[..., :3] = rs.uniform(1, 1e3, (H, W, 3)) * lit[..., None]
    buf[H // 2, W // 2 - 1, :3] = (7.0, 8.0, 9.0)
    return buf


@pytest.mark.parametrize('vals,shape,seed', [((96.0, 0.0, 1.0), (40, 72), 1), ((11.0, 4.4, 0.6), (56, 80), 2),
                                             ((23.0, 0.0, 0.4), (48, 64), 3)])
def test_model_gather_form_equals_scatter_form(vals, shape, seed):
    """de_gather_at (gather form written from the DESIGN.md §4.6 text, S summed directly over the disc) and de_filter
    (scatter form through kernel()) agree to 1e-12 at every output pixel.  Together the parameter sets cover R = 96,
    Rmin > 0, densities in (0, 1), spreading bins on every edge of the buffer and bins that stay beside spreading ones."""
    buf = sparse_accum(*shape, seed)
    w = buf[..., 3]
    m = radii16(w, *vals)
    spreads = m >= 16
    assert ((w > 0) & (w < 1)).any()
    assert spreads[0].any() and spreads[-1].any() and spreads[:, 0].any() and spreads[:, -1].any()
    assert (~spreads & (np.roll(spreads, 1, 1) | np.roll(spreads, -1, 1))).any()
    if vals[0] == 96:
        assert (m == 1536).any() and ((m > 0) & (m < 16)).any()
    if vals[1] > 0:
        assert (m == np.floor(16 * vals[1] + 0.5)).sum() > 10            # clamped at Rmin
    g = de_gather_at(buf, *vals, np.argwhere(np.ones(shape, bool))).reshape(buf.shape)
    s = de_filter(buf, *vals)
    err = np.abs(g - s) - (1e-12 * np.abs(s) + 1e-15 * np.abs(s).max())
    assert not (err > 0).any(), (err.max(), np.unravel_index(np.argmax(err), err.shape))


def test_kernel_cut_is_exact_at_every_radius():
    """k_de_gather keeps a tap when its float32 exponent e = fma(a, dy^2, a dx^2), a = kA / m^2, is >= kCut
    (de_model.kernel_exponent restates that arithmetic).  DESIGN.md §4.6 argues that this is exactly the integer disc
    test 256 (dx^2 + dy^2) <= m^2, because 256 n - m^2 is never 1..6 and e's rounding is far below the cut's 1e-6 margin.
    Checked for every m = 16 .. 1536 over the disc's bounding box and one ring beyond it (the gather also visits offsets
    up to its tile's largest radius; further out e only falls, as every step is a monotone rounding); e depends on dx^2
    and dy^2 alone, so the quadrant dx, dy >= 0 stands for the box.  The margin is needed: without it, points exactly on
    the edge (256 n == m^2, so m a multiple of 16) are lost at some radii."""
    assert not any((-m * m) % 256 in range(1, 7) for m in range(16, 1537))
    cut0 = np.float32(-4.5 * 1.4426950408889634)            # the cut without its margin
    evals = on_edge = 0
    lost = []
    for m in range(16, 1537):
        I = m // 16 + 1
        dy, dx = np.mgrid[0:I + 1, 0:I + 1]
        n = dx * dx + dy * dy
        e = kernel_exponent(m, dx * dx, dy * dy)
        inside = 256 * n <= m * m
        assert np.array_equal(e >= KERNEL_CUT, inside), (m, np.argwhere((e >= KERNEL_CUT) != inside)[:4])
        edge = 256 * n == m * m
        evals += n.size
        on_edge += edge.sum()
        if (edge & (e < cut0)).any():
            lost.append(m)
    assert evals > 4.9e6 and on_edge > 0
    assert lost and all(m % 16 == 0 for m in lost) and 48 in lost and 80 in lost, lost


@pytest.mark.parametrize('curve', [1.0, 0.6])
def test_radius_rounding_needs_double(curve):
    """near_half_densities: float32 densities whose 16 h lies within 1e-5 of a rounding half, on both sides and no
    closer than 1e-9.  radii16 (h in double: the contract) rounds each to the nearer integer; a float32 pow and rounding
    (radii16_float) picks the other m for about 30 % of them (most of those below the half), which
    test_gpu_de_radii.test_de_rounds_h_in_double would catch."""
    w, below = near_half_densities(96.0, curve)
    assert below.sum() >= 150 and (~below).sum() >= 150
    s = 16.0 * (96.0 * w.astype(np.float64) ** -curve)
    m = radii16(w, 96.0, 0.0, curve)
    assert np.array_equal(m, np.where(below, np.floor(s), np.ceil(s)))
    flips = radii16_float(w, 96.0, 0.0, curve) != m
    assert 0.25 < flips.mean() < 0.35 and flips[below].mean() > 0.5, (flips.mean(), flips[below].mean())


def test_reach_and_band_path():
    assert distributed.FILTER_REACH['de'] == 96 == filters.DensityEstimation.max_radius
    assert distributed.chain_reach(DE_ORDER) == 105 <= distributed.BAND_HALO
    gp = gprof_for(1920, 1080, output={'type': 'raw'})
    dim = render.Framebuffers.calc_dim(1920, 1080)
    out = output.get_output_for_profile(gp)
    assert distributed.band_path_ok(out, dim, [f.name for f in filters.create(gp)])
    assert not distributed.band_path_ok(out, dim, ['yuv', 'bilateral', 'de', 'logscale', 'smearclip'])
