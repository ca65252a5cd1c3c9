"""
The `bloom` filter on the host: its taps and scalars, the id, its place in the chain, the reach the
sample-sharded path relies on, profile-side factors, and the properties of the float64 model (tests/bloom_model.py) that the
GPU tests hold the kernels to.
"""
import json
import os
import re

import numpy as np
import pytest

import bloom_model as BM
from bloom_cases import CASES, gamma_buffer, impulse_buffer
from common import REPO
from cuburn_amd import _lib, configs, distributed, filters, profile, render

BLOOM_ORDER = ['bilateral', 'logscale', 'bloom', 'colorclip']


def gprof_for(w=1920, h=1080, gnm=None, **prof_kw):
    g, prof = configs.cfg2()
    gnm = g if gnm is None else gnm
    return profile.wrap(dict(prof, width=w, height=h, filter_order=BLOOM_ORDER, **prof_kw), gnm)


def bloom_scalars(gp, tc=0.5):
    ss = filters.supersample_of(gp)
    dim = render.Framebuffers.calc_dim(ss * gp.width, ss * gp.height)
    return filters.Bloom().scalars(gp, gp.filters.bloom, dim, tc)


# ------------------------------------------------------------------ taps
@pytest.mark.parametrize('sigma', [0.0, 0.2, 1.0 / 3.0, 1.0, 5.0, 12.0, 16.0, 24.0, 100.0, 128.0])
def test_taps(sigma):
    t = filters.bloom_taps(sigma)
    n = 2 * int(np.ceil(3 * sigma)) + 1
    assert t.dtype == np.float32 and t.shape == (n,)
    assert np.array_equal(t, t[::-1]) and t.argmax() == n // 2 and (t > 0).all()
    assert abs(t.astype(np.float64).sum() - 1.0) <= n * 2.0 ** -24
    assert np.array_equal(t.astype(np.float64), BM.taps(sigma))          # the model derives them on its own
    if sigma == 0:
        assert list(t) == [1.0]


def test_taps_refuse_bad_sigma():
    for s in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='sigma'):
            filters.bloom_taps(s)


# ------------------------------------------------------------------ scalars
def test_scalars_scale_with_width():
    for w, h, sigma in ((1920, 1080, 12.0), (3840, 2160, 24.0), (960, 540, 6.0)):
        vals = bloom_scalars(gprof_for(w, h))
        R = int(np.ceil(3 * sigma))
        assert len(vals) == 3 + R and all(isinstance(v, np.float32) for v in vals)
        assert vals[0] == np.float32(1.0) and vals[1] == np.float32(0.25)
        assert np.array_equal(np.array(vals[2:]), filters.bloom_taps(sigma)[R:])
        assert [float(v) for v in vals] == [float(v) for v in BM.params(1.0, 0.25, sigma)]


def test_scalars_at_supersample_2():
    """The accumulator of a supersampled frame is twice as wide: so is the Gaussian, in bins."""
    vals = bloom_scalars(gprof_for(1920, 1080, supersample=2))
    assert len(vals) == 3 + 72 and np.array_equal(np.array(vals[2:]), filters.bloom_taps(24.0)[72:])


def test_scalars_limit():
    g, _ = configs.cfg2()
    g = json.loads(json.dumps(g))
    g.setdefault('filters', {})['bloom'] = {'radius': 128.0}
    assert len(bloom_scalars(gprof_for(gnm=g))) == 3 + 384 == 3 + filters.Bloom.max_reach
    for w, h, radius in ((1920, 1080, 128.5), (3840, 2160, 64.5)):
        g['filters']['bloom'] = {'radius': radius}
        with pytest.raises(ValueError) as e:
            bloom_scalars(gprof_for(w, h, gnm=g))
        assert '%g' % radius in str(e.value) and str(w) in str(e.value) and '384' in str(e.value)
    g['filters']['bloom'] = {'radius': 64.5}
    with pytest.raises(ValueError, match='384'):
        bloom_scalars(gprof_for(1920, 1080, gnm=g, supersample=2))


def test_profile_factors():
    g, _ = configs.cfg2()
    g = json.loads(json.dumps(g))
    g.setdefault('filters', {})['bloom'] = {'threshold': 2.0, 'radius': 3.0, 'strength': 0.5}
    vals = bloom_scalars(gprof_for(gnm=g, filters={'bloom': {'threshold': 0.75, 'radius': 2.0, 'strength': 3.0}}))
    assert vals[0] == np.float32(1.5) and vals[1] == np.float32(1.5)
    assert np.array_equal(np.array(vals[2:]), filters.bloom_taps(6.0)[18:])


# ------------------------------------------------------------------ id, chain, reach
def test_filter_id_is_the_headers():
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    m = re.search(r'\bFL_FILT_BLOOM\s*=\s*(\d+)', hdr)
    assert m and _lib.FILT['bloom'] == int(m.group(1)) == 9
    m = re.search(r'#define\s+FL_BLOOM_MAX_REACH\s+(\d+)', hdr)
    assert m and int(m.group(1)) == filters.Bloom.max_reach == BM.MAX_REACH == 384


def test_chain_places_it_where_the_profile_lists_it():
    assert [f.name for f in filters.create(gprof_for())] == ['yuv'] + BLOOM_ORDER
    assert isinstance(filters.create(gprof_for())[3], filters.Bloom)
    g, prof = configs.cfg2()
    assert 'bloom' not in [f.name for f in filters.create(profile.wrap(prof, g))]


def test_reach_and_band_path():
    assert distributed.FILTER_REACH['bloom'] == 384 == filters.Bloom.max_reach
    assert distributed.chain_reach(['yuv'] + BLOOM_ORDER) > distributed.BAND_HALO


# ------------------------------------------------------------------ the model
def test_model_identity_at_strength_0():
    buf = gamma_buffer(48, 64)
    out, babs = BM.bloom(buf, 1.0, 0.0, 5.0)
    assert np.array_equal(out, buf.astype(np.float64)) and babs.max() > 0
    out, babs = BM.bloom(buf, float(buf[..., 3].max()), 0.25, 5.0)           # nothing above the threshold
    assert np.array_equal(out, buf.astype(np.float64)) and not babs.any()


@pytest.mark.parametrize('sigma', [0.0, 1.0, 5.0])
def test_model_interior_impulse(sigma):
    buf = np.zeros((64, 96, 4), np.float32)
    buf[30, 40] = (3.0, 2.0, 1.0, 4.0)
    E = 0.75 * buf[30, 40].astype(np.float64)
    out, _ = BM.bloom(buf, 1.0, 0.25, sigma)
    t = BM.taps(sigma)
    R = len(t) // 2
    want = buf.astype(np.float64)
    want[30 - R:31 + R, 40 - R:41 + R] += 0.25 * np.outer(t, t)[..., None] * E
    assert np.allclose(out, want, rtol=1e-14, atol=0) and (out[30 - R, 40 - R] > 0).all()
    glare = 0.25 * BM.blur(BM.excess(buf, 1.0), sigma)
    assert np.allclose(glare.sum((0, 1)), 0.25 * t.sum() ** 2 * E, rtol=1e-12, atol=0)
    assert abs(t.sum() - 1.0) <= len(t) * 2.0 ** -24


def test_model_corner_impulse_loses_what_falls_outside():
    buf = np.zeros((48, 64, 4), np.float32)
    buf[0, 0] = (1.0, 1.0, 1.0, 2.0)
    out, _ = BM.bloom(buf, 1.0, 1.0, 4.0)
    t = BM.taps(4.0)
    R = len(t) // 2
    inside = t[R:].sum()                                   # the taps at 0 .. R: the quarter of the footprint that is inside
    glare = BM.blur(BM.excess(buf, 1.0), 4.0)
    assert np.allclose(glare.sum((0, 1)), inside * inside * 0.5 * buf[0, 0], rtol=1e-12, atol=0)
    assert np.allclose(out, buf + glare, rtol=1e-15, atol=0)
    far = np.zeros((48, 64, 4), np.float32)
    far[47, 63] = buf[0, 0]
    assert np.array_equal(BM.bloom(far, 1.0, 1.0, 4.0)[0][::-1, ::-1], out)


def test_model_excess_rule():
    buf = np.zeros((1, 5, 4), np.float32)
    buf[0, :, 3] = (0.0, 0.5, 1.0, 4.0, np.nan)
    buf[0, :, :3] = 2.0
    E = BM.excess(buf, 1.0)
    assert not E[0, :3].any() and np.array_equal(E[0, 3], [1.5, 1.5, 1.5, 3.0])
    assert not E[0, 4, :3].any()                                          # a NaN w: f = 0


def test_float32_restatement_is_inside_the_bar():
    """The bar of the GPU test, (2 ntaps + 16) 2^-24 strength blur(|E|) + 2 * 2^-24 |out|, holds a plain float32 evaluation in
    tap order on the test's own shapes (cases of up to 121 taps here: the 769-tap ones run on the GPU)."""
    worst = 0.0
    for (w, h), sigma in CASES:
        if sigma > 20:
            continue
        d = render.Framebuffers.calc_dim(w, h)
        for buf in (gamma_buffer(d.ah, d.astride), impulse_buffer(d.ah, d.astride)):
            out, babs = BM.bloom(buf, 1.0, 0.25, sigma)
            got = bloom_float32(buf, np.float32(1.0), np.float32(0.25), sigma)
            ratio = np.abs(got.astype(np.float64) - out) / np.maximum(BM.bar(out, babs, 0.25, sigma), 1e-300)
            worst = max(worst, float(ratio.max()))
    assert 0 < worst < 1.0, worst


def bloom_float32(buf, thr, strength, sigma):
    t = BM.taps(sigma).astype(np.float32)
    w = buf[..., 3]
    with np.errstate(invalid='ignore', divide='ignore'):
        f = np.where(w > thr, (w - thr) / w, np.float32(0)).astype(np.float32)
    a = f[..., None] * buf
    for axis in (1, 0):
        R = len(t) // 2
        pad = [(0, 0)] * 3
        pad[axis] = (R, R)
        p = np.pad(a, pad)
        acc = np.zeros_like(a)
        for i in range(2 * R + 1):
            acc = acc + t[i] * np.take(p, np.arange(i, i + a.shape[axis]), axis=axis)
        a = acc
    return buf + strength * a
