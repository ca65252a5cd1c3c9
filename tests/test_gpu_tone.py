"""
The tone-mapping kernels (filters.hip, tone_device.h, and the same per-pixel functions as the tail of de.hip's last direction)
against the float64 model of tests/tone_model.py, on every branch: the atlas and the scalar grid of tests/test_cpu_tone.py.

Bars.  For each (filter, branch class) the device may deviate from the model by 32 x what the float32 oracle itself deviates from
it in that class ON THE SAME INPUT (computed here, at run time; tests/test_cpu_tone.py pins those figures in a table), and at least
by 32 x 2^-24 of the class's largest model value (of the value itself for the relative metrics).  Why 32: the device's
pow(x, y) = exp2(y log2 x) with a 1-ulp hardware log2 carries |y log2 x| ulp of exponent error into the result — at most 13.3 on the
atlas (w = 1e-4, y <= 1; 15 after the logscale in front of the plain clips) — plus an ulp each for exp2 and rcp: about 16 ulp where
libm's powf gives at most 1.  The other factor of two is headroom.  The device is measured against the model, never against
itself; metrics as in tests/test_cpu_tone.py (colorclip, logencode absolute; logscale and the plain clips relative per element;
yuv in ulp, where the bar is a flat 4 ulp: plain multiply-adds).  The device's worst deviations per class are appended to
tone_errors.txt in the directory the environment variable FLAME_TEST_REPORT_DIR names, when it is set
(FLAME_TEST_REPORT_DIR=out pytest tests/test_gpu_tone.py).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from common import O, frame_times
from cuburn_amd import configs, profile, render, _lib
import tone_model as TM
import tone_cases as T
from accum_inputs import synth_accum, sparse_accum
from gpu_harness import run_filter, check_chain_error, filter_chain_on_device, oracle_chain

pytestmark = pytest.mark.gpu

BIG = (200, 120)                    # 224 x 144 padded: 7 x 18 workgroups of 32 x 8
FACTOR = 32.0


@pytest.fixture(scope='module')
def mgr(built):
    return render.RenderManager(device=0, nslots=1024, host_seed=7)


def report(test, worst):
    try:
        out = os.environ.get('FLAME_TEST_REPORT_DIR')
        if out and os.path.isdir(out):
            with open(os.path.join(out, 'tone_errors.txt'), 'a') as fp:
                for (name, cls), (dev, bar) in sorted(worst.items()):
                    fp.write('%s: %s / %s: device %.3e bar %.3e\n' % (test, name, cls, dev, bar))
    except OSError:
        pass


def check(worst, name, dev, model, cls, ref, what, src=None):
    """Device against model per class, under FACTOR x the oracle's own deviation (and the floor); records the worst of both."""
    got = T.deviation(name, dev, model, cls, src)
    own = T.deviation(name, ref, model, cls, src)
    scale = T.scale_of(name, model, cls)
    for k, v in got.items():
        bar = 4.0 if name == 'yuv' else FACTOR * max(own[k], 2.0 ** -24 * scale[k])
        old = worst.get((name, k), (0.0, 0.0))
        worst[(name, k)] = (max(old[0], v), max(old[1], bar))
        assert v <= bar, '%s, class %s: device deviates %.3e from the model, bar %.3e (oracle %.3e)' % (what, k, v, bar, own[k])


def dims(mgr, size):
    dim, d = mgr.fb.calc_dim(*size), O.calc_dim(*size)
    assert (dim.ah, dim.astride) == (d.ah, d.astride)
    return dim, d


def big_input(dim, d, seed=1, colour=1.0):
    """A 200 x 120 accumulator after yuv and the model's logscale (more than one workgroup column and row); `colour` scales its
    colour-to-density ratios."""
    buf = TM.logscale(O.yuv_to_rgb(d, synth_accum(dim, seed)), T.LOG_K1, 0.002).astype(np.float32)
    buf[:, :3] *= np.float32(colour)
    return buf


def half_atlas():
    """Every other density row of the atlas: the 32 x 32 padded buffer of a 1 x 1 frame."""
    return np.ascontiguousarray(T.atlas().reshape(64, 32, 4)[::2].reshape(-1, 4))


# ------------------------------------------------------------------ colorclip
def test_colorclip_whole_grid_on_the_atlas(mgr):
    dim, d = dims(mgr, (T.AW, T.AH))
    buf = T.atlas()
    worst, seen = {}, np.zeros(7, np.int64)
    try:
        for vals in T.colorclip_grid():
            dev = run_filter(mgr, 'colorclip', dim, buf, vals)
            model, cls = TM.colorclip(buf, *vals)
            seen += np.bincount(cls, minlength=7)
            check(worst, 'colorclip', dev, model, cls, O.colorclip(d, buf, *vals), 'colorclip %r' % [float(v) for v in vals])
    finally:
        report('colorclip atlas', worst)
    assert (seen > 0).all() and len(worst) == 6


@pytest.mark.parametrize('vib,highpow', [(1.0, 1.5), (0.5, 1.5), (1.0, -0.5), (0.5, -0.5)])
def test_colorclip_many_workgroups(mgr, vib, highpow):
    dim, d = dims(mgr, BIG)
    buf = big_input(dim, d, colour=3.0)                        # ratios up to 5: maxa > 1 at vib = 0.5 too
    vals = [np.float32(vib), np.float32(highpow), np.float32(0.25), np.float32(0.01), TM.lingam_of(0.25, 0.01)]
    worst = {}
    dev = run_filter(mgr, 'colorclip', dim, buf, vals)
    model, cls = TM.colorclip(buf, *vals)
    try:
        check(worst, 'colorclip', dev, model, cls, O.colorclip(d, buf, *vals), 'colorclip 200 x 120 vib %g highpow %g' % (vib, highpow))
    finally:
        report('colorclip 200x120 vib %g highpow %g' % (vib, highpow), worst)
    assert (cls == (TM.HIGHLIGHT if highpow >= 0 else TM.BLENDED)).sum() >= 256 and len(worst) >= 3


def test_filters_on_the_smallest_frame(mgr):
    """1 x 1: one workgroup column, the whole padded buffer is gutter."""
    dim, d = dims(mgr, (1, 1))
    assert (dim.ah, dim.astride) == (32, 32)
    buf = half_atlas()
    worst = {}
    try:
        for vals in T.colorclip_grid()[7::17]:
            model, cls = TM.colorclip(buf, *vals)
            check(worst, 'colorclip', run_filter(mgr, 'colorclip', dim, buf, vals), model, cls, O.colorclip(d, buf, *vals), '1 x 1 colorclip')
        k2 = np.float32(0.002)
        check(worst, 'logscale', run_filter(mgr, 'logscale', dim, buf, [T.LOG_K1, k2]), TM.logscale(buf, T.LOG_K1, k2), T.LIVE[:1024],
              O.logscale(d, buf, np.float32(T.LOG_K1), k2), '1 x 1 logscale')
        lbuf = T.logscaled(buf)
        for name, vals in T.clip_cases()[:6]:
            model, cls = T.model_clip(name, lbuf, d.ah, d.astride, vals)
            check(worst, name, run_filter(mgr, name, dim, lbuf, vals), model, cls, T.oracle_clip(name, d, lbuf, vals), '1 x 1 %s' % name)
    finally:
        report('1x1', worst)


# ------------------------------------------------------------------ logscale
def test_logscale_down_to_the_rounding_of_the_sum(mgr):
    """The atlas densities and 1e-6 .. 3e8 at the k2 of cfg1 .. cfg5 and 1e-6: relative to the model (whose sum 1 + w k2 is the
    float32 one), and exactly zero — not NaN — in all four channels where that sum is 1."""
    dim, d = dims(mgr, (T.AW, T.AH))
    worst = {}
    flat_seen = 0
    try:
        for src in (T.atlas(), T.wide_atlas()):
            for k2 in T.config_k2s():
                dev = run_filter(mgr, 'logscale', dim, src, [T.LOG_K1, k2])
                flat = (np.float32(1) + src[:, 3] * k2) == 1
                flat_seen += int((flat & (src[:, 3] > 0)).sum())
                assert not np.isnan(dev).any() and not dev[flat].any(), 'logscale k2 %g: %d non-zero values where 1 + w k2 rounds to 1' % (
                    k2, np.count_nonzero(dev[flat]))
                check(worst, 'logscale', dev, TM.logscale(src, T.LOG_K1, k2), T.LIVE, O.logscale(d, src, np.float32(T.LOG_K1), k2),
                      'logscale k2 %g' % k2)
    finally:
        report('logscale', worst)
    assert flat_seen >= 64


# ------------------------------------------------------------------ smearclip, haloclip, plainclip
@pytest.mark.parametrize('size', [(T.AW, T.AH), BIG], ids=['atlas', '200x120'])
def test_plain_clips(mgr, size):
    """The five (gam, lin) pairs, smear widths 0.3 / 0.7 / 2.0, brightness 0.5 / 4, on the logscaled atlas (64 x 32: every pixel is
    within reach of an edge, so every clamp direction of the four blur patterns is used, and the model is the judge there) and on
    a 224 x 144 buffer."""
    dim, d = dims(mgr, size)
    buf = T.logscaled(T.atlas()) if size != BIG else big_input(dim, d)
    worst = {}
    try:
        for name, vals in T.clip_cases():
            dev = run_filter(mgr, name, dim, buf, vals)
            model, cls = T.model_clip(name, buf, d.ah, d.astride, vals)
            check(worst, name, dev, model, cls, T.oracle_clip(name, d, buf, vals), '%s %r' % (name, [float(v) for v in vals]))
    finally:
        report('plain clips %dx%d' % size, worst)
    assert ('smearclip', 'plain<lin') in worst and ('plainclip', 'plain<lin') in worst and ('haloclip', 'plain') in worst


def test_filters_do_not_depend_on_what_ran_before(mgr):
    """d_side, d_back and d_blur are shared scratch: each filter's result is bit-identical whichever filter used them last."""
    dim, d = dims(mgr, BIG)
    buf = big_input(dim, d, seed=4)
    g, l = 0.25, 0.01
    gm1, lin, lingam = np.float32(g - 1), np.float32(l), TM.lingam_of(g, l)
    steps = {'smearclip': [np.float32(0.7), gm1, lin, lingam], 'haloclip': [gm1], 'plainclip': [gm1, lin, lingam, np.float32(1.3)],
             'logencode': [np.float32(2.2)], 'colorclip': [np.float32(0.9), np.float32(1.5), np.float32(g), lin, lingam]}
    for a in ('smearclip', 'haloclip', 'plainclip', 'colorclip', 'logencode'):
        first = run_filter(mgr, a, dim, buf, steps[a])
        for b in steps:
            if b == a:
                continue
            run_filter(mgr, b, dim, buf[::-1].copy(), steps[b])
            again = run_filter(mgr, a, dim, buf, steps[a])
            assert np.array_equal(first.view(np.uint32), again.view(np.uint32)), (a, 'after', b)


# ------------------------------------------------------------------ logencode, yuv
@pytest.mark.parametrize('degamma', [1.0, 2.2])
def test_logencode(mgr, degamma):
    dim, d = dims(mgr, (T.AW, T.AH))
    buf = T.logscaled(T.atlas())
    model = TM.logencode(buf, degamma)
    assert np.isneginf(model).sum() > 500 and np.isfinite(model).sum() > 5000
    dev = run_filter(mgr, 'logencode', dim, buf, [np.float32(degamma)])
    assert not np.isnan(dev).any()                            # -inf where the model is -inf: asserted by deviation()
    worst = {}
    try:
        check(worst, 'logencode', dev, model, T.LIVE, O.logencode(d, buf, np.float32(degamma)), 'logencode %g' % degamma)
    finally:
        report('logencode %g' % degamma, worst)


def test_yuv_every_clamp(mgr):
    dim, d = dims(mgr, (T.AW, T.AH))
    buf = T.yuv_atlas()
    model = TM.yuv_to_rgb(buf)
    live = buf[:, 3] > 0
    for c in range(3):
        assert ((model[:, c] == 0) & live & (np.abs(buf[:, :3]).max(1) > 0)).sum() >= 64 and (model[:, c] > 0).sum() >= 64, c
    dev = run_filter(mgr, 'yuv', dim, buf, [])
    assert np.array_equal(dev[:, 3], buf[:, 3])
    worst = {}
    try:
        check(worst, 'yuv', dev, model, T.LIVE, O.yuv_to_rgb(d, buf), 'yuv', src=buf)
    finally:
        report('yuv', worst)


# ------------------------------------------------------------------ the tail of the last DE direction
TAIL_POINTS = [(0.9, 1.5, 1.0 / 3.0, 0.02), (1.0, 3.0, 0.25, 0.01), (0.9, 0.0, 0.1, 0.3), (0.9, -0.5, 0.25, 0.01), (1.0, -0.5, 0.1, 0.3),
               (0.5, -2.0, 1.0 / 3.0, 0.02), (0.0, 1.5, 0.9, 0.0), (0.9, -1.0, 1.0, 0.05), (1.0, 1.5, 0.9, 0.0), (0.5, -0.5, 0.25, 0.01)]
BIL = [6.0 * BIG[0] / 1920., 0.05, 1.5, 0.8, 4.0]
TAIL_LOG = [4.1875, 0.02]


def tail_inputs(dim, d):
    """Dense, sparse, and sparse with colours up to 3 x the density: below `lin` only such colours reach maxa > 1."""
    vivid = sparse_accum(dim, seed=5)
    vivid[:, :3] *= np.float32(3)
    return [('dense', O.yuv_to_rgb(d, synth_accum(dim))), ('sparse', sparse_accum(dim)), ('vivid', vivid)]


@pytest.mark.parametrize('with_log', [True, False], ids=['bilateral-logscale-colorclip', 'bilateral-colorclip'])
def test_fused_tail(mgr, with_log):
    """logscale and colorclip riding on the last DE direction, at 10 grid points: (a) bit-identical to the run that looks at the
    buffer between the calls (every step a kernel of its own), and (b) equal, under the class bars, to the model's logscale and
    colorclip of the device's OWN bilateral output — the tail alone, without the DE's tolerance in between."""
    lib = _lib.load()
    dim, d = dims(mgr, BIG)
    worst, seen = {}, np.zeros(7, np.int64)

    def run(buf, chain, peek):
        _lib.check(lib.fl_debug_clear(mgr.fb.ctx, dim.w, dim.h, 0))
        mgr.fb.write('front', buf)
        looks = []
        for name, vals in chain:
            arr = np.asarray(vals, np.float32)
            _lib.check(lib.fl_filter(mgr.fb.ctx, _lib.FILT[name], dim.w, dim.h, arr.ctypes.data, len(arr)))
            if peek:
                looks.append(mgr.fb.read('front', buf.shape, np.float32))
        return mgr.fb.read('front', buf.shape, np.float32), looks

    try:
        for (kind, buf), (vib, hp, g, l) in [(i, p) for i in tail_inputs(dim, d) for p in TAIL_POINTS]:
            clip = [np.float32(vib), np.float32(hp), np.float32(g), np.float32(l), TM.lingam_of(g, l)]
            chain = [('bilateral', BIL)] + ([('logscale', TAIL_LOG)] if with_log else []) + [('colorclip', clip)]
            fused, _ = run(buf, chain, False)
            apart, looks = run(buf, chain, True)
            assert np.array_equal(fused.view(np.uint32), apart.view(np.uint32)), (kind, with_log, clip)
            bil = looks[0]
            assert np.isfinite(bil).all()
            mid, ref = bil, bil
            if with_log:
                mid, ref = TM.logscale(bil, *TAIL_LOG), O.logscale(d, bil, *[np.float32(v) for v in TAIL_LOG])
            model, cls = TM.colorclip(mid, *clip)
            seen += np.bincount(cls, minlength=7)
            check(worst, 'colorclip', fused, model, cls, O.colorclip(d, ref, *clip), 'fused tail %s %r' % (kind, [float(v) for v in clip]))
    finally:
        report('fused tail %s' % ('log+clip' if with_log else 'clip'), worst)
    assert (seen >= 8).all(), seen


# ------------------------------------------------------------------ a non-default genome end to end
def test_rich_flam3_chain_against_the_oracle(mgr, tmp_path):
    """The `rich` flam3 file (vibrancy 0.9, highlight_power 1.5, gamma 3, gamma_threshold 0.02) at 320 x 240 through the
    Renderer's own filter objects: the device chain against the oracle's on the same accumulator, under the full-size bars."""
    from cuburn_amd.genome import store
    lib = _lib.load()
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'genome_front.json')))
    path = tmp_path / 'rich.flam3'
    path.write_text(gold['xml']['rich'].replace(' chaos="1 0.5 2"', ''))
    with pytest.warns(UserWarning):
        gnm, _ = store.connect(str(tmp_path)).animation(str(path))
    gprof = profile.wrap(dict(configs.cfg2()[1], width=320, height=240), gnm)
    rdr = render.Renderer(gnm, gprof)
    tc = 0.1
    dim = mgr.fb.set_dim(gprof.width, gprof.height)
    g = rdr._handle(mgr.fb)
    ts, td = frame_times(gprof, tc)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(mgr.fb.ctx, C.byref(fid)))
    mgr._copy(rdr, gnm)
    _lib.check(lib.fl_interp(mgr.fb.ctx, g, dim.w, dim.h, ts, td))
    run = C.c_uint64()
    nsamples = float(gprof.spp(tc) * gprof.width * gprof.height)
    _lib.check(lib.fl_iterate(mgr.fb.ctx, g, dim.w, dim.h, nsamples, mgr.fuse, mgr.resolve_accum_mode(dim), C.byref(run)))
    front = mgr.fb.read('front', (dim.ah * dim.astride, 4), np.float32)
    assert front[:, 3].sum() > 0.2 * nsamples
    vals, dev = filter_chain_on_device(mgr, rdr, gprof, dim, tc)
    assert vals['colorclip'][:2] == [float(np.float32(0.9)), 1.5] and abs(vals['colorclip'][2] - 1 / 3.0) < 1e-7 and vals['colorclip'][3] == float(np.float32(0.02))
    ref = oracle_chain(O.calc_dim(gprof.width, gprof.height), front, vals)
    assert (dev[:, 3] > 0).mean() > 0.05 and ref[:, :3].max() == 1.0
    check_chain_error(np.abs(dev - ref), 'rich.flam3 320x240 whole frame')
