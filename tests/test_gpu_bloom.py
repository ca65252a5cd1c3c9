"""
The `bloom` filter (csrc/bloom.hip) on the GPU, through fl_filter, against the float64 model of
tests/bloom_model.py.

Bar: every sample of every channel satisfies |dev - model| <= (2 ntaps + 16) 2^-24 strength blur(|E|) + 2 * 2^-24 |out| — the
standard bound of ntaps float32 multiply-adds per pass in any order, plus a few ulp for the division in E and the final add
(bloom_model.bar).  No sample is left out.  The worst ratio to the bar per case is appended to bloom_errors.txt in the directory
FLAME_TEST_REPORT_DIR names, when it is set.
"""
import os

import numpy as np
import pytest

import bloom_model as BM
import tone_cases as T
import tone_model as TM
from accum_inputs import synth_accum
from bloom_cases import CASES, STRENGTH, THRESHOLD, case_id, gamma_buffer, impulse_bins, impulse_buffer
from common import O
from cuburn_amd import _lib, configs, filters, profile, render
from gpu_harness import run_filter

pytestmark = pytest.mark.gpu

BIG = (200, 120)
FACTOR = 32.0                       # the class bars of tests/test_gpu_tone.py


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=1024, host_seed=11)
    yield m
    m.fb.free()


def report(line):
    try:
        out = os.environ.get('FLAME_TEST_REPORT_DIR')
        if out and os.path.isdir(out):
            with open(os.path.join(out, 'bloom_errors.txt'), 'a') as fp:
                fp.write(line + '\n')
    except OSError:
        pass


def device(mgr, dim, buf, vals):
    return run_filter(mgr, 'bloom', dim, buf.reshape(-1, 4), vals).reshape(buf.shape)


_models = {}


def model_of(kind, ah, astride, sigma):
    """(input, model output, blurred |E|), computed once per case."""
    key = (kind, ah, astride, sigma)
    if key not in _models:
        buf = gamma_buffer(ah, astride) if kind == 'gamma' else impulse_buffer(ah, astride)
        _models[key] = (buf,) + BM.bloom(buf, THRESHOLD, STRENGTH, sigma)
        for a in _models[key]:
            a.setflags(write=False)
    return _models[key]


@pytest.mark.parametrize('kind', ['gamma', 'impulses'])
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_bloom_matches_model(mgr, case, kind):
    size, sigma = case
    dim = mgr.fb.calc_dim(*size)
    buf, out, babs = model_of(kind, dim.ah, dim.astride, sigma)
    w = buf[..., 3]
    if kind == 'gamma':
        assert 0.25 < (w > THRESHOLD).mean() < 0.35 and (w == 0).any() and (w == np.float32(THRESHOLD)).any() and buf.min() >= 0
    else:
        assert (0, 0) in impulse_bins(dim.ah, dim.astride) and (dim.ah - 1, dim.astride - 1) in impulse_bins(dim.ah, dim.astride)
    vals = BM.params(THRESHOLD, STRENGTH, sigma)
    assert len(vals) == 3 + BM.reach(sigma)
    dev = device(mgr, dim, buf, vals).astype(np.float64)
    assert np.isfinite(dev).all()
    bar = BM.bar(out, babs, STRENGTH, sigma)
    err = np.abs(dev - out)
    ratio = float((err / np.maximum(bar, 1e-300)).max())
    print('bloom %s %s: worst |dev - model| / bar = %.3f' % (case_id(case), kind, ratio))
    report('%s %s: worst ratio to the bar %.4f' % (case_id(case), kind, ratio))
    bad = err > bar
    assert not bad.any(), ('%d of %d samples beyond the bar' % (bad.sum(), bad.size), np.argwhere(bad)[:4].tolist(), ratio)
    assert not np.array_equal(dev, buf.astype(np.float64))                  # (something did bloom)


# ------------------------------------------------------------------ exact cases
@pytest.mark.parametrize('case', [CASES[0], CASES[5], CASES[7]], ids=case_id)
def test_identity_is_bit_exact(mgr, case):
    size, sigma = case
    dim = mgr.fb.calc_dim(*size)
    buf = gamma_buffer(dim.ah, dim.astride, seed=2)
    dev = device(mgr, dim, buf, BM.params(THRESHOLD, 0.0, sigma))
    assert np.array_equal(dev.view(np.uint32), buf.view(np.uint32)), 'strength 0'
    above = float(buf[..., 3].max())
    dev = device(mgr, dim, buf, BM.params(above, STRENGTH, sigma))           # w == threshold: no excess
    assert np.array_equal(dev.view(np.uint32), buf.view(np.uint32)), 'threshold above every w'


def test_two_runs_same_bits_and_a_refused_call_changes_nothing(mgr):
    dim = mgr.fb.calc_dim(*BIG)
    buf = gamma_buffer(dim.ah, dim.astride, seed=3)
    vals = BM.params(THRESHOLD, STRENGTH, 20.0)
    a = device(mgr, dim, buf, vals)
    b = device(mgr, dim, buf, vals)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and not np.array_equal(a, buf)
    with pytest.raises(ValueError, match='bloom'):
        device(mgr, dim, buf, [np.float32(-1.0)] + vals[1:])
    c = device(mgr, dim, buf, vals)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    # other users of the side buffer in between change nothing either
    run_filter(mgr, 'smearclip', dim, buf[::-1].reshape(-1, 4).copy(), [0.7, -0.75, 0.01, 31.6])
    c = device(mgr, dim, buf, vals)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


# ------------------------------------------------------------------ refusals
def test_refusals(mgr):
    lib = _lib.load()
    dim = mgr.fb.calc_dim(*BIG)
    buf = gamma_buffer(dim.ah, dim.astride, seed=4).reshape(-1, 4)
    good = BM.params(THRESHOLD, STRENGTH, 5.0)
    nan, inf = np.float32('nan'), np.float32('inf')
    over = good[:2] + [np.float32(1.0 / 771)] * (BM.MAX_REACH + 2)             # R = 385
    atlimit = good[:2] + [np.float32(1.0 / 769)] * (BM.MAX_REACH + 1)          # R = 384
    bad = [[], good[:1], good[:2], over, [nan] + good[1:], [inf] + good[1:], [good[0], nan] + good[2:], [good[0], -inf] + good[2:],
           good[:4] + [nan] + good[5:], good[:-1] + [inf], [np.float32(-0.5)] + good[1:]]
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, dim.w, dim.h, 0))
    mgr.fb.write('front', buf)
    for vals in bad:
        arr = np.asarray(vals, np.float32)
        rc = lib.fl_filter(mgr.fb.ctx, _lib.FILT['bloom'], dim.w, dim.h, arr.ctypes.data, len(arr))
        assert rc == _lib.FL_E_INVAL, (rc, len(vals))
    assert np.array_equal(mgr.fb.read('front', buf.shape, np.float32).view(np.uint32), buf.view(np.uint32))     # nothing ran
    assert not np.array_equal(run_filter(mgr, 'bloom', dim, buf, atlimit), buf)
    assert np.array_equal(run_filter(mgr, 'bloom', dim, buf, [np.float32(0.0), np.float32(0.0), np.float32(1.0)]), buf)


def test_scalars_refuse_radius_times_width_over_the_limit(built):
    gnm, prof = configs.cfg2()
    gprof = profile.wrap(dict(prof, width=3840, height=2160, filter_order=['logscale', 'bloom', 'colorclip'],
                              filters={'bloom': {'radius': 64.5 / 12}}), gnm)
    dim = render.Framebuffers.calc_dim(3840, 2160)
    with pytest.raises(ValueError, match='384'):
        filters.Bloom().scalars(gprof, gprof.filters.bloom, dim, 0.5)


# ------------------------------------------------------------------ in a chain
def test_chain_against_the_oracle_with_the_models_bloom(mgr):
    """yuv, logscale, bloom, colorclip on a synthetic accumulator: against the oracle's yuv and logscale, the model's bloom and the
    float64 model of colorclip, per branch class under the bars tests/test_gpu_tone.py holds colorclip to (32 x the float32
    oracle's own deviation from the model on the same input, at least 32 x 2^-24 of the class's largest value)."""
    lib = _lib.load()
    dim, d = mgr.fb.calc_dim(*BIG), O.calc_dim(*BIG)
    acc = synth_accum(dim)
    sigma = 5.0
    log = [np.float32(T.LOG_K1), np.float32(0.002)]
    clip = [np.float32(0.9), np.float32(1.5), np.float32(0.25), np.float32(0.01), TM.lingam_of(0.25, 0.01)]
    chain = [('yuv', []), ('logscale', log), ('bloom', BM.params(THRESHOLD, STRENGTH, sigma)), ('colorclip', clip)]
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, dim.w, dim.h, 0))
    mgr.fb.write('front', acc)
    for name, vals in chain:
        arr = np.asarray(vals, np.float32)
        _lib.check(lib.fl_filter(mgr.fb.ctx, _lib.FILT[name], dim.w, dim.h, arr.ctypes.data, len(arr)))
    dev = mgr.fb.read('front', acc.shape, np.float32)

    logged = O.logscale(d, O.yuv_to_rgb(d, np.ascontiguousarray(acc)), *log)
    assert 0.05 < (logged[:, 3] > THRESHOLD).mean() < 0.95
    mid = BM.bloom(logged.reshape(dim.ah, dim.astride, 4), THRESHOLD, STRENGTH, sigma)[0].astype(np.float32).reshape(-1, 4)
    assert not np.array_equal(mid, logged)
    model, cls = TM.colorclip(mid, *clip)
    got = T.deviation('colorclip', dev, model, cls)
    own = T.deviation('colorclip', O.colorclip(d, mid, *clip), model, cls)
    scale = T.scale_of('colorclip', model, cls)
    assert len(got) >= 2
    for k, v in sorted(got.items()):
        bar = FACTOR * max(own[k], 2.0 ** -24 * scale[k])
        print('bloom chain, class %s: device %.3e bar %.3e (oracle %.3e)' % (k, v, bar, own[k]))
        report('chain, class %s: device %.3e bar %.3e' % (k, v, bar))
    for k, v in got.items():
        bar = FACTOR * max(own[k], 2.0 ** -24 * scale[k])
        assert v <= bar, 'class %s: device deviates %.3e from the model, bar %.3e (oracle %.3e)' % (k, v, bar, own[k])


def test_whole_frame_with_bloom_in_the_order(built):
    gnm, prof = configs.cfg2(samples=2 ** 20)
    gprof = profile.wrap(dict(prof, width=64, height=48, filter_order=['bilateral', 'logscale', 'bloom', 'colorclip']), gnm)
    m = render.RenderManager(device=0, host_seed=5)
    try:
        rdr = render.Renderer(gnm, gprof)
        assert [f.name for f in rdr.filts] == ['yuv', 'bilateral', 'logscale', 'bloom', 'colorclip']
        evt, h = m.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
        a = np.array(h).astype(np.float64)
    finally:
        m.fb.free()
    assert a.shape[:2] == (48, 64) and np.isfinite(a).all() and a[..., :3].max() > 0
