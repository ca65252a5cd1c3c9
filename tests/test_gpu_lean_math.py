"""
The device's lean math helpers, one at a time through the math tap (fl_debug_math: k_math_tap in csrc/iter.hip, compiled with
the iterate kernels' flags), against float64 — the bars, input sets and the float32 restatement are tests/lean_math_model.py's,
and tests/test_cpu_lean_math.py proves on the CPU that the restatement itself stays inside every bar.

  * bare instructions (v_rcp_f32, v_sqrt_f32, v_exp_f32, v_log_f32, v_sin_f32, v_cos_f32): twice the maxima recorded in DESIGN.md
    ("Accuracy of the lean math"), rounded up to half an ulp; the figures are printed again on every run;
  * composite helpers: the bar against float64, the special values bit for bit with the restatement, and — a separate test, so
    that a result which fails ONLY there is reported as such, with its inputs — the envelope of the restatements over every
    combination of +-1 ulp instruction errors, widened by 2 ulp of the result (lean_math_model.envelope_width).
"""
import numpy as np
import pytest

import lean_math_model as M
from cuburn_amd import render, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mgr(built):
    return render.RenderManager(device=0, nslots=1024, host_seed=7)


_results = {}


def tap(mgr, fn, name):
    """raw result bits of helper fn on input set `name` (one tap call per set and module run)"""
    if (fn, name) not in _results:
        a, b = M.input_sets(fn)[name]
        out = np.zeros(a.size, np.uint32)
        _lib.check(_lib.load().fl_debug_math(mgr.fb.ctx, _lib.MATH[fn], a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        _results[fn, name] = out
    return _results[fn, name]


BARE_CASES = [(fn, name) for fn in M.BARE for name in M.SET_NAMES[fn]]
CASES = [(fn, name) for fn in M.COMPOSITE for name in M.SET_NAMES[fn]]
ENV_CASES = [(fn, name) for fn, name in CASES if fn != 'trunca' and name not in ('uncovered', 'far')]
_ids = lambda cases: ['%s-%s' % c for c in cases]


@pytest.mark.parametrize('fn,name', BARE_CASES, ids=_ids(BARE_CASES))
def test_bare_instruction_within_twice_its_recorded_error(mgr, fn, name):
    a, b = M.input_sets(fn)[name]
    res = tap(mgr, fn, name)
    print(fn, name, 'measured:', M.bare_errors(fn, name, a, M.from_bits(res)), 'recorded:', M.MEASURED[fn], 'bar:', M.bare_bar(fn))
    fails, _, fig = M.judge(fn, name, a, b, res)
    print(fn, name, 'share of the bar used:', fig)
    assert not fails, fails[:3]


@pytest.mark.parametrize('fn,name', CASES, ids=_ids(CASES))
def test_helper_within_its_bar(mgr, fn, name):
    a, b = M.input_sets(fn)[name]
    fails, _, fig = M.judge(fn, name, a, b, tap(mgr, fn, name))
    print(fn, name, 'share of the bar used, counts:', fig)
    assert fig.get('uncovered', 0) == M.UNCOVERED.get((fn, name), 0)
    assert not fails, fails[:3]


@pytest.mark.parametrize('fn,name', ENV_CASES, ids=_ids(ENV_CASES))
def test_helper_within_the_envelope_of_the_restatements(mgr, fn, name):
    """A device form that has drifted from the source the restatement follows fails here even inside the float64 bar."""
    a, b = M.input_sets(fn)[name]
    _, env_fails, fig = M.judge(fn, name, a, b, tap(mgr, fn, name), with_envelope=True)
    assert fig['envelope'] > 0 or name == 'special'
    assert not env_fails, env_fails[:3]


def test_argument_validation(mgr):
    lib, ctx = _lib.load(), mgr.fb.ctx
    z, o = np.zeros(4, np.float32), np.zeros(4, np.uint32)
    ok = lambda *args: lib.fl_debug_math(*args)
    assert ok(ctx, 0, 4, z.ctypes.data, z.ctypes.data, o.ctypes.data) == _lib.FL_OK
    assert ok(None, 0, 4, z.ctypes.data, z.ctypes.data, o.ctypes.data) == _lib.FL_E_INVAL
    assert ok(ctx, 0, 4, None, z.ctypes.data, o.ctypes.data) == _lib.FL_E_INVAL
    assert ok(ctx, 0, 4, z.ctypes.data, None, o.ctypes.data) == _lib.FL_E_INVAL
    assert ok(ctx, 0, 4, z.ctypes.data, z.ctypes.data, None) == _lib.FL_E_INVAL
    assert ok(ctx, 0, 0, z.ctypes.data, z.ctypes.data, o.ctypes.data) == _lib.FL_E_INVAL
    for fn in (-1, len(M.FN), 1000):
        assert ok(ctx, fn, 4, z.ctypes.data, z.ctypes.data, o.ctypes.data) == _lib.FL_E_INVAL
    with pytest.raises(ValueError):
        _lib.check(ok(ctx, len(M.FN), 4, z.ctypes.data, z.ctypes.data, o.ctypes.data))
