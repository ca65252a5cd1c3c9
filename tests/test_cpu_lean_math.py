"""
The bars of the lean math helpers are satisfiable by the reference alone (no GPU): tests/lean_math_model.py restates every
composite helper of csrc/flame_device.h and csrc/variations.h in float32, operation for operation, with each hardware instruction
anywhere within +-1 ulp of the correctly rounded result, and this file holds that restatement — for every combination of those
instruction errors — to the same bars against float64 that tests/test_gpu_lean_math.py holds the device to.

Two helpers did not meet their bars when these tests were written, restatement and device alike, and were mended (the restatement
follows them):
  * fsin / fcos took v_fract_f32 of a NEGATIVE argument, which is 1 + t rounded to the 2^-24 grid below 1 (up to 2 pi 2^-24 = 3.7e-7
    of angle; fsin(x) = -3.745e-7 for every -1.9e-7 < x < 0): 1.5 to 3 x the bar c_hw + 2^-23 |x| for x < 0.  They take the fraction of
    |t| now (the sine gets the sign back); x >= 0 is unchanged bit for bit.  The sets are still judged in halves by sign.
  * v_sinh / v_cosh used the float32 log2 e alone, 1.93e-8 short: another 0.22 |x| 2^-24 of the result, 1.07 x the bar
    (8 + |x|) 2^-24 at |x| = 45.3 .. 46.6 where |x| log2 e is just above 64.  The exponent takes log2 e in two floats now.
"""
import numpy as np
import pytest

import lean_math_model as M

CASES = [(fn, name) for fn in M.COMPOSITE for name in M.SET_NAMES[fn]]


@pytest.mark.parametrize('fn,name', CASES, ids=['%s-%s' % c for c in CASES])
def test_restatement_stays_inside_its_bar(fn, name):
    a, b = M.input_sets(fn)[name]
    assert a.size == b.size and 0 < a.size <= 1 << 20
    fails, worst = [], {}
    for ks in M.KS[fn]:
        r, covered = M.MODEL[fn](a, b, ks)
        # the uncovered masks select what the source comment says, and nothing else
        assert int((~covered).sum()) == M.UNCOVERED.get((fn, name), 0), (fn, name, ks)
        f, _, fig = M.judge(fn, name, a, b, r if fn == 'trunca' else M.bits(r))
        fails += ['ks=%r %s' % (ks, x) for x in f]
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0), v)
    print(fn, name, worst)
    assert not fails, fails[:3]


def test_tap_numbers_match_the_header():
    """the FL_MATH_* enum of include/flame_hip.h, read from the header, against the binding's table (the tests' one name list)"""
    import os
    import re
    from common import REPO
    from cuburn_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    body = re.search(r'enum\s*\{([^}]*FL_MATH_COUNT[^}]*)\}', hdr).group(1)
    names = re.findall(r'FL_MATH_([A-Z0-9_]+)', body)
    assert re.search(r'FL_MATH_RCP\s*=\s*0\b', body) and len(re.findall(r'=', body)) == 1      # consecutive from 0
    assert names[-1] == 'COUNT' and len(names) == 20
    assert dict((n.lower(), i) for i, n in enumerate(names[:-1])) == _lib.MATH
    assert M.FN is _lib.MATH and set(M.MODEL) == set(_lib.MATH)


def test_uncovered_ranges_are_what_the_source_declares():
    a, b = M.input_sets('atan2')['uncovered']
    big = np.maximum(np.abs(a), np.abs(b))
    assert (((big > 2.0 ** 126) & np.isfinite(big)) | ((np.abs(a) < M.FLT_MIN) & (np.abs(b) < M.FLT_MIN) & (a != 0) & (b != 0))).all()
    assert not M.m_atan2(a, b)[1].any()
    # next to the ranges, on the covered side
    a, b = M.A([2.0 ** 126, 1e-45, 1e-45, np.inf, 0.0]), M.A([1.0, 0.0, M.FLT_MIN, 1.0, 1e-45])
    assert M.m_atan2(a, b)[1].all()
    a, b = M.input_sets('fmod')['uncovered']
    assert (np.abs(b) > 2.0 ** 126).all() and not M.m_fmod(a, b)[1].any()
    assert M.m_fmod(M.A([3.0, 1e38]), M.A([2.0 ** 126, -2.0 ** 126]))[1].all()


def test_specials():
    """The special values the source and its comments state, spelled out (the sets' `special` members are compared with the
    restatement bit for bit; here the restatement is compared with the statement)."""
    pi, pi2 = M.FM_PI, M.FM_PI_2
    want = [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.0, -0.0, 0.0), (-0.0, -0.0, -0.0),          # atan2(0, 0) = 0, a's sign
            (0.0, 1.0, 0.0), (-0.0, 1.0, -0.0), (0.0, -1.0, pi), (-0.0, -1.0, -pi),
            (1.0, 0.0, pi2), (1.0, -0.0, pi2), (-1.0, 0.0, -pi2), (-1.0, -0.0, -pi2),
            (1.0, np.inf, 0.0), (-1.0, np.inf, -0.0), (1.0, -np.inf, pi), (-1.0, -np.inf, -pi),
            (np.inf, 1.0, pi2), (-np.inf, -1.0, -pi2), (np.inf, 0.0, pi2)]
    for ks in M.KS['atan2']:
        for a, b, w in want:
            r = M.m_atan2(M.A([a]), M.A([b]), ks)[0]
            assert M.bits(r)[0] == M.bits(M.A([w]))[0], (a, b, r, w)
        for a, b in ((np.nan, 1.0), (1.0, np.nan), (np.inf, np.inf), (-np.inf, np.inf), (np.inf, -np.inf), (-np.inf, -np.inf)):
            assert np.isnan(M.m_atan2(M.A([a]), M.A([b]), ks)[0][0]), (a, b)
    for ks in M.KS['div']:
        r = M.m_div(M.A([1, -2.5, 1, 0, -0.0]), M.A([0.0, 0.0, -0.0, 0.0, 0.0]), ks)[0]
        assert r[0] == np.inf and r[1] == -np.inf and r[2] == -np.inf and np.isnan(r[3]) and np.isnan(r[4])
    for ks in M.KS['pow']:
        r = M.m_pow(M.A([0, 0, -1, -2.5]), M.A([0.5, 3, 2, 0.5]), ks)[0]
        assert M.bits(r)[0] == 0 and M.bits(r)[1] == 0 and np.isnan(r[2]) and np.isnan(r[3])
    x = M.A([0.0, -0.0, 1e-45, -1e-40, 88.7, -88.7, 89.5, -89.5, np.inf, -np.inf])
    for ks in M.KS['sinh']:
        s, c = M.m_sinh(x, ks=ks)[0], M.m_cosh(x, ks=ks)[0]
        assert (M.bits(s)[:4] == M.bits(x)[:4]).all()                         # +-0 and denormals come back as they went in
        assert np.isfinite(s[4:6]).all() and np.isfinite(c[4:6]).all()      # no overflow before the result's own
        assert (s[6:] == M.A([np.inf, -np.inf, np.inf, -np.inf])).all() and (c[6:] == np.inf).all()
        assert np.isnan(M.m_sinh(M.A([np.nan]), ks=ks)[0][0]) and np.isnan(M.m_cosh(M.A([np.nan]), ks=ks)[0][0])
    for fn in ('sinh', 'cosh'):
        for name in M.SET_NAMES[fn]:
            for ks in M.KS[fn]:
                a = M.input_sets(fn)[name][0]
                assert (M.m_cosh(a[~np.isnan(a)], ks=ks)[0] >= 1).all(), (name, ks)
    for fn in ('sin', 'cos', 'tan'):
        assert np.isnan(M.MODEL[fn](M.A([np.inf, -np.inf, np.nan]))[0]).all()


def test_specials_do_not_depend_on_the_instruction_errors():
    for fn, name in (('atan2', 'special'), ('div', 'special')):
        a, b = M.input_sets(fn)[name]
        assert M.model_constant(fn, a, b)[1].all(), (fn, name)


def test_trunca_statement():
    """round to nearest EVEN, saturating, NaN -> 0: spelled out, not taken from the restatement's own rint"""
    f = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.49999997, 1023.5, 1024.5, 2.0 ** 31 - 128, 2.0 ** 31, 2.0 ** 32, np.inf,
         -2.0 ** 31, -2.0 ** 31 * (1 + 2.0 ** -23), -2.0 ** 32, -np.inf, np.nan, -0.0, 8388607.5]
    want = [0, 2, 2, 0, -2, -2, 0, 1024, 1024, 2 ** 31 - 128, 0x7fffffff, 0x7fffffff, 0x7fffffff,
            -2 ** 31, -2 ** 31, -2 ** 31, -2 ** 31, 0, 0, 8388608]
    got = M.m_trunca(M.A(f))[0]
    assert got.view(np.int32).tolist() == want
    k = np.arange(-1024, 1025)
    ties = M.m_trunca(M.r32(k + 0.5))[0].view(np.int32)
    assert (ties % 2 == 0).all() and (np.abs(ties - (k + 0.5)) == 0.5).all()


def test_bare_bars_are_twice_the_measured_maximum_rounded_up_to_half_an_ulp():
    assert M.bare_bar('rcp') == (2.0, None) and M.bare_bar('sqrt') == (2.0, None) and M.bare_bar('exp2') == (2.0, None)
    assert M.bare_bar('log2') == (2.0, 2.0 * 2.0 ** -24)
    assert M.bare_bar('hw_sin')[1] == 4.5 * 2.0 ** -24 and M.bare_bar('hw_cos')[1] == 4.5 * 2.0 ** -24
    for fn, (u, a) in M.MEASURED.items():
        for m, bar in zip((u, a), (M._bar_of(u), M._bar_of(a))):
            assert m is None or (2 * m <= bar < 2 * m + 0.5 and bar % 0.5 == 0)
    assert M.C_HW >= max(M.MEASURED['hw_sin'][1], M.MEASURED['hw_cos'][1]) * 2.0 ** -24 * 0.999


def test_fmod_pi_clause_serves_at_most_one_percent():
    for name in M.SET_NAMES['fmod_pi']:
        a, b = M.input_sets('fmod_pi')[name]
        _, _, fig = M.judge('fmod_pi', name, a, b, M.bits(M.m_fmod_pi(a)[0]))
        assert fig['pi clause share'] <= 0.01, (name, fig)
