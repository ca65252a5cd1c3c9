"""
CPU restatement of the device's lean math helpers (cuburn_amd/csrc/flame_device.h, cuburn_amd/csrc/variations.h), their float64 truth,
the input sets and the bars of tests/test_cpu_lean_math.py and tests/test_gpu_lean_math.py.

Restatement rules.  float32 arithmetic, operation for operation as the source is written (it is compiled with -ffp-contract=off):
a multiply or add rounds to float32 after each step; fmaf is a float64 product and sum rounded ONCE to float32 (the product of two
float32 is exact in float64); denormals are kept by plain arithmetic.  A hardware instruction (v_rcp_f32, v_sqrt_f32, v_exp_f32,
v_log_f32, v_sin_f32, v_cos_f32) is the correctly rounded float64 result moved by k float32 ulps, k in {-1, 0, +1}: the bracket of a
"1 ulp" instruction; results that are 0, infinite or NaN are not moved, and a denormal input or result of such an instruction is
flushed to zero.  A helper with several instructions takes one k per instruction (`ks`, in source order); `KS[fn]` lists every
combination.  Where the source declares a range uncovered the model returns libm's answer and covered = False.

Every model function returns (result float32 array, covered bool array).
"""
import itertools

import numpy as np

f32, f64 = np.float32, np.float64
FLT_MIN = f32(1.17549435e-38)
DENORM_MIN = f32(1e-45)
FM_PI = f32(3.14159274101257)
FM_PI_2 = f32(1.57079637050629)
FM_LOG2E = f32(1.44269502162933)
LOG2E_LO = f32(1.925963e-8)                       # variations.h V_LOG2E_LO: log2 e - FM_LOG2E
LN2_F = f32(0.69314718246460)
INV_2PI_F = f32(0.15915494309189532)
INV_PI_F = f32(0.318309886183791)
U = 2.0 ** -24                                    # half a float32 ulp, relative
NAN = f32(np.nan)

# include/flame_hip.h FL_MATH_* (tests/test_cpu_lean_math.py reads the enum itself and compares)
from cuburn_amd._lib import MATH as FN  # noqa: E402


def A(x):
    return np.ascontiguousarray(x, dtype=f32)


def r32(x):
    """float64 -> float32, one rounding (overflow to inf is the rounding's own)"""
    with np.errstate(over='ignore', invalid='ignore'):
        return np.asarray(x, f64).astype(f32)


def mul(a, b):
    with np.errstate(all='ignore'):
        return r32(a.astype(f64) * b.astype(f64))


def add(a, b):
    with np.errstate(all='ignore'):
        return r32(a.astype(f64) + b.astype(f64))


def sub(a, b):
    with np.errstate(all='ignore'):
        return r32(a.astype(f64) - b.astype(f64))


def fma(a, b, c):
    with np.errstate(all='ignore'):
        return r32(np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64))


def bits(x):
    return A(x).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(f32)


def move_ulps(x, n):
    """float32 array moved by n ulps (towards +inf for n > 0); zeros, infinities and NaN stay"""
    x = A(x).copy()
    go = np.isfinite(x) & (x != 0)
    for _ in range(abs(int(n))):
        x[go] = np.nextafter(x[go], f32(np.inf if n > 0 else -np.inf))
    return x


def ulp_of(t):
    """float32 ulp at the magnitude of the float64 value t (2^-149 below FLT_MIN)"""
    _, e = np.frexp(np.abs(np.asarray(t, f64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def _flush(x):
    x = A(x).copy()
    den = (np.abs(x) < FLT_MIN) & (x != 0)
    x[den] = np.copysign(f32(0), x[den])
    return x


def hw(op, x, k):
    """One hardware instruction: correctly rounded from float64, moved by k ulps; denormals in and out flushed."""
    x = _flush(x).astype(f64)
    with np.errstate(all='ignore'):
        if op == 'rcp':
            t = 1.0 / x
        elif op == 'sqrt':
            t = np.sqrt(x)
        elif op == 'exp2':
            t = np.exp2(x)
        elif op == 'log2':
            t = np.log2(x)
        elif op in ('sin', 'cos'):
            # argument in revolutions.  (The ISA manual gives +-256 revolutions as the valid domain; an MI355X reduces every finite
            # argument exactly — probed through the tap up to 2^20 + 1/4 — and so does this model.  The helpers never rely on it:
            # v_fract_f32 comes first.  The bare instructions are measured and held to their bars inside the documented domain.)
            t = np.where(np.isfinite(x), sin_rev(x) if op == 'sin' else cos_rev(x), np.nan)
        else:
            raise KeyError(op)
    r = _flush(move_ulps(r32(t), k))
    return np.clip(r, f32(-1), f32(1)) if op in ('sin', 'cos') else r      # (a sine moved above 1 is no bracket of anything)


def sin_rev(x):
    """sin(2 pi x) in float64, x in revolutions: reduced EXACTLY to [-1/4, 1/4] first, so that the result next to a zero of the sine
    keeps its relative accuracy (sin(2 pi * 0.5) is 0, not pi's rounding error)"""
    x = np.asarray(x, f64)
    with np.errstate(invalid='ignore'):
        red = x - np.rint(x)                                            # [-1/2, 1/2], exact
        red = np.where(np.abs(red) > 0.25, np.copysign(0.5, red) - red, red)
        return np.where(x == 0, x, np.sin(2 * np.pi * red))              # (sin(-0) = -0)


def cos_rev(x):
    x = np.asarray(x, f64)
    with np.errstate(invalid='ignore'):
        return np.sin(2 * np.pi * (0.25 - np.abs(x - np.rint(x))))       # the difference is exact


def fract(t):
    """v_fract_f32: t - floor(t), never 1.0 (clamped to the float below)"""
    t = A(t)
    with np.errstate(all='ignore'):
        fr = np.minimum(sub(t, np.floor(t)), f32(0.99999994))
    return np.where(np.isfinite(t), fr, NAN).astype(f32)


# ---- the helpers ------------------------------------------------------------------------------------------------------------
def _all(a):
    return np.ones(A(a).shape, bool)


def m_rcp(a, b=None, ks=(0,)):
    return hw('rcp', a, ks[0]), _all(a)


def m_sqrt(a, b=None, ks=(0,)):
    return hw('sqrt', a, ks[0]), _all(a)


def m_exp2(a, b=None, ks=(0,)):
    return hw('exp2', a, ks[0]), _all(a)


def m_log2(a, b=None, ks=(0,)):
    return hw('log2', a, ks[0]), _all(a)


def m_hw_sin(a, b=None, ks=(0,)):
    return hw('sin', a, ks[0]), _all(a)


def m_hw_cos(a, b=None, ks=(0,)):
    return hw('cos', a, ks[0]), _all(a)


def m_div(a, b, ks=(0,)):
    return mul(A(a), hw('rcp', b, ks[0])), _all(a)


def m_exp(a, b=None, ks=(0,)):
    return hw('exp2', mul(A(a), np.full_like(A(a), FM_LOG2E)), ks[0]), _all(a)


def m_log(a, b=None, ks=(0,)):
    return mul(hw('log2', a, ks[0]), np.full_like(A(a), LN2_F)), _all(a)


def m_pow(a, b, ks=(0, 0)):
    return hw('exp2', mul(A(b), hw('log2', a, ks[0])), ks[1]), _all(a)


def m_sin(a, b=None, ks=(0,)):
    t = mul(A(a), np.full_like(A(a), INV_2PI_F))
    return hw('sin', np.copysign(fract(np.abs(t)), t), ks[0]), _all(a)


def m_cos(a, b=None, ks=(0,)):
    return hw('cos', fract(np.abs(mul(A(a), np.full_like(A(a), INV_2PI_F)))), ks[0]), _all(a)


def m_tan(a, b=None, ks=(0, 0, 0)):
    s, c = m_sin(a, ks=ks[0:1])[0], m_cos(a, ks=ks[1:2])[0]
    return mul(s, hw('rcp', c, ks[2])), _all(a)


def m_atan2(a, b, ks=(0,)):
    a, b = A(a), A(b)
    ax, ay = np.abs(b), np.abs(a)
    with np.errstate(all='ignore'):
        mx = np.fmax(np.fmax(ax, ay), FLT_MIN)
        mn = np.fmin(ax, ay)
        q = mul(mn, hw('rcp', mx, ks[0]))
        s = mul(q, q)
        p = fma(s, f32(-0.004355378448963165), f32(0.023040037602186203))
        for c in (-0.05777344852685928, 0.09794224053621292, -0.13976578414440155, 0.19962702691555023, -0.3333165943622589):
            p = fma(s, p, f32(c))
        r = fma(mul(q, s), p, q)
        r = np.where(ay > ax, sub(np.full_like(r, FM_PI_2), r), r)
        r = np.where(b < 0, sub(np.full_like(r, FM_PI), r), r)
        r = np.where(np.isnan(a) | np.isnan(b), NAN, r)
        r = np.copysign(r, a).astype(f32)
        big = np.fmax(ax, ay)
        covered = ~((big > f32(2.0 ** 126)) & np.isfinite(big)) & ~((ax < FLT_MIN) & (ay < FLT_MIN) & (ax > 0) & (ay > 0))
        lib = r32(np.arctan2(a.astype(f64), b.astype(f64)))
    return np.where(covered, r, lib).astype(f32), covered


def m_cosh(a, b=None, ks=(0, 0)):
    x = A(a)
    h = hw('exp2', fma(np.abs(x), FM_LOG2E, fma(np.abs(x), LOG2E_LO, f32(-1))), ks[0])
    return fma(f32(0.25), hw('rcp', h, ks[1]), h), _all(a)


def m_sinh(a, b=None, ks=(0, 0)):
    x = A(a)
    ax = np.abs(x)
    h = hw('exp2', fma(ax, FM_LOG2E, fma(ax, LOG2E_LO, f32(-1))), ks[0])
    big, x2 = fma(f32(-0.25), hw('rcp', h, ks[1]), h), mul(x, x)
    p = fma(x2, f32(2.7557319e-6), f32(1.9841270e-4))
    p = fma(x2, p, f32(8.3333333e-3))
    p = fma(x2, p, f32(1.6666667e-1))
    with np.errstate(invalid='ignore'):
        return np.where(ax < f32(0.5), fma(mul(x, x2), p, x), np.copysign(big, x)).astype(f32), _all(a)


def libm_fmod(a, b):
    with np.errstate(all='ignore'):
        return np.fmod(A(a), A(b)).astype(f32)          # float32 in, float32 out: the exact remainder


def fmod_lean_mask(a, b, ks=(0,)):
    with np.errstate(all='ignore'):
        return np.abs(mul(A(a), hw('rcp', b, ks[0]))) < f32(2097152.0)


def m_fmod(a, b, ks=(0,)):
    a, b = A(a), A(b)
    with np.errstate(all='ignore'):
        qf = mul(a, hw('rcp', b, ks[0]))
        lean = np.abs(qf) < f32(2097152.0)
        r = fma(-np.trunc(qf), b, a)
        sb = np.copysign(b, a)
        r = np.where(np.abs(r) >= np.abs(b), sub(r, sb), r)
        r = np.where((r != 0) & ((r < 0) != (a < 0)), add(r, sb), r)
        r = np.copysign(r, a).astype(f32)
        lib = libm_fmod(a, b)
        covered = ~(lean & (np.abs(b) > f32(2.0 ** 126)))
    return np.where(lean & covered, r, lib).astype(f32), covered


def m_fmod_pi(a, b=None, ks=()):
    a = A(a)
    return fma(np.full_like(a, -FM_PI), np.floor(mul(a, np.full_like(a, INV_PI_F))), a), _all(a)


def m_trunca(a, b=None, ks=()):
    """-> uint32 bits of the saturating round-to-nearest-even, NaN -> 0"""
    f = A(a)
    with np.errstate(all='ignore'):
        c = np.fmin(np.fmax(f, f32(-2147483648.0)), f32(2147483520.0))
        i = np.where(np.isnan(c), 0, np.rint(c.astype(f64))).astype(np.int64)
        i = np.where(f >= f32(2147483648.0), 0x7fffffff, i)
        i = np.where(np.isnan(f), 0, i)
    return (i & 0xffffffff).astype(np.uint32), _all(a)


MODEL = dict(rcp=m_rcp, div=m_div, sqrt=m_sqrt, exp2=m_exp2, log2=m_log2, exp=m_exp, log=m_log, pow=m_pow, sin=m_sin, cos=m_cos,
             tan=m_tan, atan2=m_atan2, sinh=m_sinh, cosh=m_cosh, fmod=m_fmod, fmod_pi=m_fmod_pi, trunca=m_trunca,
             hw_sin=m_hw_sin, hw_cos=m_hw_cos)
NINSTR = dict(rcp=1, div=1, sqrt=1, exp2=1, log2=1, exp=1, log=1, pow=2, sin=1, cos=1, tan=3, atan2=1, sinh=2, cosh=2, fmod=1,
              fmod_pi=0, trunca=0, hw_sin=1, hw_cos=1)
KS = dict((fn, list(itertools.product((-1, 0, 1), repeat=n))) for fn, n in NINSTR.items())
BARE = ('rcp', 'sqrt', 'exp2', 'log2', 'hw_sin', 'hw_cos')
COMPOSITE = ('div', 'exp', 'log', 'pow', 'sin', 'cos', 'tan', 'atan2', 'sinh', 'cosh', 'fmod', 'fmod_pi', 'trunca')


def envelope(fn, a, b):
    """(lowest, highest) result of the restatement over every combination of instruction errors; NaN where any is NaN"""
    lo = hi = None
    for ks in KS[fn]:
        r = MODEL[fn](a, b, ks)[0].astype(f64)
        with np.errstate(invalid='ignore'):
            lo = r if lo is None else np.where(np.isnan(r) | np.isnan(lo), np.nan, np.minimum(lo, r))
            hi = r if hi is None else np.where(np.isnan(r) | np.isnan(hi), np.nan, np.maximum(hi, r))
    return lo, hi


# ---- float64 truth -------------------------------------------------------------------------------------------------------------
def truth(fn, a, b=None):
    a = A(a).astype(f64)
    b = None if b is None else A(b).astype(f64)
    with np.errstate(all='ignore'):
        if fn == 'rcp': return 1.0 / a
        if fn == 'div': return a / b
        if fn == 'sqrt': return np.sqrt(a)
        if fn == 'exp2': return np.exp2(a)
        if fn == 'log2': return np.log2(a)
        if fn == 'exp': return np.exp(a)
        if fn == 'log': return np.log(a)
        if fn == 'pow': return np.power(a, b)
        if fn == 'sin': return np.sin(a)
        if fn == 'cos': return np.cos(a)
        if fn == 'tan': return np.tan(a)
        if fn == 'atan2': return np.arctan2(a, b)
        if fn == 'sinh': return np.sinh(a)
        if fn == 'cosh': return np.cosh(a)
        if fn == 'fmod': return np.fmod(a, b)                     # exact in float64 for float32 operands
        if fn == 'fmod_pi': return a - f64(FM_PI) * np.floor(a / f64(FM_PI))
        if fn == 'hw_sin': return np.where(np.isfinite(a), sin_rev(a), np.nan)
        if fn == 'hw_cos': return np.where(np.isfinite(a), cos_rev(a), np.nan)
    raise KeyError(fn)


# ---- bars ----------------------------------------------------------------------------------------------------------------------
# Bare instructions: measured on an MI355X against float64 ("Accuracy of the lean math"; tests/test_gpu_lean_math.py
# prints the figures again on every run), maxima over the sets below.  The test bar is TWICE the recorded maximum rounded up to the
# next 0.5 ulp: the sample is not exhaustive.  `ulp` holds for results of normal magnitude; `abs` (in units of 2^-24) is the
# absolute form: LOG2 on [0.5, 2], where the result passes through 0 and an error of a fraction of 2^-24 is many ulp of it, and
# HW_SIN / HW_COS everywhere.  (As measured, both forms hold together: v_log_f32 keeps its ulp through x = 1, and the sine and
# cosine stay within 10 ulp of the result right up to their zeros — the tests assert both.)
MEASURED = {
    # fn: (max ulp error on normal results, max absolute error / 2^-24 where the absolute form applies)
    'rcp': (0.869, None), 'sqrt': (0.917, None), 'exp2': (0.774, None), 'log2': (0.99987, 0.997),
    'hw_sin': (9.82, 2.104), 'hw_cos': (9.82, 2.078),
}
C_HW = 1.2542e-7      # measured absolute error of the bare sine and cosine on [0, 1) revolutions (sine 1.2541e-7, cosine 1.2387e-7)


def _bar_of(m):
    return None if m is None else float(np.ceil(2.0 * m / 0.5) * 0.5)


def bare_bar(fn):
    """(ulp bar, absolute bar) of a bare instruction: twice the measured maximum, rounded up to 0.5 ulp (0.5 * 2^-24)"""
    u, a = MEASURED[fn]
    return _bar_of(u), (None if a is None else _bar_of(a) * U)


def log2_err_bar(x):
    """Bound on |v_log_f32(x) - log2 x|: the ulp bar, or the absolute one on [0.5, 2]"""
    bu, ba = bare_bar('log2')
    t = np.log2(np.asarray(x, f64))
    return np.where((x >= 0.5) & (x <= 2.0), np.maximum(ba, 0.0), bu * ulp_of(t))


def sin_arg_bar(x):
    """fsin / fcos: c_hw + 2^-23 |x| (the float32 rounding of x / 2 pi), |x| <= 2^20"""
    return C_HW + 2.0 ** -23 * np.abs(np.asarray(x, f64))


TAN_COS_CUT = 2.0 ** -6


def tan_bar(x):
    """ftan = fsin * frcp(fcos) with |sin error|, |cos error| <= E = sin_arg_bar(x), the reciprocal within its bar and one rounding of
    the product: |(s + es) / (c + ec) (1 + rho) - s / c| <= (|s| + E) / (|c| - E) rho + E (|s| + |c|) / (|c| (|c| - E)).
    Compared only where |cos x| >= 2^-6 and |cos x| >= 2 E (past that the quotient's own error has no useful bound).
    -> (bar, compared mask)"""
    x = np.asarray(x, f64)
    s, c, E = np.abs(np.sin(x)), np.abs(np.cos(x)), sin_arg_bar(x)
    rho = (1 + bare_bar('rcp')[0] * 2 * U) * (1 + U) - 1
    use = (c >= TAN_COS_CUT) & (c >= 2 * E) & (np.abs(x) <= 2.0 ** 20)
    with np.errstate(all='ignore'):
        bar = (s + E) / (c - E) * rho + E * (s + c) / (c * (c - E))
    return bar, use


def div_bar(t):
    """fdiv = a * rcp(b): the reciprocal's bar and one rounding, relative (normal quotient and reciprocal)"""
    return ((1 + bare_bar('rcp')[0] * 2 * U) * (1 + U) - 1) * np.abs(t)


def exp_bar(x):
    """fexp = exp2(x * log2e_f): the exponent carries the constant's error and one rounding, |t| (eps + 2^-24), into the result as
    2^d - 1; then the instruction's bar.  Relative, for results of normal magnitude."""
    x = np.asarray(x, f64)
    eps = abs(f64(FM_LOG2E) - np.log2(np.e)) / np.log2(np.e)
    d = np.abs(x * np.log2(np.e)) * (eps + U * (1 + eps))
    return np.exp(x) * ((1 + bare_bar('exp2')[0] * 2 * U) * np.exp2(d) - 1)


def log_bar(x):
    """flog = log2(x) * ln2_f: |err| <= |log2 x| (|ln2_f - ln 2| + ln2_f 2^-24) + e_log2 ln2_f (1 + 2^-24)"""
    x = np.asarray(x, f64)
    c = f64(LN2_F)
    return np.abs(np.log2(x)) * (abs(c - np.log(2.0)) + c * U) + log2_err_bar(x) * c * (1 + U)


def pow_bar(x, y):
    """fpow = exp2(y * log2 x): the exponent is off by |y| e_log2 + |y log2 x| 2^-24; relative error 2^d (1 + exp2 bar) - 1"""
    x, y = np.asarray(x, f64), np.asarray(y, f64)
    d = np.abs(y) * log2_err_bar(x) * (1 + U) + np.abs(y * np.log2(x)) * U
    return np.power(x, y) * ((1 + bare_bar('exp2')[0] * 2 * U) * np.exp2(d) - 1)


ATAN2_BAR = 6e-7                                  # absolute everywhere; relative in the first octant
def hyp_bar(x):
    """v_sinh / v_cosh, relative: (8 + |x|) 2^-24 up to |x| = 88 (the |x| term: the float32 rounding of |x| log2 e)"""
    return (8.0 + np.abs(np.asarray(x, f64))) * U
SINH_SERIES_BAR = 2.0 ** -23                      # relative, |x| < 0.5


# ---- input sets (fixed seeds) -------------------------------------------------------------------------------------------------
def _signs(rs, n):
    return rs.choice(f32([-1, 1]), n)


def _logu(rs, n, lo, hi):
    """log-uniform magnitudes in 2^lo .. 2^hi"""
    return r32(np.exp2(rs.uniform(lo, hi, n)))


def _near(vals, n):
    """every float32 within n ulps of each value"""
    v = A(vals).reshape(-1, 1)
    i = v.view(np.int32).astype(np.int64) + np.arange(-n, n + 1)      # sign-magnitude order: fine away from 0
    return i.astype(np.int32).view(f32).ravel()


def _pair(a, b=None):
    a = A(a)
    return a, (np.zeros_like(a) if b is None else A(b))


_cache = {}


def input_sets(fn):
    """-> {set name: (a, b)} float32 arrays of at most 2^20 elements (b is zeros for unary helpers)"""
    if fn not in _cache:
        _cache[fn] = _SETS[fn]()
    return _cache[fn]


def _sets_rcp():
    n = 1 << 20
    x = r32(np.exp2(np.linspace(-126, 126, n))) * np.where(np.arange(n) & 1, f32(-1), f32(1))
    return {'log': _pair(x), 'edge': _pair([0.0, -0.0, np.inf, -np.inf, np.nan, 1, -1, 2, FLT_MIN, 2.0 ** 126])}


def _sets_sqrt():
    x = r32(np.exp2(np.linspace(-126, 127.99, 1 << 20)))
    return {'log': _pair(x), 'edge': _pair([0.0, np.inf, -1.0, np.nan, 1, 4, 2, FLT_MIN])}


def _sets_exp2():
    n = 1 << 20
    x = r32(np.exp2(np.linspace(-30, np.log2(125.9), n))) * np.where(np.arange(n) & 1, f32(-1), f32(1))
    return {'log': _pair(x), 'edge': _pair([0.0, -0.0, -np.inf, np.inf, np.nan, 1, -1, -126, 127, 128, -150])}


def _sets_log2():
    x = r32(np.exp2(np.linspace(-126, 127.99, 1 << 20)))
    x = x[(x < 0.5) | (x > 2.0)]
    near1 = np.random.RandomState(11).uniform(0.5, 2.0, (1 << 20) - 129)
    return {'log': _pair(x), 'near1': _pair(np.concatenate([r32(near1), _near([1.0], 64)])),
            'edge': _pair([1.0, 0.0, np.inf, -1.0, np.nan, 2, 0.5, 4, FLT_MIN])}


def _sets_hw_trig():
    n = 1 << 20
    rs = np.random.RandomState(12)
    x = r32(np.exp2(np.linspace(-30, 8, n))) * np.where(np.arange(n) & 1, f32(-1), f32(1))
    return {'log': _pair(x), 'unit': _pair(np.minimum(r32(rs.uniform(0, 1, n)), f32(0.99999994))),
            'wide': _pair(r32(rs.uniform(-256, 256, n))),
            'edge': _pair([0.0, 0.25, 0.5, 0.75, 0.125, 1.0, -0.25, 256.0, np.inf, -np.inf, np.nan])}


ATAN2_SPECIALS = [(a, b) for a in (0.0, -0.0) for b in (0.0, -0.0)] + \
    [(a, b) for a in (0.0, -0.0) for b in (1.0, -1.0, 1e-30, -1e30)] + \
    [(a, b) for a in (1.0, -1.0, 1e-30, -1e30) for b in (0.0, -0.0)] + \
    [(np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.nan, 0.0), (np.inf, np.nan)] + \
    [(a, b) for a in (np.inf, -np.inf) for b in (np.inf, -np.inf)] + \
    [(a, b) for a in (np.inf, -np.inf) for b in (1.0, -1.0, 0.0, -0.0)] + \
    [(a, b) for a in (1.0, -1.0, 0.0, -0.0) for b in (np.inf, -np.inf)]


def _sets_atan2():
    rs = np.random.RandomState(20)
    n = 1 << 18
    uni = (r32(rs.uniform(-2, 2, n)), r32(rs.uniform(-2, 2, n)))
    log = (_logu(rs, n, -120, 120) * _signs(rs, n), _logu(rs, n, -120, 120) * _signs(rs, n))
    # octant boundaries: the diagonals (|a| = |b| moved by 0, +-1, +-2 ulp) and the axes (one operand +-0, +-denorm_min, +-FLT_MIN
    # next to a normal one)
    m = 1 << 15
    base = _logu(rs, m, -20, 20)
    moved = base.copy()
    j = rs.randint(-2, 3, m)
    for d in (-2, -1, 1, 2):
        moved[j == d] = move_ulps(base[j == d], d)
    sw = rs.rand(m) < 0.5
    da, db = np.where(sw, moved, base) * _signs(rs, m), np.where(sw, base, moved) * _signs(rs, m)
    tiny = rs.choice(f32([0.0, 1e-45, 1.17549435e-38]), m) * _signs(rs, m)
    other = _logu(rs, m, -20, 20) * _signs(rs, m)
    sw = rs.rand(m) < 0.5
    octant = (np.concatenate([da, np.where(sw, tiny, other)]), np.concatenate([db, np.where(sw, other, tiny)]))
    sp = np.array(ATAN2_SPECIALS, f32)
    # the ranges the source declares uncovered: max(|a|, |b|) above 2^126 (finite), both operands denormal
    k = 256
    ua = np.concatenate([_logu(rs, k, 126.01, 127.9) * _signs(rs, k), _logu(rs, k, -30, 127) * _signs(rs, k),
                         r32(rs.randint(1, 1 << 23, k)).astype(np.uint32).view(f32) * _signs(rs, k)])
    ub = np.concatenate([_logu(rs, k, -30, 127) * _signs(rs, k), _logu(rs, k, 126.01, 127.9) * _signs(rs, k),
                         r32(rs.randint(1, 1 << 23, k)).astype(np.uint32).view(f32) * _signs(rs, k)])
    return {'uniform': uni, 'log': log, 'octant': octant, 'special': (A(sp[:, 0]), A(sp[:, 1])), 'uncovered': (A(ua), A(ub))}


HYP_BANDS = ((0, 0.5), (0.5, 2), (2, 10), (10, 40), (40, 88))
HYP_SPECIALS = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 88.7, -88.7, 89.5, -89.5, np.inf, -np.inf, np.nan]


def _sets_hyp():
    rs = np.random.RandomState(30)
    n = 1 << 16
    sets = {'switch': _pair(_near([0.5, -0.5], 64)), 'special': _pair(HYP_SPECIALS)}
    for lo, hi in HYP_BANDS:
        sets['band %g-%g' % (lo, hi)] = _pair(np.minimum(r32(rs.uniform(lo, hi, n)), f32(88)) * _signs(rs, n))
    return sets


FMOD_SPECIALS = [(a, b) for a in (1.5, -1.5, 0.0, -0.0, np.inf, np.nan) for b in (0.0, -0.0, np.nan, 2.0)] + \
    [(np.inf, 1.0), (-np.inf, -3.0), (np.nan, 1.0)]


def _sets_fmod():
    rs = np.random.RandomState(40)
    n = 1 << 18
    uni = (r32(rs.uniform(-20, 20, n)), r32(rs.uniform(-3, 3, n)))
    e = np.log2(np.e) * 30
    log = (_logu(rs, n, -e, e) * _signs(rs, n), _logu(rs, n, -e, e) * _signs(rs, n))
    b = np.where(rs.rand(n) < 0.5, r32(rs.uniform(-3, 3, n)), _logu(rs, n, -20, 20) * _signs(rs, n)).astype(f32)
    m = rs.randint(-999, 1000, n)
    a = mul(r32(m), b)
    j = rs.randint(-1, 2, n)
    for d in (-1, 1):
        a[j == d] = move_ulps(a[j == d], d)
    sb = r32(rs.uniform(0.5, 3, 1 << 14)) * _signs(rs, 1 << 14)
    sa = r32(sb.astype(f64) * 2.0 ** 21 * (1 + rs.uniform(-1, 1, sb.size) * 2.0 ** -10)) * _signs(rs, sb.size)
    sp = np.array(FMOD_SPECIALS, f32)
    k = 256
    ub = np.concatenate([_logu(rs, k, 126.01, 127.9) * _signs(rs, k), f32([np.inf, -np.inf])])
    ua = np.concatenate([_logu(rs, k, 100, 127.9) * _signs(rs, k), f32([1.0, -2.0])])
    return {'uniform': uni, 'log': log, 'multiples': (A(a), A(b)), 'straddle': (A(sa), A(sb)),
            'special': (A(sp[:, 0]), A(sp[:, 1])), 'uncovered': (A(ua), A(ub))}


TRIG_SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan]


def _sets_trig():
    rs = np.random.RandomState(50)
    n = 1 << 18
    kk = np.arange(-64, 65)
    zeros = np.concatenate([_near(r32(kk[kk != 0] * (np.pi / 2)), 8), np.arange(-8, 9) * DENORM_MIN])
    sets = {'far': _pair([2.0 ** 24, -2.0 ** 24, 2.0 ** 30, -2.0 ** 30]), 'special': _pair(TRIG_SPECIALS)}
    # each set is judged in two halves, by the sign of the argument: v_fract_f32 of a negative argument rounds (1 + t), which is why
    # fsin / fcos take the fraction of |t|; a helper that took it of t would fail the x < 0 halves alone
    for name, x in (('pi', r32(rs.uniform(-np.pi, np.pi, n))), ('log', _logu(rs, n, -30, 20) * _signs(rs, n)), ('zeros', A(zeros))):
        neg = np.signbit(x)
        sets[name + ' x>=0'], sets[name + ' x<0'] = _pair(x[~neg]), _pair(x[neg])
    return sets


def _sets_pow():
    rs = np.random.RandomState(60)
    n = 1 << 18
    m = 1 << 10
    y = r32(rs.uniform(-4, 4, m))
    x = _logu(rs, m, -60, 60)
    lines = (np.concatenate([np.zeros(m, f32), -x, x, np.ones(m, f32)]),
             np.concatenate([np.abs(y) + f32(1e-3), y, np.zeros(m, f32), y]))
    return {'main': (_logu(rs, n, -60, 60), r32(rs.uniform(-4, 4, n))), 'lines': (A(lines[0]), A(lines[1]))}


def _sets_exp():
    rs = np.random.RandomState(61)
    n = 1 << 18
    return {'uniform': _pair(r32(rs.uniform(-87, 87, n))), 'log': _pair(_logu(rs, n, -30, 6) * _signs(rs, n))}


def _sets_log():
    rs = np.random.RandomState(62)
    n = 1 << 18
    return {'log': _pair(_logu(rs, n, -120, 120)), 'near1': _pair(np.concatenate([r32(rs.uniform(0.5, 2, n)), _near([1.0], 64)]))}


DIV_SPECIALS = [(1.0, 0.0), (1.0, -0.0), (-2.5, 0.0), (-2.5, -0.0), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0)]


def _sets_div():
    rs = np.random.RandomState(63)
    n = 1 << 18
    sp = np.array(DIV_SPECIALS, f32)
    return {'log': (_logu(rs, n, -60, 60) * _signs(rs, n), _logu(rs, n, -60, 60) * _signs(rs, n)),
            'uniform': (r32(rs.uniform(-20, 20, n)), r32(rs.uniform(-3, 3, n))), 'special': (A(sp[:, 0]), A(sp[:, 1]))}


def _sets_fmod_pi():
    rs = np.random.RandomState(70)
    n = 1 << 18
    a = r32(rs.uniform(0, 8 * np.pi, n))
    a = a[a > 0]
    near = _near(r32(np.arange(1, 9) * f64(FM_PI)), 16)
    return {'uniform': _pair(a), 'near': _pair(near[near <= r32(8 * np.pi)])}


def _sets_trunca():
    rs = np.random.RandomState(80)
    k = np.arange(-1024, 1025)
    edge = [2.0 ** 31 - 128, -(2.0 ** 31 - 128), 2.0 ** 31, -2.0 ** 31, 2.0 ** 31 * (1 + 2.0 ** -23), -2.0 ** 31 * (1 + 2.0 ** -23),
            2.0 ** 32, -2.0 ** 32, np.inf, -np.inf, np.nan, 0.0, -0.0, 0.49999997, -0.49999997, 8388607.5, -8388607.5]
    return {'ties': _pair(r32(k + 0.5)), 'edge': _pair(edge), 'uniform': _pair(r32(rs.uniform(-2.0 ** 31, 2.0 ** 31, 1 << 16))),
            'small': _pair(r32(rs.uniform(-300, 300, 1 << 16)))}


_SETS = dict(rcp=_sets_rcp, sqrt=_sets_sqrt, exp2=_sets_exp2, log2=_sets_log2, hw_sin=_sets_hw_trig, hw_cos=_sets_hw_trig,
             atan2=_sets_atan2, sinh=_sets_hyp, cosh=_sets_hyp, fmod=_sets_fmod, sin=_sets_trig, cos=_sets_trig, tan=_sets_trig,
             pow=_sets_pow, exp=_sets_exp, log=_sets_log, div=_sets_div, fmod_pi=_sets_fmod_pi, trunca=_sets_trunca)
_HYP_NAMES = tuple('band %g-%g' % b for b in HYP_BANDS) + ('switch', 'special')
_TRIG_NAMES = ('pi x>=0', 'pi x<0', 'log x>=0', 'log x<0', 'zeros x>=0', 'zeros x<0')
SET_NAMES = dict(rcp=('log', 'edge'), sqrt=('log', 'edge'), exp2=('log', 'edge'), log2=('log', 'near1', 'edge'),
                 hw_sin=('log', 'unit', 'wide', 'edge'), hw_cos=('log', 'unit', 'wide', 'edge'),
                 atan2=('uniform', 'log', 'octant', 'special', 'uncovered'), sinh=_HYP_NAMES, cosh=_HYP_NAMES,
                 fmod=('uniform', 'log', 'multiples', 'straddle', 'special', 'uncovered'),
                 sin=_TRIG_NAMES + ('far', 'special'), cos=_TRIG_NAMES + ('far', 'special'), tan=_TRIG_NAMES, pow=('main', 'lines'), exp=('uniform', 'log'), log=('log', 'near1'),
                 div=('log', 'uniform', 'special'), fmod_pi=('uniform', 'near'), trunca=('ties', 'edge', 'uniform', 'small'))
# the number of elements of each set that lie in a range the source declares uncovered (zero for every set not named here)
UNCOVERED = {('atan2', 'uncovered'): 768, ('fmod', 'uncovered'): 258}


# ---- measuring a bare instruction ------------------------------------------------------------------------------------------------
def bare_errors(fn, name, a, dev):
    """Error of a device result `dev` (float32) of bare instruction fn on set `name` against float64:
    -> dict(ulp = max error in ulp of the truth over normal results, abs = max absolute error, n = compared)."""
    t = truth(fn, a)
    d = A(dev).astype(f64)
    with np.errstate(all='ignore'):
        normal = np.isfinite(t) & (np.abs(t) >= f64(FLT_MIN)) & (np.abs(t) <= 3.4e38) & (np.abs(A(a)) >= FLT_MIN) & np.isfinite(d)
        err = np.abs(d - t)
    if not normal.any():
        return dict(ulp=0.0, abs=0.0, n=0)
    e, u = err[normal], err[normal] / ulp_of(t[normal])
    i = int(np.argmax(u))
    return dict(ulp=float(u.max()), abs=float(e.max()), n=int(normal.sum()), at=float(A(a)[normal][i]))


# ---- judging a result (the restatement's on the CPU, the device's on the GPU) by the bars above ---------------------------------------
def same_bits(x, y):
    """bit for bit, any NaN counting as NaN"""
    x, y = A(x), A(y)
    return (bits(x) == bits(y)) | (np.isnan(x) & np.isnan(y))


def model_constant(fn, a, b):
    """(result of the restatement with exact instructions, mask of the elements where no combination of instruction errors changes a bit)"""
    r0 = MODEL[fn](a, b, (0,) * NINSTR[fn])[0]
    same = np.ones(r0.shape, bool)
    for ks in KS[fn]:
        same &= same_bits(MODEL[fn](a, b, ks)[0], r0)
    return r0, same


def _show(bad, a, b, res, t, n=4):
    i = np.nonzero(bad)[0][:n]
    return 'n=%d inputs a=%r b=%r got=%r want=%r' % (int(bad.sum()), A(a)[i].tolist(), A(b)[i].tolist(), A(res)[i].tolist(),
                                                      np.asarray(t)[i].tolist())


def envelope_width(fn, a, b, lo, hi):
    """What the envelope of the restatements is widened by: 2 ulp of the result; for the angle functions 2 ulp of pi, or the bare
    instruction's absolute bar where that is larger (v_sin_f32 / v_cos_f32 are not 1-ulp instructions next to their zeros); ftan
    carries that of its sine and cosine through the quotient.  Every other helper, flog and fpow included: 2 ulp of the result."""
    a64, b64 = A(a).astype(f64), A(b).astype(f64)
    with np.errstate(all='ignore'):
        w = 2.0 * ulp_of(np.maximum(np.abs(lo), np.abs(hi)))
        if fn in ('sin', 'cos', 'tan'):
            wt = max(2.0 * ulp_of(np.pi), bare_bar('hw_sin')[1], bare_bar('hw_cos')[1])
            if fn == 'tan':
                s, c = np.abs(np.sin(a64)), np.abs(np.cos(a64))
                wt = wt * (s + c) / (c * (c - wt)) + w
            w = np.maximum(w, wt) if fn != 'tan' else wt
    return w


def judge(fn, name, a, b, res_bits, with_envelope=False):
    """-> (failures: list of str, envelope failures: list of str, figures: dict) for the raw result bits of helper fn on set `name`"""
    a, b = A(a), A(b)
    fails, env_fails, fig = [], [], {}
    if fn == 'trunca':
        want = m_trunca(a)[0]
        bad = np.asarray(res_bits, np.uint32) != want
        if bad.any():
            fails.append('trunca not bit-exact: ' + _show(bad, a, b, np.asarray(res_bits, np.uint32).view(np.int32), want.view(np.int32)))
        return fails, env_fails, fig
    res = from_bits(res_bits)
    r64 = res.astype(f64)
    t = truth(fn, a, b)
    r0, covered = MODEL[fn](a, b, (0,) * NINSTR[fn])
    fig['uncovered'] = int((~covered).sum())
    with np.errstate(all='ignore'):
        err = np.abs(r64 - t)
        fin = covered & np.isfinite(t) & np.isfinite(r0.astype(f64))
        normal_t = fin & (np.abs(t) >= f64(FLT_MIN)) & (np.abs(t) <= 3.0e38)

        def bar_check(what, mask, bar):
            m = mask & ~(err <= bar)                     # (a NaN result fails)
            if mask.any():
                fig[what] = float(np.nanmax(np.where(mask & (bar > 0), err / np.where(bar > 0, bar, 1), 0)))
            if m.any():
                fails.append('%s/%s %s: ' % (fn, name, what) + _show(m, a, b, res, t))

        if name in ('special', 'lines', 'edge'):
            want, const = model_constant(fn, a, b)
            if fn in BARE:
                const &= ~np.isfinite(want) | ((want == 0) & (fn not in ('hw_sin', 'hw_cos')))
            m = covered & const & ~same_bits(res, want)
            fig['bit_exact'] = int((covered & const).sum())
            if m.any():
                fails.append('%s/%s differs from the restatement bit for bit: ' % (fn, name) + _show(m, a, b, res, want))

        if fn in BARE:
            bu, ba = bare_bar(fn)
            ok_in = np.abs(a) >= FLT_MIN
            bar_check('ulp', normal_t & ok_in & (np.abs(a) <= 256 if fn in ('hw_sin', 'hw_cos') else True), bu * ulp_of(t))
            if fn in ('hw_sin', 'hw_cos'):
                bar_check('absolute', fin & (np.abs(a) <= 256), ba)
            elif fn == 'log2':
                bar_check('absolute', fin & (a >= 0.5) & (a <= 2), ba)
        elif fn == 'atan2':
            fin &= ~((a == 0) & (b == 0))        # atan2(+-0, +-0) is +-0 by the source's own statement: held to the restatement, bit for bit
            bar_check('absolute', fin, ATAN2_BAR)
            bar_check('first octant, relative', fin & (b > 0) & (np.abs(a) <= np.abs(b)) & (np.abs(t) >= 2.0 ** -100), ATAN2_BAR * np.abs(t))
        elif fn in ('sinh', 'cosh'):
            ax = np.abs(a).astype(f64)
            bar_check('relative', fin & (ax <= 88) & (a != 0), hyp_bar(a) * np.abs(t))
            if fn == 'sinh':
                bar_check('series, relative', fin & (ax < 0.5) & (a != 0), SINH_SERIES_BAR * np.abs(t))
                m = (a == 0) & (bits(res) != bits(a))
                if m.any():
                    fails.append('sinh(+-0) loses its sign: ' + _show(m, a, b, res, a))
            else:
                m = ~np.isnan(a) & ~(res >= 1)
                if m.any():
                    fails.append('cosh below 1: ' + _show(m, a, b, res, t))
            early = (ax <= 88.7) & ~np.isfinite(res)
            late = (ax >= 89.5) & ~np.isnan(a) & ~np.isinf(res)
            if early.any() or late.any():
                fails.append('%s overflows at the wrong place: ' % fn + _show(early | late, a, b, res, t))
        elif fn == 'fmod':
            lean_any = np.zeros(a.shape, bool)
            for ks in KS[fn]:
                lean_any |= fmod_lean_mask(a, b, ks)
            lib = libm_fmod(a, b)
            m = covered & ~lean_any & ~same_bits(res, lib)
            fig['library path'] = int((covered & ~lean_any).sum())
            if m.any():
                fails.append('fmod/%s library path differs from fmodf: ' % name + _show(m, a, b, res, lib))
            lean = covered & lean_any & np.isfinite(t)
            fig['lean path'] = int(lean.sum())
            fig['inexact share'] = float((lean & (err > 0)).sum() / max(1, lean.sum()))
            bar_check('lean', lean, 2.0 ** -23 * np.abs(b).astype(f64))
            m = lean & ((np.signbit(res) != np.signbit(a)) | ~(np.abs(res) < np.abs(b)))
            if m.any():
                fails.append('fmod/%s sign or magnitude: ' % name + _show(m, a, b, res, t))
        elif fn in ('sin', 'cos'):
            ax = np.abs(a).astype(f64)
            bar_check('absolute', np.isfinite(a) & (ax <= 2.0 ** 20), sin_arg_bar(a))
            m = np.isfinite(a) & ~(np.abs(res) <= 1)
            if m.any():
                fails.append('%s/%s not a finite value in [-1, 1]: ' % (fn, name) + _show(m, a, b, res, t))
            m = ~np.isfinite(a) & ~np.isnan(res)
            if m.any():
                fails.append('%s/%s of inf / NaN is not NaN: ' % (fn, name) + _show(m, a, b, res, t))
        elif fn == 'tan':
            bar, use = tan_bar(a)
            fig['compared'] = int(use.sum())
            bar_check('absolute', use & np.isfinite(a), bar)
        elif fn == 'div':
            rc = 1.0 / b.astype(f64)
            bar_check('relative', normal_t & (np.abs(rc) >= f64(FLT_MIN)) & (np.abs(rc) <= 3e38), div_bar(t))
        elif fn == 'exp':
            bar_check('relative', normal_t & (np.abs(a) <= 87), exp_bar(a))
        elif fn == 'log':
            bar_check('absolute', fin & (a >= FLT_MIN), log_bar(a))
        elif fn == 'pow':
            e = b.astype(f64) * np.log2(a.astype(f64))
            bar_check('relative', normal_t & (a >= FLT_MIN) & (np.abs(e) <= 125), pow_bar(a, b))
        elif fn == 'fmod_pi':
            ua = ulp_of(a)
            pi_f = f64(FM_PI)
            plain = err <= 4 * ua
            caveat = ~plain & (np.abs(np.abs(r64 - t) - pi_f) <= 4 * ua) & ((t <= 8 * ua) | (pi_f - t <= 8 * ua))
            fig['pi clause share'] = float(caveat.mean())
            m = ~(plain | caveat)
            if m.any():
                fails.append('fmod_pi/%s: ' % name + _show(m, a, b, res, t))
            if caveat.mean() > 0.01:
                fails.append('fmod_pi/%s: %.3f %% of the set needs the +-pi clause' % (name, 100 * caveat.mean()))
        else:
            raise KeyError(fn)

        if with_envelope and fn not in BARE:
            lo, hi = envelope(fn, a, b)
            w = envelope_width(fn, a, b, lo, hi)
            sel = covered.copy()
            if fn == 'tan':
                sel &= tan_bar(a)[1]
            if fn in ('sin', 'cos', 'tan'):
                sel &= np.abs(a) <= 2.0 ** 20
            nan_m = np.isnan(lo)
            inf_m = ~nan_m & (np.isinf(lo) | np.isinf(hi))
            m = sel & ~nan_m & ~inf_m & ~((r64 >= lo - w) & (r64 <= hi + w))
            m |= sel & nan_m & ~np.isnan(r64)
            m |= sel & inf_m & (lo == hi) & ~(r64 == lo)
            fig['envelope'] = int(sel.sum())
            if m.any():
                env_fails.append('%s/%s outside the envelope of the restatements: ' % (fn, name) + _show(m, a, b, res, (lo + hi) / 2))
    return fails, env_fails, fig
