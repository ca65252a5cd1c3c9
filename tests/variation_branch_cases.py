"""
Fixed cases that reach the branches of the variations (csrc/variations.h) which parameters, the sign of the weight or the range of
the point select — promoted from what tools/soak_variations.py draws at random.  One xform holding one variation, identity axes and
an offset (ox, oy) as its pre affine, no post affine; 1024 points uniform in [-span, span]^2 (span 0.3, 1.5 or 5.0).

A case names its branches as predicates over what the variation sees: tx, ty (the point through the pre affine, float32 as the
device computes it), the weight w, the variation's record v (parameters in sorted-name order, then precalculated values) and the
xform record xf.  tests/test_cpu_variation_branches.py asserts on the CPU that every branch is reached by at least 32 of the 1024 points,
that the oracle's result is finite for at least 90 % of them, and that at most 1.5 % of them have an oracle neighbourhood (7 x 7
inputs within 6 ulp) that spreads further than the tolerance of tests/test_gpu_variations.py — the cap of that test's
neighbourhood clause, as a condition on the case instead of a measurement of the device.
"""
import numpy as np

from cuburn_amd import configs
from cuburn_amd.genome import variations as V

NPTS = 1024
PI = np.float32(3.14159274101257)
f32 = np.float32


def _r2(tx, ty):
    return tx.astype(np.float64) ** 2 + ty.astype(np.float64) ** 2


def _quadrants():
    return {'x>0 y>0': lambda c: (c.tx > 0) & (c.ty > 0), 'x<0 y>0': lambda c: (c.tx < 0) & (c.ty > 0),
            'x>0 y<0': lambda c: (c.tx > 0) & (c.ty < 0), 'x<0 y<0': lambda c: (c.tx < 0) & (c.ty < 0)}


def _always(cond):
    return lambda c: np.full(c.tx.shape, bool(cond(c)))


def _atan2(a, b):
    return np.arctan2(a.astype(np.float64), b.astype(np.float64))


def _fan_t(c, dx, dy):
    """the compared remainder of fan / fan2 and the quotient in front of it"""
    s = _atan2(c.tx, c.ty) + dy
    return np.fmod(s, dx), np.abs(s / dx)


def _series(axis, scale=1.0):
    """the argument of v_sinh / v_cosh on and off the series (|arg| < 0.5)"""
    return {'series': lambda c: np.abs(scale * getattr(c, axis)) < 0.5, 'exponential form': lambda c: np.abs(scale * getattr(c, axis)) >= 0.5,
            'argument beyond 2': lambda c: np.abs(scale * getattr(c, axis)) > 2}


def case(cid, var, params, weight, span, branches, offset=(0.0, 0.0)):
    assert span in (0.3, 1.5, 5.0) and var in V.var_ids
    p = dict((k, dv if dv else 0.6) for k, (dv, _) in V.var_params[var].items())
    p.update(params)
    p['weight'] = weight
    return dict(id=cid, var=var, params=p, weight=weight, span=span, offset=offset, branches=branches)


def _oscope_t(c):
    # v: amplitude damping frequency separation
    tx = c.tx.astype(np.float64)
    return c.v[0] * np.exp(-np.abs(tx) * c.v[1]) * np.cos(2 * np.pi * c.v[2] * tx) + c.v[3]


def _ngon_phi(c):
    # v: circle corners power sides
    b = 2 * np.pi / c.v[3]
    th = _atan2(c.ty, c.tx)
    return th - b * np.floor(th / b), b


def _bipolar_y(c):
    return 0.5 * _atan2(f32(2) * c.ty, (_r2(c.tx, c.ty) - 1).astype(f32)) - 0.5 * np.pi * c.v[0]


def _lazysusan_r(c):
    # v: space spin twist x y
    return np.hypot(c.tx.astype(np.float64) - c.v[3], c.ty.astype(np.float64) + c.v[4])


def _boarders(c):
    rx, ry = np.rint(c.tx), np.rint(c.ty)
    return np.abs(c.tx - rx), np.abs(c.ty - ry)


_HYP = [('sin', 'ty', 1), ('cos', 'ty', 1), ('tan', 'ty', 2), ('sec', 'ty', 1), ('csc', 'ty', 1), ('cot', 'ty', 2),
        ('sinh', 'tx', 1), ('cosh', 'tx', 1), ('tanh', 'tx', 2), ('sech', 'tx', 1), ('csch', 'tx', 1), ('coth', 'tx', 2),
        ('cosine', 'ty', 1)]

CASES = [
    case('disc2 twist 7', 'disc2', dict(rot=0.6, twist=7.0), 0.8, 1.5, {'twist > 2 pi': _always(lambda c: c.v[1] > 2 * PI)}),
    case('disc2 twist -7', 'disc2', dict(rot=0.6, twist=-7.0), 0.8, 1.5, {'twist < -2 pi': _always(lambda c: c.v[1] < -2 * PI)}),
    case('disc2 twist 1', 'disc2', dict(rot=0.6, twist=1.0), 0.8, 1.5, {'no scale': _always(lambda c: abs(c.v[1]) <= 2 * PI)}),
    case('rectangles x 0', 'rectangles', dict(x=0.0, y=0.6), 0.8, 1.5, {'rx == 0, ry != 0': _always(lambda c: c.v[0] == 0 and c.v[1] != 0)}),
    case('rectangles y 0', 'rectangles', dict(x=0.6, y=0.0), 0.8, 1.5, {'ry == 0, rx != 0': _always(lambda c: c.v[1] == 0 and c.v[0] != 0)}),
    case('loonie w 0.8', 'loonie', {}, 0.8, 1.5, {'r2 < w2': lambda c: _r2(c.tx, c.ty) < c.w * c.w, 'r2 >= w2': lambda c: _r2(c.tx, c.ty) >= c.w * c.w}),
    case('loonie w -0.8', 'loonie', {}, -0.8, 1.5, {'r2 < w2': lambda c: _r2(c.tx, c.ty) < c.w * c.w, 'r2 >= w2': lambda c: _r2(c.tx, c.ty) >= c.w * c.w,
                                                   'negative weight': _always(lambda c: c.w < 0)}),
    case('lazysusan', 'lazysusan', dict(x=0.2, y=-0.1, twist=0.7, space=0.3, spin=0.5), 0.8, 1.5,
         {'inside': lambda c: _lazysusan_r(c) < c.w, 'outside': lambda c: _lazysusan_r(c) >= c.w}),
    case('whorl', 'whorl', dict(inside=0.6, outside=-0.4), 0.8, 1.5,
         {'inside': lambda c: np.sqrt(_r2(c.tx, c.ty)) < c.w, 'outside': lambda c: np.sqrt(_r2(c.tx, c.ty)) >= c.w}),
    case('bipolar shift 1.7', 'bipolar', dict(shift=1.7), 0.8, 1.5,
         {'wraps from below': lambda c: _bipolar_y(c) < -np.pi / 2, 'no wrap': lambda c: np.abs(_bipolar_y(c)) <= np.pi / 2}),
    case('bipolar shift -1.7', 'bipolar', dict(shift=-1.7), 0.8, 1.5,
         {'wraps from above': lambda c: _bipolar_y(c) > np.pi / 2, 'no wrap': lambda c: np.abs(_bipolar_y(c)) <= np.pi / 2}),
    case('modulus', 'modulus', dict(x=0.6, y=0.4), 0.8, 1.5,
         {'x above': lambda c: c.tx > c.v[0], 'x below': lambda c: c.tx < -c.v[0], 'x within': lambda c: np.abs(c.tx) <= c.v[0],
          'y above': lambda c: c.ty > c.v[1], 'y below': lambda c: c.ty < -c.v[1], 'y within': lambda c: np.abs(c.ty) <= c.v[1]}),
    case('modulus far', 'modulus', dict(x=0.6, y=0.4), -0.8, 5.0,
         {'x quotient beyond 2': lambda c: np.abs(c.tx) + c.v[0] > 4 * c.v[0], 'y quotient beyond 2': lambda c: np.abs(c.ty) + c.v[1] > 4 * c.v[1]}),
    case('oscope', 'oscope', dict(separation=1.0, frequency=1.1, amplitude=0.8, damping=0.3), 0.8, 1.5,
         {'|y| <= t': lambda c: np.abs(c.ty) <= _oscope_t(c), '|y| > t': lambda c: np.abs(c.ty) > _oscope_t(c)}),
    case('fan', 'fan', {}, 0.8, 1.5, {'t > dx2': lambda c: _fan_t(c, np.pi * c.xf[2] ** 2, c.xf[5])[0] > 0.5 * np.pi * c.xf[2] ** 2,
                                      't <= dx2': lambda c: _fan_t(c, np.pi * c.xf[2] ** 2, c.xf[5])[0] <= 0.5 * np.pi * c.xf[2] ** 2,
                                      'quotient beyond 1': lambda c: _fan_t(c, np.pi * c.xf[2] ** 2, c.xf[5])[1] > 1}, offset=(0.6, 0.3)),
    case('fan2', 'fan2', dict(x=0.6, y=0.3), 0.8, 1.5,
         {'t > dx2': lambda c: _fan_t(c, np.pi * c.v[0] ** 2, c.v[1])[0] > 0.5 * np.pi * c.v[0] ** 2,
          't <= dx2': lambda c: _fan_t(c, np.pi * c.v[0] ** 2, c.v[1])[0] <= 0.5 * np.pi * c.v[0] ** 2,
          'quotient beyond 1': lambda c: _fan_t(c, np.pi * c.v[0] ** 2, c.v[1])[1] > 1}),
    case('rings', 'rings', {}, 0.8, 1.5, {'quotient beyond 1': lambda c: np.sqrt(_r2(c.tx, c.ty)) + c.xf[2] ** 2 > 2 * c.xf[2] ** 2,
                                          'quotient below 1': lambda c: np.sqrt(_r2(c.tx, c.ty)) + c.xf[2] ** 2 < 2 * c.xf[2] ** 2,
                                          'quotient beyond 3': lambda c: np.sqrt(_r2(c.tx, c.ty)) + c.xf[2] ** 2 > 6 * c.xf[2] ** 2},
         offset=(0.6, 0.3)),
    case('rings2', 'rings2', dict(val=0.6), 0.8, 1.5,
         {'quotient beyond 1': lambda c: np.sqrt(_r2(c.tx, c.ty)) + c.v[0] ** 2 > 2 * c.v[0] ** 2,
          'quotient below 1': lambda c: np.sqrt(_r2(c.tx, c.ty)) + c.v[0] ** 2 < 2 * c.v[0] ** 2,
          'quotient beyond 3': lambda c: np.sqrt(_r2(c.tx, c.ty)) + c.v[0] ** 2 > 6 * c.v[0] ** 2}),
    case('julian power -3', 'julian', dict(power=-3.0, dist=1.0), 0.8, 1.5, {'negative power': _always(lambda c: c.v[1] < 0)}),
    case('juliascope power -3', 'juliascope', dict(power=-3.0, dist=1.0), 0.8, 1.5, {'negative power': _always(lambda c: c.v[1] < 0)}),
    case('cpow power -2', 'cpow', dict(r=1.0, i=0.2, power=-2.0), 0.8, 1.5, {'negative power': _always(lambda c: c.v[1] < 0)}),
    case('ngon', 'ngon', dict(sides=5.0, power=3.0, circle=1.0, corners=2.0), 0.8, 1.5,
         {'phi > b / 2': lambda c: _ngon_phi(c)[0] > _ngon_phi(c)[1] / 2, 'phi <= b / 2': lambda c: _ngon_phi(c)[0] <= _ngon_phi(c)[1] / 2}),
    case('perspective', 'perspective', dict(angle=0.9, dist=1.0), 0.8, 5.0,
         {'denominator > 0': lambda c: c.v[2] - c.ty.astype(np.float64) * c.v[3] > 0, 'denominator < 0': lambda c: c.v[2] - c.ty.astype(np.float64) * c.v[3] < 0}),
    case('splits', 'splits', dict(x=0.6, y=-0.4), 0.8, 1.5, _quadrants()),
    case('bent', 'bent', {}, -0.8, 1.5, _quadrants()),
    case('bent2', 'bent2', dict(x=0.6, y=-1.4), 0.8, 1.5, _quadrants()),
    case('separation', 'separation', dict(x=0.6, xinside=0.3, y=0.4, yinside=-0.2), 0.8, 1.5, _quadrants()),
    case('boarders', 'boarders', {}, 0.8, 1.5,
         {'inner': lambda c: c.u01 > 0.75, 'x arm': lambda c: (c.u01 <= 0.75) & (_boarders(c)[0] >= _boarders(c)[1]),
          'y arm': lambda c: (c.u01 <= 0.75) & (_boarders(c)[0] < _boarders(c)[1])}),
    case('cell', 'cell', dict(size=0.6), 0.8, 1.5,
         {'x cell negative': lambda c: np.floor(c.tx / c.v[0]) < 0, 'x cell positive': lambda c: np.floor(c.tx / c.v[0]) >= 0,
          'y cell negative': lambda c: np.floor(c.ty / c.v[0]) < 0, 'y cell positive': lambda c: np.floor(c.ty / c.v[0]) >= 0}),
    case('exponential span 5', 'exponential', {}, -0.8, 5.0, {'dx finite': lambda c: c.tx.astype(np.float64) - 1 < 88.5}),
    # (next to the overflow the finite results are ~1e38, beyond what the acceptance rule compares: this case holds the device to
    # the oracle where dx overflows and the variation adds nothing; the case above holds the finite values)
    case('exponential overflow', 'exponential', {}, 0.8, 1.5,
         {'dx overflows': lambda c: c.tx.astype(np.float64) - 1 > 89.2}, offset=(89.5, 0.0)),
] + [case('%s span 5' % name, name, {}, 0.8, 5.0, _series(axis, scale)) for name, axis, scale in _HYP]


def genome_for(c):
    return {'type': 'animation', 'camera': {'scale': 0.25}, 'time': {'duration': 1, 'frame_width': 0.0},
            'palette': [[0.0] + configs.palette_encode(configs.grey_ramp())],
            'xforms': {'0': {'weight': 1.0, 'color': 0.7, 'color_speed': 0.3,
                             'pre_affine': configs._affine(0.0, 1.0, c['offset'][0], c['offset'][1]),
                             'variations': {c['var']: dict(c['params'])}}}}


def inputs(c, index):
    """-> (points float32 [NPTS, 4] = x, y, colour, 0; RNG states uint32 [NPTS, 3])"""
    from cuburn_amd import mwc
    rs = np.random.RandomState(7000 + index)
    pts = np.zeros((NPTS, 4), np.float32)
    pts[:, 0] = rs.uniform(-c['span'], c['span'], NPTS)
    pts[:, 1] = rs.uniform(-c['span'], c['span'], NPTS)
    pts[:, 2] = rs.uniform(0, 1, NPTS)
    return pts, mwc.make_seeds(NPTS, 99)


class Seen:
    """what the variation sees of a case's points, given the xform's record of the parameter block"""
    def __init__(self, c, pts, rng, xf):
        xf = np.asarray(xf, np.float32)
        x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
        # fmaf(xx, x, fmaf(xy, y, xo)), each fma rounded once
        self.tx = (xf[0] * x + (xf[1] * y + xf[2]).astype(np.float32)).astype(np.float32)
        self.ty = (xf[3] * x + (xf[4] * y + xf[5]).astype(np.float32)).astype(np.float32)
        self.xf = xf.astype(np.float64)
        self.w = float(xf[17])
        self.v = xf[18:].astype(np.float64)
        # the first uniform draw of each point's stream (mwc_next_01)
        rng = np.asarray(rng, np.uint64).reshape(-1, 3)
        state = (rng[:, 0] * rng[:, 1] + rng[:, 2]) & np.uint64(0xffffffff)
        self.u01 = state.astype(np.float32) * np.float32(1.0 / 4294967296.0)


# ---- the oracle's view of a case (CPU only) ------------------------------------------------------------------------------------------
TOL_ABS, TOL_REL = 2e-4, 2e-3          # the plain tolerance of tests/test_gpu_variations.py
PROFILE = {'width': 64, 'height': 64, 'spp': 1, 'fps': 1, 'duration': 1, 'frame_width': 0}


def _step(v, n):
    v = np.array(v, np.float32)
    for _ in range(abs(n)):
        v = np.nextafter(v, np.float32(np.inf if n > 0 else -np.inf))
    return v


def oracle_view(c, index):
    """-> dict(seen = Seen, ref = the oracle's points [NPTS, 2] float64, spread_share = share of the points whose oracle results over the
    7 x 7 inputs within 6 ulp spread further than the plain tolerance or leave the finite range)"""
    import ctypes as C
    from common import O, prepare
    gnm = genome_for(c)
    F = prepare(gnm, PROFILE)
    prog, P = F['packer'].prog, np.ascontiguousarray(F['params'][5], np.float32)
    pts, rng = inputs(c, index)
    L = O.lib()
    L.ref_apply_xf_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p]

    def run(p, r):
        p, r = np.ascontiguousarray(p, np.float32).copy(), np.ascontiguousarray(r, np.uint32).copy()
        assert L.ref_apply_xf_n(prog.ctypes.data, P.ctypes.data, 0, len(p), p.ctypes.data, r.ctypes.data) == 0
        return p[:, :2].astype(np.float64)

    ref = run(pts, rng)
    steps = range(-6, 7, 2)
    nb = np.repeat(pts[:, None, :], 49, 1)                               # [NPTS, 49, 4]
    for j, (du, dv) in enumerate((du, dv) for du in steps for dv in steps):
        nb[:, j, 0], nb[:, j, 1] = _step(pts[:, 0], du), _step(pts[:, 1], dv)
    outs = run(nb.reshape(-1, 4), np.repeat(rng[:, None, :], 49, 1).reshape(-1, 3)).reshape(NPTS, 49, 2)
    with np.errstate(all='ignore'):
        # (a point whose own oracle result is beyond 1e6 or not finite is settled by that test without the neighbourhood)
        plain = np.isfinite(ref).all(1) & (np.abs(ref).max(1) < 1e6)
        wild = ~np.isfinite(outs).all((1, 2)) | (np.abs(outs).max((1, 2)) >= 1e6)
        spread = outs.max(1) - outs.min(1)
        loose = (spread > TOL_ABS + TOL_REL * np.abs(ref)).any(1)
    xf = P[prog[5]:prog[5] + prog[6]]
    return dict(seen=Seen(c, pts, rng, xf), ref=ref, plain_share=float(plain.mean()), spread_share=float((plain & (wild | loose)).mean()))
