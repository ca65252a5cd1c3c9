"""
Float64 model of the two kernels at the head of every frame (cuburn_amd/csrc/interp.hip): the Catmull-Rom splines of
cuburn/code/interp.py:299-355 in the linear and the lin-log "magnitude" domain, the eleven op kinds of include/flame_hip.h (6)
composed from them (cuburn/code/iter.py:12-30,56-95; cuburn/code/variations.py:136-140,267-273,292-294,630-634), and the palette
blend, dither and packing of cuburn/code/interp.py:372-433.  Vectorised over the temporal samples.

What is float32 on purpose: the table values, and the SAMPLE TIME.  The kernel computes tstep = f32(td / f32(nts)) and
time = f32(ts + f32(f32(id) * tstep)); kernel and oracle are built without contraction, so those three roundings are the
operation, and the model takes them as they are.  Everything after them is float64.

The table is the FLAT one the kernel indexes, nrows x 32 words, followed by one padding row (times 1e9, knots 0): a row with 32
knots evaluated after its 31st takes its fourth support point from the next row, and the last row from the padding
(include/flame_hip.h (4)).

Every quantity travels with its SCALE: a bound, in units of 2^-24, on what one float32 rounding per operation can do to it.
  * spline: the sum of the absolute monomial contributions
        |m1|(|u|^3 + 2u^2 + |u|) + |k1|(2|u|^3 + 3u^2 + 1) + |m2|(|u|^3 + u^2) + |k2|(2|u|^3 + 3u^2)
    (not the four Hermite terms: u^3 - 2u^2 + u cancels near u = 1, and each monomial is rounded before that);
  * exact words (FL_OP_CONST, the last CDF word): 0;
  * a product carries the product of its factors' scales, a sum their sum, a quotient x / y carries sx sy / y^2: the sum of the
    absolute products of the formula, each spline entering with its scale;
  * sin / cos of an angle a carry |trig a| + sa |trig' a|: the value's own rounding and the |a| 2^-24 a float32 angle brings in
    (|trig'| <= 1 gives the (1 + |a|) of a plain bound; with the derivative the scale stays honest where the function is 0).
A magnitude spline is measured where it is computed, in the magnitude domain: |linlog(x) - r| / scale.
"""
import numpy as np

F32 = np.float32
KNOTS = 32
PAD_TIME = F32(1e9)
ELBOW = 0.0625
ELOG1 = 5.0
PI = float(F32(3.14159274101257))           # the kernels' float32 constants, cuburn/code/util.py:148-160
PI_2 = float(F32(1.57079637050629))
E20 = float(F32(1.0e-20))
E9 = float(F32(1e-9))
OPACITY_POW = float(F32(3.3219281))
ONE_M = float(F32(1.0) - F32(1.0e-6))
Q_MIN = float(F32(2.3283064e-10))           # 2^-32
TINY = 2.0 ** -126                          # smallest normal float32

(OP_SPLINE, OP_SPLINE_MAG, OP_CAMERA, OP_AFFINE, OP_CDF, OP_RATIO2, OP_INVSQ, OP_PERSP, OP_INVSQ_MAX, OP_CONST,
 OP_OPACITY) = range(11)
OP_NAMES = ['spline', 'spline_mag', 'camera', 'affine', 'cdf', 'ratio2', 'invsq', 'persp', 'invsq_max', 'const', 'opacity']
NDST = {OP_SPLINE: 1, OP_SPLINE_MAG: 1, OP_CAMERA: 6, OP_AFFINE: 6, OP_RATIO2: 1, OP_INVSQ: 1, OP_PERSP: 3, OP_INVSQ_MAX: 1,
        OP_CONST: 1, OP_OPACITY: 1}

# segment kinds, in the order of precedence in which a sample is filed
SEG = ['on-knot', 'extrapolated', 'padding', 'by-step', 'interior', 'next-row']      # next-row: the fourth support point lies beyond a 32-knot row
BRANCH = ['lin', 'log+', 'log-']
OPACITY_CLS = ['zero', 'one', 'flushed', 'power']


def sample_times(ts, td, n):
    """The float32 times of the n samples of a frame window (interp.hip, k_interp_params; n = 64 for the palette rows)."""
    tstep = F32(F32(td) / F32(n))
    return (F32(ts) + np.arange(n, dtype=F32) * tstep).astype(F32)


def flat_table(times, knots):
    """(nrows, 32) float32 rows -> the flat table with its trailing padding row."""
    times, knots = np.asarray(times, F32), np.asarray(knots, F32)
    assert times.shape == knots.shape and times.shape[1] == KNOTS
    return (np.concatenate([times.reshape(-1), np.full(KNOTS, PAD_TIME, F32)]),
            np.concatenate([knots.reshape(-1), np.zeros(KNOTS, F32)]))


def binsearch32(hay, base, t):
    """cuburn/code/util.py:219-230: five strict compares; the rightmost of hay[base ..] strictly below t (0 if none of 1 .. 31)."""
    lo = np.zeros(len(t), np.int64)
    for step in (16, 8, 4, 2, 1):
        lo += step * (t > hay[base + lo + step])
    return lo


def linlog(x):
    x = np.asarray(x, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(x > ELBOW, np.log2(np.abs(x)) + ELOG1, np.where(x < -ELBOW, -(np.log2(np.abs(x)) + ELOG1), x / ELBOW))


def linlog_branch(x):
    return np.where(x > ELBOW, 1, np.where(x < -ELBOW, 2, 0))


def linexp(v):
    return np.where(v >= 1.0, np.exp2(np.minimum(v, 200.0) - ELOG1), np.where(v <= -1.0, -np.exp2(np.minimum(-v, 200.0) - ELOG1), v * ELBOW))


def linexp_branch(v):
    return np.where(v >= 1.0, 1, np.where(v <= -1.0, 2, 0))


def linslope(x, m):
    return np.where(x >= ELBOW, m / np.where(x == 0, 1, x), np.where(x <= -ELBOW, m / np.where(x == 0, 1, -x), m / ELBOW))


class Spline(object):
    """What the model says about one row at n sample times.
         value   what the op writes (after linexp for a magnitude row)
         r       the spline in the domain it is evaluated in (== value for a linear row)
         scale   the monomial scale of r
         vscale  the scale of `value` as a factor of a further formula (scale for a linear row; for a magnitude row
                 |value| (1 + ln 2 scale) in the exponential branches, scale / 16 in the linear one)
         seg     index into SEG;  k1b, k2b, rb: indices into BRANCH (magnitude rows; else 0)
         on_knot samples whose time equals a knot time exactly
         inter   every intermediate a float32 evaluation holds, for the denormal check"""
    pass


def spline(T, K, row, t, mag):
    T64, K64 = T.astype(np.float64), K.astype(np.float64)
    t = np.asarray(t, F32)
    base = row * KNOTS
    idx = np.maximum(binsearch32(T, base, t), 1)
    b = base + idx
    t64 = t.astype(np.float64)
    t1 = T64[b]
    t2 = T64[b + 1] - t1
    assert (t2 > 0).all(), 'row %d: a sample selects a segment of length 0' % row
    rt2 = 1.0 / t2
    t0, t3 = (T64[b - 1] - t1) * rt2, (T64[b + 2] - t1) * rt2
    u = (t64 - t1) * rt2
    k0, k1, k2, k3 = K64[b - 1], K64[b], K64[b + 1], K64[b + 2]
    m1, m2 = (k2 - k0) / (1.0 - t0), (k3 - k1) / t3
    S = Spline()
    S.k1b = S.k2b = S.rb = np.zeros(len(t), np.int64)
    if mag:
        S.k1b, S.k2b = linlog_branch(k1), linlog_branch(k2)
        m1, m2 = linslope(k1, m1), linslope(k2, m2)
        k1, k2 = linlog(k1), linlog(k2)
    uu, uuu = u * u, u * u * u
    r = m1 * (uuu - 2.0 * uu + u) + k1 * (2.0 * uuu - 3.0 * uu + 1.0) + m2 * (uuu - uu) + k2 * (-2.0 * uuu + 3.0 * uu)
    a1, a2, a3 = np.abs(u), uu, np.abs(uuu)
    S.scale = np.abs(m1) * (a3 + 2 * a2 + a1) + np.abs(k1) * (2 * a3 + 3 * a2 + 1) + np.abs(m2) * (a3 + a2) + np.abs(k2) * (2 * a3 + 3 * a2)
    S.r = r
    if mag:
        S.rb = linexp_branch(r)
        S.value = linexp(r)
        S.vscale = np.where(S.rb == 0, S.scale * ELBOW, np.abs(S.value) * (1.0 + np.log(2.0) * S.scale))
    else:
        S.value, S.vscale = r, S.scale
    S.on_knot = (t64 == t1) | (t64 == T64[b + 1])
    by_step = (T64[b - 1] == t1) | (T64[b + 2] == T64[b + 1])
    S.seg = np.where(S.on_knot, 0, np.where(idx + 2 >= KNOTS, 5, np.where(u < 0, 1, np.where(T64[b + 2] >= 1e8, 2, np.where(by_step, 3, 4)))))
    S.u, S.idx = u, idx
    S.inter = [t0, t3, u, uu, uuu, m1, m2, k1, k2, r, S.value]
    return S


def mag_deviation(x, S):
    """|linlog(x) - r| for a magnitude row's outputs x."""
    return np.abs(linlog(np.asarray(x, np.float64)) - S.r)


# ------------------------------------------------------------------ values with scales
class V(object):
    """A float64 array with the scale of its float32 evaluation."""

    def __init__(self, v, s):
        self.v, self.s = np.asarray(v, np.float64), np.asarray(s, np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(np.float64(x), np.abs(np.float64(x)))

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.s * o.s)
    __rmul__ = __mul__

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.s + o.s)
    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.s + o.s)

    def __neg__(self):
        return V(-self.v, self.s)

    def __truediv__(self, o):
        o = V.of(o)
        return V(self.v / o.v, self.s * o.s / (o.v * o.v))

    def __rtruediv__(self, o):
        return V.of(o) / self

    def sin(self):
        return V(np.sin(self.v), np.abs(np.sin(self.v)) + self.s * np.abs(np.cos(self.v)))

    def cos(self):
        return V(np.cos(self.v), np.abs(np.cos(self.v)) + self.s * np.abs(np.sin(self.v)))

    def maximum(self, c):
        return V(np.maximum(self.v, c), np.where(self.v > c, self.s, abs(c)))


def _row(T, K, row, t, mag):
    S = spline(T, K, row, t, mag)
    return V(S.value, S.vscale), S


def op_values(T, K, op, t, dim):
    """(values (n, ndst) float64, scales (n, ndst), classes (n,) or None, the splines it read) of one op at float32 times t.
    dim = (w, aw, ah).  Classes: SEG index for the two spline ops (more through the Spline), OPACITY_CLS index for the opacity."""
    kind, _, a, b = [int(x) for x in op]
    n = len(t)
    one = np.ones(n)
    R = lambda r, mag: _row(T, K, r, t, mag)
    cls, used = None, []
    if kind in (OP_SPLINE, OP_SPLINE_MAG):
        S = spline(T, K, a, t, kind == OP_SPLINE_MAG)
        return S.value[:, None], S.scale[:, None], S.seg, [S]
    if kind == OP_CONST:
        w = np.array([a], np.int32).view(F32).astype(np.float64)[0]
        return np.full((n, 1), w), np.zeros((n, 1)), None, []
    if kind == OP_CAMERA:                                              # cuburn/code/iter.py:56-79
        (rot, s0), (cx, s1), (cy, s2), (sc, s3) = R(a, False), R(a + 1, False), R(a + 2, False), R(a + 3, True)
        used = [s0, s1, s2, s3]
        rot = rot * PI / 180.0
        rs, rc = rot.sin(), rot.cos()
        scale = sc * float(dim[0])
        out = [scale * rc, scale * -rs, scale * (rs * cy - rc * cx) + 0.5 * float(dim[1]),
               scale * rs, scale * rc, scale * -(rs * cx + rc * cy) + 0.5 * float(dim[2])]
    elif kind == OP_AFFINE:                                            # cuburn/code/iter.py:81-95
        rows = [R(a, False), R(a + 1, False), R(a + 2, True), R(a + 3, True), R(a + 4, False), R(a + 5, False)]
        used = [x[1] for x in rows]
        pri, spr = rows[0][0] * PI / 180.0, rows[1][0] * PI / 180.0
        mx, my = rows[2][0], rows[3][0]
        out = [mx * (pri - spr).cos(), -my * (pri + spr).cos(), rows[4][0], -mx * (pri - spr).sin(), my * (pri + spr).sin(), -rows[5][0]]
    elif kind == OP_CDF:                                               # cuburn/code/iter.py:12-30
        ws = [R(a + k, False) for k in range(b)]
        used = [x[1] for x in ws]
        tot = ws[0][0]
        for w, _ in ws[1:]:
            tot = tot + w
        rsum = 1.0 / tot
        out, acc = [], None
        for w, _ in ws:
            acc = w * rsum if acc is None else acc + w * rsum
            out.append(acc)
        out[-1] = V(2.0 * one, 0.0 * one)
    elif kind == OP_RATIO2:                                            # cuburn/code/variations.py:292-294
        (x, s0), (y, s1) = R(a, True), R(b, True)
        used = [s0, s1]
        out = [x / (2.0 * y)]
    elif kind == OP_INVSQ:                                             # cuburn/code/variations.py:136-140
        v, s0 = R(a, False)
        used = [s0]
        out = [1.0 / (v * v + E20)]
    elif kind == OP_INVSQ_MAX:                                         # cuburn/code/variations.py:630-634
        v, s0 = R(a, True)
        used = [s0]
        out = [1.0 / (v * v).maximum(E20)]
    elif kind == OP_PERSP:                                             # cuburn/code/variations.py:267-273
        (ang, s0), (dist, s1) = R(a, False), R(b, True)
        used = [s0, s1]
        ang = ang * PI_2
        pd = dist.maximum(E9)
        out = [pd, ang.sin(), pd * ang.cos()]
    elif kind == OP_OPACITY:                                           # include/flame_hip.h (6)
        v, s0 = R(a, True)
        used = [s0]
        p = np.clip(v.v, 0.0, 1.0)
        live = (p > 0) & (p < ONE_M)
        ps = np.where(live, p, 0.5)
        l = np.log2(ps)
        e = l * OPACITY_POW
        q = np.exp2(e)
        se = (np.abs(l) + v.s / (ps * np.log(2.0))) * OPACITY_POW
        cls = np.where(p <= 0, 0, np.where(p >= ONE_M, 1, np.where(q < Q_MIN, 2, 3)))
        val = np.where(cls == 1, 1.0, np.where(cls == 3, q, 0.0))
        out = [V(val, np.where(cls == 3, q * (1.0 + np.log(2.0) * se), 0.0))]
        # how far the spline is from each outcome's threshold, relative (to its scale at the threshold 0)
        pv = v.v
        with np.errstate(divide='ignore', invalid='ignore'):
            p_q = 2.0 ** (-32.0 / OPACITY_POW)
            near = np.minimum(np.minimum(np.abs(pv) / v.s, np.abs(pv - ONE_M) / ONE_M), np.abs(pv - p_q) / p_q)
        used[0].opacity_margin = np.where(np.isfinite(near), near, 1.0)
    else:
        raise ValueError('op kind %d' % kind)
    vals = np.stack([np.broadcast_to(o.v, (n,)) for o in out], 1)
    scales = np.stack([np.broadcast_to(o.s, (n,)) for o in out], 1)
    return vals, scales, cls, used


def blocks(T, K, ops, t, dim, pstride):
    """The parameter blocks (n, pstride) the op list writes at times t, their scales, and the mask of written words."""
    val, sc, written = np.zeros((len(t), pstride)), np.zeros((len(t), pstride)), np.zeros(pstride, bool)
    for op in ops:
        v, s, _, _ = op_values(T, K, op, t, dim)
        d = int(op[1])
        val[:, d:d + v.shape[1]], sc[:, d:d + v.shape[1]] = v, s
        written[d:d + v.shape[1]] = True
    return val, sc, written


# ------------------------------------------------------------------ palette
YUV = np.array([[F32(0.299), F32(0.587), F32(0.114)], [F32(-0.168736), F32(-0.331264), F32(0.5)],
                [F32(0.5), F32(-0.418688), F32(-0.081312)]], np.float64)                    # cuburn/code/color.py:18-23


def dither_draws(seeds, mwc_stream):
    """The three draws per cell of cuburn/code/interp.py:422-424 as the float32 0.49 * mwc_next_11 holds them, (64, 256, 3), and
    the RNG states after.  mwc_stream(state, n) gives the next n u32 of one state (the oracle's)."""
    seeds = np.ascontiguousarray(seeds, np.uint32).reshape(64 * 256, 3)
    u = np.stack([mwc_stream(s, 3) for s in seeds]).astype(np.uint32)
    after = seeds.copy()
    mul, state, carry = [seeds[:, i].astype(np.uint64) for i in range(3)]
    for _ in range(3):
        x = mul * state + carry
        state, carry = x & np.uint64(0xffffffff), x >> np.uint64(32)
    after[:, 1], after[:, 2] = state.astype(np.uint32), carry.astype(np.uint32)
    assert np.array_equal(after[:, 1], u[:, 2])
    f = u.view(np.int32).astype(F32).astype(np.float64) * 2.0 ** -31            # cvt.rn.f32.s32, then * 2^-31 (exact)
    return (f * float(F32(0.49))).reshape(64, 256, 3), after.reshape(64, 256, 3)


def palette(pals, ptimes, ts, td, draws):
    """(pre-truncation Y, U, V (64, 256, 3) float64, packed cells (64, 256) uint64) of cuburn/code/interp.py:372-433."""
    pals = np.asarray(pals, F32)
    pt = np.full(KNOTS, PAD_TIME, F32)
    pt[:len(ptimes)] = ptimes
    src = np.zeros((KNOTS, 256, 4), np.float64)
    src[:len(pals)] = pals
    time = sample_times(ts, td, 64)
    idx = np.maximum(binsearch32(pt, 0, time) + 1, 1)
    pt64, t64 = pt.astype(np.float64), time.astype(np.float64)
    tr = pt64[idx]
    past = tr > 1.0
    with np.errstate(divide='ignore', invalid='ignore'):
        lf = np.where(past, 1.0, (tr - t64) / (tr - pt64[idx - 1]))
    rf = np.where(past, 0.0, 1.0 - lf)
    left = src[idx - 1][:, :, :3]
    right = np.where(past[:, None, None], left, src[idx][:, :, :3])
    yuv = (left @ YUV.T) * lf[:, None, None] + (right @ YUV.T) * rf[:, None, None]
    yuv[:, :, 1:] += 0.5
    pre = yuv * 255.0 + draws
    q = np.where(pre > 0, np.floor(np.minimum(np.where(np.isnan(pre), 0.0, pre), 4294967040.0)), 0.0)
    q = np.minimum(q, 255.0).astype(np.uint64)
    hi = (np.uint64(1) << np.uint64(22)) | (q[:, :, 0] << np.uint64(4))
    lo = (q[:, :, 1] << np.uint64(18)) | q[:, :, 2]
    return pre, (hi << np.uint64(32)) | lo


def unpack_yuv(cells):
    """(64, 256) packed palette cells -> (64, 256, 3) y, u, v."""
    cells = np.asarray(cells, np.uint64)
    hi, lo = cells >> np.uint64(32), cells & np.uint64(0xffffffff)
    return np.stack([(hi >> np.uint64(4)) & np.uint64(0x3ffff), lo >> np.uint64(18), lo & np.uint64(0x3ffff)], 2).astype(np.int64)


def palette_condition(cells, pre, model_cells):
    """(number of y / u / v values that differ from the model's, how many of those lie further than 2^-12 from an integer of
    the model's pre-truncation value, share of all values that lie within 2^-12 of one)."""
    got, want = unpack_yuv(cells), unpack_yuv(model_cells)
    near = np.abs(pre - np.round(pre)) <= 2.0 ** -12
    diff = got != want
    return int(diff.sum()), int((diff & ~near).sum()), float(near.mean())
