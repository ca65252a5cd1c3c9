"""
The case atlas of the interpolation tests (tests/test_cpu_interp.py, tests/test_gpu_interp.py): synthetic genomes written
straight onto the C ABI (include/flame_hip.h (4)-(6)), the frame windows, the palette cases, and the metric that compares any
evaluation — the float32 oracle's, a float32 numpy restatement's, the device's — with the float64 model of tests/interp_model.py.

A synthetic genome is the smallest program fl_genome_create accepts (one linear xform, no final: cdf_off 6, xf_off 8, xf_stride
20, var_stride 4, its two structure words) with a parameter block long enough that every case op writes words of its own
behind the record.  The opacity ops must write word 15 of a selectable record, one per record, so they get a program of their
own with one xform each.  Row 0 of every table is a guard whose second knot lies before every window.

Knot times are dyadic wherever a case is about landing on a knot: at 1024 samples the window (-0.25, 2.0) steps by 2^-9 and
hits the knots at multiples of 1/32; at 1536 the step is f32(1 / 768), whose multiples of 24 round onto them as well, and
every other sample lies off the dyadic grid.
"""
import numpy as np

from common import O
from cuburn_amd import mwc
import interp_model as M

F32 = np.float32
MAGIC = 0x464c5032
LINEAR = 0                                   # flam3 variation number of `linear`
WINDOWS = [(-0.25, 2.0), (0.5 - 2.0 ** -11, 2.0 ** -10), (0.5, 0.0), (1.0, 0.0), (0.96875, 0.0625)]
WINDOW_IDS = ['wide', 'straddle', 'still-0.5', 'still-1', 'last-frame']
SLOTS = [1024, 1536]
FRAMES = [(200, 120), (33, 17)]
R_MAX = 64.0                                 # beyond |r| = 64 exp2f overflows, in the reference as well: cut
UP = float(np.nextafter(F32(0.0625), F32(1)))


class Genome(object):
    """prog, ops (n, 4) int32, times / knots (nrows, 32) float32, labels (one per op), pstride."""

    def __init__(self, nxf=1, opacity=False):
        self.nxf, self.opacity = nxf, opacity
        self.xf_off = 8 if nxf == 1 else (6 + nxf + 3) // 4 * 4
        self.next = self.xf_off + nxf * 20
        self.rows, self.ops, self.labels = [], [], []
        for i in range(nxf):
            rec = self.xf_off + 20 * i
            self.op(M.OP_CONST, rec + 14, 1 | (512 if opacity else 0), 0, 'nvar')
            self.op(M.OP_CONST, rec + 16, LINEAR, 0, 'id')
        self.row([-4, -3, 3, 4], [0.75, 0.75, 0.75, 0.75])            # the guard (and a constant)

    def row(self, times, knots):
        assert len(times) == len(knots) <= 32 and list(times) == sorted(times)
        self.rows.append((np.asarray(times, F32), np.asarray(knots, F32)))
        return len(self.rows) - 1

    def op(self, kind, dst, a, b, label):
        self.ops.append((kind, dst, a, b))
        self.labels.append(label)

    def add(self, kind, a, b, label):
        """An op writing fresh words behind the record."""
        n = b if kind == M.OP_CDF else M.NDST[kind]
        self.op(kind, self.next, a, b, label)
        self.next += n

    def finish(self, pstride=None):
        self.pstride = pstride or (self.next + 3) // 4 * 4
        assert self.next <= self.pstride <= 4096
        self.prog = np.array([MAGIC, self.nxf, 0, self.pstride, 6, self.xf_off, 20, 4], np.int32)
        self.ops = np.array(self.ops, np.int32).reshape(-1, 4)
        self.nrows = len(self.rows)
        self.times = np.full((self.nrows, 32), M.PAD_TIME, F32)
        self.knots = np.zeros((self.nrows, 32), F32)
        for i, (t, k) in enumerate(self.rows):
            self.times[i, :len(t)], self.knots[i, :len(k)] = t, k
        self.T, self.K = M.flat_table(self.times, self.knots)
        return self


STD = [-2, 0, 1, 3]
QUART = [-2, 0, 0.25, 0.5, 0.75, 1, 3]


def long_row(ninterior):
    """ninterior knots in [0, 1] at multiples of 1/32 (the last at 1) between the guards at -2 and 3."""
    t = [-2.0] + [k / 32.0 for k in range(ninterior - 1)] + [1.0, 3.0]
    k = [0.5] + [0.5 + 0.4 * np.sin(1.7 * i) + 0.01 * i for i in range(ninterior)] + [0.25]
    return t, k


def spline_rows():
    """(name, times, knots) of the rows every spline case evaluates in both domains."""
    a = 0.5 - 2.0 ** -11
    return [
        ('ramp', STD, [0.5, 0.0, 1.0, -0.25]),                                        # guard knots off the line
        ('velocities', STD, [-0.75, 0.25, 0.75, -1.25]),                              # end velocities +0.5 / -0.5
        ('step', [-2, 0, 0.5, 0.5, 1, 3], [0.25, 0.25, 0.0, 1.0, 0.75, 0.75]),
        ('elbows', QUART, [0.5, 0.03125, 0.125, -0.03125, -0.25, 0.046875, 0.5]),     # both sides of +-0.0625
        ('short', [-2, 0, a, a + 2.0 ** -10, 1, 3], [0.3, 0.3, 0.2, 0.6, 0.4, 0.4]),   # a segment of length 2^-10
        ('on-elbow', QUART, [0.0625, 0.0625, UP, -0.0625, -UP, 0.0625, 0.0625]),
        ('crossing', STD, [4.0, 4.0, -3.0, -3.0]),
        ('decades', [-2] + [i / 8.0 for i in range(9)] + [3], [1e-4] + [1e-4 * 10 ** (9 * i / 8.0) for i in range(9)] + [1e5]),
        ('knots31',) + long_row(29),
        ('knots32',) + long_row(30),
        ('after32', STD, [0.125, 0.5, 0.25, 0.75]),                                   # what the 32-knot row borrows from
    ]


ON_KNOT_ROWS = ['step', 'elbows', 'on-elbow', 'decades', 'knots31', 'knots32']


def spline_genome(last32=False):
    """Every spline row as FL_OP_SPLINE and as FL_OP_SPLINE_MAG.  last32: the 32-knot row alone behind the guard, as the LAST row."""
    g = Genome()
    for name, t, k in spline_rows():
        if last32 and name != 'knots32':
            continue
        r = g.row(t, k)
        g.add(M.OP_SPLINE, r, 0, name)
        g.add(M.OP_SPLINE_MAG, r, 0, name)
    return g.finish()


def precalc_genome():
    """Every other op kind (but the opacity), at ordinary values and at its edges."""
    g = Genome()
    zero, milli = g.row(STD, [0, 0, 0, 0]), g.row(STD, [1e-3] * 4)
    ramp, vel = g.row(STD, [0.5, 0.0, 1.0, -0.25]), g.row(STD, [0.75, 0.25, 0.75, 1.25])
    cross = g.row(STD, [4.0, 4.0, -3.0, -3.0])
    for r, lab in ((zero, 'v=0'), (milli, 'v=1e-3'), (ramp, 'ramp')):
        g.add(M.OP_INVSQ, r, 0, lab)
    for r, lab in ((zero, 'v=0'), (vel, 'ordinary'), (cross, 'crossing')):
        g.add(M.OP_INVSQ_MAX, r, 0, lab)
    quarter = [g.row(STD, [q] * 4) for q in (0.0, 1.0, 2.5)]
    g.add(M.OP_PERSP, quarter[0], zero, 'angle 0, dist 0')
    g.add(M.OP_PERSP, quarter[1], vel, 'angle 1')
    g.add(M.OP_PERSP, quarter[2], vel, 'angle 2.5')
    g.add(M.OP_PERSP, ramp, milli, 'angle ramp')
    g.add(M.OP_RATIO2, vel, 0, 'vel / guard')
    g.add(M.OP_RATIO2, cross, vel, 'crossing / vel')
    # affine: angle, spread, magnitude.x, magnitude.y, offset.x, offset.y
    first = g.row(STD, [-720, -720, 720, 720])
    for t, k in ((STD, [0, 0, 90, 90]), (STD, [-0.8] * 4), (STD, [0.75, 0.25, 0.75, 1.25]), (STD, [0.5, 0.0, 1.0, -0.25]), (STD, [2, -1, 1, 2])):
        g.row(t, k)
    g.add(M.OP_AFFINE, first, 0, '+-720 degrees, negative magnitude')
    first = g.row(STD, [30] * 4)
    for t, k in ((STD, [0] * 4), (STD, [1] * 4), (STD, [0.5] * 4), (STD, [0] * 4), (STD, [-0.25] * 4)):
        g.row(t, k)
    g.add(M.OP_AFFINE, first, 0, 'constant')
    # camera: rotation, center.x, center.y, scale
    first = g.row(STD, [-30, -30, 400, 400])
    for t, k in ((STD, [0.5, 0.0, 1.0, -0.25]), (STD, [-1, 0.5, -0.5, 1]), (STD, [0.5, 0.5, 2, 2])):
        g.row(t, k)
    g.add(M.OP_CAMERA, first, 0, 'turning')
    first = g.row(STD, [0] * 4)
    for t, k in ((STD, [0] * 4), (STD, [0] * 4), (STD, [1] * 4)):
        g.row(t, k)
    g.add(M.OP_CAMERA, first, 0, 'identity')
    # cumulative densities: lengths 1, 2, 9, 64; a zero weight; a weight whose spline dips below zero between its knots
    over = (QUART, [0, 0, 0, 1, 0, 0, 0])
    rng = np.random.RandomState(5)
    weights = [(STD, [w, w, v, v]) for w, v in F32(0.125 + rng.rand(64, 2))]
    g.add(M.OP_CDF, g.row(*weights[0]), 1, 'length 1')
    first = g.row(STD, [0.75] * 4)
    g.row(*over)
    g.add(M.OP_CDF, first, 2, 'length 2, overshoot')
    first = g.row(*weights[1])
    for i in range(2, 9):
        g.row(*(weights[i] if i != 4 else (STD, [0] * 4)))
    g.row(*over)
    g.add(M.OP_CDF, first, 9, 'length 9, zero weight')
    first = g.row(*weights[0])
    for w in weights[1:]:
        g.row(*w)
    g.add(M.OP_CDF, first, 64, 'length 64')
    return g.finish()


def opacity_rows():
    return [('through 0', STD, [-0.03, -0.03, 0.05, 0.05]), ('through 0.00126', STD, [0.0005, 0.0005, 0.004, 0.004]),
            ('through 1', STD, [0.9, 0.9, 1.1, 1.1]), ('constant 1', STD, [1.0] * 4), ('constant 0', STD, [0.0] * 4),
            ('ordinary', STD, [0.2, 0.2, 0.8, 0.8])]


def opacity_genome():
    rows = opacity_rows()
    g = Genome(nxf=len(rows), opacity=True)
    for i, (name, t, k) in enumerate(rows):
        g.op(M.OP_OPACITY, g.xf_off + 20 * i + 15, g.row(t, k), 0, name)
    return g.finish()


# ------------------------------------------------------------------ evaluations
def times_of(window, nts):
    return M.sample_times(window[0], window[1], nts)


def oracle_row(g, row, t, mag):
    """The float32 oracle's spline of one row at float32 times t, on the flat table (a 32-knot row sees its neighbour)."""
    fn = O.lib().ref_catmull_rom
    pt, pk = g.T.ctypes.data + 128 * row, g.K.ctypes.data + 128 * row
    ut, inv = np.unique(t, return_inverse=True)
    return np.array([fn(pt, pk, float(x), int(mag)) for x in ut], F32)[inv]


def f32_op(g, op, t, dim):
    """The op formulas in float32 numpy over the oracle's spline values, in the order interp.hip writes them: the float32
    yardstick of the precalc ops.  (n, ndst) float32."""
    kind, _, a, b = [int(x) for x in op]
    R = lambda r, mag: oracle_row(g, r, t, mag)
    one, two, half = F32(1), F32(2), F32(0.5)
    pi, pi_2, d180 = F32(M.PI), F32(M.PI_2), F32(180)
    if kind in (M.OP_SPLINE, M.OP_SPLINE_MAG):
        out = [R(a, kind == M.OP_SPLINE_MAG)]
    elif kind == M.OP_CONST:
        out = [np.full(len(t), np.array([a], np.int32).view(F32)[0])]
    elif kind == M.OP_CAMERA:
        rot = R(a, False) * pi / d180
        rs, rc = np.sin(rot), np.cos(rot)
        cx, cy = R(a + 1, False), R(a + 2, False)
        sc = R(a + 3, True) * F32(dim[0])
        out = [sc * rc, sc * -rs, sc * (rs * cy - rc * cx) + half * F32(dim[1]), sc * rs, sc * rc, sc * -(rs * cx + rc * cy) + half * F32(dim[2])]
    elif kind == M.OP_AFFINE:
        pri, spr = R(a, False) * pi / d180, R(a + 1, False) * pi / d180
        mx, my = R(a + 2, True), R(a + 3, True)
        out = [mx * np.cos(pri - spr), -my * np.cos(pri + spr), R(a + 4, False), -mx * np.sin(pri - spr), my * np.sin(pri + spr), -R(a + 5, False)]
    elif kind == M.OP_CDF:
        ws = [R(a + k, False) for k in range(b)]
        tot = np.zeros(len(t), F32)
        for w in ws:
            tot = tot + w
        rsum = one / tot
        acc, out = np.zeros(len(t), F32), []
        for w in ws:
            acc = acc + w * rsum
            out.append(acc)
        out[-1] = np.full(len(t), two)
    elif kind == M.OP_RATIO2:
        out = [R(a, True) / (two * R(b, True))]
    elif kind == M.OP_INVSQ:
        v = R(a, False)
        out = [one / (v * v + F32(1.0e-20))]
    elif kind == M.OP_INVSQ_MAX:
        v = R(a, True)
        out = [one / np.maximum(F32(1e-20), v * v)]
    elif kind == M.OP_PERSP:
        ang = R(a, False) * pi_2
        pd = np.maximum(F32(1e-9), R(b, True))
        out = [pd, np.sin(ang), pd * np.cos(ang)]
    elif kind == M.OP_OPACITY:
        p = np.minimum(np.maximum(R(a, True), F32(0)), one)
        with np.errstate(divide='ignore'):
            q = np.exp2(np.log2(p) * F32(3.3219281))
        q = np.where(q < F32(2.3283064e-10), F32(0), q)
        out = [np.where(p <= 0, F32(0), np.where(p >= one - F32(1.0e-6), one, q))]
    out = np.stack(out, 1)
    assert out.dtype == F32
    return out


def f32_blocks(g, t, dim=(1, 1, 1)):
    """Parameter blocks (n, pstride) float32 of the float32 evaluation above."""
    out = np.zeros((len(t), g.pstride), F32)
    for op in g.ops:
        v = f32_op(g, op, t, dim)
        out[:, op[1]:op[1] + v.shape[1]] = v
    return out


def frame_dim(w, h):
    d = O.calc_dim(w, h)
    return (d.w, d.aw, d.ah)


# ------------------------------------------------------------------ the metric
def ratio(dev, scale):
    """dev / scale, 0 where both are 0, inf where only the scale is."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(dev == 0, 0.0, dev / scale)


def spline_classes(S, mag):
    """{class key: sample mask} of one evaluated row: the segment kinds, and for a magnitude row the branch of k1, k2 and r."""
    dom = 'mag' if mag else 'lin'
    out = {(dom, M.SEG[i]): S.seg == i for i in range(len(M.SEG))}
    if mag:
        for what, br in (('k1', S.k1b), ('k2', S.k2b), ('r', S.rb)):
            for i, name in enumerate(M.BRANCH):
                out[(dom, what + ' ' + name)] = br == i
    return out


def spline_deviations(g, got, t, count=None):
    """Worst deviation / scale per class of the spline ops of blocks `got` (n, pstride) at times t, {key: value}.  Magnitude rows
    are measured in the magnitude domain and cut to the model's |r| <= R_MAX.  count (optional dict) receives the population
    per class, and per (label, domain) the share cut and the number of samples with time == knot."""
    worst = {}
    for op, label in zip(g.ops, g.labels):
        if op[0] not in (M.OP_SPLINE, M.OP_SPLINE_MAG):
            continue
        mag = op[0] == M.OP_SPLINE_MAG
        S = M.spline(g.T, g.K, int(op[2]), t, mag)
        x = got[:, op[1]].astype(np.float64)
        keep = np.abs(S.r) <= R_MAX if mag else np.ones(len(t), bool)
        assert np.isfinite(x[keep]).all(), (label, mag)
        with np.errstate(invalid='ignore'):
            dev = ratio(M.mag_deviation(x, S) if mag else np.abs(x - S.r), S.scale)
        for key, mask in spline_classes(S, mag).items():
            mask = mask & keep
            if mask.any():
                worst[key] = max(worst.get(key, 0.0), float(dev[mask].max()))
            if count is not None:
                count[key] = count.get(key, 0) + int(mask.sum())
        if count is not None:
            count[('cut', label, mag)] = max(count.get(('cut', label, mag), 0.0), 1.0 - float(keep.mean()))
            count[('on', label, mag)] = count.get(('on', label, mag), 0) + int(S.on_knot.sum())
    return worst


OPACITY_MARGIN = 1e-6                        # samples this close (relative) to an outcome's threshold are not held to the outcome


def op_deviations(g, got, t, dim, count=None, cdf_last=True):
    """The same for every other op kind, {(kind name, label-independent class): worst deviation / scale}; exact words (FL_OP_CONST,
    the last CDF word, the opacity outcomes 0 and 1 away from their thresholds) are asserted here, bit for bit."""
    worst = {}
    for op, label in zip(g.ops, g.labels):
        kind = int(op[0])
        if kind in (M.OP_SPLINE, M.OP_SPLINE_MAG):
            continue
        val, sc, cls, used = M.op_values(g.T, g.K, op, t, dim)
        x = got[:, op[1]:op[1] + val.shape[1]]
        if kind == M.OP_CONST:
            assert (x.view(np.int32) == op[2]).all(), 'FL_OP_CONST word %d' % op[1]
            continue
        x = x.astype(np.float64)
        assert np.isfinite(x).all(), (M.OP_NAMES[kind], label)
        if kind == M.OP_CDF and cdf_last:
            assert (x[:, -1] == 2.0).all(), 'CDF %s: the last word is not 2.0' % label
        dev = ratio(np.abs(x - val), sc)
        if kind == M.OP_CDF and not cdf_last:
            dev[:, -1] = 0.0                                           # (the reference stores the last cumulative sum itself)
        if kind == M.OP_OPACITY:
            sure = used[0].opacity_margin > OPACITY_MARGIN
            for c in (0, 1, 2):                                        # zero, one, flushed: exact outcomes
                m = sure & (cls == c)
                assert (x[m, 0] == (1.0 if c == 1 else 0.0)).all(), 'opacity %s: outcome %s' % (label, M.OPACITY_CLS[c])
            m = sure & (cls == 3)
            assert ((x[m, 0] > 0) & (x[m, 0] < 1)).all(), 'opacity %s: outcome power' % label
            if count is not None:
                count[('unsure', label)] = max(count.get(('unsure', label), 0), len(np.unique(t[~sure])))
                for c in range(4):
                    count[('opacity', M.OPACITY_CLS[c])] = count.get(('opacity', M.OPACITY_CLS[c]), 0) + int((sure & (cls == c)).sum())
            dev = np.where((sure & (cls == 3))[:, None], dev, 0.0)
        key = (M.OP_NAMES[kind], 'all')
        worst[key] = max(worst.get(key, 0.0), float(dev.max()))
    return worst


class Packed(object):
    """A real genome's packer output in the shape of a Genome above: ops, labels, flat table."""

    def __init__(self, packer, gnm):
        self.ops = np.ascontiguousarray(packer.ops_array, np.int32).reshape(-1, 4)
        self.labels = ['.'.join(packer.packed[int(o[1])]) for o in self.ops]
        self.times, self.knots = packer.pack(gnm)
        self.T, self.K = M.flat_table(self.times, self.knots)
        self.pstride, self.nrows = packer.pstride, packer.nrows


def intermediates(g, t):
    """Every intermediate of every spline op the model can see, for the denormal check."""
    out = []
    for op in g.ops:
        if op[0] in (M.OP_SPLINE, M.OP_SPLINE_MAG):
            out += M.spline(g.T, g.K, int(op[2]), t, op[0] == M.OP_SPLINE_MAG).inter
    return np.concatenate([np.ravel(x) for x in out])


# ------------------------------------------------------------------ palettes
def _blocks(vals):
    """A 256-entry palette of equal blocks of the given grey levels."""
    p = np.ones((256, 4), F32)
    p[:, :3] = np.repeat(np.asarray(vals, F32), 256 // len(vals))[:, None]
    return p


def palette_cases():
    """(name, palettes (n, 256, 4) float32, times, (ts, td), seed of the 64 x 256 RNG states)."""
    rng = np.random.RandomState(11)
    P = lambda n: np.concatenate([F32(rng.rand(n, 256, 3)), np.ones((n, 256, 1), F32)], 2)
    edge = P(2)
    edge[0, :, :3] = _blocks([0.0, 1.0, 1.5, -0.5])[:, :3]
    edge[1, :, :3] = _blocks([1.5, -0.5, 0.0, 1.0])[:, :3] * F32([1.0, 0.5, 2.0])
    return [
        ('one', P(1), [0.0], (0.25, 0.5), 101),
        ('two, window past both ends', P(2), [0.0, 1.0], (-0.25, 1.5), 102),
        ('three, a row on the middle one', P(3), [0.0, 0.5, 1.0], (0.0, 1.0), 103),
        ('thirty-one', P(31), [i / 30.0 for i in range(31)], (0.0, 1.0), 104),
        ('first rows extrapolate', P(2), [0.25, 0.75], (0.0, 1.0), 105),
        ('two at the same time', P(4), [0.0, 0.5, 0.5, 1.0], (0.0, 1.0), 106),
        ('outside [0, 1]', edge, [0.0, 1.0], (0.0, 1.0), 107),
        ('the second after t = 1', P(2), [0.0, 1.5], (0.0, 1.0), 108),        # tr > 1 with a real palette to its right
    ]


def palette_seeds(seed):
    return np.ascontiguousarray(mwc.make_seeds(64 * 256, seed), np.uint32).reshape(64 * 256, 3)


_model_cache = {}


def palette_model(i):
    """(pre-truncation values, model cells, RNG states after) of palette case i, computed once."""
    if i not in _model_cache:
        name, pals, times, (ts, td), seed = palette_cases()[i]
        draws, after = M.dither_draws(palette_seeds(seed), O.mwc_stream)
        pre, cells = M.palette(pals, times, ts, td, draws)
        _model_cache[i] = (pre, cells, after.reshape(-1, 3))
    return _model_cache[i]
