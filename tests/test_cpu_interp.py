"""
CPU tests of the parameter and palette interpolation (cuburn_amd/csrc/interp.hip): the float64 model of tests/interp_model.py,
the float32 oracle (oracle/flame_ref.c: ref_catmull_rom, ref_interp_palette) and the blocks the reference's own generated kernel
wrote (golden/interp_params.npz) tied together on the atlas of tests/interp_cases.py, which reaches every branch of the two
kernels: samples on a knot, knots with equal times, windows that start before t = 0 and end after the last real knot, the three
branches each of linlog / linslope / linexp and their joins, rows of 31 and 32 knots, stills, every precalc op at its clamps, and
palettes before, on, between and after their times.  tests/test_gpu_interp.py holds the HIP kernels to the same model on the same
atlas; its bars are multiples of what the float32 evaluations here deviate from the model, and ORACLE_DEV is what keeps those
from growing unnoticed.

All deviations are in units of the model's scale (tests/interp_model.py), so 2^-24 = 6e-8 is one float32 rounding.
"""
import os

import numpy as np
import pytest

from common import O, REPO, GenomePacker
from cuburn_amd import configs
import interp_model as M
import interp_cases as T

U = 2.0 ** -24

# The float32 evaluations' worst deviation from the float64 model, per class, over every case below, as measured (glibc libm,
# x86-64; in units of 2^-24 of the model's scale, rounded up to two digits).  Splines: the oracle, per (domain, segment kind) and
# for the magnitude domain per branch of linlog(k1), linlog(k2) and linexp(r).  Op kinds: the float32 numpy restatement of
# tests/interp_cases.py (f32_op) over the oracle's splines.
ORACLE_DEV = {
    ('lin', 'on-knot'): 0.0,
    ('lin', 'extrapolated'): 2.7,
    ('lin', 'padding'): 2.7,
    ('lin', 'by-step'): 2.5,
    ('lin', 'interior'): 3.3,
    ('lin', 'next-row'): 2.2,
    ('mag', 'on-knot'): 0.74,
    ('mag', 'extrapolated'): 3.3,
    ('mag', 'padding'): 4.9,
    ('mag', 'by-step'): 2.6,
    ('mag', 'interior'): 5.2,
    ('mag', 'next-row'): 2.3,
    ('mag', 'k1 lin'): 5.2,
    ('mag', 'k1 log+'): 4.2,
    ('mag', 'k1 log-'): 2.2,
    ('mag', 'k2 lin'): 4.9,
    ('mag', 'k2 log+'): 4.2,
    ('mag', 'k2 log-'): 5.2,
    ('mag', 'r lin'): 2.9,
    ('mag', 'r log+'): 4.9,
    ('mag', 'r log-'): 5.2,
    ('camera', 'all'): 1.6,
    ('affine', 'all'): 1.9,
    ('cdf', 'all'): 9.4,
    ('ratio2', 'all'): 0.51,
    ('invsq', 'all'): 3.7,
    ('persp', 'all'): 3.4,
    ('invsq_max', 'all'): 1.3,
    ('opacity', 'all'): 2.0,
}

_measured = {}


def merge(worst, dev):
    for k, v in dev.items():
        worst[k] = max(worst.get(k, 0.0), v)


def measure():
    """(worst deviation per class of the float32 evaluations, population counts), over every genome, window and slot count."""
    if not _measured:
        worst, count = {}, {}
        for g in (T.spline_genome(), T.spline_genome(last32=True)):
            for w in T.WINDOWS:
                for n in T.SLOTS:
                    t = T.times_of(w, n)
                    merge(worst, T.spline_deviations(g, T.f32_blocks(g, t), t, count))
        for g in (T.precalc_genome(), T.opacity_genome()):
            for w in T.WINDOWS:
                for fr in T.FRAMES:
                    t, dim = T.times_of(w, 1024), T.frame_dim(*fr)
                    merge(worst, T.op_deviations(g, T.f32_blocks(g, t, dim), t, dim, count))
        _measured['worst'], _measured['count'] = worst, count
    return _measured['worst'], _measured['count']


def test_oracle_stays_within_its_table_of_the_model(built):
    worst, _ = measure()
    assert set(worst) == set(ORACLE_DEV), sorted(set(worst) ^ set(ORACLE_DEV), key=str)
    for key in sorted(worst):
        print('%-28s measured %.3f  table %.3g   (x 2^-24 of scale)' % (key, worst[key] / U, ORACLE_DEV[key]))
    for key, v in worst.items():
        assert 0.7 * ORACLE_DEV[key] <= v / U <= ORACLE_DEV[key], (key, v / U, ORACLE_DEV[key])       # the table IS what is measured
    # what the issue of this file measured: the worst spline class at 5.2, on a magnitude row at the +-0.0625 join
    assert max(v for (d, _), v in ORACLE_DEV.items() if d in ('lin', 'mag')) <= 5.2
    assert max(v for (d, _), v in ORACLE_DEV.items() if d == 'lin') < 3.8


def test_population(built):
    """A condition, from the model alone: every class holds at least 8 samples (so both sides of every linlog / linslope /
    linexp join are populated), every on-knot row has samples whose time equals a knot exactly, at most a quarter of any
    magnitude row is cut by |r| <= 64, at most 4 samples of an opacity row lie within 1e-6 of an outcome's threshold and every
    outcome occurs, and nothing the model can see is a float32 denormal."""
    _, count = measure()
    for key in ORACLE_DEV:
        if key[0] in ('lin', 'mag'):
            assert count[key] >= 8, (key, count[key])
    for name in T.ON_KNOT_ROWS:
        for mag in (False, True):
            assert count[('on', name, mag)] >= 8, name
    cuts = {k: v for k, v in count.items() if k[0] == 'cut'}
    assert len(cuts) == 2 * len(T.spline_rows()) and max(cuts.values()) <= 0.25, cuts
    assert not any(v for k, v in cuts.items() if not k[2])
    for name, _, _ in T.opacity_rows():
        assert count[('unsure', name)] <= 4, name
    for c in M.OPACITY_CLS:
        assert count[('opacity', c)] >= 8, c
    g = T.spline_genome()
    assert not ((np.abs(g.T) < M.TINY) & (g.T != 0)).any() and not ((np.abs(g.K) < M.TINY) & (g.K != 0)).any()
    for w in T.WINDOWS:
        for n in T.SLOTS:
            x = np.abs(T.intermediates(g, T.times_of(w, n)))
            assert not ((x > 0) & (x < M.TINY)).any(), w


def test_windows_land_on_the_knots():
    """(-0.25, 2.0) steps by 2^-9 at 1024 samples and by f32(1 / 768) at 1536, 192 of which round to 0.25 exactly: both slot
    counts put a sample on each of the knots at 0, 0.25, 0.5, 0.75 and 1, and on the step the model takes the lower knot."""
    g = T.spline_genome()
    row = [n for n, _, _ in T.spline_rows()].index('elbows') + 1
    hit = lambda n: int(M.spline(g.T, g.K, row, T.times_of(T.WINDOWS[0], n), False).on_knot.sum())
    assert hit(1024) == 5 and hit(1536) == 5
    step = [n for n, _, _ in T.spline_rows()].index('step') + 1
    for w in (T.WINDOWS[0], T.WINDOWS[2]):
        t = T.times_of(w, 1024)
        S = M.spline(g.T, g.K, step, t, False)
        at = t == np.float32(0.5)
        assert at.any() and (S.value[at] == 0.0).all()               # strictly-below search: on the step, the lower knot
        assert (M.spline(g.T, g.K, step, t, True).value[at] == 0.0).all()
    t = T.times_of(T.WINDOWS[1], 1024)                                # the straddling frame sees both sides
    v = M.spline(g.T, g.K, step, t, False).value
    assert v[t <= 0.5].max() < 0.01 and v[t > 0.5].min() > 0.99


def test_row_of_32_knots_borrows_from_its_neighbour(built):
    """After its 31st knot a 32-knot row takes the fourth support point from word 0 of the next row — of the padding when it is
    the last (include/flame_hip.h (4)); model and oracle agree on both, and the two results differ."""
    name = [n for n, _, _ in T.spline_rows()]
    t = T.times_of(T.WINDOWS[4], 1024)
    mid, last = T.spline_genome(), T.spline_genome(last32=True)
    a = M.spline(mid.T, mid.K, name.index('knots32') + 1, t, False)
    b = M.spline(last.T, last.K, 1, t, False)
    late = a.seg == M.SEG.index('next-row')
    assert late.sum() >= 8 and np.array_equal(late, b.seg == M.SEG.index('next-row'))
    assert np.array_equal(a.value[~late], b.value[~late]) and (a.value[late] != b.value[late]).all()
    for g, row, S in ((mid, name.index('knots32') + 1, a), (last, 1, b)):
        for mag in (False, True):
            S = M.spline(g.T, g.K, row, t, mag)
            dev = M.mag_deviation(T.oracle_row(g, row, t, mag), S) if mag else np.abs(T.oracle_row(g, row, t, mag) - S.r)
            assert (T.ratio(dev, S.scale)[late] <= 4 * U).all()


@pytest.mark.parametrize('cfg', ['cfg3', 'cfg5', 'allvars'])
def test_reference_kernel_blocks_against_the_model(cfg):
    """golden/interp_params.npz holds the blocks the reference's own generated interp_iter_params kernel wrote: by field name
    they lie within the float32 evaluations' table of the model, under the same metric (the last cumulative density aside, which
    the reference stores as a sum and this project as 2.0)."""
    gold = np.load(os.path.join(REPO, 'tests', 'golden', 'interp_params.npz'))
    gnm, _ = configs.allvars() if cfg == 'allvars' else configs.CONFIGS[cfg]()
    packer = GenomePacker(gnm)
    g = T.Packed(packer, gnm)
    names = ['.'.join(n) for n in packer.packed]
    t, d = gold[cfg + '_times'], gold[cfg + '_dim']
    dim = (int(d[0]), int(d[2]), int(d[3]))
    val, _, _ = M.blocks(g.T, g.K, g.ops, t, dim, g.pstride)
    got = val.astype(np.float32)                            # (structure words and the last density keep the model's value)
    ref_names = [str(x) for x in gold[cfg + '_names']]
    for j, rn in enumerate(ref_names):
        got[:, names.index('den.' + rn[4:] if rn.startswith('den_') else rn)] = gold[cfg + '_blocks'][:, j]
    worst = T.spline_deviations(g, got, t)
    worst.update(T.op_deviations(g, got, t, dim, cdf_last=False))
    assert len(worst) >= 4
    for key, v in worst.items():
        assert v / U <= max(ORACLE_DEV[key], 1.5), (cfg, key, v / U)


@pytest.mark.parametrize('case', range(len(T.palette_cases())), ids=[c[0] for c in T.palette_cases()])
def test_palette_oracle_against_the_model(built, case):
    """The oracle's packed cells differ from the model's only where the model's value before truncation lies within 2^-12 of an
    integer, and at most 0.2 % of a case's 49152 values lie there; the RNG states afterwards are the model's."""
    name, pals, times, (ts, td), seed = T.palette_cases()[case]
    pre, cells, after = T.palette_model(case)
    got, rng = O.interp_palette(pals, np.array(times, np.float32), ts, td, T.palette_seeds(seed))
    ndiff, far, near = M.palette_condition(got, pre, cells)
    print('%s: %d of 49152 values differ, %.4f %% within 2^-12 of an integer' % (name, ndiff, 100 * near))
    assert far == 0 and near <= 0.002, (name, ndiff, far, near)
    assert np.array_equal(rng.reshape(-1, 3), after)
    assert (M.unpack_yuv(cells) <= 255).all() and (cells >> np.uint64(54) == 1).all()


def test_palette_cases_reach_their_branches():
    c = T.palette_cases()
    hay = lambda i: np.concatenate([np.float32(c[i][2]), np.full(32 - len(c[i][2]), M.PAD_TIME, np.float32)])
    rows = lambda i: M.sample_times(c[i][3][0], c[i][3][1], 64)
    tr = lambda i: hay(i)[np.maximum(M.binsearch32(hay(i), 0, rows(i)) + 1, 1)]
    assert (tr(0) > 1).all()                                                          # one palette: always the tr > 1 branch
    assert (rows(1) < 0).sum() >= 8 and ((tr(1) > 1) & (rows(1) > 1)).sum() >= 8       # before the first, after the last
    assert (rows(2) == np.float32(0.5)).sum() == 1                                     # a row on the middle palette's time
    assert len(c[3][1]) == 31 and len(np.unique(M.binsearch32(hay(3), 0, rows(3)))) >= 30
    assert (rows(4) < 0.25).sum() >= 8 and ((tr(4) > 1) & (rows(4) > 0.75)).sum() >= 8  # lf > 1, then tr > 1
    assert (rows(5) == np.float32(0.5)).sum() == 1 and c[5][2][1] == c[5][2][2]
    assert (tr(7) == np.float32(1.5)).all()                                            # tr > 1, and a real palette there
    pre = T.palette_model(6)[0]
    assert (pre < -1).sum() >= 256 and (pre > 256).sum() >= 256                        # f2u_trunc sees negatives, the clamp > 255


if __name__ == '__main__':
    for key, v in measure()[0].items():
        print('    (%r, %r): %.2g,' % (key[0], key[1], v / U))
