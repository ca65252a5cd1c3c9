"""
The compile-time forms of the per-genome iterate kernel (csrc/iter.hip with FL_RTC), as a table of genome structures that reaches
every one of them, and a plain-Python mirror of the constexpr predicates that choose the form.  DESIGN.md 4.1 has the table of
thresholds; this module is its executable statement:

  * form_of() restates kSpecResident, kHoistCol / kHoistAff / kHoistPost, kHoistFinal, kSpecPost[FL_SPEC_NXF], kTab, SPLIT_FUSE
    (= ROT3) and MERGE from (xform count, post affines, final xform, hoist budget);
  * tests/test_cpu_iter_forms.py has the COMPILER confirm form_of() for every row against the header the library generates
    (tests/iter_forms_probe.hip: iter.hip + one static_assert), so a predicate that moves in iter.hip without moving here fails;
  * tests/test_gpu_iter_forms.py holds every row to the oracle's device model (or, for rows with parametric variations, to the
    interpreter kernel) bit for bit.

Oracle rows use `linear` and `bent` only (no transcendentals: the device model is exact), unequal weights, distinct colours and
colour speeds, and post affines / final xforms that are not the identity.  They start from flames.nxf_flame's ring.
"""
import copy
import itertools

import numpy as np

from cuburn_amd import configs
from flames import nxf_flame
from gpu_harness import run_device_model, setup_frame

BUDGETS = (12, 7, 5, 0)         # FL_HOIST_BUDGET: the default, and what rtc_iter_kernel falls back to past the register limit
MERGE_MAX_XF = 4                # FL_ITER_MERGE_MAX_XF
# the source lines of the two predicates that are local to iter_body (no static_assert can see them): pinned verbatim
SPLIT_FUSE_LINE = 'constexpr bool SPLIT_FUSE = !SPEC || FL_SPEC_NXF <= 9;'
MERGE_LINE = 'constexpr bool MERGE = BINNED && SPEC && SPLIT_FUSE && FL_SPEC_NXF <= FL_ITER_MERGE_MAX_XF && !CHAOS;'
MERGE_MAX_LINE = '#define FL_ITER_MERGE_MAX_XF 4'
PROBED = ('resident', 'col', 'aff', 'post', 'final', 'final_post', 'tab')      # what the probe's static_assert compares (-DEXP_<NAME>)


def form_of(nxf, posts, final, final_post, budget=12, chaos=False):
    """iter.hip's predicates for a genome of `nxf` selectable xforms of which `posts` have a post affine, with (`final`) or
    without a final xform, which has (`final_post`) a post affine or not, compiled with FL_HOIST_BUDGET = `budget`.
    `merge` is that of the BINNED kernels (the atomic ones never merge)."""
    resident = nxf <= 4 and 9 * nxf + 6 * posts <= 48
    col = resident and nxf + 2 <= budget
    aff = col and 3 * nxf + 2 <= budget
    post = aff and 3 * nxf + 2 + 2 * posts <= budget
    hfinal = bool(final) and budget >= 7
    tab = (not resident) and budget >= 12 and nxf <= 16 and not chaos
    split = nxf <= 9
    return dict(resident=resident, col=col, aff=aff, post=post, final=hfinal, final_post=hfinal and bool(final_post),
                tab=tab, plain=not resident and not tab, split_fuse=split, merge=split and nxf <= MERGE_MAX_XF and not chaos,
                cam=budget >= 2)


# ------------------------------------------------------------------------------------------------ genomes
def _post(i):
    return configs._affine(4.0 + 3.0 * i, 0.93 + 0.01 * (i % 4), 0.05 - 0.02 * (i % 3), -0.04 + 0.015 * (i % 5))


def ring(n, posts=(), final=None, scale=None, mag=None, bent=0.15, off=1.0, center=None):
    """nxf_flame's ring of n xforms at 256 x 144, with per-xform colour speeds, a little `bent` beside `linear`, post affines on
    the xforms numbered in `posts` (positions in the packer's key order) and a final xform: None, 'plain' or 'post'.
    `mag`: the ring's contraction (nxf_flame: 0.45).  One or two strongly contracting maps put everything on a few cells:
    rows of few xforms use weak contractions so that no cell fills up and the packed cells themselves can be compared (`off` scales
    the ring's radius: the fixed point of one weak contraction lies at offset / (1 - mag))."""
    gnm, prof = nxf_flame(n)
    gnm = copy.deepcopy(gnm)
    keys = sorted(gnm['xforms'])
    for i, k in enumerate(keys):
        xf = gnm['xforms'][k]
        xf['color'] = (i + 0.35) / n
        xf['color_speed'] = 0.25 + 0.5 * (i + 1) / (n + 1)
        xf['variations'] = {'linear': {'weight': 1.0 - bent}, 'bent': {'weight': bent}}
        if mag is not None:
            xf['pre_affine']['magnitude'] = {'x': mag, 'y': mag * 0.96}
        xf['pre_affine']['offset'] = {'x': xf['pre_affine']['offset']['x'] * off, 'y': xf['pre_affine']['offset']['y'] * off + 0.02 * off}
        if i in posts:
            xf['post_affine'] = _post(i)
    assert all(p < n for p in posts)
    if final:
        gnm['final_xform'] = {'color': 0.3, 'color_speed': 0.2, 'pre_affine': configs._affine(-8.0, 0.97, 0.02, 0.01),
                              'variations': {'linear': {'weight': 0.9}, 'bent': {'weight': 0.1}}}
        if final == 'post':
            gnm['final_xform']['post_affine'] = configs._affine(6.0, 1.03, -0.03, 0.02)
    if scale is not None:
        gnm['camera']['scale'] = scale
    if center is not None:
        gnm['camera']['center'] = {'x': center[0], 'y': center[1]}
    return gnm, prof


class Row(object):
    def __init__(self, name, nxf, posts, final, expect, build, kind='oracle'):
        self.name, self.nxf, self.posts, self.final, self.build, self.kind = name, nxf, tuple(posts), final, build, kind
        self.form = form_of(nxf, len(self.posts), final is not None, final == 'post')
        # the form the row is MEANT to reach, stated beside it: a slip in the row (or in form_of) shows here, without a compiler
        want = dict(resident=False, col=False, aff=False, post=False, final=False, final_post=False, tab=False, plain=False,
                    split_fuse=nxf <= 9, merge=nxf <= 4, cam=True)
        want.update(dict((k, True) for k in expect.split()))
        assert self.form == want, (name, self.form, want)

    def modes(self):
        """accumulate modes of the oracle comparison: one or two contracting maps wrap the packed count in atomic mode
        (test_gpu_edges.test_xform_counts_bit_exact), those rows run binned only"""
        return (1,) if self.nxf <= 2 else (0, 1)

    def genome(self):
        return self.build()

    def __repr__(self):
        return self.name


def _row(name, n, posts, final, expect, **kw):
    return Row(name, n, posts, final, expect, lambda: ring(n, posts, final, **kw))


ORACLE_ROWS = [
    # (one weak contraction: with its post affine a cloud that shrinks by 0.96 x 0.92 a round around the map's fixed point, where the camera looks, zoomed in)
    _row('n1_post_finalpost', 1, (0,), 'post', 'resident col aff post final final_post', mag=1.03, bent=0.05, off=0.06, scale=1.5, center=(1.224, -0.404)),
    _row('n2_posts2', 2, (0, 1), None, 'resident col aff post', mag=0.93, scale=0.3),
    _row('n2_posts2_final', 2, (0, 1), 'plain', 'resident col aff post final', mag=0.93, scale=0.3),
    _row('n3', 3, (), None, 'resident col aff post', mag=0.8, scale=0.32),                # aff at 11; no post affine: kHoistPost holds vacuously
    _row('n3_post1', 3, (1,), None, 'resident col aff', mag=0.8, scale=0.32),            # 13 > 12: the post offsets come from the head
    _row('n4', 4, (), None, 'resident col', mag=0.75, scale=0.4),
    _row('n4_posts2', 4, (0, 2), None, 'resident col', mag=0.75, scale=0.4),            # 48 SGPRs: the last resident structure
    _row('n4_posts3', 4, (0, 1, 3), None, 'tab', mag=0.75, scale=0.4),                  # 54: records per round, table + merge
    _row('n4_posts3_finalpost', 4, (0, 1, 3), 'post', 'tab final final_post', mag=0.75, scale=0.4),
    _row('n5', 5, (2,), None, 'tab', mag=0.7, scale=0.4),
    _row('n9_post', 9, (0, 4, 8), None, 'tab', mag=0.6, scale=0.4),
    _row('n10_post', 10, (1, 5, 9), None, 'tab', mag=0.6, scale=0.4),
    _row('n16', 16, (3,), None, 'tab', mag=0.55, scale=0.4),
    _row('n17', 17, (16,), None, 'plain', mag=0.55, scale=0.4),
    _row('n17_final', 17, (0,), 'plain', 'plain final', mag=0.55, scale=0.4),
]


# ---- rows held to the interpreter kernel: parametric variations, whose parameters come through XfTail / VTail
def _lazysusan(i):
    return {'weight': 0.3, 'x': 0.1 + 0.02 * i, 'y': -0.12 + 0.03 * i, 'twist': 0.4 + 0.05 * i, 'space': 0.2 - 0.01 * i, 'spin': 0.7 + 0.1 * i}


def _mobius(i):
    return {'weight': 0.6, 're_a': 1.0, 'im_a': 0.05 * (i + 1), 're_b': 0.1 - 0.02 * i, 'im_b': 0.03 * i, 're_c': 0.04 * (i % 3), 'im_c': -0.05,
            're_d': 1.1, 'im_d': 0.02 * i}


def tail_ring(n, which, final=None, mag=0.6, scale=0.25):
    """`which` 'cross27': every xform is bent + lazysusan — the five-parameter variation SECOND in its record, at var_stride 7 its
    parameters are words 25..29, of which 25..27 are in the tail's registers and 28, 29 in memory.  'mobius': var_stride 10;
    even xforms mobius alone (parameters 18..25, all in the tail), odd ones linear + mobius (weight in word 27, parameters 28..35)."""
    gnm, prof = ring(n, posts=(0,), final=final, mag=mag, scale=scale)
    for i, k in enumerate(sorted(gnm['xforms'])):
        if which == 'cross27':
            gnm['xforms'][k]['variations'] = {'bent': {'weight': 0.7}, 'lazysusan': _lazysusan(i)}
        else:
            gnm['xforms'][k]['variations'] = {'mobius': _mobius(i)} if i % 2 == 0 else {'linear': {'weight': 0.4}, 'mobius': _mobius(i)}
    if final:
        gnm['final_xform']['variations'] = {'bent': {'weight': 0.8}, 'lazysusan': _lazysusan(7)} if which == 'cross27' else {'linear': {'weight': 0.5}, 'mobius': _mobius(2)}
    return gnm, prof


def _irow(name, n, which, expect, final=None, **kw):
    return Row(name, n, (0,), final, expect, lambda: tail_ring(n, which, final, **kw), kind='interp')


# (contractions and cameras chosen with the oracle: every launch keeps well over 100000 samples in the frame)
INTERP_ROWS = [
    _irow('cross27_n2', 2, 'cross27', 'resident col aff post', mag=0.5, scale=0.9),
    _irow('cross27_n5', 5, 'cross27', 'tab', mag=0.6, scale=0.35),
    _irow('cross27_n17', 17, 'cross27', 'plain', mag=0.6, scale=0.5),
    _irow('mobius_n2', 2, 'mobius', 'resident col aff post', mag=1.1, scale=0.5),
    _irow('mobius_n5', 5, 'mobius', 'tab', mag=1.0, scale=0.6),
    _irow('mobius_n17', 17, 'mobius', 'plain', mag=0.9, scale=0.6),
    _irow('tfin_n3_final_cross27', 3, 'cross27', 'resident col aff final', final='plain', mag=0.5, scale=0.3),
]

ROWS = ORACLE_ROWS + INTERP_ROWS
BY_NAME = dict((r.name, r) for r in ROWS)
assert len(BY_NAME) == len(ROWS)

# The rows whose form a fallback budget changes, and what each budget makes of them (tests/test_gpu_iter_forms.py runs one child
# process per budget: rtc.hip's module cache is not keyed by FLAME_RTC_FLAGS).
BUDGET_ROWS = ('n1_post_finalpost', 'n3', 'n4_posts3', 'n5')
BUDGET_EXPECT = {
    ('n1_post_finalpost', 7): 'resident col aff post final final_post cam',
    ('n1_post_finalpost', 5): 'resident col aff cam',
    ('n1_post_finalpost', 0): 'resident',
    ('n3', 7): 'resident col cam', ('n3', 5): 'resident col cam', ('n3', 0): 'resident',
    ('n4_posts3', 7): 'plain cam', ('n4_posts3', 5): 'plain cam', ('n4_posts3', 0): 'plain',
    ('n5', 7): 'plain cam', ('n5', 5): 'plain cam', ('n5', 0): 'plain',
}


def budget_form(name, budget):
    r = BY_NAME[name]
    return form_of(r.nxf, len(r.posts), r.final is not None, r.final == 'post', budget=budget)


def _check_budget_rows():
    for (name, b), expect in BUDGET_EXPECT.items():
        f = budget_form(name, b)
        got = set(k for k in ('resident', 'col', 'aff', 'post', 'final', 'final_post', 'tab', 'plain', 'cam') if f[k])
        assert got == set(expect.split()), (name, b, sorted(got))
    assert set(BUDGET_EXPECT) == set(itertools.product(BUDGET_ROWS, BUDGETS[1:]))
    # every budget changes the form of its rows (but for the one xform that fits seven registers whole)
    same = [(n, b) for n, b in BUDGET_EXPECT if budget_form(n, b) == BY_NAME[n].form]
    assert same == [('n1_post_finalpost', 7)], same


def _check_coverage():
    """The rows together reach every value of every predicate, and both sides of every threshold of DESIGN.md's table."""
    forms = [r.form for r in ROWS] + [budget_form(n, b) for n, b in BUDGET_EXPECT]
    for key in forms[0]:
        assert set(f[key] for f in forms) == {False, True}, key
    have = set((r.nxf, len(r.posts), r.final) for r in ORACLE_ROWS)
    nxfs = set(r.nxf for r in ORACLE_ROWS)
    # (xforms, posts) pairs on both sides: residency at 48 SGPRs; kHoistPost held at (1, 1) and (2, 2), lost at (3, 1); kHoistAff lost at 4
    for n, p in ((4, 2), (4, 3), (1, 1), (2, 2), (3, 0), (3, 1), (4, 0)):
        assert any(h[:2] == (n, p) for h in have), (n, p)
    assert BY_NAME['n4_posts2'].form['resident'] and not BY_NAME['n4_posts3'].form['resident']
    assert BY_NAME['n2_posts2'].form['post'] and not BY_NAME['n3_post1'].form['post'] and BY_NAME['n3_post1'].form['aff']
    assert BY_NAME['n3'].form['aff'] and not BY_NAME['n4'].form['aff'] and BY_NAME['n4'].form['col']
    assert {4, 5} <= nxfs and {9, 10} <= nxfs and {16, 17} <= nxfs             # MERGE, SPLIT_FUSE, kTab
    assert form_of(9, 0, 0, 0)['split_fuse'] and not form_of(10, 0, 0, 0)['split_fuse']
    assert form_of(16, 0, 0, 0)['tab'] and form_of(17, 0, 0, 0)['plain']
    # tab together with merge, with and without a final xform; a plain row with a final xform; final with and without its post
    assert all(BY_NAME[n].form['tab'] and BY_NAME[n].form['merge'] for n in ('n4_posts3', 'n4_posts3_finalpost'))
    assert BY_NAME['n5'].form['tab'] and not BY_NAME['n5'].form['merge']
    assert BY_NAME['n17_final'].form['plain'] and BY_NAME['n17_final'].form['final']
    assert BY_NAME['n2_posts2_final'].form['final'] and not BY_NAME['n2_posts2_final'].form['final_post']
    assert any(9 <= r.nxf <= 10 and r.posts for r in ORACLE_ROWS)
    # the budgets: 7 keeps the final xform and loses the table, 5 loses the final xform, 0 the camera's registers as well
    assert budget_form('n1_post_finalpost', 7)['final'] and not budget_form('n1_post_finalpost', 5)['final']
    assert budget_form('n4_posts3', 7)['plain'] and budget_form('n4_posts3', 7)['merge']
    assert budget_form('n5', 7)['plain'] and budget_form('n5', 7)['split_fuse']
    # the interpreter-held rows: each parameter layout in resident, table and plain form, and a hoisted final xform's tail
    for which in ('cross27', 'mobius'):
        fs = [r.form for r in INTERP_ROWS if r.name.startswith(which)]
        assert any(f['resident'] for f in fs) and any(f['tab'] for f in fs) and any(f['plain'] for f in fs)
    assert BY_NAME['tfin_n3_final_cross27'].form['final']


_check_budget_rows()
_check_coverage()


# ------------------------------------------------------------------------------------------------ the GPU comparisons
# Three launches of 7 plotted rounds, the first behind 3 fuse rounds: they start at rounds 0, 10 and 17, i.e. at swap phases 0, 1
# and 2 — the three-copy round loop (ROT3) is entered with each of the three destinations first, the rotating form mid-cycle.
NROUNDS, FUSE, LAUNCHES, NSLOTS = 7, 3, 3, 1024
MIN_ACCEPTED = 100000


def check_oracle_row(mgr, row, mode):
    """One row in one accumulate mode on `mgr` (1024 four-wave slots) against the oracle's device model, launch by launch:
    counters, density, packed cells (no cell fills up in these rows: asserted, not assumed), flags, colour; RNG and walkers at
    the end.  Returns the accepted samples per launch."""
    gnm, prof = row.genome()
    res, ref_state, dev_state, dim, _ = run_device_model(mgr, gnm, prof, nrounds=NROUNDS, fuse=FUSE, launches=LAUNCHES, mode=mode)
    assert len(res) == LAUNCHES
    for k, r in enumerate(res):
        tag = (row.name, mode, k)
        assert np.array_equal(r['ctr_dev'][:3], r['ctr_ref'][:3]), (tag, r['ctr_dev'], r['ctr_ref'])
        assert int(r['ctr_dev'][0]) > MIN_ACCEPTED, (tag, r['ctr_dev'])
        assert np.array_equal(r['front_dev'][:, 3], r['front_ref'][:, 3]), (tag, int((r['front_dev'][:, 3] != r['front_ref'][:, 3]).sum()))
        # neither side drained a cell (the camera scales see to it: tests/test_cpu_iter_forms.py holds the oracle alone to this) ...
        assert int(r['ctr_dev'][3]) == 0 and int(r['ctr_ref'][3]) == 0, (tag, r['ctr_dev'], r['ctr_ref'])
        assert int((r['atom_ref'] >> np.uint64(54)).max()) < 256, tag
        # ... so the packed cells themselves are compared, everywhere
        bad = np.nonzero(r['atom_dev'] != r['atom_ref'])[0]
        assert bad.size == 0, (tag, bad.size, int(bad[0]), hex(int(r['atom_dev'][bad[0]])), hex(int(r['atom_ref'][bad[0]])))
        assert int((r['atom_dev'] >> np.uint64(54)).sum()) == int(r['ctr_dev'][0]), tag
        assert np.array_equal(r['hot_dev'], r['hot_ref']), tag
        np.testing.assert_allclose(r['front_dev'][:, :3], r['front_ref'][:, :3], rtol=5e-5, atol=1e-3)      # the bar of test_xform_counts_bit_exact
    bad = np.nonzero((dev_state[0] != ref_state[0]).any(1))[0]
    assert bad.size == 0, (row.name, mode, 'rng', bad.size, int(bad[0]))
    a, b = dev_state[1][:, :3].view(np.uint32), ref_state[1][:, :3].view(np.uint32)
    bad = np.nonzero((a != b).any(1))[0]
    assert bad.size == 0, (row.name, mode, 'walker', bad.size, int(bad[0]), dev_state[1][bad[0]], ref_state[1][bad[0]])
    return [int(r['ctr_dev'][0]) for r in res]


def animated(gnm, prof):
    """The genome in motion over a frame window that spans the animation: every xform's offset and colour and the camera move, so
    every temporal sample has its own parameter block — its own resident records, its own operand table."""
    gnm = copy.deepcopy(gnm)
    for i, k in enumerate(sorted(gnm['xforms'])):
        xf = gnm['xforms'][k]
        ox, c = xf['pre_affine']['offset']['x'], xf['color']
        xf['pre_affine']['offset']['x'] = [ox, 0.15, ox + 0.15 - 0.05 * (i % 3), 0.15]
        xf['color'] = [c, -0.1, c - 0.1, -0.1]
    cx = gnm['camera']['center']['x']
    gnm['camera']['center'] = dict(gnm['camera']['center'], x=[cx - 0.05, 0.1, cx + 0.05, 0.1])
    gnm['time'] = {'duration': 1, 'frame_width': 1.0}
    return gnm, dict(prof, frame_width=1.0, fps=1, duration=1)


def gpu_launches(m, gnm, prof, mode, seeds_in=None):
    """The same three launches on the device alone; `seeds_in`: RNG states to start from (written before the palette is made).
    Returns per launch the counters, the packed cells and the flushed accumulator, and at the end RNG states and walker points."""
    from cuburn_amd import _lib
    lib = _lib.load()
    if seeds_in is not None:
        m.fb.write('seeds', seeds_in)
    seeds0 = m.fb.read('seeds', (m.fb.nwalkers, 3), np.uint32)
    rdr, gprof, dim, g, ts, td = setup_frame(m, gnm, prof)
    nbins, nwalk = dim.ah * dim.astride, m.fb.nslots * m.fb.nthreads
    _lib.check(lib.fl_debug_clear(m.fb.ctx, dim.w, dim.h, 1))
    out = dict(ctr=[], atom=[], front=[], seeds0=seeds0)
    r0 = 0
    for k in range(LAUNCHES):
        f = FUSE if k == 0 else 0
        _lib.check(lib.fl_debug_iter_launch(m.fb.ctx, g, dim.w, dim.h, r0, NROUNDS + f, f, mode))
        ctr = np.zeros(4, np.uint64)
        _lib.check(lib.fl_debug_counters(m.fb.ctx, ctr.ctypes.data))
        out['ctr'].append(ctr)
        out['atom'].append(m.fb.read('atom', (nbins,), np.uint64))
        if mode == 1:                       # binned mode never thins: no flags are kept (as run_device_model)
            _lib.check(lib.fl_debug_clear_hot(m.fb.ctx, dim.w, dim.h))
        _lib.check(lib.fl_debug_flush(m.fb.ctx, dim.w, dim.h))
        if mode == 1:
            _lib.check(lib.fl_debug_clear_hot(m.fb.ctx, dim.w, dim.h))
        out['front'].append(m.fb.read('front', (nbins, 4), np.float32))
        r0 += NROUNDS + f
    out['rng'] = m.fb.read('seeds', (m.fb.nwalkers, 3), np.uint32)[:nwalk]
    out['pts'] = m.fb.read('points', (nwalk, 4), np.float32)
    return out


def defines(form):
    """the probe's -DEXP_* options for a form"""
    return ['-DEXP_%s=%d' % (k.upper(), int(form[k])) for k in PROBED]
