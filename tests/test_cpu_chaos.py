"""
Xform chaos (flam3 xaos) on the host side (no GPU): the canonical form (an all-ones table is the keyless genome), the layout of
a chaos genome (include/flame_hip.h (5) prog[8], (6) FL_OP_CHAOS_CDF), the front end (genome/store.py moves a node's table onto
its animation), the Renderer's rejections and warnings, the per-genome kernels of chaos genomes (hipRTC compiles without a
device), and the bars of tests/test_gpu_chaos.py held against the model of tests/chaos_model.py itself.
"""
import copy
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest

from common import prepare
from cuburn_amd import _lib, configs, profile, render
from cuburn_amd.genome import blend, store
from cuburn_amd.packer import GenomePacker, OP_CDF, OP_CHAOS_CDF, PROG_MAGIC
import chaos_model as X
from flames import FRACTIONAL, FORBIDDEN, CYCLE, many_xforms, rich_xml
from gpu_harness import pack_digest, compile_check as _compile, kernel_resources as _resources

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def const_inputs(table, weights=X.WEIGHTS):
    """Weights (1, n) and entries (1, n, n) of a constant table as the op sees them (float32 knots)."""
    w = np.array([weights], np.float32)
    c = np.array([[[1.0 if v is None else v for v in row] for row in table]], np.float32)
    return w, c


# ------------------------------------------------------------------ canonical form
@pytest.mark.parametrize('ones', [1, 1.0, [1.0, 1.0], [1.0, 0.0, 1.0, 0.0], [1.0, 0.0, 1.0, 0.0, 0.25, 1.0, 0.5, 1.0]],
                         ids=['int', 'float', 'two-values', 'with-velocities', 'interior-knots'])
def test_all_ones_table_packs_as_the_keyless_genome(ones):
    keyless = X.nine_boxes()[0]
    for table in ([[ones] * 3] * 3, [[ones, None, None], [None, None, None], [None, ones, None]]):
        gnm = X.nine_boxes(table)[0]
        assert any('chaos' in xf for xf in gnm['xforms'].values())
        a, b = GenomePacker(keyless), GenomePacker(gnm)
        assert len(b.prog) == 8 and np.array_equal(a.prog, b.prog)
        assert np.array_equal(a.ops_array, b.ops_array)
        assert a.rows == b.rows and a.packed == b.packed and a.pstride == b.pstride
        assert pack_digest(a) == pack_digest(b)
        ta, ka = a.pack(keyless)
        tb, kb = b.pack(gnm)
        assert np.array_equal(ta, tb) and np.array_equal(ka, kb)
    cfg2 = configs.cfg2()[0]
    ones2 = copy.deepcopy(cfg2)
    for k in ones2['xforms']:
        ones2['xforms'][k]['chaos'] = dict((n, ones) for n in ones2['xforms'])
    assert pack_digest(GenomePacker(ones2)) == pack_digest(GenomePacker(cfg2))


# ------------------------------------------------------------------ layout
def test_chaos_genome_layout():
    keyless = X.nine_boxes()[0]
    table = [[1.0, 0.5, None], [None, None, None], [[0.0, 1.0], 3.0, -1.0]]
    gnm = X.nine_boxes(table)[0]
    a, b = GenomePacker(keyless), GenomePacker(gnm)
    n = 3
    assert len(b.prog) == 9 and b.prog[0] == PROG_MAGIC
    assert np.array_equal(b.prog[[0, 1, 2, 4, 5, 6, 7]], a.prog[[0, 1, 2, 4, 5, 6, 7]])          # every keyless offset keeps its value
    chaos_off = int(b.prog[8])
    assert chaos_off == a.pstride == int(a.prog[5]) + n * int(a.prog[6])                      # behind the last record
    assert b.pstride == int(b.prog[3]) == chaos_off + n * n
    assert b.packed[:a.pstride] == a.packed
    assert b.packed[chaos_off:] == [('chaos', str(p), str(k)) for p in range(n) for k in range(n)]
    # the keyless ops and rows come first, unchanged; then one chaos op per prior, its rows consecutive in key order
    assert np.array_equal(b.ops_array[:len(a.ops_array)], a.ops_array) and b.rows[:a.nrows] == a.rows
    extra = b.ops_array[len(a.ops_array):]
    cdf = [o for o in a.ops_array if o[0] == OP_CDF][0]
    assert len(extra) == n
    for p, o in enumerate(extra):
        first = a.nrows + p * n
        assert o.tolist() == [OP_CHAOS_CDF, chaos_off + p * n, int(cdf[2]), n | (first << 8)]
        assert [path for path, mag in b.rows[first:first + n]] == [('xforms', str(p), 'chaos', str(k)) for k in range(n)]
        assert not any(mag for _, mag in b.rows[first:first + n])                             # linear-domain splines
    assert b.nrows == a.nrows + n * n
    # missing entries are rows of the constant 1
    times, knots = b.pack(gnm)
    for p in range(n):
        for k in range(n):
            row = a.nrows + p * n + k
            real = times[row] < 1e8
            if table[p][k] is None:
                assert (knots[row][real] == 1.0).all() and real.sum() >= 2, (p, k)
            elif not isinstance(table[p][k], list):
                assert (knots[row][real] == np.float32(table[p][k])).all(), (p, k)
    assert set(knots[a.nrows + 2 * n][times[a.nrows + 2 * n] < 1e8]) == {0.0, 1.0}             # the animated entry keeps its knots
    # a keyless genome of the same structure still has 8 words
    assert len(a.prog) == 8


def test_one_entry_off_one_makes_a_chaos_genome():
    for v in (0.0, 0.999, 2, [1.0, 0.1], [0.0, 1.0, 1.0, 0.5]):
        pk = GenomePacker(X.nine_boxes([[None, None, None], [None, v, None], [None, None, None]])[0])
        assert len(pk.prog) == 9 and (pk.ops_array[:, 0] == OP_CHAOS_CDF).sum() == 3, v


# ------------------------------------------------------------------ rejections and warnings


def test_renderer_rejects_33_xforms_with_chaos_only():
    for n, chaos, ok in ((32, True, True), (33, False, True), (33, True, False)):
        gnm, prof = many_xforms(n, chaos)
        gprof = profile.wrap(prof, gnm)
        if ok:
            rdr = render.Renderer(gnm, gprof)
            assert len(rdr.packer.prog) == (9 if chaos else 8)
        else:
            with pytest.raises(ValueError, match='chaos'):
                render.Renderer(gnm, gprof)


def test_renderer_warns_about_unknown_targets_and_final_chaos():
    gnm, prof = X.nine_boxes(FRACTIONAL)
    gprof = profile.wrap(prof, gnm)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        ref = render.Renderer(gnm, gprof).packer                                               # a well-formed table: silence
    bad = copy.deepcopy(gnm)
    bad['xforms']['1']['chaos']['7'] = 0.0
    with pytest.warns(UserWarning, match='names no xform'):
        pk = render.Renderer(bad, gprof).packer
    assert pack_digest(pk) == pack_digest(ref)                                                 # ... and ignored
    fin = copy.deepcopy(gnm)
    fin['final_xform'] = dict(copy.deepcopy(gnm['xforms']['0']), chaos={'0': 0.5})
    nofin = copy.deepcopy(fin)
    del nofin['final_xform']['chaos']
    with pytest.warns(UserWarning, match='final_xform.chaos'):
        pk = render.Renderer(fin, gprof).packer
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert pack_digest(pk) == pack_digest(render.Renderer(nofin, gprof).packer)


# ------------------------------------------------------------------ front end


def test_flam3_file_with_chaos_becomes_an_animation_that_carries_the_table(tmp_path):
    path = tmp_path / 'rich.flam3'
    path.write_text(rich_xml())
    with pytest.warns(UserWarning, match='flames in file'):
        gnm, base = store.connect(str(tmp_path)).animation(str(path))
    assert base == 'rich' and gnm['type'] == 'animation'
    assert sorted(gnm['xforms']) == ['0_0', '1_1', '2_2']
    assert gnm['xforms']['0_0']['chaos'] == {'0_0': 1.0, '1_1': 0.5, '2_2': 2.0}
    assert 'chaos' not in gnm['xforms']['1_1'] and 'chaos' not in gnm['xforms']['2_2']
    pk = GenomePacker(gnm)
    assert len(pk.prog) == 9 and (pk.ops_array[:, 0] == OP_CHAOS_CDF).sum() == 3
    # without the attribute: the same animation but for the table, and a keyless program
    (tmp_path / 'plain.flam3').write_text(rich_xml().replace(' chaos="1 0.5 2"', ''))
    with pytest.warns(UserWarning, match='flames in file'):
        plain, _ = store.connect(str(tmp_path)).animation(str(tmp_path / 'plain.flam3'))
    del gnm['xforms']['0_0']['chaos']
    assert gnm == plain and len(GenomePacker(plain).prog) == 8


def test_store_node_and_edge(tmp_path):
    from cuburn_amd.genome import convert
    node = convert.flam3_to_node(convert.XMLGenomeParser.parse(rich_xml())[0])
    assert node['xforms']['0']['chaos'] == {'0': 1.0, '1': 0.5, '2': 2.0}
    keep = copy.deepcopy(node)
    (tmp_path / 'a.json').write_text(json.dumps(node))
    (tmp_path / 'b.json').write_text(json.dumps(node))
    edge = {'type': 'edge', 'link': {'src': 'a', 'dst': 'b'}, 'blend': {'duration': 2}}
    (tmp_path / 'e.json').write_text(json.dumps(edge))
    db = store.connect(str(tmp_path))
    gnm, _ = db.animation('a')
    assert gnm['xforms']['0_0']['chaos'] == {'0_0': 1.0, '1_1': 0.5, '2_2': 2.0}
    with pytest.warns(UserWarning, match='chaos'):
        anim, _ = db.animation('e')
    assert anim['type'] == 'animation' and not any('chaos' in xf for xf in anim['xforms'].values())
    assert len(GenomePacker(anim).prog) == 8
    assert node == keep                                                                         # the caller's document is not edited


# ------------------------------------------------------------------ the per-genome kernels
@pytest.mark.parametrize('which', ['nine_boxes', 'cfg2', 'cfg5'])
def test_chaos_kernels_compile_within_budget(built, tmp_path, monkeypatch, which):
    """Chaos genomes compile for the walker geometries and accumulate modes of test_per_genome_kernel_compiles; the 4-wave binned
    kernel has no scratch, no spills, no static LDS and at most 96 vector registers (five 28 KB workgroups per CU)."""
    monkeypatch.delenv('FLAME_RTC_FLAGS', raising=False)
    if which == 'nine_boxes':
        gnm = X.nine_boxes(FRACTIONAL)[0]
    else:
        gnm = configs.CONFIGS[which]()[0]
        keys = sorted(gnm['xforms'])
        gnm['xforms'][keys[0]]['chaos'] = {keys[0]: 0.0, keys[1]: 1.5}
        gnm['xforms'][keys[-1]]['opacity'] = 0.5
    for nw, count, acc in ((4, 1, 0), (8, 0, 3), (16, 3, 1)):
        rc, log = _compile(gnm, nw, count, acc)
        assert rc == 0, log[:3000]
    monkeypatch.setenv('FLAME_RTC_DUMP', str(tmp_path))
    rc, log = _compile(gnm, 4, 0, 1)
    assert rc == 0, log[:3000]
    assert '#define FL_SPEC_CHAOS 1' in open(str(tmp_path / 'flame_spec.h')).read()
    r = _resources(tmp_path)
    print(which, r)
    assert r['vgpr'] <= 96 and r['spill'] == 0 and r['scratch'] == 0 and r['lds'] == 0, r


def test_compile_check_rejects_bad_chaos_programs(built):
    """(fl_genome_create's rejections need a context: tests/test_gpu_chaos.py.)"""
    pk = GenomePacker(X.nine_boxes(FRACTIONAL)[0])
    ops = np.ascontiguousarray(pk.ops_array, np.int32)
    log = C.create_string_buffer(4096)

    def check(prog):
        prog = np.ascontiguousarray(prog, np.int32)
        return _lib.load().fl_rtc_compile_check(prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), 4, 0, 1, log, len(log))
    rc = check(pk.prog)
    if rc == _lib.FL_E_UNSUPPORTED:
        pytest.skip('libhiprtc is not installed')
    assert rc == 0
    for off in (-1, 0, int(pk.prog[5]), int(pk.prog[8]) - 1, int(pk.prog[3]) - 8, int(pk.prog[3]), 1 << 30):
        bad = pk.prog.copy(); bad[8] = off
        assert check(bad) == _lib.FL_E_INVAL, off


# ------------------------------------------------------------------ the bars are sane without a GPU
def test_float32_restatement_of_the_op_against_float64():
    rng = np.random.default_rng(5)
    for n in (2, 3, 32):
        w = rng.uniform(0.05, 2.0, (64, n)).astype(np.float32)
        c = rng.uniform(-0.5, 3.0, (64, n, n)).astype(np.float32)
        c[:8, 0, :] = 0.0                      # rows of zeros: the fallback
        c[8:16] = np.abs(c[8:16]) + np.float32(0.125)
        c[8:16, :, 1] = 0.0                    # a zero column (its rows keep a permitted successor)
        w[16:24, n - 1] = 0.0                  # a weight of 0
        a, b = X.cdf64(w, c), X.cdf32(w, c)
        assert (b[..., -1] == 2.0).all() and (a[..., -1] == 2.0).all()
        dev = np.abs(a[..., :-1] - b[..., :-1].astype(np.float64)).max()
        # n products, n adds, one reciprocal, and per word a product and an add, each half an ulp of a value <= 1
        assert dev <= (2 * n + 3) * 2.0 ** -24, (n, dev * 2.0 ** 24)
        assert (np.diff(b[..., :-1].astype(np.float64), axis=-1) >= 0).all()
        plain = X.cdf64(w, np.ones_like(c))
        assert np.array_equal(a[:8, 0], plain[:8, 0])                                            # the fallback is the plain row
        if n >= 3:
            assert np.array_equal(a[8:16, :, 1], a[8:16, :, 0]) and np.array_equal(b[8:16, :, 1], b[8:16, :, 0])      # nothing leads to xform 1
    w, c = const_inputs([[1, 1, 1]] * 3)
    assert np.array_equal(X.cdf32(w, c)[0, 1], X.cdf32(w, c)[0, 0])
    # all-ones rows are FL_OP_CDF's own row, bit for bit (the same operations on the same values)
    s = np.float32(0)
    for k in range(3):
        s = s + w[0, k]
    r, run, row = np.float32(1) / s, np.float32(0), []
    for k in range(3):
        run = run + w[0, k] * r
        row.append(run)
    assert np.array_equal(np.array(row[:2], np.float32), X.cdf32(w, c)[0, 0, :2])


def test_pair_masses_of_a_known_chain():
    M = X.transition(X.cdf64(*const_inputs(CYCLE))[0])
    assert np.allclose(M, [[0, 1, 0], [0, 0, 1], [1, 0, 0]])
    assert np.allclose(X.stationary(M), 1 / 3.0)
    M = X.transition(X.cdf64(*const_inputs([[1, 1, 1]] * 3))[0])                                 # no chaos: independent draws
    assert np.allclose(X.pair_masses(M), np.outer(X.WEIGHTS, X.WEIGHTS)) and X.lambda2(M) < 1e-12
    M = X.transition(X.cdf64(*const_inputs(FRACTIONAL))[0])
    P = X.pair_masses(M)
    assert abs(P.sum() - 1) < 1e-12 and np.allclose(P.sum(0), P.sum(1))                          # stationarity: in = out


def test_nine_boxes_are_disjoint_and_the_model_meets_the_statistical_bar():
    """The geometry the GPU tests rest on, and the statistical bar of test_gpu_chaos.py held against the model itself: 2^22
    samples of the model's chaos game against the exact pair masses at 6 sigma per box."""
    keyless, prof = X.nine_boxes()
    F = prepare(keyless, prof)
    cam, aff = X.affines_of(F['params'][0], F['packer'].prog)
    dim = (F['dim'].ah, F['dim'].astride)
    first, second = X.box_rects(cam, aff)
    rects = list(second.values())
    for i, a in enumerate(rects):
        assert 0 <= a[0] and a[1] < dim[0] and 0 <= a[2] and a[3] < F['dim'].aw
        assert (a[1] - a[0] + 1, a[3] - a[2] + 1) in ((19, 19), (20, 20), (19, 20), (20, 19))     # 16 pixels + rounding + the margin
        for b in rects[i + 1:]:
            assert X.rect_gap(a, b) >= 8, (a, b)
    for (p, n), r in second.items():
        f = first[n]
        assert f[0] <= r[0] and r[1] <= f[1] and f[2] <= r[2] and r[3] <= f[3]
    table = FORBIDDEN
    w, c = const_inputs(table)
    rows = X.cdf64(w, c)[0]
    M = X.transition(rows)
    lam = X.lambda2(M)
    assert lam <= 0.5, lam
    exact = X.pair_masses(M)
    N = 2 ** 22
    hist = X.chaos_game(cam, aff, X.cdf64(w, np.ones_like(c))[0, 0], rows, 4096, N // 4096, 16, dim)
    assert hist.sum() == N                                                                       # everything in frame
    seen = 0
    for (p, n), r in second.items():
        got = int(X.in_rect(hist, r).sum())
        seen += got
        bar = 6 * X.sigma(N, exact[p, n], lam)
        if table[p][n] == 0:
            assert got == 0 and exact[p, n] == 0, (p, n)
        else:
            assert got > 0 and abs(got - N * exact[p, n]) <= bar, (p, n, got, N * exact[p, n], bar)
    assert seen == N                                                                             # and every sample in one of the nine boxes
