"""
Xform opacity on the host side (no GPU): what the packer emits for the `opacity` key, the plot-probability curve of
FL_OP_OPACITY in float32, and the per-genome iterate kernels of genomes with an opacity (hipRTC compiles without a
device).  The contract is include/flame_hip.h (5) words 14 / 15 and (6) FL_OP_OPACITY; DESIGN.md §4.1.

The "three boxes" test flame that tests/test_gpu_opacity.py renders too is in tests/flames.py.
"""
import copy
import ctypes as C
import json
import os
import re
import warnings

import numpy as np
import pytest

from cuburn_amd import _lib, configs, profile, render
from cuburn_amd.packer import GenomePacker, OP_CONST, OP_OPACITY, OP_SPLINE_MAG
from flames import three_boxes, with_opacity, plot_probability
from gpu_harness import pack_digest, compile_check as _compile, kernel_resources as _resources

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def plot_probability_f32(p):
    """csrc/interp.hip, case FL_OP_OPACITY, restated operation by operation in float32."""
    f = np.float32
    p = np.minimum(np.maximum(f(p), f(0)), f(1))
    with np.errstate(divide='ignore'):
        q = np.exp2(np.log2(p) * f(3.3219281))
    assert q.dtype == np.float32
    if q < f(2.3283064e-10):
        q = f(0)
    return f(0) if p <= f(0) else f(1) if p >= f(1) - f(1.0e-6) else q


def _consts(pk):
    return dict((int(o[1]), int(o[2])) for o in pk.ops_array if o[0] == OP_CONST)


# ------------------------------------------------------------------ 1. the packer
# sha256 (first 32 hex digits) of prog + ops_array + rows (path, magnitude flag) + packed names of the keyless configs, made with
# the packer of the commit before opacity existed (56035f0)
KEYLESS_PACKS = {'cfg1': 'cd519df5d228bc4f9d20826907b02a69', 'cfg2': 'a5b54a14e3b0f1eb3388fbf145f9fcee',
                 'cfg3': '64527c157a84760fa4cd02392cd84681', 'cfg5': '1dc894a6ef16badcbff93601eae748e0',
                 'allvars': 'a1b1251d2635c55c5fe8d21df77ec55c'}


@pytest.mark.parametrize('cfg', ['cfg1', 'cfg2', 'cfg3', 'cfg5', 'allvars'])
def test_keyless_genomes_pack_as_before(cfg):
    """No `opacity` key: program, ops, rows and block names bit for bit what the previous packer made (stored digests); and, spelt
    out, no op of kind 10, no bit 9 in any structure word, no name for word 15."""
    gnm, _ = (configs.allvars if cfg == 'allvars' else configs.CONFIGS[cfg])()
    pk = GenomePacker(gnm)
    assert pack_digest(pk) == KEYLESS_PACKS[cfg]
    assert not (pk.ops_array[:, 0] == OP_OPACITY).any() and pk.ops_array[:, 0].max() == OP_CONST
    p = pk.prog
    for i in range(p[1] + p[2]):
        rec = p[5] + i * p[6]
        assert _consts(pk)[rec + 14] >> 9 == 0
        assert pk.packed[rec + 15][0] == 'pad'
    assert not any('opacity' in path for path, _ in pk.rows)
    gold = json.load(open(os.path.join(GOLD, 'packer.json')))
    if cfg in gold:
        assert set(gold[cfg]['rows']) <= set('.'.join(path) for path, _ in pk.rows)
    # and the digest does see the key
    marked = copy.deepcopy(gnm)
    marked['xforms'][sorted(marked['xforms'])[0]]['opacity'] = 1.0
    assert pack_digest(GenomePacker(marked)) != KEYLESS_PACKS[cfg]


def test_packer_opacity_rows_ops_and_flags():
    """`opacity` on xforms 0 and 2 only (and on the final xform, where it is ignored): one extra magnitude row per such
    xform, one FL_OP_OPACITY with dst = record + 15, bit 9 in exactly those structure words."""
    base, prof = configs.cfg3()
    gnm = with_opacity(base, ['0', '2'])
    gnm['xforms']['2']['opacity'] = [1.0, 0.0, 0.2, 0.0]                  # animated: still one row
    gnm['final_xform']['opacity'] = 0.3
    pk0, pk = GenomePacker(base), GenomePacker(gnm)
    assert OP_OPACITY == _lib.FL_OP_OPACITY == 10
    assert pk.nrows == pk0.nrows + 2 and len(pk.ops) == len(pk0.ops) + 2 and pk.pstride == pk0.pstride
    assert np.array_equal(pk.prog, pk0.prog)
    new_rows = [(path, mag) for path, mag in pk.rows if path not in [r for r, _ in pk0.rows]]
    assert new_rows == [(('xforms', '0', 'opacity'), True), (('xforms', '2', 'opacity'), True)]
    p, c, c0 = pk.prog, _consts(pk), _consts(pk0)
    opac = dict((int(o[1]), int(o[2])) for o in pk.ops_array if o[0] == OP_OPACITY)
    for i in range(p[1] + p[2]):
        rec = p[5] + i * p[6]
        marked = i in (0, 2)
        assert c[rec + 14] == c0[rec + 14] | (0x200 if marked else 0)
        assert (rec + 15 in opac) == marked
        if marked:
            path, mag = pk.rows[opac[rec + 15]]
            assert path == ('xforms', str(i), 'opacity') and mag
            assert pk.packed[rec + 15] == ('xforms', str(i), '#plot_probability')
        else:
            assert pk.packed[rec + 15][0] == 'pad'
    assert len(opac) == 2
    # everything else is what the keyless genome packs to
    def named(k):          # ops with their rows by path (an opacity row shifts the numbers of the rows behind it)
        out = []
        for kind, dst, a, b in k.ops_array.tolist():
            if kind == OP_OPACITY or (kind == OP_CONST and (dst - p[5]) % p[6] == 14):
                continue
            out.append((kind, dst, a if kind == OP_CONST else k.rows[a][0], k.rows[b][0] if kind in (5, 7) else b))
        return out
    assert named(pk) == named(pk0)
    times, knots = pk.pack(gnm)
    r = opac[p[5] + 2 * p[6] + 15]
    assert knots[r, :4].tolist() != [0, 0, 0, 0] and (times[r] < 1e8).sum() >= 2
    r = opac[p[5] + 15]
    assert (times[r] < 1e8).sum() >= 1 and np.float32(0.5) in knots[r]


def test_final_xform_opacity_warns_once_per_renderer():
    base, prof = configs.cfg3()
    gprof = profile.wrap(prof, base)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        render.Renderer(base, gprof)                                      # no key, and opacity 1: silent
        ok = copy.deepcopy(base)
        ok['final_xform']['opacity'] = 1
        render.Renderer(ok, gprof)
    gnm = copy.deepcopy(base)
    gnm['final_xform']['opacity'] = 0.3
    with pytest.warns(UserWarning, match='final_xform.opacity is ignored') as rec:
        rdr = render.Renderer(gnm, gprof)
    assert len(rec) == 1
    assert np.array_equal(rdr.packer.ops_array, GenomePacker(base).ops_array)


def test_blends_carry_opacity():
    """node -> animation and edge blends keep the key (a missing side blends from the default 1)."""
    from cuburn_amd.genome import blend
    xf = {'weight': 1, 'pre_affine': {'angle': 45}, 'variations': {'linear': {'weight': 1}}}
    a = {'type': 'node', 'xforms': {'0': dict(xf, opacity=0.25), '1': dict(xf)}}
    b = {'type': 'node', 'xforms': {'0': dict(xf, opacity=0.75), '1': dict(xf)}}
    anim = blend.blend(a, b, {'blend': {'xform_sort': 'natural'}})
    assert anim['xforms']['0_0']['opacity'] == [0.25, 0.75] and 'opacity' not in anim['xforms']['1_1']
    loop = blend.blend(a, a, {'blend': {'xform_sort': 'natural'}})
    assert loop['xforms']['0_0']['opacity'] == 0.25
    pk = GenomePacker(anim)
    assert sum(1 for o in pk.ops_array if o[0] == OP_OPACITY) == 1


# ------------------------------------------------------------------ 4. the curve in float32
def test_plot_probability_curve_float32():
    ps = [0.0, 1e-12, 1e-3] + [k / 100.0 for k in range(1, 100)] + [1 - 1e-6, 1 - 1e-7, 1.0, 1.5, -0.2]
    for p in ps:
        q32, q64 = plot_probability_f32(p), plot_probability(np.float32(p))
        if q64 in (0.0, 1.0):
            assert float(q32) == q64, (p, q32, q64)
        else:
            assert 0.0 < q32 < 1.0 and abs(float(q32) - q64) <= 2e-5 * q64, (p, q32, q64)
    assert plot_probability(0.5) == pytest.approx(0.1, rel=1e-12) and plot_probability(0.25) == pytest.approx(0.01, rel=1e-12)
    assert plot_probability_f32(0.5) == pytest.approx(0.1, rel=2e-5)
    assert plot_probability_f32(1e-12) == 0 and plot_probability_f32(1e-3) == 0          # below 2^-32
    below = np.nextafter(np.float32(1) - np.float32(1e-6), np.float32(0))             # the largest opacity that is not snapped to 1
    assert 0.0 < 1.0 - plot_probability(below) <= 3.6e-6                                 # what the snap costs at most


# ------------------------------------------------------------------ 2. / 3. the per-genome kernels


def _opacity_genomes():
    out = {'three_boxes': three_boxes((0.5, 1.0, 0.25))[0]}
    for cfg, key in (('cfg2', '2'), ('cfg3', '5'), ('cfg5', '07')):
        out[cfg] = with_opacity(configs.CONFIGS[cfg]()[0], [key])
    return out


@pytest.mark.parametrize('which', ['three_boxes', 'cfg2', 'cfg3', 'cfg5'])
def test_opacity_kernels_compile_within_budget(built, tmp_path, monkeypatch, which):
    """Genomes with an opacity compile for the walker geometries and accumulate modes of test_per_genome_kernel_compiles; the
    4-wave binned kernel has no scratch, no spills and at most 80 vector registers (rtc.hip's bound for the 1536-slot
    geometry)."""
    monkeypatch.delenv('FLAME_RTC_FLAGS', raising=False)
    gnm = _opacity_genomes()[which]
    for nw, count, acc in ((4, 1, 0), (8, 0, 3), (8, 1, 1)):
        rc, log = _compile(gnm, nw, count, acc)
        assert rc == 0, log[:3000]
    monkeypatch.setenv('FLAME_RTC_DUMP', str(tmp_path))
    rc, log = _compile(gnm, 4, 0, 1)
    assert rc == 0, log[:3000]
    assert 'kSpecOpac[] = {' in open(str(tmp_path / 'flame_spec.h')).read()
    r = _resources(tmp_path)
    print(which, r)
    assert r['vgpr'] <= 80 and r['spill'] == 0 and r['scratch'] == 0, r


# vector registers, scalar registers, static LDS and bytes of code of the 4-wave binned per-genome kernels of the keyless
# configs, as built from the commit before opacity existed (the disassemblies were compared and are identical).
# (Code bytes: 17664 / 21248 / 14848 until fsin / fcos took the fraction of |t| — a v_bfi_b32 and its mask per sine, an 8-byte
# encoding of v_fract_f32 per sine and cosine; registers and LDS as before.)
KEYLESS_KERNELS = {'cfg2': (60, 106, 0, 17792), 'cfg3': (60, 106, 0, 21504), 'cfg5': (60, 106, 0, 14976)}


@pytest.mark.parametrize('cfg', ['cfg2', 'cfg3', 'cfg5'])
def test_keyless_kernels_are_unchanged(built, tmp_path, monkeypatch, cfg):
    monkeypatch.delenv('FLAME_RTC_FLAGS', raising=False)
    monkeypatch.setenv('FLAME_RTC_DUMP', str(tmp_path))
    rc, log = _compile(configs.CONFIGS[cfg]()[0], 4, 0, 1)
    assert rc == 0, log[:3000]
    r = _resources(tmp_path)
    print(cfg, r)
    assert (r['vgpr'], r['sgpr'], r['lds'], r['text']) == KEYLESS_KERNELS[cfg], r
    assert re.search(r'kSpecOpac\[\] = \{(0,)+0\};', open(str(tmp_path / 'flame_spec.h')).read())


def test_compile_check_rejects_bad_opacity_structure(built):
    """(The same rejects of fl_genome_create need a context: tests/test_gpu_opacity.py.)"""
    gnm = three_boxes((0.5, None, None))[0]
    pk = GenomePacker(gnm)
    prog = np.ascontiguousarray(pk.prog, np.int32)
    log = C.create_string_buffer(4096)
    lib = _lib.load()

    def check(ops):
        ops = np.ascontiguousarray(ops, np.int32)
        return lib.fl_rtc_compile_check(prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), 4, 0, 1, log, len(log))
    rec = int(prog[5])
    ops = pk.ops_array.copy()
    i14 = [i for i, o in enumerate(ops) if o[0] == OP_CONST and o[1] == rec + 14][0]
    ops[i14, 2] |= 1 << 10
    assert check(ops) == _lib.FL_E_INVAL
    ops = pk.ops_array.copy()
    iop = [i for i, o in enumerate(ops) if o[0] == OP_OPACITY][0]
    ops[iop, 1] = rec + 13
    assert check(ops) == _lib.FL_E_INVAL
