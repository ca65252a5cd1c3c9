"""
Every row of tests/iter_forms.py is the form of the per-genome iterate kernel that it claims to be — proved without a GPU:

  * the row's genome is packed and compiled for gfx950 by the library itself (fl_rtc_compile_check: hipRTC needs no device), in the
    four-wave geometry and the accumulate modes tests/test_gpu_iter_forms.py runs it in, with FLAME_RTC_DUMP keeping the generated
    flame_spec.h and the code object;
  * tests/iter_forms_probe.hip — `#include "iter.hip"` and one static_assert over kSpecResident, kHoistCol, kHoistAff, kHoistPost,
    kHoistFinal, kSpecPost[FL_SPEC_NXF] and kTab — is compiled host-only and syntax-only against THAT header with the values
    iter_forms.form_of() gives as -DEXP_*: iter.hip's own constexpr predicates decide, the Python mirror is only ever compared;
  * the fallback budgets (FL_HOIST_BUDGET 7 / 5 / 0, which rtc_iter_kernel applies past the register limit) the same way, for the
    rows whose form they change;
  * SPLIT_FUSE and MERGE are local to iter_body: their defining source lines are pinned verbatim;
  * every default-budget kernel needs at most 80 vector registers (rtc_iter_kernel's limit at 1536 four-wave slots; 128 at the
    1024 of the GPU tests), so the GPU run of a default row cannot silently be a fallback-budget kernel.

The compiles run once per session in a pool of at most 8 child processes (a fresh process per compile: the library reads
FLAME_RTC_DUMP / FLAME_RTC_FLAGS from its environment).  The oracle alone is also held to the two conditions the GPU comparison
needs of every row: more than 100000 accepted samples per launch, and no cell that fills up (so the packed cells are compared).
"""
import json
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from common import REPO, O, prepare
import iter_forms as IF

CSRC = os.path.join(REPO, 'cuburn_amd', 'csrc')
READELF = '/opt/rocm/lib/llvm/bin/llvm-readelf'
VGPR_LIMIT = 80

# (row, budget): the default budget for every row, the fallback budgets for the rows they change
JOBS = [(r.name, 12) for r in IF.ROWS] + sorted(IF.BUDGET_EXPECT, key=lambda nb: (-nb[1], IF.BUDGET_ROWS.index(nb[0])))

CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(tests)r)
import numpy as np
from cuburn_amd import _lib
from cuburn_amd.packer import GenomePacker
import iter_forms as IF
gnm, prof = IF.BY_NAME[%(name)r].genome()
pk = GenomePacker(gnm)
prog = np.ascontiguousarray(pk.prog, np.int32); ops = np.ascontiguousarray(pk.ops_array, np.int32)
log = C.create_string_buffer(8192)
rc = _lib.load().fl_rtc_compile_check(prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), 4, 1, %(acc)d, log, len(log))
print(json.dumps(dict(rc=rc, unsupported=rc == _lib.FL_E_UNSUPPORTED, log=log.value.decode(errors='replace')[:3000], var_stride=int(pk.var_stride))))
'''


def accs(row):
    """accumulate modes the GPU tests run a row in (count = 1 always): binned for all, atomic from three xforms"""
    return (1,) if row.nxf <= 2 else (1, 0)


def log_pack3():
    """-DFL_LOG_PACK3=<n> as the library's build passes it to hipRTC (rtc.hip keeps the option as a string)"""
    from cuburn_amd import _lib
    m = re.search(rb'-DFL_LOG_PACK3=(\d+)', open(_lib.LIB_PATH, 'rb').read())
    assert m, 'libflame_hip.so does not carry its FL_LOG_PACK3 option'
    return int(m.group(1))


def probe(hipcc, hdr_dir, form, budget, pack3):
    cmd = [hipcc, '--cuda-host-only', '-fsyntax-only', '-std=c++20', '-DFL_RTC=1', '-DFL_LOG_PACK3=%d' % pack3,
           '-I' + hdr_dir, '-I' + CSRC, '-I' + os.path.join(REPO, 'include')] + IF.defines(form)
    if budget != 12:
        cmd.append('-DFL_HOIST_BUDGET=%d' % budget)
    return subprocess.run(cmd + [os.path.join(REPO, 'tests', 'iter_forms_probe.hip')], capture_output=True, text=True, timeout=600)


def one_job(base, name, budget, hipcc, pack3):
    row = IF.BY_NAME[name]
    env = {k: v for k, v in os.environ.items() if k not in ('FLAME_RTC_FLAGS', 'FLAME_RTC_DUMP')}
    if budget != 12:
        env['FLAME_RTC_FLAGS'] = '-DFL_HOIST_BUDGET=%d' % budget
    out = dict(compiles={}, vgpr={})
    for acc in accs(row):
        d = os.path.join(base, '%s_b%d_a%d' % (name, budget, acc))
        os.makedirs(d)
        r = subprocess.run([sys.executable, '-c', CHILD % dict(repo=REPO, tests=os.path.join(REPO, 'tests'), name=name, acc=acc)],
                           capture_output=True, text=True, timeout=900, env=dict(env, FLAME_RTC_DUMP=d))
        res = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 and r.stdout.strip() else dict(rc=-1, unsupported=False, log=r.stderr[-3000:])
        out['compiles'][acc] = res
        if res['rc'] != 0:
            continue
        if os.path.exists(READELF):
            notes = subprocess.run([READELF, '--notes', os.path.join(d, 'k_iter_spec.co')], capture_output=True, text=True, timeout=120).stdout
            num = lambda key: int(re.search(r'\.' + key + r':\s+(\d+)', notes).group(1))
            out['vgpr'][acc] = (num('vgpr_count'), num('vgpr_spill_count'), num('private_segment_fixed_size'))
        if acc == 1:
            out['header'] = open(os.path.join(d, 'flame_spec.h')).read()
            out['hdr_dir'] = d
            if hipcc:
                p = probe(hipcc, d, IF.budget_form(name, budget) if budget != 12 else row.form, budget, pack3)
                out['probe'] = (p.returncode, p.stderr[-3000:])
    return out


@pytest.fixture(scope='module')
def compiled(built, tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    hipcc = hipcc if os.path.exists(hipcc) else None
    base = str(tmp_path_factory.mktemp('iter_forms'))
    pack3 = log_pack3()
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        futs = dict(((n, b), pool.submit(one_job, base, n, b, hipcc, pack3)) for n, b in JOBS)
        res = dict((k, f.result()) for k, f in futs.items())
    res['hipcc'], res['pack3'] = hipcc, pack3
    return res


@pytest.mark.parametrize('name,budget', JOBS)
def test_row_compiles_to_the_form_it_states(compiled, name, budget):
    r = compiled[name, budget]
    row = IF.BY_NAME[name]
    if any(c['unsupported'] for c in r['compiles'].values()):
        pytest.skip('libhiprtc is not installed')
    for acc, c in r['compiles'].items():
        assert c['rc'] == 0, (name, budget, acc, c['log'])
    # the header is this structure's
    nposts = len(row.posts)
    hdr = r['header']
    assert '#define FL_SPEC_NXF %d\n' % row.nxf in hdr and '#define FL_SPEC_FINAL %d\n' % (row.final is not None) in hdr
    post = [int(v) for v in re.search(r'kSpecPost\[\] = \{([0-9,]+)\}', hdr).group(1).rstrip(',').split(',')]
    assert len(post) == row.nxf + (row.final is not None) + 1 and sum(post[:row.nxf]) == nposts
    assert post[row.nxf] == (1 if row.final == 'post' else 0)
    assert '#define FL_SPEC_CHAOS 0\n' in hdr and '#define FL_SPEC_NW 4\n' in hdr
    if compiled['hipcc'] is None:
        pytest.skip('no hipcc')
    rc, err = r['probe']
    assert rc == 0, (name, budget, IF.defines(IF.budget_form(name, budget)), err)


def test_probe_refuses_a_wrong_form(compiled):
    """The static_assert does decide: the header of 4 xforms with 3 posts and a final xform passes as (resident 0, col 0, aff 0,
    post 0, final 1, final's post 1, table 1) — above — and fails with the same expectations at FL_HOIST_BUDGET 5, and with any
    single expectation flipped."""
    if compiled['hipcc'] is None:
        pytest.skip('no hipcc')
    r = compiled['n4_posts3_finalpost', 12]
    if 'hdr_dir' not in r:
        pytest.skip('libhiprtc is not installed')
    form = IF.BY_NAME['n4_posts3_finalpost'].form
    assert [int(form[k]) for k in IF.PROBED] == [0, 0, 0, 0, 1, 1, 1]
    p = probe(compiled['hipcc'], r['hdr_dir'], form, 5, compiled['pack3'])
    assert p.returncode != 0 and 'static assertion failed' in p.stderr and "not the one tests/iter_forms.py states" in p.stderr, p.stderr[-2000:]
    for k in ('resident', 'tab'):
        p = probe(compiled['hipcc'], r['hdr_dir'], dict(form, **{k: not form[k]}), 12, compiled['pack3'])
        assert p.returncode != 0 and 'static assertion failed' in p.stderr, (k, p.stderr[-2000:])


@pytest.mark.parametrize('row', IF.ROWS, ids=repr)
def test_default_budget_kernels_fit_the_register_limit(compiled, row):
    r = compiled[row.name, 12]
    if not os.path.exists(READELF):
        pytest.skip('no llvm-readelf')
    if any(c['unsupported'] for c in r['compiles'].values()):
        pytest.skip('libhiprtc is not installed')
    assert sorted(r['vgpr']) == sorted(accs(row))
    for acc, (vgpr, spill, scratch) in r['vgpr'].items():
        print(row.name, 'acc', acc, 'vgpr', vgpr, 'spill', spill, 'scratch', scratch)
        assert vgpr <= VGPR_LIMIT and spill == 0, (row.name, acc, vgpr, spill, scratch)
        if row.kind == 'oracle':        # (linear and bent need no private segment; a parametric variation's library code may)
            assert scratch == 0, (row.name, acc, scratch)


def test_interpreter_held_rows_have_the_parameter_layouts_they_claim(compiled):
    """bent + lazysusan: var_stride 7, the second variation's parameters are words 25..29 of the record (the tail's registers
    end at word 27); mobius: var_stride 10."""
    from cuburn_amd.packer import GenomePacker
    for row in IF.INTERP_ROWS:
        pk = GenomePacker(row.genome()[0])
        rec = int(pk.prog[5])
        if 'cross27' in row.name:
            assert pk.var_stride == 7
            names = [pk.packed[rec + w][-1] for w in range(25, 30)]
            assert pk.packed[rec + 25][-2] == 'lazysusan' and names == ['space', 'spin', 'twist', 'x', 'y'], pk.packed[rec + 23:rec + 30]
        else:
            assert pk.var_stride == 10
            assert pk.packed[rec + 18][-2:] == ('mobius', 'im_a') and pk.packed[rec + int(pk.prog[6]) + 27][-2:] == ('mobius', 'weight')
    src = open(os.path.join(CSRC, 'iter.hip')).read()
    assert 'constexpr int kTailFirst = FL_XF_HDR + 2, kTailWords = 10;' in src
    assert re.search(r'#define FL_XF_HDR\s+16\b', open(os.path.join(CSRC, 'flame_device.h')).read() + open(os.path.join(REPO, 'include', 'flame_hip.h')).read())


def test_loop_shape_thresholds_are_the_source_lines():
    """SPLIT_FUSE (= ROT3) and MERGE are constexpr locals of iter_body; form_of() restates the lines below."""
    src = open(os.path.join(CSRC, 'iter.hip')).read()
    for line in (IF.SPLIT_FUSE_LINE, IF.MERGE_LINE, IF.MERGE_MAX_LINE, 'constexpr bool ROT3 = SPLIT_FUSE;', '#define FL_HOIST_BUDGET 12',
                 '#define FL_XTAB_BYTES 256'):
        assert src.count(line) == 1, line
    rtc = open(os.path.join(CSRC, 'rtc.hip')).read()
    assert 'const char *budgets[] = {nullptr, "-DFL_HOIST_BUDGET=7", "-DFL_HOIST_BUDGET=5", "-DFL_HOIST_BUDGET=0"};' in rtc
    assert IF.BUDGETS == (12, 7, 5, 0) and IF.MERGE_MAX_XF == 4


def test_rows_reach_every_form_and_both_sides_of_every_threshold():
    IF._check_budget_rows()
    IF._check_coverage()
    # the mirror itself at the thresholds of DESIGN.md's table
    f = IF.form_of
    assert f(4, 2, 0, 0)['resident'] and not f(4, 3, 0, 0)['resident'] and not f(5, 0, 0, 0)['resident']
    assert f(3, 0, 0, 0)['aff'] and not f(4, 0, 0, 0)['aff'] and f(4, 0, 0, 0)['col']
    assert f(1, 1, 0, 0)['post'] and f(2, 2, 0, 0)['post'] and not f(3, 1, 0, 0)['post']
    assert f(1, 0, 1, 1, budget=7)['final_post'] and not f(1, 0, 1, 1, budget=5)['final']
    assert f(5, 0, 0, 0)['tab'] and not f(5, 0, 0, 0, budget=7)['tab'] and not f(5, 0, 0, 0, chaos=True)['tab']
    assert f(16, 0, 0, 0)['tab'] and f(17, 0, 0, 0)['plain']
    assert f(9, 0, 0, 0)['split_fuse'] and not f(10, 0, 0, 0)['split_fuse']
    assert f(4, 3, 0, 0)['merge'] and f(4, 3, 0, 0)['tab'] and not f(5, 0, 0, 0)['merge'] and not f(4, 0, 0, 0, chaos=True)['merge']


def oracle_launches(row, mode, nrounds=7, fuse=3, launches=3, nslots=1024):
    """The launches of tests/test_gpu_iter_forms.py on the oracle alone (its own float64 parameter blocks): per launch the
    accepted samples, the drains of full cells and the largest count of a packed cell."""
    gnm, prof = row.genome()
    F = prepare(gnm, prof, 0.5, nslots=nslots)
    d = F['dim']
    nbins, nwalk = d.ah * d.astride, nslots * 256
    rng, points = F['seeds'][:nwalk].copy(), np.full((nwalk, 4), np.nan, np.float32)
    hot, atom, out4 = np.zeros(nbins // 16, np.uint32), np.zeros(nbins, np.uint64), np.zeros((nbins, 4), np.float32)
    out, r0 = [], 0
    for k in range(launches):
        f = fuse if k == 0 else 0
        ctr = O.iter_launch(O.GEOM_4x64, d, F['packer'].prog, F['params'], F['palette'], rng, points, nslots, hot, atom, out4, r0, nrounds + f, f)
        out.append((int(ctr[0]), int(ctr[3]), int((atom >> np.uint64(54)).max())))
        if mode == 1:
            hot[:] = 0
        O.flush(d, atom, out4, hot)
        if mode == 1:
            hot[:] = 0
        r0 += nrounds + f
    return out


@pytest.mark.parametrize('row', IF.ORACLE_ROWS, ids=repr)
def test_oracle_alone_meets_the_conditions_of_the_gpu_comparison(built, row):
    """Camera scales are chosen so that every launch of every row accepts more than 100000 samples and no cell reaches the
    256 hits at which the binned accumulate's LDS cells drain (512: the packed-atomic scheme's) — the packed cells of every row
    are then compared bit for bit, in every mode the row runs in."""
    for mode in row.modes():
        for k, (acc, spill, top) in enumerate(oracle_launches(row, mode)):
            assert acc > 100000 and spill == 0 and top < 256, (row.name, mode, k, acc, spill, top)
