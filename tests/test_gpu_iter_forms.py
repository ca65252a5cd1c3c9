"""
Every compile-time form of the per-genome iterate kernel (tests/iter_forms.py; DESIGN.md 4.1 has the table) on the device.

  * Oracle rows (linear + bent only): the oracle's device model is exact for them.  Three launches that start at rounds 0, 10
    and 17 — swap phases 0, 1 and 2 — in both accumulate modes (binned only for one and two xforms): counters, density, PACKED
    CELLS (the rows' cameras keep every cell below the drain thresholds, which is asserted), hot flags and colour per launch, RNG
    states and walker points at the end.  tests/test_cpu_iter_forms.py proves with the compiler that each row is the form it claims.
  * Interpreter rows (parametric variations whose parameters cross the tail's last register, word 27, and mobius): the per-genome
    kernel against the precompiled interpreter kernel (FLAME_RTC=0) from the same seeds, bit for bit.
  * Fallback budgets: rtc.hip keys its module cache by device, register limit and the generated header — NOT by FLAME_RTC_FLAGS —
    so one process cannot see two hoist budgets for one structure.  (That is left as it is; it only matters to whoever changes
    FLAME_RTC_FLAGS inside a process.)  One fresh child process per budget, started one after the other, runs the rows whose
    form the budget changes against the oracle; a child that dies of a signal or runs into its time limit fails the test and
    no further child is started.
  * Large workgroups: the resident and the table form at (8 waves, 512 slots) and (16 waves, 256 slots), whose sub-blocks of four
    waves are the walkers of 1024 four-wave slots (one operand table per sub-block): bit for bit the four-wave run of the same
    seeds, which the oracle rows hold to the oracle.

Chaos forms stay with tests/test_gpu_chaos.py.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from common import REPO
from cuburn_amd import render
import iter_forms as IF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def mgr(built):
    m = render.RenderManager(device=0, nslots=IF.NSLOTS, host_seed=11)
    assert (m.fb.nw, m.fb.nslots) == (4, IF.NSLOTS)
    return m


# ------------------------------------------------------------------------------------------------ oracle rows
@pytest.mark.parametrize('row', IF.ORACLE_ROWS, ids=repr)
def test_form_equals_oracle(mgr, row, capfd):
    for mode in row.modes():
        acc = IF.check_oracle_row(mgr, row, mode)
        print(row.name, 'mode', mode, 'accepted', acc)
    assert 'interpreter kernel' not in capfd.readouterr().err, 'the per-genome kernel was not used'


# ------------------------------------------------------------------------------------------------ interpreter rows
@pytest.mark.parametrize('row', IF.INTERP_ROWS, ids=repr)
def test_form_equals_interpreter(built, row, monkeypatch, capfd):
    gnm, prof = row.genome()
    out = {}
    for rtc in ('0', '1'):
        monkeypatch.setenv('FLAME_RTC', rtc)
        m = render.RenderManager(device=0, nslots=IF.NSLOTS, host_seed=5)
        seeds = None
        for mode in row.modes()[::-1]:                       # (binned first; the atomic run from the same RNG states)
            out[rtc, mode] = IF.gpu_launches(m, gnm, prof, mode, seeds_in=seeds)
            seeds = out[rtc, mode]['seeds0']
        m.fb.free()
    assert 'interpreter kernel' not in capfd.readouterr().err, 'the per-genome kernel was not used'
    for mode in row.modes():
        a, b = out['0', mode], out['1', mode]
        assert np.array_equal(a['seeds0'], b['seeds0'])
        for k in range(IF.LAUNCHES):
            tag = (row.name, mode, k)
            assert np.array_equal(a['ctr'][k][:3], b['ctr'][k][:3]), (tag, a['ctr'][k], b['ctr'][k])
            assert int(a['ctr'][k][0]) > IF.MIN_ACCEPTED, (tag, a['ctr'][k])
            assert np.array_equal(a['front'][k][:, 3], b['front'][k][:, 3]), tag
            # the bar of test_every_variation_per_genome_kernel_equals_interpreter (float atomics of drained cells: the order varies)
            assert np.allclose(a['front'][k][:, :3], b['front'][k][:, :3], rtol=1e-5, atol=1e-5), tag
            if int(a['ctr'][k][3]) == 0 and int(b['ctr'][k][3]) == 0 and int((a['atom'][k] >> np.uint64(54)).max()) < 256:
                assert np.array_equal(a['atom'][k], b['atom'][k]), tag
        bad = np.nonzero((a['rng'] != b['rng']).any(1))[0]
        assert bad.size == 0, (row.name, mode, 'rng', bad.size, int(bad[0]))
        both_nan = np.isnan(a['pts']) & np.isnan(b['pts'])
        pa, pb = a['pts'].view(np.uint32), b['pts'].view(np.uint32)
        bad = np.nonzero(((pa != pb) & ~both_nan).any(1))[0]
        assert bad.size == 0, (row.name, mode, 'walker', bad.size, int(bad[0]), a['pts'][bad[0]], b['pts'][bad[0]])


# ------------------------------------------------------------------------------------------------ fallback budgets
CHILD = r'''
import sys, time
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(tests)r)
from cuburn_amd import render
import iter_forms as IF
m = render.RenderManager(device=0, nslots=IF.NSLOTS, host_seed=11)
for name in IF.BUDGET_ROWS:
    row = IF.BY_NAME[name]
    for mode in row.modes():
        t = time.time()
        acc = IF.check_oracle_row(m, row, mode)
        print(name, 'mode', mode, 'accepted', acc, '%%.1f s' %% (time.time() - t), flush=True)
print('BUDGET CHILD OK')
'''
CHILD_TIMEOUT = 420           # seven hipRTC compiles of small linear genomes and as many oracle passes: about a minute
_dead = []                    # children that died of a signal or timed out: nothing further is started


@pytest.mark.parametrize('budget', IF.BUDGETS[1:])
def test_fallback_budget_equals_oracle(built, budget):
    if _dead:
        pytest.fail('not started: the child of budget %s died or hung' % _dead)
    env = dict(os.environ, FLAME_RTC_FLAGS='-DFL_HOIST_BUDGET=%d' % budget)
    env.pop('FLAME_RTC', None)
    t = time.time()
    try:
        r = subprocess.run([sys.executable, '-c', CHILD % dict(repo=REPO, tests=os.path.join(REPO, 'tests'))], capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT, env=env)
    except subprocess.TimeoutExpired as e:
        _dead.append(budget)
        pytest.fail('budget %d: the child ran into its time limit (%d s); stderr tail: %s' % (budget, CHILD_TIMEOUT, (e.stderr or b'')[-3000:]))
    print('budget %d: child wall time %.1f s' % (budget, time.time() - t))
    print(r.stdout)
    if r.returncode < 0:
        _dead.append(budget)
    assert r.returncode == 0, (budget, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert 'BUDGET CHILD OK' in r.stdout and r.stdout.count('accepted') == sum(len(IF.BY_NAME[n].modes()) for n in IF.BUDGET_ROWS)
    assert 'interpreter kernel' not in r.stderr, r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ large workgroups
LARGE = ('n2_posts2', 'n5')
_four = {}


def _geometry_run(name, nw, nslots, monkeypatch):
    row = IF.BY_NAME[name]
    gnm, prof = IF.animated(*row.genome())          # every temporal sample its own parameter block: a sub-block that read another's would show
    if nw != 4:
        monkeypatch.setenv('FLAME_NW', str(nw))
    else:
        monkeypatch.delenv('FLAME_NW', raising=False)
    m = render.RenderManager(device=0, nslots=nslots, host_seed=46)
    assert (m.fb.nw, m.fb.nslots, m.fb.nwalkers) == (nw, nslots, 1024 * 256 + 64 * 256 + 65536)
    out, seeds = {}, None
    for mode in row.modes()[::-1]:
        out[mode] = IF.gpu_launches(m, gnm, prof, mode, seeds_in=seeds)
        seeds = out[mode]['seeds0']
    m.fb.free()
    return out


@pytest.mark.parametrize('geom', [(8, 512), (16, 256)])
@pytest.mark.parametrize('name', LARGE)
def test_large_workgroups_equal_four_wave_slots(built, name, geom, monkeypatch, capfd):
    """Set up as test_gpu_parity.test_paired_halves_are_the_walkers_of_1024_four_wave_slots: the halves of 512 eight-wave slots
    and the quarters of 256 sixteen-wave slots walk the temporal samples of 1024 four-wave slots.  n=2: every record resident
    (per sub-block: each reads its own parameter block); n=5: one operand table per sub-block, xtab[half * 16 + k].  The genomes
    are animated (iter_forms.animated) so that the sub-blocks' records and tables differ."""
    if name not in _four:
        _four[name] = _geometry_run(name, 4, 1024, monkeypatch)
    four, big = _four[name], _geometry_run(name, geom[0], geom[1], monkeypatch)
    assert 'interpreter kernel' not in capfd.readouterr().err, 'the per-genome kernel was not used'
    for mode in IF.BY_NAME[name].modes():
        a, b = four[mode], big[mode]
        assert np.array_equal(a['seeds0'], b['seeds0'])
        for k in range(IF.LAUNCHES):
            tag = (name, geom, mode, k)
            assert np.array_equal(a['ctr'][k][:3], b['ctr'][k][:3]), (tag, a['ctr'][k], b['ctr'][k])
            assert int(a['ctr'][k][0]) > IF.MIN_ACCEPTED and int(a['ctr'][k][3]) == 0 and int(b['ctr'][k][3]) == 0, (tag, a['ctr'][k], b['ctr'][k])
            assert int((a['atom'][k] >> np.uint64(54)).max()) < 256, tag          # no drains: the packed cells are compared
            assert np.array_equal(a['atom'][k], b['atom'][k]), tag
            assert np.array_equal(a['front'][k].view(np.uint32), b['front'][k].view(np.uint32)), tag
        assert np.array_equal(a['rng'], b['rng']), (name, geom, mode)
        assert np.array_equal(a['pts'].view(np.uint32), b['pts'].view(np.uint32)), (name, geom, mode)
