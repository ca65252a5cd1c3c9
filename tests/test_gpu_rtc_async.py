"""
Per-genome kernels compiled beside the frame loop (FLAME_RTC_ASYNC=1, csrc/rtc.hip).

Three structures — a plain ring, one with an `opacity`, one with a `chaos` table — animated (iter_forms.animated), three frames
each at the small frame, launches and sample count of tests/test_gpu_iter_forms.py, from one fixed seed:

  * an asynchronous context with the worker HELD (fl_debug_rtc_hold) prepares the genome and renders frame 1: the process-wide
    counters show launches on the interpreter kernel with a job pending and none on a per-genome kernel;
  * released, and after fl_rtc_wait, frames 2 and 3 show launches on the per-genome kernel only;
  * a synchronous context renders the same three frames from the same seed, and after every frame the two are compared exactly
    as test_gpu_iter_forms.test_form_equals_interpreter compares the two kernels: counters, densities, RNG states and walker
    points bit for bit, packed cells bit for bit where no cell was drained, colour sums at that test's rtol = atol = 1e-5.

  (The synchronous context runs second: the process keeps one module cache for both, so a kernel the baseline had compiled first
  would be there for the asynchronous context at once and nothing would ever be pending.  The baseline then launches the kernels
  the asynchronous walk settled on; that the synchronous walk settles on the same code objects is what the shared disk-cache key
  says, and tests/test_gpu_rtc_cache.py counts.)

Destroying the genome and the context while their job is held, then releasing the worker, in a child process under a time limit:
exit status 0.  A compile that fails in the compiler: today's message once, in both modes, and the baseline's frames from the
interpreter kernel.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, render
import iter_forms as IF
from rtc_async_frames import TIMES, SEED, STRUCTURES, render_frames

pytestmark = pytest.mark.gpu

MESSAGE = 'per-genome kernel not available'


def assert_same_frames(name, mode, fa, fb):
    """test_gpu_iter_forms.test_form_equals_interpreter's comparison, frame by frame"""
    assert len(fa) == len(fb) == len(TIMES)
    for i, (a, b) in enumerate(zip(fa, fb)):
        for k in range(IF.LAUNCHES):
            tag = (name, mode, 'frame', i, 'launch', k)
            assert np.array_equal(a['ctr'][k][:3], b['ctr'][k][:3]), (tag, a['ctr'][k], b['ctr'][k])
            assert int(a['ctr'][k][0]) > IF.MIN_ACCEPTED, (tag, a['ctr'][k])
            assert np.array_equal(a['front'][k][:, 3], b['front'][k][:, 3]), tag
            assert np.allclose(a['front'][k][:, :3], b['front'][k][:, :3], rtol=1e-5, atol=1e-5), tag
            if int(a['ctr'][k][3]) == 0 and int(b['ctr'][k][3]) == 0 and int((a['atom'][k] >> np.uint64(54)).max()) < 256:
                assert np.array_equal(a['atom'][k], b['atom'][k]), tag
        bad = np.nonzero((a['rng'] != b['rng']).any(1))[0]
        assert bad.size == 0, (name, mode, i, 'rng', bad.size, int(bad[0]))
        both_nan = np.isnan(a['pts']) & np.isnan(b['pts'])
        pa, pb = a['pts'].view(np.uint32), b['pts'].view(np.uint32)
        bad = np.nonzero(((pa != pb) & ~both_nan).any(1))[0]
        assert bad.size == 0, (name, mode, i, 'walker', bad.size, int(bad[0]), a['pts'][bad[0]], b['pts'][bad[0]])


_baseline = {}          # (structure, mode) -> the synchronous context's frames, computed once and left alone


def _sync_frames(name, mode, monkeypatch):
    if (name, mode) not in _baseline:
        monkeypatch.delenv('FLAME_RTC_ASYNC', raising=False)
        monkeypatch.delenv('FLAME_RTC', raising=False)
        gnm, prof = IF.animated(*STRUCTURES[name]())
        m = render.RenderManager(device=0, nslots=IF.NSLOTS, host_seed=SEED)
        _baseline[name, mode] = render_frames(m, gnm, prof, mode)
        m.fb.free()
    return _baseline[name, mode]


@pytest.mark.parametrize('mode', [1, 0], ids=['binned', 'atomic'])
@pytest.mark.parametrize('name', sorted(STRUCTURES))
def test_async_frames_equal_synchronous_frames(built, name, mode, monkeypatch, capfd):
    lib = _lib.load()
    monkeypatch.delenv('FLAME_RTC', raising=False)
    monkeypatch.delenv('FLAME_RTC_FLAGS', raising=False)
    monkeypatch.setenv('FLAME_RTC_ASYNC', '1')
    gnm, prof = IF.animated(*STRUCTURES[name]())
    m = render.RenderManager(device=0, nslots=IF.NSLOTS, host_seed=SEED)
    queued0 = render.rtc_stats()['jobs_queued']

    def before_frame(k, ctx, g, dim):
        if k == 0:
            assert lib.fl_debug_rtc_hold(1) == 0
            _lib.check(lib.fl_genome_prepare(ctx, g, dim.w, dim.h, mode))
            assert render.rtc_stats()['jobs_queued'] == queued0 + 1
            assert lib.fl_rtc_wait(ctx, g) == _lib.FL_E_INVAL            # held: the wait would never end, and says so
        if k == 1:
            assert lib.fl_debug_rtc_hold(0) == 0
            _lib.check(lib.fl_rtc_wait(ctx, g))

    try:
        fa = render_frames(m, gnm, prof, mode, before_frame)
    finally:
        lib.fl_debug_rtc_hold(0)
    m.fb.free()
    moved = [f['moved'] for f in fa]
    print(name, mode, moved)
    assert (moved[0]['interp_launches_pending'], moved[0]['spec_launches'], moved[0]['compiles']) == (IF.LAUNCHES, 0, 0), moved[0]
    assert moved[0]['jobs_queued'] == 1                                  # the counting variant the taps launch, beside the prepared one
    for mv in moved[1:]:
        assert (mv['interp_launches_pending'], mv['spec_launches'], mv['jobs_queued'], mv['compiles']) == (0, IF.LAUNCHES, 0, 0), mv
    fb = _sync_frames(name, mode, monkeypatch)
    assert all(f['moved']['spec_launches'] == IF.LAUNCHES and f['moved']['jobs_queued'] == 0 for f in fb), [f['moved'] for f in fb]
    assert MESSAGE not in capfd.readouterr().err
    assert_same_frames(name, mode, fa, fb)


CHILD_DESTROY = r'''
import sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(tests)r)
import os
os.environ['FLAME_RTC_ASYNC'] = '1'
from cuburn_amd import _lib, profile, render
import iter_forms as IF
lib = _lib.load()
gnm, prof = IF.ring(3, posts=(0, 2), mag=0.8, scale=0.32)
gprof = profile.wrap(prof, gnm)
m = render.RenderManager(device=0, nslots=IF.NSLOTS, host_seed=3)
rdr = render.Renderer(gnm, gprof)
g = rdr._handle(m.fb)
dim = m.fb.calc_dim(gprof.width, gprof.height)
assert lib.fl_debug_rtc_hold(1) == 0
_lib.check(lib.fl_genome_prepare(m.fb.ctx, g, dim.w, dim.h, 1))
_lib.check(lib.fl_genome_prepare(m.fb.ctx, g, dim.w, dim.h, 0))
st = render.rtc_stats()
assert st['jobs_queued'] == 2 and st['compiles'] == 0, st
lib.fl_genome_destroy(g)
rdr.mod = None
m.fb.free()
assert lib.fl_debug_rtc_hold(0) == 0
print('DESTROY CHILD OK', flush=True)
'''


def test_destroy_with_a_held_job(built):
    env = dict(os.environ)
    for k in ('FLAME_RTC', 'FLAME_RTC_FLAGS', 'FLAME_RTC_CACHE'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, '-c', CHILD_DESTROY % dict(repo=REPO, tests=os.path.join(REPO, 'tests'))], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert 'DESTROY CHILD OK' in r.stdout


CHILD_FAIL = r"""
import sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(tests)r)
import numpy as np
from cuburn_amd import _lib, render
import iter_forms as IF
import rtc_async_frames as T
lib = _lib.load()
gnm, prof = IF.animated(*T.STRUCTURES['plain']())
m = render.RenderManager(device=0, nslots=IF.NSLOTS, host_seed=T.SEED)

def before_frame(k, ctx, g, dim):
    if k == 0:
        _lib.check(lib.fl_genome_prepare(ctx, g, dim.w, dim.h, 1))
        _lib.check(lib.fl_rtc_wait(ctx, g))

frames = T.render_frames(m, gnm, prof, 1, before_frame)
m.fb.free()
flat = {}
for i, f in enumerate(frames):
    for key in ('ctr', 'atom', 'front'):
        for k, v in enumerate(f[key]):
            flat['%%d/%%s/%%d' %% (i, key, k)] = v
    flat['%%d/rng' %% i], flat['%%d/pts' %% i] = f['rng'], f['pts']
    flat['%%d/spec' %% i] = np.array(f['moved']['spec_launches'])
np.savez(%(out)r, **flat)
print('FAIL CHILD OK', render.rtc_stats(), flush=True)
"""


@pytest.mark.parametrize('async_', [False, True], ids=['sync', 'async'])
def test_compile_failure_falls_back_once(built, async_, monkeypatch, tmp_path):
    """The plain structure in a fresh process whose FLAME_RTC_FLAGS break the kernel's source: the compiler refuses it, the
    library says so once and the three frames come from the interpreter kernel — the synchronous baseline's frames."""
    base = _sync_frames('plain', 1, monkeypatch)
    out = str(tmp_path / 'frames.npz')
    env = dict(os.environ, FLAME_RTC_FLAGS='-Dfloat4=@')
    for k in ('FLAME_RTC', 'FLAME_RTC_CACHE', 'FLAME_RTC_ASYNC'):
        env.pop(k, None)
    if async_:
        env['FLAME_RTC_ASYNC'] = '1'
    r = subprocess.run([sys.executable, '-c', CHILD_FAIL % dict(repo=REPO, tests=os.path.join(REPO, 'tests'), out=out)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert 'FAIL CHILD OK' in r.stdout
    assert r.stderr.count(MESSAGE) == 1 and 'hiprtc compile failed' in r.stderr, r.stderr[-3000:]
    z = np.load(out)
    frames = []
    for i in range(len(TIMES)):
        assert int(z['%d/spec' % i]) == 0
        f = dict((key, [z['%d/%s/%d' % (i, key, k)] for k in range(IF.LAUNCHES)]) for key in ('ctr', 'atom', 'front'))
        f['rng'], f['pts'] = z['%d/rng' % i], z['%d/pts' % i]
        frames.append(f)
    assert_same_frames('plain, failed compile', 1, frames, base)
