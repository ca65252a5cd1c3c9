"""
The disk cache of per-genome kernels on the device (FLAME_RTC_CACHE, csrc/rtc.hip + rtc_cache.h).

The module cache is per process, so every run is a fresh child process; they run one after another, each under its own time
limit, and after a child that died of a signal or ran into its limit no further child is started.  One structure (the `n3` ring
of tests/iter_forms.py) at the smallest geometry, 1024 four-wave slots, one frame of seven rounds through queue_frame: a cold run
compiles one kernel.  The frame keeps every cell below the drain threshold (iter_forms: asserted there), so its bytes are a
function of the kernel and the seeds alone and are compared exactly.

Counters decide; nothing here looks at a clock.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from common import REPO

pytestmark = pytest.mark.gpu

CHILD = r'''
import json, os, sys
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(tests)r)
import numpy as np
from cuburn_amd import _lib, profile, render
import iter_forms as IF
gnm, prof = IF.BY_NAME['n3'].genome()
prof = dict(prof, spp=49)                                  # 49 x 256 x 144 samples: seven rounds of 1024 x 256 walkers, one launch
gprof = profile.wrap(prof, gnm)
m = render.RenderManager(device=0, nslots=IF.NSLOTS, host_seed=77)
m.fuse = IF.FUSE
rdr = render.Renderer(gnm, gprof)
if render.async_compile():                                 # the frame must come from the per-genome kernel in every run
    m.prepare(rdr, gprof, 0.5)
    _lib.check(_lib.load().fl_rtc_wait(m.fb.ctx, rdr._handle(m.fb)))
evt, h_out = m.queue_frame(rdr, gnm, gprof, 0.5)
evt.synchronize()
np.save(%(out)r, np.array(h_out))
t = m.timings()
print(json.dumps(dict(stats=render.rtc_stats(), spec=t['spec_launches'], interp=t['interp_launches'], lit=int((np.array(h_out)[..., :3] > 0).sum()))))
m.fb.free()
'''
CHILD_TIMEOUT = 300
_dead = []


def run_child(tmp, tag, **env_extra):
    if _dead:
        pytest.fail('not started: the child %s died or hung' % _dead)
    env = dict(os.environ)
    for k in ('FLAME_RTC', 'FLAME_RTC_FLAGS', 'FLAME_RTC_CACHE', 'FLAME_RTC_ASYNC', 'FLAME_RTC_DUMP', 'FLAME_NW'):
        env.pop(k, None)
    env.update(env_extra)
    out = os.path.join(str(tmp), tag + '.npy')
    try:
        r = subprocess.run([sys.executable, '-c', CHILD % dict(repo=REPO, tests=os.path.join(REPO, 'tests'), out=out)], capture_output=True,
                           text=True, timeout=CHILD_TIMEOUT, env=env)
    except subprocess.TimeoutExpired as e:
        _dead.append(tag)
        pytest.fail('%s: the child ran into its time limit (%d s); stderr tail: %s' % (tag, CHILD_TIMEOUT, (e.stderr or b'')[-3000:]))
    if r.returncode < 0:
        _dead.append(tag)
    assert r.returncode == 0, (tag, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads(r.stdout.strip().split('\n')[-1])
    print(tag, res)
    assert res['spec'] == 1 and res['interp'] == 0 and res['lit'] > 1000, (tag, res)       # one launch, on the per-genome kernel, of a picture
    return res['stats'], np.load(out).tobytes(), r.stderr


def disk(st):
    return st['compiles'], st['disk_hits'], st['disk_misses'], st['disk_writes'], st['disk_rejects']


def listing(d):
    return dict((f, open(os.path.join(d, f), 'rb').read()) for f in sorted(os.listdir(d)))


@pytest.fixture(scope='module')
def runs(built, tmp_path_factory):
    """No cache; run 1, cold; run 2, warm."""
    tmp = tmp_path_factory.mktemp('rtc_cache')
    d = str(tmp / 'cache')                                  # (missing: the library makes it)
    none = run_child(tmp, 'none')
    cold = run_child(tmp, 'cold', FLAME_RTC_CACHE=d)
    files = listing(d)
    warm = run_child(tmp, 'warm', FLAME_RTC_CACHE=d)
    return dict(tmp=tmp, dir=d, none=none, cold=cold, warm=warm, files=files)


def test_cold_run_writes_what_it_compiles(runs):
    st, frame, err = runs['cold']
    n = st['compiles']
    assert n > 0 and disk(st) == (n, 0, n, n, 0), st
    assert 'libflame_hip' not in err, err[-2000:]
    assert len(runs['files']) == n and all(f.endswith('.co') and len(f) == 35 for f in runs['files']), sorted(runs['files'])
    print('code object sizes:', [len(v) - 44 for v in runs['files'].values()])
    st0, frame0, err0 = runs['none']
    assert disk(st0) == (n, 0, 0, 0, 0) and 'libflame_hip' not in err0      # no switch: the same compiles, no file touched
    assert frame == frame0


def test_warm_run_compiles_nothing(runs):
    n = runs['cold'][0]['compiles']
    st, frame, err = runs['warm']
    assert disk(st) == (0, n, 0, 0, 0), st
    assert 'libflame_hip' not in err, err[-2000:]
    assert frame == runs['cold'][1] and frame == runs['none'][1]
    assert listing(runs['dir']) == runs['files']


def test_truncated_file_is_rejected_and_replaced(runs):
    name = sorted(runs['files'])[0]
    path = os.path.join(runs['dir'], name)
    whole = runs['files'][name]
    open(path, 'wb').write(whole[:len(whole) - 1000])
    st, frame, err = run_child(runs['tmp'], 'cut', FLAME_RTC_CACHE=runs['dir'])
    n = runs['cold'][0]['compiles']
    assert disk(st) == (1, n - 1, 0, 1, 1), st
    assert 'libflame_hip' not in err, err[-2000:]
    assert open(path, 'rb').read() == whole and listing(runs['dir']) == runs['files']
    assert frame == runs['cold'][1]


def test_other_options_are_other_keys(runs):
    st, frame, err = run_child(runs['tmp'], 'budget5', FLAME_RTC_CACHE=runs['dir'], FLAME_RTC_FLAGS='-DFL_HOIST_BUDGET=5')
    n = st['compiles']
    assert n > 0 and disk(st) == (n, 0, n, n, 0), st                                  # misses only
    now = listing(runs['dir'])
    assert len(now) == len(runs['files']) + n and all(now[f] == v for f, v in runs['files'].items())
    assert not [f for f in now if '.tmp.' in f]


def test_async_walk_settles_on_the_synchronous_walks_kernels(runs):
    """FLAME_RTC_ASYNC=1 with a cold cache of its own: the worker thread leaves the files the synchronous run left, byte for
    byte, and the frame is the same; warm, it runs no compiler either."""
    d = str(runs['tmp'] / 'cache_async')
    st, frame, err = run_child(runs['tmp'], 'async_cold', FLAME_RTC_CACHE=d, FLAME_RTC_ASYNC='1')
    n = runs['cold'][0]['compiles']
    assert disk(st) == (n, 0, n, n, 0) and st['jobs_queued'] == n, st
    assert listing(d) == runs['files']
    assert frame == runs['cold'][1]
    st, frame, err = run_child(runs['tmp'], 'async_warm', FLAME_RTC_CACHE=d, FLAME_RTC_ASYNC='1')
    assert disk(st) == (0, n, 0, 0, 0) and st['jobs_queued'] == n, st
    assert frame == runs['cold'][1]


def test_unusable_directory_warns_once_and_renders(runs):
    blocker = runs['tmp'] / 'blocker'
    blocker.write_text('a regular file')
    st, frame, err = run_child(runs['tmp'], 'unusable', FLAME_RTC_CACHE=str(blocker / 'cache'))     # (root ignores mode bits; nobody makes a directory inside a file)
    lines = [l for l in err.split('\n') if 'libflame_hip' in l]
    assert len(lines) == 1 and 'FLAME_RTC_CACHE' in lines[0] and 'without the kernel cache' in lines[0], err
    assert disk(st) == (runs['cold'][0]['compiles'], 0, 0, 0, 0), st
    assert frame == runs['cold'][1]
