"""What tests/test_gpu_rtc_async.py and its child processes share: the three genome structures and the frames they render."""
import numpy as np

from common import frame_times
from cuburn_amd import _lib, profile, render
import iter_forms as IF

TIMES = (0.25, 0.5, 0.75)
SEED = 23


def _plain():
    return IF.ring(3, mag=0.8, scale=0.32)


def _opacity():
    gnm, prof = IF.ring(3, posts=(1,), mag=0.8, scale=0.32)
    gnm['xforms'][sorted(gnm['xforms'])[1]]['opacity'] = 0.5
    return gnm, prof


def _chaos():
    gnm, prof = IF.ring(3, final='plain', mag=0.8, scale=0.32)
    keys = sorted(gnm['xforms'])
    table = [[1.0, 0.5, 2.0], [0.25, 1.0, 1.5], [2.0, 1.0, 0.5]]
    for i, k in enumerate(keys):
        gnm['xforms'][k]['chaos'] = dict((t, table[i][j]) for j, t in enumerate(keys))
    return gnm, prof


STRUCTURES = {'plain': _plain, 'opacity': _opacity, 'chaos': _chaos}


def render_frames(m, gnm, prof, mode, before_frame=None):
    """Three frames of one genome handle on `m`, each the three launches of iter_forms.gpu_launches (rounds 0, 10, 17).  Per frame:
    counters, packed cells and flushed accumulator per launch, RNG states and walker points at its end, and what the process-wide
    counters moved by.  before_frame(k, ctx, g, dim) runs before frame k's first launch."""
    lib = _lib.load()
    gprof = profile.wrap(prof, gnm)
    rdr = render.Renderer(gnm, gprof)
    g = rdr._handle(m.fb)
    m._copy(rdr, gnm)
    dim = m.fb.calc_dim(gprof.width, gprof.height)
    nbins, nwalk = dim.ah * dim.astride, m.fb.nslots * m.fb.nthreads
    frames = []
    for k, tc in enumerate(TIMES):
        if before_frame:
            before_frame(k, m.fb.ctx, g, dim)
        st0 = render.rtc_stats()
        ts, td = frame_times(gprof, tc)
        _lib.check(lib.fl_interp(m.fb.ctx, g, dim.w, dim.h, ts, td))
        _lib.check(lib.fl_debug_clear(m.fb.ctx, dim.w, dim.h, 1))
        out = dict(ctr=[], atom=[], front=[])
        r0 = 0
        for n in range(IF.LAUNCHES):
            f = IF.FUSE if n == 0 else 0
            _lib.check(lib.fl_debug_iter_launch(m.fb.ctx, g, dim.w, dim.h, r0, IF.NROUNDS + f, f, mode))
            ctr = np.zeros(4, np.uint64)
            _lib.check(lib.fl_debug_counters(m.fb.ctx, ctr.ctypes.data))
            out['ctr'].append(ctr)
            out['atom'].append(m.fb.read('atom', (nbins,), np.uint64))
            if mode == 1:
                _lib.check(lib.fl_debug_clear_hot(m.fb.ctx, dim.w, dim.h))
            _lib.check(lib.fl_debug_flush(m.fb.ctx, dim.w, dim.h))
            if mode == 1:
                _lib.check(lib.fl_debug_clear_hot(m.fb.ctx, dim.w, dim.h))
            out['front'].append(m.fb.read('front', (nbins, 4), np.float32))
            r0 += IF.NROUNDS + f
        out['rng'] = m.fb.read('seeds', (m.fb.nwalkers, 3), np.uint32)[:nwalk]
        out['pts'] = m.fb.read('points', (nwalk, 4), np.float32)
        st1 = render.rtc_stats()
        out['moved'] = dict((key, st1[key] - st0[key]) for key in st1)
        frames.append(out)
    del rdr
    return frames
