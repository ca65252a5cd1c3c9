#!/usr/bin/env python3
"""
The `de` filter (FL_FILT_DE, cuburn_amd/csrc/de_adaptive.hip) alone on real accumulators: HIP-event time per
fl_filter call (fl_timings_detail[3]), averaged over --calls calls after --warmup, each on a fresh copy of the
frame's accumulator after `yuv` (the filter works in place).  Cases: cfg2 at 1080p, cfg4 at 4K, and a sparse
cfg2 frame (2^22 samples at 1080p: little for the tile culling to cut); each at the genome's parameters and
at twice the radius.  Writes profiles/de_adaptive_bench.json (with the sha256 of the library measured).

    python3 tools/de_adaptive_bench.py [--calls 200] [--warmup 20] [--cases cfg2_1080p,...] [--out PATH]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cuburn_amd import _lib, configs, filters, profile, render  # noqa: E402

CASES = {
    'cfg2_1080p': lambda: configs.cfg2(),
    'cfg4_4k': lambda: configs.cfg4(),
    'cfg2_1080p_sparse': lambda: configs.cfg2(samples=2 ** 22),
}


def accumulator(m, gnm, gprof, tc=0.5):
    """The frame's accumulator after `yuv` (the input of the filters that follow it), on the host."""
    lib = _lib.load()
    dim = m.fb.set_dim(gprof.width, gprof.height)
    rdr = render.Renderer(gnm, gprof)
    td = gprof.frame_width(tc) / round(gprof.fps * gprof.duration)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(m.fb.ctx, C.byref(fid)))
    m._copy(rdr, gnm)
    g = rdr._handle(m.fb)
    _lib.check(lib.fl_interp(m.fb.ctx, g, dim.w, dim.h, tc - 0.5 * td, td))
    run = C.c_uint64()
    nsamples = float(gprof.spp(tc) * gprof.width * gprof.height)
    _lib.check(lib.fl_iterate(m.fb.ctx, g, dim.w, dim.h, nsamples, m.fuse, m.resolve_accum_mode(dim), C.byref(run)))
    _lib.check(lib.fl_filter(m.fb.ctx, _lib.FILT['yuv'], dim.w, dim.h, None, 0))
    return dim, m.fb.read('front', (dim.ah * dim.astride, 4), np.float32), run.value


def time_de(m, dim, src, vals, calls, warmup):
    lib = _lib.load()
    arr = np.asarray(vals, np.float32)

    def one():
        m.fb.write('front', src)
        _lib.check(lib.fl_filter(m.fb.ctx, _lib.FILT['de'], dim.w, dim.h, arr.ctypes.data, len(arr)))

    for _ in range(warmup):
        one()
    _lib.check(lib.fl_timings_reset(m.fb.ctx))
    for _ in range(calls):
        one()
    ms = (C.c_float * 6)()
    _lib.check(lib.fl_timings_detail(m.fb.ctx, C.byref(ms)))
    return ms[3] / calls


def spread_fraction(w, R, Rmin, curve):
    """Fraction of the accumulator's bins whose kernel radius is >= 1 px (those that the filter moves)."""
    w = w.astype(np.float64)
    h = np.clip(R * np.maximum(w, 1.0) ** -float(curve), Rmin, R)
    return float(((w > 0) & (np.floor(16 * h + 0.5) >= 16)).mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'de_adaptive_bench.json'))
    args = ap.parse_args()
    import torch
    rows = []
    for name in args.cases.split(','):
        gnm, prof = CASES[name]()
        m = render.RenderManager(device=0, host_seed=42)
        try:
            for mult in (1.0, 2.0):
                gprof = profile.wrap(dict(prof, filter_order=['de', 'logscale', 'smearclip'],
                                          filters={'de': {'radius': mult}}), gnm)
                if mult == 1.0:
                    dim, src, nrun = accumulator(m, gnm, gprof)
                vals = filters.DensityEstimation().scalars(gprof, gprof.filters.de, dim, 0.5)
                ms = time_de(m, dim, src, vals, args.calls, args.warmup)
                row = dict(case=name, radius_mult=mult, width=dim.w, height=dim.h, samples=int(nrun),
                           R=float(vals[0]), Rmin=float(vals[1]), curve=float(vals[2]), calls=args.calls, ms=round(ms, 4),
                           spread_bin_fraction=round(spread_fraction(src[:, 3], *map(float, vals)), 4))
                print(json.dumps(row), flush=True)
                rows.append(row)
        finally:
            m.fb.free()
    lib = _lib.LIB_PATH
    out = dict(tool='tools/de_adaptive_bench.py', device=torch.cuda.get_device_name(0),
               lib_sha256=hashlib.sha256(open(lib, 'rb').read()).hexdigest(), rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
