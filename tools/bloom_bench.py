#!/usr/bin/env python3
"""
The `bloom` filter (FL_FILT_BLOOM, cuburn_amd/csrc/bloom.hip) alone on real frames: HIP-event time per fl_filter call
(fl_timings_detail[3]: both kernels), averaged over --calls calls after --warmup, each on a fresh copy of the frame's buffer
after `yuv` and `logscale` (the filter works in place).  Cases: cfg2 at 1080p and cfg4 at 4K, each at the default radius and at
the largest the size allows (R = 384 bins).  Beside each: the time the library's own streaming copy (fl_measure_copy) needs for
the bytes the two kernels cannot avoid moving: the float4 buffer five times over (rows: front read, side written; columns:
side read, front read and written; halo re-reads are served by the caches and not counted).
Run with FLAME_LANES=1.  Writes profiles/bloom_bench.json (with the sha256 of the library measured).

Per-kernel times come from a kernel trace in a run of its own, one case per run:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bloom -- python3 tools/bloom_bench.py --cases 4k_default --calls 20 --out /dev/null
    python3 tools/bloom_bench.py --kernel-stats 4k_default=DIR/bloom_kernel_stats.csv ...

    python3 tools/bloom_bench.py [--calls 100] [--warmup 10] [--cases 1080p_default,...] [--out PATH]
"""
import argparse
import csv
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from cuburn_amd import _lib, configs, filters, profile, render  # noqa: E402

MAX_SIGMA = filters.Bloom.max_reach / 3.0
CASES = {      # name: (config, radius factor of the profile; None: the largest)
    '1080p_default': ('cfg2', 1.0),
    '1080p_max': ('cfg2', None),
    '4k_default': ('cfg4', 1.0),
    '4k_max': ('cfg4', None),
}
ORDER = ['logscale', 'bloom', 'colorclip']


def tone_mapped(m, gnm, gprof, tc=0.5):
    """The frame's buffer after `yuv` and `logscale` (the input of `bloom` in ORDER), on the host."""
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
    for filt in rdr.filts[:2]:
        assert filt.name in ('yuv', 'logscale'), filt.name
        filt.apply(m.fb, gprof, getattr(gprof.filters, filt.name), dim, tc)
    return dim, m.fb.read('front', (dim.ah * dim.astride, 4), np.float32)


def time_bloom(m, dim, src, vals, calls, warmup):
    lib = _lib.load()
    arr = np.asarray(vals, np.float32)

    def one():
        m.fb.write('front', src)
        _lib.check(lib.fl_filter(m.fb.ctx, _lib.FILT['bloom'], dim.w, dim.h, arr.ctypes.data, len(arr)))

    for _ in range(warmup):
        one()
    _lib.check(lib.fl_timings_reset(m.fb.ctx))
    for _ in range(calls):
        one()
    ms = (C.c_float * 6)()
    _lib.check(lib.fl_timings_detail(m.fb.ctx, C.byref(ms)))
    return ms[3] / calls


def copy_rate(device):
    """Bytes per second of the library's streaming copy, counting the bytes read plus the bytes written."""
    ms = C.c_float()
    _lib.check(_lib.load().fl_measure_copy(device, 1 << 30, 20, C.byref(ms)))
    return 2.0 * (1 << 30) / (ms.value * 1e-3)


def kernel_times(path):
    """{kernel: average microseconds} of the two bloom kernels from a rocprofv3 kernel_stats.csv."""
    out = {}
    for r in csv.DictReader(open(path)):
        for k in ('k_bloom_rows', 'k_bloom_cols'):
            if k in r['Name']:
                out[k + '_us'] = round(float(r['AverageNs']) / 1e3, 2)
                out[k + '_calls'] = int(r['Calls'])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--kernel-stats', action='append', default=[], metavar='CASE=CSV')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bloom_bench.json'))
    args = ap.parse_args()
    import torch
    traced = dict(s.split('=', 1) for s in args.kernel_stats)
    rate = copy_rate(0)
    rows = []
    for name in args.cases.split(','):
        cfg, factor = CASES[name]
        gnm, prof = configs.CONFIGS[cfg]()
        if factor is None:
            factor = MAX_SIGMA / (12.0 * prof['width'] / 1920.0)
        gprof = profile.wrap(dict(prof, filter_order=ORDER, filters={'bloom': {'radius': factor}}), gnm)
        m = render.RenderManager(device=0, host_seed=42)
        try:
            dim, src = tone_mapped(m, gnm, gprof)
            vals = filters.Bloom().scalars(gprof, gprof.filters.bloom, dim, 0.5)
            ms = time_bloom(m, dim, src, vals, args.calls, args.warmup)
        finally:
            m.fb.free()
        nbytes = 16.0 * dim.ah * dim.astride
        moved = 5 * nbytes                       # rows: one read, one write; columns: two reads, one write
        row = dict(case=name, width=dim.w, height=dim.h, ah=dim.ah, astride=dim.astride, threshold=float(vals[0]),
                   strength=float(vals[1]), reach=len(vals) - 3, taps=2 * (len(vals) - 3) + 1, calls=args.calls, ms=round(ms, 4),
                   bins_above_threshold=round(float((src[:, 3] > vals[0]).mean()), 4),
                   copy_ms_for_the_bytes_moved=round(moved / rate * 1e3, 4), copy_rate_TBps=round(rate / 1e12, 3))
        if name in traced:
            row.update(kernel_times(traced[name]))
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = dict(tool='tools/bloom_bench.py', device=torch.cuda.get_device_name(0), lanes=os.environ.get('FLAME_LANES'),
               lib_sha256=hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest(), rows=rows)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
