#!/usr/bin/env python3
"""
The `spatial` filter (fl_resample, cuburn_amd/csrc/resample.hip) at 1080p output, and what supersampling costs a frame.

Kernel: supersample 2, 3 and 4 at radius 1 (8, 11 and 14 taps per axis), HIP-event time per fl_resample call from fl_timings
over --calls calls after --warmup, on one stream lane (FLAME_LANES=1).  Twice: `warm`, the calls back to back (the source of
call k is what calls k-1 and k-2 left in the two buffers: up to supersample 2 they fit the 256 MiB Infinity Cache), and `cold`,
a 2 GiB streaming copy (fl_measure_copy) between the calls, so that every source bin comes from HBM.  Beside each: the bytes the
call must move, 16 * (astride_in * ah_in + astride_out * ah_out), the time those bytes take at the library's own streaming copy
rate (fl_measure_copy, 1 GiB each way), and the ratio.
Frame: cfg2 (1080p, 2^28 samples) through RenderManager.queue_frame at supersample 1 (the path of a profile without the key),
2 and 4, interleaved in rounds; frame time and the filters' share.  Writes profiles/spatial_bench.json (with the sha256 of the
library measured).

    python3 tools/bench_spatial.py [--calls 50] [--warmup 10] [--frames 12] [--rounds 3] [--kernel-only] [--out PATH]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

os.environ.setdefault('FLAME_LANES', '1')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
from cuburn_amd import _lib, configs, filters, profile, render  # noqa: E402

W, H, RADIUS = 1920, 1080, 1.0


def copy_rate(device=0):
    """Bytes per ms of the library's streaming copy: 1 GiB read + 1 GiB written per launch."""
    ms = C.c_float()
    _lib.check(_lib.load().fl_measure_copy(device, 1 << 30, 20, C.byref(ms)))
    return 2.0 * (1 << 30) / ms.value, ms.value


def filter_ms(m):
    ft = C.c_float()
    _lib.check(_lib.load().fl_timings(m.fb.ctx, None, None, C.byref(ft), None))
    return ft.value


def time_resample(m, ss, calls, warmup, cold):
    lib = _lib.load()
    din, dout = m.fb.calc_dim(ss * W, ss * H), m.fb.calc_dim(W, H)
    taps = filters.spatial_taps(RADIUS, ss)
    _lib.check(lib.fl_reserve(m.fb.ctx, din.w, din.h))
    src = np.random.RandomState(ss).uniform(0, 1, (din.ah * din.astride, 4)).astype(np.float32)
    one = lambda: _lib.check(lib.fl_resample(m.fb.ctx, W, H, ss, taps.ctypes.data, len(taps)))
    for _ in range(2):                                   # both buffers hold finite data (a call swaps them)
        m.fb.write('front', src)
        one()
    del src
    flush = C.c_float()
    for _ in range(warmup):
        one()
    _lib.check(lib.fl_timings_reset(m.fb.ctx))
    for _ in range(calls):
        if cold:
            _lib.check(lib.fl_ctx_sync(m.fb.ctx))
            _lib.check(lib.fl_measure_copy(m.fb.device, 1 << 30, 1, C.byref(flush)))
        one()
    nbytes = 16 * (din.astride * din.ah + dout.astride * dout.ah)
    return dict(ss=ss, radius=RADIUS, ntaps=len(taps), calls=calls, cold=bool(cold), bytes=nbytes,
                source_mib=round(16 * din.astride * din.ah / 2.0 ** 20, 1), ms=round(filter_ms(m) / calls, 4))


def run_frames(m, rdr, gnm, gprof, n):
    _lib.check(_lib.load().fl_timings_reset(m.fb.ctx))
    frame_ms = []
    for _ in range(n):
        evt, h = m.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
        frame_ms.append(evt.time())
    t = m.timings()
    return float(np.mean(frame_ms)), t['filter_ms'] / n, t['iter_ms'] / n, t['flush_ms'] / n


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=12, help='frames per supersample in all (split over the rounds)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true', help='skip the cfg2 frames')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'spatial_bench.json'))
    args = ap.parse_args()
    import torch
    rate, copy_ms = copy_rate()
    print(json.dumps(dict(copy_ms_per_gib_each_way=round(copy_ms, 4), copy_tb_per_s=round(rate * 1e3 / 1e12, 3))), flush=True)
    kernel, frames = [], []
    m = render.RenderManager(device=0, host_seed=42)
    try:
        for ss in (2, 3, 4):
            for cold in (False, True):
                row = time_resample(m, ss, args.calls, args.warmup, cold)
                row['copy_rate_ms'] = round(row['bytes'] / rate, 4)
                row['ms_over_copy_rate_ms'] = round(row['ms'] / row['copy_rate_ms'], 3)
                print(json.dumps(row), flush=True)
                kernel.append(row)
    finally:
        m.fb.free()
    m = render.RenderManager(device=0, host_seed=42)
    try:
        gnm, prof = configs.cfg2()
        state, acc = {}, {}
        per_round = (args.frames + args.rounds - 1) // args.rounds
        sss = () if args.kernel_only else (1, 2, 4)
        for ss in sss:
            gprof = profile.wrap(prof if ss == 1 else dict(prof, supersample=ss), gnm)
            state[ss] = (render.Renderer(gnm, gprof), gnm, gprof)
            run_frames(m, *state[ss], 3)
        for _ in range(args.rounds):
            for ss in sss:
                acc.setdefault(ss, []).append(run_frames(m, *state[ss], per_round))
        for ss in sss:
            a = np.array(acc[ss])
            row = dict(config='cfg2', ss=ss, filters=[f.name for f in state[ss][0].filts], frames=per_round * args.rounds,
                       frame_ms=round(float(a[:, 0].mean()), 4), frame_ms_rounds=[round(float(x), 4) for x in a[:, 0]],
                       filter_ms=round(float(a[:, 1].mean()), 4), iter_ms=round(float(a[:, 2].mean()), 4),
                       drain_ms=round(float(a[:, 3].mean()), 4))
            print(json.dumps(row), flush=True)
            frames.append(row)
    finally:
        m.fb.free()
    out = dict(tool='tools/bench_spatial.py', device=torch.cuda.get_device_name(0), width=W, height=H, lanes=os.environ['FLAME_LANES'],
               copy_ms_per_gib_each_way=round(copy_ms, 4), copy_bytes_per_ms=round(rate, 1),
               lib_sha256=hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest(), kernel=kernel, frames=frames)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
