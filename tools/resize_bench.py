#!/usr/bin/env python3
"""
The Lanczos downscale (fl_resize, cuburn_amd/csrc/resize.hip) alone, and the profile's `proxies` in the frame loop.

Kernels: HIP-event time per fl_resize call (fl_timings_detail[3]: both kernels), averaged over --calls calls after --warmup, each
on a fresh copy of a source buffer (the call swaps the buffers).  Cases: 1920x1080 -> 960x540, 3840x2160 -> 1920x1080, and
1920x1080 -> 240x135 (ratio 8: the widest tables).  Beside each: the time the library's own streaming copy (fl_measure_copy)
needs for the bytes the kernels cannot avoid moving — the source's picture area read once, the result's padded buffer written
once — and for the bytes the two passes do move (the intermediate of h rows by w2 columns written and read on top of that; halo
re-reads are served by the caches and not counted).  Run with FLAME_LANES=1.

Frame loop: the command line's one-ahead loop on cfg2 at 1080p with an mjpeg output, every frame handed to its module: frames/s
without a proxy, with one 960x540 proxy, and — with --parent-lib PATH, a build of the parent commit's library (FLAME_HIP_LIB) —
without a proxy on that library.  Each step runs in a process of its own; the loops alternate --rounds times.

    python3 tools/resize_bench.py [--calls 100] [--warmup 10] [--frames 200] [--rounds 3] [--parent-lib PATH] [--out PATH]

Writes profiles/resize_bench.json (with the sha256 of the library measured).
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

CASES = {'1080p_to_540p': (1920, 1080, 960, 540), '4k_to_1080p': (3840, 2160, 1920, 1080), '1080p_to_135p': (1920, 1080, 240, 135)}


def kernels(name, calls, warmup):
    from cuburn_amd import _lib, filters, render
    lib = _lib.load()
    w, h, w2, h2 = CASES[name]
    m = render.RenderManager(device=0, host_seed=42)
    try:
        din, dout = m.fb.set_dim(w, h), m.fb.calc_dim(w2, h2)
        src = np.random.RandomState(1).gamma(0.7, 0.3, (din.ah * din.astride, 4)).astype(np.float32)
        _lib.check(lib.fl_reserve(m.fb.ctx, w, h))

        def one():
            m.fb.write('front', src)
            filters.resize(m.fb, din, w2, h2)

        for _ in range(warmup):
            one()
        _lib.check(lib.fl_timings_reset(m.fb.ctx))
        for _ in range(calls):
            one()
        ms = (C.c_float * 6)()
        _lib.check(lib.fl_timings_detail(m.fb.ctx, C.byref(ms)))
        rate_ms = C.c_float()
        _lib.check(lib.fl_measure_copy(0, 1 << 30, 20, C.byref(rate_ms)))
    finally:
        m.fb.free()
    rate = 2.0 * (1 << 30) / (rate_ms.value * 1e-3)             # bytes read plus bytes written per second
    least = 16.0 * (w * h + dout.ah * dout.astride)
    moved = least + 2 * 16.0 * h * w2
    nxt, nyt = filters.resize_tables(w, w2)[1].shape[1], filters.resize_tables(h, h2)[1].shape[1]
    return dict(case=name, source=[w, h], result=[w2, h2], nxt=nxt, nyt=nyt, calls=calls, ms=round(ms[3] / calls, 4),
                copy_ms_for_the_least_bytes=round(least / rate * 1e3, 4), copy_ms_for_the_bytes_moved=round(moved / rate * 1e3, 4),
                copy_rate_TBps=round(rate / 1e12, 3))


def loop(proxy, nframes, warmup=5):
    """Frames/s of the one-ahead loop, every frame (and proxy frame) waited for and handed to its output module."""
    from cuburn_amd import configs, profile, render
    from cuburn_amd.__main__ import _one_ahead
    gnm, prof = configs.cfg2()
    prof = dict(prof, width=1920, height=1080, spp=2 ** 28 / (1920.0 * 1080.0), fps=25, output={'type': 'mjpeg'})
    if proxy:
        prof['proxies'] = [{'width': 960, 'height': 540}]
    gprof = profile.wrap(prof, gnm)
    mgr = render.RenderManager(device=0, host_seed=42)
    rdr = render.Renderer(gnm, gprof)
    mods = [px.out for px in getattr(rdr, 'proxies', [])]
    t0 = None
    times = [0.5] * (warmup + nframes)
    for idx, (evt, frame) in _one_ahead(lambda t: mgr.queue_frame(rdr, gnm, gprof, t), times):
        evt.synchronize()
        rdr.out.encode(frame)
        for mod, buf in zip(mods, getattr(evt, 'proxies', [])):
            mod.encode(buf)
        if idx == warmup:                                           # (frame warmup + 1 is queued already)
            t0 = time.perf_counter()
    dt = time.perf_counter() - t0
    sizes = [len(next(iter(mod.encode(None)[0].values())).read()) for mod in [rdr.out] + mods]
    mgr.fb.free()
    return dict(proxy=bool(proxy), frames=nframes, fps=round(nframes / dt, 2), ms_per_frame=round(1e3 * dt / nframes, 4), file_bytes=sizes)


def child(args, limit, env=None):
    """One step in a process of its own; its last line is the step's JSON."""
    print('step: ' + ' '.join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, timeout=limit)
    if r.returncode:
        raise SystemExit('step %s ended with status %d: nothing more is started' % (' '.join(args), r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-lib', metavar='PATH', help='a build of the parent commit\'s library, measured without a proxy')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'resize_bench.json'))
    ap.add_argument('--step', nargs='+', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        kind = args.step[0]
        res = kernels(args.step[1], args.calls, args.warmup) if kind == 'kernels' else loop(kind == 'loop_proxy', args.frames)
        print(json.dumps(res), flush=True)
        return
    import torch
    from cuburn_amd import _lib
    one = dict(os.environ, FLAME_LANES='1')
    common = ['--calls', str(args.calls), '--warmup', str(args.warmup), '--frames', str(args.frames)]
    rows = [child(['--step', 'kernels', name] + common, 300, one) for name in CASES]
    for row in rows:
        print(json.dumps(row), flush=True)
    loops = {'no_proxy': [], 'proxy_960x540': []}
    steps = [('no_proxy', 'loop_plain', None), ('proxy_960x540', 'loop_proxy', None)]
    if args.parent_lib:
        loops['parent_lib_no_proxy'] = []
        steps.append(('parent_lib_no_proxy', 'loop_plain', {'FLAME_HIP_LIB': os.path.abspath(args.parent_lib)}))
    for _ in range(args.rounds):
        for key, step, env in steps:
            loops[key].append(child(['--step', step] + common, 300, env))
            print(key, json.dumps(loops[key][-1]), flush=True)
    summary = dict((k, dict(fps=[r['fps'] for r in v], fps_median=float(np.median([r['fps'] for r in v])), frames=args.frames, runs=len(v),
                            file_bytes=v[-1]['file_bytes'])) for k, v in loops.items())
    out = dict(tool='tools/resize_bench.py', device=torch.cuda.get_device_name(0), lib_sha256=hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest(),
               kernels=rows, frame_loop=summary)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
