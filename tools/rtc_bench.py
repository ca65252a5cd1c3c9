#!/usr/bin/env python3
"""
What the per-genome kernels' compiles cost a workload of many genomes, and what FLAME_RTC_CACHE and FLAME_RTC_ASYNC change
(DESIGN.md 4.12).  Every setting runs in a fresh child process (the module cache is per process):

    baseline      neither switch, the PARENT commit's library (--parent-lib, loaded through FLAME_HIP_LIB); skipped without it
    none          neither switch, this library
    async         FLAME_RTC_ASYNC=1
    cold          FLAME_RTC_CACHE=<an empty directory>
    warm          the same directory again
    async_warm    both switches, the same directory

The child renders --genomes structurally distinct genomes made from configs.cfg2 (other variations per xform), one 256 x 144
frame each through the shim (Renderer + queue_frame), preparing genome k+1 before it waits for genome k's frame when the
asynchronous mode is on, as the command line does; then the first ten frames of cfg2 itself at 1080p.  It reports the wall time
per genome, the time to the first finished frame, per cfg2 frame the wall time, the frame's HIP-event time, the iterate kernel's
HIP-event time and which kernel ran it, and the process-wide counters (fl_rtc_stats); the parent adds the child's wall time
from start to exit.  The parent also times one hipRTC compile
of cfg2's four-wave binned kernel per hoist budget.  Writes profiles/rtc_bench.json (with the libraries' sha256 and the number
of runs).

    python3 tools/rtc_bench.py [--runs 2] [--genomes 6] [--parent-lib PATH] [--out PATH]
"""
import argparse
import copy
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

VARIATIONS = ['linear', 'spherical', 'swirl', 'sinusoidal', 'horseshoe', 'polar', 'handkerchief', 'heart', 'disc', 'spiral',
              'hyperbolic', 'diamond', 'ex', 'julia', 'bent', 'fisheye']
CHILD_TIMEOUT = 420


def load_lib():
    """The library named by FLAME_HIP_LIB; entry points the parent commit's build does not have are left out of the binding."""
    from cuburn_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH, mode=C.RTLD_GLOBAL)
    missing = [n for n in _lib._SIGS if not hasattr(raw, n)]
    for n in missing:
        del _lib._SIGS[n]
    return _lib.load(), missing


def genomes(n):
    from cuburn_amd import configs
    out = []
    for i in range(n):
        gnm, prof = configs.cfg2(samples=2 ** 21)
        gnm = copy.deepcopy(gnm)
        for j, k in enumerate(sorted(gnm['xforms'])):
            a, b = VARIATIONS[(2 * i + j) % len(VARIATIONS)], VARIATIONS[(2 * i + j + 5) % len(VARIATIONS)]
            gnm['xforms'][k]['variations'] = {a: {'weight': 0.7}, b: {'weight': 0.3}} if a != b else {a: {'weight': 1.0}}
        out.append((gnm, dict(prof, width=256, height=144, spp=2 ** 21 / (256 * 144))))
    return out


def child(args):
    t_start = time.perf_counter()
    lib, missing = load_lib()
    from cuburn_amd import _lib, configs, profile, render
    use_async = not missing and render.async_compile()
    stats = (lambda: render.rtc_stats()) if not missing else (lambda: {})
    m = render.RenderManager(device=0, nslots=1024, host_seed=42)
    t_ctx = time.perf_counter()
    res = dict(ctx_s=t_ctx - t_start, genomes=[], cfg2=[])
    work = [(render.Renderer(g, profile.wrap(p, g)), g, profile.wrap(p, g)) for g, p in genomes(args.genomes)]
    t0 = time.perf_counter()
    if use_async:
        m.prepare(work[0][0], work[0][2], 0.5)
    for k, (rdr, gnm, gprof) in enumerate(work):
        m.timings_reset()
        t = time.perf_counter()
        evt, h = m.queue_frame(rdr, gnm, gprof, 0.5)
        if use_async and k + 1 < len(work):
            m.prepare(work[k + 1][0], work[k + 1][2], 0.5)           # the next genome's compile runs while this frame is waited for
        evt.synchronize()
        now = time.perf_counter()
        if k == 0:
            res['first_frame_s'] = now - t0
        lt = m.timings()
        res['genomes'].append(dict(wall_s=now - t, spec_launches=lt['spec_launches'], interp_launches=lt['interp_launches']))
    res['genomes_total_s'] = time.perf_counter() - t0
    res['stats_after_genomes'] = stats()
    m.fb.free()
    # cfg2 as bench.py renders it, first ten frames of a fresh context
    gnm, prof = configs.cfg2()
    gprof = profile.wrap(prof, gnm)
    m = render.RenderManager(device=0, host_seed=42)
    rdr = render.Renderer(gnm, gprof)
    t0 = time.perf_counter()
    for k in range(10):
        m.timings_reset()
        t = time.perf_counter()
        evt, h = m.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
        now = time.perf_counter()
        lt = m.timings()
        res['cfg2'].append(dict(wall_ms=1e3 * (now - t), frame_ms=evt.time(), iter_ms=lt['iter_ms'],
                                kernel='per-genome' if lt['spec_launches'] and not lt['interp_launches'] else
                                'interpreter' if lt['interp_launches'] and not lt['spec_launches'] else 'both'))
        if k == 0:
            res['cfg2_first_frame_s'] = now - t0
    res['cfg2_total_s'] = time.perf_counter() - t0
    # asynchronous mode: how many frames run the interpreter kernel before the per-genome kernel takes over (at most 2000 more)
    if use_async and res['cfg2'][-1]['kernel'] != 'per-genome':
        for k in range(10, 2010):
            m.timings_reset()
            evt, h = m.queue_frame(rdr, gnm, gprof, 0.5)
            evt.synchronize()
            if m.timings()['spec_launches']:
                res['cfg2_switch'] = dict(frame=k, s=time.perf_counter() - t0)
                break
    res['slots'], res['waves_per_slot'] = m.fb.nslots, m.fb.nw
    res['stats'] = stats()
    m.fb.free()
    print('RTC_BENCH ' + json.dumps(res), flush=True)


def run_child(args, env_extra, lib=None):
    env = dict(os.environ)
    for k in ('FLAME_RTC', 'FLAME_RTC_FLAGS', 'FLAME_RTC_CACHE', 'FLAME_RTC_ASYNC', 'FLAME_RTC_DUMP', 'FLAME_HIP_LIB'):
        env.pop(k, None)
    env.update(env_extra)
    if lib:
        env['FLAME_HIP_LIB'] = lib
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--genomes', str(args.genomes)], capture_output=True,
                       text=True, timeout=CHILD_TIMEOUT, env=env)
    process_s = time.perf_counter() - t             # imports, two contexts, the work, and the exit (which joins the compile thread)
    if r.returncode != 0:
        raise RuntimeError('child failed (%d): %s' % (r.returncode, r.stderr[-3000:]))
    line = [l for l in r.stdout.split('\n') if l.startswith('RTC_BENCH ')][-1]
    return dict(json.loads(line[len('RTC_BENCH '):]), process_s=process_s)


def compile_times():
    """One hipRTC compile of cfg2's four-wave binned kernel per hoist budget (needs no device), seconds."""
    import numpy as np
    from cuburn_amd import _lib, configs
    from cuburn_amd.packer import GenomePacker
    lib = _lib.load()
    pk = GenomePacker(configs.cfg2()[0])
    prog, ops = np.ascontiguousarray(pk.prog, np.int32), np.ascontiguousarray(pk.ops_array, np.int32)
    log = C.create_string_buffer(8192)
    out = {}
    for budget in ('default', '7', '5', '0'):
        if budget == 'default':
            os.environ.pop('FLAME_RTC_FLAGS', None)
        else:
            os.environ['FLAME_RTC_FLAGS'] = '-DFL_HOIST_BUDGET=' + budget
        t = time.perf_counter()
        rc = lib.fl_rtc_compile_check(prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), 4, 0, 1, log, len(log))
        out[budget] = round(time.perf_counter() - t, 3) if rc == 0 else None
    os.environ.pop('FLAME_RTC_FLAGS', None)
    return out


def summary(rows):
    """Means over the runs of one setting."""
    import numpy as np
    mean = lambda xs: round(float(np.mean(xs)), 4)
    out = dict(runs=len(rows),
               genome_wall_s=mean([g['wall_s'] for r in rows for g in r['genomes']]),
               genomes_total_s=mean([r['genomes_total_s'] for r in rows]),
               first_frame_s=mean([r['first_frame_s'] for r in rows]),
               cfg2_first_frame_s=mean([r['cfg2_first_frame_s'] for r in rows]),
               cfg2_ten_frames_s=mean([r['cfg2_total_s'] for r in rows]),
               process_s=mean([r['process_s'] for r in rows]))
    for kernel in ('interpreter', 'per-genome'):
        fr = [f for r in rows for f in r['cfg2'][1:] if f['kernel'] == kernel]       # (frame 0 carries the buffers' allocation)
        out['cfg2_%s_frames' % kernel.replace('-', '_')] = dict(
            n=len(fr), frame_ms=mean([f['frame_ms'] for f in fr]) if fr else None, iter_ms=mean([f['iter_ms'] for f in fr]) if fr else None,
            wall_ms=mean([f['wall_ms'] for f in fr]) if fr else None)
    out['genomes_on_interpreter'] = sum(1 for r in rows for g in r['genomes'] if g['interp_launches'] and not g['spec_launches'])
    if any('cfg2_switch' in r for r in rows):
        out['cfg2_switch'] = [r.get('cfg2_switch') for r in rows]
    out['stats'] = rows[-1].get('stats')
    return out


def sha256(path):
    return hashlib.sha256(open(path, 'rb').read()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--genomes', type=int, default=6)
    ap.add_argument('--parent-lib', default=None, help="the parent commit's libflame_hip.so: the baseline")
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'rtc_bench.json'))
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    from cuburn_amd import _lib
    rows = {}
    for run in range(args.runs):
        d = tempfile.mkdtemp(prefix='rtc_bench_')
        try:
            settings = [('none', {}, None), ('async', dict(FLAME_RTC_ASYNC='1'), None), ('cold', dict(FLAME_RTC_CACHE=d), None),
                        ('warm', dict(FLAME_RTC_CACHE=d), None), ('async_warm', dict(FLAME_RTC_CACHE=d, FLAME_RTC_ASYNC='1'), None)]
            if args.parent_lib:
                settings.insert(0, ('baseline', {}, os.path.abspath(args.parent_lib)))
            for name, env, lib in settings:
                res = run_child(args, env, lib)
                rows.setdefault(name, []).append(res)
                print(run, name, json.dumps(dict(genomes_total_s=round(res['genomes_total_s'], 3), first_frame_s=round(res['first_frame_s'], 3),
                                                 cfg2_first_frame_s=round(res['cfg2_first_frame_s'], 3), cfg2_total_s=round(res['cfg2_total_s'], 3), process_s=round(res['process_s'], 3),
                                                 cfg2_kernels=[f['kernel'][0] for f in res['cfg2']], stats=res['stats'])), flush=True)
            files = sorted(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
        finally:
            shutil.rmtree(d, ignore_errors=True)
    import torch
    out = dict(tool='tools/rtc_bench.py', device=torch.cuda.get_device_name(0), runs=args.runs, genomes=args.genomes,
               lib_sha256=sha256(_lib.LIB_PATH), parent_lib_sha256=sha256(args.parent_lib) if args.parent_lib else None,
               cache_files=len(files), cache_file_bytes=files, compile_s_by_hoist_budget=compile_times(),
               settings=dict((name, summary(r)) for name, r in rows.items()), raw=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out['settings'], indent=1))


if __name__ == '__main__':
    main()
