#!/usr/bin/env python3
"""
What xform chaos (flam3 xaos) costs the iterate kernel: cfg2 at 1080p, 2^28 samples, without a `chaos` key, with a full
3 x 3 table whose entries are all non-zero, and with the same table with a zero diagonal (no xform follows itself), in
ONE process on one stream lane (FLAME_LANES=1: kernels un-overlapped).  Per case, over --frames frames after --warmup: the per-genome iterate kernel's HIP-event time per
frame (fl_timings_detail[0]), the tile accumulate's, and the frame time of queue_frame; plus the registers and code size of the
four-wave binned kernel as hipRTC compiles it (dynamic LDS: +2 KB per 256 walkers for a chaos kernel, iter_lds_bytes).  The
cases are interleaved in rounds so that clock drift of the box spreads over all of them.  Writes
profiles/chaos_bench.json (with the sha256 of the library measured).

    python3 tools/chaos_bench.py [--frames 60] [--warmup 10] [--rounds 3] [--out PATH]
"""
import argparse
import copy
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

os.environ.setdefault('FLAME_LANES', '1')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
from cuburn_amd import _lib, configs, profile, render  # noqa: E402
from cuburn_amd.packer import GenomePacker  # noqa: E402

FULL = [[1.0, 0.5, 2.0], [0.25, 1.0, 1.0], [1.0, 3.0, 0.5]]
CASES = [('keyless', None), ('full_table', FULL),
         ('zero_diagonal', [[0.0 if p == n else v for n, v in enumerate(row)] for p, row in enumerate(FULL)])]


def genome(table):
    gnm, prof = configs.cfg2()
    gnm = copy.deepcopy(gnm)
    keys = sorted(gnm['xforms'])
    if table is not None:
        for p, k in enumerate(keys):
            gnm['xforms'][k]['chaos'] = dict(zip(keys, table[p]))
    return gnm, prof


def kernel_resources(gnm):
    """Registers of the four-wave binned per-genome kernel (hipRTC needs no launch)."""
    readelf = '/opt/rocm/lib/llvm/bin/llvm-readelf'
    d = tempfile.mkdtemp()
    os.environ['FLAME_RTC_DUMP'] = d
    try:
        pk = GenomePacker(gnm)
        prog = np.ascontiguousarray(pk.prog, np.int32)
        ops = np.ascontiguousarray(pk.ops_array, np.int32)
        log = C.create_string_buffer(8192)
        rc = _lib.load().fl_rtc_compile_check(prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), 4, 0, 1, log, len(log))
        if rc or not os.path.exists(readelf):
            return {}
        notes = subprocess.run([readelf, '--notes', os.path.join(d, 'k_iter_spec.co')], capture_output=True, text=True).stdout
        num = lambda key: int(re.search(r'\.' + key + r':\s+(\d+)', notes).group(1))
        sect = subprocess.run([readelf, '-S', os.path.join(d, 'k_iter_spec.co')], capture_output=True, text=True).stdout
        text = int(re.search(r'\.text\s+PROGBITS\s+\S+\s+\S+\s+([0-9a-f]+)', sect).group(1), 16)
        return dict(vgpr=num('vgpr_count'), sgpr=num('sgpr_count'), sgpr_spill=num('sgpr_spill_count'),
                    vgpr_spill=num('vgpr_spill_count'), scratch=num('private_segment_fixed_size'), text_bytes=text,
                    swap_lds_bytes_per_256_walkers=2 * (4 if len(pk.prog) > 8 else 3) * 256 * 4)
    finally:
        del os.environ['FLAME_RTC_DUMP']


def run_frames(m, rdr, gnm, gprof, n):
    lib = _lib.load()
    _lib.check(lib.fl_timings_reset(m.fb.ctx))
    frame_ms = []
    for _ in range(n):
        evt, h = m.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
        frame_ms.append(evt.time())
    ms = (C.c_float * 6)()
    _lib.check(lib.fl_timings_detail(m.fb.ctx, C.byref(ms)))
    stats = (C.c_uint32 * 4)()
    _lib.check(lib.fl_launch_stats(m.fb.ctx, C.byref(stats)))
    assert stats[0] > 0 and stats[1] == 0, 'the per-genome kernel did not run'
    return ms[0] / n, ms[1] / n, float(np.mean(frame_ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--frames', type=int, default=60, help='frames per case in all (split over the rounds)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'chaos_bench.json'))
    args = ap.parse_args()
    import torch
    m = render.RenderManager(device=0, host_seed=42)
    per_round = (args.frames + args.rounds - 1) // args.rounds
    state, acc = {}, {}
    try:
        for name, table in CASES:
            gnm, prof = genome(table)
            gprof = profile.wrap(prof, gnm)
            state[name] = (render.Renderer(gnm, gprof), gnm, gprof)
            run_frames(m, *state[name], args.warmup)
        for rnd in range(args.rounds):
            for name, _ in CASES:
                acc.setdefault(name, []).append(run_frames(m, *state[name], per_round))
        slots, nw = m.fb.nslots, m.fb.nw
    finally:
        m.fb.free()
    rows = []
    for name, table in CASES:
        a = np.array(acc[name])
        row = dict(case=name, chaos=table, frames=per_round * args.rounds, iter_ms=round(float(a[:, 0].mean()), 4),
                   iter_ms_rounds=[round(float(x), 4) for x in a[:, 0]], accum_ms=round(float(a[:, 1].mean()), 4),
                   frame_ms=round(float(a[:, 2].mean()), 4), kernel=kernel_resources(genome(table)[0]))
        rows.append(row)
    base = rows[0]
    for row in rows:
        row['iter_vs_keyless'] = round(row['iter_ms'] / base['iter_ms'], 4)
        row['frame_vs_keyless'] = round(row['frame_ms'] / base['frame_ms'], 4)
        print(json.dumps(row), flush=True)
    out = dict(tool='tools/chaos_bench.py', device=torch.cuda.get_device_name(0), width=1920, height=1080, samples=2 ** 28,
               slots=slots, waves_per_slot=nw, lanes=os.environ['FLAME_LANES'],
               lib_sha256=hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest(), rows=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
