"""
JPEG stills: the host encoder against the device encoder on cfg2 at 1920x1080.

  python tools/jpeg_bench.py [--frames N] [--quality Q] [--out profiles/jpeg_bench.json] [--sweep]

Prints and writes, per frame:
  * the host Pillow encode (PILOutput.encode of a rendered frame, one thread);
  * the device encode by fl_timings_detail()[5] (HIP events around its four kernels) and, from a child process run under
    `rocprofv3 --kernel-trace --stats` (a run of its own, one stream lane), per kernel;
  * the stream's bytes;
  * frames/s of the command line's frame loop (__main__._one_ahead: frame k + 1 is queued before frame k is waited for and
    encoded) with the host JPEG, with the device JPEG, and with no encode at all;
  * --sweep: the device encode at other restart intervals (FLAME_JPEG_RI; a fresh context each).
There is no fallback: without a GPU the tool fails.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np                                                    # noqa: E402


def setup(block, host_seed=42):
    from cuburn_amd import configs, profile, render
    gnm, prof = configs.cfg2()
    gprof = profile.wrap(dict(prof, output=block), gnm)
    mgr = render.RenderManager(device=0, host_seed=host_seed)
    return mgr, render.Renderer(gnm, gprof), gnm, gprof


def loop(block, nframes, encode=True, warmup=3):
    """Frames/s of the one-ahead loop, each frame waited for and (encode) handed to the output module; also the last media."""
    from cuburn_amd.__main__ import _one_ahead
    mgr, rdr, gnm, gprof = setup(block)
    media, t0 = None, None
    times = [0.5] * (warmup + nframes)
    mgr.timings_reset()
    for idx, (evt, frame) in _one_ahead(lambda t: mgr.queue_frame(rdr, gnm, gprof, t), times):
        evt.synchronize()
        if encode:
            media, _ = rdr.out.encode(frame)
        if idx == warmup:                                             # (frame warmup + 1 is queued already)
            mgr.timings_reset()
            t0 = time.perf_counter()
    dt = time.perf_counter() - t0
    tm = mgr.timings()
    res = dict(fps=nframes / dt, ms_per_frame=1e3 * dt / nframes, jpeg_slot_ms_per_frame=tm['jpeg_ms'] / (nframes - 1))
    if media:
        res['bytes'] = len(next(iter(media.values())).getvalue())
    frame = None if frame is None else np.array(frame)               # (the pinned ring goes with the manager)
    mgr.fb.free()
    return res, frame


def kernels_only(quality, nframes):
    """What the profiled child runs: device-encoded frames, nothing else."""
    mgr, rdr, gnm, gprof = setup({'type': 'jpeg', 'device': True, 'quality': quality})
    for _ in range(nframes):
        evt, frame = mgr.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
    mgr.fb.free()


def profiled_kernels(quality, nframes):
    """Average duration per launch of the JPEG kernels, from rocprofv3's kernel statistics of a child process."""
    out = tempfile.mkdtemp(prefix='jpeg_prof_', dir=os.environ.get('TMPDIR', '/tmp'))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'jpeg', '--',
           sys.executable, os.path.abspath(__file__), '--kernels-only', '--quality', str(quality), '--frames', str(nframes)]
    subprocess.run(cmd, check=True, env=dict(os.environ, FLAME_LANES='1'), stdout=subprocess.DEVNULL, timeout=600)
    found = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if not found:
        raise RuntimeError('rocprofv3 wrote no kernel statistics under %s' % out)
    rows = {}
    for r in csv.DictReader(open(found[0])):
        if 'jpeg' in r['Name'] or 'f32_to_yuv' in r['Name']:
            rows[r['Name']] = dict(calls=int(r['Calls']), avg_us=float(r['AverageNs']) / 1e3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--quality', type=int, default=100)
    ap.add_argument('--out', default=None, help='also write the figures to this JSON file')
    ap.add_argument('--sweep', action='store_true', help='device encode at restart intervals 1, 2, 4, 8, 16, 21')
    ap.add_argument('--no-profile', action='store_true', help='skip the rocprofv3 child')
    ap.add_argument('--kernels-only', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_only:
        return kernels_only(args.quality, args.frames)
    q = args.quality
    res = dict(config='cfg2 1920x1080 2^28 samples', quality=q, frames=args.frames)
    if not args.no_profile:
        res['rocprofv3_kernels'] = profiled_kernels(q, 40)
        res['rocprofv3_jpeg_us_per_frame'] = sum(v['avg_us'] * v['calls'] for k, v in res['rocprofv3_kernels'].items() if 'jpeg' in k) / 40.0
    res['loop_no_encode'], frame = loop({'type': 'raw'}, args.frames, encode=False)
    res['loop_host_jpeg'], frame = loop({'type': 'jpeg', 'quality': q}, args.frames)
    res['loop_device_jpeg'], _ = loop({'type': 'jpeg', 'device': True, 'quality': q}, args.frames)
    # the host encoder alone, on the last frame of the host loop
    from cuburn_amd import output
    pil = output.PILOutput('jpeg', quality=q)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        media, _ = pil.encode(frame)
        t.append(1e3 * (time.perf_counter() - t0))
    res['host_pillow_encode_ms'] = dict(min=min(t), median=float(np.median(t)))
    res['host_pillow_bytes'] = len(media['.jpg'].getvalue())
    if args.sweep:
        res['restart_interval_sweep'] = {}
        for ri in (1, 2, 4, 8, 16, 21):
            os.environ['FLAME_JPEG_RI'] = str(ri)
            r, _ = loop({'type': 'jpeg', 'device': True, 'quality': q}, max(20, args.frames // 4))
            res['restart_interval_sweep'][ri] = dict(jpeg_slot_ms_per_frame=r['jpeg_slot_ms_per_frame'], bytes=r['bytes'], fps=r['fps'])
        del os.environ['FLAME_JPEG_RI']
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
