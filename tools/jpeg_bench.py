"""
JPEG stills: the host encoder against the device encoder on cfg2 at 1920x1080.

  python tools/jpeg_bench.py [--frames N] [--quality Q] [--out profiles/jpeg_bench.json] [--sweep] [--sampling 444|420]
  python tools/jpeg_bench.py --codec mjpeg [--frames N] [--out profiles/mjpeg_bench.json] [--sweep]      
  python tools/jpeg_bench.py --optimize [--frames N] [--out profiles/jpeg_opt_bench.json]                

Prints and writes, per frame:
  * the host Pillow encode (PILOutput.encode of a rendered frame, one thread);
  * the device encode by fl_timings_detail()[5] (HIP events around its four kernels) and, from a child process run under
    `rocprofv3 --kernel-trace --stats` (a run of its own, one stream lane), per kernel;
  * the stream's bytes;
  * frames/s of the command line's frame loop (__main__._one_ahead: frame k + 1 is queued before frame k is waited for and
    encoded) with the host JPEG, with the device JPEG, and with no encode at all;
  * --sweep: the device encode at other restart intervals (FLAME_JPEG_RI; a fresh context each).
  * --sampling 420: the device figures for 4:2:0 stills (the sweep then covers 1, 2, 4, 5, 8, 10).
  * --codec mjpeg: the loop with MJPEGOutput (4:2:0, frames appended to an AVI file) at quality 90 and 100, against device 4:4:4
    stills and no encode; bytes per frame 4:2:0 against 4:4:4; fl_timings_detail()[5] per frame; --sweep over the 4:2:0 intervals.
  * --optimize: the loop with and without `optimize` (Huffman tables from each frame's own statistics) for device
    4:4:4 stills at quality 100 and mjpeg at quality 90 and 100: frames/s, bytes per frame, fl_timings_detail()[5] per frame; per
    kernel from the rocprofv3 child for the optimised 4:4:4 stills and the optimised 4:2:0 frames at quality 90.
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
    if encode and hasattr(rdr.out, 'fps'):                             # a video output: its segment comes with the flush
        media, _ = rdr.out.encode(None)
        seg = next(iter(media.values()))
        res['file_bytes'] = len(seg.read())
        res['bytes'] = (res['file_bytes'] - 232) // (warmup + nframes) - 24      # per frame, less the chunk header and the index entry
        seg.close()
    frame = None if frame is None else np.array(frame)               # (the pinned ring goes with the manager)
    mgr.fb.free()
    return res, frame


def device_block(quality, sampling):
    block = {'type': 'jpeg', 'device': True, 'quality': quality}
    return block if sampling == '444' else dict(block, sampling=sampling)


def sweep(block, nframes, intervals, runs=1):
    """The device loop at every interval, `runs` times over the whole list (so that drift falls on all values alike); with more
    than one run the figures are lists, one entry per run, and `median_ms` is what the values are ranked by."""
    out = dict((ri, dict(jpeg_slot_ms_per_frame=[], fps=[])) for ri in intervals)
    for _ in range(runs):
        for ri in intervals:
            os.environ['FLAME_JPEG_RI'] = str(ri)
            r, _ = loop(block, nframes)
            out[ri]['jpeg_slot_ms_per_frame'].append(r['jpeg_slot_ms_per_frame'])
            out[ri]['fps'].append(r['fps'])
            out[ri]['bytes'] = r['bytes']
    del os.environ['FLAME_JPEG_RI']
    for v in out.values():
        if runs == 1:
            v['jpeg_slot_ms_per_frame'], v['fps'] = v['jpeg_slot_ms_per_frame'][0], v['fps'][0]
        else:
            v['runs'], v['median_ms'] = runs, float(np.median(v['jpeg_slot_ms_per_frame']))
    return out


def mjpeg(args):
    """--codec mjpeg: one run of every loop (`runs` says so next to the figures)."""
    n = args.frames
    res = dict(config='cfg2 1920x1080 2^28 samples', frames=n, runs=1)
    res['loop_no_encode'], _ = loop({'type': 'raw'}, n, encode=False)
    for q in (90, 100):
        res['loop_mjpeg_420_q%d' % q], _ = loop({'type': 'mjpeg', 'quality': q}, n)
        res['loop_device_jpeg_444_q%d' % q], _ = loop(device_block(q, '444'), n)
        res['bytes_per_frame_q%d' % q] = {'420': res['loop_mjpeg_420_q%d' % q]['bytes'], '444': res['loop_device_jpeg_444_q%d' % q]['bytes']}
    if args.sweep:
        for q in (90, 100):
            res['restart_interval_sweep_420_q%d' % q] = sweep({'type': 'mjpeg', 'quality': q}, max(20, n // 4), (1, 2, 4, 5, 8, 10),
                                                              args.sweep_runs)
    return res


def optimize(args):
    """--optimize: every loop once without and once with the key, the pairs next to each other."""
    n = args.frames
    res = dict(config='cfg2 1920x1080 2^28 samples', frames=n, runs=1)
    res['loop_no_encode'], _ = loop({'type': 'raw'}, n, encode=False)
    for name, block in (('device_jpeg_444_q100', device_block(100, '444')), ('mjpeg_420_q90', {'type': 'mjpeg', 'quality': 90}),
                        ('mjpeg_420_q100', {'type': 'mjpeg', 'quality': 100})):
        off, _ = loop(block, n)
        on, _ = loop(dict(block, optimize=True), n)
        res['loop_' + name], res['loop_' + name + '_optimize'] = off, on
        if not args.no_profile and name != 'mjpeg_420_q100':
            res['rocprofv3_kernels_' + name + '_optimize'] = profiled_kernels(block['quality'], 40, block.get('sampling', '420' if block['type'] == 'mjpeg' else '444'), True)
        res['optimize_' + name] = dict(bytes_ratio=on['bytes'] / float(off['bytes']), fps_ratio=on['fps'] / off['fps'],
                                       jpeg_slot_ms_added=on['jpeg_slot_ms_per_frame'] - off['jpeg_slot_ms_per_frame'])
    return res


def kernels_only(quality, nframes, sampling='444', optimize=False):
    """What the profiled child runs: device-encoded frames, nothing else."""
    mgr, rdr, gnm, gprof = setup(dict(device_block(quality, sampling), optimize=True) if optimize else device_block(quality, sampling))
    for _ in range(nframes):
        evt, frame = mgr.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
    mgr.fb.free()


def profiled_kernels(quality, nframes, sampling='444', optimize=False):
    """Average duration per launch of the JPEG kernels, from rocprofv3's kernel statistics of a child process."""
    out = tempfile.mkdtemp(prefix='jpeg_prof_', dir=os.environ.get('TMPDIR', '/tmp'))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'jpeg', '--',
           sys.executable, os.path.abspath(__file__), '--kernels-only', '--quality', str(quality), '--frames', str(nframes),
           '--sampling', sampling] + (['--optimize'] if optimize else [])
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
    ap.add_argument('--sweep', action='store_true', help='device encode at restart intervals 1, 2, 4, 8, 16, 21 (4:2:0: 1, 2, 4, 5, 8, 10)')
    ap.add_argument('--sweep-runs', type=int, default=1, help='repeat the whole sweep this many times (figures become lists)')
    ap.add_argument('--sampling', choices=['444', '420'], default='444', help='chroma sampling of the device stills')
    ap.add_argument('--codec', choices=['jpeg', 'mjpeg'], default='jpeg', help='mjpeg: the Motion-JPEG figures of DESIGN.md 4.10')
    ap.add_argument('--optimize', action='store_true', help='the figures of DESIGN.md 4.11: every loop with and without output.optimize')
    ap.add_argument('--no-profile', action='store_true', help='skip the rocprofv3 child')
    ap.add_argument('--kernels-only', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_only:
        return kernels_only(args.quality, args.frames, args.sampling, args.optimize)
    if args.codec == 'mjpeg' or args.optimize:
        text = json.dumps(optimize(args) if args.optimize else mjpeg(args), indent=1, sort_keys=True)
        print(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text + '\n')
        return
    q = args.quality
    res = dict(config='cfg2 1920x1080 2^28 samples', quality=q, frames=args.frames, sampling=args.sampling)
    if not args.no_profile:
        res['rocprofv3_kernels'] = profiled_kernels(q, 40, args.sampling)
        res['rocprofv3_jpeg_us_per_frame'] = sum(v['avg_us'] * v['calls'] for k, v in res['rocprofv3_kernels'].items() if 'jpeg' in k) / 40.0
    res['loop_no_encode'], frame = loop({'type': 'raw'}, args.frames, encode=False)
    res['loop_host_jpeg'], frame = loop({'type': 'jpeg', 'quality': q}, args.frames)
    res['loop_device_jpeg'], _ = loop(device_block(q, args.sampling), args.frames)
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
        res['restart_interval_sweep'] = sweep(device_block(q, args.sampling), max(20, args.frames // 4),
                                              (1, 2, 4, 8, 16, 21) if args.sampling == '444' else (1, 2, 4, 5, 8, 10), args.sweep_runs)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
