"""
Lossless WebP: the device encoder against the same loop encoding nothing and against the device PNG, GIF and Motion-JPEG, on cfg2
at 1920x1080 (2^28 samples) and at 480x270 (the same samples per pixel).

  python tools/webp_bench.py [--frames N] [--rounds R] [--no-profile] [--out profiles/webp_bench.json]

Every step is a process of its own (a render manager, its frames, nothing else), started one after the other; the loop steps are
repeated R times over in the same order and the median of the rounds is the figure to quote.  Prints and writes:
  * per size, frames/s of the command line's frame loop (__main__._one_ahead: frame k + 1 is queued before frame k is waited for
    and handed to the output module) with `webp`, `webp_alpha`, `png` (the device PNG), `gif`, `mjpeg` and `none` (the 8-bit raw
    frame, copied and dropped), and the encode by fl_timings_detail()[5] (HIP events around its kernels);
  * per size, the bytes of 8 different frames as one-frame WebP files, as the device PNG's files of the same pixels (fl_png_encode)
    and as Pillow's save(lossless=True) of the same pixels, and what the stream's parts weigh (sub-images, group headers, pixels);
  * per size, the WebP kernels' time per launch from a child run under `rocprofv3 --kernel-trace --stats` with one stream lane.
There is no fallback: without a GPU the tool fails.
"""
import argparse
import csv
import glob
import io
import json
import os
import re
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = {'1080p': (1920, 1080), '270p': (480, 270)}
BLOCKS = dict(none={'type': 'raw'}, mjpeg={'type': 'mjpeg'}, gif={'type': 'gif'}, png={'type': 'png', 'encoder': 'device'},
              webp={'type': 'webp'}, webp_alpha={'type': 'webp', 'alpha': True})
ORDER = ('webp', 'webp_alpha', 'png', 'gif', 'mjpeg', 'none')


def setup(kind, size, host_seed=42):
    from cuburn_amd import configs, profile, render
    w, h = SIZES[size]
    gnm, prof = configs.cfg2()
    gprof = profile.wrap(dict(prof, width=w, height=h, spp=2 ** 28 / (1920.0 * 1080.0), fps=25, output=BLOCKS[kind]), gnm)
    mgr = render.RenderManager(device=0, host_seed=host_seed)
    return mgr, render.Renderer(gnm, gprof), gnm, gprof


def loop(kind, size, nframes, warmup=3):
    """Frames/s of the one-ahead loop, each frame waited for and (but for `none`) handed to the output module."""
    from cuburn_amd.__main__ import _one_ahead
    mgr, rdr, gnm, gprof = setup(kind, size)
    t0 = None
    times = [0.5] * (warmup + nframes)
    mgr.timings_reset()
    for idx, (evt, frame) in _one_ahead(lambda t: mgr.queue_frame(rdr, gnm, gprof, t), times):
        evt.synchronize()
        if kind != 'none':
            rdr.out.encode(frame)
        if idx == warmup:                                             # (frame warmup + 1 is queued already)
            mgr.timings_reset()
            t0 = time.perf_counter()
    dt = time.perf_counter() - t0
    tm = mgr.timings()
    res = dict(fps=nframes / dt, ms_per_frame=1e3 * dt / nframes, encode_slot_ms_per_frame=tm['encode_ms'] / (nframes - 1))
    if kind != 'none':
        media, _ = rdr.out.encode(None)
        if media:                                                     # (a stills output has handed its files over frame by frame)
            res['file_bytes_per_frame'] = len(next(iter(media.values())).read()) / float(warmup + nframes)
    mgr.fb.free()
    return res


def file_bytes(kind, size, nframes=8):
    """One-frame files of nframes different frames: the device's WebP, the device's PNG of the same pixels, Pillow's lossless WebP."""
    import numpy as np
    import PIL.Image
    import torch
    from cuburn_amd import _lib
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import webp_model
    mgr, rdr, gnm, gprof = setup(kind, size)
    lib = _lib.load()
    channels = rdr.out.channels
    ours = png = theirs = 0
    parts = None
    for k in range(nframes):
        evt, frame = mgr.queue_frame(rdr, gnm, gprof, (k + 0.5) / nframes)
        evt.synchronize()
        rdr.out.encode(frame)
        data = rdr.out.encode(None)[0]['.webp'].read()
        im = PIL.Image.open(io.BytesIO(data))
        assert im.n_frames == 1
        pixels = np.ascontiguousarray(np.asarray(im.convert('RGBA')))
        again = io.BytesIO()
        im.save(again, 'WEBP', lossless=True)
        h, w = pixels.shape[:2]
        t = torch.from_numpy(pixels).to('cuda:%d' % mgr.fb.device)
        torch.cuda.synchronize(mgr.fb.device)
        cap = lib.fl_png_bound(w, h, channels)
        buf = mgr.fb._pinned((cap,), 'u1')
        _lib.check(lib.fl_png_encode(mgr.fb.ctx, w, h, t.data_ptr(), channels, buf.ctypes.data, 0, cap))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        nbytes, status = (int(v) for v in np.frombuffer(buf[:8], '<u4'))
        assert status == 0
        if k == 0 and size != '1080p':                                # what the parts weigh, by the model (minutes at 1080p)
            info = webp_model.payload_bits(pixels, channels)[1]
            parts = dict((key, info[key]) for key in ('sub_bits', 'header_bits', 'pixel_bits'))
        ours += len(data)
        png += nbytes
        theirs += len(again.getvalue())
    mgr.fb.free()
    return dict(frames=nframes, device_webp_bytes=ours, device_png_bytes=png, pillow_lossless_webp_bytes=theirs, webp_over_png=ours / float(png),
                webp_over_pillow=ours / float(theirs), first_frame_parts_bits=parts)


def child(args, limit, env=None):
    """One step in a process of its own; its last line is the step's JSON."""
    print('step: ' + ' '.join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, timeout=limit)
    if r.returncode:
        raise SystemExit('step %s ended with status %d: nothing more is started' % (' '.join(args), r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def profiled_kernels(size, nframes):
    """Average duration per launch of the WebP kernels, from rocprofv3's kernel statistics of a child process."""
    out = tempfile.mkdtemp(prefix='webp_prof_', dir=os.environ.get('TMPDIR', '/tmp'))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'webp', '--',
           sys.executable, os.path.abspath(__file__), '--step', 'loop', '--kind', 'webp', '--size', size, '--frames', str(nframes)]
    r = subprocess.run(cmd, env=dict(os.environ, FLAME_LANES='1'), stdout=subprocess.DEVNULL, timeout=300)
    if r.returncode:
        raise SystemExit('the profiled step ended with status %d: nothing more is started' % r.returncode)
    found = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if not found:
        raise RuntimeError('rocprofv3 wrote no kernel statistics under %s' % out)
    rows = {}
    for r in csv.DictReader(open(found[0])):
        if 'webp' in r['Name'] or 'f32_to_rgba' in r['Name']:
            m = re.search(r'k_\w+', r['Name'])
            rows[m.group(0) if m else r['Name']] = dict(calls=int(r['Calls']), avg_us=float(r['AverageNs']) / 1e3)
    return rows


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the figures to this JSON file')
    ap.add_argument('--no-profile', action='store_true', help='skip the rocprofv3 children')
    ap.add_argument('--step', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--kind', default='webp', help=argparse.SUPPRESS)
    ap.add_argument('--size', default='1080p', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == 'loop':
        print(json.dumps(loop(args.kind, args.size, args.frames)))
        return
    if args.step == 'bytes':
        print(json.dumps(file_bytes(args.kind, args.size)))
        return
    res = dict(config='cfg2, 2^28 samples at 1920x1080 and the same samples per pixel at 480x270', frames=args.frames, rounds=args.rounds,
               runs='every step a process of its own; the loops in the order %s, %d times over, medians of the rounds; file bytes and '
                    'kernel times from one run each' % (', '.join(ORDER), args.rounds))
    for size in SIZES:
        runs = dict((k, []) for k in ORDER)
        for _ in range(args.rounds):
            for kind in ORDER:
                runs[kind].append(child(['--step', 'loop', '--kind', kind, '--size', size, '--frames', str(args.frames)], 300))
        s = res[size] = {}
        for kind in ORDER:
            r = runs[kind]
            s['loop_' + kind] = dict(output=BLOCKS[kind], rounds=r, fps=median([x['fps'] for x in r]),
                                     encode_slot_ms_per_frame=median([x['encode_slot_ms_per_frame'] for x in r]),
                                     file_bytes_per_frame=r[-1].get('file_bytes_per_frame'))
        s['webp_over_none_fps'] = s['loop_webp']['fps'] / s['loop_none']['fps']
        s['webp_over_png_fps'] = s['loop_webp']['fps'] / s['loop_png']['fps']
        s['bytes_rgb'] = child(['--step', 'bytes', '--kind', 'webp', '--size', size], 300)
        s['bytes_rgba'] = child(['--step', 'bytes', '--kind', 'webp_alpha', '--size', size], 300)
        if not args.no_profile:
            s['rocprofv3_kernels'] = profiled_kernels(size, 40)
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
