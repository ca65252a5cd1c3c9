"""
APNG: the device's frame blocks against the same loop encoding nothing, against the device PNG, GIF and lossless WebP, and against
the host-side alternative — retagging the device PNG's IDATs as fdATs with zlib.crc32 — on cfg2 at 1920x1080 (2^28 samples) and at
480x270 (the same samples per pixel).

  python tools/apng_bench.py [--frames N] [--rounds R] [--out profiles/apng_bench.json]

Every step is a process of its own (a render manager, its frames, nothing else), started one after the other; the steps are
repeated R times over in the same order and the median of the rounds is the figure to quote.  Prints and writes, per size:
  * frames/s of the command line's frame loop (__main__._one_ahead: frame k + 1 is queued before frame k is waited for and handed
    to the output module) with `apng`, `apng16` (bits 16), `webp`, `gif`, `png` (the device PNG) and `none` (the 8-bit raw frame,
    copied and dropped), and the encode by fl_timings_detail()[5] (HIP events around its kernels);
  * `retag`: the `png` loop whose every frame but the first is rewritten on the host as the fdAT chunks of an APNG (sequence
    number in front of each chunk's data, zlib.crc32 over tag, number and data) and written to a temporary file: frames/s of that
    loop, and the host's milliseconds per frame in the rewriting alone.
There is no fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIZES = {'1080p': (1920, 1080), '270p': (480, 270)}
BLOCKS = dict(none={'type': 'raw'}, gif={'type': 'gif'}, png={'type': 'png', 'encoder': 'device'}, webp={'type': 'webp'},
              apng={'type': 'apng'}, apng16={'type': 'apng', 'bits': 16}, retag={'type': 'png', 'encoder': 'device'})
ORDER = ('apng', 'apng16', 'png', 'retag', 'webp', 'gif', 'none')


def setup(kind, size, host_seed=42):
    from cuburn_amd import configs, profile, render
    w, h = SIZES[size]
    gnm, prof = configs.cfg2()
    gprof = profile.wrap(dict(prof, width=w, height=h, spp=2 ** 28 / (1920.0 * 1080.0), fps=25, output=BLOCKS[kind]), gnm)
    mgr = render.RenderManager(device=0, host_seed=host_seed)
    return mgr, render.Renderer(gnm, gprof), gnm, gprof


class Retag(object):
    """What a host-side APNG mux would do with the device PNG's file: every IDAT of a frame behind the first becomes an fdAT."""

    def __init__(self):
        self.file, self.seq, self.frames, self.seconds = tempfile.TemporaryFile(), 0, 0, 0.0

    def encode(self, frame):
        from cuburn_amd.output import DeviceEncodedOutput
        t0 = time.perf_counter()
        data = bytes(DeviceEncodedOutput.file_bytes(frame, 'PNG file'))
        p, out = 33, []
        self.seq += 1                                                 # (the fcTL's number)
        while data[p + 4:p + 8] == b'IDAT':
            n, = struct.unpack('>I', data[p:p + 4])
            if self.frames == 0:
                out.append(data[p:p + 12 + n])
            else:
                body = b'fdAT' + struct.pack('>I', self.seq) + data[p + 8:p + 8 + n]
                out.append(struct.pack('>I', n + 4) + body + struct.pack('>I', zlib.crc32(body) & 0xffffffff))
                self.seq += 1
            p += 12 + n
        self.file.write(b''.join(out))
        self.frames += 1
        self.seconds += time.perf_counter() - t0


def loop(kind, size, nframes, warmup=3):
    """Frames/s of the one-ahead loop, each frame waited for and (but for `none`) handed to the output module."""
    from cuburn_amd.__main__ import _one_ahead
    mgr, rdr, gnm, gprof = setup(kind, size)
    sink = Retag() if kind == 'retag' else rdr.out
    t0 = None
    times = [0.5] * (warmup + nframes)
    mgr.timings_reset()
    for idx, (evt, frame) in _one_ahead(lambda t: mgr.queue_frame(rdr, gnm, gprof, t), times):
        evt.synchronize()
        if kind != 'none':
            sink.encode(frame)
        if idx == warmup:                                             # (frame warmup + 1 is queued already)
            mgr.timings_reset()
            t0 = time.perf_counter()
            if kind == 'retag':
                sink.seconds = 0.0
    dt = time.perf_counter() - t0
    tm = mgr.timings()
    res = dict(fps=nframes / dt, ms_per_frame=1e3 * dt / nframes, encode_slot_ms_per_frame=tm['encode_ms'] / (nframes - 1))
    if kind == 'retag':
        res['host_retag_ms_per_frame'] = 1e3 * sink.seconds / nframes
        res['file_bytes_per_frame'] = sink.file.tell() / float(warmup + nframes)
    elif kind != 'none':
        media, _ = rdr.out.encode(None)
        if media:                                                     # (a stills output has handed its files over frame by frame)
            res['file_bytes_per_frame'] = len(next(iter(media.values())).read()) / float(warmup + nframes)
    mgr.fb.free()
    return res


def child(args, limit, env=None):
    """One step in a process of its own; its last line is the step's JSON."""
    print('step: ' + ' '.join(args), file=sys.stderr, flush=True)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, timeout=limit)
    if r.returncode:
        raise SystemExit('step %s ended with status %d: nothing more is started' % (' '.join(args), r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the figures to this JSON file')
    ap.add_argument('--step', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--kind', default='apng', help=argparse.SUPPRESS)
    ap.add_argument('--size', default='1080p', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == 'loop':
        print(json.dumps(loop(args.kind, args.size, args.frames)))
        return
    res = dict(config='cfg2, 2^28 samples at 1920x1080 and the same samples per pixel at 480x270', frames=args.frames, rounds=args.rounds,
               runs='every step a process of its own; the loops in the order %s, %d times over, medians of the rounds' % (', '.join(ORDER), args.rounds))
    for size in SIZES:
        runs = dict((k, []) for k in ORDER)
        for _ in range(args.rounds):
            for kind in ORDER:
                runs[kind].append(child(['--step', 'loop', '--kind', kind, '--size', size, '--frames', str(args.frames)], 300))
        s = res[size] = {}
        for kind in ORDER:
            r = runs[kind]
            s['loop_' + kind] = dict(output=BLOCKS[kind], rounds=r, fps=median([x['fps'] for x in r]),
                                     fps_spread=[min(x['fps'] for x in r), max(x['fps'] for x in r)],
                                     encode_slot_ms_per_frame=median([x['encode_slot_ms_per_frame'] for x in r]),
                                     file_bytes_per_frame=r[-1].get('file_bytes_per_frame'))
        s['loop_retag']['host_retag_ms_per_frame'] = median([x['host_retag_ms_per_frame'] for x in runs['retag']])
        s['apng_over_png_fps'] = s['loop_apng']['fps'] / s['loop_png']['fps']
        s['apng_over_none_fps'] = s['loop_apng']['fps'] / s['loop_none']['fps']
        s['apng_over_retag_fps'] = s['loop_apng']['fps'] / s['loop_retag']['fps']
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
