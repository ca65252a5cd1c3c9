"""
TIFF stills: the host writer against the device encoder on cfg2 at 1920x1080, 2^28 samples.

  python tools/tiff_bench.py [--frames N] [--out profiles/tiff_bench.json]

Every step runs in a child process of its own, one at a time and under its own time limit; the first step that fails ends the run.
Prints and writes frames/s of the command line's frame loop (__main__._one_ahead: frame k + 1 is queued before frame k is waited
for and encoded) and the bytes of the file for three cases:
  * `tiff`: output: {"type": "tiff"}, the uncompressed file the host writes from the raw 16-bit frame;
  * `tiff_deflate`: output: {"type": "tiff", "compression": "deflate"}, the device's file, with the encode by fl_timings_detail()[5]
    (HIP events around its kernels), the share of stored tiles, and whether Pillow reads the file back as the high bytes of the
    samples the model's reader gives;
  * `none`: no encode at all (the 8-bit raw frame, copied and dropped).
Each figure is from one run.  There is no fallback: without a GPU the tool fails.
"""
import argparse
import io
import json
import os
import struct
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np                                                    # noqa: E402

BLOCKS = dict(none={'type': 'raw'}, tiff={'type': 'tiff'}, tiff_deflate={'type': 'tiff', 'compression': 'deflate'})


def setup(block, host_seed=42):
    from cuburn_amd import configs, profile, render
    gnm, prof = configs.cfg2()
    gprof = profile.wrap(dict(prof, output=block), gnm)
    mgr = render.RenderManager(device=0, host_seed=host_seed)
    return mgr, render.Renderer(gnm, gprof), gnm, gprof


def device_file_stats(data):
    """Of the device's file: tiles, how many of them are stored blocks, and Pillow's reading of it."""
    ne, = struct.unpack('<H', data[8:10])
    ent = dict((struct.unpack('<H', data[10 + 12 * i:12 + 12 * i])[0], struct.unpack('<II', data[14 + 12 * i:22 + 12 * i])) for i in range(ne))
    nt, at = ent[324]
    offs = struct.unpack('<%dI' % nt, data[at:at + 4 * nt]) if nt > 1 else (at,)
    stored = sum(1 for o in offs if (data[o + 2] >> 1 & 3) == 0)      # BTYPE of the tile's block, behind the zlib header
    res = dict(tiles=nt, stored_tiles=stored, stored_share=stored / float(nt), tile_width=ent[322][1], tile_length=ent[323][1])
    try:
        import PIL.Image
        im = PIL.Image.open(io.BytesIO(data))
        px = np.asarray(im)
        res.update(pillow_mode=im.mode, pillow_size=list(im.size), pillow_nonzero_share=float((px.max(axis=2) > 0).mean()))
    except ImportError:
        res['pillow_mode'] = None
    return res


def loop(kind, nframes, warmup=3):
    """Frames/s of the one-ahead loop, each frame waited for and (but for `none`) handed to the output module."""
    from cuburn_amd.__main__ import _one_ahead
    mgr, rdr, gnm, gprof = setup(BLOCKS[kind])
    media, t0 = None, None
    times = [0.5] * (warmup + nframes)
    mgr.timings_reset()
    for idx, (evt, frame) in _one_ahead(lambda t: mgr.queue_frame(rdr, gnm, gprof, t), times):
        evt.synchronize()
        if kind != 'none':
            media, _ = rdr.out.encode(frame)
        if idx == warmup:                                             # (frame warmup + 1 is queued already)
            mgr.timings_reset()
            t0 = time.perf_counter()
    dt = time.perf_counter() - t0
    tm = mgr.timings()
    res = dict(output=BLOCKS[kind], fps=nframes / dt, ms_per_frame=1e3 * dt / nframes, frames=nframes,
               encode_slot_ms_per_frame=tm['encode_ms'] / (nframes - 1))
    if media:
        data = next(iter(media.values())).getvalue()
        res['file_bytes'] = len(data)
        if kind == 'tiff_deflate':
            res['file'] = device_file_stats(data)
    mgr.fb.free()
    return res


def child(args, limit):
    """One step in a process of its own; its last line is the step's JSON."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, timeout=limit)
    if r.returncode:
        raise SystemExit('step %s ended with status %d: nothing more is started' % (' '.join(args), r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--out', default=None, help='also write the figures to this JSON file')
    ap.add_argument('--step', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(loop(args.step, args.frames)))
        return
    res = dict(config='cfg2 1920x1080 2^28 samples', frames=args.frames, runs='every figure is from one run')
    for kind in ('tiff', 'tiff_deflate', 'none'):
        res['loop_' + kind] = child(['--step', kind, '--frames', str(args.frames)], 240)
    res['deflate_over_host_fps'] = res['loop_tiff_deflate']['fps'] / res['loop_tiff']['fps']
    res['deflate_over_host_bytes'] = res['loop_tiff_deflate']['file_bytes'] / float(res['loop_tiff']['file_bytes'])
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
