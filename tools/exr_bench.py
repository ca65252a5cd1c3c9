"""
OpenEXR stills: the device encoder at half and at float against the device's deflate TIFF and no encode at all, on cfg2 at
1920x1080, 2^28 samples.

  python tools/exr_bench.py [--frames N] [--rounds R] [--out profiles/exr_bench.json]

All four cases run in this one process, one after the other, R times over in the same order (so every case meets the same drift
of the machine); each case has a render manager of its own, freed before the next starts.  Prints and writes, per case and round,
frames/s of the command line's frame loop (__main__._one_ahead: frame k + 1 is queued before frame k is waited for and handed to
the output module), the encode by fl_timings_detail()[5] (HIP events around its kernels) and the bytes of the file; for the
OpenEXR files also how many tiles are stored raw.  The median of the rounds is the figure to quote.
  * `exr_half`: output: {"type": "exr"};
  * `exr_float`: output: {"type": "exr", "pixel": "float"};
  * `tiff_deflate`: output: {"type": "tiff", "compression": "deflate"};
  * `none`: no encode at all (the 8-bit raw frame, copied and dropped).
There is no fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import struct
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BLOCKS = dict(none={'type': 'raw'}, tiff_deflate={'type': 'tiff', 'compression': 'deflate'}, exr_half={'type': 'exr'},
              exr_float={'type': 'exr', 'pixel': 'float'})
ORDER = ('exr_half', 'exr_float', 'tiff_deflate', 'none')


def setup(block, host_seed=42):
    from cuburn_amd import configs, profile, render
    gnm, prof = configs.cfg2()
    gprof = profile.wrap(dict(prof, output=block), gnm)
    mgr = render.RenderManager(device=0, host_seed=host_seed)
    return mgr, render.Renderer(gnm, gprof), gnm, gprof


def exr_file_stats(data):
    """Of the device's file: tiles, and how many of them are stored raw (dataSize equal to the cropped tile's bytes)."""
    p = 8
    attrs = {}
    while data[p]:
        q = data.index(b'\0', p)
        r = data.index(b'\0', q + 1)
        size, = struct.unpack('<i', data[r + 1:r + 5])
        attrs[data[p:q]] = data[r + 5:r + 5 + size]
        p = r + 5 + size
    p += 1
    w, h = (v + 1 for v in struct.unpack('<4i', attrs[b'dataWindow'])[2:])
    tw, th = struct.unpack('<II', attrs[b'tiles'][:8])
    nch = (len(attrs[b'channels']) - 1) // 18
    bps = 2 if struct.unpack('<i', attrs[b'channels'][2:6])[0] == 1 else 4
    nt = -(-w // tw) * -(-h // th)
    raw = 0
    for o in struct.unpack('<%dQ' % nt, data[p:p + 8 * nt]):
        tx, ty, _, _, size = struct.unpack('<5i', data[o:o + 20])
        raw += size == min(tw, w - tx * tw) * min(th, h - ty * th) * nch * bps
    return dict(tiles=nt, raw_tiles=raw, tile_width=tw, tile_rows=th, header_bytes=p)


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
    res = dict(fps=nframes / dt, ms_per_frame=1e3 * dt / nframes, encode_slot_ms_per_frame=tm['encode_ms'] / (nframes - 1))
    if media:
        data = next(iter(media.values())).getvalue()
        res['file_bytes'] = len(data)
        if kind.startswith('exr'):
            res['file'] = exr_file_stats(data)
    mgr.fb.free()
    return res


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the figures to this JSON file')
    args = ap.parse_args()
    res = dict(config='cfg2 1920x1080 2^28 samples', frames=args.frames, rounds=args.rounds,
               runs='one process; the cases in the order %s, %d times over; medians of the rounds' % (', '.join(ORDER), args.rounds))
    runs = dict((k, []) for k in ORDER)
    for _ in range(args.rounds):
        for kind in ORDER:
            runs[kind].append(loop(kind, args.frames))
    for kind in ORDER:
        r = runs[kind]
        res['loop_' + kind] = dict(output=BLOCKS[kind], rounds=r, fps=median([x['fps'] for x in r]),
                                   encode_slot_ms_per_frame=median([x['encode_slot_ms_per_frame'] for x in r]),
                                   file_bytes=r[-1].get('file_bytes'))
    res['half_over_tiff_fps'] = res['loop_exr_half']['fps'] / res['loop_tiff_deflate']['fps']
    res['float_over_half_fps'] = res['loop_exr_float']['fps'] / res['loop_exr_half']['fps']
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
