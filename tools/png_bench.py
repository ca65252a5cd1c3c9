"""
PNG stills: the host encoder against the device encoder on cfg2 at 1920x1080, 2^28 samples.

  python tools/png_bench.py [--frames N] [--host-frames N] [--out profiles/png_bench.json] [--sweep] [--no-profile]

Every step runs in a child process of its own, one at a time and under its own time limit; the first step that fails ends the run.
Prints and writes:
  * frames/s of the command line's frame loop (__main__._one_ahead: frame k + 1 is queued before frame k is waited for and
    encoded) with no encode at all, with the host PNG (output: {"type": "png"}) and with the device PNG
    (output: {"type": "png", "encoder": "device"}), and the device encode by fl_timings_detail()[5] (HIP events around its kernels);
  * the bytes of the device's file, of Pillow's file of the same pixels, and of zlib at Z_RLE, level 6, with a full flush every
    segment_bytes over the device's own filtered bytes — the same tokens and the same segmentation, so that the difference is the
    device's length limiting and block headers;
  * per kernel, from a child run under `rocprofv3 --kernel-trace --stats` with one stream lane;
  * --sweep: the device loop at other segment lengths (FLAME_PNG_SEG);
  * --forms (instead of the above): the loop, the encode slot, the file's bytes, the rows per filter type and the share of stored
    segments for the four forms of the device file — 8 / 16 bits x all-Paeth / a type per row — and the loop of the 16-bit TIFF;
  * --ab DIR (instead of the above): the default form in this tree and in the built checkout of another commit at DIR (its own
    copy of this tool and its own library), alternated --ab-rounds times.
    With --out these two add their keys to the file the plain run wrote and leave the rest of it as it is.
Each figure is from one run.  There is no fallback: without a GPU the tool fails.
"""
import argparse
import csv
import glob
import io
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

import numpy as np                                                    # noqa: E402

BLOCKS = dict(none={'type': 'raw'}, host={'type': 'png'}, device={'type': 'png', 'encoder': 'device'},
              device_alpha={'type': 'png', 'encoder': 'device', 'alpha': True}, tiff={'type': 'tiff'},
              device_adaptive={'type': 'png', 'encoder': 'device', 'filter': 'adaptive'},
              device16={'type': 'png', 'encoder': 'device', 'bits': 16},
              device16_adaptive={'type': 'png', 'encoder': 'device', 'bits': 16, 'filter': 'adaptive'})
FORMS = ('device', 'device_adaptive', 'device16', 'device16_adaptive')


def setup(block, host_seed=42):
    from cuburn_amd import configs, profile, render
    gnm, prof = configs.cfg2()
    gprof = profile.wrap(dict(prof, output=block), gnm)
    mgr = render.RenderManager(device=0, host_seed=host_seed)
    return mgr, render.Renderer(gnm, gprof), gnm, gprof


def idat_bodies(data):
    out, p = [], 8
    while p < len(data):
        n, = struct.unpack('>I', data[p:p + 4])
        if data[p + 4:p + 8] == b'IDAT':
            out.append(data[p + 8:p + 8 + n])
        p += 12 + n
    return out


def idat_stream(data):
    return b''.join(idat_bodies(data))


def form_stats(data):
    """Of a device file of any depth: how many rows took each filter type, and how many segments (one IDAT each) are stored blocks."""
    w, h, bits, ctype = struct.unpack('>IIBB', data[16:26])
    rowlen = 1 + w * (3 if ctype == 2 else 4) * bits // 8
    filtered = np.frombuffer(zlib.decompress(idat_stream(data)), np.uint8)
    bodies = idat_bodies(data)
    stored = sum(1 for i, b in enumerate(bodies) if (b[2 if i == 0 else 0] >> 1 & 3) == 0)      # BTYPE of the segment's first block
    return dict(bits=bits, rows_per_filter_type=[int(v) for v in np.bincount(filtered[::rowlen], minlength=5)], segments=len(bodies),
                stored_segments=stored, stored_share=stored / float(len(bodies)), file_bytes=len(data))


def sizes(data, seg):
    """The device's file beside Pillow's file of the same pixels and zlib's Z_RLE coding of the same filtered bytes."""
    import PIL.Image
    im = PIL.Image.open(io.BytesIO(data))
    im.load()
    pil = io.BytesIO()
    im.save(pil, 'png')
    filtered = zlib.decompress(idat_stream(data))
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    rle = sum(len(co.compress(filtered[lo:lo + seg])) + len(co.flush(zlib.Z_FULL_FLUSH)) for lo in range(0, len(filtered), seg)) + len(co.flush())
    raw = im.size[0] * im.size[1] * len(im.getbands())
    px = np.asarray(im)
    return dict(device_file_bytes=len(data), device_zlib_stream_bytes=len(idat_stream(data)), pillow_file_bytes=len(pil.getvalue()),
                zlib_rle_flushed_stream_bytes=rle, raw_bytes=raw, segment_bytes=seg, segments=-(-len(filtered) // seg),
                device_over_raw=len(data) / float(raw), pillow_over_raw=len(pil.getvalue()) / float(raw),
                zero_pixels=float((px.reshape(-1, px.shape[2])[:, :3].max(axis=1) == 0).mean()))


def loop(kind, nframes, warmup=3):
    """Frames/s of the one-ahead loop, each frame waited for and (but for `none`) handed to the output module."""
    from cuburn_amd.__main__ import _one_ahead
    mgr, rdr, gnm, gprof = setup(BLOCKS[kind])
    media, t0, frame = None, None, None
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
    res = dict(fps=nframes / dt, ms_per_frame=1e3 * dt / nframes, frames=nframes, encode_slot_ms_per_frame=tm['encode_ms'] / (nframes - 1))
    if media:
        data = next(iter(media.values())).getvalue()
        res['bytes'] = len(data)
        if kind.startswith('device'):
            res['form'] = form_stats(data)
            if res['form']['bits'] == 8:                              # (Pillow reads the high bytes of a 16-bit file only)
                res['sizes'] = sizes(data, int(np.frombuffer(frame[8:12], '<u4')[0]))
    mgr.fb.free()
    return res


def kernels_only(nframes):
    """What the profiled child runs: device-encoded frames, nothing else."""
    mgr, rdr, gnm, gprof = setup(BLOCKS['device'])
    for _ in range(nframes):
        evt, frame = mgr.queue_frame(rdr, gnm, gprof, 0.5)
        evt.synchronize()
    mgr.fb.free()


def child(args, limit, env=None, tree=None):
    """One step in a process of its own; its last line is the step's JSON.  tree: another built checkout, whose own copy of this tool runs."""
    cmd = [sys.executable, os.path.join(os.path.abspath(tree), 'tools', 'png_bench.py') if tree else os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, timeout=limit, cwd=tree)
    if r.returncode:
        raise SystemExit('step %s ended with status %d: nothing more is started' % (' '.join(args), r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def profiled_kernels(nframes):
    """Average duration per launch of the PNG kernels, from rocprofv3's kernel statistics of a child process."""
    out = tempfile.mkdtemp(prefix='png_prof_', dir=os.environ.get('TMPDIR', '/tmp'))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', 'png', '--',
           sys.executable, os.path.abspath(__file__), '--step', 'kernels', '--frames', str(nframes)]
    r = subprocess.run(cmd, env=dict(os.environ, FLAME_LANES='1'), stdout=subprocess.DEVNULL, timeout=300)
    if r.returncode:
        raise SystemExit('the profiled step ended with status %d: nothing more is started' % r.returncode)
    found = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if not found:
        raise RuntimeError('rocprofv3 wrote no kernel statistics under %s' % out)
    rows = {}
    for r in csv.DictReader(open(found[0])):
        if 'png' in r['Name'] or 'f32_to_rgba' in r['Name']:
            rows[r['Name']] = dict(calls=int(r['Calls']), avg_us=float(r['AverageNs']) / 1e3)
    return rows


def merge_out(path, res):
    """--forms and --ab add their keys (sorted, behind what is there) to the JSON file the plain run wrote, and leave the rest of it as it is."""
    old = json.load(open(path)) if os.path.exists(path) else {}
    for k in sorted(res):
        old.pop(k, None)
        old[k] = res[k]
    with open(path, 'w') as f:
        f.write(json.dumps(old, indent=1) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--host-frames', type=int, default=8, help='frames of the host PNG loop (each takes most of a second)')
    ap.add_argument('--out', default=None, help='also write the figures to this JSON file')
    ap.add_argument('--sweep', action='store_true', help='device loop at segment lengths 8192 .. 32768')
    ap.add_argument('--no-profile', action='store_true', help='skip the rocprofv3 child')
    ap.add_argument('--forms', action='store_true', help='only the four forms of the device file (8 / 16 bits x paeth / adaptive) and the tiff loop')
    ap.add_argument('--ab', default=None, metavar='DIR', help='only the default form, this tree alternated with the built checkout of another commit at DIR')
    ap.add_argument('--ab-rounds', type=int, default=3)
    ap.add_argument('--step', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == 'kernels':
        return kernels_only(args.frames)
    if args.step:
        print(json.dumps(loop(args.step, args.frames)))
        return
    if args.forms or args.ab:
        res = {}
        if args.forms:
            res['forms'] = dict((k, child(['--step', k, '--frames', str(args.frames)], 120)) for k in FORMS)
            res['forms_frames'] = args.frames
            res['loop_tiff'] = child(['--step', 'tiff', '--frames', str(args.frames)], 240)
            res['tiff_file_bytes'] = res['loop_tiff']['bytes']
        if args.ab:                                                   # the default form: this tree and another commit's, alternated
            runs = []
            for _ in range(args.ab_rounds):
                for name, tree in (('this', None), ('other', args.ab)):
                    r = child(['--step', 'device', '--frames', str(args.frames)], 120, tree=tree)
                    runs.append(dict(tree=name, encode_slot_ms_per_frame=r['encode_slot_ms_per_frame'], fps=r['fps'], bytes=r['bytes']))
            res['default_form_a_b'] = runs
            res['default_form_a_b_frames'] = args.frames
        print(json.dumps(res, indent=1, sort_keys=True))
        if args.out:
            merge_out(args.out, res)
        return
    res = dict(config='cfg2 1920x1080 2^28 samples', frames=args.frames, runs='every figure is from one run')
    res['loop_no_encode'] = child(['--step', 'none', '--frames', str(args.frames)], 120)
    res['loop_device_png'] = child(['--step', 'device', '--frames', str(args.frames)], 120)
    res['loop_device_png_alpha'] = child(['--step', 'device_alpha', '--frames', str(args.frames)], 120)
    res['loop_host_png'] = child(['--step', 'host', '--frames', str(args.host_frames)], 240)
    if args.sweep:
        res['segment_sweep'] = {}
        for seg in (8192, 16384, 24576, 32768):
            r = child(['--step', 'device', '--frames', str(max(20, args.frames // 2))], 120, env={'FLAME_PNG_SEG': str(seg)})
            res['segment_sweep'][seg] = dict(encode_slot_ms_per_frame=r['encode_slot_ms_per_frame'], bytes=r['bytes'], fps=r['fps'])
    if not args.no_profile:
        res['rocprofv3_kernels'] = profiled_kernels(40)
        res['rocprofv3_png_us_per_frame'] = sum(v['avg_us'] * v['calls'] for k, v in res['rocprofv3_kernels'].items() if 'png' in k) / 40.0
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
