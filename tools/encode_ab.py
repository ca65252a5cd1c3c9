"""
Every device encoder in this tree against the same encoder in the built checkout of another commit, on cfg2 at 1920x1080
(DESIGN.md §4.8): the refactor of the encoders' shared spine must leave each of them as fast as it was.

  python tools/encode_ab.py --ab DIR [--rounds 5] [--frames 40] [--outputs jpeg,gif,...] [--lanes N] [--out profiles/encode_spine_all_ab.json] [--no-profile]

DIR holds the other commit, built (its own cuburn_amd package and library; it needs no copy of this tool).  For each of the eight
``output`` blocks at their defaults — device jpeg, mjpeg, device png, apng, deflate tiff, exr, gif, webp — the two trees
alternate, --rounds times each.  Every run is a child process of its own, one at a time and under its own time limit; the first
that fails ends the run.  A child warms up three frames, then times --frames of the command line's frame loop
(__main__._one_ahead: frame k + 1 is queued before frame k is waited for and handed to the output module) and reports frames/s
and the encode's kernels per frame by fl_timings_detail()[5] (HIP events around them).

Per output and figure, this tree's mean is accepted where it lies within the other tree's own round-to-round spread (max - min
over its rounds) of the other tree's mean; a slower encode outside it is not.  An output that falls outside is run once more per
tree under `rocprofv3 --kernel-trace --stats`, with one stream lane, and reported with its kernels' average times.
--lanes N runs the children with FLAME_LANES=N (1: an encode shares the GPU with no other frame's kernels, so slot 5 is the
encode's kernels and the gaps between them alone); its figures go under "<output>@lanes=N".
With --out the outputs measured are merged into the file, so that a run can be split over several calls (--outputs).
Frames are not bit-reproducible from run to run (the accumulate's atomics), so a file's bytes differ by a few between any two runs.
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

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLOCKS = dict(jpeg={'type': 'jpeg', 'device': True}, mjpeg={'type': 'mjpeg'}, png={'type': 'png', 'encoder': 'device'},
              apng={'type': 'apng'}, tiff={'type': 'tiff', 'compression': 'deflate'}, exr={'type': 'exr'}, gif={'type': 'gif'},
              webp={'type': 'webp'})
ORDER = ('jpeg', 'mjpeg', 'png', 'apng', 'tiff', 'exr', 'gif', 'webp')
WARMUP = 3


def loop(kind, nframes):
    """What a child runs, with the tree under test first on sys.path: the one-ahead loop with every frame handed to the output."""
    from cuburn_amd import configs, profile, render
    from cuburn_amd.__main__ import _one_ahead
    gnm, prof = configs.cfg2()
    gprof = profile.wrap(dict(prof, output=BLOCKS[kind]), gnm)
    mgr = render.RenderManager(device=0, host_seed=42)
    rdr = render.Renderer(gnm, gprof)
    t0, nbytes = None, 0
    mgr.timings_reset()
    for idx, (evt, frame) in _one_ahead(lambda t: mgr.queue_frame(rdr, gnm, gprof, t), [0.5] * (WARMUP + nframes)):
        evt.synchronize()
        rdr.out.encode(frame)
        nbytes = int(frame[:4].view('<u4')[0])
        if idx == WARMUP:                                             # (frame WARMUP + 1 is queued already)
            mgr.timings_reset()
            t0 = time.perf_counter()
    dt = time.perf_counter() - t0
    tm = mgr.timings()
    rdr.out.encode(None)
    mgr.fb.free()
    return dict(fps=nframes / dt, encode_slot_ms_per_frame=tm['encode_ms'] / (nframes - 1), bytes=nbytes)


def child(tree, kind, nframes, lanes=None, limit=180):
    """One run of `kind` in a process of its own, with `tree` (None: this one) as the package's home; its last line is the JSON."""
    cmd = [sys.executable, os.path.abspath(__file__), '--step', kind, '--frames', str(nframes), '--tree', os.path.abspath(tree or HERE)]
    env = dict(os.environ, FLAME_LANES=str(lanes)) if lanes else None
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=limit, cwd=os.path.abspath(tree or HERE), env=env)
    if r.returncode:
        raise SystemExit('%s in %s ended with status %d: nothing more is started' % (kind, tree or 'this tree', r.returncode))
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def profiled_kernels(tree, kind, nframes=20):
    """Average duration per launch of every kernel of a child that encodes `kind`, from rocprofv3's kernel statistics."""
    out = tempfile.mkdtemp(prefix='encode_ab_', dir=os.environ.get('TMPDIR', '/tmp'))
    home = os.path.abspath(tree or HERE)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', out, '-o', kind, '--',
           sys.executable, os.path.abspath(__file__), '--step', kind, '--frames', str(nframes), '--tree', home]
    r = subprocess.run(cmd, env=dict(os.environ, FLAME_LANES='1'), stdout=subprocess.DEVNULL, timeout=300, cwd=home)
    if r.returncode:
        raise SystemExit('the profiled %s ended with status %d: nothing more is started' % (kind, r.returncode))
    found = glob.glob(os.path.join(out, '**', '*kernel_stats.csv'), recursive=True)
    if not found:
        raise RuntimeError('rocprofv3 wrote no kernel statistics under %s' % out)
    return dict((r['Name'], dict(calls=int(r['Calls']), avg_us=float(r['AverageNs']) / 1e3)) for r in csv.DictReader(open(found[0])))


def judge(this, other, key, lower_is_better):
    """This tree's mean against the other's, with the other's own spread as the margin."""
    a, b = [r[key] for r in this], [r[key] for r in other]
    mean_a, mean_b, spread = sum(a) / len(a), sum(b) / len(b), max(b) - min(b)
    worse = (mean_a - mean_b) if lower_is_better else (mean_b - mean_a)
    return dict(this_mean=mean_a, other_mean=mean_b, other_min=min(b), other_max=max(b), other_spread=spread, this_min=min(a), this_max=max(a),
                within_spread=abs(mean_a - mean_b) <= spread, accepted=worse <= spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ab', default=None, metavar='DIR', help='the built checkout of the other commit')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--outputs', default=','.join(ORDER))
    ap.add_argument('--lanes', type=int, default=None, help='FLAME_LANES of the children (default: what the library chooses)')
    ap.add_argument('--out', default=None, help='merge the figures into this JSON file')
    ap.add_argument('--no-profile', action='store_true', help='no rocprofv3 children for outputs outside their spread')
    ap.add_argument('--step', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, args.tree)
        print(json.dumps(loop(args.step, args.frames)))
        return
    if not args.ab or args.rounds < 2:
        ap.error('--ab DIR and at least two rounds')
    res = {}
    for kind in args.outputs.split(','):
        runs = {'this': [], 'other': []}
        for _ in range(args.rounds):
            for name, tree in (('other', args.ab), ('this', None)):
                runs[name].append(child(tree, kind, args.frames, args.lanes))
        r = dict(block=BLOCKS[kind], frames=args.frames, rounds=args.rounds, runs=runs,
                 encode_slot_ms_per_frame=judge(runs['this'], runs['other'], 'encode_slot_ms_per_frame', True),
                 fps=judge(runs['this'], runs['other'], 'fps', False))
        if not (r['encode_slot_ms_per_frame']['within_spread'] and r['fps']['within_spread']) and not args.no_profile:
            r['rocprofv3_kernels'] = dict(this=profiled_kernels(None, kind), other=profiled_kernels(args.ab, kind))
        res[kind + ('@lanes=%d' % args.lanes if args.lanes else '')] = r
        s, f = r['encode_slot_ms_per_frame'], r['fps']
        print('%-5s slot 5 ms/frame: other %.4f (spread %.4f) this %.4f %s | frames/s: other %.2f (spread %.2f) this %.2f %s'
              % (kind, s['other_mean'], s['other_spread'], s['this_mean'], 'within' if s['within_spread'] else 'OUTSIDE',
                 f['other_mean'], f['other_spread'], f['this_mean'], 'within' if f['within_spread'] else 'OUTSIDE'), flush=True)
        if args.out:                                                  # (after every output: a run that is cut short keeps what it measured)
            old = json.load(open(args.out)) if os.path.exists(args.out) else {}
            old.setdefault('config', 'cfg2 1920x1080, the eight output blocks at their defaults; "other" is the parent commit')
            old.setdefault('outputs', {}).update(res)
            with open(args.out, 'w') as fh:
                fh.write(json.dumps(old, indent=1, sort_keys=True) + '\n')


if __name__ == '__main__':
    main()
