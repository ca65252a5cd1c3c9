"""
The library's kernel launches as a list, to compare two builds of it: a refactor of the host side leaves the list equal.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o trace -- python tools/launch_trace.py render
  python tools/launch_trace.py list DIR/trace_kernel_trace.csv OUT.txt

`render` queues a fixed set of frames through RenderManager on the default two lanes (FLAME_HIP_LIB selects the build): three
cfg2 frames at 640 x 360 with 2^25 samples, one with the chain bilateral -> logscale -> smearclip, one with de -> logscale ->
haloclip (`yuv` leads every chain), and one cfg3 frame of 2731 rounds (three launches: 1024 + 1024 + 683, pipelined on the lane's two streams).
`list` writes one line per dispatch in dispatch order: kernel name, grid, workgroup size, and the stream (or, in traces without a
stream column, the queue) numbered by first appearance.
"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def render():
    from cuburn_amd import configs, profile, render as R
    mgr = R.RenderManager(device=0, nslots=1024, host_seed=42)
    gnm, prof = configs.cfg2(samples=2 ** 25)
    small = dict(prof, width=640, height=360, spp=2 ** 25 / (640.0 * 360.0))
    jobs = [(gnm, small)] * 3
    jobs.append((gnm, dict(small, filter_order=['bilateral', 'logscale', 'smearclip'])))
    jobs.append((gnm, dict(small, filter_order=['de', 'logscale', 'haloclip'])))
    gnm3, prof3 = configs.cfg3()
    jobs.append((gnm3, dict(prof3, width=640, height=360, spp=2731 * 1024 * 256 / (640.0 * 360.0))))
    rdrs = {}
    for g, p in jobs:
        gp = profile.wrap(p, g)
        key = (id(g), tuple(gp.filter_order))
        if key not in rdrs:
            rdrs[key] = R.Renderer(g, gp)
        evt, out = mgr.queue_frame(rdrs[key], g, gp, 0.5)
        evt.synchronize()
        print([f.name for f in rdrs[key].filts], mgr.timings()['launches'], 'iterate launches so far')
    mgr.fb.free()


def listing(src, dst):
    rows = list(csv.DictReader(open(src)))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    where = 'Stream_Id' if 'Stream_Id' in rows[0] and len(set(r['Stream_Id'] for r in rows)) > 1 else 'Queue_Id'
    seen = {}
    with open(dst, 'w') as f:
        f.write('# kernel | grid | workgroup | %s (numbered by first appearance)\n' % where.split('_')[0].lower())
        for r in rows:
            grid = 'x'.join(r['Grid_Size_' + a] for a in 'XYZ')
            wg = 'x'.join(r['Workgroup_Size_' + a] for a in 'XYZ')
            f.write('%s | %s | %s | %d\n' % (r['Kernel_Name'], grid, wg, seen.setdefault(r[where], len(seen))))
    print('%d dispatches, %d %ss -> %s' % (len(rows), len(seen), where.split('_')[0].lower(), dst))


if __name__ == '__main__':
    if sys.argv[1:2] == ['render']:
        render()
    elif sys.argv[1:2] == ['list'] and len(sys.argv) == 4:
        listing(sys.argv[2], sys.argv[3])
    else:
        sys.exit(__doc__)
