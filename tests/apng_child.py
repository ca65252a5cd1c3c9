"""
The device side of tests/test_gpu_apng.py, as a process of its own: the library reads FLAME_PNG_SEG once, and the frames of
tests/apng_cases.py need segments of 8192 bytes to have more than one chunk.  Usage: FLAME_PNG_SEG=8192 python apng_child.py OUT.
For every case it queues fl_png_encode_f and fl_apng_encode in every form the test looks at, into buffers pre-filled with a
sentinel, and pickles the buffers as it found them afterwards; it judges nothing (one failed call ends it with a traceback).
"""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from cuburn_amd import _lib, encoders, render          # noqa: E402
import apng_cases as A                                  # noqa: E402


def main(path):
    import torch
    lib = _lib.load()
    mgr = render.RenderManager(device=0, nslots=1024, host_seed=42)
    ctx = mgr.fb.ctx
    dev = 'cuda:%d' % mgr.fb.device

    def sync():
        _lib.check(lib.fl_ctx_sync(ctx))
        torch.cuda.synchronize(mgr.fb.device)

    def host_call(t, w, h, ch, bits, flags, seq, cap, pinned=True):
        """(rc, the buffer of cap + SLACK bytes afterwards) of fl_apng_encode into host memory"""
        buf = mgr.fb._pinned((cap + A.SLACK,), 'u1') if pinned else np.empty(cap + A.SLACK, np.uint8)
        buf[:] = A.SENTINEL
        rc = lib.fl_apng_encode(ctx, w, h, t.data_ptr(), ch, bits, flags, seq, buf.ctypes.data, 0, cap)
        sync()
        return rc, np.array(buf)

    def device_call(t, w, h, ch, bits, flags, seq, cap, skew):
        """The same into device memory at an address `skew` bytes past an aligned one; the whole tensor afterwards"""
        out = torch.full((skew + cap + A.SLACK,), A.SENTINEL, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(mgr.fb.device)
        rc = lib.fl_apng_encode(ctx, w, h, t.data_ptr(), ch, bits, flags, seq, None, out.data_ptr() + skew, cap)
        sync()
        return rc, out.cpu().numpy()

    results = {'seg_env': os.environ.get('FLAME_PNG_SEG')}
    for shape in A.SHAPES:
        w, h, ch, bits = shape
        n = int(lib.fl_apng_chunks(w, h, ch, bits))
        for pattern in A.PATTERNS:
            src = A.source(w, h, bits, pattern)
            t = torch.from_numpy(np.ascontiguousarray(src).view(np.uint8)).to(dev)
            torch.cuda.synchronize(mgr.fb.device)
            for flags in A.FLAGS:
                r = {'n': n, 'src': src}
                pcap = int(lib.fl_png_bound_f(w, h, ch, bits, flags))
                pbuf = mgr.fb._pinned((pcap + A.SLACK,), 'u1')
                pbuf[:] = A.SENTINEL
                _lib.check(lib.fl_png_encode_f(ctx, w, h, t.data_ptr(), ch, bits, flags, pbuf.ctypes.data, 0, pcap))
                sync()
                r['png_cap'], r['png'] = pcap, np.array(pbuf)
                cap = int(lib.fl_apng_bound(w, h, ch, bits, flags))
                r['cap'] = cap
                rc, r['idat'] = host_call(t, w, h, ch, bits, flags, A.IDAT_SEQ, cap)
                _lib.check(rc)
                r['fdat'] = {}
                for seq in A.seqs_for(n):
                    rc, r['fdat'][seq] = host_call(t, w, h, ch, bits, flags, seq, cap)
                    _lib.check(rc)
                # numbers that do not fit: the return code, and a buffer that nothing was queued for
                r['overflow'] = {}
                for seq in A.overflowing_seqs(n):
                    r['overflow'][seq] = host_call(t, w, h, ch, bits, flags, seq, cap)
                # capacity: one byte short, and exact, with the block's length as the record of seq 254 reports it
                need = int(np.frombuffer(r['fdat'][254][:4], '<u4')[0])
                r['short'] = {}
                for seq, nbytes in ((254, need), (A.IDAT_SEQ, need - 4 * n)):
                    short = 16 + nbytes - 1
                    r['short'][seq] = dict(cap=short, pinned=host_call(t, w, h, ch, bits, flags, seq, short),
                                           pageable=host_call(t, w, h, ch, bits, flags, seq, short, pinned=False),
                                           device=device_call(t, w, h, ch, bits, flags, seq, short, 1))
                r['exact'] = dict(cap=16 + need, pinned=host_call(t, w, h, ch, bits, flags, 254, 16 + need),
                                  pageable=host_call(t, w, h, ch, bits, flags, 254, 16 + need, pinned=False))
                r['odd'] = dict(cap=16 + need + 7, device=device_call(t, w, h, ch, bits, flags, 254, 16 + need + 7, 1),
                                device3=device_call(t, w, h, ch, bits, flags, 254, 16 + need + 7, 3))
                # the file of three frames of these pixels, through APNGOutput in this process (whose fl_apng_chunks is this n)
                out = encoders.APNGOutput(alpha=ch == 4, bits=bits, filter='adaptive' if flags else 'paeth', loop=2)
                seqs = [out.number(w, h) for _ in range(3)]
                for seq in seqs:
                    rc, buf = host_call(t, w, h, ch, bits, flags, seq, cap)
                    _lib.check(rc)
                    assert out.encode(buf) == ({}, [])
                media, _ = out.encode(None)
                r['seqs'], r['file'] = seqs, media['.apng'].read()
                results[A.case_id(shape, pattern, flags)] = r
    sync()
    mgr.fb.free()
    with open(path, 'wb') as f:
        pickle.dump(results, f, protocol=4)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1]))
