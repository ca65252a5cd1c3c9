"""
The frame-block form of the device PNG encoder (cuburn_amd/csrc/png.hip, k_png_scan and k_png_gather; fl_apng_encode,
fl_output_apng) and the APNG output on top of it (encoders.APNGOutput).  The reference is the device's own PNG file of the same
pixels, which tests/test_gpu_png.py and tests/test_gpu_png_ext.py hold to their models byte for byte: an IDAT block is that file
without its first 33 and last 12 bytes, and an fdAT block is the IDAT block with a number in front of every chunk's data, under a
CRC-32 that zlib recomputes here.  The frames (tests/apng_cases.py) are encoded in a child process with FLAME_PNG_SEG=8192
(tests/apng_child.py), since the library reads the variable once and they need segments that short to have three chunks; the
child runs once for the module.  The whole path — fl_output_apng against fl_output, and three frames of a flame through
queue_frame against the raw output of the same seeds — runs here, with the library's own segment length.
"""
import ctypes as C
import functools
import io
import os
import pickle
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from cuburn_amd import _lib, configs, encoders, output, profile, render
import apng_cases as A
import encoder_contract as EC
import encoder_harness as H
import png_ext_model as X

pytestmark = pytest.mark.gpu

CASES = [(s, p, f) for s in A.SHAPES for p in A.PATTERNS for f in A.FLAGS]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def child(built, tmp_path_factory):
    """Every device call of the cases, made once in a process whose segments are 8192 bytes."""
    path = str(tmp_path_factory.mktemp('apng') / 'blocks.pickle')
    run = subprocess.run([sys.executable, os.path.join(HERE, 'apng_child.py'), path], env=dict(os.environ, FLAME_PNG_SEG=str(A.SMALL_SEG)),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert run.returncode == 0, run.stdout.decode('utf-8', 'replace')[-4000:]
    with open(path, 'rb') as f:
        return pickle.load(f)


record = functools.partial(H.record, chunks=True)          # (nbytes, status, segment, chunks)


def block_of(buf, n, seg=A.SMALL_SEG):
    nbytes, status, param, nchunks = record(buf)
    assert (status, param, nchunks) == (0, seg, n)
    return bytes(buf[16:16 + nbytes])


def untouched(buf, cap):
    return bool((buf[cap:] == A.SENTINEL).all()) and len(buf) > cap


@pytest.mark.parametrize('shape, pattern, flags', CASES, ids=[A.case_id(*c) for c in CASES])
def test_idat_block_is_the_png_files_middle(child, shape, pattern, flags):
    """(1) exact: bytes [33 : -12] of fl_png_encode_f's file of the same source."""
    w, h, ch, bits = shape
    r = child[A.case_id(shape, pattern, flags)]
    n = r['n']
    assert n == A.chunks_of(w, h, ch, bits, A.SMALL_SEG) == {(5, 3): 1, (100, 60): 3, (33, 70): 3, (257, 1): 1}[(w, h)]
    nbytes, status, seg, zero = record(r['png'])
    assert (status, seg, zero) == (0, A.SMALL_SEG, 0) and untouched(r['png'], r['png_cap'])       # the PNG's record is what it was
    png = bytes(r['png'][16:16 + nbytes])
    assert png[:8] == A.SIGNATURE and png[-12:] == A.chunk(b'IEND', b'')
    assert untouched(r['idat'], r['cap'])
    block = block_of(r['idat'], n)
    assert block == png[33:-12]
    tags = [t for t, _ in A.read_chunks(block)]
    assert tags == [b'IDAT'] * n
    assert r['cap'] == r['png_cap'] - 33 - 12 + 4 * n and 16 + len(block) + 4 * n <= r['cap']
    # and the pixels are in there
    ps = X.parse(png, A.SMALL_SEG)
    assert np.array_equal(ps.pixels, r['src'][:, :, :ch]) and set(ps.filters) <= ({0, 1, 2, 3, 4} if flags else {4})
    if pattern == 'zero_runs' and w * h > 100:
        assert any(b['type'] == 2 for b in ps.blocks)      # (dynamic blocks, not only stored ones)


@pytest.mark.parametrize('shape, pattern, flags', CASES, ids=[A.case_id(*c) for c in CASES])
def test_fdat_blocks(child, shape, pattern, flags):
    """(2) tag, length, number and CRC of every chunk at first numbers whose low bytes carry; without the numbers: the IDAT block."""
    r = child[A.case_id(shape, pattern, flags)]
    n = r['n']
    idat = block_of(r['idat'], n)
    lens = [len(b) for _, b in A.read_chunks(idat)]
    assert set(r['fdat']) == set(A.seqs_for(n)) and len(r['fdat']) == 5
    for seq, buf in r['fdat'].items():
        assert untouched(buf, r['cap']), seq
        block = block_of(buf, n)
        assert len(block) == len(idat) + 4 * n
        p = 0
        for i in range(n):                                 # by hand, field by field
            length, = struct.unpack('>I', block[p:p + 4])
            assert length == lens[i] + 4 and block[p + 4:p + 8] == b'fdAT', (seq, i)
            assert block[p + 8:p + 12] == struct.pack('>I', seq + i), (seq, i)
            crc, = struct.unpack('>I', block[p + 8 + length:p + 12 + length])
            assert crc == zlib.crc32(block[p + 4:p + 8 + length]) & 0xffffffff, (seq, i)
            p += 12 + length
        assert p == len(block)
        assert A.retag(block, seq) == idat, seq
    assert sorted(r['overflow']) == A.overflowing_seqs(n) and len(r['overflow']) == n - 1
    assert 0xffffffff - (n - 1) in r['overflow'] or n == 1
    if n == 1:
        assert 0xfffffffe in r['fdat']                     # one chunk: the largest number there is fits
    for seq, (rc, buf) in r['overflow'].items():
        assert rc == _lib.FL_E_INVAL and (buf == A.SENTINEL).all(), hex(seq)      # refused, and nothing was queued


@pytest.mark.parametrize('shape, pattern, flags', CASES, ids=[A.case_id(*c) for c in CASES])
def test_capacity_and_destinations(child, shape, pattern, flags):
    """(3) one byte short: status 1, nothing behind the record, nothing at or beyond cap — pinned, pageable and device memory; an
    exact capacity; device destinations at odd addresses."""
    r = child[A.case_id(shape, pattern, flags)]
    n = r['n']
    want = {254: block_of(r['fdat'][254], n), A.IDAT_SEQ: block_of(r['idat'], n)}
    for seq, s in r['short'].items():
        cap = s['cap']
        assert cap == 16 + len(want[seq]) - 1
        for where in ('pinned', 'pageable'):
            rc, buf = s[where]
            assert rc == 0 and record(buf) == (len(want[seq]), 1, A.SMALL_SEG, n), (seq, where)
            assert untouched(buf, cap), (seq, where)
        assert (s['pinned'][1][16:] == A.SENTINEL).all()   # the kernels wrote the record and nothing else
        rc, dev = s['device']
        assert rc == 0 and dev[0] == A.SENTINEL and record(dev[1:17]) == (len(want[seq]), 1, A.SMALL_SEG, n)
        assert (dev[17:] == A.SENTINEL).all()
    for where in ('pinned', 'pageable'):
        rc, buf = r['exact'][where]
        assert rc == 0 and untouched(buf, r['exact']['cap']) and block_of(buf, n) == want[254], where
    for key, skew in (('device', 1), ('device3', 3)):
        rc, dev = r['odd'][key]
        cap = r['odd']['cap']
        assert rc == 0 and (dev[:skew] == A.SENTINEL).all() and (dev[skew + cap:] == A.SENTINEL).all()
        assert block_of(dev[skew:], n) == want[254]
        assert (dev[skew + 16 + len(want[254]):] == A.SENTINEL).all()


@pytest.mark.parametrize('shape, pattern, flags', CASES, ids=[A.case_id(*c) for c in CASES])
def test_frame_bytes_in_the_file(child, shape, pattern, flags):
    """(6) a frame of the file is the device PNG's bytes minus 45 (signature, IHDR, IEND), plus the fcTL's 38 and 4 per fdAT."""
    w, h, ch, bits = shape
    r = child[A.case_id(shape, pattern, flags)]
    n = r['n']
    png_bytes = record(r['png'])[0]
    ap = A.parse_file(r['file'])
    assert r['seqs'] == [A.IDAT_SEQ, 2, 2 + n + 1]
    assert (ap.w, ap.h, ap.bits, ap.channels, ap.num_frames, ap.num_plays) == (w, h, bits, ch, 3, 2)
    assert ap.frame_bytes == [png_bytes - 45 + 38, png_bytes - 45 + 38 + 4 * n, png_bytes - 45 + 38 + 4 * n]
    assert len(r['file']) == 33 + 20 + sum(ap.frame_bytes) + 12
    assert ap.numbers == list(range(3 + 2 * n))
    for k in range(3):
        assert np.array_equal(X.parse(A.frame_as_png(ap, k), A.SMALL_SEG).pixels, r['src'][:, :, :ch])
    if bits == 8:
        PIL_Image = pytest.importorskip('PIL.Image')
        im = PIL_Image.open(io.BytesIO(r['file']))
        assert im.n_frames == 3 and im.info['loop'] == 2
        for k in range(3):
            im.seek(k)
            assert np.array_equal(np.asarray(im), r['src'][:, :, :ch])


# ------------------------------------------------------------------ the whole path, in this process
mgr = EC.mgr_fixture()


@pytest.mark.parametrize('bits', (8, 16))
def test_output_apng_is_output_then_encode(mgr, bits):
    """(4) fl_output_apng = fl_output + fl_apng_encode: the same block, the same dither states afterwards, a closed frame."""
    import torch
    lib = _lib.load()
    w, h = 64, 48
    dim = mgr.fb.set_dim(w, h)
    fid = C.c_uint32()
    _lib.check(lib.fl_frame_begin(mgr.fb.ctx, C.byref(fid)))      # first: a frame chooses the lane whose buffers the calls below use
    _lib.check(lib.fl_debug_clear(mgr.fb.ctx, w, h, 0))
    rs = np.random.RandomState(11 + bits)
    mgr.fb.write('front', (rs.rand(dim.ah * dim.astride, 4) * 1.3 - 0.1).astype(np.float32))
    start = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    plain = np.empty((h, w, 4), np.uint8 if bits == 8 else np.uint16)
    _lib.check(lib.fl_output(mgr.fb.ctx, w, h, _lib.OUT['rgba8' if bits == 8 else 'rgba16'], plain.ctypes.data, 0))
    _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
    after_plain = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
    assert not np.array_equal(start, after_plain) and plain.std() > (10 if bits == 8 else 1000)
    t = torch.from_numpy(plain.view(np.uint8)).to('cuda:%d' % mgr.fb.device)
    torch.cuda.synchronize(mgr.fb.device)

    def call(entry, *args):
        cap = args[-1]
        buf = mgr.fb._pinned((cap + A.SLACK,), 'u1')
        buf[:] = A.SENTINEL
        _lib.check(getattr(lib, entry)(*(args[:-1] + (buf.ctypes.data, 0, cap))))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        assert (buf[cap:] == A.SENTINEL).all()
        return buf

    for ch, flags, seq in ((3, 0, A.IDAT_SEQ), (4, A.ADAPTIVE, 2), (3, A.ADAPTIVE, 0x01fffffe), (4, 0, A.IDAT_SEQ)):
        cap = lib.fl_apng_bound(w, h, ch, bits, flags)
        n = lib.fl_apng_chunks(w, h, ch, bits)
        encoded = call('fl_apng_encode', mgr.fb.ctx, w, h, t.data_ptr(), ch, bits, flags, seq, cap)
        mgr.fb.write('seeds', start)                          # (the frame stays open: the same lane, the same framebuffer)
        whole = call('fl_output_apng', mgr.fb.ctx, w, h, ch, bits, flags, seq, cap)
        ms = C.c_float(-1.0)
        _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
        assert ms.value >= 0.0
        assert np.array_equal(mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32), after_plain)
        nbytes, status, seg, nchunks = record(whole)
        assert (status, nchunks) == (0, n) and record(encoded) == record(whole)
        assert bytes(whole[16:16 + nbytes]) == bytes(encoded[16:16 + nbytes])
        # ... which is the middle of the PNG of the plain call's pixels
        pcap = lib.fl_png_bound_f(w, h, ch, bits, flags)
        png = call('fl_png_encode_f', mgr.fb.ctx, w, h, t.data_ptr(), ch, bits, flags, pcap)
        middle = bytes(png[16:16 + record(png)[0]])[33:-12]
        block = bytes(whole[16:16 + nbytes])
        assert (block if seq == A.IDAT_SEQ else A.retag(block, seq)) == middle


class _WithRaw(encoders.APNGOutput):
    """The output the profile chose, which also takes the raw (raw16) output of the same frame from the same seeds: fl_output
    first, the dither states put back, then the frame block (as tests/test_gpu_png_ext.py does for the stills)."""

    def copy(self, fb, dim, **kw):
        lib = _lib.load()
        _lib.check(lib.fl_ctx_sync(fb.ctx))
        seeds = fb.read('seeds', (fb.nwalkers, 3), np.uint32)
        raw = (output.Raw16Output() if self.bits == 16 else output.RawOutput()).copy(fb, dim)
        _lib.check(lib.fl_ctx_sync(fb.ctx))
        self.raws = getattr(self, 'raws', []) + [np.array(raw)]
        fb.write('seeds', seeds)
        return encoders.APNGOutput.copy(self, fb, dim, **kw)


@pytest.mark.parametrize('bits, alpha', ((8, False), (8, True), (16, True)))
def test_three_frames_through_the_frame_queue(built, bits, alpha):
    """(5) output: {"type": "apng"} through profile, Renderer and queue_frame, a frame ahead as the command line runs them."""
    PIL_Image = pytest.importorskip('PIL.Image')
    block = {'type': 'apng', 'bits': bits, 'alpha': alpha, 'loop': 5, 'filter': 'adaptive' if bits == 16 else 'paeth'}
    gnm, prof = configs.cfg2(samples=2 ** 13)
    prof = dict(prof, width=64, height=48, spp=2 ** 13 / (64.0 * 48.0), fps=24, output=block)
    gprof = profile.wrap(prof, gnm)
    ch = 4 if alpha else 3
    m = render.RenderManager(device=0, host_seed=7)
    try:
        rdr = render.Renderer(gnm, gprof)
        assert type(rdr.out) is encoders.APNGOutput and (rdr.out.bits, rdr.out.alpha, rdr.out.loop) == (bits, alpha, 5)
        rdr.out = out = _WithRaw(fps=rdr.out.fps, alpha=alpha, bits=bits, filter=rdr.out.filter, loop=5)
        inflight, files = None, {}
        for tc in (0.25, 0.5, 0.75):
            nxt = m.queue_frame(rdr, gnm, gprof, tc)
            if inflight is not None:
                inflight[0].synchronize()
                assert out.encode(inflight[1]) == ({}, [])
            inflight = nxt
        inflight[0].synchronize()
        assert out.encode(inflight[1]) == ({}, [])
        files, logs = out.encode(None)
        assert list(files) == ['.apng'] and logs == []
        data = files['.apng'].read()
        n, raws = out.chunks(64, 48), out.raws
        # the size identity with the device PNG of the same pixels
        lib = _lib.load()
        sizes = []
        for raw in raws:
            import torch
            t = torch.from_numpy(raw.view(np.uint8)).to('cuda:%d' % m.fb.device)
            torch.cuda.synchronize(m.fb.device)
            cap = lib.fl_png_bound_f(64, 48, ch, bits, _lib.PNG_FILTERS[out.filter])
            buf = np.empty(cap, np.uint8)
            _lib.check(lib.fl_png_encode_f(m.fb.ctx, 64, 48, t.data_ptr(), ch, bits, _lib.PNG_FILTERS[out.filter], buf.ctypes.data, 0, cap))
            _lib.check(lib.fl_ctx_sync(m.fb.ctx))
            assert record(buf)[1] == 0
            sizes.append(record(buf)[0])
    finally:
        m.fb.free()
    assert len(raws) == 3 and not np.array_equal(raws[0], raws[1]) and raws[0][:, :, :3].max() > 0
    ap = A.parse_file(data)
    assert (ap.w, ap.h, ap.bits, ap.channels, ap.num_frames, ap.num_plays) == (64, 48, bits, ch, 3, 5)
    assert ap.numbers == list(range(3 + 2 * n)) and all(f[1:] == (64, 48, 0, 0, 1, 24, 0, 0) for f in ap.fctl)
    assert ap.frame_bytes == [sizes[0] - 45 + 38] + [s - 45 + 38 + 4 * n for s in sizes[1:]]
    for k in range(3):
        assert np.array_equal(X.parse(A.frame_as_png(ap, k)).pixels, raws[k][:, :, :ch]), k
    im = PIL_Image.open(io.BytesIO(data))
    assert im.size == (64, 48) and im.n_frames == 3 and im.info['loop'] == 5
    for k in range(3):
        im.seek(k)
        assert abs(im.info['duration'] - 1000.0 / 24.0) < 1e-9
        if bits == 8:
            assert im.mode == ('RGBA' if alpha else 'RGB') and np.array_equal(np.asarray(im), raws[k][:, :, :ch]), k
