"""
CPU tests (no GPU) of the Lanczos downscale and the profile's `proxies`: the tables of filters.resize_tables
against the float64 model of tests/resize_model.py, the model against Pillow's Image.resize(LANCZOS), the ABI's declaration, and
the host side — profile key, refusals, --proxy, file names, the resume rule.
"""
import argparse
import os
import re
import types

import numpy as np
import pytest

from common import REPO
from cuburn_amd import _lib, configs, distributed, filters, output, profile, render
from cuburn_amd import __main__ as cli
from cuburn_amd.genome import specs
import resize_cases as RC
import resize_model as M

AXES = sorted(set([(c[0], c[2]) for c in RC.CASES] + [(c[1], c[3]) for c in RC.CASES]
                  + [(1920, 960), (1080, 540), (1920, 240), (1080, 135), (7, 1), (8, 1), (5, 5), (1, 1), (97, 13)]))


# ------------------------------------------------------------------ tables
@pytest.mark.parametrize('n_in,n_out', AXES, ids=['%d-%d' % a for a in AXES])
def test_tables_match_the_model(n_in, n_out):
    first, taps = filters.resize_tables(n_in, n_out)
    mfirst, mtaps = M.tables(n_in, n_out)
    assert first.dtype == np.int32 and taps.dtype == np.float32 and taps.flags['C_CONTIGUOUS']
    assert first.shape == (n_out,) and taps.shape == mtaps.shape and np.array_equal(first, mfirst)
    # both normalise in float64 and round to float32 once: they may disagree where the float64 sums differ in their last bit and
    # the quotient sits on a float32 rounding boundary, by one unit of the float32 there at the most
    assert (np.abs(taps.astype(np.float64) - mtaps.astype(np.float64)) <= np.spacing(np.abs(mtaps))).all()
    nt = taps.shape[1]
    assert 1 <= nt <= filters.RESIZE_MAX_TAPS == M.MAX_TAPS
    assert first.min() >= 0 and (first.astype(np.int64) + nt <= n_in).all()
    assert np.abs(taps.astype(np.float64).sum(1) - 1.0).max() <= 2.0 ** -23
    assert np.isfinite(taps).all()
    # the window of the model sits inside the row, zeros around it
    for i, (lo, wt) in enumerate(M.windows(n_in, n_out)):
        off = lo - int(first[i])
        assert off >= 0 and off + len(wt) <= nt
        assert not taps[i, :off].any() and not taps[i, off + len(wt):].any()


def test_a_cut_window_is_renormalised():
    """At the edge Pillow drops the taps outside the picture and divides by what is left: the first row of 64 -> 24 has fewer
    live taps than an interior row, still sums to 1, and its weights are the interior shape scaled up."""
    first, taps = filters.resize_tables(64, 24)
    win = M.windows(64, 24)
    assert win[0][0] == 0 and len(win[0][1]) < len(win[12][1])
    assert abs(float(taps[0].astype(np.float64).sum()) - 1.0) <= 2.0 ** -23
    scale = 64 / 24.0
    x = np.arange(len(win[0][1]))
    raw = M.lanczos((x - 0.5 * scale + 0.5) / scale)
    lo12, w12 = win[12]
    whole = M.lanczos((np.arange(lo12, lo12 + len(w12)) - 12.5 * scale + 0.5) / scale)
    assert raw.sum() < 0.97 * whole.sum()                       # the part of the kernel inside the picture is short of a whole one
    assert np.allclose(win[0][1], raw / raw.sum(), rtol=0, atol=1e-15)
    # ratio 1: the identity
    first, taps = filters.resize_tables(40, 40)
    for i in range(40):
        row = np.zeros(40)
        row[first[i]:first[i] + taps.shape[1]] = taps[i]
        assert abs(row[i] - 1.0) <= 2.0 ** -23 and np.abs(np.delete(row, i)).max() <= 1e-7


def test_ratio_limits():
    assert filters.resize_tables(400, 50)[1].shape[1] <= 50 and filters.resize_tables(8, 1)[1].shape == (1, 8)
    for n_in, n_out in ((401, 50), (9, 1), (50, 51), (10, 0), (1920, 239)):
        with pytest.raises(ValueError) as e:
            filters.resize_tables(n_in, n_out)
        assert str(n_in) in str(e.value) and str(n_out) in str(e.value) and '8' in str(e.value)
    first, taps = filters.resize_tables(333, 167)
    with pytest.raises(ValueError):
        taps[0, 0] = 1.0                                        # shared between calls: read-only
    assert filters.resize_tables(333, 167)[1] is taps


# ------------------------------------------------------------------ Pillow
def test_model_agrees_with_pillow():
    """Image.resize(LANCZOS) on mode F images, channel by channel.  Pillow sums in double and rounds the intermediate image and the
    result to float32, the model rounds nothing but the taps: 2^-24 of A per rounding, and as much again for Pillow's double taps
    against the model's float32 ones (each within 2^-24 of the other, relatively): 4 * 2^-24 * A."""
    Image = pytest.importorskip('PIL.Image')
    worst = 0.0
    for case in ((64, 36, 24, 9), (333, 131, 167, 47), (40, 24, 40, 24), (400, 264, 50, 33)):
        w, h, w2, h2 = case
        rs = np.random.RandomState(5)
        pic = rs.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
        out, A = M.resize_picture(pic, *RC.tables(*case))
        for ch in range(4):
            got = np.asarray(Image.fromarray(pic[:, :, ch], mode='F').resize((w2, h2), Image.LANCZOS), np.float64)
            err = np.abs(got - out[:, :, ch])
            bar = 4 * 2.0 ** -24 * A[:, :, ch]
            worst = max(worst, float((err / bar).max()))
            assert (err <= bar).all(), (case, ch, float(err.max()), float((err / bar).max()))
    assert 0 < worst <= 1


# ------------------------------------------------------------------ header and library
def test_header_and_library(built):
    hdr = open(os.path.join(REPO, 'include', 'flame_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'#define\s+FL_RESIZE_MAX_TAPS\s+50\b', code)
    decl = re.search(r'int\s+fl_resize\s*\(([^;]*)\)\s*;', code)
    assert decl is not None
    args = [' '.join(a.split()) for a in decl.group(1).split(',')]
    assert args == ['fl_ctx *ctx', 'uint32_t w', 'uint32_t h', 'uint32_t w2', 'uint32_t h2', 'const int32_t *xfirst', 'const float *xtaps',
                    'uint32_t nxt', 'const int32_t *yfirst', 'const float *ytaps', 'uint32_t nyt']
    assert re.search(r'#define\s+FL_ABI_VERSION\s+1\b', code)
    lib = _lib.load()
    assert 'fl_resize' in _lib.EXPORTS and hasattr(lib, 'fl_resize') and lib.fl_abi_version() == 1
    assert len(_lib._SIGS['fl_resize'][1]) == len(args)
    (xf, xt), (yf, yt) = filters.resize_tables(64, 24), filters.resize_tables(36, 9)
    rc = lib.fl_resize(None, 64, 36, 24, 9, xf.ctypes.data, xt.ctypes.data, xt.shape[1], yf.ctypes.data, yt.ctypes.data, yt.shape[1])
    assert rc == _lib.FL_E_INVAL and lib.fl_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


# ------------------------------------------------------------------ profile
def wrapped(**over):
    gnm, prof = configs.cfg2()
    return gnm, profile.wrap(dict(prof, width=1920, height=1080, **over), gnm)


def test_profile_spec_takes_proxies():
    node = specs.profile['proxies']
    assert set(node.type) == {'width', 'height', 'suffix', 'output'} and tuple(node.default) == ()
    gnm, gprof = wrapped(output={'type': 'png'}, proxies=[{'width': 480, 'height': 270, 'suffix': '_web', 'output': {'type': 'exr', 'pixel': 'float'}},
                                                         {'width': 960, 'height': 540}])
    assert [(p.width, p.height) for p in gprof.proxies] == [(480, 270), (960, 540)]
    px = output.get_proxies_for_profile(gprof)
    # from the largest to the smallest; the suffix defaults to _<H>p, the output to the master's
    assert [(p.width, p.height, p.suffix) for p in px] == [(960, 540, '_540p'), (480, 270, '_web')]
    assert type(px[0].out) is type(output.get_output_for_profile(gprof)) is output.PILOutput and px[0].out.type == 'png'
    assert type(px[1].out) is output.DeviceEXROutput and px[1].out.pixel == 'float'
    assert px[0].out is not px[1].out
    assert (px[0].gprof.width, px[0].gprof.height, px[1].gprof.width) == (960, 540, 480) and gprof.width == 1920
    assert px[0].gprof.fps == gprof.fps and px[0].gprof.raw().get('proxies') is None
    assert output.get_proxy_files_for_profile(gprof) == ['_540p.png', '_web.exr']
    # every codec the profile can name, external pipes included
    for block, cls in (({'type': 'x264'}, 'X264Output'), ({'type': 'vp9'}, 'VPxOutput'), ({'type': 'mjpeg'}, 'MJPEGOutput'),
                       ({'type': 'gif'}, 'GIFOutput'), ({'type': 'tiff', 'compression': 'deflate'}, 'DeviceTIFFOutput')):
        _, g = wrapped(proxies=[{'width': 960, 'height': 540, 'output': block}])
        assert type(output.get_proxies_for_profile(g)[0].out).__name__ == cls


REFUSALS = [
    ([{'width': 1921, 'height': 540}], r'proxies\[0\].*larger'),
    ([{'width': 960, 'height': 1081}], r'proxies\[0\].*larger'),
    ([{'width': 239, 'height': 135}], r'proxies\[0\].*1/8 of the master'),
    ([{'width': 240, 'height': 134}], r'proxies\[0\].*1/8 of the master'),
    ([{'width': 960, 'height': 540}, {'width': 119, 'height': 68}], r'proxies\[1\].*1/8 of proxies\[0\] \(960 x 540\)'),
    ([{'width': 961, 'height': 541, 'output': {'type': 'mjpeg'}}], r'proxies\[0\].*odd.*4:2:0'),
    ([{'width': 960, 'height': 541, 'output': {'type': 'jpeg', 'device': True, 'sampling': '420'}}], r'proxies\[0\].*odd.*4:2:0'),
    ([{'width': 961, 'height': 540, 'output': {'type': 'vp9', 'pix_fmt': 'yuv420p10'}}], r'proxies\[0\].*odd.*4:2:0'),
    ([{'width': 960, 'height': 540, 'suffix': '_a'}, {'width': 480, 'height': 270, 'suffix': '_a'}], r'proxies\[1\].*proxies\[0\].*same suffix'),
    ([{'width': 960, 'height': 540}, {'width': 480, 'height': 540}], r'same suffix "_540p"'),
    ([{'width': 960, 'height': 540, 'suffix': ''}], r'proxies\[0\]\.suffix.*non-empty'),
    ([{'width': 960, 'height': 540, 'output': {'type': 'png', 'pixel': 'half'}}], r'proxies\[0\]\.output\.pixel'),
    ([{'width': 960, 'height': 200, 'suffix': '_a'}, {'width': 400, 'height': 540, 'suffix': '_b'}], r'proxies\[0\] \(960 x 200\) is made from proxies\[1\] \(400 x 540\)'),
    ([{'width': 960}], r'proxies\[0\]\.height'),
    ([{'width': 960, 'height': 540, 'size': 3}], r'proxies\[0\].*unknown key size'),
]


@pytest.mark.parametrize('proxies,pattern', REFUSALS, ids=[str(k) for k in range(len(REFUSALS))])
def test_refusals_name_the_entry_and_the_reason(proxies, pattern):
    gnm, gprof = wrapped(proxies=proxies)
    with pytest.raises(ValueError) as e:
        output.get_proxies_for_profile(gprof)
    assert re.search(pattern, str(e.value)), str(e.value)
    with pytest.raises(ValueError):
        render.Renderer(gnm, gprof)


def test_a_ratio_beyond_8_is_reached_through_a_size_in_between():
    """The limit is that of one resize: a proxy is held to 8 against the frame it is made from, not against the master."""
    _, gprof = wrapped(proxies=[{'width': 120, 'height': 68}, {'width': 960, 'height': 540}])
    assert [(p.width, p.height) for p in output.get_proxies_for_profile(gprof)] == [(960, 540), (120, 68)]
    _, gprof = wrapped(proxies=[{'width': 120, 'height': 68}])
    with pytest.raises(ValueError):
        output.get_proxies_for_profile(gprof)


def test_an_older_library_may_lack_fl_resize_alone():
    assert _lib._NEWER == ('fl_resize',)


def test_an_odd_proxy_is_fine_where_nothing_subsamples():
    _, gprof = wrapped(proxies=[{'width': 961, 'height': 541, 'output': {'type': 'png', 'encoder': 'device'}},
                                {'width': 481, 'height': 271, 'output': {'type': 'mjpeg', 'sampling': '444'}}])
    assert [(p.width, p.height) for p in output.get_proxies_for_profile(gprof)] == [(961, 541), (481, 271)]


def test_renderer_without_proxies_is_what_it_was():
    gnm, gprof = wrapped()
    rdr = render.Renderer(gnm, gprof)
    assert rdr.proxies == [] and output.get_proxy_files_for_profile(gprof) == []
    assert sorted(vars(rdr)) == sorted(['packer', 'lib', 'cubin', 'mod', '_mod_key', 'filts', 'out', 'proxies'])
    assert [f.name for f in rdr.filts] == ['yuv'] + list(gprof.filter_order) and type(rdr.out) is type(output.get_output_for_profile(gprof))
    gnm, gp = wrapped(proxies=[{'width': 960, 'height': 540}])
    rp = render.Renderer(gnm, gp)
    assert [f.name for f in rp.filts] == [f.name for f in rdr.filts] and type(rp.out) is type(rdr.out)
    assert len(rp.proxies) == 1 and type(rp.proxies[0].out) is type(rp.out) and rp.proxies[0].out is not rp.out


def test_sharded_renders_refuse_proxies():
    gnm, gprof = wrapped(proxies=[{'width': 960, 'height': 540}])
    with pytest.raises(ValueError) as e:
        distributed.refuse_proxies(gprof)
    assert 'proxies' in str(e.value) and 'jobs.py' in str(e.value)
    rdr = types.SimpleNamespace(filts=[], proxies=[object()])
    with pytest.raises(ValueError):
        next(distributed.sharded_frame_steps(None, rdr, gnm, wrapped()[1], 0.5, 0, 2))
    distributed.refuse_proxies(wrapped()[1], types.SimpleNamespace(proxies=[]))
    # frame sharding: a gathered loop refuses the profile before it queues a frame
    queued = []
    evt = types.SimpleNamespace(synchronize=lambda: None)
    gather = types.SimpleNamespace(block=4, slot=lambda: None, submit=lambda: None, flush=lambda: None)

    def queue(slot):
        queued.append(slot)
        return evt, None
    with pytest.raises(ValueError) as e:
        distributed.run_frame_loop(queue, 2, gather=gather, gprof=gprof)
    assert 'proxies' in str(e.value) and queued == []
    assert distributed.run_frame_loop(queue, 2, gather=gather, gprof=wrapped()[1]) == 2 and len(queued) == 2
    assert distributed.run_frame_loop(queue, 1, gprof=gprof) == 1          # nothing is gathered: every rank keeps its own files


# ------------------------------------------------------------------ command line
def parse(*argv):
    return cli.build_parser().parse_args(['B'] + list(argv))


def test_proxy_option_parses():
    assert profile.parse_proxy('960x540') == {'width': 960, 'height': 540}
    assert profile.parse_proxy('960X540:_web') == {'width': 960, 'height': 540, 'suffix': '_web'}
    for bad in ('960', '960x', 'axb', '960x540:', '0x540', '960x540x3'):
        with pytest.raises(argparse.ArgumentTypeError):
            profile.parse_proxy(bad)
    args = parse('-P', '1080p', '--codec', 'mjpeg', '--proxy', '960x540', '--proxy', '480x270:_web')
    _, prof = profile.get_from_args(args)
    assert prof['proxies'] == [{'width': 960, 'height': 540}, {'width': 480, 'height': 270, 'suffix': '_web'}]
    gprof = profile.wrap(prof, configs.cfg2()[0])
    px = output.get_proxies_for_profile(gprof)
    assert [(p.suffix, type(p.out).__name__, p.out.sampling) for p in px] == [('_540p', 'MJPEGOutput', '420'), ('_web', 'MJPEGOutput', '420')]
    assert 'proxies' not in profile.get_from_args(parse('-P', '1080p'))[1]


def test_file_names_and_the_resume_rule(tmp_path):
    args = parse('-P', '1080p', '--codec', 'png', '--proxy', '960x540', '--proxy', '480x270:_web', '-o', str(tmp_path), '--end', '3')
    _, prof = profile.get_from_args(args)
    gprof = profile.wrap(prof, configs.cfg2()[0])
    jobs = profile.enumerate_jobs(gprof, 'B', args, resume=False)
    names = [j[0] for j in jobs]
    assert names == [os.path.join(str(tmp_path), 'B_%05d' % k) for k in (1, 2, 3)]
    assert output.get_proxy_files_for_profile(gprof) == ['_540p.png', '_web.png']
    touch = lambda p: open(p, 'w').close()
    # job 1: every file; job 2: the master and one proxy; job 3: the proxies without the master
    for ext in ('.png', '_540p.png', '_web.png'):
        touch(names[0] + ext)
    touch(names[1] + '.png'); touch(names[1] + '_540p.png')
    touch(names[2] + '_540p.png'); touch(names[2] + '_web.png')
    assert [j[0] for j in profile.enumerate_jobs(gprof, 'B', args, resume=True)] == names[1:]
    touch(names[1] + '_web.png')
    assert [j[0] for j in profile.enumerate_jobs(gprof, 'B', args, resume=True)] == names[2:]
    # without proxies the rule is the old one
    args0 = parse('-P', '1080p', '--codec', 'png', '-o', str(tmp_path), '--end', '3')
    g0 = profile.wrap(profile.get_from_args(args0)[1], configs.cfg2()[0])
    assert [j[0] for j in profile.enumerate_jobs(g0, 'B', args0, resume=True)] == names[2:]


def test_render_job_delivers_and_aborts_every_module(monkeypatch, tmp_path):
    """The command line's frame loop with the device replaced by a stub: every proxy frame goes to its own module and is written
    as <name><suffix><ext>; a failing frame aborts every module."""
    from cuburn_amd import jobs as J, render as R
    from cuburn_amd.genome import store

    gnm = configs.cfg2()[0]
    made, aborted = [], []

    class Out(output.Output):
        def __init__(self, tag):
            self.tag = tag
            made.append(self)

        def encode(self, buf):
            import io
            return ({} if buf is None else {'.bin': io.BytesIO(bytes(buf))}), []

        def abort(self):
            aborted.append(self.tag)
            if self.tag == '1920x1080':
                raise IOError('the master\'s encoder is gone')      # the proxies' modules are aborted all the same

    class Evt(object):
        def __init__(self, proxies):
            self.proxies = proxies
        synchronize = lambda self: self
        query = lambda self: True
        time = lambda self: 1.0

    class Mgr(object):
        fail = False

        def __init__(self, device=None):
            self.fb = types.SimpleNamespace(ctx=None)

        def queue_frame(self, rdr, gnm, gprof, t):
            if Mgr.fail:
                raise RuntimeError('frame lost')
            return Evt([np.frombuffer(p.suffix.encode(), np.uint8) for p in rdr.proxies]), np.frombuffer(b'master', np.uint8)

    monkeypatch.setattr(store, 'connect', lambda db: types.SimpleNamespace(animation=lambda flame, half: (gnm, 'B')))
    monkeypatch.setattr(R, 'RenderManager', Mgr)
    monkeypatch.setattr(output, 'get_output_for_profile', lambda g: Out('%dx%d' % (g.width, g.height)))
    args = parse('-P', '1080p', '--proxy', '960x540', '--proxy', '480x270:_web', '-o', str(tmp_path), '--still')
    _, prof = profile.get_from_args(args)
    assert cli.render(args, prof) == 0
    files = sorted(os.listdir(str(tmp_path)))
    assert files == ['B_00002.bin', 'B_00002_540p.bin', 'B_00002_web.bin']
    assert open(os.path.join(str(tmp_path), 'B_00002_web.bin'), 'rb').read() == b'_web'
    assert open(os.path.join(str(tmp_path), 'B_00002.bin'), 'rb').read() == b'master'
    for f in files:
        os.remove(os.path.join(str(tmp_path), f))
    Mgr.fail = True
    assert cli.render(args, prof) == 1
    assert sorted(set(aborted)) == ['1920x1080', '480x270', '960x540']      # (once per attempt)
