"""
The contract of the device encoders' entry points, stated once (harness module; tests/test_gpu_encoder_contract.py runs it and
tests/test_cpu_encoder_contract.py holds ROWS to the library's prototype table).  Every fl_X_encode* goes through encode_source,
every fl_output_X through encode_front and both through encode_on (cuburn_amd/csrc/flame_abi.hip), so what they promise of a
destination, a capacity, a refused call, the whole path and the timing slot is the same for all of them:

  capacity      a too-small cap gives (need, 1, param) in the record, nothing at or beyond cap is written and nothing behind the
                record either (jpeg, png and tiff store their header there all the same: Row.header_on_overflow); an exact cap
                gives the file;
  pageable      a host destination that is not pinned receives the same bytes, and the same record when it is too small, with
                nothing at or beyond cap (below cap it then receives what the lane's staging buffer held);
  device        a device destination at an odd address receives the same bytes, and a host destination beside it too;
  refusals      every refused tuple returns its code, sets fl_last_error, touches nothing and leaves the next frame right;
  whole path    fl_output_X is fl_output plus the encode: the same bytes, the same dither states afterwards, a closed frame;
  timed         the encode's kernels are timed in slot 5 of fl_timings_detail.

An encoder is a row of ROWS: its entry points, its arguments, its sources (the arrays of the *_cases.py modules) and its model.
A call is (w, h, src, *mid, host, dev, cap); `mid` is the tuple of the entry point's middle arguments, of which fl_output_X and
fl_X_bound take those behind the first `lead` (exr's source stride).  Also here: the helpers the per-format modules had a copy
each of (the manager fixture, file_of, small_profile, run_cli).
"""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from cuburn_amd import _lib, configs, profile, render
import encoder_harness as H
from encoder_harness import SENTINEL, SLACK, first_difference, record
import exr_cases
import exr_model
import gif_cases
import gif_model
import jpeg420_model
import jpeg_cases
import jpeg_model
import jpeg_opt_cases
import jpeg_opt_model
import png_cases
import png_ext_cases
import png_ext_model
import png_model
import tiff_cases
import tiff_model
import webp_cases
import webp_model

HERE = os.path.dirname(os.path.abspath(__file__))
CLAUSES = ('capacity', 'pageable', 'device', 'refusals', 'timed')      # (the whole path takes its frame from fl_output, not from a source)
ODD = (1, 2, 3)                                                        # the device destination's offsets from an aligned address
INVAL, UNSUPPORTED = _lib.FL_E_INVAL, _lib.FL_E_UNSUPPORTED
S444, S420, OPT, ADAPTIVE = _lib.JPEG_SAMPLING['444'], _lib.JPEG_SAMPLING['420'], _lib.JPEG_OPTIMIZE, _lib.PNG_ADAPTIVE
HALF, FLOAT = exr_model.HALF, exr_model.FLOAT


# ------------------------------------------------------------------ the helpers every per-format module had a copy of
def mgr_fixture():
    """`mgr = mgr_fixture()` in a test module: its one manager, freed behind the module's last test."""
    @pytest.fixture(scope='module')
    def mgr(built):
        m = render.RenderManager(device=0, nslots=1024, host_seed=42)
        yield m
        _lib.check(_lib.load().fl_ctx_sync(m.fb.ctx))
        m.fb.free()
    return mgr


def file_of(row, buf, mid=None, param=None, what=''):
    """The file or block behind a record of status 0; with `mid`, the record's parameter is the row's for it (or `param`)."""
    nbytes, status, p = record(buf)
    assert status == 0, '%s: %s: status %d' % (row.name, what, status)
    if param is None and mid is not None and not row.probe:
        param = row.model_param(mid)
    assert param is None or p == param, '%s: %s: the record says parameter %d, not %d' % (row.name, what, p, param)
    return bytes(buf[16:16 + nbytes])


def small_profile(block, width=64, height=48, **over):
    """(genome, profile) of the 2^22-sample config at a small size with `block` as its output."""
    gnm, prof = configs.cfg2(samples=2 ** 22)
    prof = dict(prof, width=width, height=height, spp=2 ** 22 / float(width * height), output=block, **over)
    return gnm, profile.wrap(prof, gnm)


def run_cli(tmp_path, *args):
    """python -m cuburn_amd B -d tmp_path -o tmp_path *args on the golden genome B; returns the paths of the files it wrote."""
    gold = json.load(open(os.path.join(HERE, 'golden', 'genome_front.json')))
    (tmp_path / 'B.json').write_text(json.dumps(gold['db']['B']))
    before = set(os.listdir(str(tmp_path)))
    out = subprocess.run([sys.executable, '-m', 'cuburn_amd', 'B', '-d', str(tmp_path), '-o', str(tmp_path)] + list(args),
                         cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stderr[-500:])
    return [os.path.join(str(tmp_path), f) for f in sorted(set(os.listdir(str(tmp_path))) - before)]


# ------------------------------------------------------------------ the rows
class Row:
    """An encoder's entry point as the clauses see it.  Data and small callables:

    encode, output, bound   the three entry names
    lead, bound_args(mid)   how many of mid only `encode` takes, and which of the rest fl_X_bound takes
    planar                  the source is [3][h][w], not [h][w][4]
    sources                 clause -> the names of its sources (`capacity` stands in for a clause that is not there)
    source(name, param)     -> (array, mid): the array of a *_cases.py module and the good middle arguments for it
    model(arr, mid, param)  the model's bytes; they are the device's unless there is
    criteria(mgr, what, data, arr, mid, param)   what a file is held to besides; all there is where the model does not fix the bytes
                            (`exact` is False: the JPEG family, whose coefficients are right within a bound)
    model_param(mid)        the record's third word by the model; `probe` = (array, mid, lo, hi) where the device chooses it
                            within lo..hi and the record of that tiny frame says what it chose
    min_cap(w, h, mid)      the smallest cap that is not refused: the record and the header
    refused                 edits of the good call, {field or index into mid: value}, or (edit, code) where the code is not
                            FL_E_INVAL; null source, no destination and min_cap - 1 are every row's and are not listed
    facts                   (entry, args, True where it is 0) of the fl_X_bound calls that stand beside the refusals
    whole                   (fl_output format, w, h, the mids run on one open frame)

    and the flags that say where the device does something else than the clause's strongest form."""
    lead, planar, exact, probe, criteria, facts, whole = 0, False, True, None, None, (), ()
    header_on_overflow = False    # True: the placement kernel stores the header behind the record whatever the status, also of a file that does not fit
    bound_args = staticmethod(lambda mid: mid)

    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def __repr__(self):
        return self.name


def _jpeg_row(name, suffix, sampling, mid_of, probe_hi, whole_size, refused, optimised=False):
    """A row of the JPEG family: fl_jpeg_encode<suffix> at `sampling`, mid_of(quality) its middle arguments."""
    cases = jpeg_opt_cases.case if optimised else lambda case, ri, s: jpeg_opt_cases.CASE_MODULE[s].case(case, ri)
    side = 16 if sampling == S420 else 8                      # one MCU

    def source(case, ri):
        planes, quality, _ = cases(case, ri, sampling)
        return planes, mid_of(quality)

    def model(planes, mid, ri):
        if optimised:
            return jpeg_opt_model.encode(planes, mid[0], ri, sampling)
        return (jpeg420_model if sampling == S420 else jpeg_model).encode(planes, mid[0], ri)

    def criteria(mgr, what, data, planes, mid, ri):
        standard = None
        if optimised:                                         # the stream fl_jpeg_encode_s writes from the same planes
            _, h, w = planes.shape
            buf, _ = H.encode(mgr, 'fl_jpeg_encode_s', planes, w, h, mid[:2], _lib.load().fl_jpeg_bound_s(w, h, sampling), what=what + ': the standard stream')
            assert record(buf)[1] == 0, '%s: the standard stream: status %d' % (what, record(buf)[1])
            standard = bytes(buf[16:16 + record(buf)[0]])
        H.assert_jpeg_criteria(data, planes, mid[0], ri, sampling, standard)

    return Row(name, encode='fl_jpeg_encode' + suffix, output='fl_output_jpeg' + suffix, bound='fl_jpeg_bound' + suffix, bound_args=lambda mid: tuple(mid[1:]),
               planar=True, exact=False, header_on_overflow=True, sources={'capacity': (jpeg_cases.NOISE_Q100,)}, source=source, model=model, criteria=criteria,
               model_param=lambda mid: jpeg_opt_cases.CASE_MODULE[sampling].MODEL_RI, probe=(np.zeros((3, side, side), np.uint8), mid_of(50), 1, probe_hi),
               min_cap=lambda w, h, mid: 16 + jpeg_model.HEADER_BYTES, refused=refused, whole=(('yuv444p',) + whole_size + ((mid_of(90),),),))


def _reads_back(what, ps, field, arr, ch, bits):
    """The model's reader returns the source's samples at the chosen channel count and depth."""
    assert (ps.w, ps.h, ps.channels, ps.bits) == (arr.shape[1], arr.shape[0], ch, bits), '%s: the file says %r' % (what, (ps.w, ps.h, ps.channels, ps.bits))
    assert np.array_equal(getattr(ps, field), arr[:, :, :ch]), '%s: %d samples differ' % (what, int((getattr(ps, field) != arr[:, :, :ch]).sum()))


def _png_f_row(name, flags):
    """fl_png_encode_f at 16 bits with one of its filter flags; a source's name is ten_band's (w, bpp) and the channel count."""
    return Row(name, encode='fl_png_encode_f', output='fl_output_png_f', bound='fl_png_bound_f', header_on_overflow=True,
               sources={'capacity': ((40, 8, 4),), 'pageable': ((33, 6, 3),), 'device': ((33, 8, 4),), 'refusals': ((37, 8, 4),)},
               source=lambda name, seg: (png_ext_cases.source(png_ext_cases.ten_band(name[0], name[1]), name[2], 16), (name[2], 16, flags)),
               model=lambda arr, mid, seg: png_ext_model.encode(arr, mid[0], mid[1], mid[2], seg),
               criteria=lambda mgr, what, data, arr, mid, seg: _reads_back(what, png_ext_model.parse(data, seg), 'pixels', arr, mid[0], mid[1]),
               model_param=lambda mid: png_ext_cases.MODEL_SEG, probe=(np.zeros((1, 1, 4), np.uint16), (3, 16, 0), 256, 65535),
               min_cap=lambda w, h, mid: 16 + png_model.HEADER_BYTES,
               refused=[{1: 0, 2: 0}, {1: 12, 2: 0}, {1: 32, 2: 1}, {2: 2}, {1: 8, 2: 3}, {0: 3, 2: 0x80000000},
                        {'w': 9000, 'h': 65535, 2: 0},        # a frame whose fl_png_bound_f is 0 (and whose fl_png_bound is not)
                        {0: 5, 2: 0}, {'w': 0, 2: 0}],
               facts=(('fl_png_bound', (9000, 65535, 4), False), ('fl_png_bound_f', (9000, 65535, 4, 16, 0), True)),
               whole=(('rgba16', 64, 48, ((3, 16, flags), (4, 16, flags))),))


def _tiff_row(name, bits):
    """fl_tiff_encode at one depth; a source's name is its kind and the channel count."""
    kinds = {'mixed': lambda ch: tiff_cases.mixed(bits, tiff_cases.MIXED_SEED[(bits, ch)]), 'noise37': lambda ch: tiff_cases.noise(37, 10, bits, 4) // 7,
             'noise70': lambda ch: tiff_cases.noise(70, 70, bits, 2)}
    return Row(name, encode='fl_tiff_encode', output='fl_output_tiff', bound='fl_tiff_bound', header_on_overflow=True,
               sources={'capacity': (('mixed', 4),), 'pageable': (('mixed', 3),), 'refusals': (('noise37', 4),), 'timed': (('noise70', 3),)},
               source=lambda name, _: (kinds[name[0]](name[1]), (name[1], bits)),
               model=lambda arr, mid, _: tiff_model.encode(arr, mid[0], mid[1]),
               criteria=lambda mgr, what, data, arr, mid, _: _reads_back(what, tiff_model.parse(data), 'samples', arr, mid[0], mid[1]),
               model_param=lambda mid: tiff_model.tile_bytes(mid[0], mid[1]), min_cap=lambda w, h, mid: 16 + tiff_model.header_bytes(w, h, mid[0], mid[1]),
               refused=[{'w': 0}, {'h': 0}, {'w': 65536}, {'h': 65536}, {0: 2}, {0: 5}, {0: 0}, {1: 0}, {1: 12}, {1: 32},
                        {'w': 20000, 'h': 65535, 1: 8}],      # a frame whose fl_tiff_bound is 0: beyond 2^32 - 1
               facts=(('fl_tiff_bound', (20000, 65535, 4, 8), True), ('fl_tiff_bound', (20000, 65535, 3, 16), True)),
               whole=(('rgba%d' % bits, 64, 48, ((3, bits), (4, bits))),))


def _exr_source(name, _):
    """f32 [h][w][4] and (stride, channels, pixel); a source's name is its kind, the pixel type and the channel count."""
    kind, pixel, ch = name
    arr = {'mixed': lambda: exr_cases.mixed(pixel, exr_cases.MIXED_SEED[(pixel, ch)]), 'ramps37': lambda: exr_cases.ramps(37, 10, 4),
           'ramps70': lambda: exr_cases.ramps(70, 70, 2)}[kind]()
    return arr, (arr.shape[1], ch, pixel)


ROWS = (
    _jpeg_row('jpeg', '', S444, lambda q: (q,), 65535, (64, 48), [{0: 0}, {0: 101}, {0: -5}, {'w': 0}, {'h': 0}, {'w': 65536}, {'h': 65536}]),
    _jpeg_row('jpeg_s420', '_s', S420, lambda q: (q, S420), 10, (70, 50),      # (an interval of at most 10 MCUs: six lanes per MCU, one wave per interval)
              [{1: 2}, {1: -1}, {1: 420}, {0: 0}, {0: 101}, {'w': 0}, {'h': 65536}]),
    _jpeg_row('jpeg_f444', '_f', S444, lambda q: (q, S444, OPT), 21, (70, 50),
              [{2: 2}, {2: 3}, {2: 0x80000001}, {1: 2}, {1: -1}, {0: 0}, {0: 101}, {'w': 0}, {'h': 65536},
               ({'w': 30000, 'h': 30000}, UNSUPPORTED)], True),      # more than 2^24 blocks: refused before the source is looked at or anything is queued
    _jpeg_row('jpeg_f420', '_f', S420, lambda q: (q, S420, OPT), 10, (70, 50),
              [{2: 2}, {2: 3}, {2: 0x80000001}, {1: 2}, {1: -1}, {0: 0}, {0: 101}, {'w': 0}, {'h': 65536},
               ({'w': 30000, 'h': 30000}, UNSUPPORTED)], True),
    Row('png', encode='fl_png_encode', output='fl_output_png', bound='fl_png_bound', header_on_overflow=True,
        sources={'capacity': (png_cases.NOISE,), 'device': ('smooth_256x96',)},
        source=lambda name, seg: (lambda rgba, ch, _: (rgba, (ch,)))(*png_cases.case(name, seg)),
        model=lambda arr, mid, seg: png_model.encode(arr[:, :, :mid[0]], seg),
        criteria=lambda mgr, what, data, arr, mid, seg: H.assert_png_criteria(data, arr, mid[0], seg),
        model_param=lambda mid: png_cases.MODEL_SEG, probe=(np.zeros((1, 1, 4), np.uint8), (3,), 256, 65535),
        min_cap=lambda w, h, mid: 16 + png_model.HEADER_BYTES,
        refused=[{0: 0}, {0: 2}, {0: 5}, {0: -3}, {'w': 0}, {'h': 0}, {'w': 65536}, {'h': 65536}, {'w': 65535, 'h': 65535}],
        whole=(('rgba8', 64, 48, ((3,), (4,))),)),
    _png_f_row('png_f_paeth', 0), _png_f_row('png_f_adaptive', ADAPTIVE),
    _tiff_row('tiff', 16), _tiff_row('tiff_8', 8),
    Row('exr', encode='fl_exr_encode', output='fl_output_exr', bound='fl_exr_bound', lead=1, bound_args=lambda mid: tuple(mid[1:]),
        sources={'capacity': (('mixed', HALF, 4),), 'pageable': (('mixed', FLOAT, 3),), 'device': (('mixed', HALF, 3),), 'refusals': (('ramps37', HALF, 4),),
                 'timed': (('ramps70', HALF, 3),)},
        source=_exr_source, model=lambda arr, mid, _: exr_model.encode(arr, mid[1], mid[2]), model_param=lambda mid: exr_model.tile_bytes(mid[1]),
        min_cap=lambda w, h, mid: 16 + exr_model.header_bytes(w, h, mid[1], mid[2]) + 8 * int(np.prod(exr_model.geometry(w, h, mid[2])[1:])),      # (and the offset table)
        refused=[{'w': 0}, {'h': 0}, {'w': 65536, 0: 65536}, {'h': 65536}, {1: 2}, {1: 5}, {1: 0}, {2: 0}, {2: 3}, {2: 16},
                 {'w': 20000, 'h': 65535, 0: 20000},          # a frame whose fl_exr_bound is 0: beyond 2^32 - 1
                 {0: 37 - 1}, {0: 0}],                        # a stride below the width of the refusals' source
        facts=(('fl_exr_bound', (20000, 65535, 4, HALF), True), ('fl_exr_bound', (20000, 65535, 3, FLOAT), True))),      # (no whole path: fl_output_exr reads the front buffer in place, tests/test_gpu_exr.py)
    Row('gif', encode='fl_gif_encode', output='fl_output_gif', bound='fl_gif_bound', bound_args=lambda mid: (),
        sources={'capacity': ('37x29',), 'pageable': ('gradient_c256_a8',), 'device': ('gradient_c256_a8',)},
        source=lambda name, _: (gif_cases.cases()[name][0], tuple(gif_cases.cases()[name][1:])),
        model=lambda arr, mid, seg: gif_model.frame_block(arr, mid[0], mid[1], seg), model_param=lambda mid: gif_model.SEG,
        min_cap=lambda w, h, mid: 16 + gif_model.HEADER_BYTES,
        refused=[{0: 1}, {0: 257}, {0: 0}, {0: -4}, {1: -1}, {1: 65}, {'w': 0}, {'h': 0}, {'w': 65536, 'h': 1}, {'w': 4097, 'h': 4096, 'cap': 1 << 30}],
        whole=(('rgba8', 70, 50, ((64, 8),)),)),
    Row('webp', encode='fl_webp_encode', output='fl_output_webp', bound='fl_webp_bound',
        sources={'capacity': ('plasma_17x17', 'plasma_65x64'), 'pageable': ('plasma_130x70',), 'device': ('plasma_130x70',), 'refusals': ('plasma_17x17',)},
        source=lambda name, _: (webp_cases.cases()[name][0], (webp_cases.cases()[name][1],)),
        model=lambda arr, mid, _: webp_model.encode(arr, mid[0]), model_param=lambda mid: _lib.WEBP_PB | _lib.WEBP_EB << 8,
        min_cap=lambda w, h, mid: 16 + 8,
        refused=[{0: 2}, {0: 5}, {0: 0}, {0: 1}, {'w': 0}, {'h': 0}, {'w': 16385, 'h': 1, 'cap': 1 << 30}, {'w': 1, 'h': 16385, 'cap': 1 << 30},
                 {'w': 65536, 'h': 1, 'cap': 1 << 30}],
        whole=(('rgba8', 70, 50, ((4,),)),)),
)
ROW = dict((r.name, r) for r in ROWS)
EXEMPT = {'fl_apng_encode': 'a fourth record word and a sequence number; its cases run in the child process of tests/test_gpu_apng.py'}


# ------------------------------------------------------------------ what the clauses share
def dims(row, arr):
    return (arr.shape[2], arr.shape[1]) if row.planar else (arr.shape[1], arr.shape[0])


def bound_of(row, w, h, mid):
    return getattr(_lib.load(), row.bound)(w, h, *row.bound_args(mid))


def encode(mgr, row, arr, mid, cap=None, buf=None, what=''):
    """The row's fl_X_encode of a source into pinned memory (or `buf`) pre-filled with the sentinel, with its fl_X_bound as cap unless
    one is given; waits, and checks the sentinel at and beyond cap.  Returns (buffer, cap)."""
    w, h = dims(row, arr)
    if cap is None:
        cap = bound_of(row, w, h, mid)
        assert cap, '%s: %s is 0 at %d x %d, %r' % (row.name, row.bound, w, h, mid)
    return H.encode(mgr, row.encode, np.ascontiguousarray(arr).view(np.uint8), w, h, mid, cap, buf, what or row.name)


def sources_of(row, clause):
    return row.sources.get(clause, row.sources['capacity'])


def param_of(mgr, row, mid=None):
    """The record's third word: the model's, or what the device says it chose (read once per manager, from a tiny frame)."""
    if not row.probe:
        return row.model_param(mid)
    seen = mgr.__dict__.setdefault('_contract_params', {})
    if row.name not in seen:
        arr, pmid, lo, hi = row.probe
        what = '%s: the record of a %d x %d frame' % ((row.name,) + dims(row, arr))
        seen[row.name] = record(encode(mgr, row, arr, pmid, what=what)[0])[2]
        assert lo <= seen[row.name] <= hi, '%s: parameter %d outside %d..%d' % (what, seen[row.name], lo, hi)
    return seen[row.name]


def verify(mgr, row, what, data, arr, mid, param):
    """`data` is what the row's model says the encoder writes for the source."""
    if row.exact:
        want = row.model(arr, mid, param)
        assert data == want, '%s: not the bytes of the model: %s' % (what, first_difference(data, want))
    if row.criteria:
        try:
            row.criteria(mgr, what, data, arr, mid, param)
        except AssertionError as e:                           # (the criteria of encoder_harness.py do not know the row or the clause)
            raise AssertionError('%s: the file misses its criteria: %s' % (what, e)) from e


class Reference:
    """A source of a row on the device, and the file the encoder writes for it into a destination of fl_X_bound bytes."""

    def __init__(self, mgr, row, clause, name):
        self.what = '%s: %s: %r' % (row.name, clause, name)
        self.row = row
        self.arr, self.mid = row.source(name, param_of(mgr, row) if row.probe else None)
        self.param = param_of(mgr, row, self.mid)
        self.w, self.h = dims(row, self.arr)
        self.bound = bound_of(row, self.w, self.h, self.mid)
        assert self.bound, '%s: %s is 0' % (self.what, row.bound)
        buf = self.encode(mgr, self.bound)
        assert record(buf)[2] == self.param, '%s: the record says parameter %d, not %d' % (self.what, record(buf)[2], self.param)
        self.data = file_of(row, buf, what=self.what)
        self.need = len(self.data)
        assert 16 + self.need <= self.bound, '%s: %d bytes behind the record, %s says %d' % (self.what, self.need, row.bound, self.bound)
        verify(mgr, row, self.what, self.data, self.arr, self.mid, self.param)

    def encode(self, mgr, cap, buf=None):
        return encode(mgr, self.row, self.arr, self.mid, cap, buf, self.what)[0]


def references(mgr, row, clause):
    """The clause's sources, each encoded and verified once per manager."""
    seen = mgr.__dict__.setdefault('_contract_references', {})
    refs = []
    for name in sources_of(row, clause):
        if (row.name, name) not in seen:
            seen[(row.name, name)] = Reference(mgr, row, clause, name)
        refs.append(copy.copy(seen[(row.name, name)]))           # (a view of its own: the message names the clause that asks)
        refs[-1].what = '%s: %s: %r' % (row.name, clause, name)
    return refs


def refused_calls(row, w, h, src, mid, host, cap):
    """[(edit, code, fl_X_encode's arguments, fl_output_X's or None)] of the row's refused calls and every row's three.  fl_output_X
    takes neither a source nor the leading middle arguments, so an edit of those alone leaves its call good: there is none."""
    edits = [e if isinstance(e, tuple) else (e, INVAL) for e in row.refused]
    edits += [({'src': 0}, INVAL), ({'host': None}, INVAL), ({'cap': row.min_cap(w, h, mid) - 1}, INVAL)]
    calls = []
    for edit, code in edits:
        a, m = dict(w=w, h=h, src=src, host=host, cap=cap), list(mid)
        for k, v in edit.items():
            if isinstance(k, int):
                m[k] = v
            else:
                a[k] = v
        reaches_output = any(k != 'src' and not (isinstance(k, int) and k < row.lead) for k in edit)
        calls.append((edit, code, (a['w'], a['h'], a['src']) + tuple(m) + (a['host'], 0, a['cap']),
                      (a['w'], a['h']) + tuple(m[row.lead:]) + (a['host'], 0, a['cap']) if reaches_output else None))
    return calls


def overflow_caps(row, need, w, h, mid):
    """One byte short; the record and the header alone; and, where the file is long enough, a thousand bytes short."""
    lo = row.min_cap(w, h, mid)
    return [16 + need - 1, lo] + ([16 + need - 1000] if 16 + need - 1000 > lo else [])


def assert_overflowed(ref, what, buf, cap, staged=False):
    """The record says what is needed and nothing at or beyond cap was written; nor anything behind the record (where the row says
    so, behind the record and the header), unless the destination is `staged`: a pageable one receives a copy of the first cap
    bytes of the lane's staging buffer, whatever an earlier file left there."""
    want = (ref.need, 1, ref.param)
    assert record(buf) == want, '%s: the record is %r, not %r' % (what, record(buf), want)
    H.assert_untouched(buf, cap, what)
    if staged:
        return
    lo = ref.row.min_cap(ref.w, ref.h, ref.mid) if ref.row.header_on_overflow else 16
    written = np.nonzero(buf[lo:cap] != SENTINEL)[0]
    assert not len(written), '%s: %d bytes written behind the first %d, the last at %d' % (what, len(written), lo, lo + int(written[-1]) if len(written) else 0)


# ------------------------------------------------------------------ the clauses
def check_capacity(mgr, row):
    for ref in references(mgr, row, 'capacity'):
        for cap in overflow_caps(row, ref.need, ref.w, ref.h, ref.mid):
            what = '%s, cap %d of %d' % (ref.what, cap, 16 + ref.need)
            assert_overflowed(ref, what, ref.encode(mgr, cap), cap)
        cap = 16 + ref.need
        what = '%s, the exact cap %d' % (ref.what, cap)
        buf = ref.encode(mgr, cap)
        assert record(buf) == (ref.need, 0, ref.param), '%s: the record is %r, not %r' % (what, record(buf), (ref.need, 0, ref.param))
        H.assert_untouched(buf, cap, what)
        got = file_of(row, buf, what=what)
        assert got == ref.data, '%s: %s' % (what, first_difference(got, ref.data))


def check_pageable(mgr, row):
    """A destination that is not pinned receives a copy; the bytes are the same."""
    for ref in references(mgr, row, 'pageable'):
        got = file_of(row, ref.encode(mgr, ref.bound, np.empty(ref.bound + SLACK, np.uint8)), what=ref.what)
        assert got == ref.data, '%s: %s' % (ref.what, first_difference(got, ref.data))
        cap = 16 + ref.need - 1
        buf = ref.encode(mgr, cap, np.empty(16 + ref.need + SLACK, np.uint8))
        assert_overflowed(ref, '%s, cap %d of %d' % (ref.what, cap, 16 + ref.need), buf, cap, staged=True)


def check_device_destination(mgr, row):
    """A device destination of any alignment receives the same bytes, alone (no copy back) and with a pinned host destination
    beside it, which receives them too."""
    import torch
    lib = _lib.load()
    for ref in references(mgr, row, 'device'):
        cap = 16 + ref.need + 7
        t = H.upload(mgr, ref.arr.view(np.uint8))
        for odd, beside in [(ODD[0], False)] + [(odd, True) for odd in ODD]:
            what = '%s, device address + %d%s' % (ref.what, odd, '' if beside else ', no host destination')
            out = torch.full((cap + SLACK,), SENTINEL, dtype=torch.uint8, device=t.device)
            torch.cuda.synchronize(mgr.fb.device)
            host = mgr.fb._pinned((cap + SLACK,), 'u1')
            host[:] = SENTINEL
            _lib.check(getattr(lib, row.encode)(mgr.fb.ctx, ref.w, ref.h, t.data_ptr(), *ref.mid, host.ctypes.data if beside else None,
                                                out.data_ptr() + odd, cap))
            _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
            dev = out.cpu().numpy()
            assert (dev[:odd] == SENTINEL).all(), '%s: bytes in front of the destination were written' % what
            H.assert_untouched(dev[odd:], cap, what + ', on the device')
            H.assert_untouched(host, cap if beside else 0, what + ', on the host')
            for where, buf in (('device', dev[odd:]),) + ((('host', host),) if beside else ()):
                assert record(buf) == (ref.need, 0, ref.param), '%s: the %s record is %r' % (what, where, record(buf))
                got = file_of(row, buf, what=what)
                assert got == ref.data, '%s: on the %s: %s' % (what, where, first_difference(got, ref.data))


def check_refusals(mgr, row):
    """Every refused call returns its code, says why, touches nothing, and the frame behind it is right."""
    lib = _lib.load()
    for entry, args, zero in row.facts:
        assert (getattr(lib, entry)(*args) == 0) is zero, '%s: refusals: %s%r is %s0' % (row.name, entry, args, 'not ' if zero else '')
    for ref in references(mgr, row, 'refusals'):
        t = H.upload(mgr, ref.arr.view(np.uint8))
        cap = ref.bound
        buf = mgr.fb._pinned((cap + SLACK,), 'u1')
        for edit, code, enc, out in refused_calls(row, ref.w, ref.h, t.data_ptr(), ref.mid, buf.ctypes.data, cap):
            what = '%s, refused %r' % (ref.what, enc)
            buf[:] = SENTINEL
            rc = getattr(lib, row.encode)(mgr.fb.ctx, *enc)
            assert rc == code, '%s: %s returned %d, not %d' % (what, row.encode, rc, code)
            assert lib.fl_last_error(), '%s: fl_last_error says nothing' % what
            if out is not None:
                rc = getattr(lib, row.output)(mgr.fb.ctx, *out)
                assert rc == code, '%s: %s%r returned %d, not %d' % (what, row.output, out, rc, code)
            _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
            assert (buf == SENTINEL).all(), '%s: the destination was written' % what
            got = file_of(row, ref.encode(mgr, cap, buf), what=what + ', the frame behind it')      # ... and the next frame is still right
            assert got == ref.data, '%s: the frame behind it: %s' % (what, first_difference(got, ref.data))


PLAIN = {'yuv444p': lambda w, h: np.empty((3, h, w), np.uint8), 'rgba8': lambda w, h: np.empty((h, w, 4), np.uint8),
         'rgba16': lambda w, h: np.empty((h, w, 4), np.uint16)}


def check_whole_path(mgr, row):
    """fl_output_X = fl_output(the row's format) + the encode: the plain call's frame is the encoder's source, the dither states
    afterwards are the plain call's, the frame is closed, and the encode is timed."""
    lib = _lib.load()
    assert row.whole, '%s: whole path: the row has none' % row.name
    for fmt, w, h, mids in row.whole:
        dim = mgr.fb.set_dim(w, h)
        fid = C.c_uint32()
        _lib.check(lib.fl_frame_begin(mgr.fb.ctx, C.byref(fid)))      # first: a frame chooses the lane whose buffers the calls below use
        _lib.check(lib.fl_debug_clear(mgr.fb.ctx, w, h, 0))
        front = (np.random.RandomState(11).rand(dim.ah * dim.astride, 4) * 1.3 - 0.1).astype(np.float32)
        mgr.fb.write('front', front)
        start = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
        plain = PLAIN[fmt](w, h)
        _lib.check(lib.fl_output(mgr.fb.ctx, w, h, _lib.OUT[fmt], plain.ctypes.data, 0))
        _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
        after_plain = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
        what = '%s: whole path: %s at %d x %d' % (row.name, fmt, w, h)
        assert not np.array_equal(start, after_plain), '%s: fl_output drew no dither' % what
        colour = plain if row.planar else plain[:, :, :3]
        assert min(plain.std(), colour.std()) > (1000 if fmt == 'rgba16' else 10) and (plain & 255).std() > 10, '%s: a flat frame' % what
        for mid in mids:
            what = '%s: whole path: %s at %d x %d, %r' % (row.name, fmt, w, h, mid)
            param = param_of(mgr, row, mid)
            mgr.fb.write('seeds', start)                      # (the frame stays open: the same lane, the same framebuffer)
            _lib.check(lib.fl_timings_reset(mgr.fb.ctx))
            cap = bound_of(row, w, h, mid)
            buf = mgr.fb._pinned((cap + SLACK,), 'u1')
            buf[:] = SENTINEL
            _lib.check(getattr(lib, row.output)(mgr.fb.ctx, w, h, *mid[row.lead:], buf.ctypes.data, 0, cap))
            ms = C.c_float(-1.0)
            _lib.check(lib.fl_frame_ms(mgr.fb.ctx, fid.value, C.byref(ms)))
            assert ms.value >= 0.0, '%s: the frame is not closed' % what
            _lib.check(lib.fl_ctx_sync(mgr.fb.ctx))
            H.assert_untouched(buf, cap, what)
            after = mgr.fb.read('seeds', (mgr.fb.nwalkers, 3), np.uint32)
            assert np.array_equal(after, after_plain), '%s: the dither states are not those behind fl_output' % what
            tm = mgr.timings()                                # (before anything else encodes: verify() may, and the direct call does)
            assert tm['encode_ms'] > 0.0 and tm['jpeg_ms'] == tm['encode_ms'], '%s: slot 5 of fl_timings_detail is %r' % (what, tm['encode_ms'])
            data = file_of(row, buf, param=param, what=what)
            verify(mgr, row, what, data, plain, mid, param)   # the plain call's frame is what was encoded
            direct, _ = encode(mgr, row, plain, mid, cap, what=what)
            got = file_of(row, direct, param=param, what=what + ', from the plain frame')
            assert got == data, '%s: %s of the plain frame differs: %s' % (what, row.encode, first_difference(got, data))


def check_timed(mgr, row):
    """The encode's kernels are in slot 5 of fl_timings_detail."""
    for ref in references(mgr, row, 'timed'):
        what = '%s: slot 5 of fl_timings_detail' % ref.what
        _lib.check(_lib.load().fl_timings_reset(mgr.fb.ctx))
        ms = mgr.timings()['encode_ms']
        assert ms == 0.0, '%s is %r behind fl_timings_reset' % (what, ms)
        ref.encode(mgr, ref.bound)
        ms = mgr.timings()['encode_ms']
        assert ms > 0.0, '%s is %r behind an encode' % (what, ms)
