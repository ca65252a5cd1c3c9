"""
The disk cache of the per-genome kernels' code objects (csrc/rtc_cache.h, FLAME_RTC_CACHE), without a GPU.

  * tests/rtc_cache_probe.cpp, a host program that includes rtc_cache.h alone, is built with -fsanitize=address,undefined and
    run as a program, one check per test: what was written is read back; a file cut anywhere, with any header byte or a payload
    byte flipped, with a byte too many, or another key's complete file under this name is a miss and is replaced by the next write;
    temporary files left behind are neither read nor in the way; the digest moves with every single input (each source, the spec
    header, each option, option order and boundaries, the architecture string and its target features, the version).
  * The digest of one fixed input is pinned as a literal: whoever changes the key function or the file layout changes
    rtc_cache::kFormatVersion (which is itself part of the key) and this literal with it.
  * fl_rtc_stats needs no device, and starts at zero.
  * The library end to end, as far as it goes without a device (hipRTC needs none): fl_rtc_compile_check in fresh processes —
    cold, warm, after a file was cut, with another option list, and with a directory that cannot be used.
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

from common import REPO

CSRC = os.path.join(REPO, 'cuburn_amd', 'csrc')
PINNED_DIGEST = '7683c35f8932560d02bb9cb8ab724e0f'       # rtc_cache_probe.cpp fixed_input(), format version 1
# MurmurHash3_x64_128, seed 0, of two well-known strings (h1 then h2, each little-endian): the function in the header is the
# published one, not a lookalike
MURMUR_HELLO = '029bbd41b3a7d8cb191dae486a901e5b'
MURMUR_PANGRAM = '6c1b07bc7bbc4be347939ac4a93c437a'


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    cxx = shutil.which('g++')
    if not cxx:
        pytest.skip('no g++')
    exe = str(tmp_path_factory.mktemp('rtc_cache_probe') / 'rtc_cache_probe')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-I', CSRC, os.path.join(REPO, 'tests', 'rtc_cache_probe.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_probe(exe, check, d):
    r = subprocess.run([exe, check, str(d)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and 'FAIL' not in r.stdout and not r.stderr, (check, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize('check', ['roundtrip', 'truncated', 'flipped', 'other_key', 'leftover_tmp', 'digest_inputs', 'dir'])
def test_probe(probe, tmp_path, check):
    assert run_probe(probe, check, tmp_path).startswith(check)


def test_header_includes_no_hip_header():
    src = open(os.path.join(CSRC, 'rtc_cache.h')).read()
    assert '#include <hip' not in src and '#include "' not in src


def test_digest_is_pinned_and_stable(probe, tmp_path):
    a, b = run_probe(probe, 'digest', tmp_path), run_probe(probe, 'digest', tmp_path)
    assert a == b
    out = dict(line.split(' ', 1) for line in a.strip().split('\n'))
    assert out['format'] == '1 header 44'
    assert out['hello'] == MURMUR_HELLO and out['empty'] == '0' * 32
    assert out['pangram'] == MURMUR_PANGRAM
    assert out['digest'] == PINNED_DIGEST, 'the key function changed: bump rtc_cache::kFormatVersion and pin the new digest'


def test_rtc_stats_need_no_device_and_start_at_zero(built):
    code = ('import ctypes as C, json, sys; sys.path.insert(0, %r)\n'
            'from cuburn_amd import _lib\n'
            'st = (C.c_uint64 * 8)(*([7] * 8)); rc = _lib.load().fl_rtc_stats(C.byref(st))\n'
            'from cuburn_amd import render\n'
            'print(json.dumps([rc, list(st), render.rtc_stats()]))\n' % REPO)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rc, st, named = json.loads(r.stdout.strip().split('\n')[-1])
    assert rc == 0 and st == [0] * 8
    assert list(named) == ['compiles', 'disk_hits', 'disk_misses', 'disk_writes', 'disk_rejects', 'jobs_queued',
                           'interp_launches_pending', 'spec_launches'] and set(named.values()) == {0}


def test_cli_switches_and_several_ids(tmp_path, capsys, monkeypatch):
    """--kernel-cache / --async-compile set the two variables before anything renders (they are no profile keys), and several
    IDs are walked in order, each told which one follows."""
    from cuburn_amd import __main__ as cli
    gold = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'genome_front.json')))
    (tmp_path / 'A.json').write_text(json.dumps(gold['db']['A']))
    monkeypatch.delenv('FLAME_RTC_CACHE', raising=False)
    monkeypatch.delenv('FLAME_RTC_ASYNC', raising=False)
    assert cli.main(['A', 'A', '-d', str(tmp_path), '--print']) == 0
    assert capsys.readouterr().out == (gold['json_text']['A/full'] + '\n') * 2
    assert 'FLAME_RTC_CACHE' not in os.environ and 'FLAME_RTC_ASYNC' not in os.environ
    seen = []
    monkeypatch.setattr(cli, 'render', lambda args, prof, flame=None, ahead=None: seen.append(
        (flame, ahead, os.environ.get('FLAME_RTC_CACHE'), os.environ.get('FLAME_RTC_ASYNC'), sorted(k for k in prof if 'cache' in k or 'async' in k))) or 0)
    monkeypatch.setenv('FLAME_RTC_CACHE', '')              # (monkeypatch restores what main() sets)
    monkeypatch.setenv('FLAME_RTC_ASYNC', '')
    assert cli.main(['A', 'B', 'C', '-d', str(tmp_path), '--kernel-cache', str(tmp_path / 'kc'), '--async-compile']) == 0
    assert seen == [('A', 'B', str(tmp_path / 'kc'), '1', []), ('B', 'C', str(tmp_path / 'kc'), '1', []), ('C', None, str(tmp_path / 'kc'), '1', [])]


# ------------------------------------------------------------------------------------------------ the library, no device
CHILD = r'''
import ctypes as C, json, sys
sys.path.insert(0, %(repo)r)
import numpy as np
from cuburn_amd import _lib, configs, render
from cuburn_amd.packer import GenomePacker
lib = _lib.load()
gnm, prof = configs.cfg1()
pk = GenomePacker(gnm)
prog, ops = np.ascontiguousarray(pk.prog, np.int32), np.ascontiguousarray(pk.ops_array, np.int32)
log = C.create_string_buffer(8192)
rcs = [lib.fl_rtc_compile_check(prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), 4, 0, 1, log, len(log)) for _ in range(%(n)d)]
print(json.dumps(dict(rc=rcs, stats=render.rtc_stats())))
'''


def child(env_extra, n=1):
    env = dict(os.environ, **env_extra)
    for k in ('FLAME_RTC_FLAGS', 'FLAME_RTC_DUMP'):
        if k not in env_extra:
            env.pop(k, None)
    r = subprocess.run([sys.executable, '-c', CHILD % dict(repo=REPO, n=n)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().split('\n')[-1])
    return out['rc'], out['stats'], r.stderr


def test_library_cold_warm_damaged_other_options(built, tmp_path):
    d = tmp_path / 'cache'                                # (missing: the library makes it)
    rc, st, err = child(dict(FLAME_RTC_CACHE=str(d)))
    if rc == [-5]:
        pytest.skip('libhiprtc is not installed')
    assert rc == [0] and err == ''
    assert (st['compiles'], st['disk_hits'], st['disk_misses'], st['disk_writes'], st['disk_rejects']) == (1, 0, 1, 1, 0), st
    files = sorted(os.listdir(d))
    assert len(files) == 1 and files[0].endswith('.co') and len(files[0]) == 32 + 3
    whole = (d / files[0]).read_bytes()
    assert whole[:8] == b'FLRTCCO\0' and whole[44:48] == b'\x7fELF' and int.from_bytes(whole[28:36], 'little') == len(whole) - 44
    print('code object: %d bytes' % (len(whole) - 44))
    # warm, twice in one process: no compiler run
    rc, st, err = child(dict(FLAME_RTC_CACHE=str(d)), n=2)
    assert rc == [0, 0] and err == ''
    assert (st['compiles'], st['disk_hits'], st['disk_misses'], st['disk_writes'], st['disk_rejects']) == (0, 2, 0, 0, 0), st
    # FLAME_RTC_DUMP still gets the header and the code object, from the cache too
    dump = tmp_path / 'dump'
    dump.mkdir()
    rc, st, err = child(dict(FLAME_RTC_CACHE=str(d), FLAME_RTC_DUMP=str(dump)))
    assert rc == [0] and st['compiles'] == 0 and (dump / 'k_iter_spec.co').read_bytes() == whole[44:]
    assert b'FL_SPEC_NXF' in (dump / 'flame_spec.h').read_bytes()
    # a cut file is a miss, and whole again afterwards
    (d / files[0]).write_bytes(whole[:len(whole) // 2])
    rc, st, err = child(dict(FLAME_RTC_CACHE=str(d)))
    assert rc == [0] and err == ''
    assert (st['compiles'], st['disk_hits'], st['disk_misses'], st['disk_writes'], st['disk_rejects']) == (1, 0, 0, 1, 1), st
    assert (d / files[0]).read_bytes() == whole           # (the compiler is deterministic)
    # another option list: another key, beside the first
    rc, st, err = child(dict(FLAME_RTC_CACHE=str(d), FLAME_RTC_FLAGS='-DFL_HOIST_BUDGET=5'))
    assert rc == [0] and (st['compiles'], st['disk_hits'], st['disk_misses'], st['disk_writes']) == (1, 0, 1, 1), st
    assert len(os.listdir(d)) == 2 and files[0] in os.listdir(d)
    assert not [f for f in os.listdir(d) if '.tmp.' in f]
    # no switch: no file is touched, the counters of the cache stay at zero
    rc, st, err = child({k: '' for k in ('FLAME_RTC_CACHE',)})
    assert rc == [0] and (st['compiles'], st['disk_hits'], st['disk_misses'], st['disk_writes'], st['disk_rejects']) == (1, 0, 0, 0, 0), st
    assert len(os.listdir(d)) == 2


def test_library_unusable_directory_warns_once(built, tmp_path):
    (tmp_path / 'file').write_text('x')
    bad = str(tmp_path / 'file' / 'cache')                 # its parent is a regular file: no permission bit decides this
    rc, st, err = child(dict(FLAME_RTC_CACHE=bad), n=2)
    if rc == [-5, -5]:
        pytest.skip('libhiprtc is not installed')
    assert rc == [0, 0]
    lines = [l for l in err.split('\n') if l]
    assert len(lines) == 1 and 'FLAME_RTC_CACHE' in lines[0] and 'without the kernel cache' in lines[0], err
    assert (st['compiles'], st['disk_hits'], st['disk_misses'], st['disk_writes'], st['disk_rejects']) == (2, 0, 0, 0, 0), st
