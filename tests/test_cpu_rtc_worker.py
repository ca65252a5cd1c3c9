"""
The compile thread of FLAME_RTC_ASYNC (csrc/rtc.hip) without a device: tests/rtc_worker_probe.cpp is a host program around
rtc.hip itself (hipRTC needs no GPU), built with hipcc and run as a program, one check per process:

  * a process that ends while a compile is in flight waits for it and exits 0.  Found as a benchmark child that died of
    SIGSEGV after printing its results: the exiting thread ran the destructors the compiler had registered while it first
    worked, the worker was still inside the code object manager, and ~Worker (the join) came after them.  worker() now makes
    the process's first compile — an empty kernel — on the calling thread before the worker exists, and the worker registers
    its join again after every compile;
  * held jobs are left alone and dropped when the process ends;
  * the job asked about last runs first.
"""
import os
import shutil
import subprocess
import sys

import pytest

from common import REPO

CSRC = os.path.join(REPO, 'cuburn_amd', 'csrc')


@pytest.fixture(scope='module')
def probe(built, tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    tmp = tmp_path_factory.mktemp('rtc_worker_probe')
    # the embedded sources, as csrc/Makefile makes them
    r = subprocess.run([sys.executable, os.path.join(CSRC, 'embed.py'), str(tmp / 'rtc_sources.inc'), 'rtc_src_iter=iter.hip',
                        'rtc_src_variations=variations.h', 'rtc_src_device=flame_device.h', 'rtc_src_abi=../../include/flame_hip.h'],
                       cwd=CSRC, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    exe = str(tmp / 'rtc_worker_probe')
    r = subprocess.run([hipcc, '-O1', '-g', '-std=c++20', '--offload-arch=gfx950', '-x', 'hip', '-I', CSRC, '-I', str(tmp),
                        os.path.join(REPO, 'tests', 'rtc_worker_probe.cpp'), '-o', exe, '-ldl', '-lpthread'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    # a real flame_spec.h: cfg2's four-wave binned kernel, kept by FLAME_RTC_DUMP in a process of its own
    code = ('import ctypes as C, sys; sys.path.insert(0, %r)\n'
            'import numpy as np\n'
            'from cuburn_amd import _lib, configs\n'
            'from cuburn_amd.packer import GenomePacker\n'
            'pk = GenomePacker(configs.cfg2()[0])\n'
            'prog, ops = np.ascontiguousarray(pk.prog, np.int32), np.ascontiguousarray(pk.ops_array, np.int32)\n'
            'log = C.create_string_buffer(8192)\n'
            'print(_lib.load().fl_rtc_compile_check(prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), 4, 0, 1, log, len(log)))\n' % REPO)
    env = dict(os.environ, FLAME_RTC_DUMP=str(tmp))
    env.pop('FLAME_RTC_FLAGS', None)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    if r.stdout.strip().split('\n')[-1] == '-5':
        pytest.skip('libhiprtc is not installed')
    assert os.path.getsize(str(tmp / 'flame_spec.h')) > 100
    return exe, str(tmp / 'flame_spec.h')


@pytest.mark.parametrize('rep', range(3))
def test_process_may_end_in_the_middle_of_a_compile(probe, rep):
    exe, header = probe
    r = subprocess.run([exe, 'exit_mid_compile', header], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert 'compiles entered' in r.stdout


@pytest.mark.parametrize('check', ['held', 'order'])
def test_worker(probe, check):
    exe, header = probe
    r = subprocess.run([exe, check, header], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith('ok ' + check), (r.returncode, r.stdout, r.stderr[-2000:])
