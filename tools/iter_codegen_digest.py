#!/usr/bin/env python3
"""Digest of the machine code of every form of the iterate kernel (no GPU needed):
    python tools/iter_codegen_digest.py [--jobs N] [--lib libflame_hip.so] [--csrc cuburn_amd/csrc] > digest.txt
One line per kernel: the matrix cell, the sha256 of its code, its register, spill, scratch and LDS figures, the size of the code
and its static instruction counts by class (vector, scalar, LDS, branch).  Run it on two commits and diff the outputs: a
change that is meant to leave the generated code alone shows every line equal (hipRTC's compile is deterministic).

The per-genome kernels are compiled by fl_rtc_compile_check with FLAME_RTC_DUMP (csrc/rtc.hip); the ahead-of-time kernels
(k_iter<...>, the taps) are the device half of iter.hip, compiled with the Makefile's flags."""
import argparse, copy, ctypes as C, hashlib, os, re, subprocess, sys, tempfile
from concurrent.futures import ProcessPoolExecutor

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
LLVM = '/opt/rocm/lib/llvm/bin/'
FORMS = ((4, 0, 1), (4, 1, 1), (4, 1, 0), (4, 0, 2), (8, 0, 3), (8, 2, 1), (16, 2, 1), (16, 0, 3))          # (nw, count | 2 * sub-blocks, acc)
FLAGS = ('-DFL_HOIST_BUDGET=7', '-DFL_HOIST_BUDGET=5', '-DFL_HOIST_BUDGET=0', '-DFL_ITER_MERGE_MAX_XF=0',
         '-DFL_SORT_FULL_COPY=0 -DFL_SORT_LOCAL_TID=0')                                                   # at (4, 0, 1) only
# csrc/Makefile: CXXFLAGS and what it adds for iter.o
AOT_FLAGS = ['-O3', '-std=c++20', '--offload-arch=gfx950', '-ffp-contract=off', '-fPIC', '-fvisibility=hidden', '-Wall', '-Wno-unused-function',
             '-Wno-unused-value', '-Wno-unused-result', '-mllvm', '-structurizecfg-skip-uniform-regions=true', '-fno-slp-vectorize']


def genomes():
    sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
    from cuburn_amd import configs
    import chaos_model
    from flames import FRACTIONAL, many_xforms, three_boxes, with_opacity, spread_flame, linear_flame
    out = dict((k, configs.CONFIGS[k]()[0]) for k in ('cfg2', 'cfg3', 'cfg4', 'cfg5'))
    out['allvars'] = configs.allvars()[0]
    out['linear_post_final'] = linear_flame()[0]
    one = copy.deepcopy(out['cfg2'])
    one['xforms'] = dict(list(sorted(one['xforms'].items()))[:1])
    out['one_xform'] = one
    out['three_boxes_opac'] = three_boxes((0.5, 1.0, 0.25))[0]
    out['cfg3_opac5'] = with_opacity(out['cfg3'], ['5'])
    out['nine_boxes_chaos'] = chaos_model.nine_boxes(FRACTIONAL)[0]
    out['many_xforms_chaos'] = many_xforms(12, True)[0]
    spread = spread_flame(FRACTIONAL)[0]           # tests/test_gpu_chaos.py::test_every_kernel_form_with_opacity_and_a_final_xform
    spread['xforms']['1']['opacity'] = 0.5
    spread['final_xform'] = {'color': 0.0, 'color_speed': 0.0, 'pre_affine': configs._affine(10, 0.9, 0.02, -0.03),
                             'variations': {'linear': {'weight': 0.9}, 'spherical': {'weight': 0.02}}}
    out['chaos_opac_final'] = spread
    return out


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=600).stdout


def classes(disasm):
    """static instruction counts of a disassembly (llvm-objdump -d --no-show-raw-insn) by class"""
    n = dict(v=0, s=0, ds=0, br=0)
    for m in re.finditer(r'^\s+([a-z][a-z0-9_]+)\b', disasm, re.M):
        op = m.group(1)
        if op.startswith(('s_cbranch', 's_branch', 's_setpc', 's_swappc', 's_call')): n['br'] += 1
        elif op.startswith('ds_'): n['ds'] += 1
        elif op.startswith('s_'): n['s'] += 1
        elif op.startswith('v_'): n['v'] += 1
    return 'v=%(v)d s=%(s)d ds=%(ds)d br=%(br)d' % n


def kernels_of(co):
    """[(kernel name, resource figures)] from the code object's metadata note"""
    notes = run(LLVM + 'llvm-readelf', '--notes', co)
    out = []
    for block in re.split(r'\n\s+- \.agpr_count:', notes)[1:]:
        num = lambda key: int(re.search(r'\.' + key + r':\s+(\d+)', block).group(1))
        name = re.search(r'\.name:\s+(\S+)', block).group(1)
        out.append((name, 'vgpr=%d sgpr=%d vspill=%d sspill=%d scratch=%d lds=%d' % (
            num('vgpr_count'), num('sgpr_count'), num('vgpr_spill_count'), num('sgpr_spill_count'),
            num('private_segment_fixed_size'), num('group_segment_fixed_size'))))
    return out


def text_of(co, tmp):
    raw = os.path.join(tmp, 'text.bin')
    run(LLVM + 'llvm-objcopy', '-O', 'binary', '--only-section=.text', co, raw)
    return open(raw, 'rb').read()


def spec_cell(job):
    name, gnm, (nw, count, acc), flags = job
    cell = '%s nw=%d count=%d acc=%d flags=[%s]' % (name, nw, count, acc, flags)
    with tempfile.TemporaryDirectory() as tmp:
        os.environ['FLAME_RTC_DUMP'] = tmp
        os.environ['FLAME_RTC_FLAGS'] = flags
        sys.path[:0] = [REPO]
        import numpy as np
        from cuburn_amd import _lib
        from cuburn_amd.packer import GenomePacker
        pk = GenomePacker(gnm)
        prog, ops = np.ascontiguousarray(pk.prog, np.int32), np.ascontiguousarray(pk.ops_array, np.int32)
        log = C.create_string_buffer(8192)
        rc = _lib.load().fl_rtc_compile_check(prog.ctypes.data, len(prog), ops.ctypes.data, len(ops), nw, count, acc, log, len(log))
        if rc:
            return '%s rejected rc=%d' % (cell, rc)
        co = os.path.join(tmp, 'k_iter_spec.co')
        text = text_of(co, tmp)
        (_, res), = kernels_of(co)
        return '%s sha256=%s %s text=%d %s' % (cell, hashlib.sha256(text).hexdigest(), res, len(text),
                                              classes(run(LLVM + 'llvm-objdump', '-d', '--no-show-raw-insn', co)))


def aot_lines(csrc):
    """the device half of the ahead-of-time iter.hip: one line for the whole .text, one per kernel"""
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, 'iter_device.co')
        subprocess.run(['/opt/rocm/bin/hipcc'] + AOT_FLAGS + ['--cuda-device-only', '--no-gpu-bundle-output', '-c', os.path.join(csrc, 'iter.hip'), '-o', co],
                       check=True, timeout=1800)
        text = text_of(co, tmp)
        lines = ['aot iter.hip sha256=%s text=%d' % (hashlib.sha256(text).hexdigest(), len(text))]
        sect = run(LLVM + 'llvm-readelf', '-S', co)
        base = int(re.search(r'\.text\s+PROGBITS\s+([0-9a-f]+)', sect).group(1), 16)
        syms = {}
        for m in re.finditer(r'^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)', run(LLVM + 'llvm-readelf', '-sW', co), re.M):
            syms[m.group(3)] = (int(m.group(1), 16) - base, int(m.group(2)))
        for name, res in sorted(kernels_of(co)):
            off, size = syms[name]
            code = text[off:off + size]
            dis = run(LLVM + 'llvm-objdump', '-d', '--no-show-raw-insn', '--disassemble-symbols=' + name, co)
            lines.append('aot %s sha256=%s %s text=%d %s' % (name, hashlib.sha256(code).hexdigest(), res, size, classes(dis)))
        return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument('--lib', default='', help='the build of libflame_hip.so whose embedded iter.hip is compiled (default: the tree\'s)')
    ap.add_argument('--csrc', default=os.path.join(REPO, 'cuburn_amd', 'csrc'), help='where the ahead-of-time iter.hip lies')
    ap.add_argument('--only', default='', help='regular expression: only the cells it matches (the ahead-of-time part: aot)')
    a = ap.parse_args()
    if a.lib:
        os.environ['FLAME_HIP_LIB'] = os.path.abspath(a.lib)          # (cuburn_amd/_lib.py reads it on import)
    jobs = []
    for name, gnm in genomes().items():
        for form in FORMS:
            jobs.append((name, gnm, form, ''))
        for flags in FLAGS:
            jobs.append((name, gnm, FORMS[0], flags))
    if a.only:
        jobs = [j for j in jobs if re.search(a.only, '%s nw=%d count=%d acc=%d flags=[%s]' % (j[0], *j[2], j[3]))]
    with ProcessPoolExecutor(a.jobs) as pool:
        aot = None if a.only and not re.search(a.only, 'aot iter.hip') else pool.submit(aot_lines, a.csrc)
        for line in pool.map(spec_cell, jobs):
            print(line, flush=True)
        if aot:
            print('\n'.join(aot.result()), flush=True)


if __name__ == '__main__':
    main()
