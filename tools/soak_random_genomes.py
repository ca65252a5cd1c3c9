#!/usr/bin/env python3
"""Extended run of tests/test_gpu_random_genomes.py::test_random_genome_parity over seeds outside the committed 48
(default schedule: fuse 256).   python tools/soak_random_genomes.py [first=49] [last=200]"""
import os, sys, traceback
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from cuburn_amd import render
import flames as F
import gpu_harness as H

first = int(sys.argv[1]) if len(sys.argv) > 1 else 49
last = int(sys.argv[2]) if len(sys.argv) > 2 else 200
mgr = render.RenderManager(device=0, nslots=1024, host_seed=23)
mgr_prod = render.RenderManager(device=0, host_seed=23)
bad = []
for seed in range(first, last + 1):
    try:
        H.check_random_genome(mgr, mgr_prod, seed)
        print('ok   seed %d (%d xforms)' % (seed, len(F.random_genome(seed)[0]['xforms'])), flush=True)
    except AssertionError as e:
        bad.append(seed)
        print('FAIL seed %d (%d xforms): %s' % (seed, len(F.random_genome(seed)[0]['xforms']), str(e)[:200]), flush=True)
print('%d seeds, %d failures: %s' % (last - first + 1, len(bad), bad))
