"""
CPU tests (no GPU) of csrc/launch_plan.h, the host arithmetic that cuts a frame into iterate launches: accumulator dimensions, the
tile layout of the binned accumulate, the size of a sample log + directory set, workgroups per tile and the schedule of rounds
per launch.  tests/launch_plan_dump.hip, a stand-alone program around the header (not the library, not a Python extension), is
built with the host sanitizers (address + undefined behaviour, errors fatal) and run once as a child process for the whole table
of cases; its lines are compared with the restatement below and with the figures the project records (DESIGN.md §3 / §4.1 / §4.2,
profiles/r05_launch_cap.txt, profiles/r05_bin_parts.txt).
"""
import os
import shutil
import subprocess

import pytest

from common import REPO

GUTTER, TILE_H, MAX_BINS = 12, 64, 2047


def layout(w, h, nw, bin_rounds=16, force_wide=0, forced_parts=0, write_rounds=1024, nslots=1024):
    """The `L` line of launch_plan_dump for one image and launch."""
    aw, ah = w + 2 * GUTTER, 16 * ((h + 2 * GUTTER + 15) // 16)
    astride = 32 * ((aw + 31) // 32)
    rows = (ah + TILE_H - 1) // TILE_H
    wide = int(((astride + 127) // 128) * rows > MAX_BINS or bool(force_wide))
    tile_w = 256 if wide else 128
    tiles_x = (astride + tile_w - 1) // tile_w
    nbins = tiles_x * rows
    records = bin_rounds * nw * 64
    region = records if wide else 2 * ((((records + 2) // 3) + 1) & ~1)       # three records per 64-bit word, an even number of them
    if forced_parts:
        parts = min(forced_parts, 64)
    elif nbins > 512:
        parts = ((12800 if wide else 6400) + nbins // 2) // nbins
    else:
        parts = (16384 if wide else 8192) // nbins
    if not forced_parts:
        parts = min(max(parts, 1), 16)
    nbatch = ((write_rounds + bin_rounds - 1) // bin_rounds) * nslots
    log_words, dir_words = nbatch * region + 8, nbins * nbatch
    return dict(astride=astride, ah=ah, wide=wide, tile_w=tile_w, tiles_x=tiles_x, nbins=nbins, region=region, parts=parts,
                nbatch=nbatch, log_words=log_words, dir_words=dir_words, set_bytes=4 * (log_words + dir_words))


L_KEYS = ('astride', 'ah', 'wide', 'tile_w', 'tiles_x', 'nbins', 'region', 'parts', 'nbatch', 'log_words', 'dir_words', 'set_bytes')


def under(rounds, sub_log2, cap):
    out, batch = [], 4
    while rounds:
        n = min(rounds, batch * (256 << sub_log2), cap) if cap else min(rounds, batch * (256 << sub_log2))
        out.append(n)
        rounds -= n
        batch += batch // 2
    return out


def schedule(rounds, sub_log2, nw, fixed):
    """(cap_short, cap_long, chosen cap, rounds per launch) of a binned frame: the long cap only where it saves a launch."""
    cap_s, cap_l = 1024 << sub_log2, (1536 if nw == 16 else 2304) << sub_log2
    if fixed:
        return cap_s, cap_l, fixed, under(rounds, sub_log2, fixed)
    s, l = under(rounds, sub_log2, cap_s), under(rounds, sub_log2, cap_l)
    return (cap_s, cap_l, cap_l, l) if len(l) < len(s) else (cap_s, cap_l, cap_s, s)


# (w, h, nw, bin_rounds, force_wide, forced_parts, write_rounds, nslots)
L_CASES = [(1920, 1080, 4, 16, 0, 0, 1024, 1024), (3840, 2160, 16, 16, 0, 0, 1024, 256), (3840, 2160, 8, 16, 0, 0, 1536, 1024),
           (7680, 4320, 16, 16, 0, 0, 1536, 1024), (7680, 4320, 16, 16, 0, 0, 1, 256),
           (1920, 1080, 4, 16, 0, 5, 1024, 1024), (3840, 2160, 8, 16, 0, 64, 64, 1024),       # FLAME_BIN_PARTS
           (1920, 1080, 4, 16, 1, 0, 1024, 1024), (640, 360, 4, 16, 1, 0, 683, 1280),         # FLAME_BIN_WIDE
           (640, 360, 4, 16, 0, 0, 683, 1280), (1, 1, 4, 16, 0, 0, 1, 1024), (33, 17, 8, 7, 0, 0, 15, 512),
           (5000, 3000, 8, 16, 0, 0, 2304, 1024), (6000, 3400, 8, 16, 0, 0, 1000, 1024), (12000, 12000, 16, 16, 0, 0, 16, 256)]
# (rounds, sub_log2, nw, fixed cap)
S_CASES = [(r, sub, nw, 0) for r in (1, 2, 4, 64, 1023, 1024, 1025, 2048, 2731, 3072, 3073, 4096, 4097, 5888, 5889, 8192, 20000, 100000)
           for sub, nw in ((0, 4), (0, 8), (0, 16), (1, 8), (2, 16))]
S_CASES += [(r, sub, nw, fixed) for r in (1, 63, 64, 65, 2731, 4096) for sub, nw in ((0, 4), (2, 16)) for fixed in (16, 64, 4096)]
U_CASES = [(1, 0), (1024, 0), (1025, 0), (4096, 1), (100000, 0), (100000, 2)]


@pytest.fixture(scope='module')
def dump(tmp_path_factory):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    exe = str(tmp_path_factory.mktemp('launch_plan') / 'launch_plan_dump')
    r = subprocess.run([hipcc, '-O1', '-g', '-std=c++20', '--offload-arch=gfx950', '-Xarch_host', '-fsanitize=address,undefined',
                        '-Xarch_host', '-fno-sanitize-recover=undefined', os.path.join(REPO, 'tests', 'launch_plan_dump.hip'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    args = []
    for c in L_CASES:
        args += ['L'] + [str(v) for v in c]
    for c in S_CASES:
        args += ['S'] + [str(v) for v in c]
    for c in U_CASES:
        args += ['U'] + [str(v) for v in c]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])         # a sanitizer report is on stderr and fatal
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[0] for l in lines] == ['L'] * len(L_CASES) + ['S'] * len(S_CASES) + ['U'] * len(U_CASES)
    nums = [[int(v) for v in l[1:]] for l in lines]
    return dict(L={c: dict(zip(L_KEYS, n)) for c, n in zip(L_CASES, nums)},
                S={c: (n[0], n[1], n[2], n[3:]) for c, n in zip(S_CASES, nums[len(L_CASES):])},
                U={c: n for c, n in zip(U_CASES, nums[len(L_CASES) + len(S_CASES):])})


def test_layout_set_size_and_parts_equal_the_restatement(dump):
    for c in L_CASES:
        assert dump['L'][c] == layout(*c), c
    assert any(v['wide'] for v in dump['L'].values()) and not all(v['wide'] for v in dump['L'].values())
    assert any(v['nbins'] > 512 and not v['wide'] for v in dump['L'].values())


def test_layout_figures_on_record(dump):
    hd = dump['L'][(1920, 1080, 4, 16, 0, 0, 1024, 1024)]
    assert (hd['astride'], hd['ah'], hd['wide'], hd['tile_w'], hd['tiles_x'], hd['nbins']) == (1952, 1104, 0, 128, 16, 16 * 18)
    assert hd['region'] == 2 * 1366 and hd['parts'] == 16
    assert hd['nbatch'] == 64 * 1024 and hd['set_bytes'] == 4 * (64 * 1024 * (2732 + 288) + 8)
    for nw_case in ((3840, 2160, 16, 16, 0, 0, 1024, 256), (3840, 2160, 8, 16, 0, 0, 1536, 1024)):
        k4 = dump['L'][nw_case]
        assert (k4['astride'], k4['ah'], k4['wide'], k4['tile_w'], k4['nbins'], k4['parts']) == (3872, 2192, 0, 128, 1085, 6)
    k8 = dump['L'][(7680, 4320, 16, 16, 0, 0, 1536, 1024)]
    assert (k8['astride'], k8['ah'], k8['wide'], k8['tile_w'], k8['tiles_x'], k8['nbins'], k8['parts']) == (7712, 4352, 1, 256, 31, 31 * 68, 6)
    assert k8['region'] == 16 * 16 * 64                     # 256x64 tiles: a record per 32-bit word
    assert k8['log_words'] * 4 > 2 ** 32                    # the 1536-round log of the 8K geometry: beyond 4 GB
    # FLAME_BIN_PARTS overrides the rule (and its cap of 16); FLAME_BIN_WIDE forces 256x64 tiles on a small image
    assert dump['L'][(1920, 1080, 4, 16, 0, 5, 1024, 1024)]['parts'] == 5
    assert dump['L'][(3840, 2160, 8, 16, 0, 64, 64, 1024)]['parts'] == 64
    forced = dump['L'][(1920, 1080, 4, 16, 1, 0, 1024, 1024)]
    assert (forced['wide'], forced['tile_w'], forced['tiles_x'], forced['nbins'], forced['region']) == (1, 256, 8, 8 * 18, 16 * 256)
    # an image beyond the 8191 tiles the wide layout can number is still laid out (fl_iterate refuses it)
    assert dump['L'][(12000, 12000, 16, 16, 0, 0, 16, 256)]['nbins'] > 8191


def test_schedules_equal_the_restatement(dump):
    for c in S_CASES:
        rounds = c[0]
        cap_s, cap_l, cap, plan = dump['S'][c]
        assert (cap_s, cap_l, cap, plan) == schedule(*c), c
        # any schedule: sums to the frame's rounds, every launch has write-enabled rounds and respects the cap, and it has as
        # many entries as the launch count that picked the cap
        assert sum(plan) == rounds and min(plan) >= 1 and max(plan) <= cap, c
        if not c[3]:
            counts = {k: len(under(rounds, c[1], k)) for k in (cap_s, cap_l)}
            assert len(plan) == min(counts.values()) and (cap == cap_l) == (counts[cap_l] < counts[cap_s]), c
    for c in U_CASES:
        assert dump['U'][c] == under(c[0], c[1], 0) and sum(dump['U'][c]) == c[0], c


def test_schedule_figures_on_record(dump):
    S = dump['S']
    assert S[(2731, 0, 4, 0)] == (1024, 2304, 1024, [1024, 1024, 683])         # cfg3: the long cap saves no launch
    assert S[(4096, 0, 4, 0)] == (1024, 2304, 2304, [1024, 1536, 1536])        # cfg5: three launches instead of four
    assert S[(4096, 0, 8, 0)][3] == [1024, 1536, 1536]
    assert S[(4096, 0, 16, 0)] == (1024, 1536, 1536, [1024, 1536, 1536])       # 16-wave geometry: the long cap stops at 1536
    assert S[(8192, 0, 16, 0)][3] == [1024, 1536, 1536, 1536, 1536, 1024] and S[(8192, 0, 4, 0)][3] == [1024, 1536, 2304, 2304, 1024]
    # sub-blocks: units and caps scale by 2 and 4 — the same launches for twice / four times the rounds
    assert S[(8192, 1, 8, 0)] == (2048, 4608, 4608, [2048, 3072, 3072])
    assert S[(4096, 1, 8, 0)] == (2048, 4608, 2048, [2048, 2048])
    assert S[(4096, 2, 16, 0)] == (4096, 6144, 4096, [4096])
    assert S[(20000, 2, 16, 0)][:3] == (4096, 6144, 6144) and S[(20000, 2, 16, 0)][3] == [4096, 6144, 6144, 3616]
    # FLAME_LAUNCH_ROUNDS: a fixed cap, taken as it is in every geometry
    assert S[(2731, 0, 4, 64)][2:] == (64, [64] * 42 + [43])
    assert S[(65, 2, 16, 64)][2:] == (64, [64, 1]) and S[(4096, 0, 4, 4096)][2:] == (4096, [1024, 1536, 1536])
    # one round, and fewer rounds than a usual fuse: one launch of as many write-enabled rounds (the fuse rounds come on top)
    assert S[(1, 0, 4, 0)][3] == [1] and S[(4, 0, 16, 0)][3] == [4] and S[(64, 2, 16, 0)][3] == [64]
    # without a cap (the atomic modes) the batches grow 4, 6, 9, 13 x 256
    assert dump['U'][(100000, 0)][:5] == [1024, 1536, 2304, 3328, 4864]
