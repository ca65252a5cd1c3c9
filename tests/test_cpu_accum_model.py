"""
CPU tests (no GPU) of the binned accumulate's model and of its hand-built logs (tests/accum_model.py, tests/accum_cases.py):
the format round-trips with garbage in every slot no run owns, the model is a plain histogram, the host's gate in front of
fl_debug_accum (accum_log_check, called here through fl_debug_accum_check: no device) and the model's `validate` agree on
every case and every invalid example, and the case list really holds each shape it is there for — asserted on the generated
directories and logs, not on the cases' names.
"""
import numpy as np
import pytest

import accum_cases as AC
import accum_model as M
from cuburn_amd import _lib


def encoded(name):
    c = AC.case(name)
    return (c,) + AC.encoded(name)


def host_check(w, h, log, dirw, nbatch_total, batch_records, nslots, nparts, wide):
    log, dirw = np.ascontiguousarray(log, np.uint32), np.ascontiguousarray(dirw, np.uint32)
    return _lib.load().fl_debug_accum_check(w, h, log.ctypes.data, log.size, dirw.ctypes.data, dirw.size,
                                            nbatch_total, batch_records, nslots, nparts, wide)


@pytest.mark.parametrize('name', AC.NAMES)
def test_log_round_trips_with_garbage_in_unowned_slots(name):
    c, log, dirw = encoded(name)
    got = M.decode_log(log, dirw, c.g)
    for a, b in zip(got, c.runs):
        assert np.array_equal(a, b)
    # other garbage, same records; and the garbage is there: ones in the spare words, and bit 63 of packed words
    log2, dir2 = M.encode_log(c.runs, c.g, np.random.default_rng(77))
    assert np.array_equal(dir2, dirw) and not np.array_equal(log2, log)
    assert np.array_equal(M.decode_log(log2, dir2, c.g).rec, c.runs.rec)
    assert log[-8:].any() and log2[-8:].any()
    if not c.g.wide:
        assert (log[1:c.g.nbatch * c.g.region:2] >> 31).any()


@pytest.mark.parametrize('name', AC.NAMES)
def test_accumulate_is_a_plain_histogram(name):
    c, log, dirw = encoded(name)
    runs = M.decode_log(log, dirw, c.g)
    got = M.accumulate(runs, c.g, c.palette, c.preload)
    ref = np.zeros((4, c.g.ncells), np.int64)
    x0 = (runs.tile % c.g.tiles_x) * c.g.tile_w + ((runs.rec.astype(np.int64) >> 8) & (c.g.tile_w - 1))
    y0 = (runs.tile // c.g.tiles_x) * 64 + (runs.rec.astype(np.int64) >> (8 + c.g.twl))
    slot = runs.batch // (c.g.nbatch // c.g.nslots)
    pal = np.asarray(c.palette, np.uint64).reshape(64, 256)[slot * 64 // c.g.nslots, runs.rec & 255]
    np.add.at(ref[0], y0 * c.g.astride + x0, 1)
    for k, sh in ((1, 36), (2, 18), (3, 0)):
        np.add.at(ref[k], y0 * c.g.astride + x0, ((pal >> np.uint64(sh)) & np.uint64(0x3ffff)).astype(np.int64))
    if c.preload is not None:
        ref += np.stack(M.unpack_cells(c.preload))
    assert np.array_equal(got, ref)
    # what the device has to hold: counts below 2^24 (exact in float32), no carry out of a packed cell's fields
    assert got[0].max(initial=0) < 2 ** 24
    if c.preload is not None:
        touched = np.stack(M.unpack_cells(c.preload))[0] > 0
        assert got[0][touched].max() <= 1023 and got[1:, touched].max() < 2 ** 18


@pytest.mark.parametrize('name', AC.NAMES)
def test_every_case_passes_the_model_and_the_host_gate(built, name):
    c, log, dirw = encoded(name)
    assert M.validate(c.g.w, c.g.h, log, dirw, *c.g.args()) is None
    rc = host_check(c.g.w, c.g.h, log, dirw, *c.g.args())
    assert rc == _lib.FL_OK, _lib.load().fl_last_error()
    for p in range(c.g.nparts):                             # every batch of a chunk finds its palette row among the staged ones
        for cb, ce, row_lo, nrows in c.g.chunks(p):
            rows = c.g.row_of(np.arange(cb, ce))
            assert rows.min() >= row_lo and rows.max() < row_lo + nrows


def test_invalid_examples_are_refused_by_the_model_and_by_the_host(built):
    examples = AC.invalid_examples()
    names = ' '.join(n for n, _ in examples)
    for what in ('nslots=', 'nbatch=0', 'nbatch+1', 'records=0', 'records=16385', 'parts=0', 'parts=65', 'log-1', 'log-spare', 'dir-1',
                 'layout', 'past-batch', 'gap', 'descending', 'overlap', 'cell-right', 'cell-below', 'high-bits', 'too-many'):
        assert what in names
    for name, args in examples:
        assert M.validate(*args) is not None, name
        assert host_check(*args) == _lib.FL_E_INVAL, name


def test_no_part_is_ever_without_batches():
    """b_lo == b_hi needs fewer batches than parts; a launch has at least 256 batches (a batch per slot, 256 slots) and at most
    64 parts, so the accumulate's `b_lo >= b_hi` exit cannot be reached through fl_debug_accum."""
    for nbatch in (256, 257, 512, 768):
        for nparts in range(1, 65):
            assert all(nbatch * p // nparts < nbatch * (p + 1) // nparts for p in range(nparts))


# ---- the shapes the list is there for, found in what was generated ---------------------------------------------------------------
def directory(name):
    c, log, dirw = encoded(name)
    d = dirw.reshape(c.g.nbins, c.g.nbatch).astype(np.int64)
    return c, log, dirw, d & 0xffff, d >> 16


def frames(kind):
    return [n for n in AC.NAMES if (AC.case(n).g.w, AC.case(n).g.h, AC.case(n).g.wide) == AC.FRAMES[kind]]


def test_parameters_cover_the_issue():
    gs = [AC.case(n).g for n in AC.NAMES]
    assert (gs[0].astride, gs[0].ah) == (224, 144)
    for kind, tiles in (('narrow', (2, 3)), ('wide', (3, 3)), ('ganged', (33, 17))):
        g = AC.case(frames(kind)[0]).g
        assert (g.tiles_x, g.tiles_y) == tiles
    g = AC.case(frames('ganged')[0]).g
    assert g.nbins == 561 and g.gang == 32 and g.nbins % 32 == 17
    for kind in ('narrow', 'wide'):
        sub = [AC.case(n).g for n in frames(kind)]
        assert {256, 1024, 16384} <= {g.nslots for g in sub}
        assert {1, 3} <= {g.per_slot for g in sub} and {256, 16384} <= {g.batch_records for g in sub}
        assert {1, 3, 16, 64} <= {g.nparts for g in sub}
        assert any(g.nbatch == 256 and g.nparts == 64 for g in sub)              # parts of four batches
        assert any(len(g.chunks(0)) > 4 for g in sub if g.nparts == 1)           # the re-staging loop
        assert any(g.big_thr == 16 for g in sub)
        pals = [np.stack(M.unpack_cells(AC.case(n).palette)) for n in frames(kind)]
        assert any((p[1:] == 255).all() for p in pals)
        rows = next(p for p in pals if not (p[1:] == 255).all())
        assert len({tuple(r) for r in rows[1:].reshape(3, 64, 256).transpose(1, 0, 2).reshape(64, -1)}) == 64      # every row its own colours


@pytest.mark.parametrize('kind', ['narrow', 'wide'])
def test_run_alignment_shapes(kind):
    pairs_last, pairs_any, singles, tile0, edges = set(), set(), set(), set(), set()
    for name in frames(kind):
        c, log, dirw, cnt, first = directory(name)
        g = c.g
        t, b = np.nonzero((cnt >= 1) & (cnt <= 4))
        rf, rl, n = first[t, b], first[t, b] + cnt[t, b] - 1, cnt[t, b]
        for ti, bi, f, l, k in zip(t, b, rf, rl, n):
            pairs_any.add((f % 3, l % 3))
            if ti == g.nbins - 1:
                pairs_last.add((f % 3, l % 3, k))
            if ti == 0:
                tile0.add(k)
            if k == 1 and 0 < ti < g.nbins - 1 and cnt[ti - 1, bi] and cnt[ti + 1, bi]:
                singles.add(f % 3)
            for p, (lo, hi) in enumerate(g.parts()):
                if p in (0, g.nparts - 1) and bi in (lo, hi - 1):
                    edges.add((p == 0, bi == lo))
    nine = {(f, l) for f in range(3) for l in range(3)}
    assert pairs_any == nine
    assert {(f, l) for f, l, _ in pairs_last} == nine and {k for _, _, k in pairs_last} == {1, 2, 3, 4}
    assert tile0 >= {1, 2, 3, 4}
    assert singles == {0, 1, 2}            # a one-record run in each slot of a word, a neighbour on either side (slot 1: in the same word)
    assert edges == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize('kind', ['narrow', 'wide'])
def test_empty_run_shapes(kind):
    seen = set()
    for name in frames(kind):
        c, log, dirw, cnt, first = directory(name)
        g = c.g
        if cnt.sum() == 0:
            seen.add('launch without a record')
            continue
        if ((cnt == 0) & (first == 0)).any():
            seen.add('empty at 0')
        if ((cnt == 0) & (first > 0)).any():
            seen.add('empty behind records')
        if (cnt.sum(1) == 0).any():
            seen.add('tile without a record')
        by = {}
        for p, wave, g0, ge, tot in M.group_totals(dirw, g):
            by.setdefault(p, []).append((wave, g0, ge, tot))
        for p, groups in by.items():
            for (w0, a0, a1, t0), (w1, b0, b1, t1), (w2, c0, c1, t2) in zip(groups, groups[1:], groups[2:]):
                full = (t0 > 0) & (t1 == 0) & (t2 > 0)
                if full.any() and b1 - b0 == 64:
                    seen.add('empty group between full ones')
                    if (w0, w1, w2) == (0, 1, 2) and b0 == a1 and c0 == b1:
                        seen.add('... on three waves of one workgroup')
    assert seen == {'launch without a record', 'empty at 0', 'empty behind records', 'tile without a record',
                    'empty group between full ones', '... on three waves of one workgroup'}


@pytest.mark.parametrize('kind', ['narrow', 'wide'])
def test_group_total_shapes(kind):
    totals, sixteen = set(), 0
    for name in frames(kind):
        c, log, dirw, cnt, first = directory(name)
        groups = M.group_totals(dirw, c.g)
        for p, wave, g0, ge, tot in groups:
            totals |= set(int(x) for x in tot)
        for p in range(c.g.nparts):
            mine = [(wave, tot) for q, wave, g0, ge, tot in groups if q == p]
            if sorted(w for w, _ in mine) == list(range(16)):
                for t in range(c.g.nbins):
                    sixteen += len({int(tot[t]) for _, tot in mine}) == 16
    assert totals >= set(AC.TOTALS[kind])
    assert sixteen >= 2                    # sixteen waves, sixteen different totals: in the first part and in the last


@pytest.mark.parametrize('kind', ['narrow', 'wide'])
def test_long_run_shape(kind):
    found = set()
    for name in frames(kind):
        c, log, dirw, cnt, first = directory(name)
        for t, b in zip(*np.nonzero(cnt == 16384)):
            assert c.g.batch_records == 16384
            alone = cnt[:, max(b - 1, 0)].sum() + cnt[:, min(b + 1, c.g.nbatch - 1)].sum() == (0 if 0 < b < c.g.nbatch - 1 else 16384)
            if alone:
                found.add('first tile' if t == 0 else 'last tile' if t == c.g.nbins - 1 else 'other')
    assert found >= {'first tile', 'last tile'}


@pytest.mark.parametrize('kind', ['narrow', 'wide', 'ganged'])
def test_hot_cell_shapes(kind):
    seen = set()
    for name in frames(kind):
        c, log, dirw, cnt, first = directory(name)
        g = c.g
        model = M.accumulate(c.runs, g, c.palette, c.preload)
        if len(c.runs.rec) and model[0].max() == len(c.runs.rec):        # a point attractor: every record of every batch
            assert (cnt.sum(0) == g.batch_records).all()
            seen.add('point')
            if model[0][g.ncells - 1]:
                seen.add('point in the last cell')
        if kind == 'ganged' or g.nbatch > 4096:
            continue
        for p, t, g0, step, trigger, sets in M.hot_steps(log, dirw, g):
            if trigger == 47 and max(sets) == 47:
                seen.add('47 lanes')
            if trigger == 48 and sets[1] == 15:
                seen.add('48 lanes, group of 15')
            if trigger == 48 and sets[1] == 16:
                seen.add('48 lanes, group of 16')
    want = {'point', 'point in the last cell'}
    assert seen == (want if kind == 'ganged' else want | {'47 lanes', '48 lanes, group of 15', '48 lanes, group of 16'})


@pytest.mark.parametrize('kind', ['narrow', 'wide'])
def test_fill_threshold_shapes(kind):
    lds, big, pre = set(), set(), set()
    for name in frames(kind):
        c, log, dirw, cnt, first = directory(name)
        g = c.g
        part, cell, hits = M.part_hits(c.runs, g)
        if hits.max(initial=0) > 100000:                    # (the point attractors)
            continue
        quiet = not M.takes_hot_path(M.hot_steps(log, dirw, g)) if g.nbatch <= 4096 else False
        if quiet:
            lds |= {255, 256, 257} & set(int(h) for h in hits)
            for h in (g.big_thr - 1, g.big_thr, g.big_thr + 1):
                if (hits == h).any():
                    big.add((g.nparts, h - g.big_thr))
        if c.preload is not None:
            n0 = M.unpack_cells(c.preload)[0]
            total = M.accumulate(c.runs, g, c.palette, c.preload)
            for k in np.nonzero(n0)[0]:
                adds = hits[cell == k]
                assert len(adds) == g.nparts and n0[k] + adds.sum() <= 1023 and total[1:, k].max() < 2 ** 18
                pre.add((int(n0[k]), bool(n0[k] + adds.sum() - adds.min() >= 512)))
    assert lds == {255, 256, 257}
    assert big >= {(n, k) for n in (16, 64) for k in (-1, 0, 1)}
    assert pre == {(500, True), (500, False), (511, True)}       # with and without an add that finds 512 hits (511: always, from the second part on)


@pytest.mark.parametrize('kind', ['narrow', 'wide'])
def test_palette_chunk_shapes(kind):
    crossing = row63 = False
    for name in frames(kind):
        c, log, dirw, cnt, first = directory(name)
        g = c.g
        per_batch = cnt.sum(0)
        for p in range(g.nparts):
            chunks = g.chunks(p)
            for (cb, ce, r0, n0), (cb2, ce2, r1, n1) in zip(chunks, chunks[1:]):
                # records either side of the boundary, and the part does not begin on a row's first slot
                if per_batch[ce - 1] and per_batch[cb2] and (chunks[0][0] // g.per_slot) % g.spr:
                    crossing = True
            if chunks[-1][1] == g.nbatch and per_batch[g.nbatch - 1] and g.row_of(g.nbatch - 1) == 63:
                row63 = True
    assert crossing and row63


def test_ganged_shapes():
    tiles = set()
    for name in frames('ganged'):
        c, log, dirw, cnt, first = directory(name)
        tiles |= set(int(t) for t in np.nonzero(cnt.sum(1))[0])
    assert {0, 31, 32, 543, 544, 560} <= tiles
