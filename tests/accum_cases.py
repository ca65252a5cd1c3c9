"""
Hand-built sample logs for the binned accumulate (tests/accum_model.py is the format and the model; tests/test_cpu_accum_model.py
asserts that every shape named here is really in the generated directories; tests/test_gpu_accum_log.py runs them).

A case is a geometry, a palette, the runs and — some — preloaded accumulator cells.  Three frame geometries: `narrow` 200 x 110
(2 x 3 tiles of 128x64, ragged right and bottom: k_accum_tiles_p3), `wide` 600 x 150 in 256x64 tiles (3 x 3, ragged both ways:
k_accum_tiles<8>), `ganged` 4200 x 1064 (33 x 17 = 561 tiles of 128x64: gangs of 32, the last gang of 17).  The batch
parameters (slots, batches per slot, records per batch, workgroups per tile) are the P_* tuples below.
"""
import collections
import functools

import numpy as np

import accum_model as M

FRAMES = dict(narrow=(200, 110, 0), wide=(600, 150, 1), ganged=(4200, 1064, 0))

# (nslots, batches per slot, batch_records, nparts)
P_ONE = (256, 1, 256, 1)            # one workgroup per tile: 16 palette chunks of 16 batches, the re-staging loop
P_THREE = (256, 3, 256, 3)          # 3 divides neither the batches' slots nor the chunks: parts begin inside a slot's row
P_SIX = (1024, 1, 256, 3)           # parts of 341 / 342 batches: six groups per part on waves 0..5
P_16 = (1024, 1, 256, 16)           # parts of 64 batches = one group, big_thr = 64
P_64 = (1024, 3, 256, 64)           # parts of 48 batches, big_thr = 16
P_FOUR = (256, 1, 256, 64)          # 256 batches for 64 workgroups per tile: parts of four batches
P_MANY = (16384, 1, 256, 16)        # the largest slot count: parts of 1024 batches, a group for each of the sixteen waves
P_LONG = (256, 1, 16384, 3)         # batches of 16384 records

TOTALS = dict(narrow=(63, 64, 65, 128, 129, 192, 193), wide=(255, 256, 257, 512, 513))
TOTALS16 = dict(narrow=(63, 64, 65, 128, 129, 192, 193, 1, 2, 3, 127, 191, 0, 66, 130, 194),
                wide=(255, 256, 257, 512, 513, 1, 2, 254, 258, 511, 514, 0, 3, 64, 65, 768))

Case = collections.namedtuple('Case', 'name g runs palette preload seed')


def palette_rows():
    """Every row its own colours, every column too: a wrong row or column changes all three sums."""
    row, col = np.arange(M.PAL_H)[:, None], np.arange(M.PAL_W)[None, :]
    return M.pack_cells(1 + 0 * (row + col), (row * 4 + col // 64) & 255, (col + row * 3) & 255, (row * 37 + col * 11 + 5) & 255)


def palette_max():
    """Every field at the largest value the palette kernel writes (csrc/interp.hip: min(255, .))."""
    return M.pack_cells(np.ones((M.PAL_H, M.PAL_W), np.int64), 255, 255, 255)


class Builder(object):
    def __init__(self, name, frame, params, seed, palette=palette_rows):
        w, h, wide = FRAMES[frame]
        self.name, self.seed, self.palette = name, seed, palette()
        self.g = M.Geometry(w, h, wide, *params)
        self.rng = np.random.default_rng(seed)
        self.b, self.t, self.r = [], [], []
        self.preload = None
        self.used = set()

    # records -----------------------------------------------------------------------------------------------------------------
    def cell(self, tile, lx, ly, ci=None, n=1):
        """n records of one cell of `tile` (random palette columns unless given)."""
        ci = self.rng.integers(0, 256, n) if ci is None else np.full(n, ci)
        return self.g.record(np.full(n, lx), np.full(n, ly), ci)

    def spread(self, tile, n, distinct=False):
        """n records in random cells of `tile` inside the accumulator; `distinct`: no cell twice."""
        nx, ny = self.g.tile_extent(tile)
        c = self.rng.choice(nx * ny, n, replace=False) if distinct else self.rng.integers(0, nx * ny, n)
        return self.g.record(c % nx, c // nx, self.rng.integers(0, 256, n))

    def add(self, batch, tile, recs):
        recs = np.atleast_1d(recs)
        self.b.append(np.full(len(recs), batch)); self.t.append(np.full(len(recs), tile)); self.r.append(recs)

    def run(self, batch, tile, recs, rfirst=0, right=0):
        """A run of `tile` that begins at record `rfirst` of its batch: that many records go to the tile in front of it (tile 0
        can only begin at 0), `right` records to the tile behind it."""
        assert batch not in self.used, 'one designed run per batch'
        self.used.add(batch)
        if rfirst:
            assert tile > 0
            self.add(batch, tile - 1, self.spread(tile - 1, rfirst))
        self.add(batch, tile, recs)
        if right:
            self.add(batch, tile + 1, self.spread(tile + 1, right))

    def edge_batches(self):
        """First and last batch of the first and the last part, then of every other part, then the batches in between."""
        parts = self.g.parts()
        order = [parts[0][0], parts[0][1] - 1, parts[-1][0], parts[-1][1] - 1]
        order += [b for lo, hi in parts[1:-1] for b in (lo, hi - 1)]
        order += list(range(self.g.nbatch))
        return list(dict.fromkeys(order))

    def edge_tiles(self):
        n = self.g.nbins
        return list(dict.fromkeys([n - 1, 0, n // 2, n - 2, 1]))

    def build(self):
        cat = (lambda x: np.concatenate(x)) if self.b else (lambda x: np.zeros(0, np.int64))
        return Case(self.name, self.g, M.make_runs(cat(self.b), cat(self.t), cat(self.r)), self.palette, self.preload, self.seed)


# ---- the shapes ----------------------------------------------------------------------------------------------------------------
def c_random(bd):
    """Every batch a random number of records over random tiles: what a flame gives, thin enough that no cell fills."""
    g = bd.g
    for b in range(g.nbatch):
        n = int(bd.rng.integers(0, min(g.batch_records, 256) + 1)) if b % 7 else 0
        tiles = np.sort(bd.rng.integers(0, g.nbins, n))
        for t in np.unique(tiles):
            bd.add(b, int(t), bd.spread(int(t), int((tiles == t).sum())))


def c_nothing(bd):
    """A launch without a record: every count zero, the log all garbage."""


def c_align(bd):
    """rfirst % 3 x rlast % 3, all nine pairs, as counts 1..4 from every first slot; in the last tile (nothing behind the run in
    its batch), in the tile in front of it (a neighbour on either side) and in tile 0 (rfirst = 0 only); the one-record runs
    among them sit in each of a word's three slots between two non-empty neighbours.  First and last batches of the parts."""
    g, batches = bd.g, iter(bd.edge_batches())
    last = g.nbins - 1
    for tile, right in ((last, 0), (last - 1, 2), (0, 1)):
        for rfirst in ((0, 1, 2, 3, 4, 5) if tile else (0,)):
            for count in (1, 2, 3, 4):
                bd.run(next(batches), tile, bd.spread(tile, count, distinct=True), rfirst=rfirst, right=right)


def c_empty_group(bd):
    """64 batches without a record between two groups of full ones, per part: the middle wave finds a total of zero."""
    g = bd.g
    for p, (lo, hi) in enumerate(g.parts()):
        groups = [(g0, ge) for _, g0, ge in g.groups(p)]
        assert len(groups) >= 3
        tile = bd.edge_tiles()[p % 3]
        for g0, ge in (groups[0], groups[2]):
            for b in range(g0, ge):
                bd.run(b, tile, bd.spread(tile, 5 + b % 4), rfirst=(b % 3 if tile else 0))


def _group_with_total(bd, tile, g0, ge, total):
    """Runs of `tile` in the batches [g0, ge) whose log words (128x64 tiles) or records (256x64) add up to `total`."""
    g, n = bd.g, ge - g0
    per = bd.rng.multinomial(total, np.full(n, 1.0 / n))
    for b, wds in zip(range(g0, ge), per):
        if wds == 0:
            continue
        if g.wide:
            bd.run(b, tile, bd.spread(tile, int(wds)), rfirst=(b % 3 if tile else 0))
        else:
            assert wds <= 80
            rfirst = b % 3 if tile else 0
            count = max(1, 3 * int(wds) - rfirst - b % 2)       # the run ends in word rfirst // 3 + wds - 1, in any slot
            bd.run(b, tile, bd.spread(tile, count), rfirst=rfirst, right=(1 if tile + 1 < g.nbins else 0))


def c_totals(bd):
    """One wave's group with each total at which the rotation of the register sets wraps (63 .. 193 words; 255 .. 513 records)."""
    g = bd.g
    totals = TOTALS['wide' if g.wide else 'narrow']
    tiles = bd.edge_tiles()
    groups = [(g0, ge) for p in range(g.nparts) for _, g0, ge in g.groups(p) if ge - g0 >= 16]
    assert len(groups) >= len(totals)
    for k, total in enumerate(totals):
        g0, ge = groups[k * len(groups) // len(totals)]
        _group_with_total(bd, tiles[k % len(tiles)], g0, ge, total)


def c_totals16(bd):
    """All sixteen waves of a workgroup with different totals, in the first and the last part."""
    g = bd.g
    totals = TOTALS16['wide' if g.wide else 'narrow']
    for p, tile in ((0, g.nbins - 1), (g.nparts - 1, 0)):
        groups = g.groups(p)
        assert sorted(wave for wave, _, _ in groups) == list(range(16))
        for wave, g0, ge in groups:
            _group_with_total(bd, tile, g0, ge, totals[(wave + p) % 16])


def c_long(bd):
    """A batch whose 16384 records all belong to one tile, next to empty batches: in the first tile and in the last."""
    g = bd.g
    lo, hi = g.parts()[1]
    bd.run(lo, 0, bd.spread(0, g.batch_records))
    bd.run(g.nbatch - 1, g.nbins - 1, bd.spread(g.nbins - 1, g.batch_records))
    bd.run(3, g.nbins // 2, bd.spread(g.nbins // 2, 40), rfirst=2)


def _hot(bd, lanes, group):
    """Runs that are alone in their group, so that a step begins with their first record: `lanes` of the step's first 64 records
    (first slots) in one cell, `group` live records of the second record set in another; everything else in cells of its own."""
    g = bd.g
    parts = g.parts()
    for k, b in enumerate((parts[0][0], parts[0][1] - 1, parts[-1][0], parts[-1][1] - 1)):     # (a group and tile for each)
        tile = bd.edge_tiles()[k % 2]
        nx, ny = g.tile_extent(tile)
        if g.wide:
            recs = bd.spread(tile, 256, distinct=True)
            hot, second = recs[0] >> 8, recs[64] >> 8
            recs[:lanes] = (hot << 8) | (recs[:lanes] & 255)
            recs[64:64 + group] = (second << 8) | (recs[64:64 + group] & 255)
        else:
            recs = bd.spread(tile, 192, distinct=True)
            hot, second = recs[0] >> 8, recs[1] >> 8
            recs[0:3 * lanes:3] = (hot << 8) | (recs[0:3 * lanes:3] & 255)
            recs[1:3 * group:3] = (second << 8) | (recs[1:3 * group:3] & 255)
        bd.run(b, tile, recs)


def c_hot47(bd):
    """47 of a step's first 64 records in one cell: one short of the examined path, everything goes through the LDS tile."""
    _hot(bd, 47, 16)


def c_hot48_15(bd):
    """48: the step is examined, the 48 go to the floats in one piece; the second set's group of 15 stays in the tile."""
    _hot(bd, 48, 15)


def c_hot48_16(bd):
    """48, and a group of exactly 16 in the second set: both are spilled."""
    _hot(bd, 48, 16)


def _point(bd, tile, lx, ly):
    g = bd.g
    assert g.nbatch * g.batch_records < 2 ** 24
    for b in range(g.nbatch):
        bd.add(b, tile, bd.cell(tile, lx, ly, n=g.batch_records))


def c_point(bd):
    """A point attractor: every record of every batch in one cell inside the first tile."""
    _point(bd, 0, 37, 21)


def c_point_corner(bd):
    """The same in the last cell of the accumulator, the corner of the last tile."""
    nx, ny = bd.g.tile_extent(bd.g.nbins - 1)
    _point(bd, bd.g.nbins - 1, nx - 1, ny - 1)


def _fill(bd, part, tile, hits, from_end=False):
    """Cells of `tile` that receive exactly hits[k] records from ONE part: a record per word's middle slot (every 3rd record),
    between records of cells of their own, so that no step looks hot."""
    g = bd.g
    lo, hi = g.parts()[part]
    nx, ny = g.tile_extent(tile)
    cells = bd.rng.choice(nx * ny, len(hits), replace=False)
    mids = np.concatenate([bd.g.record(np.full(h, c % nx), np.full(h, c // nx), bd.rng.integers(0, 256, h)) for c, h in zip(cells, hits)])
    per = 63 if hi - lo >= (len(mids) + 62) // 63 else 84
    assert hi - lo >= (len(mids) + per - 1) // per
    others = np.setdiff1d(np.arange(nx * ny), cells)        # (the records around them stay clear of the counted cells)
    for k in range(0, len(mids), per):
        m = mids[k:k + per]
        c = bd.rng.choice(others, 3 * len(m))
        recs = g.record(c % nx, c // nx, bd.rng.integers(0, 256, len(c)))
        recs[1::3] = m
        bd.run(hi - 1 - k // per if from_end else lo + k // per, tile, recs, rfirst=(3 * ((k // per) % 2) if tile else 0))


def c_fill(bd):
    """Cells that receive 255, 256, 257 hits (the early drain of the LDS tile) and big_thr - 1, big_thr, big_thr + 1 (the tile
    add's direct spill) within one workgroup: in the first part and tile 0, in the last part and the last tile."""
    g = bd.g
    hits = sorted({255, 256, 257, g.big_thr - 1, g.big_thr, g.big_thr + 1})
    lo, hi = g.parts()[0]
    hits = [h for h in hits if h < 1023 and sum(x for x in hits if x <= h) <= (hi - lo) * 84]
    _fill(bd, 0, 0, hits)
    _fill(bd, g.nparts - 1, g.nbins - 1, hits, from_end=True)


def c_preload(bd):
    """Packed cells that hold 500 and 511 hits before the launch; every part adds a little: the adds that find 512 or more take
    the cell to the floats (`full`).  500 + 3 x 6 and 511 + 3 x 1: no count passes 1023, no field 2^18."""
    g = bd.g
    assert g.nparts == 3
    tile = g.nbins - 1
    nx, ny = g.tile_extent(tile)
    x0, y0 = g.tile_origin(tile)
    bd.preload = np.zeros(g.ncells, np.uint64)
    for (lx, ly), n0, per_part in (((3, 2), 500, 6), ((nx - 1, ny - 1), 511, 1), ((5, 7), 511, 6), ((9, 1), 500, 1)):
        bd.preload[(y0 + ly) * g.astride + x0 + lx] = M.pack_cells(n0, n0 * 255, n0 * 100, n0 * 3)
        for p, (lo, hi) in enumerate(g.parts()):
            recs = np.concatenate([bd.cell(tile, lx, ly, n=per_part), bd.spread(tile, 9)])
            bd.add(lo + (n0 + per_part) % 5, tile, bd.rng.permutation(recs))


def c_chunks(bd):
    """Records in the first and the last batch of every palette chunk of every part: a batch range that crosses chunks keeps
    every batch on its own palette row, up to row 63."""
    g = bd.g
    for p in range(g.nparts):
        for k, (cb, ce, _, _) in enumerate(g.chunks(p)):
            for b in {cb, ce - 1}:
                tile = bd.edge_tiles()[(k + b) % 3]
                bd.run(b, tile, bd.spread(tile, 7, distinct=True), rfirst=(b % 3 if tile else 0))


def c_gang(bd):
    """Runs in the first and last tile of the first gang, of the ragged last gang and of one in between, over the batch edges."""
    g = bd.g
    assert g.gang == 32 and g.nbins % 32
    last_gang = g.nbins // 32 * 32
    batches = iter(bd.edge_batches())
    for tile in (0, 31, 32, 287, 288, last_gang - 1, last_gang, g.nbins - 2, g.nbins - 1):
        for rfirst in ((0, 1, 2) if tile else (0,)):
            for count in (1, 4, 200):
                bd.run(next(batches), tile, bd.spread(tile, count), rfirst=rfirst, right=(1 if tile + 1 < g.nbins else 0))


SPECS = collections.OrderedDict()


def _spec(shape, frame, params, palette=palette_rows):
    p = '-'.join(str(x) for x in params)
    SPECS['%s/%s/%s%s' % (shape.__name__[2:], frame, p, '/max' if palette is palette_max else '')] = (shape, frame, params, palette)


for _frame in ('narrow', 'wide'):
    for _params in (P_ONE, P_THREE, P_16, P_64, P_FOUR):
        _spec(c_random, _frame, _params)
    _spec(c_random, _frame, P_16, palette_max)
    _spec(c_nothing, _frame, P_THREE)
    for _params in (P_ONE, P_THREE, P_64, P_FOUR):
        _spec(c_align, _frame, _params)
    _spec(c_empty_group, _frame, P_SIX)
    _spec(c_empty_group, _frame, P_MANY)
    for _params in (P_SIX, P_ONE):
        _spec(c_totals, _frame, _params)
    _spec(c_totals16, _frame, P_MANY)
    _spec(c_long, _frame, P_LONG)
    for _shape in (c_hot47, c_hot48_15, c_hot48_16):
        _spec(_shape, _frame, P_16)
    _spec(c_hot48_16, _frame, P_THREE)
    _spec(c_point, _frame, P_FOUR)
    _spec(c_point_corner, _frame, P_ONE)
    _spec(c_point_corner, _frame, P_16, palette_max)
    for _params in (P_ONE, P_THREE, P_16, P_64):
        _spec(c_fill, _frame, _params)
    _spec(c_fill, _frame, P_16, palette_max)
    _spec(c_preload, _frame, P_THREE)
    for _params in (P_ONE, P_THREE, P_SIX):
        _spec(c_chunks, _frame, _params)
for _params in (P_ONE, P_THREE):
    _spec(c_gang, 'ganged', _params)
_spec(c_point_corner, 'ganged', P_THREE)
_spec(c_random, 'ganged', P_THREE)

NAMES = list(SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    shape, frame, params, palette = SPECS[name]
    bd = Builder(name, frame, params, seed=NAMES.index(name) + 1, palette=palette)
    shape(bd)
    return bd.build()


@functools.lru_cache(maxsize=None)
def encoded(name):
    """(log, directory) of a case, garbage in every slot no run owns (seeded by the case)."""
    c = case(name)
    return M.encode_log(c.runs, c.g, np.random.default_rng(1000 + c.seed))


# ---- inputs fl_debug_accum must refuse: (name, (w, h, log, dir, nbatch_total, batch_records, nslots, nparts, wide)) ----------------
def invalid_examples():
    out = []
    for frame in ('narrow', 'wide'):
        name = 'align/%s/%s' % (frame, '-'.join(str(x) for x in P_THREE))
        c, (log, dirw) = case(name), encoded(name)
        g = c.g
        good = (g.w, g.h, log, dirw) + g.args()
        assert M.validate(*good) is None

        def bad(what, **kw):
            a = dict(zip('w h log dir nbatch_total batch_records nslots nparts wide'.split(), good), **kw)
            out.append(('%s/%s' % (what, frame), tuple(a[k] for k in 'w h log dir nbatch_total batch_records nslots nparts wide'.split())))

        for ns in (0, 128, 768, 1000, 16640):
            bad('nslots=%d' % ns, nslots=ns)
        bad('nbatch=0', nbatch_total=0)
        bad('nbatch+1', nbatch_total=g.nbatch + 1)
        bad('nbatch/2', nbatch_total=g.nbatch // 2 + 128)
        bad('records=0', batch_records=0)
        bad('records=16385', batch_records=16385)
        bad('records=250', batch_records=250)
        bad('parts=0', nparts=0)
        bad('parts=65', nparts=65)
        bad('log-1', log=log[:-1])
        bad('log+1', log=np.concatenate([log, log[:1]]))
        bad('log-spare', log=log[:-8])
        bad('dir-1', dir=dirw[:-1])
        bad('dir+tile', dir=np.concatenate([dirw, dirw[:g.nbatch]]))
        bad('layout', wide=1 - g.wide)
        d = dirw.reshape(g.nbins, g.nbatch)
        cnt = d & 0xffff
        t, b = (int(x[0]) for x in np.nonzero((cnt > 0) & (np.arange(g.nbins)[:, None] == g.nbins - 1)))      # a run of the last tile
        e = d.copy(); e[t, b] = ((g.batch_records - 1) << 16) | 2; e[t - 1, b] = (e[t - 1, b] & 0xffff0000)
        bad('past-batch', dir=e.reshape(-1))
        e = d.copy(); e[t, b] += 1 << 16
        bad('gap', dir=e.reshape(-1))
        e = d.copy(); e[t - 1, b], e[t, b] = d[t, b], d[t - 1, b]
        bad('descending', dir=e.reshape(-1))
        e = d.copy(); e[t - 1, b] += 1
        bad('overlap', dir=e.reshape(-1))
        # a record the directory owns, moved out of the accumulator: right of the last tile's columns, below its rows
        first = int(d[t, b] >> 16)
        nx, ny = g.tile_extent(t)
        for what, rec in (('right', g.record(nx, 0, 1)), ('below', g.record(0, ny, 1)), ('corner', g.record(g.tile_w - 1, M.TILE_H - 1, 255))):
            l2 = log.copy()
            if g.wide:
                l2[b * g.region + first] = rec
            else:
                w64 = l2[:g.nbatch * g.region].view(np.uint64)
                sh = np.uint64(M.REC_BITS * (first % 3))
                i = b * g.batch_words + first // 3
                w64[i] = (w64[i] & ~(np.uint64((1 << M.REC_BITS) - 1) << sh)) | (np.uint64(rec) << sh)
            bad('cell-' + what, log=l2)
        if g.wide:
            l2 = log.copy(); l2[b * g.region + first] |= np.uint32(1 << 22)
            bad('high-bits', log=l2)
        # the same garbage in a slot NO run owns is none of the gate's business
        l2 = log.copy(); l2[-8:] = 0xffffffff
        assert M.validate(g.w, g.h, l2, dirw, *g.args()) is None
    # more narrow tiles than a record can name
    out.append(('too-many-narrow-tiles', (7680, 4320, np.zeros(8, np.uint32), np.zeros(8, np.uint32), 256, 256, 256, 1, 0)))
    return out
