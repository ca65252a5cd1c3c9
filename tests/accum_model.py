"""
Integer model of the binned accumulate's input and output (csrc/binned.hip, csrc/launch_plan.h; numpy only, no GPU).

The sample log of a launch holds, per batch, a region of records sorted by image tile, and the directory one word per
(tile, batch): (first record << 16) | count.  Records are (cell << 8) | palette column, the cell being (ly << 7) | lx in a
128x64 tile — 21 bits, three to an aligned 64-bit word (bit 21 j of the word starts slot j, bit 63 is unused), regions of
fl_pack3_words 64-bit words — or (ly << 8) | lx in a 256x64 tile: 22 bits, one record per 32-bit word.  The runs of a batch are
contiguous and ascending by tile; a slot no run owns (the other slots of a word two runs share, the tail of a region, the 8
spare words) holds whatever the writer's LDS held.

`Geometry` restates the host arithmetic (calc_dim, bin_layout, bin_set, launch_accum_tiles) and how the kernel cuts the
batches into parts, palette chunks and groups of 64 directory entries per wave; `encode_log` / `decode_log` are the format,
`accumulate` what the accumulate has to produce, `validate` the twin of the host's gate (accum_log_check), `virtual_arrays`
and `hot_steps` the kernel's walk over a group's runs as far as the hot-cell path depends on it.
"""
import collections

import numpy as np

GUTTER, TILE_H, PAL_W, PAL_H = 12, 64, 256, 64
REC_BITS, MAX_BINS, MAX_BINS_WIDE = 21, 2047, 8191
ROWS_MAX, ROWS_MAX_WIDE, WAVES = 5, 12, 16          # ACC_ROWS_MAX, the wide launch's 12 rows, waves per accumulate workgroup
FIELD = (1 << 18) - 1

Runs = collections.namedtuple('Runs', 'batch tile rec')       # parallel arrays, sorted by (batch, tile); order inside a run kept


def pack3_words(batch_records):
    return ((batch_records + 2) // 3 + 1) & ~1


def nslots_valid(nslots):
    return (nslots >= 1024 or nslots in (512, 256)) and nslots % 256 == 0 and nslots <= 16384


def make_runs(batch, tile, rec):
    batch, tile, rec = (np.asarray(a, np.int64) for a in (batch, tile, rec))
    order = np.lexsort((tile, batch))                       # stable: records of one run keep their order
    return Runs(batch[order], tile[order], rec[order].astype(np.uint32))


class Geometry(object):
    def __init__(self, w, h, wide, nslots, per_slot, batch_records, nparts):
        self.w, self.h, self.wide, self.nslots, self.per_slot = w, h, int(bool(wide)), nslots, per_slot
        self.batch_records, self.nparts = batch_records, nparts
        self.aw, self.ah = w + 2 * GUTTER, 16 * ((h + 2 * GUTTER + 15) // 16)
        self.astride = 32 * ((self.aw + 31) // 32)
        self.ncells = self.ah * self.astride
        self.twl = 8 if self.wide else 7
        self.tile_w = 1 << self.twl
        self.tiles_x = (self.astride + self.tile_w - 1) // self.tile_w
        self.tiles_y = (self.ah + TILE_H - 1) // TILE_H
        self.nbins = self.tiles_x * self.tiles_y
        self.nbatch = nslots * per_slot
        self.batch_words = pack3_words(batch_records)                        # 64-bit words of a packed region
        self.region = batch_records if self.wide else 2 * self.batch_words   # 32-bit words
        self.log_words, self.dir_words = self.nbatch * self.region + 8, self.nbins * self.nbatch
        # launch_accum_tiles
        self.big_thr = 1024 // nparts
        self.spr = nslots // PAL_H
        want = ((nslots + nparts - 1) // nparts + self.spr - 1) // self.spr + 1
        self.rows_cap = min(max(want, 2), ROWS_MAX_WIDE if self.wide else ROWS_MAX)
        self.chunk_slots = (self.rows_cap - 1) * self.spr
        self.gang = 32 if self.nbins > 512 else 0

    def args(self):
        """The scalar arguments of fl_debug_accum behind the buffers."""
        return (self.nbatch, self.batch_records, self.nslots, self.nparts, self.wide)

    def tile_origin(self, t):
        return (t % self.tiles_x) * self.tile_w, (t // self.tiles_x) * TILE_H

    def tile_extent(self, t):
        """Columns and rows of tile t that lie inside the accumulator."""
        x0, y0 = self.tile_origin(t)
        return min(self.tile_w, self.astride - x0), min(TILE_H, self.ah - y0)

    def record(self, lx, ly, ci):
        return ((np.asarray(ly, np.int64) << self.twl | lx) << 8 | ci).astype(np.uint32)

    def cell_of(self, tile, rec):
        """Accumulator index of every record, and whether it lies inside the accumulator."""
        tile, off = np.asarray(tile, np.int64), np.asarray(rec, np.int64) >> 8
        px = (tile % self.tiles_x) * self.tile_w + (off & (self.tile_w - 1))
        py = (tile // self.tiles_x) * TILE_H + (off >> self.twl)
        return py * self.astride + px, (px < self.astride) & (py < self.ah)

    def row_of(self, batch):
        return (np.asarray(batch, np.int64) // self.per_slot) * PAL_H // self.nslots

    def parts(self):
        return [(self.nbatch * p // self.nparts, self.nbatch * (p + 1) // self.nparts) for p in range(self.nparts)]

    def part_of(self, batch):
        """The part whose batch range holds each batch."""
        lo = np.array([b for b, _ in self.parts()], np.int64)
        return np.searchsorted(lo, np.asarray(batch, np.int64), side='right') - 1

    def chunks(self, part):
        """(first batch, end, first staged palette row, staged rows) of the part's palette chunks."""
        b_lo, b_hi = self.parts()[part]
        out, cb = [], b_lo
        while cb < b_hi:
            cs_lo = cb // self.per_slot
            ce = min(b_hi, (cs_lo + self.chunk_slots) * self.per_slot)
            row_lo = cs_lo // self.spr
            out.append((cb, ce, row_lo, min(self.rows_cap, PAL_H - row_lo)))
            cb = ce
        return out

    def groups(self, part):
        """(wave, first batch, end) of every group of up to 64 directory entries, in the order a wave meets them."""
        out = []
        for cb, ce, _, _ in self.chunks(part):
            for wave in range(WAVES):
                for g0 in range(cb + wave * 64, ce, WAVES * 64):
                    out.append((wave, g0, min(g0 + 64, ce)))
        return out


def _positions(runs, g):
    """Index of every record within its batch (the runs are sorted by batch and tile)."""
    n = len(runs.batch)
    start = np.zeros(g.nbatch + 1, np.int64)
    np.cumsum(np.bincount(runs.batch, minlength=g.nbatch), out=start[1:])
    return np.arange(n, dtype=np.int64) - start[runs.batch]


def encode_log(runs, g, rng):
    """Log and directory words (uint32) of `runs`; every slot no run owns is random bits."""
    counts = np.bincount(runs.tile * g.nbatch + runs.batch, minlength=g.dir_words).reshape(g.nbins, g.nbatch)
    assert counts.sum(0).max(initial=0) <= g.batch_records, 'a batch holds more records than batch_records'
    first = np.cumsum(counts, 0) - counts
    dirw = ((first << 16) | counts).astype(np.uint32).reshape(-1)
    log = rng.integers(0, 1 << 32, g.log_words, dtype=np.uint32)
    pos = _positions(runs, g)
    if g.wide:
        log[runs.batch * g.region + pos] = runs.rec
    else:
        w64 = log[:g.nbatch * g.region].view(np.uint64)
        word, slot = runs.batch * g.batch_words + pos // 3, pos % 3
        for s in range(3):                                  # a word's three slots in three passes: no index twice in one
            m = slot == s
            sh = np.uint64(REC_BITS * s)
            keep = ~(np.uint64((1 << REC_BITS) - 1) << sh)
            w64[word[m]] = (w64[word[m]] & keep) | (runs.rec[m].astype(np.uint64) << sh)
    return log, dirw


def decode_log(log, dirw, g):
    """The runs a directory names, read from the log; nothing but the directory decides which slots are read."""
    d = np.asarray(dirw, np.uint32).reshape(g.nbins, g.nbatch).T.astype(np.int64)          # [batch][tile]
    cnt, first = (d & 0xffff).reshape(-1), (d >> 16).reshape(-1)
    n = int(cnt.sum())
    run = np.repeat(np.arange(cnt.size, dtype=np.int64), cnt)
    start = np.cumsum(cnt) - cnt
    pos = first[run] + np.arange(n, dtype=np.int64) - start[run]
    batch, tile = run // g.nbins, run % g.nbins
    log = np.asarray(log, np.uint32)
    if g.wide:
        rec = log[batch * g.region + pos]
    else:
        w64 = log[:g.nbatch * g.region].view(np.uint64)
        rec = ((w64[batch * g.batch_words + pos // 3] >> (REC_BITS * (pos % 3)).astype(np.uint64)) & np.uint64((1 << REC_BITS) - 1))
    return Runs(batch, tile, rec.astype(np.uint32))


def unpack_cells(cells):
    """count, y, u, v (int64) of packed 64-bit cells or palette entries."""
    c = np.asarray(cells, np.uint64)
    f = np.uint64(FIELD)
    return tuple(a.astype(np.int64) for a in (c >> np.uint64(54), (c >> np.uint64(36)) & f, (c >> np.uint64(18)) & f, c & f))


def pack_cells(n, y, u, v):
    n, y, u, v = (np.asarray(a, np.int64).astype(np.uint64) for a in (n, y, u, v))
    return (n << np.uint64(54)) | (y << np.uint64(36)) | (u << np.uint64(18)) | v


def accumulate(runs, g, palette, preload=None):
    """Per cell: hits and the integer sums of the three palette fields, [4][ncells] int64 (count, y, u, v).  `preload`: packed
    cells already in the accumulator."""
    palette = np.asarray(palette, np.uint64).reshape(PAL_H, PAL_W)
    gi, inside = g.cell_of(runs.tile, runs.rec)
    assert inside.all()
    pc, py, pu, pv = unpack_cells(palette[g.row_of(runs.batch), runs.rec & 255])
    assert (pc == 1).all(), 'a palette entry counts one hit'
    out = np.zeros((4, g.ncells), np.int64)
    for k, f in enumerate((pc, py, pu, pv)):                # (float64 weights: exact below 2^53)
        out[k] = np.bincount(gi, weights=f.astype(np.float64), minlength=g.ncells).astype(np.int64)
    if preload is not None:
        out += np.stack(unpack_cells(preload))
    return out


def part_hits(runs, g):
    """(part, cell, hits) of every cell a part's workgroup adds to."""
    gi, _ = g.cell_of(runs.tile, runs.rec)
    key, hits = np.unique(g.part_of(runs.batch) * g.ncells + gi, return_counts=True)
    return key // g.ncells, key % g.ncells, hits


def float_adds_bound(runs, g):
    """Per cell, an upper bound of the float adds the accumulate and the flush make into one colour channel (see
    tests/test_gpu_accum_log.py): per part that touches the cell max(hits // 16, hits - 256, 0) spills of hot groups and LDS
    drains and two at the tile add; one for the flush."""
    part, cell, hits = part_hits(runs, g)
    k = np.ones(g.ncells, np.int64)
    np.add.at(k, cell, np.maximum(np.maximum(hits // 16, hits - 256), 0) + 2)
    return k


def validate(w, h, log, dirw, nbatch_total, batch_records, nslots, nparts, wide):
    """None if fl_debug_accum may launch this, else the reason (the twin of accum_log_check, csrc/launch_plan.h)."""
    if not (1 <= w <= 32768 and 1 <= h <= 32768):
        return 'image size out of range'
    if not nslots_valid(nslots):
        return 'nslots'
    if nbatch_total <= 0 or nbatch_total % nslots:
        return 'nbatch_total'
    if nbatch_total // nslots > 16384:
        return 'batches per slot'
    if not 1 <= batch_records <= 16384:
        return 'batch_records'
    if not 1 <= nparts <= 64:
        return 'nparts'
    g = Geometry(w, h, wide, nslots, nbatch_total // nslots, batch_records, nparts)
    if not g.wide and (g.astride + 127) // 128 * g.tiles_y > MAX_BINS:
        return 'needs wide tiles'
    if g.nbins > MAX_BINS_WIDE:
        return 'too many tiles'
    if not g.wide and g.batch_words + 4 < 64:
        return 'regions shorter than 60 words'
    if len(log) != g.log_words or len(dirw) != g.dir_words:
        return 'sizes'
    d = np.asarray(dirw, np.uint32).reshape(g.nbins, g.nbatch).astype(np.int64)
    cnt, first = d & 0xffff, d >> 16
    if (first[1:] != first[:-1] + cnt[:-1]).any():
        return 'not contiguous'
    if (first + cnt > batch_records).any():
        return 'run ends outside its batch'
    runs = decode_log(log, dirw, g)
    if g.wide and (runs.rec >> 22).any():
        return 'bits above the cell'
    if not g.cell_of(runs.tile, runs.rec)[1].all():
        return 'cell outside the accumulator'
    return None


def run_words(dirw, g):
    """[tile][batch] log words of every run as the kernel counts them: 64-bit words (128x64 tiles) or records (256x64)."""
    d = np.asarray(dirw, np.uint32).reshape(g.nbins, g.nbatch).astype(np.int64)
    cnt, first = d & 0xffff, d >> 16
    if g.wide:
        return cnt
    return np.where(cnt > 0, (first + cnt - 1) // 3 - first // 3 + 1, 0)


def group_totals(dirw, g):
    """(part, wave, first batch, end, totals[tile]) of every group of every part."""
    words = run_words(dirw, g)
    return [(p, wave, g0, ge, words[:, g0:ge].sum(1)) for p in range(g.nparts) for wave, g0, ge in g.groups(p)]


def virtual_arrays(log, dirw, g):
    """The kernel's view of every non-empty (tile, group): the group's runs as one array.  Yields (part, tile, g0, batch[],
    cells[n][S], live[n][S], raw) with S = 3 slots per 64-bit word (128x64 tiles; `live` = the slots the word's run owns) or
    S = 1 record; raw(k) = the cells of the word a lane past the array's end reads."""
    d = np.asarray(dirw, np.uint32).reshape(g.nbins, g.nbatch).astype(np.int64)
    cnt, first = d & 0xffff, d >> 16
    log = np.asarray(log, np.uint32)
    w64 = None if g.wide else log[:g.nbatch * g.region].view(np.uint64)
    words = run_words(dirw, g)
    for p, wave, g0, ge, tot in group_totals(dirw, g):
        for t in np.nonzero(tot)[0]:
            b = np.arange(g0, ge)
            c = words[t, g0:ge]
            run = np.repeat(np.arange(ge - g0), c)
            k = np.arange(int(c.sum())) - (np.cumsum(c) - c)[run]                 # word / record within its run
            rf, rc = first[t, g0:ge][run], cnt[t, g0:ge][run]
            if g.wide:
                rec = log[b[run] * g.region + rf + k].astype(np.int64)
                cells, live, raw = (rec >> 8)[:, None], np.ones((len(rec), 1), bool), None     # (such lanes are never live here)
            else:
                wi = rf // 3 + k
                wv = w64[b[run] * g.batch_words + wi]
                cells = np.stack([((wv >> np.uint64(REC_BITS * s + 8)) & np.uint64(0x1fff)).astype(np.int64) for s in range(3)], 1)
                slot = wi[:, None] * 3 + np.arange(3)[None, :]
                live = (slot >= rf[:, None]) & (slot < (rf + rc)[:, None])

                def raw(lanes, g0=g0):
                    wv = w64[g0 * g.batch_words + lanes]
                    return np.stack([((wv >> np.uint64(REC_BITS * s + 8)) & np.uint64(0x1fff)).astype(np.int64) for s in range(3)], 1)
            yield p, int(t), g0, b[run], cells, live, raw


def hot_steps(log, dirw, g):
    """Every step of the record loop as the hot-cell test sees it: (part, tile, g0, step, trigger, groups).  `trigger`: lanes of
    the step's first 64 records (128x64 tiles: the first slots of its 64 words, whoever owns them, lanes past the end included)
    that share lane 0's cell — from 48 on the step is examined; `groups`: per record set (slot; 256x64 tiles: the four sets of 64
    records of a step), the live records that share the cell of the set's first lane — from 16 on an examined step sends them
    to the float accumulator in one piece."""
    out = []
    for p, t, g0, _, cells, live, raw in virtual_arrays(log, dirw, g):
        n = len(cells)
        if g.wide:
            for s in range(0, n, 256):
                sets = []
                for k in range(4):
                    c = cells[s + 64 * k:s + 64 * k + 64, 0]        # (a set past the end has no live record)
                    sets.append(int((c == c[0]).sum()) if len(c) else 0)
                out.append((p, t, g0, s // 256, sets[0], sets))
        else:
            for s in range(0, n, 64):
                c, lv = cells[s:s + 64], live[s:s + 64]
                if len(c) < 64:                             # lanes past the end read the words behind the group's first
                    lanes = np.arange(len(c), 64)
                    c = np.concatenate([c, raw(lanes)])
                    lv = np.concatenate([lv, np.zeros((len(lanes), 3), bool)])
                trigger = int((c[:, 0] == c[0, 0]).sum())
                sets = []
                for j in range(3):
                    liv = np.nonzero(lv[:, j])[0]
                    sets.append(int((c[liv, j] == c[liv[0], j]).sum()) if len(liv) else 0)
                out.append((p, t, g0, s // 64, trigger, sets))
    return out


def takes_hot_path(steps):
    """Does any step send a group to the float accumulator?"""
    return any(trigger >= 48 and max(sets) >= 16 for _, _, _, _, trigger, sets in steps)


def is_plain(runs, log, dirw, g, preload=None):
    """True if the launch leaves the float accumulator alone: nothing preloaded, no workgroup gives a cell min(256, big_thr)
    hits (the LDS tile's early drain; the tile add's direct spill), no cell collects 512 from all of them (the tile add's drain
    of a full packed cell), no step takes the hot-cell path.  The packed cells then hold the model's integers bit for bit."""
    _, cell, hits = part_hits(runs, g)
    total = np.bincount(cell, weights=hits).max(initial=0)
    return (preload is None and hits.max(initial=0) < min(256, g.big_thr) and total < 512
            and not takes_hot_path(hot_steps(log, dirw, g)))
