// launch_plan.h — how a frame's samples are cut into iterate launches, and what a launch needs: the tile geometry of the
// binned accumulate, the size of a sample log + directory set, workgroups per tile and the schedule of rounds per launch.
// Host arithmetic only (no HIP runtime calls): flame_abi.hip acts on it, tests/test_cpu_launch_plan.py checks it without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "flame_device.h"

// cuburn/render.py:79-89: the accumulator is the image plus a gutter, padded to whole 32 x 16 blocks
static inline fl_dim calc_dim(uint32_t w, uint32_t h)
{
    fl_dim d = {w, h, w + 2 * FL_GUTTER, 16 * ((h + 2 * FL_GUTTER + 15) / 16), 0};
    d.astride = 32 * ((d.aw + 31) / 32);
    return d;
}

// Tile geometry of the binned accumulate for one image, and what a batch takes in the sample log.
struct BinLayout {
    bool wide;            // 256x64 tiles with separately staged tile numbers (else 128x64)
    uint32_t tile_w, tiles_x, nbins;
    size_t region;        // 32-bit words of the log per batch
};
static inline BinLayout bin_layout(const fl_dim &d, int nw, uint32_t bin_rounds, bool force_wide)
{
    BinLayout b;
    const uint32_t nt = (uint32_t)nw * 64;
    // 128x64 tiles while their number fits the 11 bits left in a staged record (up to 4K);
    // larger images use 256x64 tiles with separately staged tile numbers
    const uint32_t rows = (d.ah + FL_TILE_H - 1) / FL_TILE_H;
    b.wide = ((d.astride + 127) / 128) * rows > FL_MAX_BINS || force_wide;
    b.tile_w = b.wide ? (1u << FL_TILE_W_WIDE_LOG2) : 128u;
    b.tiles_x = (d.astride + b.tile_w - 1) / b.tile_w;
    b.nbins = b.tiles_x * rows;
    // a region per batch — bin_rounds * nt records, one per word (256x64 tiles) or three per 64-bit word (flame_device.h)
    b.region = !b.wide && FL_LOG_PACK3 ? 2 * (size_t)fl_pack3_words(bin_rounds * nt) : (size_t)bin_rounds * nt;
    return b;
}

// One sample log + directory set for a launch of `write_rounds` write-enabled rounds: every slot writes a batch per bin_rounds rounds.
struct BinSet {
    uint32_t nbatch;                  // batches of the launch, all slots together
    size_t log_words, dir_words;      // 32-bit words
    size_t bytes() const { return 4 * (log_words + dir_words); }
};
static inline BinSet bin_set(const BinLayout &b, uint64_t write_rounds, uint32_t bin_rounds, uint32_t nslots)
{
    BinSet s;
    s.nbatch = (uint32_t)((write_rounds + bin_rounds - 1) / bin_rounds) * nslots;
    s.log_words = (size_t)s.nbatch * b.region + 8;
    s.dir_words = (size_t)b.nbins * s.nbatch;
    return s;
}

// Slot counts a context can be created with: a multiple of 256 from 1024 up, or 512 / 256 slots whose 8- / 16-wave workgroups walk
// two / four temporal samples each
static inline bool nslots_valid(uint32_t nslots)
{
    return (nslots >= FL_NTEMPORAL || nslots == FL_NTEMPORAL / 2 || nslots == FL_NTEMPORAL / 4) && nslots % 256 == 0 && nslots <= 16384;
}

// fl_debug_accum's gate: may the tile accumulate (binned.hip) be launched on this log + directory?  Null if so, else the reason.
// The kernels trust their input — the run lookup, the LDS tile and the spills of full and hot cells take every index as it comes
// (only the tile add tests px < astride, py < aheight) — so everything they rely on is established here, on the host, record by
// record: sizes as bin_set gives them, runs of a batch contiguous and ascending by tile and inside the batch, every record a run
// owns in a cell of the accumulator (256x64 tiles: nothing above the record's 22 bits, which would index past the LDS tile).
// Slots no run owns may hold anything.  `d` and `b` receive the frame and tile geometry the launch is to use.
static inline const char *accum_log_check(uint32_t w, uint32_t h, const uint32_t *log, size_t log_words, const uint32_t *dir, size_t dir_words,
                                          uint32_t nbatch_total, uint32_t batch_records, uint32_t nslots, uint32_t nparts, int wide,
                                          fl_dim *d, BinLayout *b)
{
    if (!log || !dir) return "null log or directory";
    if (!w || !h || w > 32768u || h > 32768u) return "image size out of range";
    if (!nslots_valid(nslots)) return "nslots is not a slot count of fl_ctx_create";
    if (!nbatch_total || nbatch_total % nslots) return "nbatch_total must be a positive multiple of nslots";
    if (nbatch_total / nslots > 16384u) return "more than 16384 batches per slot";
    if (batch_records < 1u || batch_records > 16384u) return "batch_records outside 1..16384";
    if (nparts < 1u || nparts > 64u) return "nparts outside 1..64";
    *d = calc_dim(w, h);
    *b = bin_layout(*d, 1, 1, wide != 0);
    if (b->wide != (wide != 0)) return "more 128x64 tiles than a record can name: the image needs 256x64 tiles";
    if (b->nbins > FL_MAX_BINS_WIDE) return "image too large for the binned accumulate (> 8191 tiles of 256x64)";
    const uint32_t bw = fl_pack3_words(batch_records);
    b->region = !b->wide && FL_LOG_PACK3 ? 2 * (size_t)bw : (size_t)batch_records;
    // (a step of the packed accumulate whose lanes lie past the group's end reads the 64 words that follow the group's first: they
    // must lie inside the log, the 8 spare words included, for a group that starts in the last batch too)
    if (!b->wide && FL_LOG_PACK3 && bw + 4u < 64u) return "packed batch regions shorter than 60 words";
    const BinSet s = bin_set(*b, nbatch_total / nslots, 1, nslots);
    if (s.nbatch != nbatch_total || log_words != s.log_words || dir_words != s.dir_words) return "log or directory size is not what bin_set gives";
    const uint32_t twl = b->wide ? FL_TILE_W_WIDE_LOG2 : 7u;
    for (uint32_t batch = 0; batch < nbatch_total; ++batch) {
        const uint32_t *reg = log + (size_t)batch * b->region;
        uint32_t expect = 0;
        for (uint32_t t = 0; t < b->nbins; ++t) {
            const uint32_t e = dir[(size_t)t * nbatch_total + batch], first = e >> 16, count = e & 0xffffu;
            if (t && first != expect) return "runs of a batch are not contiguous and ascending by tile";
            if (first + count > batch_records) return "a run ends outside its batch";
            expect = first + count;
            const uint32_t x0 = (t % b->tiles_x) << twl, y0 = (t / b->tiles_x) * FL_TILE_H;
            for (uint32_t i = first; i < first + count; ++i) {
                uint32_t rec;
                if (!b->wide && FL_LOG_PACK3) {
                    const uint64_t word = reg[2 * (i / 3u)] | (uint64_t)reg[2 * (i / 3u) + 1u] << 32;
                    rec = (uint32_t)(word >> (FL_REC_BITS * (i % 3u))) & ((1u << FL_REC_BITS) - 1u);
                } else {
                    rec = reg[i];
                    if (rec >> (8u + twl + FL_TILE_H_LOG2)) return "a record has bits above its cell";
                }
                const uint32_t off = rec >> 8, px = x0 + (off & ((1u << twl) - 1u)), py = y0 + (off >> twl);
                if (px >= d->astride || py >= d->ah) return "a record's cell lies outside the accumulator";
            }
        }
    }
    return nullptr;
}

// Workgroups per tile of the accumulate: enough of them to fill the chip several times over (~8192 in all),
// no more — every workgroup zeroes and drains a whole LDS tile whatever its share of records
// (256x64 tiles, one workgroup per CU: twice as many — a dense region then spreads over more
// workgroups; cfg5 8K: 3 per tile 20.7 ms of accumulate per frame, 8 per tile 16.2, 12: 18.2)
// (round 5: with the ganged tile order of images of more than 512 tiles — launch_accum_tiles — six per tile at 4K and 8K:
// 507 / 531 / 619 us per 4K launch with 6 / 8 / 12, 2187 / 2410 / 2677 at 8K; profiles/r05_bin_parts.txt)
// `forced`: FLAME_BIN_PARTS (0: the rule above, at most 16; forced values up to 64).
static inline uint32_t accum_parts(uint32_t nbins, bool wide, uint32_t forced)
{
    if (forced) return std::min(forced, 64u);
    const uint32_t parts = nbins > 512u ? ((wide ? 12800u : 6400u) + nbins / 2u) / nbins : (wide ? 16384u : 8192u) / nbins;
    return std::min(std::max(parts, 1u), 16u);
}

// Maximum write-enabled rounds of one binned launch (bounds the sample log: nslots*NT*4 B per round).  The reference's batches grow
// 1024, 1536, 2304, ... rounds (cuburn/render.py:338-369); here they stop growing at 1024 — equal launches overlap best in the
// lane's two-stream pipeline (cfg3, 2731 rounds: 1024 + 1024 + 683 is 1.7 % faster than 1024 + 1536 + 171) — unless following the
// reference's schedule up to 2304 rounds saves a launch, i.e. a flush and a zeroed + added tile per workgroup (cfg5, 4096 rounds:
// 1024 + 1536 + 1536 instead of 4 x 1024, frame 37.0 -> 36.1 ms; profiles/r05_launch_cap.txt).
// (16-wave workgroups: the long cap stops at the 1536 rounds that tests/test_gpu_parity.py::test_long_launch_log_beyond_4gb... pins —
// a 2304-round launch of the 8K geometry is a 14.5 GB log whose record indices pass 2^31)
// (workgroups in sub-blocks have a half or a quarter of the walkers of their plain geometry: their rounds count double / fourfold
// for the same samples per launch, i.e. the same log, flush schedule and number of launches)
#define FL_BIN_MAX_ROUNDS 1024u
#define FL_BIN_MAX_ROUNDS_LONG 2304u
#define FL_NO_CAP (~0ull)
static inline uint64_t launch_cap(bool longer, uint32_t sub_log2, int nw)
{
    return (uint64_t)(!longer ? FL_BIN_MAX_ROUNDS : nw == 16 ? 1536u : FL_BIN_MAX_ROUNDS_LONG) << sub_log2;
}

// Write-enabled rounds of every launch of a frame of `rounds` rounds: cuburn/render.py:338-369, batches grow 4, 6, 9, 13, ...
// (x 256 rounds, x 2 / 4 in sub-blocks), none longer than `cap` rounds (a fixed cap — FLAME_LAUNCH_ROUNDS — is taken as it is).
struct LaunchPlan { uint64_t cap; std::vector<uint32_t> rounds; };
static inline LaunchPlan launch_schedule_under(uint64_t rounds, uint32_t sub_log2, uint64_t cap)
{
    LaunchPlan plan = {cap, {}};
    const uint64_t unit = 256ull << sub_log2;
    for (uint64_t batch = 4; rounds; batch += batch / 2) {
        const uint64_t n = std::min(std::min(rounds, batch * unit), cap);
        plan.rounds.push_back((uint32_t)n);
        rounds -= n;
    }
    return plan;
}
// The plan of a binned frame: under the fixed cap if there is one (0: none), else under the long cap where that saves a launch
// (fl_iterate falls back to the short one if the longer logs do not fit the device), else under the short cap.
static inline LaunchPlan launch_schedule(uint64_t rounds, uint32_t sub_log2, int nw, uint32_t fixed)
{
    if (fixed) return launch_schedule_under(rounds, sub_log2, fixed);
    LaunchPlan shorter = launch_schedule_under(rounds, sub_log2, launch_cap(false, sub_log2, nw));
    LaunchPlan longer = launch_schedule_under(rounds, sub_log2, launch_cap(true, sub_log2, nw));
    return longer.rounds.size() < shorter.rounds.size() ? longer : shorter;
}
