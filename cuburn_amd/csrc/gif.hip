// gif.hip — one GIF frame block (image descriptor, a local colour table of its own, LZW data in sub-blocks) from u8 [h][w][4] on
// the device.  DESIGN.md §4.15; the format is fixed in include/flame_hip.h.
// Eight launches per frame, no host wait between them:
//   k_gif_clear     the histogram of 32768 cells {count, sum r, sum g, sum b} to zero
//   k_gif_hist      a wave reads 64 pixels a step, joins the lanes of equal cell and keeps the cell it meets in all 64 lanes in
//                   registers: a flat background costs four atomics a wave, not four a pixel
//   k_gif_cut       one workgroup of 1024: the non-empty cells compacted (cell | box in LDS, counts in the scratch), then the median
//                   cut by population, two passes over the list per split; the palette
//   k_gif_lut       the inverse colour map: every cell's nearest palette entry
//   k_gif_map       four pixels a thread: ordered dither, the cell's entry, one word of indices
//   k_gif_lzw       one wave per workgroup, LANES of its lanes each code one segment with a hash table of its own in LDS
//   k_gif_scan      one workgroup: where every segment's bytes go; the record, the descriptor, the palette, the terminator
//   k_gif_gather    one workgroup per segment: its bytes with the sub-blocks' length bytes between them, stored with store_bytes
// Nothing is stored at or beyond `cap`: when the block does not fit, the scan stores the record alone and the gather nothing.
#include "kernels.h"
#include "encode_device.h"
#include <algorithm>
#include <cstdlib>

namespace {

constexpr uint32_t kCells = 32768u;
constexpr uint32_t kHead = FL_GIF_HEADER_BYTES;               // 2C, the descriptor, the table, 08

__device__ __forceinline__ uint32_t cell_of(uint32_t r, uint32_t g, uint32_t b) { return (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3); }

__global__ void __launch_bounds__(256) k_gif_clear(uint4 *__restrict__ hist)
{
    hist[blockIdx.x * 256u + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- histogram -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void hist_add(uint32_t *hist, uint32_t cell, uint32_t n, uint32_t r, uint32_t g, uint32_t b)
{
    uint32_t *h = hist + 4u * cell;
    atomicAdd(h, n); atomicAdd(h + 1, r); atomicAdd(h + 2, g); atomicAdd(h + 3, b);
}

// The lanes of one cell are summed in one 64-bit word: count (at most 64) in bits 0..6, the sums (at most 64 * 255) in 14 bits each.
__global__ void __launch_bounds__(256)
k_gif_hist(const uint32_t *__restrict__ src, uint32_t npix, uint32_t *__restrict__ hist)
{
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    constexpr uint32_t kNone = 0xffffffffu;
    uint32_t akey = kNone, an = 0, ar = 0, ag = 0, ab = 0;    // the cell this wave keeps in registers (the same in every lane)
    for (uint32_t base = wave * 64u; base < npix; base += nwaves * 64u) {
        const bool valid = base + lane < npix;
        const uint32_t px = valid ? src[base + lane] : 0u;
        const uint32_t r = px & 255u, g = px >> 8 & 255u, b = px >> 16 & 255u;
        const uint32_t key = valid ? cell_of(r, g, b) : kNone;
        u64 todo = __ballot(valid);
        while (todo) {
            const uint32_t lead = (uint32_t)__builtin_ctzll(todo);
            const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)lead);
            const bool in = key == k;
            const u64 m = __ballot(in);
            u64 v = in ? 1ull | (u64)r << 7 | (u64)g << 21 | (u64)b << 35 : 0ull;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
            const uint32_t n = (uint32_t)v & 127u, sr = (uint32_t)(v >> 7) & 16383u, sg = (uint32_t)(v >> 21) & 16383u, sb = (uint32_t)(v >> 35) & 16383u;
            if (k == akey) { an += n; ar += sr; ag += sg; ab += sb; }
            else if (akey == kNone || m == ~0ull) {           // a cell that fills the wave takes the registers
                if (akey != kNone && lane == 0) hist_add(hist, akey, an, ar, ag, ab);
                akey = k; an = n; ar = sr; ag = sg; ab = sb;
            } else if (lane == lead) hist_add(hist, k, n, sr, sg, sb);
            todo &= ~m;
        }
    }
    if (akey != kNone && lane == 0) hist_add(hist, akey, an, ar, ag, ab);
}

// ---- median cut ----------------------------------------------------------------------------------------------------
// Dynamic LDS: kCells words, entry i of the compacted list = cell | box << 16.  ccnt[i] = the entry's pixels.
// pal[0..255] = r | g << 8 | b << 16 (entries from nb on are 0), pal[256] = nb.
__global__ void __launch_bounds__(1024)
k_gif_cut(const uint4 *__restrict__ hist, uint32_t *__restrict__ ccnt, uint32_t *__restrict__ pal, uint32_t colors)
{
    extern __shared__ uint32_t s_ent[];
    __shared__ u64 s_sum[1024];
    __shared__ uint32_t s_pop[256], s_nc[256], s_lo[3][256], s_hi[3][256], s_acc[256][4], s_bin[32];
    __shared__ u64 s_best[4];
    const uint32_t t = threadIdx.x;
    const auto coord = [](uint32_t e, uint32_t ax) -> uint32_t { return e >> (10u - 5u * ax) & 31u; };
    const auto tally = [&](uint32_t box, uint32_t e, uint32_t cnt) {
        atomicAdd(&s_pop[box], cnt); atomicAdd(&s_nc[box], 1u);
#pragma unroll
        for (uint32_t a = 0; a < 3; ++a) { atomicMin(&s_lo[a][box], coord(e, a)); atomicMax(&s_hi[a][box], coord(e, a)); }
    };

    uint32_t mine = 0;                                        // thread t brings cells 32 t .. 32 t + 31
    for (uint32_t k = 0; k < 32u; ++k) mine += hist[32u * t + k].x ? 1u : 0u;
    u64 total;
    uint32_t at = (uint32_t)block_excl_scan_1024(s_sum, mine, t, total);
    const uint32_t n = (uint32_t)total;
    for (uint32_t k = 0; k < 32u; ++k) {
        const uint32_t cnt = hist[32u * t + k].x;
        if (cnt) { s_ent[at] = 32u * t + k; ccnt[at] = cnt; ++at; }
    }
    if (t < 256u) {
        s_pop[t] = 0; s_nc[t] = 0;
        for (uint32_t a = 0; a < 3; ++a) { s_lo[a][t] = 31u; s_hi[a][t] = 0u; }
        for (uint32_t a = 0; a < 4; ++a) s_acc[t][a] = 0;
    }
    __threadfence_block();
    __syncthreads();
    for (uint32_t i = t; i < n; i += 1024u) tally(0u, s_ent[i], ccnt[i]);
    __syncthreads();

    uint32_t nb = 1;
    while (nb < colors) {
        if (t < 256u) {                                       // the box of most pixels among those that can be split, the lowest on a tie
            u64 key = t < nb && s_nc[t] > 1u ? (u64)s_pop[t] << 8 | (255u - t) : 0ull;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) { const u64 o = __shfl_xor(key, d, 64); key = o > key ? o : key; }
            if ((t & 63u) == 0) s_best[t >> 6] = key;
        }
        __syncthreads();
        u64 best = s_best[0];
        for (uint32_t k = 1; k < 4; ++k) best = s_best[k] > best ? s_best[k] : best;
        if (!best) break;
        const uint32_t sel = 255u - ((uint32_t)best & 255u), pop = (uint32_t)(best >> 8);
        const uint32_t er = s_hi[0][sel] - s_lo[0][sel], eg = s_hi[1][sel] - s_lo[1][sel], eb = s_hi[2][sel] - s_lo[2][sel];
        const uint32_t ax = er >= eg && er >= eb ? 0u : eg >= eb ? 1u : 2u;
        const uint32_t lo = s_lo[ax][sel], hi = s_hi[ax][sel];
        if (t < 32u) s_bin[t] = 0;
        __syncthreads();
        for (uint32_t i = t; i < n; i += 1024u) {
            const uint32_t e = s_ent[i];
            if (e >> 16 == sel) atomicAdd(&s_bin[coord(e, ax)], ccnt[i]);
        }
        __syncthreads();
        uint32_t c = 31u, cum = 0;
        for (uint32_t k = 0; k < 32u; ++k) { cum += s_bin[k]; if (2u * cum >= pop) { c = k; break; } }
        c = min(max(c, lo), hi - 1u);
        if (t == 0) {
            s_pop[sel] = 0; s_nc[sel] = 0; s_pop[nb] = 0; s_nc[nb] = 0;
            for (uint32_t a = 0; a < 3; ++a) { s_lo[a][sel] = 31u; s_hi[a][sel] = 0u; s_lo[a][nb] = 31u; s_hi[a][nb] = 0u; }
        }
        __syncthreads();
        for (uint32_t i = t; i < n; i += 1024u) {
            const uint32_t e = s_ent[i];
            if (e >> 16 != sel) continue;
            const bool up = coord(e, ax) > c;
            if (up) s_ent[i] = (e & 0xffffu) | nb << 16;
            tally(up ? nb : sel, e, ccnt[i]);
        }
        ++nb;
        __syncthreads();
    }

    for (uint32_t i = t; i < n; i += 1024u) {
        const uint32_t e = s_ent[i];
        const uint4 hc = hist[e & 0xffffu];
        uint32_t *acc = s_acc[e >> 16];
        atomicAdd(acc, hc.x); atomicAdd(acc + 1, hc.y); atomicAdd(acc + 2, hc.z); atomicAdd(acc + 3, hc.w);
    }
    __syncthreads();
    if (t < 256u) {
        uint32_t v = 0;
        if (t < nb) {
            const uint32_t cnt = s_acc[t][0];
            for (uint32_t a = 0; a < 3; ++a) v |= ((s_acc[t][1u + a] + cnt / 2u) / cnt) << (8u * a);
        }
        pal[t] = v;
    }
    if (t == 0) pal[256] = nb;
}

// ---- inverse colour map --------------------------------------------------------------------------------------------
// Four cells a thread: the entry among 0 .. nb - 1 nearest to the cell's rounded mean (its centre where it is empty), the lowest on a tie.
__global__ void __launch_bounds__(256)
k_gif_lut(const uint4 *__restrict__ hist, const uint32_t *__restrict__ pal, uint32_t *__restrict__ lut)
{
    __shared__ uint32_t s_pal[256];
    const uint32_t t = threadIdx.x, nb = pal[256];
    s_pal[t] = pal[t];
    __syncthreads();
    uint32_t word = 0;
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t cell = 4u * (blockIdx.x * 256u + t) + k;
        const uint4 hc = hist[cell];
        int pr, pg, pb;
        if (hc.x) { pr = (int)((hc.y + hc.x / 2u) / hc.x); pg = (int)((hc.z + hc.x / 2u) / hc.x); pb = (int)((hc.w + hc.x / 2u) / hc.x); }
        else { pr = (int)(8u * (cell >> 10) + 4u); pg = (int)(8u * (cell >> 5 & 31u) + 4u); pb = (int)(8u * (cell & 31u) + 4u); }
        uint32_t bi = 0, bd = 0xffffffffu;
        for (uint32_t i = 0; i < nb; ++i) {
            const uint32_t p = s_pal[i];
            const int dr = pr - (int)(p & 255u), dg = pg - (int)(p >> 8 & 255u), db = pb - (int)(p >> 16 & 255u);
            const uint32_t d = (uint32_t)(dr * dr + dg * dg + db * db);
            if (d < bd) { bd = d; bi = i; }
        }
        word |= bi << (8u * k);
    }
    lut[blockIdx.x * 256u + t] = word;
}

// ---- indices -------------------------------------------------------------------------------------------------------
__constant__ unsigned char c_bayer[64] = {0, 32, 8, 40, 2, 34, 10, 42, 48, 16, 56, 24, 50, 18, 58, 26, 12, 44, 4, 36, 14, 46, 6, 38, 60, 28, 52, 20, 62, 30, 54, 22,
                                          3, 35, 11, 43, 1, 33, 9, 41, 51, 19, 59, 27, 49, 17, 57, 25, 15, 47, 7, 39, 13, 45, 5, 37, 63, 31, 55, 23, 61, 29, 53, 21};

__global__ void __launch_bounds__(256)
k_gif_map(const uint32_t *__restrict__ src, uint32_t w, uint32_t npix, int amp, const unsigned char *__restrict__ lut, uint32_t *__restrict__ idx)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (4u * i >= npix) return;
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint32_t p = 4u * i + k;
        if (p >= npix) break;
        const uint32_t px = src[p], y = p / w, x = p - y * w;
        const int d = 2 * (int)c_bayer[(y & 7u) * 8u + (x & 7u)] + 1 - 64, delta = (d * amp) >> 7;
        const uint32_t r = (uint32_t)min(max((int)(px & 255u) + delta, 0), 255), g = (uint32_t)min(max((int)(px >> 8 & 255u) + delta, 0), 255),
                       b = (uint32_t)min(max((int)(px >> 16 & 255u) + delta, 0), 255);
        word |= (uint32_t)lut[cell_of(r, g, b)] << (8u * k);
    }
    idx[i] = word;
}

// ---- LZW -----------------------------------------------------------------------------------------------------------
// One wave; lane l < lanes codes segment blockIdx.x * lanes + l.  Dynamic LDS: lanes tables of `slots` words (a power of two, at least
// 2 S: a slot is key << 12 | code with key = prefix << 8 | byte, 0 when free; a segment adds at most S strings), then lanes rows of
// spad bytes, the segments' indices.  The codes go to segbuf + seg * stride (word aligned), least significant bit first; lens[seg] =
// their bytes.  A segment holds at most 9 + 12 S + 12 + 63 bits, and stride is that in bytes, rounded up to a word.
__global__ void __launch_bounds__(64)
k_gif_lzw(const unsigned char *__restrict__ idx, uint32_t npix, uint32_t S, uint32_t nseg, uint32_t lanes, uint32_t slots_log2, uint32_t spad,
          unsigned char *__restrict__ segbuf, uint32_t stride, uint32_t *__restrict__ lens)
{
    extern __shared__ uint32_t s_mem[];
    const uint32_t lane = threadIdx.x, slots = 1u << slots_log2, mask = slots - 1u;
    unsigned char *s_pix = (unsigned char *)(s_mem + lanes * slots);
    for (uint32_t i = lane; i < lanes * slots; i += 64u) s_mem[i] = 0;
    const uint32_t seg0 = blockIdx.x * lanes, first = seg0 * S, count = min(npix - first, lanes * S);
    for (uint32_t i = lane; i < count; i += 64u) { const uint32_t r = i / S; s_pix[r * spad + (i - r * S)] = idx[first + i]; }
    __syncthreads();
    const uint32_t seg = seg0 + lane;
    if (lane >= lanes || seg >= nseg) return;
    uint32_t *T = s_mem + lane * slots;
    const unsigned char *pix = s_pix + lane * spad;
    const uint32_t n = min(S, npix - seg * S);
    uint32_t *o = (uint32_t *)(segbuf + (size_t)seg * stride);
    u64 acc = 0;
    uint32_t nbits = 0, nw = 0;
    const auto emit = [&](uint32_t code, uint32_t wd) {
        acc |= (u64)code << nbits;
        nbits += wd;
        if (nbits >= 32u) { o[nw++] = (uint32_t)acc; acc >>= 32; nbits -= 32u; }
    };
    uint32_t width = 9u, next = 258u;
    emit(256u, 9u);
    uint32_t p = pix[0];
    for (uint32_t i = 1; i < n; ++i) {
        const uint32_t c = pix[i], key = p << 8 | c;
        uint32_t h = (key * 2654435761u) >> (32u - slots_log2), e;
        while ((e = T[h]) != 0u && e >> 12 != key) h = (h + 1u) & mask;
        if (e) { p = e & 0xfffu; continue; }
        emit(p, width);
        T[h] = key << 12 | next;
        ++next;
        if (next > 1u << width && width < 12u) ++width;
        p = c;
    }
    emit(p, width);
    ++next;                                                   // the string the decoder adds: it cannot know that the segment ends
    if (next > 1u << width && width < 12u) ++width;
    if (seg + 1u == nseg) {
        emit(257u, width);
        if (nbits & 7u) emit(0u, 8u - (nbits & 7u));
    } else {
        emit(256u, width);
        while (nbits & 7u) emit(256u, 9u);
    }
    if (nbits) o[nw] = (uint32_t)acc;
    lens[seg] = 4u * nw + nbits / 8u;
}

// ---- placement -----------------------------------------------------------------------------------------------------
// offs[i] = where segment i's bytes start in the data stream; info's own word is the stream's bytes.  The record, the descriptor,
// the table, the code size and the block terminator go to `out` (cap >= 16 + kHead: the callers checked).
__global__ void __launch_bounds__(1024)
k_gif_scan(const uint32_t *__restrict__ lens, uint32_t nseg, uint32_t S, uint32_t w, uint32_t h, const uint32_t *__restrict__ pal,
           uint32_t *__restrict__ offs, uint32_t *__restrict__ info, unsigned char *__restrict__ out, u64 cap)
{
    __shared__ u64 s_sum[1024];
    const uint32_t t = threadIdx.x;
    const auto len = [&](uint32_t i) { return lens[i]; };
    const Placement p = place_pieces(s_sum, nseg, t, 0ull, len);
    const u64 total = p.total, need = kHead + total + (total + 254u) / 255u + 1u;
    if (finish_placement(info, out, need, cap, S, (uint32_t)total, t)) return;      // a block that does not fit leaves nothing behind the record
    store_offsets(offs, p, len);
    unsigned char *blk = out + 16u;
    if (t < 10u) {
        const unsigned char d[10] = {0x2c, 0, 0, 0, 0, (unsigned char)w, (unsigned char)(w >> 8), (unsigned char)h, (unsigned char)(h >> 8), 0x87};
        blk[t] = d[t];
    }
    if (t < 768u) blk[10u + t] = (unsigned char)(pal[t / 3u] >> (8u * (t % 3u)));
    if (t == 768u) blk[kHead - 1u] = 8u;
    if (t == 769u) blk[need - 1u] = 0u;
}

// Stream byte j lies at q = j + j / 255 + 1 behind the code size; q = 256 g is the length byte of sub-block g.  A segment stores from
// its first byte (from the length byte in front of it where it begins a sub-block) to its last, the length bytes between them included.
// Dynamic LDS: stride + stride / 255 + 2 bytes in words, and 2 words of padding.
__global__ void __launch_bounds__(256)
k_gif_gather(const unsigned char *__restrict__ segbuf, uint32_t stride, const uint32_t *__restrict__ lens, const uint32_t *__restrict__ offs,
             const uint32_t *__restrict__ info, unsigned char *__restrict__ out)
{
    extern __shared__ uint32_t s_mem[];
    unsigned char *s_bytes = (unsigned char *)s_mem;
    const uint32_t t = threadIdx.x, seg = blockIdx.x;
    if (info[kInfoStatus]) return;
    const uint32_t o = offs[seg], L = lens[seg], total = info[kInfoExtra], last = o + L - 1u;
    const uint32_t q0 = o + o / 255u + (o % 255u ? 1u : 0u), q1 = last + last / 255u + 1u, n = q1 - q0 + 1u;
    const unsigned char *from = segbuf + (size_t)seg * stride;
    for (uint32_t i = t; i < n; i += 256u) {
        const uint32_t q = q0 + i, g = q >> 8;
        s_bytes[i] = (q & 255u) ? from[q - g - 1u - o] : (unsigned char)min(255u, total - 255u * g);
    }
    __syncthreads();
    store_bytes<256>(out + 16u + kHead + q0, s_mem, n, t);
}

} // namespace

uint32_t gif_segment_pixels()
{
    uint32_t v = FL_GIF_SEG;
    if (const char *e = getenv("FLAME_GIF_SEG")) { const long x = atol(e); if (x >= 256 && x <= 3584) v = (uint32_t)x; }
    return v;
}

GifLayout gif_layout(uint32_t w, uint32_t h, uint32_t seg)
{
    GifLayout l;
    l.npix = w * h;
    l.seg = seg;
    l.nseg = (l.npix + seg - 1u) / seg;
    l.stride = ((12u * seg + 9u + 12u + 63u + 7u) / 8u + 3u) & ~3u;
    l.slots_log2 = 9u;
    while (1u << l.slots_log2 < 2u * seg) ++l.slots_log2;
    l.lanes = std::max(1u, FL_GIF_LZW_TABLE_BYTES / (4u << l.slots_log2));
    // words: histogram (16-byte cells) | the compacted counts | palette and nb | the cells' entries | indices | coded segments | offsets | lengths | info
    l.hist = 0;
    l.ccnt = l.hist + 4u * (size_t)kCells;
    l.pal = l.ccnt + kCells;
    l.lut = l.pal + 260u;
    l.idx = l.lut + kCells / 4u;
    l.segbuf = l.idx + (l.npix + 3u) / 4u + 1u;
    l.offs = l.segbuf + (size_t)l.nseg * (l.stride / 4u);
    l.lens = l.offs + l.nseg;
    l.info = l.lens + l.nseg;
    l.words = l.info + 4u;
    return l;
}

void launch_gif_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int colors, int amp, uint32_t seg, uint32_t *scratch,
                       unsigned char *out, size_t cap)
{
    const GifLayout l = gif_layout(w, h, seg);
    uint32_t *hist = scratch + l.hist, *ccnt = scratch + l.ccnt, *pal = scratch + l.pal, *lut = scratch + l.lut, *idx = scratch + l.idx;
    uint32_t *offs = scratch + l.offs, *lens = scratch + l.lens, *info = scratch + l.info;
    unsigned char *segbuf = (unsigned char *)(scratch + l.segbuf);
    const uint32_t *pix = (const uint32_t *)src;
    // (k_gif_cut's 128 KiB list lies beside 20 KiB of static LDS: the cap asked for is the list's own size, once per device)
    static unsigned long long cut_lds = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) dev = 63;
    if (!(cut_lds >> dev & 1ull)) {
        hipFuncSetAttribute((const void *)k_gif_cut, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * (int)kCells);
        if (dev != 63) cut_lds |= 1ull << dev;
    }
    hipLaunchKernelGGL(k_gif_clear, dim3(kCells / 256u), dim3(256), 0, st, (uint4 *)hist);
    hipLaunchKernelGGL(k_gif_hist, dim3(std::min(512u, (l.npix + 255u) / 256u)), dim3(256), 0, st, pix, l.npix, hist);
    hipLaunchKernelGGL(k_gif_cut, dim3(1), dim3(1024), 4 * (size_t)kCells, st, (const uint4 *)hist, ccnt, pal, (uint32_t)colors);
    hipLaunchKernelGGL(k_gif_lut, dim3(kCells / 1024u), dim3(256), 0, st, (const uint4 *)hist, (const uint32_t *)pal, lut);
    hipLaunchKernelGGL(k_gif_map, dim3(((l.npix + 3u) / 4u + 255u) / 256u), dim3(256), 0, st, pix, w, l.npix, amp, (const unsigned char *)lut, idx);
    const uint32_t spad = (seg + 3u) & ~3u;
    hipLaunchKernelGGL(k_gif_lzw, dim3((l.nseg + l.lanes - 1u) / l.lanes), dim3(64), (size_t)l.lanes * ((4u << l.slots_log2) + spad), st,
                       (const unsigned char *)idx, l.npix, seg, l.nseg, l.lanes, l.slots_log2, spad, segbuf, l.stride, lens);
    hipLaunchKernelGGL(k_gif_scan, dim3(1), dim3(1024), 0, st, (const uint32_t *)lens, l.nseg, seg, w, h, (const uint32_t *)pal, offs, info, out, (u64)cap);
    hipLaunchKernelGGL(k_gif_gather, dim3(l.nseg), dim3(256), 4 * (size_t)((l.stride + l.stride / 255u + 2u + 3u) / 4u + 2u), st,
                       (const unsigned char *)segbuf, l.stride, (const uint32_t *)lens, (const uint32_t *)offs, (const uint32_t *)info, out);
}
