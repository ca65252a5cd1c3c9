// webp.hip — one lossless WebP frame block (a whole `VP8L` chunk) from u8 [h][w][4] on the device.  DESIGN.md §4.16; the format is
// fixed in include/flame_hip.h.
// Seven launches per frame, no host wait between them:
//   k_webp_modes    one workgroup per 16 x 16 predictor tile, a thread per pixel: the six modes' costs, the cheapest mode
//   k_webp_stats    one workgroup per 64 x 64 entropy tile: four histograms of the residuals, four length-limited codes, the
//                   group's header bits into a staging area, the bit count of each of the tile's row-runs; and one workgroup more:
//                   the fixed header, the mode sub-image and the entropy sub-image into a staging area
//   k_webp_scan     one workgroup: where every group header and every run begins, in bits; the record and the chunk header
//   k_webp_clear    the words of the assembly buffer that the stream will occupy, to zero
//   k_webp_heads    one workgroup per staged piece: its bits OR-ed into the assembly buffer at its bit offset
//   k_webp_emit     a wave per run, a lane per pixel: the pixel's four codes, a scan of their lengths, the run's bits put together
//                   in LDS and stored at the run's bit offset (the two boundary words by atomicOr, the words between them plainly)
//   k_webp_copy     the assembly buffer to the destination with store_bytes
// The prediction is recomputed from the source in modes, stats and emit; no residual picture is stored.
// Nothing is stored at or beyond `cap`: when the block does not fit, the scan stores the record alone.
#include "kernels.h"
#include "encode_device.h"
#include <algorithm>

namespace {

constexpr uint32_t kPB = FL_WEBP_PB, kEB = FL_WEBP_EB, kPT = 1u << kPB, kET = 1u << kEB;
constexpr uint32_t kCodeBits = 76u + 256u * 14u;              // one normal code's header: see fl_webp_bound
constexpr uint32_t kGroupBits = 4u * kCodeBits + 4u;
constexpr uint32_t kCodeWords = (kCodeBits + 31u) / 32u + 1u;
constexpr uint32_t kHdrWords = (kGroupBits + 31u) / 32u + 2u; // a group's staged header
constexpr uint32_t kBlack = 0xff000000u;                      // what (0, 0) is predicted from: r, g, b = 0, a = 255

// ---- the predictor -------------------------------------------------------------------------------------------------
// A pixel is r - g | g << 8 | b - g << 16 | a << 24, green already subtracted; alpha reads 255 with three channels.
__device__ __forceinline__ uint32_t load_px(const uint32_t *__restrict__ src, size_t i, bool alpha)
{
    const uint32_t p = src[i], g = p >> 8 & 255u;
    return ((p - g) & 255u) | g << 8 | ((((p >> 16) - g) & 255u) << 16) | (alpha ? p & 0xff000000u : 0xff000000u);
}

__device__ __forceinline__ uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }      // floor, per byte

__device__ __forceinline__ uint32_t sub_px(uint32_t a, uint32_t b)                                                       // (a - b) mod 256, per byte
{
    return (((a | 0x00ff00ffu) - (b & 0xff00ff00u)) & 0xff00ff00u) | (((a | 0xff00ff00u) - (b & 0x00ff00ffu)) & 0x00ff00ffu);
}

__device__ __forceinline__ uint32_t cost_px(uint32_t r)
{
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) { const uint32_t v = r >> (8u * k) & 255u; c += min(v, 256u - v); }
    return c;
}

struct Nb { uint32_t P, L, T, TL, TR; bool first, top, left; };

__device__ __forceinline__ Nb load_nb(const uint32_t *__restrict__ src, uint32_t w, uint32_t x, uint32_t y, bool alpha)
{
    Nb n;
    const size_t i = (size_t)y * w + x;
    n.P = load_px(src, i, alpha);
    n.L = x ? load_px(src, i - 1u, alpha) : 0u;
    n.T = y ? load_px(src, i - w, alpha) : 0u;
    n.TL = x && y ? load_px(src, i - w - 1u, alpha) : 0u;
    n.TR = y ? load_px(src, x + 1u < w ? i - w + 1u : (size_t)y * w, alpha) : 0u;      // the last column's: pixel (0, y)
    n.first = !x && !y; n.top = !y; n.left = !x;
    return n;
}

__device__ __forceinline__ uint32_t predict(uint32_t mode, const Nb &n)
{
    if (n.first) return kBlack;
    if (n.top) return n.L;
    if (n.left) return n.T;
    switch (mode) {
    case 1: return n.L;
    case 2: return n.T;
    case 7: return avg2(n.L, n.T);
    case 10: return avg2(avg2(n.L, n.TL), avg2(n.T, n.TR));
    case 11: {
        int dl = 0, dt = 0;                                   // |e - L| = |T - TL|, |e - T| = |L - TL| with e = L + T - TL
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const int l = (int)(n.L >> (8u * k) & 255u), tt = (int)(n.T >> (8u * k) & 255u), tl = (int)(n.TL >> (8u * k) & 255u);
            dl += abs(tt - tl); dt += abs(l - tl);
        }
        return dl < dt ? n.L : n.T;
    }
    default: {
        uint32_t p = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const int e = (int)(n.L >> (8u * k) & 255u) + (int)(n.T >> (8u * k) & 255u) - (int)(n.TL >> (8u * k) & 255u);
            p |= (uint32_t)min(max(e, 0), 255) << (8u * k);
        }
        return p;
    }
    }
}

__device__ __forceinline__ uint32_t residual(const uint32_t *__restrict__ src, uint32_t w, uint32_t x, uint32_t y, bool alpha,
                                             const unsigned char *__restrict__ modes, uint32_t ptx)
{
    const Nb n = load_nb(src, w, x, y, alpha);
    return sub_px(n.P, predict(modes[(y >> kPB) * ptx + (x >> kPB)], n));
}

__constant__ unsigned char c_modes[6] = {1, 2, 7, 10, 11, 12};

__global__ void __launch_bounds__(256)
k_webp_modes(const uint32_t *__restrict__ src, uint32_t w, uint32_t h, int alpha, unsigned char *__restrict__ modes)
{
    __shared__ uint32_t s_c[4][6];
    const uint32_t t = threadIdx.x, x = blockIdx.x * kPT + (t & (kPT - 1u)), y = blockIdx.y * kPT + (t >> kPB);
    uint32_t c[6] = {0, 0, 0, 0, 0, 0};
    if (x < w && y < h) {
        const Nb n = load_nb(src, w, x, y, alpha != 0);
#pragma unroll
        for (uint32_t k = 0; k < 6u; ++k) c[k] = cost_px(sub_px(n.P, predict(c_modes[k], n)));
    }
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) {
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) c[k] += __shfl_xor(c[k], d, 64);
        if ((t & 63u) == 0) s_c[t >> 6][k] = c[k];
    }
    __syncthreads();
    if (t == 0) {
        uint32_t best = 0, bc = 0xffffffffu;
        for (uint32_t k = 0; k < 6u; ++k) {
            const uint32_t v = s_c[0][k] + s_c[1][k] + s_c[2][k] + s_c[3][k];
            if (v < bc) { bc = v; best = k; }                 // a tie keeps the lower mode
        }
        modes[blockIdx.y * gridDim.x + blockIdx.x] = c_modes[best];
    }
}

// ---- prefix codes and their headers --------------------------------------------------------------------------------
// One thread's bit writer into words of its own (LDS), least significant bit first; n <= 32 and v < 2^n.
struct BW {
    uint32_t *w; u64 acc; uint32_t n, nw;
    __device__ void put(uint32_t v, uint32_t nb)
    {
        acc |= (u64)v << n; n += nb;
        if (n >= 32u) { w[nw++] = (uint32_t)acc; acc >>= 32; n -= 32u; }
    }
    __device__ uint32_t finish() { if (n) w[nw] = (uint32_t)acc; return nw * 32u + n; }
};

// The same into zeroed words that others write too, from any bit position.
struct ABW {
    uint32_t *w; u64 pos;
    __device__ void put(uint32_t v, uint32_t nb)
    {
        if (!nb) return;
        const uint32_t s = (uint32_t)pos & 31u;
        const u64 tv = (u64)v << s;
        uint32_t *p = w + (pos >> 5);
        if ((uint32_t)tv) atomicOr(p, (uint32_t)tv);
        if (s + nb > 32u && (uint32_t)(tv >> 32)) atomicOr(p + 1, (uint32_t)(tv >> 32));
        pos += nb;
    }
};

// nbits bits at src (from its bit 0; the bits behind them in the last word are zero) OR-ed into dst from bit D on, by nthreads threads.
__device__ __forceinline__ void or_bits(uint32_t *dst, u64 D, const uint32_t *src, uint32_t nbits, uint32_t t, uint32_t nthreads)
{
    const uint32_t s = (uint32_t)D & 31u;
    uint32_t *p = dst + (D >> 5);
    for (uint32_t i = t; i < (nbits + 31u) / 32u; i += nthreads) {
        const uint32_t v = src[i];
        if (!v) continue;
        atomicOr(p + i, v << s);
        if (s && v >> (32u - s)) atomicOr(p + i + 1u, v >> (32u - s));
    }
}

struct CodeWork {
    uint32_t hist[4][kSymPad];
    unsigned char len[4][kSymPad];
    unsigned short tok[4][256];                               // kind | extra value << 8
    uint32_t tf[4][32];
    unsigned char cllen[4][32];
    uint32_t clcode[4][32];
    uint32_t hb[4][kCodeWords];                               // each code's header bits
    uint32_t nb[4], used[4], single[4], ntok[4];
    HuffTmp T;
};

__constant__ unsigned char c_clorder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

// lens[0 .. n - 1], lens[n - 1] != 0, as tokens: zeros in runs of 18 while at least 11 remain, then 17, then literal zeros.  One thread.
__device__ uint32_t tokenise(const unsigned char *lens, uint32_t n, unsigned short *tok, uint32_t *tf)
{
    uint32_t ntok = 0, i = 0;
    while (i < n) {
        const uint32_t l = lens[i];
        if (l) { tok[ntok++] = (unsigned short)l; ++tf[l]; ++i; continue; }
        uint32_t run = 0;
        while (i + run < n && !lens[i + run]) ++run;
        i += run;
        while (run >= 11u) { const uint32_t m = min(run, 138u); tok[ntok++] = (unsigned short)(18u | (m - 11u) << 8); ++tf[18]; run -= m; }
        if (run >= 3u) { tok[ntok++] = (unsigned short)(17u | (run - 3u) << 8); ++tf[17]; run = 0; }
        for (; run; --run) { tok[ntok++] = 0; ++tf[0]; }
    }
    return ntok;
}

// Codes 0 .. NC - 1 (green, red, blue, alpha) from W.hist, by the whole workgroup of 256: W.len, code (NC tables of 256: bit-reversed
// code | length << 16, all 0 for a code of at most one symbol), and every code's header bits in W.hb / W.nb.
template <uint32_t NC>
__device__ void build_codes(CodeWork &W, uint32_t *code)
{
    const uint32_t t = threadIdx.x;
    for (uint32_t c = 0; c < NC; ++c) {
        const bool mine = W.hist[c][t] != 0;
        const uint32_t n = (uint32_t)__syncthreads_count(mine);
        if (t == 0) { W.used[c] = n; if (!n) W.single[c] = 0; }
        if (n == 1u && mine) W.single[c] = t;
        if (n >= 2u) build_lengths(W.hist[c], c ? 256u : 280u, 15u, W.len[c], W.T);
        else {
            for (uint32_t i = t; i < kSymPad; i += 256u) W.len[c][i] = 0;
            __syncthreads();
        }
        canonical_codes(W.len[c], 256u, code + 256u * c, W.T);
    }
    const uint32_t mc = t >> 6;
    if ((t & 63u) == 0 && mc < NC) {
        for (uint32_t k = 0; k < 32u; ++k) W.tf[mc][k] = 0;
        W.ntok[mc] = 0;
        if (W.used[mc] >= 2u) {
            uint32_t last = 255u;
            while (!W.len[mc][last]) --last;
            W.ntok[mc] = tokenise(W.len[mc], last + 1u, W.tok[mc], W.tf[mc]);
        }
    }
    __syncthreads();
    for (uint32_t c = 0; c < NC; ++c) {
        if (W.used[c] < 2u) continue;                         // (the same in every thread)
        build_lengths(W.tf[c], 19u, 7u, W.cllen[c], W.T);
        canonical_codes(W.cllen[c], 19u, W.clcode[c], W.T);
    }
    if ((t & 63u) == 0 && mc < NC) {
        BW b = {W.hb[mc], 0ull, 0u, 0u};
        if (W.used[mc] < 2u) {
            const uint32_t s = W.single[mc];
            b.put(1u, 2u);                                    // simple, one symbol
            b.put(s > 1u ? 1u : 0u, 1u);
            b.put(s, s > 1u ? 8u : 1u);
        } else {
            b.put(0u, 1u);
            uint32_t ncl = 19u;
            while (ncl > 4u && !W.cllen[mc][c_clorder[ncl - 1u]]) --ncl;
            b.put(ncl - 4u, 4u);
            for (uint32_t i = 0; i < ncl; ++i) b.put(W.cllen[mc][c_clorder[i]], 3u);
            const uint32_t ntok = W.ntok[mc], m = ntok - 2u, bl = m ? 32u - (uint32_t)__clz((int)m) : 0u, k = max(1u, (bl + 1u) / 2u);
            b.put(1u, 1u);
            b.put(k - 1u, 3u);
            b.put(m, 2u * k);
            for (uint32_t i = 0; i < ntok; ++i) {
                const uint32_t tk = W.tok[mc][i], kind = tk & 31u, cc = W.clcode[mc][kind];
                b.put(cc & 0xffffu, cc >> 16);
                if (kind == 17u) b.put(tk >> 8, 3u);
                if (kind == 18u) b.put(tk >> 8, 7u);
            }
        }
        W.nb[mc] = b.finish();
    }
    __syncthreads();
}

// ---- the fixed header and the two sub-images ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t *s_w, uint32_t mine, uint32_t t, uint32_t &total)
{
    const uint32_t incl = wave_incl_scan(mine, t & 63u);
    if ((t & 63u) == 63u) s_w[t >> 6] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t k = 0; k < (t >> 6); ++k) before += s_w[k];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return before + incl - mine;
}

// An entropy-coded image of n pixels at bit `pos` of `sub`: green = modes[i] (red 0), or green = i & 255 and red = i >> 8 when modes
// is null; blue 0, alpha 255.  Returns the position behind it.
__device__ u64 sub_image(CodeWork &W, uint32_t *s_code, uint32_t *s_w, uint32_t *sub, u64 pos, const unsigned char *modes, uint32_t n)
{
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < 2u * kSymPad; i += 256u) (&W.hist[0][0])[i] = 0;
    __syncthreads();
    for (uint32_t i = t; i < n; i += 256u) {
        atomicAdd(&W.hist[0][modes ? modes[i] : i & 255u], 1u);
        atomicAdd(&W.hist[1][modes ? 0u : i >> 8], 1u);
    }
    __syncthreads();
    build_codes<2>(W, s_code);
    or_bits(sub, pos + 1u, W.hb[0], W.nb[0], t, 256u);        // (the bit in front: no colour cache)
    or_bits(sub, pos + 1u + W.nb[0], W.hb[1], W.nb[1], t, 256u);
    pos += 1u + W.nb[0] + W.nb[1];
    if (t == 0) {
        ABW b = {sub, pos};
        b.put(1u, 4u);                                        // blue: simple, symbol 0
        b.put(5u | 255u << 3, 11u);                           // alpha: simple, symbol 255 in 8 bits
        b.put(1u, 4u);                                        // distance: simple, symbol 0
    }
    pos += 19u;
    const uint32_t per = (n + 255u) / 256u, lo = min(t * per, n), hi = min(lo + per, n);
    uint32_t mine = 0, total;
    for (uint32_t i = lo; i < hi; ++i) mine += (s_code[modes ? modes[i] : i & 255u] >> 16) + (s_code[256u + (modes ? 0u : i >> 8)] >> 16);
    ABW b = {sub, pos + block_excl_scan_256(s_w, mine, t, total)};
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t cg = s_code[modes ? modes[i] : i & 255u], cr = s_code[256u + (modes ? 0u : i >> 8)];
        b.put(cg & 0xffffu, cg >> 16);
        b.put(cr & 0xffffu, cr >> 16);
    }
    __syncthreads();
    return pos + total;
}

// The stream up to the first group header, by one workgroup: sub (subwords words) is zeroed here; subinfo[0] = the bits.
__device__ void sub_images(CodeWork &W, uint32_t *s_code, uint32_t *s_w, uint32_t w, uint32_t h, int alpha, const unsigned char *__restrict__ modes,
                           uint32_t npt, uint32_t ng, uint32_t *__restrict__ sub, uint32_t subwords, uint32_t *__restrict__ subinfo)
{
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < subwords; i += 256u) sub[i] = 0;
    __threadfence_block();
    __syncthreads();
    if (t == 0) {
        ABW b = {sub, 0ull};
        b.put(0x2fu, 8u); b.put(w - 1u, 14u); b.put(h - 1u, 14u); b.put(alpha ? 1u : 0u, 1u); b.put(0u, 3u);
        b.put(1u | 2u << 1, 3u);                              // a transform: subtract green
        b.put(1u | 0u << 1 | (kPB - 2u) << 3, 6u);            // a transform: the predictor, its tile bits
    }
    u64 pos = sub_image(W, s_code, s_w, sub, 49ull, modes, npt);
    if (t == 0) { ABW b = {sub, pos}; b.put(0u | 0u << 1 | 1u << 2 | (kEB - 2u) << 3, 6u); }      // no transform, no cache, meta codes, their tile bits
    pos = sub_image(W, s_code, s_w, sub, pos + 6u, nullptr, ng);
    if (t == 0) subinfo[0] = (uint32_t)pos;
}

// ---- statistics and codes of one entropy tile ------------------------------------------------------------------------
// Workgroup g < G: tile g.  codes: G x 4 x 256 words; hdr: G x kHdrWords words; cnt[g] = the group header's bits;
// cnt[G + y * gx + tile column] = a run's bits.  Workgroup G: the fixed header and the two sub-images (they need the mode map only, and
// one workgroup's serial work hides behind the tiles').
__global__ void __launch_bounds__(256)
k_webp_stats(const uint32_t *__restrict__ src, uint32_t w, uint32_t h, int alpha, const unsigned char *__restrict__ modes, uint32_t ptx, uint32_t pty,
             uint32_t gx, uint32_t G, uint32_t *__restrict__ codes, uint32_t *__restrict__ hdr, uint32_t *__restrict__ cnt, uint32_t *__restrict__ sub,
             uint32_t subwords, uint32_t *__restrict__ subinfo)
{
    __shared__ CodeWork W;
    __shared__ uint32_t s_res[kET * kET], s_out[kHdrWords], s_code[512], s_w[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, g = blockIdx.x, by = g / gx, bx = g - by * gx;
    if (g == G) { sub_images(W, s_code, s_w, w, h, alpha, modes, ptx * pty, G, sub, subwords, subinfo); return; }
    for (uint32_t i = t; i < 4u * kSymPad; i += 256u) (&W.hist[0][0])[i] = 0;
    for (uint32_t i = t; i < kHdrWords; i += 256u) s_out[i] = 0;
    __syncthreads();
    const uint32_t x = bx * kET + lane;
    for (uint32_t ry = wv; ry < kET; ry += 4u) {
        const uint32_t y = by * kET + ry;
        if (x < w && y < h) {
            const uint32_t r = residual(src, w, x, y, alpha != 0, modes, ptx);
            s_res[ry * kET + lane] = r;
            atomicAdd(&W.hist[0][r >> 8 & 255u], 1u); atomicAdd(&W.hist[1][r & 255u], 1u);
            atomicAdd(&W.hist[2][r >> 16 & 255u], 1u); atomicAdd(&W.hist[3][r >> 24], 1u);
        }
    }
    __syncthreads();
    build_codes<4>(W, codes + (size_t)g * 1024u);
    uint32_t at = 0;
    for (uint32_t c = 0; c < 4u; ++c) { or_bits(s_out, at, W.hb[c], W.nb[c], t, 256u); at += W.nb[c]; }
    if (t == 0) { ABW b = {s_out, at}; b.put(1u, 4u); }       // the distance code: simple, symbol 0
    at += 4u;
    __syncthreads();
    for (uint32_t i = t; i < (at + 31u) / 32u; i += 256u) hdr[(size_t)g * kHdrWords + i] = s_out[i];
    if (t == 0) cnt[g] = at;
    for (uint32_t ry = wv; ry < kET; ry += 4u) {
        const uint32_t y = by * kET + ry;
        if (y >= h) break;
        uint32_t n = 0;
        if (x < w) {
            const uint32_t r = s_res[ry * kET + lane];
            n = (uint32_t)W.len[0][r >> 8 & 255u] + W.len[1][r & 255u] + W.len[2][r >> 16 & 255u] + W.len[3][r >> 24];
        }
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) n += __shfl_xor(n, d, 64);
        if (lane == 0) cnt[G + (size_t)y * gx + bx] = n;
    }
}

// ---- placement -----------------------------------------------------------------------------------------------------
// off[i] = the bit at which piece i (group headers, then runs in raster order) begins; info's own word is the payload's bytes.
__global__ void __launch_bounds__(1024)
k_webp_scan(const uint32_t *__restrict__ cnt, uint32_t n, const uint32_t *__restrict__ subinfo, u64 *__restrict__ off, uint32_t *__restrict__ info,
            unsigned char *__restrict__ out, u64 cap)
{
    __shared__ u64 s_sum[1024];
    const uint32_t t = threadIdx.x;
    const auto len = [&](uint32_t i) { return cnt[i]; };
    const Placement p = place_pieces(s_sum, n, t, (u64)subinfo[0], len);
    const u64 payload = (subinfo[0] + p.total + 7u) / 8u, need = 8u + payload + (payload & 1u);
    if (finish_placement(info, out, need, cap, kPB | kEB << 8, (uint32_t)payload, t)) return;      // a block that does not fit leaves nothing behind the record
    store_offsets(off, p, len);
    if (t < 8u) {
        const unsigned char hd[8] = {'V', 'P', '8', 'L', (unsigned char)payload, (unsigned char)(payload >> 8), (unsigned char)(payload >> 16), (unsigned char)(payload >> 24)};
        out[16u + t] = hd[t];
    }
    if (t == 8u && (payload & 1u)) out[24u + payload] = 0u;
}

__global__ void __launch_bounds__(256) k_webp_clear(const uint32_t *__restrict__ info, uint32_t *__restrict__ asmb)
{
    if (info[kInfoStatus]) return;
    const uint32_t nw = (info[kInfoExtra] + 3u) / 4u + 2u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < nw; i += gridDim.x * 256u) asmb[i] = 0;
}

// Workgroup g < G: group g's header; workgroup G: the stream's beginning.
__global__ void __launch_bounds__(256)
k_webp_heads(const uint32_t *__restrict__ hdr, const uint32_t *__restrict__ cnt, const u64 *__restrict__ off, const uint32_t *__restrict__ sub,
             const uint32_t *__restrict__ subinfo, const uint32_t *__restrict__ info, uint32_t G, uint32_t *__restrict__ asmb)
{
    if (info[kInfoStatus]) return;
    const uint32_t g = blockIdx.x;
    if (g < G) or_bits(asmb, off[g], hdr + (size_t)g * kHdrWords, cnt[g], threadIdx.x, 256u);
    else or_bits(asmb, 0ull, sub, subinfo[0], threadIdx.x, 256u);
}

// ---- emission ------------------------------------------------------------------------------------------------------
// A run of at most 64 pixels is at most 64 * 60 bits behind at most 31 bits of its first word: 122 words.
__global__ void __launch_bounds__(256)
k_webp_emit(const uint32_t *__restrict__ src, uint32_t w, uint32_t h, int alpha, const unsigned char *__restrict__ modes, uint32_t ptx, uint32_t gx,
            const uint32_t *__restrict__ codes, const u64 *__restrict__ roff, const uint32_t *__restrict__ info, uint32_t *__restrict__ asmb)
{
    __shared__ uint32_t s_w[4][124];
    if (info[kInfoStatus]) return;
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6, nr = h * gx, r = blockIdx.x * 4u + wv;
    uint32_t *sw = s_w[wv];
    for (uint32_t i = lane; i < 124u; i += 64u) sw[i] = 0;
    __syncthreads();
    u64 bits = 0, base = 0;
    uint32_t len = 0;
    if (r < nr) {
        const uint32_t y = r / gx, tx = r - y * gx, x = tx * kET + lane;
        base = roff[r];                                       // (the runs' offsets: behind the G group headers')
        if (x < w) {
            const uint32_t res = residual(src, w, x, y, alpha != 0, modes, ptx);
            const uint32_t *cd = codes + ((size_t)(y >> kEB) * gx + tx) * 1024u;
            const uint32_t c[4] = {cd[res >> 8 & 255u], cd[256u + (res & 255u)], cd[512u + (res >> 16 & 255u)], cd[768u + (res >> 24)]};
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) { bits |= (u64)(c[k] & 0xffffu) << len; len += c[k] >> 16; }
        }
    }
    const uint32_t incl = wave_incl_scan(len, lane), total = (uint32_t)__shfl((int)incl, 63, 64), s0 = (uint32_t)base & 31u;
    if (len) {
        const uint32_t p = s0 + incl - len, s = p & 31u;
        const u64 tv = bits << s;
        atomicOr(&sw[p >> 5], (uint32_t)tv);
        if ((uint32_t)(tv >> 32)) atomicOr(&sw[(p >> 5) + 1u], (uint32_t)(tv >> 32));
        if (s && (uint32_t)(bits >> (64u - s))) atomicOr(&sw[(p >> 5) + 2u], (uint32_t)(bits >> (64u - s)));
    }
    __syncthreads();
    const uint32_t nw = total ? (s0 + total + 31u) / 32u : 0u;
    uint32_t *dst = asmb + (base >> 5);
    for (uint32_t i = lane; i < nw; i += 64u) {
        const uint32_t v = sw[i];
        if (i == 0 || i + 1u == nw) { if (v) atomicOr(dst + i, v); }      // a word that a neighbouring piece writes too
        else dst[i] = v;
    }
}

// Workgroup b: payload bytes 4096 b .. of the assembly buffer, which is readable a word beyond them, to out + 24.
__global__ void __launch_bounds__(256)
k_webp_copy(const uint32_t *__restrict__ asmb, const uint32_t *__restrict__ info, unsigned char *__restrict__ out)
{
    __shared__ uint32_t s_b[1026];
    const uint32_t t = threadIdx.x, start = blockIdx.x * 4096u;
    if (info[kInfoStatus] || start >= info[kInfoExtra]) return;
    const uint32_t n = min(4096u, info[kInfoExtra] - start);
    for (uint32_t i = t; i <= n / 4u + 1u; i += 256u) s_b[i] = asmb[start / 4u + i];
    __syncthreads();
    store_bytes<256>(out + 24u + start, s_b, n, t);
}

} // namespace

uint64_t webp_bound_bits(uint32_t w, uint32_t h)
{
    const uint64_t pt = (uint64_t)((w + kPT - 1u) / kPT) * ((h + kPT - 1u) / kPT), g = (uint64_t)((w + kET - 1u) / kET) * ((h + kET - 1u) / kET);
    return 49u + (1u + kGroupBits + 60u * pt) + 6u + (1u + kGroupBits + 60u * g) + g * kGroupBits + 60u * (uint64_t)w * h;
}

WebpLayout webp_layout(uint32_t w, uint32_t h)
{
    WebpLayout l;
    l.ptx = (w + kPT - 1u) / kPT; l.pty = (h + kPT - 1u) / kPT;
    l.gx = (w + kET - 1u) / kET; l.gy = (h + kET - 1u) / kET;
    l.G = l.gx * l.gy;
    l.NR = h * l.gx;
    const uint64_t pt = (uint64_t)l.ptx * l.pty;
    l.subwords = (uint32_t)((49u + (1u + kGroupBits + 60u * pt) + 6u + (1u + kGroupBits + 60u * (uint64_t)l.G) + 31u) / 32u + 2u);
    l.asmwords = (size_t)((webp_bound_bits(w, h) + 31u) / 32u + 4u);
    // words: the mode map | the groups' code tables | their staged headers | the pieces' bit counts | their bit offsets (u64) | the staged beginning | its bits | info | the assembly buffer
    l.modes = 0;
    l.codes = l.modes + (size_t)(pt + 3u) / 4u;
    l.hdr = l.codes + (size_t)l.G * 1024u;
    l.cnt = l.hdr + (size_t)l.G * kHdrWords;
    l.off = (l.cnt + l.G + l.NR + 1u) & ~(size_t)1u;
    l.sub = l.off + 2u * ((size_t)l.G + l.NR);
    l.subinfo = l.sub + l.subwords;
    l.info = l.subinfo + 4u;
    l.asmb = l.info + 4u;
    l.words = l.asmb + l.asmwords;
    return l;
}

void launch_webp_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int channels, uint32_t *scratch, unsigned char *out,
                        size_t cap, size_t bound)
{
    const WebpLayout l = webp_layout(w, h);
    const uint32_t *pix = (const uint32_t *)src;
    unsigned char *modes = (unsigned char *)(scratch + l.modes);
    uint32_t *codes = scratch + l.codes, *hdr = scratch + l.hdr, *cnt = scratch + l.cnt, *sub = scratch + l.sub, *subinfo = scratch + l.subinfo;
    uint32_t *info = scratch + l.info, *asmb = scratch + l.asmb;
    u64 *off = (u64 *)(scratch + l.off);
    const int alpha = channels == 4;
    const uint32_t n = l.G + l.NR;
    const size_t room = std::min(cap, bound) - 24u;            // payload bytes that can fit (cap >= 24: the callers checked)
    hipLaunchKernelGGL(k_webp_modes, dim3(l.ptx, l.pty), dim3(256), 0, st, pix, w, h, alpha, modes);
    hipLaunchKernelGGL(k_webp_stats, dim3(l.G + 1u), dim3(256), 0, st, pix, w, h, alpha, (const unsigned char *)modes, l.ptx, l.pty, l.gx, l.G, codes, hdr, cnt,
                       sub, l.subwords, subinfo);
    hipLaunchKernelGGL(k_webp_scan, dim3(1), dim3(1024), 0, st, (const uint32_t *)cnt, n, (const uint32_t *)subinfo, off, info, out, (u64)cap);
    hipLaunchKernelGGL(k_webp_clear, dim3((uint32_t)std::min<size_t>(2048u, (l.asmwords + 255u) / 256u)), dim3(256), 0, st, (const uint32_t *)info, asmb);
    hipLaunchKernelGGL(k_webp_heads, dim3(l.G + 1u), dim3(256), 0, st, (const uint32_t *)hdr, (const uint32_t *)cnt, (const u64 *)off, (const uint32_t *)sub,
                       (const uint32_t *)subinfo, (const uint32_t *)info, l.G, asmb);
    hipLaunchKernelGGL(k_webp_emit, dim3((l.NR + 3u) / 4u), dim3(256), 0, st, pix, w, h, alpha, (const unsigned char *)modes, l.ptx, l.gx, (const uint32_t *)codes,
                       (const u64 *)off + l.G, (const uint32_t *)info, asmb);
    if (room)
        hipLaunchKernelGGL(k_webp_copy, dim3((uint32_t)((room + 4095u) / 4096u)), dim3(256), 0, st, (const uint32_t *)asmb, (const uint32_t *)info, out);
}
