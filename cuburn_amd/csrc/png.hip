// png.hip — truecolour PNG (colour type 2 or 6, not interlaced; 8 or 16 bits a sample) from u8 or u16 [h][w][4] on the device.  DESIGN.md §4.9.
// Four launches per frame (five with FL_PNG_ADAPTIVE), no host wait between them:
//   k_png_choose    FL_PNG_ADAPTIVE only, one workgroup per row: the row's cost under each of the five filter types -> its type
//   k_png_filter    the Paeth filter on every row: pixels -> the filtered byte stream (a filter byte 4, then w * channels residuals per row);
//   k_png_filter_x  the same for 16-bit samples (most significant byte first) and for rows of chosen types
//   k_png_segment   one workgroup per segment of `seg` filtered bytes, coded with no reference before its start: tokens (literal / run
//                   of distance 1) -> histogram -> length-limited Huffman code -> one dynamic block packed in LDS, or one stored block
//                   when that is no smaller (decided from the counted bits, before anything is emitted); the segment's Adler-32 parts
//                   (its TILES form, launch_deflate_tiles, codes the tiles of tiff.hip: every segment a final block of its own;
//                   with LENS, launch_deflate_pieces, the cropped tiles of exr.hip, each of its own length)
//   k_png_scan      one workgroup: the segments' places in the file, the Adler-32 of the whole stream, the 16-byte record and the header
//   k_png_gather    one workgroup per segment: the finished IDAT (length, tag, bytes, CRC-32) copied to its place, IEND behind the last
// The frame-block form of the last two (launch_apng_encode) writes one frame of an APNG: the same chunks with no header
// in front and no IEND behind, as IDATs (frame 0) or as fdATs, each with its sequence number in front of the data and under the CRC.
// The segments are byte aligned (an empty stored block behind a dynamic one) and share no history, which is what makes them parallel.
// Nothing is stored at or beyond `cap`: the gather stores nothing when the file does not fit.
#include "kernels.h"
#include "encode_device.h"
#include <cstdlib>

namespace {

constexpr uint32_t kAdlerMod = 65521u;
constexpr uint32_t kCrcPoly = 0xedb88320u;
constexpr uint32_t kLitSyms = 286u, kClSyms = 19u;
__device__ const unsigned char g_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};      // RFC 1951 3.2.7

struct PngHeaderArg { unsigned char b[FL_PNG_HEADER_BYTES]; };

// ---- the filter ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t paeth(int a, int b, int c)
{
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (uint32_t)(pa <= pb && pa <= pc ? a : pb <= pc ? b : c);
}

// A thread per four bytes of the stream (F < 2^32 bytes, rows of rowlen = 1 + w * CH); filt holds ceil(F / 4) words.
template <int CH>
__global__ void __launch_bounds__(256)
k_png_filter(const unsigned char *__restrict__ src, uint32_t w, uint32_t rowlen, uint32_t F, uint32_t *__restrict__ filt)
{
    const u64 p64 = ((u64)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (p64 >= F) return;
    const uint32_t p0 = (uint32_t)p64;
    uint32_t row = p0 / rowlen, col = p0 - row * rowlen, out = 0;
    const size_t pitch = (size_t)w * 4u;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (p64 + k >= F) break;
        uint32_t v = 4u;                                      // the row's filter byte: Paeth
        if (col) {
            const uint32_t x = col - 1u, px = x / CH, cp = x - px * CH;
            const unsigned char *s = src + (size_t)row * pitch + (size_t)px * 4u + cp;
            const int a = px ? s[-4] : 0, b = row ? *(s - pitch) : 0, c = px && row ? *(s - pitch - 4) : 0;
            v = ((uint32_t)s[0] - paeth(a, b, c)) & 0xffu;
        }
        out |= v << (8u * k);
        if (++col == rowlen) { col = 0; ++row; }
    }
    filt[p0 >> 2] = out;
}

// ---- 16-bit samples and the per-row filter choice (FL_PNG_ADAPTIVE) -----------------------------------------------------
// Byte cp (0 .. CH * BITS / 8 - 1) of the pixel at pix (u8 or u16 [4], native byte order): the file holds a 16-bit sample most
// significant byte first.
template <int BITS>
__device__ __forceinline__ int sample_byte(const unsigned char *pix, uint32_t cp)
{
    if (BITS == 8) return pix[cp];
    return ((const unsigned short *)pix)[cp >> 1] >> (8u * (1u - (cp & 1u))) & 0xffu;
}

// What filter type ft (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) predicts from the bytes to the left, above and above left
__device__ __forceinline__ uint32_t predict(uint32_t ft, int a, int b, int c)
{
    return ft == 0 ? 0u : ft == 1 ? (uint32_t)a : ft == 2 ? (uint32_t)b : ft == 3 ? (uint32_t)(a + b) >> 1 : paeth(a, b, c);
}

// One workgroup per row, a thread per pixel (and per 256th pixel behind it): cost[t] = the sum over the row's residual bytes r under
// filter type t of min(r, 256 - r), exact in 32 bits (at most 65535 * 8 * 128); types[row] = the smallest t of minimal cost.
template <int CH, int BITS>
__global__ void __launch_bounds__(256)
k_png_choose(const unsigned char *__restrict__ src, uint32_t w, unsigned char *__restrict__ types)
{
    constexpr uint32_t BPP = CH * BITS / 8, PIX = 4 * BITS / 8;
    __shared__ uint32_t s_cost[4][5];
    const uint32_t t = threadIdx.x, row = blockIdx.x;
    const size_t pitch = (size_t)w * PIX;
    const unsigned char *line = src + (size_t)row * pitch;
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (uint32_t px = t; px < w; px += 256u) {
        const unsigned char *s = line + (size_t)px * PIX;
#pragma unroll
        for (uint32_t cp = 0; cp < BPP; ++cp) {
            const int x = sample_byte<BITS>(s, cp);
            const int a = px ? sample_byte<BITS>(s - PIX, cp) : 0, b = row ? sample_byte<BITS>(s - pitch, cp) : 0;
            const int c = px && row ? sample_byte<BITS>(s - pitch - PIX, cp) : 0;
#pragma unroll
            for (uint32_t ft = 0; ft < 5; ++ft) {
                const uint32_t r = ((uint32_t)x - predict(ft, a, b, c)) & 0xffu;
                cost[ft] += min(r, 256u - r);
            }
        }
    }
#pragma unroll
    for (uint32_t ft = 0; ft < 5; ++ft) {
#pragma unroll
        for (uint32_t d = 32; d; d >>= 1) cost[ft] += __shfl_xor(cost[ft], d, 64);
    }
    if ((t & 63u) == 0) {
#pragma unroll
        for (uint32_t ft = 0; ft < 5; ++ft) s_cost[t >> 6][ft] = cost[ft];
    }
    __syncthreads();
    if (t == 0) {
        uint32_t best = 0, least = 0xffffffffu;
        for (uint32_t ft = 0; ft < 5; ++ft) {
            const uint32_t v = s_cost[0][ft] + s_cost[1][ft] + s_cost[2][ft] + s_cost[3][ft];
            if (v < least) { least = v; best = ft; }          // (a tie keeps the lower type)
        }
        types[row] = (unsigned char)best;
    }
}

// k_png_filter for the other forms: 16-bit samples, and rows whose type comes from `types` (ADAPT) instead of being Paeth.
// The same thread per four bytes of the stream; rowlen = 1 + w * CH * BITS / 8.
template <int CH, int BITS, bool ADAPT>
__global__ void __launch_bounds__(256)
k_png_filter_x(const unsigned char *__restrict__ src, uint32_t w, uint32_t rowlen, uint32_t F, const unsigned char *__restrict__ types,
               uint32_t *__restrict__ filt)
{
    constexpr uint32_t BPP = CH * BITS / 8, PIX = 4 * BITS / 8;
    const u64 p64 = ((u64)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (p64 >= F) return;
    const uint32_t p0 = (uint32_t)p64;
    uint32_t row = p0 / rowlen, col = p0 - row * rowlen, out = 0;
    const size_t pitch = (size_t)w * PIX;
    uint32_t ft = ADAPT ? types[row] : 4u;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (p64 + k >= F) break;
        uint32_t v = ft;                                      // the row's filter byte
        if (col) {
            const uint32_t x = col - 1u, px = x / BPP, cp = x - px * BPP;
            const unsigned char *s = src + (size_t)row * pitch + (size_t)px * PIX;
            const int a = px ? sample_byte<BITS>(s - PIX, cp) : 0, b = row ? sample_byte<BITS>(s - pitch, cp) : 0;
            const int c = px && row ? sample_byte<BITS>(s - pitch - PIX, cp) : 0;
            v = ((uint32_t)sample_byte<BITS>(s, cp) - (ADAPT ? predict(ft, a, b, c) : paeth(a, b, c))) & 0xffu;
        }
        out |= v << (8u * k);
        if (++col == rowlen) {
            col = 0; ++row;
            if (ADAPT && p64 + k + 1u < F) ft = types[row];   // (row < h while a byte of the stream is left)
        }
    }
    filt[p0 >> 2] = out;
}

// ---- tokens ---------------------------------------------------------------------------------------------------------
// A segment's bytes fall into groups: a head, which differs from the byte before it (or starts the segment), and the bytes behind it
// that repeat it.  The head is a literal; r repeats are matches of distance 1 and length min(r, 258) while r >= 3, then literals.
// A group belongs to the lane in whose span its head lies, so the tokens do not depend on how the spans cut the segment.
__device__ __forceinline__ void len_symbol(uint32_t L, uint32_t &sym, uint32_t &eb, uint32_t &ev)      // 3 <= L <= 258 (RFC 1951 3.2.5)
{
    const uint32_t l = L - 3u;
    if (L == 258u) { sym = 285u; eb = 0; ev = 0; return; }
    if (l < 8u) { sym = 257u + l; eb = 0; ev = 0; return; }
    eb = 29u - (uint32_t)__clz(l);                            // floor(log2 l) - 2
    sym = 261u + 4u * eb + (l >> eb & 3u);
    ev = l & ((1u << eb) - 1u);
}

struct Tok { int prev; uint32_t run; };
template <class S>
__device__ __forceinline__ void flush_run(uint32_t run, int prev, S &s)
{
    while (run >= 3u) { const uint32_t L = min(run, 258u); s.match(L); run -= L; }
    for (; run; --run) s.lit((uint32_t)prev);
}
template <class S>
__device__ __forceinline__ void step(Tok &t, uint32_t b, S &s)
{
    if ((int)b == t.prev) { ++t.run; return; }
    flush_run(t.run, t.prev, s);
    t.run = 0; t.prev = (int)b;
    s.lit(b);
}

// f(pos, byte) for the bytes [from, hi) of the segment at sp (16-byte aligned; the buffer is readable up to the next 16-byte boundary)
template <class Fn>
__device__ __forceinline__ void for_bytes(const unsigned char *sp, uint32_t from, uint32_t hi, Fn &&f)
{
    for (uint32_t q = from & ~15u; q < hi; q += 16u) {
        const uint4 v = *(const uint4 *)(sp + q);
        const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
#pragma unroll 1
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t pos = q + 4u * j + k;
                if (pos >= from && pos < hi) f(pos, wd[j] >> (8u * k) & 0xffu);
            }
    }
}

struct Bits {                         // a lane's writer into the segment's bit buffer: bytes fill from the least significant bit, words are little-endian
    uint32_t *words; uint32_t w; u64 acc; uint32_t n;
    __device__ __forceinline__ void put(uint32_t v, uint32_t len)          // len <= 32, n < 32
    {
        acc |= (u64)v << n;
        n += len;
        if (n >= 32u) { atomicOr(&words[w++], (uint32_t)acc); acc >>= 32; n -= 32u; }
    }
    __device__ __forceinline__ void flush() { if (n) atomicOr(&words[w], (uint32_t)acc); }
};
__device__ __forceinline__ Bits bits_at(uint32_t *words, uint32_t bit) { return Bits{words, bit >> 5, 0, bit & 31u}; }

struct HistSink {
    uint32_t *hist; uint32_t nm;
    __device__ __forceinline__ void lit(uint32_t b) { atomicAdd(&hist[b], 1u); }
    __device__ __forceinline__ void match(uint32_t L) { uint32_t s, eb, ev; len_symbol(L, s, eb, ev); atomicAdd(&hist[s], 1u); ++nm; }
};
struct CountSink {                    // code[s] = bit-reversed code | length << 16
    const uint32_t *code; uint32_t bits;
    __device__ __forceinline__ void lit(uint32_t b) { bits += code[b] >> 16; }
    __device__ __forceinline__ void match(uint32_t L) { uint32_t s, eb, ev; len_symbol(L, s, eb, ev); bits += (code[s] >> 16) + eb + 1u; }
};
struct EmitSink {
    const uint32_t *code; Bits b;
    __device__ __forceinline__ void lit(uint32_t v) { const uint32_t c = code[v]; b.put(c & 0xffffu, c >> 16); }
    __device__ __forceinline__ void match(uint32_t L)
    {
        uint32_t s, eb, ev;
        len_symbol(L, s, eb, ev);
        const uint32_t c = code[s];
        b.put(c & 0xffffu, c >> 16);
        b.put(ev, eb + 1u);                                   // the extra bits, and the lone distance code (symbol 0, one bit: 0)
    }
};

// ---- length-limited Huffman codes: build_lengths, canonical_codes and their HuffTmp are in encode_device.h (the JPEG encoder builds its tables with
// the first, the WebP encoder its codes with both) ----

// ---- one segment per workgroup -----------------------------------------------------------------------------------------
// Lane t owns the bytes [t * per, (t + 1) * per) of the segment (per a multiple of 16, 256 * per >= seg).  The segment's bytes
// (lens[it] of them, at most n + 5: the stored form) go to segbuf + it * stride; adl[it] = its own Adler-32 (a | b << 16).
// Dynamic LDS: the bit buffer, (seg + 8) / 4 + 2 words.
// TILES (tiff.hip): every segment is a stream of its own, so each one ends like the last — BFINAL set, no empty stored block behind it.
// LENS (exr.hip, with TILES): segment `it` holds lens[it] bytes (1 .. seg) where the kernel starts, not min(seg, F - base).
template <bool TILES, bool LENS = false>
__global__ void __launch_bounds__(256)
k_png_segment(const unsigned char *__restrict__ filt, uint32_t F, uint32_t seg, uint32_t nseg, uint32_t per,
              unsigned char *__restrict__ segbuf, uint32_t stride, uint32_t *__restrict__ lens, uint32_t *__restrict__ adl)
{
    extern __shared__ uint32_t s_bits[];
    __shared__ uint32_t s_hist[kSymPad], s_code[kSymPad], s_clfreq[kClSyms], s_clcode[kClSyms], s_misc[8], s_wsum[4];
    __shared__ unsigned char s_len[kSymPad], s_cllen[kClSyms];
    __shared__ unsigned short s_lead[256], s_seq[320];
    __shared__ HuffTmp T;
    enum { kMatches = 0, kSum1, kSum2, kNseq, kHdrBits, kHclen, kHlit };
    const uint32_t t = threadIdx.x, it = blockIdx.x;
    const uint32_t base = it * seg, n = LENS ? lens[it] : min(seg, F - base);
    const bool last = TILES || it + 1u == nseg;
    const unsigned char *sp = LENS ? filt + (size_t)it * seg : filt + base;
    const uint32_t lo = min(t * per, n), hi = min(lo + per, n);
    for (uint32_t i = t; i < kSymPad; i += 256u) s_hist[i] = i == 256u ? 1u : 0u;      // one end-of-block
    if (t < kClSyms) s_clfreq[t] = 0;
    if (t < 8u) s_misc[t] = 0;
    __syncthreads();

    // pass A: the histogram of the groups whose head lies here, the leading bytes that belong to a group before, the Adler sums
    const int prevb = lo && lo < hi ? (int)sp[lo - 1u] : -1;
    uint32_t lead = 0, s1 = 0, s2 = 0;
    bool started = false;
    HistSink hs = {s_hist, 0};
    Tok tk = {prevb, 0};
    for_bytes(sp, lo, hi, [&](uint32_t pos, uint32_t b) {
        s1 += b; s2 += (n - pos) * b;                         // (per <= 128: below 2^30)
        if (!started) {
            if ((int)b == prevb) { ++lead; return; }
            started = true;
        }
        step(tk, b, hs);
    });
    s_lead[t] = (unsigned short)lead;
    if (s1) { atomicAdd(&s_misc[kSum1], s1 % kAdlerMod); atomicAdd(&s_misc[kSum2], s2 % kAdlerMod); }
    __syncthreads();
    uint32_t tail = 0;                                        // bytes of this lane's last group: its repeats here and in the lanes behind
    if (started) {
        tail = tk.run;
        for (uint32_t j = t + 1u; j < 256u; ++j) {
            const uint32_t jlo = min(j * per, n), jn = min(jlo + per, n) - jlo, l = s_lead[j];
            tail += l;
            if (jn == 0 || l < jn) break;
        }
        flush_run(tail, tk.prev, hs);
    }
    if (hs.nm) atomicAdd(&s_misc[kMatches], hs.nm);
    __syncthreads();
    const uint32_t nmatch = s_misc[kMatches];

    build_lengths(s_hist, kLitSyms, 15u, s_len, T);
    canonical_codes(s_len, kLitSyms, s_code, T);

    // the code lengths, run-length coded in the code-length alphabet (RFC 1951 3.2.7): s_seq = symbol | extra << 8
    if (t == 0) {
        uint32_t hlit = kLitSyms;
        while (hlit > 257u && s_len[hlit - 1u] == 0) --hlit;
        const uint32_t N = hlit + 1u, dlen = nmatch ? 1u : 0u;            // one distance code: length 1 when a match uses it, 0 when none does
        uint32_t ns = 0;
        auto emit = [&](uint32_t sym, uint32_t extra) { s_seq[ns++] = (unsigned short)(sym | extra << 8); ++s_clfreq[sym]; };
        for (uint32_t i = 0; i < N;) {
            const uint32_t v = i < hlit ? s_len[i] : dlen;
            uint32_t r = 1;
            while (i + r < N && (i + r < hlit ? s_len[i + r] : dlen) == v) ++r;
            i += r;
            if (v == 0) {
                while (r >= 11u) { const uint32_t k = min(r, 138u); emit(18u, k - 11u); r -= k; }
                if (r >= 3u) { emit(17u, r - 3u); r = 0; }
                for (; r; --r) emit(0u, 0u);
            } else {
                emit(v, 0u); --r;
                while (r >= 3u) { const uint32_t k = min(r, 6u); emit(16u, k - 3u); r -= k; }
                for (; r; --r) emit(v, 0u);
            }
        }
        s_misc[kNseq] = ns; s_misc[kHlit] = hlit;
    }
    __syncthreads();
    build_lengths(s_clfreq, kClSyms, 7u, s_cllen, T);
    canonical_codes(s_cllen, kClSyms, s_clcode, T);
    if (t == 0) {
        uint32_t hclen = kClSyms;
        while (hclen > 4u && s_cllen[g_cl_order[hclen - 1u]] == 0) --hclen;
        uint32_t bits = 3u + 14u + 3u * hclen + 2u * s_clfreq[16] + 3u * s_clfreq[17] + 7u * s_clfreq[18];
        for (uint32_t s = 0; s < kClSyms; ++s) bits += s_clfreq[s] * s_cllen[s];
        s_misc[kHdrBits] = bits; s_misc[kHclen] = hclen;
    }

    // pass B: the bits of every lane's tokens, and their prefix sum
    const uint32_t from = lo + lead;
    CountSink cs = {s_code, 0};
    if (started) {
        Tok tb = {-1, 0};
        for_bytes(sp, from, hi, [&](uint32_t, uint32_t b) { step(tb, b, cs); });
        flush_run(tail, tb.prev, cs);
    }
    const uint32_t mybits = cs.bits, lane = t & 63u, wv = t >> 6;
    uint32_t incl = wave_incl_scan(mybits, lane);
    if (lane == 63u) s_wsum[wv] = incl;
    __syncthreads();
    for (uint32_t k = 0; k < wv; ++k) incl += s_wsum[k];
    const uint32_t D = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    const uint32_t hdr = s_misc[kHdrBits], eob = s_code[256] >> 16;
    const uint32_t Tdyn = hdr + D + eob;                                 // (at most 15 bits a byte and a header below 3000: no overflow)
    // behind a dynamic block that is not the last: an empty stored block — three header bits, padding to a byte, 00 00 FF FF
    const uint32_t dynbytes = last ? (Tdyn + 7u) / 8u : (Tdyn + 3u + 7u) / 8u + 4u;
    const bool dynamic = dynbytes < n + 5u;
    const uint32_t outbytes = dynamic ? dynbytes : n + 5u, outwords = (outbytes + 3u) / 4u;
    for (uint32_t i = t; i <= outwords; i += 256u) s_bits[i] = 0;
    __syncthreads();

    if (dynamic) {
        if (t == 0) {
            Bits b = bits_at(s_bits, 0);
            const uint32_t hclen = s_misc[kHclen], ns = s_misc[kNseq];
            b.put(last ? 1u : 0u, 1u); b.put(2u, 2u);
            b.put(s_misc[kHlit] - 257u, 5u); b.put(0u, 5u); b.put(hclen - 4u, 4u);
            for (uint32_t i = 0; i < hclen; ++i) b.put(s_cllen[g_cl_order[i]], 3u);
            for (uint32_t i = 0; i < ns; ++i) {
                const uint32_t e = s_seq[i], sym = e & 0xffu, c = s_clcode[sym];
                b.put(c & 0xffffu, c >> 16);
                if (sym >= 16u) b.put(e >> 8, sym == 16u ? 2u : sym == 17u ? 3u : 7u);
            }
            b.flush();
            Bits e = bits_at(s_bits, hdr + D);
            e.put(s_code[256] & 0xffffu, eob);
            e.flush();
            if (!last)                                                     // NLEN of the empty stored block (a word that tokens may share)
                for (uint32_t pos = dynbytes - 2u; pos < dynbytes; ++pos) atomicOr(&s_bits[pos >> 2], 0xffu << (8u * (pos & 3u)));
        }
        if (started) {
            EmitSink es = {s_code, bits_at(s_bits, hdr + incl - mybits)};
            Tok tc = {-1, 0};
            for_bytes(sp, from, hi, [&](uint32_t, uint32_t b) { step(tc, b, es); });
            flush_run(tail, tc.prev, es);
            es.b.flush();
        }
    } else {
        unsigned char *bytes = (unsigned char *)s_bits;
        if (t == 0) {
            bytes[0] = last ? 1 : 0;
            bytes[1] = (unsigned char)n; bytes[2] = (unsigned char)(n >> 8);
            bytes[3] = (unsigned char)~n; bytes[4] = (unsigned char)(~n >> 8);
        }
        for (uint32_t i = t; i < n; i += 256u) bytes[5u + i] = sp[i];
    }
    __syncthreads();
    uint32_t *dst = (uint32_t *)(segbuf + (size_t)it * stride);
    for (uint32_t i = t; i < outwords; i += 256u) dst[i] = s_bits[i];
    if (t == 0) {
        lens[it] = outbytes;
        adl[it] = (1u + s_misc[kSum1]) % kAdlerMod | ((n + s_misc[kSum2]) % kAdlerMod) << 16;
    }
}

// ---- where the segments go ---------------------------------------------------------------------------------------------
// IDAT i holds segment i; the first also the two bytes of the zlib header, the last also the Adler-32.  offs[i] = where IDAT i starts in
// the file; info's own word is the file's Adler-32.  The record and the signature + IHDR go to `out`.
// form (kPngFile, kApngIdat, kApngFdat; wave-uniform): a frame block has no header and no IEND, its record's fourth word is the number
// of chunks, and an fdAT is 4 bytes longer than the IDAT of the same segment.
enum : uint32_t { kPngFile = 0, kApngIdat = 1, kApngFdat = 2 };
__device__ __forceinline__ uint32_t idat_data_bytes(uint32_t len, uint32_t i, uint32_t nseg) { return len + (i == 0 ? 2u : 0u) + (i + 1u == nseg ? 4u : 0u); }

__global__ void __launch_bounds__(1024)
k_png_scan(const uint32_t *__restrict__ lens, const uint32_t *__restrict__ adl, uint32_t nseg, uint32_t seg, uint32_t F,
           u64 *__restrict__ offs, uint32_t *__restrict__ info, unsigned char *__restrict__ out, u64 cap, PngHeaderArg hdr, uint32_t form)
{
    __shared__ u64 s_sum[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t frame = 12u + (form == kApngFdat ? 4u : 0u), front = form == kPngFile ? FL_PNG_HEADER_BYTES : 0u;
    const auto len = [&](uint32_t i) { return frame + idat_data_bytes(lens[i], i, nseg); };
    const Placement p = place_pieces(s_sum, nseg, t, (u64)front, len);
    store_offsets(offs, p, len);
    uint32_t A = 1u, B = 0u;
    if (t == 0) {
        // Adler-32 of a concatenation: a = a1 + a2 - 1, b = b1 + b2 + len2 * (a1 - 1), mod 65521
        for (uint32_t i = 0; i < nseg; ++i) {
            const uint32_t a2 = adl[i] & 0xffffu, b2 = adl[i] >> 16, len2 = i + 1u == nseg ? F - i * seg : seg;
            B = (uint32_t)((B + b2 + (u64)(len2 % kAdlerMod) * ((A + kAdlerMod - 1u) % kAdlerMod)) % kAdlerMod);
            A = (A + a2 + kAdlerMod - 1u) % kAdlerMod;
        }
    }
    // bytes behind the record, IEND included where there is one
    finish_placement(info, out, (u64)front + p.total + (form == kPngFile ? 12u : 0u), cap, seg, B << 16 | A, t);
    if (form == kPngFile) {
        if (t < FL_PNG_HEADER_BYTES) out[16u + t] = hdr.b[t];              // (cap >= 16 + the header: the callers checked)
    } else if (t >= 12u && t < 16u) out[t] = (unsigned char)(nseg >> (8u * (t - 12u)));      // (the thread that stored the record's zero there)
}

// ---- the finished chunks ---------------------------------------------------------------------------------------------
// a * b mod the CRC-32 polynomial, both in the reflected form the CRC register has (bit 31 = x^0)
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll 4
    for (uint32_t i = 0; i < 32u; ++i) {
        p ^= a & 0x80000000u >> i ? b : 0u;
        b = b & 1u ? b >> 1 ^ kCrcPoly : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t crc_pow(uint32_t x, uint32_t e)
{
    uint32_t r = 0x80000000u;                                 // 1
    for (; e; e >>= 1) { if (e & 1u) r = crc_mul(r, x); x = crc_mul(x, x); }
    return r;
}

// One workgroup per segment: length, "IDAT", the bytes, the CRC-32 (and IEND behind the last) assembled in LDS and stored at
// out + 16 + offs[it].  form kApngFdat: the tag is "fdAT", seq + it (most significant byte first) stands between the tag and the data,
// the length field and the CRC take those 4 bytes in; neither frame-block form has an IEND.
// The CRC: with a register that starts at zero the CRC is linear in the message and blind to leading zero bytes, so every lane takes
// an equal share of the (front-padded) message and the shares combine as sum of crc_k * x^(8 * bytes behind share k).  The initial 0xFFFFFFFF is the first four bytes — the tag — inverted; the final inversion is applied at the end.
// Dynamic LDS: seg + 5 + 38 + 4 bytes, rounded up to words, and 2 words of padding.
__global__ void __launch_bounds__(256)
k_png_gather(const unsigned char *__restrict__ segbuf, uint32_t stride, const uint32_t *__restrict__ lens, const u64 *__restrict__ offs,
             const uint32_t *__restrict__ info, uint32_t nseg, unsigned char *__restrict__ out, uint32_t form, uint32_t seq)
{
    extern __shared__ uint32_t s_mem[];
    __shared__ uint32_t s_tab[256], s_crc;
    unsigned char *s_chunk = (unsigned char *)s_mem;
    const uint32_t t = threadIdx.x, it = blockIdx.x;
    if (info[kInfoStatus]) return;
    const bool first = it == 0, last = it + 1u == nseg;
    const bool fdat = form == kApngFdat, iend = last && form == kPngFile;
    const uint32_t L = lens[it], dlen = idat_data_bytes(L, it, nseg), sq = fdat ? 4u : 0u, data = 8u + sq;
    {
        uint32_t c = t;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = c & 1u ? c >> 1 ^ kCrcPoly : c >> 1;
        s_tab[t] = c;
    }
    if (t == 0) {
        s_crc = 0;
        const uint32_t clen = dlen + sq, no = seq + it;       // the chunk's length field; an fdAT's sequence number
        for (uint32_t i = 0; i < 4u; ++i) s_chunk[i] = (unsigned char)(clen >> (24u - 8u * i));
        const uint32_t tag = fdat ? 0x54416466u : 0x54414449u;               // "fdAT", "IDAT"
        for (uint32_t i = 0; i < 4u; ++i) s_chunk[4u + i] = (unsigned char)(tag >> (8u * i));
        if (fdat) for (uint32_t i = 0; i < 4u; ++i) s_chunk[8u + i] = (unsigned char)(no >> (24u - 8u * i));
        if (iend) {
            const unsigned char tail[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
            for (uint32_t i = 0; i < 12u; ++i) s_chunk[12u + dlen + i] = tail[i];
        }
    }
    // the segment, behind the zlib header in the first chunk and in front of the file's Adler-32 in the last
    stage_block(s_chunk + data, (const uint32_t *)(segbuf + (size_t)it * stride), L, t, first, last ? info + kInfoExtra : nullptr);
    __syncthreads();
    // the CRC of tag (+ sequence number) + data: M bytes from s_chunk + 4, padded in front to 256 shares of S
    const uint32_t M = 4u + sq + dlen, S = (M + 255u) / 256u, pad = 256u * S - M;
    uint32_t crc = 0;
    for (uint32_t v = t * S; v < (t + 1u) * S; ++v) {
        if (v < pad) continue;
        const uint32_t m = v - pad, byte = s_chunk[4u + m] ^ (m < 4u ? 0xffu : 0u);
        crc = s_tab[(crc ^ byte) & 0xffu] ^ crc >> 8;
    }
    const uint32_t xs = crc_pow(0x00800000u, S);              // x^(8 S)
    crc = crc_mul(crc, crc_pow(xs, 255u - t));
    if (crc) atomicXor(&s_crc, crc);
    __syncthreads();
    if (t < 4u) s_chunk[data + dlen + t] = (unsigned char)(~s_crc >> (24u - 8u * t));
    __syncthreads();
    store_bytes<256>(out + 16u + offs[it], s_mem, data + 4u + dlen + (iend ? 12u : 0u), t);      // (s_chunk, with the 2 words of padding behind it)
}

uint32_t crc32_host(const unsigned char *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = c & 1u ? c >> 1 ^ kCrcPoly : c >> 1;
    }
    return ~c;
}
void put32(unsigned char *&p, uint32_t v) { *p++ = (unsigned char)(v >> 24); *p++ = (unsigned char)(v >> 16); *p++ = (unsigned char)(v >> 8); *p++ = (unsigned char)v; }

} // namespace

uint32_t png_segment_bytes()
{
    static const uint32_t seg = [] {
        uint32_t v = FL_PNG_SEG;
        if (const char *e = getenv("FLAME_PNG_SEG")) { const long x = atol(e); if (x >= 8192 && x <= 32768) v = (uint32_t)x & ~15u; }
        return v;
    }();
    return seg;
}

PngLayout png_layout(uint32_t w, uint32_t h, int channels, uint32_t seg, int bits, unsigned flags)
{
    PngLayout l;
    l.rowlen = 1u + w * (uint32_t)(channels * bits / 8);
    l.F = (uint64_t)l.rowlen * h;
    l.nseg = (uint32_t)((l.F + seg - 1u) / seg);
    l.stride = seg + 16u;                                     // a stored segment is seg + 5 bytes; rows of the scratch stay 16-byte aligned
    l.per = 16u * ((seg + 4095u) / 4096u);
    // words: the filtered stream (read in 16-byte pieces) | the coded segments | offsets (u64) | lengths | Adler parts | info | the rows' filter types (FL_PNG_ADAPTIVE)
    l.filt = 0;
    l.segbuf = l.filt + (size_t)((l.F + 15u) / 16u) * 4u + 4u;
    l.offs = l.segbuf + (size_t)l.nseg * (l.stride / 4u);
    l.offs += l.offs & 1u;
    l.lens = l.offs + 2u * (size_t)l.nseg;
    l.adl = l.lens + l.nseg;
    l.info = l.adl + l.nseg;
    l.types = l.info + 4u;
    l.words = l.types + (flags & FL_PNG_ADAPTIVE ? (h + 3u) / 4u : 0u);
    return l;
}

// The filter stage with FL_PNG_ADAPTIVE: the choice of every row's type, then the filter that reads it.
template <int CH, int BITS>
static void launch_png_adaptive(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, const PngLayout &l, dim3 fgrid,
                                unsigned char *types, uint32_t *filt)
{
    hipLaunchKernelGGL((k_png_choose<CH, BITS>), dim3(h), dim3(256), 0, st, src, w, types);
    hipLaunchKernelGGL((k_png_filter_x<CH, BITS, true>), fgrid, dim3(256), 0, st, src, w, l.rowlen, (uint32_t)l.F, (const unsigned char *)types, filt);
}

// The file (form kPngFile) or one frame's block of an APNG (kApngIdat; kApngFdat with the first chunk's sequence number)
static void launch_png_form(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int channels, int bits, unsigned flags, uint32_t seg,
                            uint32_t *scratch, unsigned char *out, size_t cap, uint32_t form, uint32_t seq)
{
    const PngLayout l = png_layout(w, h, channels, seg, bits, flags);
    const uint32_t F = (uint32_t)l.F;                         // (the callers refuse frames whose stream passes 2^32 - 1 bytes)
    uint32_t *filt = scratch + l.filt, *lens = scratch + l.lens, *adl = scratch + l.adl, *info = scratch + l.info;
    unsigned char *segbuf = (unsigned char *)(scratch + l.segbuf), *types = (unsigned char *)(scratch + l.types);
    u64 *offs = (u64 *)(scratch + l.offs);
    const bool adaptive = flags & FL_PNG_ADAPTIVE;
    PngHeaderArg hdr = {};
    unsigned char *p = hdr.b;
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (const unsigned char c : sig) *p++ = c;
    put32(p, 13);
    unsigned char *ihdr = p;
    for (const unsigned char c : {'I', 'H', 'D', 'R'}) *p++ = c;
    put32(p, w); put32(p, h);
    *p++ = (unsigned char)bits; *p++ = channels == 4 ? 6 : 2; *p++ = 0; *p++ = 0; *p++ = 0;      // 8 or 16 bit, truecolour (with alpha), deflate, adaptive filtering, not interlaced
    put32(p, crc32_host(ihdr, 17));
    static_assert(FL_PNG_HEADER_BYTES == 8 + 12 + 13, "header layout");
    const uint32_t nthreads4 = (uint32_t)((l.F + 3u) / 4u);
    const dim3 fgrid((nthreads4 + 255u) / 256u);
    if (adaptive) {
        if (bits == 8 && channels == 4) launch_png_adaptive<4, 8>(st, src, w, h, l, fgrid, types, filt);
        else if (bits == 8) launch_png_adaptive<3, 8>(st, src, w, h, l, fgrid, types, filt);
        else if (channels == 4) launch_png_adaptive<4, 16>(st, src, w, h, l, fgrid, types, filt);
        else launch_png_adaptive<3, 16>(st, src, w, h, l, fgrid, types, filt);
    } else if (bits == 8) {                                   // the form every file had before there were others: its own kernels
        if (channels == 4) hipLaunchKernelGGL(k_png_filter<4>, fgrid, dim3(256), 0, st, src, w, l.rowlen, F, filt);
        else hipLaunchKernelGGL(k_png_filter<3>, fgrid, dim3(256), 0, st, src, w, l.rowlen, F, filt);
    } else {
        if (channels == 4) hipLaunchKernelGGL((k_png_filter_x<4, 16, false>), fgrid, dim3(256), 0, st, src, w, l.rowlen, F, (const unsigned char *)nullptr, filt);
        else hipLaunchKernelGGL((k_png_filter_x<3, 16, false>), fgrid, dim3(256), 0, st, src, w, l.rowlen, F, (const unsigned char *)nullptr, filt);
    }
    hipLaunchKernelGGL(k_png_segment<false>, dim3(l.nseg), dim3(256), 4 * (size_t)((seg + 8u) / 4u + 2u), st, (const unsigned char *)filt, F, seg,
                       l.nseg, l.per, segbuf, l.stride, lens, adl);
    hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(1024), 0, st, lens, adl, l.nseg, seg, F, offs, info, out, (u64)cap, hdr, form);
    hipLaunchKernelGGL(k_png_gather, dim3(l.nseg), dim3(256), 4 * (size_t)((seg + 5u + 38u + 4u + 3u) / 4u + 2u), st, segbuf, l.stride, lens, offs, info,
                       l.nseg, out, form, seq);
}

void launch_png_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int channels, int bits, unsigned flags, uint32_t seg,
                       uint32_t *scratch, unsigned char *out, size_t cap)
{
    launch_png_form(st, src, w, h, channels, bits, flags, seg, scratch, out, cap, kPngFile, 0u);
}

void launch_apng_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int channels, int bits, unsigned flags, uint32_t seg,
                        uint32_t seq, uint32_t *scratch, unsigned char *out, size_t cap)
{
    launch_png_form(st, src, w, h, channels, bits, flags, seg, scratch, out, cap, seq == FL_APNG_IDAT ? kApngIdat : kApngFdat, seq);
}

void launch_deflate_tiles(hipStream_t st, const unsigned char *bytes, uint32_t tile_bytes, uint32_t ntiles, unsigned char *segbuf, uint32_t stride,
                          uint32_t *lens, uint32_t *adl)
{
    hipLaunchKernelGGL(k_png_segment<true>, dim3(ntiles), dim3(256), 4 * (size_t)((tile_bytes + 8u) / 4u + 2u), st, bytes, ntiles * tile_bytes, tile_bytes,
                       ntiles, 16u * ((tile_bytes + 4095u) / 4096u), segbuf, stride, lens, adl);
}

void launch_deflate_pieces(hipStream_t st, const unsigned char *bytes, uint32_t tile_bytes, uint32_t ntiles, unsigned char *segbuf, uint32_t stride,
                           uint32_t *lens, uint32_t *adl)
{
    hipLaunchKernelGGL((k_png_segment<true, true>), dim3(ntiles), dim3(256), 4 * (size_t)((tile_bytes + 8u) / 4u + 2u), st, bytes, 0u, tile_bytes,
                       ntiles, 16u * ((tile_bytes + 4095u) / 4096u), segbuf, stride, lens, adl);
}
