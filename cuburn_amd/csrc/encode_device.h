// encode_device.h — device helpers the seven encoders share (jpeg.hip, png.hip and its APNG frame blocks, tiff.hip, exr.hip, gif.hip,
// webp.hip; Motion-JPEG is jpeg.hip's).  DESIGN.md §4.8 "What the encoders share".
#pragma once
#include "kernels.h"

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(v, d, 64); if (lane >= d) v += o; }
    return v;
}

// The placement kernels' scan: one workgroup of 1024 threads, thread t brings `mine`.  Returns the sum of the threads before t;
// `total` = the sum of all.  s_sum holds the inclusive sums afterwards.
__device__ __forceinline__ u64 block_excl_scan_1024(u64 *s_sum, u64 mine, uint32_t t, u64 &total)
{
    s_sum[t] = mine;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const u64 o = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += o;
        __syncthreads();
    }
    total = s_sum[1023];
    return s_sum[t] - mine;
}

// ---- placement: one workgroup of 1024 threads lays n pieces end to end ------------------------------------------------
// Thread t takes the pieces [lo, hi), ceil(n / 1024) consecutive ones; run = where piece lo begins (`front` + the pieces before it);
// total = the sum of all pieces, without `front`.
struct Placement { uint32_t lo, hi; u64 run, total; };

// len(i) = the bytes (or bits) piece i takes.  s_sum: 1024 u64 of LDS.
template <class Len>
__device__ __forceinline__ Placement place_pieces(u64 *s_sum, uint32_t n, uint32_t t, u64 front, Len &&len)
{
    const uint32_t per = (n + 1023u) / 1024u, lo = min(t * per, n), hi = min(lo + per, n);
    u64 mine = 0, total;
    for (uint32_t i = lo; i < hi; ++i) mine += len(i);
    const u64 before = block_excl_scan_1024(s_sum, mine, t, total);
    return {lo, hi, front + before, total};
}

// f(i, where piece i begins) for the thread's pieces; offs[i] = that, in the width of Off (a file below 2^32 bytes keeps u32)
template <class Len, class Fn>
__device__ __forceinline__ void for_placed(Placement p, Len &&len, Fn &&f)
{
    for (uint32_t i = p.lo; i < p.hi; ++i) { f(i, p.run); p.run += len(i); }
}
template <class Off, class Len>
__device__ __forceinline__ void store_offsets(Off *offs, const Placement &p, Len &&len)
{
    for_placed(p, len, [&](uint32_t i, u64 at) { offs[i] = (Off)at; });
}

// What a placement kernel leaves for the kernels behind it, 4 words: the bytes behind the record, whether they do not fit, and one
// word of the encoder's own (png: the file's Adler-32; gif: the stream's bytes; webp: the payload's bytes; else 0).
enum : uint32_t { kInfoNeedLo = 0, kInfoNeedHi = 1, kInfoStatus = 2, kInfoExtra = 3 };

// The 16-byte record in front of every encoded file: u32 min(need, 2^32 - 1), status, param, 0, little-endian, by threads 0..15.
__device__ __forceinline__ void write_record(unsigned char *out, u64 need, uint32_t status, uint32_t param, uint32_t t)
{
    if (t < 16) {
        const uint32_t rec[4] = {need > 0xffffffffull ? 0xffffffffu : (uint32_t)need, status, param, 0u};
        out[t] = (unsigned char)(rec[t >> 2] >> (8u * (t & 3u)));
    }
}

// The end of every placement: status = whether `need` bytes behind the record pass cap; info by thread 0 (which alone needs a valid
// `extra`) and the record.  Returns the status.
__device__ __forceinline__ uint32_t finish_placement(uint32_t *info, unsigned char *out, u64 need, u64 cap, uint32_t param, uint32_t extra, uint32_t t)
{
    const uint32_t status = need > cap - 16u ? 1u : 0u;
    if (t == 0) { info[kInfoNeedLo] = (uint32_t)need; info[kInfoNeedHi] = (uint32_t)(need >> 32); info[kInfoStatus] = status; info[kInfoExtra] = extra; }
    write_record(out, need, status, param, t);
    return status;
}

__device__ __forceinline__ void put_le32(unsigned char *p, uint32_t v)      // (p may have any alignment)
{
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) p[k] = (unsigned char)(v >> (8u * k));
}

// A coded deflate block on its way into a file, by 256 threads: its L bytes from `row` (word aligned, readable through word
// (L - 1) / 4) to the LDS bytes at dst, which may have any alignment.  zhead: the zlib header stands at dst and the block behind it;
// adler (null: none): *adler — a | b << 16, read by thread 0 alone — follows the block, most significant byte first.  No barrier.
__device__ __forceinline__ void stage_block(unsigned char *dst, const uint32_t *row, uint32_t L, uint32_t t, bool zhead, const uint32_t *adler)
{
    unsigned char *body = dst + (zhead ? 2u : 0u);
    if (t == 0) {
        if (zhead) { dst[0] = 0x78; dst[1] = 0x01; }          // zlib: deflate, 32 KiB window, no dictionary, FCHECK
        if (adler) {
            const uint32_t ad = *adler;
            for (uint32_t i = 0; i < 4u; ++i) body[L + i] = (unsigned char)(ad >> (24u - 8u * i));
        }
    }
    for (uint32_t i = t; i < (L + 3u) / 4u; i += 256u) {
        const uint32_t wd = row[i];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) if (4u * i + k < L) body[4u * i + k] = (unsigned char)(wd >> (8u * k));
    }
}

// nbytes from LDS to dst, which may have any alignment, by NTHREADS threads (t the thread's index): bytes up to the first 4-byte
// boundary of dst, dwords funnel-shifted out of two LDS words, and the bytes that are left.  No byte outside [dst, dst + nbytes)
// is stored.  The precondition on the LDS side: lds_words is word aligned and readable one word beyond nbytes, i.e. through
// word nbytes / 4 (the dword loop reads the word behind the one it shifts; the bytes it holds beyond nbytes go nowhere).
template <uint32_t NTHREADS>
__device__ __forceinline__ void store_bytes(unsigned char *dst, const uint32_t *lds_words, uint32_t nbytes, uint32_t t)
{
    const unsigned char *lds_bytes = (const unsigned char *)lds_words;
    const uint32_t head = min(nbytes, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u)), nmid = (nbytes - head) >> 2, tail0 = head + 4u * nmid;
    if (t < head) dst[t] = lds_bytes[t];
    for (uint32_t m = t; m < nmid; m += NTHREADS) {
        const uint32_t so = head + 4u * m, sh = (so & 3u) * 8u;
        const uint32_t a = lds_words[so >> 2], c = lds_words[(so >> 2) + 1u];
        *(uint32_t *)(dst + so) = sh ? a >> sh | c << (32u - sh) : a;
    }
    if (t < nbytes - tail0) dst[tail0 + t] = lds_bytes[tail0 + t];
}

// ---- length-limited Huffman codes, by the whole workgroup (256 threads, nsym <= 288) ----------------------------------
constexpr uint32_t kSymPad = 288u;                            // the largest alphabet (deflate's 286 literal / length symbols), rounded up
struct HuffTmp {
    uint32_t sfreq[kSymPad], nfreq[kSymPad], cnt[32], next[16];
    unsigned short ssym[kSymPad], lpar[kSymPad], npar[kSymPad];
};

// lens[s] = code length of symbol s (0: unused) of a complete prefix code with no length above maxlen, Huffman's where that obeys the
// limit.  A lone used symbol gets a one-bit code and so does an unused neighbour, which keeps the code complete.
static __device__ void build_lengths(const uint32_t *freq, uint32_t nsym, uint32_t maxlen, unsigned char *lens, HuffTmp &T)
{
    const uint32_t t = threadIdx.x;
    uint32_t used = 0;
    for (uint32_t i = t; i < kSymPad; i += 256u) {
        const uint32_t f = i < nsym ? freq[i] : 0u;
        if (i < nsym) lens[i] = 0;
        if (f) {                                              // rank by (frequency, symbol), ascending
            uint32_t r = 0;
#pragma unroll 8
            for (uint32_t j = 0; j < nsym; ++j) { const uint32_t fj = freq[j]; r += fj && (fj < f || (fj == f && j < i)) ? 1u : 0u; }
            T.sfreq[r] = f; T.ssym[r] = (unsigned short)i;
            ++used;
        }
    }
    if (t < 32u) T.cnt[t] = 0;
    const uint32_t n = (uint32_t)__syncthreads_count(used >= 1u) + (uint32_t)__syncthreads_count(used >= 2u);
    if (n == 0) return;
    if (n == 1u) {
        if (t == 0) { const uint32_t s = T.ssym[0]; lens[s] = 1; lens[s ? 0 : 1] = 1; }
        __syncthreads();
        return;
    }
    if (t == 0) {                                             // the two-queue merge: leaves in order, inner nodes in order of creation
        constexpr uint32_t kNone = 0xffffffffu;               // an empty queue (no frequency reaches it)
        uint32_t leaf = 0, node = 0;
        uint32_t lf = T.sfreq[0], lf1 = T.sfreq[1], nf = kNone;      // the queues' heads, and the leaf behind the head: loaded ahead of their use
        for (uint32_t k = 0; k + 1u < n; ++k) {
            uint32_t f = 0;
#pragma unroll
            for (int pick = 0; pick < 2; ++pick) {
                if (lf <= nf) {                               // (a tie takes the leaf)
                    f += lf; T.lpar[leaf++] = (unsigned short)k;
                    lf = lf1; lf1 = leaf + 1u < n ? T.sfreq[leaf + 1u] : kNone;
                } else {
                    f += nf; T.npar[node++] = (unsigned short)k;
                    nf = node < k ? T.nfreq[node] : kNone;
                }
            }
            T.nfreq[k] = f;
            if (node == k) nf = f;                            // the new node is the only one waiting
        }
    }
    __syncthreads();
    for (uint32_t i = t; i < n; i += 256u) {                  // a leaf's depth: the steps from it to the root, node n - 2
        uint32_t d = 1u;
        for (uint32_t k = T.lpar[i]; k != n - 2u; k = T.npar[k]) ++d;
        atomicAdd(&T.cnt[min(d, maxlen)], 1u);
    }
    __syncthreads();
    if (t == 0) {                                             // depths cut at maxlen over-subscribe the code: lengthen until Kraft's sum is 1 again
        uint32_t total = 0;
        for (uint32_t l = 1; l <= maxlen; ++l) total += T.cnt[l] << (maxlen - l);
        while (total > 1u << maxlen) {
            --T.cnt[maxlen];
            for (uint32_t l = maxlen - 1u; l > 0; --l)
                if (T.cnt[l]) { --T.cnt[l]; T.cnt[l + 1u] += 2u; break; }
            --total;
        }
    }
    __syncthreads();
    for (uint32_t i = t; i < n; i += 256u) {                  // the rarest symbols take the longest codes
        uint32_t l = maxlen, above = T.cnt[maxlen];
        while (i >= above && l > 1u) above += T.cnt[--l];
        lens[T.ssym[i]] = (unsigned char)l;
    }
    __syncthreads();
}

// code[s] = the canonical code of RFC 1951 3.2.2, bit-reversed (deflate sends Huffman codes from their most significant bit) | length << 16
static __device__ void canonical_codes(const unsigned char *lens, uint32_t nsym, uint32_t *code, HuffTmp &T)
{
    const uint32_t t = threadIdx.x;
    if (t < 32u) T.cnt[t] = 0;
    __syncthreads();
    for (uint32_t i = t; i < nsym; i += 256u) if (lens[i]) atomicAdd(&T.cnt[lens[i]], 1u);
    __syncthreads();
    if (t == 0) {
        uint32_t c = 0;
        T.next[0] = 0;
        for (uint32_t b = 1; b < 16u; ++b) { c = (c + T.cnt[b - 1u]) << 1; T.next[b] = c; }
    }
    __syncthreads();
    for (uint32_t i = t; i < nsym; i += 256u) {
        const uint32_t l = lens[i];
        uint32_t r = 0;
        if (l) {
#pragma unroll 8
            for (uint32_t j = 0; j < i; ++j) r += lens[j] == l ? 1u : 0u;
        }
        code[i] = l ? __brev(T.next[l] + r) >> (32u - l) | l << 16 : 0u;
    }
    __syncthreads();
}
