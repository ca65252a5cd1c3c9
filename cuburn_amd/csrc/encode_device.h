// encode_device.h — device helpers the still encoders share (jpeg.hip, png.hip).  DESIGN.md §4.8 "What the encoders share".
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

// The 16-byte record in front of every encoded file: u32 min(need, 2^32 - 1), status, param, 0, little-endian, by threads 0..15.
__device__ __forceinline__ void write_record(unsigned char *out, u64 need, uint32_t status, uint32_t param, uint32_t t)
{
    if (t < 16) {
        const uint32_t rec[4] = {need > 0xffffffffull ? 0xffffffffu : (uint32_t)need, status, param, 0u};
        out[t] = (unsigned char)(rec[t >> 2] >> (8u * (t & 3u)));
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
