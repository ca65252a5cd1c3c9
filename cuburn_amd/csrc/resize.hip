// resize.hip — Lanczos downscale of the float frame to an arbitrary smaller size (fl_resize).
//
// The source is the picture area (w x h, FL_GUTTER bins in) of the buffer laid out for w x h; the result is the whole padded
// buffer of a w2 x h2 frame.  The filter is separable, x then y, and arrives as two tables: output i of an axis is the sum of
// nt source samples from first[i] on, weighted by row i of taps[..][nt].  fl_resize has checked 0 <= first[i] and
// first[i] + nt <= n_in for every row, so neither kernel tests a source coordinate: the gutter and the padding are never read.
//
// Two kernels and the scratch buffer `side`, which holds the h source rows brought down to w2 columns (laid out with the
// result's stride, FL_GUTTER columns in, so that the second kernel's runs start where the result's do):
//   k_resize_rows  a workgroup takes RZ_XSEG consecutive output columns of RZ_XROWS source rows.  Every output column has its own
//                  phase, so its weights differ from lane to lane: the RZ_XSEG tap rows are one contiguous piece of the table, loaded
//                  once per workgroup into LDS, transposed (tap-major: a wave reads 64 consecutive words).  A wave then takes one
//                  source row at a time: it stages the span of source bins its 64 outputs see (one run of float4; at most
//                  RZ_XSPAN bins, which fl_resize has checked with resize_rows_fit) in its own part of LDS, and every lane sums its nxt
//                  products: behind the one barrier that makes the tap rows whole, the waves do not wait for one another.
//   k_resize_cols  a workgroup takes a strip of RZ_CW padded columns and RZ_CH padded rows of the result, RZ_CK consecutive rows
//                  per wave.  The rows of `side` its outputs see go through LDS in bands of RZ_CB rows, each read from memory once
//                  per workgroup and used by every output row whose window holds it.  Which tap a band row meets is wave-uniform
//                  (scalar compares, weights by scalar loads from the table).  Bins outside the picture area are stored as +0.
// Fixed summation order (ascending source coordinate), no atomics: two runs give the same bits.
#include <algorithm>
#include "kernels.h"

#define RZ_XSEG FL_RESIZE_XSEG           // rows pass: output columns per workgroup = one wave's lanes
#define RZ_XSPAN FL_RESIZE_XSPAN         // ... and the source bins they may span
#define RZ_XWAVES 4
#define RZ_XRPW 4                        // source rows per wave
#define RZ_XROWS (RZ_XWAVES * RZ_XRPW)   // source rows per workgroup
#define RZ_CW 64                         // columns pass: strip width = one wave
#define RZ_CK 4                          // output rows per wave
#define RZ_CWAVES 4
#define RZ_CH (RZ_CK * RZ_CWAVES)        // output rows per workgroup (the padded height is a multiple of 16)
#define RZ_CB 16                         // source rows per LDS band

__device__ __forceinline__ void rz_fma(float4 &a, float t, const float4 &v) {
    a.x = fmaf(t, v.x, a.x); a.y = fmaf(t, v.y, a.y); a.z = fmaf(t, v.z, a.z); a.w = fmaf(t, v.w, a.w);
}

// what one lane of a wave wrote to LDS, every lane of that wave may read behind this (binned.hip's wave_sync)
__device__ __forceinline__ void rz_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(RZ_XSEG * RZ_XWAVES)
k_resize_rows(fl_dim din, int w2, int sstride, float4 *__restrict__ side, const float4 *__restrict__ src,
              const int32_t *__restrict__ xfirst, const float *__restrict__ xtaps, int nxt)
{
    __shared__ float wl[FL_RESIZE_MAX_TAPS][RZ_XSEG];          // wl[i][c]: tap i of output column X0 + c
    __shared__ float4 e[RZ_XWAVES][RZ_XSPAN];
    const int lane = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int X0 = blockIdx.x * RZ_XSEG, X = X0 + lane;
    const bool okx = X < w2;
    const int ncol = min(RZ_XSEG, w2 - X0);
    const float *tp = xtaps + (size_t)X0 * (size_t)nxt;
    for (int idx = wv * RZ_XSEG + lane; idx < ncol * nxt; idx += RZ_XSEG * RZ_XWAVES) {
        const int c = idx / nxt;
        wl[idx - c * nxt][c] = tp[idx];
    }
    // the span of source bins the wave's outputs see: [s0, s0 + span)
    const int fx = okx ? xfirst[X] : 0;
    int lo = okx ? fx : 0x7fffffff, hi = okx ? fx : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { lo = min(lo, __shfl_xor(lo, m)); hi = max(hi, __shfl_xor(hi, m)); }
    const int s0 = __builtin_amdgcn_readfirstlane(lo);
    const int span = min(__builtin_amdgcn_readfirstlane(hi) + nxt - s0, RZ_XSPAN);
    const float4 *mine = &e[wv][okx ? fx - s0 : 0];
    const size_t sw = din.astride;
    __syncthreads();                                 // wl is whole; from here on a wave works on its own part of e
#pragma unroll 1
    for (int q = 0; q < RZ_XRPW; ++q) {
        const int y = blockIdx.y * RZ_XROWS + RZ_XWAVES * q + wv;
        if (y >= (int)din.h) break;                  // (wave-uniform)
        const float4 *rp = src + (size_t)(FL_GUTTER + y) * sw + (size_t)(FL_GUTTER + s0);
        rz_wave_sync();                              // the row before this one has been read
        for (int k = lane; k < span; k += RZ_XSEG) e[wv][k] = rp[k];
        rz_wave_sync();
        if (!okx) continue;
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
        for (int i = 0; i < nxt; ++i) rz_fma(acc, wl[i][lane], mine[i]);
        side[(size_t)y * (size_t)sstride + (size_t)(FL_GUTTER + X)] = acc;
    }
}

__global__ void __launch_bounds__(RZ_CW * RZ_CWAVES)
k_resize_cols(fl_dim dout, int hsrc, float4 *__restrict__ dst, const float4 *__restrict__ side,
              const int32_t *__restrict__ yfirst, const float *__restrict__ ytaps, int nyt)
{
    __shared__ float4 band[RZ_CB][RZ_CW];
    const int lane = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int sw = (int)dout.astride, h2 = (int)dout.h;
    const int cx = blockIdx.x * RZ_CW + lane;                                    // padded column
    const bool inbuf = cx < sw, okc = cx >= FL_GUTTER && cx < FL_GUTTER + (int)dout.w;
    const int py0 = blockIdx.y * RZ_CH;                                          // first padded row of the workgroup
    // the rows of `side` the workgroup's output rows see: [lo, hi)
    int lo = 0x7fffffff, hi = 0;
    for (int r = 0; r < RZ_CH; ++r) {
        const int Y = py0 + r - FL_GUTTER;
        if (Y >= 0 && Y < h2) { const int f = yfirst[Y]; lo = min(lo, f); hi = max(hi, f + nyt); }
    }
    hi = min(hi, hsrc);                              // (fl_resize has checked the table: this changes nothing)
    int fo[RZ_CK];                                   // first source row of the wave's output row o; a row outside the picture sees none
    const float *to[RZ_CK];
    float4 acc[RZ_CK];
#pragma unroll
    for (int o = 0; o < RZ_CK; ++o) {
        const int Y = py0 + RZ_CK * wv + o - FL_GUTTER;
        const bool oky = Y >= 0 && Y < h2;
        fo[o] = oky ? yfirst[Y] : 0x40000000;
        to[o] = ytaps + (size_t)(oky ? Y : 0) * (size_t)nyt;
        acc[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    for (int sy0 = lo; sy0 < hi; sy0 += RZ_CB) {
        __syncthreads();                             // the band before this one has been read
#pragma unroll
        for (int q = 0; q < RZ_CB / RZ_CWAVES; ++q) {
            const int r = wv + RZ_CWAVES * q, sy = sy0 + r;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (sy < hi && okc) v = side[(size_t)sy * (size_t)sw + (size_t)cx];
            band[r][lane] = v;
        }
        __syncthreads();
        const int nr = min(RZ_CB, hi - sy0);
        for (int r = 0; r < nr; ++r) {
            const float4 v = band[r][lane];
#pragma unroll
            for (int o = 0; o < RZ_CK; ++o) {
                const int j = sy0 + r - fo[o];       // the tap through which output row o sees this row
                if (j >= 0 && j < nyt) rz_fma(acc[o], to[o][j], v);
            }
        }
    }
    if (!inbuf) return;
#pragma unroll
    for (int o = 0; o < RZ_CK; ++o) {
        const int py = py0 + RZ_CK * wv + o;
        if (py >= (int)dout.ah) break;
        const bool oky = py >= FL_GUTTER && py < FL_GUTTER + h2;
        dst[(size_t)py * (size_t)sw + (size_t)cx] = oky && okc ? acc[o] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

bool resize_rows_fit(const int32_t *xfirst, uint32_t w2, uint32_t nxt)
{
    for (uint32_t X0 = 0; X0 < w2; X0 += RZ_XSEG) {
        int32_t lo = xfirst[X0], hi = xfirst[X0];
        for (uint32_t X = X0; X < w2 && X < X0 + RZ_XSEG; ++X) { lo = std::min(lo, xfirst[X]); hi = std::max(hi, xfirst[X]); }
        if ((int64_t)hi + (int64_t)nxt - (int64_t)lo > RZ_XSPAN) return false;
    }
    return true;
}

void launch_resize(hipStream_t st, fl_dim din, fl_dim dout, float4 *dst, float4 *side, const float4 *src,
                   const int32_t *xfirst, const float *xtaps, int nxt, const int32_t *yfirst, const float *ytaps, int nyt)
{
    const dim3 grows((dout.w + RZ_XSEG - 1) / RZ_XSEG, (din.h + RZ_XROWS - 1) / RZ_XROWS), brows(RZ_XSEG, RZ_XWAVES);
    hipLaunchKernelGGL(k_resize_rows, grows, brows, 0, st, din, (int)dout.w, (int)dout.astride, side, src, xfirst, xtaps, nxt);
    const dim3 gcols((dout.astride + RZ_CW - 1) / RZ_CW, (dout.ah + RZ_CH - 1) / RZ_CH), bcols(RZ_CW, RZ_CWAVES);
    hipLaunchKernelGGL(k_resize_cols, gcols, bcols, 0, st, dout, (int)din.h, dst, (const float4 *)side, yfirst, ytaps, nyt);
}
