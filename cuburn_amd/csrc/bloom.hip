// bloom.hip — the `bloom` filter (FL_FILT_BLOOM): a wide Gaussian glare of the light above a threshold.
//
// A bin (r, g, b, w) of the front buffer has the excess E = f * (r, g, b, w), f = (w - t) / w where w > t and 0 elsewhere
// (k_gamma_full_hi's rule with t in place of 1).  E is blurred along x, then along y, with the 2R + 1 symmetric taps the caller
// gives (R <= FL_BLOOM_MAX_REACH), over the whole padded buffer; sources outside it count as zero and are never read.  The
// front buffer then receives in + strength * blur(E) on all four channels.
//
// Two kernels and one scratch buffer of the front buffer's size:
//   k_bloom_rows  a workgroup takes BL_SEG consecutive bins of one row: it stages their excess and R bins of halo per side in
//                 LDS, forming E as it loads, and every lane sums the 2R + 1 taps of its bin from LDS into `side`;
//   k_bloom_cols  a workgroup takes a strip of BL_CW columns (a wave's global access is one run of 1 KiB) and BL_CH output
//                 rows, BL_CK consecutive rows per lane and wave.  The rows of `side` its outputs see, at most BL_CH + 2R of
//                 them (800 at the largest reach: 800 KiB, far beyond one workgroup's LDS), go through LDS in bands of BL_CB
//                 rows; a staged bin feeds the BL_CK sums of its lane from one LDS read.  The sums are added into the front
//                 buffer in place: a lane reads and writes only its own bins.
// Taps are kernel arguments: which tap a source meets is wave-uniform in both kernels, so they arrive by scalar loads.
// A window (rows) or band (columns) whose staged values are all +-0 skips its multiply-adds: every sum starts at +0 and
// fmaf(t, +-0, s) is s for every finite t, so what is stored is what the full loop would store.  A NaN or infinity is not
// zero and takes the full loop.  Fixed summation order, no atomics: two runs give the same bits.
#include "kernels.h"

#define BL_SEG 256                       // rows pass: output bins per workgroup = threads
#define BL_CW 64                         // columns pass: strip width = one wave
#define BL_CK 8                          // output rows per lane
#define BL_CWAVES 4
#define BL_CH (BL_CK * BL_CWAVES)        // output rows per workgroup
#define BL_CB 16                         // source rows per LDS band

struct BloomTaps { float t[2 * FL_BLOOM_MAX_REACH + 1]; };      // t[R + i]: the tap at offset i = -R .. R (3 KiB of kernel arguments)

__device__ __forceinline__ void bl_fma(float4 &a, float t, const float4 &v) {
    a.x = fmaf(t, v.x, a.x); a.y = fmaf(t, v.y, a.y); a.z = fmaf(t, v.z, a.z); a.w = fmaf(t, v.w, a.w);
}
// anything but +-0 in a channel (a NaN counts)
__device__ __forceinline__ int bl_live(const float4 &v) { return !(v.x == 0.0f && v.y == 0.0f && v.z == 0.0f && v.w == 0.0f); }

__global__ void __launch_bounds__(BL_SEG)
k_bloom_rows(fl_dim d, float4 *__restrict__ side, const float4 *__restrict__ in, BloomTaps k, int R, float thr)
{
    __shared__ float4 e[BL_SEG + 2 * FL_BLOOM_MAX_REACH];
    const int tid = threadIdx.x;
    const int sw = (int)d.astride;
    const int x0 = blockIdx.x * BL_SEG;
    const size_t row = (size_t)blockIdx.y * (size_t)sw;
    int live = 0;
    for (int i = tid; i < BL_SEG + 2 * R; i += BL_SEG) {
        const int sx = x0 - R + i;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (sx >= 0 && sx < sw) {
            v = in[row + (size_t)sx];
            const float f = v.w > thr ? (v.w - thr) / v.w : 0.0f;      // (a NaN w: 0)
            v = make_float4(f * v.x, f * v.y, f * v.z, f * v.w);
        }
        e[i] = v;
        live |= bl_live(v);
    }
    const int any = __syncthreads_or(live);
    const int x = x0 + tid;
    if (x >= sw) return;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (any) {
        const float4 *src = e + tid;                 // src[j]: the bin at x - R + j
#pragma unroll 8
        for (int j = 0; j <= 2 * R; ++j) bl_fma(acc, k.t[j], src[j]);
    }
    side[row + (size_t)x] = acc;
}

__global__ void __launch_bounds__(BL_CW * BL_CWAVES)
k_bloom_cols(fl_dim d, float4 *__restrict__ front, const float4 *__restrict__ side, BloomTaps k, int R, float strength)
{
    __shared__ float4 band[BL_CB][BL_CW];
    const int lane = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int sw = (int)d.astride, sh = (int)d.ah;
    const int x = blockIdx.x * BL_CW + lane;
    const bool okx = x < sw;
    const int y0 = blockIdx.y * BL_CH, oy0 = y0 + BL_CK * wv;
    const int lo = max(y0 - R, 0), hi = min(y0 + BL_CH - 1 + R, sh - 1);      // the rows of `side` the workgroup's outputs see
    float4 acc[BL_CK];
#pragma unroll
    for (int o = 0; o < BL_CK; ++o) acc[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    for (int sy0 = lo; sy0 <= hi; sy0 += BL_CB) {
        __syncthreads();                             // the band before this one has been read
        int live = 0;
#pragma unroll
        for (int q = 0; q < BL_CB / BL_CWAVES; ++q) {
            const int r = wv + BL_CWAVES * q, sy = sy0 + r;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (sy <= hi && okx) v = side[(size_t)sy * (size_t)sw + (size_t)x];
            band[r][lane] = v;
            live |= bl_live(v);
        }
        if (!__syncthreads_or(live)) continue;
        const int dy0 = sy0 - oy0;                   // output row o of this wave sees row r of the band through the tap at dy0 + r - o
        if (sy0 + BL_CB - 1 <= hi && dy0 >= BL_CK - 1 - R && dy0 + BL_CB - 1 <= R) {
            // every output of the wave sees every row of the band: BL_CB + BL_CK - 1 consecutive taps, loaded once
            const float *tp = k.t + (R + dy0 - (BL_CK - 1));
            float tt[BL_CB + BL_CK - 1];
#pragma unroll
            for (int i = 0; i < BL_CB + BL_CK - 1; ++i) tt[i] = tp[i];
#pragma unroll
            for (int r = 0; r < BL_CB; ++r) {
                const float4 v = band[r][lane];
#pragma unroll
                for (int o = 0; o < BL_CK; ++o) bl_fma(acc[o], tt[r - o + BL_CK - 1], v);
            }
            continue;
        }
        for (int r = 0; r < BL_CB; ++r) {
            const int dy = dy0 + r;
            if (sy0 + r > hi || dy < -R || dy > R + BL_CK - 1) continue;
            const float4 v = band[r][lane];
#pragma unroll
            for (int o = 0; o < BL_CK; ++o) {
                const int i = dy - o;
                if (i >= -R && i <= R) bl_fma(acc[o], k.t[R + i], v);
            }
        }
    }
    if (!okx) return;
#pragma unroll
    for (int o = 0; o < BL_CK; ++o) {
        const int y = oy0 + o;
        if (y >= sh) break;
        const size_t i = (size_t)y * (size_t)sw + (size_t)x;
        float4 v = front[i];
        bl_fma(v, strength, acc[o]);
        front[i] = v;
    }
}

void launch_bloom(hipStream_t st, fl_dim d, float4 *front, float4 *side, const float *taps, int R, float thr, float strength)
{
    BloomTaps k;
    for (int i = 0; i <= 2 * FL_BLOOM_MAX_REACH; ++i) k.t[i] = i <= 2 * R ? taps[i < R ? R - i : i - R] : 0.0f;
    const dim3 grows((d.astride + BL_SEG - 1) / BL_SEG, d.ah), brows(BL_SEG);
    hipLaunchKernelGGL(k_bloom_rows, grows, brows, 0, st, d, side, (const float4 *)front, k, R, thr);
    const dim3 gcols((d.astride + BL_CW - 1) / BL_CW, (d.ah + BL_CH - 1) / BL_CH), bcols(BL_CW, BL_CWAVES);
    hipLaunchKernelGGL(k_bloom_cols, gcols, bcols, 0, st, d, front, (const float4 *)side, k, R, strength);
}
