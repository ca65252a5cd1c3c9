// resample.hip — flam3's spatial filter and the supersample decimation in one pass.
//
// The source is the padded buffer of an (ss*w) x (ss*h) frame, the result that of a w x h frame.  Output bin
// (X, Y) is the n x n separable filter over the source bins from (12 + ss*(X-12) - g, 12 + ss*(Y-12) - g) on,
// g = (n - ss) / 2: the footprint is centred on the ss x ss source bins the output bin covers.  Source bins
// outside the buffer count as zero and are never read.
//
// One workgroup of 256 threads takes a strip of 256 consecutive source columns and RS_TY output rows.  Vertical
// pass first, because it is the one that reads global memory and its loads are whole row segments (4 KB per row
// and workgroup, 16 bytes per lane): each thread walks down the RS_TY * ss + n - ss source rows of its column, RS_UNROLL
// loads in flight, a row's value going into each of the RS_TY column sums whose footprint holds it (which ones is
// wave-uniform: scalar branches, taps by scalar loads from the kernel arguments).  The column sums go to an LDS tile of
// RS_TY x 256; the horizontal pass produces from it the (256 - (n - ss)) / ss output bins per row that the strip
// covers whole, and the next workgroup's strip starts that many output bins further on.
#include "kernels.h"

#ifndef RS_TY
#define RS_TY 8
#endif
#ifndef RS_UNROLL
#define RS_UNROLL 8                      // source rows in flight per lane
#endif
#define RS_COLS 256                      // source columns per workgroup = threads

struct ResampleTaps { float t[FL_RESAMPLE_MAX_TAPS]; };

__device__ __forceinline__ void rs_fma(float4 &a, float t, const float4 &v) {
    a.x = fmaf(t, v.x, a.x); a.y = fmaf(t, v.y, a.y); a.z = fmaf(t, v.z, a.z); a.w = fmaf(t, v.w, a.w);
}

// output bins per row that a strip of RS_COLS source columns covers whole
static inline __host__ __device__ int rs_strip_outputs(int ss, int n) { return (RS_COLS - (n - ss)) / ss; }

template <int SS>
__global__ void __launch_bounds__(256)
k_resample(fl_dim din, fl_dim dout, float4 *__restrict__ dst, const float4 *__restrict__ src, ResampleTaps k, int n) {
    __shared__ float4 cols[RS_TY * RS_COLS];
    const int tid = threadIdx.x;
    const int txe = rs_strip_outputs(SS, n);
    const int X0 = blockIdx.x * txe, Y0 = blockIdx.y * RS_TY;
    const int g = (n - SS) / 2;
    const int sw = (int)din.astride, sh = (int)din.ah;
    const int nrows = RS_TY * SS + n - SS;
    const int sx = FL_GUTTER + SS * (X0 - FL_GUTTER) - g + tid;
    const int syb = FL_GUTTER + SS * (Y0 - FL_GUTTER) - g;
    const bool okx = sx >= 0 && sx < sw;

    float4 acc[RS_TY];
#pragma unroll
    for (int o = 0; o < RS_TY; ++o) acc[o] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // a row outside the buffer (uniform) or a column outside it is not read
    for (int r = 0; r < nrows; r += RS_UNROLL) {
        float4 v[RS_UNROLL];
#pragma unroll
        for (int u = 0; u < RS_UNROLL; ++u) {
            const int sy = syb + r + u;
            v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r + u < nrows && sy >= 0 && sy < sh && okx) v[u] = src[(size_t)sy * (size_t)sw + (size_t)sx];
        }
#pragma unroll
        for (int u = 0; u < RS_UNROLL; ++u)
#pragma unroll
            for (int o = 0; o < RS_TY; ++o) {
                const int j = r + u - SS * o;                // the tap through which output row o sees this row
                if (j >= 0 && j < n) rs_fma(acc[o], k.t[j], v[u]);
            }
    }
#pragma unroll
    for (int o = 0; o < RS_TY; ++o) cols[o * RS_COLS + tid] = acc[o];
    __syncthreads();

    for (int b = tid; b < txe * RS_TY; b += 256) {
        const int ty = b / txe, tx = b - ty * txe;
        const int X = X0 + tx, Y = Y0 + ty;
        if (X >= (int)dout.astride || Y >= (int)dout.ah) continue;
        float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 *row = cols + ty * RS_COLS + SS * tx;   // SS * (txe - 1) + n - 1 < RS_COLS
        for (int i = 0; i < n; ++i) rs_fma(out, k.t[i], row[i]);
        dst[(size_t)Y * dout.astride + X] = out;
    }
}

void launch_resample(hipStream_t st, fl_dim din, fl_dim dout, int ss, float4 *dst, const float4 *src, const float *taps, int ntaps)
{
    ResampleTaps k;
    for (int i = 0; i < FL_RESAMPLE_MAX_TAPS; ++i) k.t[i] = i < ntaps ? taps[i] : 0.0f;
    const int txe = rs_strip_outputs(ss, ntaps);
    const dim3 grid((dout.astride + txe - 1) / txe, (dout.ah + RS_TY - 1) / RS_TY), block(256);
    switch (ss) {
    case 1: hipLaunchKernelGGL(k_resample<1>, grid, block, 0, st, din, dout, dst, src, k, ntaps); break;
    case 2: hipLaunchKernelGGL(k_resample<2>, grid, block, 0, st, din, dout, dst, src, k, ntaps); break;
    case 3: hipLaunchKernelGGL(k_resample<3>, grid, block, 0, st, din, dout, dst, src, k, ntaps); break;
    case 4: hipLaunchKernelGGL(k_resample<4>, grid, block, 0, st, din, dout, dst, src, k, ntaps); break;
    default: break;      // fl_resample has checked ss
    }
}
