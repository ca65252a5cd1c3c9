// de_adaptive.hip — flam3-style adaptive density estimation (the `de` filter, FL_FILT_DE).
//
// A bin q of density w_q > 0 is spread over the integer offsets of a disc of radius
// h_q = clamp(R * max(w_q, 1)^-curve, Rmin, R), rounded to 1/16 px, with the weights
// exp(-4.5 d^2 / h_q^2) / S(h_q) (S: the same sum over the same disc, so each bin keeps its energy);
// bins with h_q < 1 or w_q <= 0 stay where they are.  DESIGN.md §4 "Adaptive density estimation"
// holds the contract and the budget arithmetic.
//
// Two kernels over tiles of 64 x 16 bins (one wave per 64-bin row strip of four rows):
//   k_de_stage   per source bin: the colour premultiplied by 1/S(h) and the exponent coefficient
//                a = -4.5 log2(e) / h^2 (pass-through bins: the colour as it is and a = kPass), and per
//                tile the largest 16h of its bins;
//   k_de_gather  per output tile: the largest 16h among the tiles whose bins can reach it; none >= 16
//                (h >= 1): the tile is left as it is (the filter writes the front buffer in place).
//                Otherwise bands of staged source rows go through LDS and every lane sums, for the four
//                outputs of its column, each source of the disc of that radius: one exponent
//                fma(a, dy^2, a dx^2), a compare against the cut, one v_exp_f32 and four FMAs.
// The gather has no atomics and a fixed summation order: two runs give bit-identical output.
#include "flame_device.h"
#include "kernels.h"
#include <cmath>
#include <vector>

#define DEA_TW 64                 // tile width = one wave
#define DEA_TH 16                 // tile height = four waves of four rows
#define DEA_RB 4                  // source rows per LDS band (8: 10 % slower, fewer workgroups per CU)
#define DEA_MAXW (DEA_TW + 2 * FL_DE_MAX_RADIUS)     // staged columns at the largest radius

// log2(e) * 4.5 * 256: a = kA / m^2 for m = 16 h
static constexpr float kA = (float)(-4.5 * 1.4426950408889634 * 256.0);
// The disc test i^2 + j^2 <= h^2 is the exponent test e = a (i^2 + j^2) >= -4.5 log2(e).  With
// m = 16 h an integer and n = i^2 + j^2, 256 n - m^2 is never in 1..6 (no square is -1..-6 mod 256),
// so a point outside the disc lies at least 7 / m^2 >= 2.9e-6 (relative) beyond the cut; e carries
// at most ~2.4e-7 of rounding.  A cut 1e-6 beyond -4.5 log2(e) keeps the boundary and nothing past it.
static constexpr float kCut = (float)(-4.5 * 1.4426950408889634 * (1.0 + 1e-6));
// a of a bin that stays where it is: a * 0 = -0 (weight 1 at its own position), a * n for n >= 1 is far below the cut
static constexpr float kPass = -3.0e38f;

__global__ void __launch_bounds__(256)
k_de_stage(fl_dim d, const float4 *__restrict__ in, float4 *__restrict__ sc, float *__restrict__ sa,
           uint32_t *__restrict__ tmax, const float *__restrict__ sinv, float R, float Rmin, float curve)
{
    __shared__ uint32_t smax;
    if (threadIdx.x == 0 && threadIdx.y == 0) smax = 0;
    __syncthreads();
    const int x = blockIdx.x * DEA_TW + threadIdx.x;
    uint32_t mymax = 0;
    if (x < (int)d.astride) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = blockIdx.y * DEA_TH + threadIdx.y * 4 + k;
            const size_t i = (size_t)y * d.astride + x;
            const float4 v = in[i];
            int m = 0;
            if (v.w > 0.0f) {          // in double: the radius, and so which 1/16 it rounds to, is the contract's
                double h = (double)R * pow(fmax((double)v.w, 1.0), -(double)curve);
                h = fmin(fmax(h, (double)Rmin), (double)R);
                m = (int)floor(16.0 * h + 0.5);
            }
            if (m >= 16) {
                const float s = sinv[m];
                sc[i] = make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
                sa[i] = kA / (float)(m * m);
                mymax = max(mymax, (uint32_t)m);
            } else {
                sc[i] = v;
                sa[i] = kPass;
            }
        }
    }
    atomicMax(&smax, mymax);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) tmax[blockIdx.y * gridDim.x + blockIdx.x] = smax;
}

__global__ void __launch_bounds__(256)
k_de_gather(fl_dim d, float4 *__restrict__ out, const float4 *__restrict__ sc, const float *__restrict__ sa,
            const uint32_t *__restrict__ tmax)
{
    __shared__ float4 lc[DEA_RB][DEA_MAXW];
    __shared__ float la[DEA_RB][DEA_MAXW];
    __shared__ uint32_t sreach;
    const int tid = threadIdx.y * DEA_TW + threadIdx.x;
    const int tx = blockIdx.x, ty = blockIdx.y, ntx = gridDim.x, nty = gridDim.y;
    if (tid == 0) sreach = 0;
    __syncthreads();
    // the largest 16h among the source tiles that reach this one: within 96 px that is 5 x 13 tiles; a tile
    // reaches if its largest h covers the gap between the nearest bins of the two tiles
    const int rx = (FL_DE_MAX_RADIUS + DEA_TW - 2) / DEA_TW, ry = (FL_DE_MAX_RADIUS + DEA_TH - 2) / DEA_TH;
    if (tid < (2 * rx + 1) * (2 * ry + 1)) {
        const int ox = tid % (2 * rx + 1) - rx, oy = tid / (2 * rx + 1) - ry;
        const int sx = tx + ox, sy = ty + oy;
        if (sx >= 0 && sx < ntx && sy >= 0 && sy < nty) {
            const uint32_t m = tmax[sy * ntx + sx];
            const int gx = ox == 0 ? 0 : DEA_TW * abs(ox) - (DEA_TW - 1);
            const int gy = oy == 0 ? 0 : DEA_TH * abs(oy) - (DEA_TH - 1);
            if ((uint32_t)(256 * (gx * gx + gy * gy)) <= m * m) atomicMax(&sreach, m);
        }
    }
    __syncthreads();
    const int mt = (int)sreach;
    if (mt < 16) return;               // every bin that reaches the tile stays where it is: the input is the output
    const int Hi = mt >> 4;            // integer offsets within the disc of radius mt / 16
    const int width = DEA_TW + 2 * Hi;
    const int lane = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int tx0 = tx * DEA_TW, ty0 = ty * DEA_TH, ry0 = ty0 + 4 * wv;
    const int c0 = tx0 - Hi;
    float4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);

    for (int sy0 = ty0 - Hi; sy0 <= ty0 + DEA_TH - 1 + Hi; sy0 += DEA_RB) {
        __syncthreads();
        for (int idx = tid; idx < DEA_RB * width; idx += 256) {
            const int r = idx / width, col = idx - r * width;
            const int sy = sy0 + r, sx = c0 + col;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float a = kPass;               // beyond the accumulator: nothing
            if (sy >= 0 && sy < (int)d.ah && sx >= 0 && sx < (int)d.astride) {
                const size_t i = (size_t)sy * d.astride + sx;
                v = sc[i]; a = sa[i];
            }
            lc[r][col] = v; la[r][col] = a;
        }
        __syncthreads();
        for (int r = 0; r < DEA_RB; ++r) {
            const int sy = sy0 + r;
            if (sy < 0 || sy >= (int)d.ah) continue;
            const int dy0 = sy - ry0;          // dy of output row k: dy0 - k
            const int dmin = dy0 < 0 ? -dy0 : (dy0 > 3 ? dy0 - 3 : 0);
            if (dmin > Hi) continue;
            // widest |dx| with dx^2 + dmin^2 <= (mt/16)^2: floor(isqrt(mt^2 - 256 dmin^2) / 16)
            const int X = mt * mt - 256 * dmin * dmin;
            int s = (int)sqrtf((float)X);
            while ((s + 1) * (s + 1) <= X) ++s;
            while (s * s > X) --s;
            const int W = s >> 4;
            float dy2[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) dy2[k] = (float)((dy0 - k) * (dy0 - k));
            const float4 *lrow = &lc[r][lane + Hi];
            const float *arow = &la[r][lane + Hi];
#pragma unroll 2
            for (int dx = -W; dx <= W; ++dx) {
                const float4 c = lrow[dx];
                const float a = arow[dx];
                const float t = a * (float)(dx * dx);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float e = fmaf(a, dy2[k], t);
                    const float wgt = e >= kCut ? __builtin_amdgcn_exp2f(e) : 0.0f;
                    acc[k].x = fmaf(c.x, wgt, acc[k].x);
                    acc[k].y = fmaf(c.y, wgt, acc[k].y);
                    acc[k].z = fmaf(c.z, wgt, acc[k].z);
                    acc[k].w = fmaf(c.w, wgt, acc[k].w);
                }
            }
        }
    }
    const int x = tx0 + lane;
    if (x < (int)d.astride) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[(size_t)(ry0 + k) * d.astride + x] = acc[k];
    }
}

size_t de_adaptive_tiles(fl_dim d) { return (size_t)((d.astride + DEA_TW - 1) / DEA_TW) * (d.ah / DEA_TH); }

void launch_de_adaptive(hipStream_t st, fl_dim d, float4 *buf, float4 *stage_c, float *stage_a, uint32_t *tmax,
                        const float *sinv, float R, float Rmin, float curve)
{
    const dim3 grid((d.astride + DEA_TW - 1) / DEA_TW, d.ah / DEA_TH), block(DEA_TW, 4);
    hipLaunchKernelGGL(k_de_stage, grid, block, 0, st, d, (const float4 *)buf, stage_c, stage_a, tmax, sinv, R, Rmin, curve);
    hipLaunchKernelGGL(k_de_gather, grid, block, 0, st, d, buf, (const float4 *)stage_c, (const float *)stage_a,
                       (const uint32_t *)tmax);
}

// 1 / S(h) for m = 16 h = 0 .. 16 * FL_DE_MAX_RADIUS (entries below 16 unused), in double: S(h) = sum over
// the rows i of the disc of g(i) * (g(0) + 2 sum_{j=1..J(i)} g(j)), g(j) = exp(-4.5 * 256 j^2 / m^2),
// J(i) the largest j with 256 (i^2 + j^2) <= m^2
void de_adaptive_norms(float *out)
{
    const int M = 16 * FL_DE_MAX_RADIUS;
    std::vector<double> g(FL_DE_MAX_RADIUS + 1), pre(FL_DE_MAX_RADIUS + 1);
    for (int m = 0; m <= M; ++m) {
        if (m < 16) { out[m] = 1.0f; continue; }
        const int I = m / 16;
        const double mm = (double)m * m;
        for (int j = 0; j <= I; ++j) g[j] = exp(-4.5 * 256.0 * j * j / mm);
        pre[0] = g[0];
        for (int j = 1; j <= I; ++j) pre[j] = pre[j - 1] + 2.0 * g[j];
        double S = 0.0;
        int J = I;
        for (int i = 0; i <= I; ++i) {         // J(i) falls as i grows
            while (J > 0 && 256LL * (i * i + J * J) > (long long)m * m) --J;
            S += (i == 0 ? 1.0 : 2.0) * g[i] * pre[J];
        }
        out[m] = (float)(1.0 / S);
    }
}
