// exr.hip — tiled OpenEXR (single part, one level, little-endian; ZIP compression; HALF or FLOAT samples, 3 or 4 channels) from
// f32 [h][stride][4] on the device.  DESIGN.md §4.14.
// Four launches per frame, no host wait between them:
//   k_exr_tiles     one workgroup per tile: the tile's pixels, cropped to the image, -> samples (half: round to nearest even) ->
//                   the raw bytes in LDS (row by row, channel by channel, low byte first) -> the staged stream: even bytes, then
//                   odd bytes, each but the first as the difference to the one before it plus 128; lens[tile] = its bytes
//   k_png_segment   (png.hip, its TILES + LENS form) one workgroup per tile: one final deflate block of lens[tile] bytes, dynamic
//                   or stored, and their Adler-32; lens[tile] = the block's bytes
//   k_exr_scan      one workgroup: every chunk's size (the zlib stream where it is smaller than the tile, the raw bytes where not),
//                   their places and the total; the 16-byte record, the header and the offset table
//   k_exr_gather    one workgroup per tile: the chunk's 20-byte head, then 78 01 + block + Adler-32, or the raw bytes built from
//                   the pixels again, copied to their place
// The staged stream is a kernel of its own, as in tiff.hip, and not folded into the coder's load: the coder reads its bytes three
// times (histogram, count, emit) in 16-byte pieces, and the split puts neighbouring staged bytes two samples apart in the source.
// Nothing is stored at or beyond `cap`: when the file does not fit, the scan stores the record alone and the gather nothing.
#include "kernels.h"
#include "encode_device.h"
#include <cstring>

namespace {

constexpr uint32_t kHeaderMax = 360u;                         // four channels: 359
struct ExrHeaderArg { unsigned char b[kHeaderMax]; uint32_t n; };
struct ExrFrame { uint32_t w, h, stride, nx, nt; };           // the image, the source's pixels per row, tiles per row and in all

template <int PIX> struct Form {
    static constexpr uint32_t BPS = PIX == FL_EXR_FLOAT ? 4u : 2u, TH = PIX == FL_EXR_FLOAT ? FL_EXR_TILE_ROWS_FLOAT : FL_EXR_TILE_ROWS_HALF;
};

// ---- samples -------------------------------------------------------------------------------------------------------
// Round to nearest, ties to even, gradual underflow: the conversion instruction (f16 denormals are never flushed on this target).
// What would round to infinity is the largest finite half instead, NaN is zero.
__device__ __forceinline__ uint32_t half_bits(float x)
{
    if (x != x) return 0u;
    const _Float16 v = (_Float16)x;
    uint32_t hb = __builtin_bit_cast(unsigned short, v);
    if ((hb & 0x7fffu) == 0x7c00u) hb = (hb & 0x8000u) | 0x7bffu;
    return hb;
}

// The tile's raw bytes: th rows of CH runs (A first with four channels, then B, G, R) of tw samples.  raw is word aligned.
template <int CH, int PIX>
__device__ __forceinline__ void fill_raw(uint32_t *raw, const float4 *__restrict__ src, const ExrFrame f, uint32_t tx, uint32_t ty,
                                         uint32_t tw, uint32_t th, uint32_t t)
{
    const float4 *corner = src + (size_t)(ty * Form<PIX>::TH) * f.stride + (size_t)tx * FL_EXR_TILE_WIDTH;
    for (uint32_t q = t; q < tw * th; q += 256u) {
        const uint32_t r = q / tw, x = q - r * tw;
        const float4 p = corner[(size_t)r * f.stride + x];
        const float comp[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (uint32_t k = 0; k < (uint32_t)CH; ++k) {
            const float s = comp[CH - 1 - k];                 // chlist order: alphabetical
            const uint32_t at = (r * CH + k) * tw + x;        // in samples
            if (PIX == FL_EXR_FLOAT) raw[at] = __float_as_uint(s);
            else ((unsigned short *)raw)[at] = (unsigned short)half_bits(s);
        }
    }
}

__device__ __forceinline__ void tile_of(const ExrFrame f, uint32_t it, uint32_t TH, uint32_t &tx, uint32_t &ty, uint32_t &tw, uint32_t &th)
{
    ty = it / f.nx; tx = it - ty * f.nx;
    tw = min(FL_EXR_TILE_WIDTH, f.w - FL_EXR_TILE_WIDTH * tx);
    th = min(TH, f.h - TH * ty);
}

// staged holds nt pieces of 8192 * CH bytes; piece `it` starts with the tile's n = lens[it] predicted bytes.
template <int CH, int PIX>
__global__ void __launch_bounds__(256)
k_exr_tiles(const float4 *__restrict__ src, ExrFrame f, uint32_t *__restrict__ staged, uint32_t *__restrict__ lens)
{
    constexpr uint32_t TILE = 8192u * CH;
    __shared__ uint32_t s_raw[TILE / 4u];
    const uint32_t t = threadIdx.x, it = blockIdx.x;
    uint32_t tx, ty, tw, th;
    tile_of(f, it, Form<PIX>::TH, tx, ty, tw, th);
    const uint32_t n = tw * th * CH * Form<PIX>::BPS, half = n >> 1;
    fill_raw<CH, PIX>(s_raw, src, f, tx, ty, tw, th, t);
    __syncthreads();
    const unsigned char *raw = (const unsigned char *)s_raw;
    const auto split = [&](uint32_t p) -> uint32_t { return p < half ? raw[2u * p] : raw[2u * (p - half) + 1u]; };
    uint32_t *dst = staged + (size_t)it * (TILE / 4u);
    for (uint32_t i = t; i < (n + 3u) / 4u; i += 256u) {      // (n <= TILE, a multiple of four: the last word stays inside the piece)
        uint32_t out = 0, prev = i ? split(4u * i - 1u) : 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t p = 4u * i + k;
            if (p >= n) break;
            const uint32_t cur = split(p);
            out |= (p ? (cur - prev + 128u) & 0xffu : cur) << (8u * k);
            prev = cur;
        }
        dst[i] = out;
    }
    if (t == 0) lens[it] = n;
}

// ---- where the chunks go -----------------------------------------------------------------------------------------------
// A chunk is its 20-byte head and the tile's data: the zlib stream (2 + block + 4 bytes) where that is smaller than the tile's n raw
// bytes, else those.  A reader tells them apart by the size alone.
__device__ __forceinline__ uint32_t data_bytes(uint32_t block, uint32_t n) { return block + 6u < n ? block + 6u : n; }

// offs[i] = where chunk i starts in the file (the file stays below 2^32 bytes: the callers checked the bound).  The record, the header
// and the offset table go to `out` (cap >= 16 + the header and the table: the callers checked).
__global__ void __launch_bounds__(1024)
k_exr_scan(const uint32_t *__restrict__ lens, ExrFrame f, uint32_t TH, uint32_t pixel_bytes, uint32_t tile_bytes, uint32_t *__restrict__ offs,
           uint32_t *__restrict__ info, unsigned char *__restrict__ out, u64 cap, ExrHeaderArg hdr)
{
    __shared__ u64 s_sum[1024];
    const uint32_t t = threadIdx.x, nt = f.nt;
    const u64 H = (u64)hdr.n + 8ull * nt;
    const auto chunk = [&](uint32_t i) -> uint32_t {
        uint32_t tx, ty, tw, th;
        tile_of(f, i, TH, tx, ty, tw, th);
        return 20u + data_bytes(lens[i], tw * th * pixel_bytes);
    };
    const Placement p = place_pieces(s_sum, nt, t, H, chunk);
    if (finish_placement(info, out, H + p.total, cap, tile_bytes, 0u, t)) return;      // a file that does not fit leaves nothing behind the record
    if (t < hdr.n) out[16u + t] = hdr.b[t];
    unsigned char *table = out + 16u + hdr.n;
    for_placed(p, chunk, [&](uint32_t i, u64 at) {
        offs[i] = (uint32_t)at;
        put_le32(table + 8u * (size_t)i, (uint32_t)at); put_le32(table + 8u * (size_t)i + 4u, 0u);
    });
}

// ---- the finished chunks -----------------------------------------------------------------------------------------------
// One workgroup per tile: the chunk assembled in LDS and stored at out + 16 + offs[it].
// Dynamic LDS: 20 + 8192 * CH bytes in words, and 2 words of padding.
template <int CH, int PIX>
__global__ void __launch_bounds__(256)
k_exr_gather(const float4 *__restrict__ src, ExrFrame f, const unsigned char *__restrict__ segbuf, uint32_t stride,
             const uint32_t *__restrict__ lens, const uint32_t *__restrict__ adl, const uint32_t *__restrict__ offs,
             const uint32_t *__restrict__ info, unsigned char *__restrict__ out)
{
    extern __shared__ uint32_t s_mem[];
    unsigned char *s_data = (unsigned char *)(s_mem + 5);
    const uint32_t t = threadIdx.x, it = blockIdx.x;
    if (info[kInfoStatus]) return;
    uint32_t tx, ty, tw, th;
    tile_of(f, it, Form<PIX>::TH, tx, ty, tw, th);
    const uint32_t n = tw * th * CH * Form<PIX>::BPS, L = lens[it], dsz = data_bytes(L, n);
    if (t < 5u) s_mem[t] = t == 0 ? tx : t == 1u ? ty : t == 4u ? dsz : 0u;      // tileX, tileY, levelX, levelY, dataSize
    if (dsz == n) fill_raw<CH, PIX>(s_mem + 5, src, f, tx, ty, tw, th, t);
    else stage_block(s_data, (const uint32_t *)(segbuf + (size_t)it * stride), L, t, true, adl + it);
    __syncthreads();
    store_bytes<256>(out + 16u + offs[it], s_mem, 20u + dsz, t);
}

void put32(unsigned char *&p, uint32_t v) { for (int k = 0; k < 4; ++k) *p++ = (unsigned char)(v >> (8 * k)); }
void putf(unsigned char *&p, float v) { uint32_t u; memcpy(&u, &v, 4); put32(p, u); }
void puts0(unsigned char *&p, const char *s) { do *p++ = (unsigned char)*s; while (*s++); }
void attr(unsigned char *&p, const char *name, const char *type, uint32_t size) { puts0(p, name); puts0(p, type); put32(p, size); }

// magic, version, the attributes in their order, the byte that ends them
uint32_t exr_header(unsigned char *b, uint32_t w, uint32_t h, int channels, int pixel)
{
    unsigned char *p = b;
    put32(p, 0x01312f76u); put32(p, 0x00000202u);             // version 2, the tiled bit
    attr(p, "channels", "chlist", 18u * (uint32_t)channels + 1u);
    for (const char *c = channels == 4 ? "ABGR" : "BGR"; *c; ++c) {
        *p++ = (unsigned char)*c; *p++ = 0;
        put32(p, (uint32_t)pixel); put32(p, 0); put32(p, 1); put32(p, 1);      // type; pLinear and three reserved bytes; x, y sampling
    }
    *p++ = 0;
    attr(p, "compression", "compression", 1); *p++ = 3;      // ZIP: 16 scan lines a block in a scan-line file, a tile here
    attr(p, "dataWindow", "box2i", 16); put32(p, 0); put32(p, 0); put32(p, w - 1u); put32(p, h - 1u);
    attr(p, "displayWindow", "box2i", 16); put32(p, 0); put32(p, 0); put32(p, w - 1u); put32(p, h - 1u);
    attr(p, "lineOrder", "lineOrder", 1); *p++ = 0;         // increasing Y
    attr(p, "pixelAspectRatio", "float", 4); putf(p, 1.0f);
    attr(p, "screenWindowCenter", "v2f", 8); putf(p, 0.0f); putf(p, 0.0f);
    attr(p, "screenWindowWidth", "float", 4); putf(p, 1.0f);
    attr(p, "tiles", "tiledesc", 9); put32(p, FL_EXR_TILE_WIDTH);
    put32(p, pixel == FL_EXR_FLOAT ? FL_EXR_TILE_ROWS_FLOAT : FL_EXR_TILE_ROWS_HALF); *p++ = 0;      // one level, round down
    *p++ = 0;
    return (uint32_t)(p - b);
}

template <int CH, int PIX>
void launch_form(hipStream_t st, const float4 *src, const ExrFrame f, const ExrLayout &l, uint32_t *scratch, unsigned char *out, size_t cap,
                 const ExrHeaderArg &hdr)
{
    uint32_t *staged = scratch + l.staged, *offs = scratch + l.offs, *lens = scratch + l.lens, *adl = scratch + l.adl, *info = scratch + l.info;
    unsigned char *segbuf = (unsigned char *)(scratch + l.segbuf);
    hipLaunchKernelGGL((k_exr_tiles<CH, PIX>), dim3(l.nt), dim3(256), 0, st, src, f, staged, lens);
    launch_deflate_pieces(st, (const unsigned char *)staged, l.tile_bytes, l.nt, segbuf, l.stride, lens, adl);
    hipLaunchKernelGGL(k_exr_scan, dim3(1), dim3(1024), 0, st, (const uint32_t *)lens, f, Form<PIX>::TH, (uint32_t)CH * Form<PIX>::BPS, l.tile_bytes,
                       offs, info, out, (u64)cap, hdr);
    hipLaunchKernelGGL((k_exr_gather<CH, PIX>), dim3(l.nt), dim3(256), 4 * (size_t)((20u + l.tile_bytes) / 4u + 2u), st, src, f,
                       (const unsigned char *)segbuf, l.stride, (const uint32_t *)lens, (const uint32_t *)adl, (const uint32_t *)offs,
                       (const uint32_t *)info, out);
}

} // namespace

ExrLayout exr_layout(uint32_t w, uint32_t h, int channels, int pixel)
{
    ExrLayout l;
    unsigned char b[kHeaderMax];
    l.th = pixel == FL_EXR_FLOAT ? FL_EXR_TILE_ROWS_FLOAT : FL_EXR_TILE_ROWS_HALF;
    l.tiles_x = (w + FL_EXR_TILE_WIDTH - 1u) / FL_EXR_TILE_WIDTH;
    l.nt = l.tiles_x * ((h + l.th - 1u) / l.th);
    l.tile_bytes = 8192u * (uint32_t)channels;
    l.stride = l.tile_bytes + 16u;                            // a stored tile is tile_bytes + 5 bytes; rows of the scratch stay 16-byte aligned
    l.header = exr_header(b, w, h, channels, pixel);
    l.H = (uint64_t)l.header + 8ull * l.nt;
    l.raw = (uint64_t)w * h * (uint32_t)channels * (pixel == FL_EXR_FLOAT ? 4u : 2u);
    // words: the staged stream (read in 16-byte pieces) | the coded tiles | offsets | lengths | Adler-32s | info
    l.staged = 0;
    l.segbuf = l.staged + (size_t)l.nt * (l.tile_bytes / 4u) + 4u;
    l.offs = l.segbuf + (size_t)l.nt * (l.stride / 4u);
    l.lens = l.offs + l.nt;
    l.adl = l.lens + l.nt;
    l.info = l.adl + l.nt;
    l.words = l.info + 4u;
    return l;
}

void launch_exr_encode(hipStream_t st, const float4 *src, uint32_t src_stride, uint32_t w, uint32_t h, int channels, int pixel, uint32_t *scratch,
                       unsigned char *out, size_t cap)
{
    const ExrLayout l = exr_layout(w, h, channels, pixel);
    const ExrFrame f = {w, h, src_stride, l.tiles_x, l.nt};
    ExrHeaderArg hdr = {};
    hdr.n = exr_header(hdr.b, w, h, channels, pixel);
    if (pixel == FL_EXR_FLOAT) {
        if (channels == 4) launch_form<4, FL_EXR_FLOAT>(st, src, f, l, scratch, out, cap, hdr);
        else launch_form<3, FL_EXR_FLOAT>(st, src, f, l, scratch, out, cap, hdr);
    } else {
        if (channels == 4) launch_form<4, FL_EXR_HALF>(st, src, f, l, scratch, out, cap, hdr);
        else launch_form<3, FL_EXR_HALF>(st, src, f, l, scratch, out, cap, hdr);
    }
}
