// tiff.hip — tiled TIFF (classic, little-endian, one IFD; Compression 8 = Adobe deflate, Predictor 2; 8 or 16 bits a sample, 3 or 4
// samples a pixel) from u8 or u16 [h][w][4] on the device.  DESIGN.md §4.13.
// Four launches per frame, no host wait between them:
//   k_tiff_tiles    pixels -> the predicted byte stream in tile order: tiles of 64 rows of TW pixels (128 at 8 bits, 64 at 16), row-major;
//                   a sample outside the image is the clamped pixel's; within a tile row every sample but the first pixel's is the
//                   difference to the same channel of the pixel to its left, mod 2^bits, low byte first
//   k_png_segment   (png.hip, its TILES form) one workgroup per tile: one final deflate block, dynamic or stored, and the tile's Adler-32
//   k_tiff_scan     one workgroup: the tiles' even offsets and the total; the 16-byte record, header, IFD, BitsPerSample, TileOffsets and
//                   TileByteCounts
//   k_tiff_gather   one workgroup per tile: 78 01, the block, the Adler-32 and the pad byte copied to their place
// File layout: bytes 0..7 | entry count, the entries, next IFD = 0 | BitsPerSample | TileOffsets, TileByteCounts (only when there is more
// than one tile: a lone tile's values sit in their entries) | the tiles, each at an even offset.
// Nothing is stored at or beyond `cap`: the gather stores nothing when the file does not fit.
#include "kernels.h"
#include "encode_device.h"

namespace {

constexpr uint32_t kHeaderMax = 8u + 2u + 12u * 13u + 4u + 2u * 4u;      // four channels: 13 entries, 4 SHORTs of BitsPerSample

// Header, IFD and BitsPerSample as the host wrote them; with one tile the value of TileByteCounts (4 bytes at count_at) is the device's.
struct TiffHeaderArg { unsigned char b[kHeaderMax]; uint32_t n, count_at; };

// ---- tiling and the predictor ------------------------------------------------------------------------------------------
template <int BITS>
__device__ __forceinline__ uint32_t sample_at(const unsigned char *line, uint32_t x, uint32_t c)
{
    if (BITS == 8) return line[(size_t)x * 4u + c];
    return ((const unsigned short *)line)[(size_t)x * 4u + c];
}

// A thread per four bytes of the stream (F = tiles * TILE < 2^32 bytes; a tile row is a multiple of four bytes, so the four share
// their tile and row); tiled holds F / 4 words.
template <int CH, int BITS>
__global__ void __launch_bounds__(256)
k_tiff_tiles(const unsigned char *__restrict__ src, uint32_t w, uint32_t h, uint32_t tiles_x, uint32_t F, uint32_t *__restrict__ tiled)
{
    constexpr uint32_t BPS = BITS / 8, TW = BITS == 8 ? 128u : 64u, ROW = TW * CH * BPS, TILE = ROW * FL_TIFF_TILE_LENGTH, MASK = BITS == 8 ? 0xffu : 0xffffu;
    static_assert(ROW % 4u == 0, "a thread's four bytes stay in one tile row");
    const u64 p64 = ((u64)blockIdx.x * 256u + threadIdx.x) * 4u;
    if (p64 >= F) return;
    const uint32_t p0 = (uint32_t)p64, tile = p0 / TILE, r = p0 - tile * TILE, ty = r / ROW, cb = r - ty * ROW;
    const uint32_t tyi = tile / tiles_x, txi = tile - tyi * tiles_x;
    const uint32_t y = min(tyi * FL_TIFF_TILE_LENGTH + ty, h - 1u), x0 = txi * TW;
    const unsigned char *line = src + (size_t)y * w * (4u * BPS);
    uint32_t out = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t b = cb + k, si = b / BPS, px = si / CH, c = si - px * CH;
        uint32_t v = sample_at<BITS>(line, min(x0 + px, w - 1u), c);
        if (px) v = (v - sample_at<BITS>(line, min(x0 + px - 1u, w - 1u), c)) & MASK;      // word arithmetic at 16 bits
        out |= (v >> (8u * (b & (BPS - 1u))) & 0xffu) << (8u * k);                          // low byte first
    }
    tiled[p0 >> 2] = out;
}

// ---- where the tiles go ------------------------------------------------------------------------------------------------
// Tile i takes lens[i] + 6 bytes (zlib header, block, Adler-32) and, unless it is the last, a zero byte behind an odd length.
__device__ __forceinline__ uint32_t tile_data_bytes(uint32_t len) { return len + 6u; }
__device__ __forceinline__ uint32_t tile_placed_bytes(uint32_t len, uint32_t i, uint32_t nt) { return len + 6u + (i + 1u < nt ? len & 1u : 0u); }

// offs[i] = where tile i starts in the file (the file stays below 2^32 bytes: the callers checked the bound).  The record, the header
// and both arrays go to `out` (cap >= 16 + the header and the arrays: the callers checked).
__global__ void __launch_bounds__(1024)
k_tiff_scan(const uint32_t *__restrict__ lens, uint32_t nt, uint32_t tile_bytes, uint32_t *__restrict__ offs, uint32_t *__restrict__ info,
            unsigned char *__restrict__ out, u64 cap, TiffHeaderArg hdr)
{
    __shared__ u64 s_sum[1024];
    const uint32_t t = threadIdx.x;
    const u64 H = (u64)hdr.n + (nt > 1u ? 8ull * nt : 0ull);
    const auto len = [&](uint32_t i) { return tile_placed_bytes(lens[i], i, nt); };
    const Placement p = place_pieces(s_sum, nt, t, H, len);
    finish_placement(info, out, H + p.total, cap, tile_bytes, 0u, t);
    if (t < hdr.n) {
        uint32_t v = hdr.b[t];
        if (nt == 1u && t - hdr.count_at < 4u) v = tile_data_bytes(lens[0]) >> (8u * (t - hdr.count_at)) & 0xffu;
        out[16u + t] = (unsigned char)v;
    }
    unsigned char *po = out + 16u + hdr.n, *pc = po + 4u * (size_t)nt;
    for_placed(p, len, [&](uint32_t i, u64 at) {
        offs[i] = (uint32_t)at;
        if (nt > 1u) { put_le32(po + 4u * (size_t)i, (uint32_t)at); put_le32(pc + 4u * (size_t)i, tile_data_bytes(lens[i])); }
    });
}

// ---- the finished tiles ------------------------------------------------------------------------------------------------
// One workgroup per tile: the zlib stream (and the pad byte) assembled in LDS and stored at out + 16 + offs[it].
// Dynamic LDS: tile_bytes + 5 + 7 bytes, rounded up to words, and 2 words of padding.
__global__ void __launch_bounds__(256)
k_tiff_gather(const unsigned char *__restrict__ segbuf, uint32_t stride, const uint32_t *__restrict__ lens, const uint32_t *__restrict__ adl,
              const uint32_t *__restrict__ offs, const uint32_t *__restrict__ info, uint32_t nt, unsigned char *__restrict__ out)
{
    extern __shared__ uint32_t s_mem[];
    unsigned char *s_tile = (unsigned char *)s_mem;
    const uint32_t t = threadIdx.x, it = blockIdx.x;
    if (info[kInfoStatus]) return;
    const uint32_t L = lens[it];
    if (t == 0) s_tile[6u + L] = 0;                           // the pad byte
    stage_block(s_tile, (const uint32_t *)(segbuf + (size_t)it * stride), L, t, true, adl + it);
    __syncthreads();
    store_bytes<256>(out + 16u + offs[it], s_mem, tile_placed_bytes(L, it, nt), t);      // (s_tile, with the 2 words of padding behind it)
}

void put16(unsigned char *&p, uint32_t v) { *p++ = (unsigned char)v; *p++ = (unsigned char)(v >> 8); }
void put32(unsigned char *&p, uint32_t v) { put16(p, v); put16(p, v >> 16); }
void entry(unsigned char *&p, uint32_t tag, uint32_t type, uint32_t count, uint32_t value)      // type 3 SHORT, 4 LONG
{
    put16(p, tag); put16(p, type); put32(p, count);
    if (type == 3u && count == 1u) { put16(p, value); put16(p, 0); }      // a lone SHORT sits left-justified in the value field
    else put32(p, value);
}

} // namespace

TiffLayout tiff_layout(uint32_t w, uint32_t h, int channels, int bits)
{
    TiffLayout l;
    l.tw = bits == 8 ? 128u : 64u;
    l.tiles_x = (w + l.tw - 1u) / l.tw;
    l.nt = l.tiles_x * ((h + FL_TIFF_TILE_LENGTH - 1u) / FL_TIFF_TILE_LENGTH);
    l.tile_bytes = l.tw * FL_TIFF_TILE_LENGTH * (uint32_t)(channels * bits / 8);
    l.stride = l.tile_bytes + 16u;                            // a stored tile is tile_bytes + 5 bytes; rows of the scratch stay 16-byte aligned
    l.entries = channels == 4 ? 13u : 12u;
    l.fixed = 8u + 2u + 12u * l.entries + 4u + 2u * (uint32_t)channels;
    l.H = (uint64_t)l.fixed + (l.nt > 1u ? 8ull * l.nt : 0ull);
    l.F = (uint64_t)l.nt * l.tile_bytes;
    // words: the tiled stream (read in 16-byte pieces) | the coded tiles | offsets | lengths | Adler-32s | info
    l.tiled = 0;
    l.segbuf = l.tiled + (size_t)(l.F / 4u) + 4u;
    l.offs = l.segbuf + (size_t)l.nt * (l.stride / 4u);
    l.lens = l.offs + l.nt;
    l.adl = l.lens + l.nt;
    l.info = l.adl + l.nt;
    l.words = l.info + 4u;
    return l;
}

void launch_tiff_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int channels, int bits, uint32_t *scratch,
                        unsigned char *out, size_t cap)
{
    const TiffLayout l = tiff_layout(w, h, channels, bits);
    const uint32_t F = (uint32_t)l.F;                         // (the callers refuse frames whose file could pass 2^32 - 1 bytes)
    uint32_t *tiled = scratch + l.tiled, *offs = scratch + l.offs, *lens = scratch + l.lens, *adl = scratch + l.adl, *info = scratch + l.info;
    unsigned char *segbuf = (unsigned char *)(scratch + l.segbuf);
    TiffHeaderArg hdr = {};
    unsigned char *p = hdr.b;
    *p++ = 'I'; *p++ = 'I'; put16(p, 42); put32(p, 8);
    put16(p, l.entries);
    const uint32_t arrays = l.fixed;                          // TileOffsets, then TileByteCounts, when they do not fit their entries
    entry(p, 256, 4, 1, w);
    entry(p, 257, 4, 1, h);
    entry(p, 258, 3, (uint32_t)channels, l.fixed - 2u * (uint32_t)channels);
    entry(p, 259, 3, 1, 8);                                   // Adobe deflate
    entry(p, 262, 3, 1, 2);                                   // RGB
    entry(p, 277, 3, 1, (uint32_t)channels);
    entry(p, 284, 3, 1, 1);                                   // chunky
    entry(p, 317, 3, 1, 2);                                   // horizontal differencing
    entry(p, 322, 4, 1, l.tw);
    entry(p, 323, 4, 1, FL_TIFF_TILE_LENGTH);
    entry(p, 324, 4, l.nt, l.nt == 1u ? l.fixed : arrays);
    entry(p, 325, 4, l.nt, l.nt == 1u ? 0u : arrays + 4u * l.nt);
    hdr.count_at = (uint32_t)(p - hdr.b) - 4u;
    if (channels == 4) entry(p, 338, 3, 1, 2);                // unassociated alpha
    put32(p, 0);
    for (int c = 0; c < channels; ++c) put16(p, (uint32_t)bits);
    hdr.n = (uint32_t)(p - hdr.b);                            // == l.fixed
    const dim3 fgrid((F / 4u + 255u) / 256u);
    if (bits == 8) {
        if (channels == 4) hipLaunchKernelGGL((k_tiff_tiles<4, 8>), fgrid, dim3(256), 0, st, src, w, h, l.tiles_x, F, tiled);
        else hipLaunchKernelGGL((k_tiff_tiles<3, 8>), fgrid, dim3(256), 0, st, src, w, h, l.tiles_x, F, tiled);
    } else {
        if (channels == 4) hipLaunchKernelGGL((k_tiff_tiles<4, 16>), fgrid, dim3(256), 0, st, src, w, h, l.tiles_x, F, tiled);
        else hipLaunchKernelGGL((k_tiff_tiles<3, 16>), fgrid, dim3(256), 0, st, src, w, h, l.tiles_x, F, tiled);
    }
    launch_deflate_tiles(st, (const unsigned char *)tiled, l.tile_bytes, l.nt, segbuf, l.stride, lens, adl);
    hipLaunchKernelGGL(k_tiff_scan, dim3(1), dim3(1024), 0, st, lens, l.nt, l.tile_bytes, offs, info, out, (u64)cap, hdr);
    hipLaunchKernelGGL(k_tiff_gather, dim3(l.nt), dim3(256), 4 * (size_t)((l.tile_bytes + 5u + 7u + 3u) / 4u + 2u), st, segbuf, l.stride, lens, adl,
                       offs, info, l.nt, out);
}
