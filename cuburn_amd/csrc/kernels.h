// kernels.h — host-callable launchers of the gfx950 kernels (internal to libflame_hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/flame_hip.h"

typedef unsigned long long u64;

// hipFuncSetAttribute is per DEVICE: raise a kernel's dynamic-LDS cap once on every device it is
// launched on (a process may hold contexts on several GPUs).  `done` is a per-kernel bit mask.
static inline void ensure_max_dynamic_lds(const void *fn, unsigned long long &done)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) dev = 63;
    if (done >> dev & 1ull) return;
    hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (dev != 63) done |= 1ull << dev;
}

// iter.hip
// One iterate launch: walker geometry, accumulate mode, buffers, rounds, and (binned modes) the tile geometry, sample log and directory.
struct IterLaunch {
    int nw; bool count; int acc; uint32_t nslots;      // waves per workgroup, debug counters, accumulate mode (iter_body's ACC), workgroups
    const int32_t *prog; const float *params; const u64 *palette; fl_mwc *rng; float4 *points;
    const uint32_t *hot; u64 *atom; float *out4; u64 *counters;
    uint32_t astride, aheight, round0, nrounds, fuse;
    uint32_t tiles_x, nbins, rounds_per_batch, nbatch_total;
    uint32_t *log, *dir;
    hipEvent_t ev_start, ev_stop;                      // bracket the kernel itself (may be null)
    uint32_t sub_log2;                                 // 8- / 16-wave workgroups of 2 / 4 temporal samples (iter_body)
    bool chaos;                                        // the program has 9 words (the CHAOS form of the walk)
};
// fn: the genome's run-time compiled kernel (rtc.hip), or nullptr for the interpreter kernel
void launch_iter(hipStream_t st, const IterLaunch &launch, hipFunction_t fn);
void launch_flush(hipStream_t st, u64 *atom, float4 *out, uint32_t *hot, uint32_t nbins, bool use_hot);
void launch_clear_frame(hipStream_t st, float4 *front, u64 *atom, uint32_t *hot, u64 *counters, float4 *points,
                        uint32_t nbins, uint32_t npoints);      // npoints = 0: the walkers are left alone
void launch_shuffle_tap(hipStream_t st, int nw, uint32_t *out, uint32_t round);
void launch_apply_xf_tap(hipStream_t st, const int32_t *prog, const float *params, uint32_t ts, int xfi,
                         uint32_t n, float4 *pts, fl_mwc *rng);
void launch_math_tap(hipStream_t st, int fn, uint32_t n, const float *a, const float *b, uint32_t *out);

// rtc.hip: structure of a genome as the run-time specialised iterate kernel needs it (include/flame_hip.h (5))
#include <string>
#include <vector>
struct IterSpec {
    int nxf = 0, has_final = 0, pstride = 0, cdf_off = 0, xf_off = 0, xf_stride = 0, var_stride = 0;
    int chaos = 0, chaos_off = 0;                // a program of 9 words: the CHAOS form of the walk, and its matrix's block offset
    std::vector<int> nvar, post, opac;           // per record (selectable xforms, then the final xform): variations, post affine, opacity
    std::vector<std::vector<int>> vids;          // flam3 variation numbers in application order
};
bool rtc_available();
unsigned rtc_epoch();      // changes when cached modules were unloaded: function handles obtained before are void
int rtc_compile(const IterSpec &spec, int nw, bool count, int acc, std::vector<char> *code, std::string *err, const char *extra_opt = nullptr, uint32_t sub_log2 = 0);
// How rtc_iter_kernel gets a variant that is not in the process cache: compile it now (0 or -1); or have the worker thread compile
// it (FLAME_RTC_ASYNC) and return 1 while a job of the variant is unfinished — RTC_WAIT instead waits for it.  Module load, function
// lookup and the register check happen on the calling thread in every mode.
enum { RTC_SYNC = 0, RTC_POLL = 1, RTC_WAIT = 2 };
int rtc_iter_kernel(int device, const IterSpec &spec, int nw, uint32_t nslots, bool count, int acc, hipFunction_t *fn, std::string *err, uint32_t sub_log2 = 0,
                    int mode = RTC_SYNC);
void rtc_stats(uint64_t out[8]);                    // fl_rtc_stats
void rtc_count_launch(bool spec, bool pending);     // an iterate launch: on a per-genome kernel / on the interpreter while a job of its variant was pending
void rtc_hold(bool on);                             // fl_debug_rtc_hold: the worker leaves queued jobs alone while held
bool rtc_held();

// binned.hip
void launch_accum_tiles(hipStream_t st, const uint32_t *log, const uint32_t *dir, const u64 *palette,
                        u64 *atom, float *out4, uint32_t tiles_x, uint32_t nbins, uint32_t nparts,
                        uint32_t nbatch_total, uint32_t batch_records, uint32_t nslots,
                        uint32_t astride, uint32_t aheight, bool wide);

// interp.hip
void launch_interp_palette(hipStream_t st, fl_mwc *rng_pal, const float *ptimes, const float4 *pals,
                           float ts, float tstep, u64 *out);
void launch_interp_params(hipStream_t st, float *params, const float *times, const float *knots,
                          const int32_t *ops, uint32_t nops, uint32_t pstride, uint32_t nts, float ts, float tstep,
                          fl_dim dim, bool zero_first);

// filters.hip
void launch_yuv_to_rgb(hipStream_t st, fl_dim d, float4 *dst, const float4 *src);
void launch_den_blur_1c(hipStream_t st, fl_dim d, float *dst, const float *src, int pattern, int upsample, const float *coefs7);
void launch_full_blur(hipStream_t st, fl_dim d, float4 *dst, const float4 *src, int pattern, int upsample, const float *coefs7);
void launch_logscale(hipStream_t st, fl_dim d, float4 *buf, float k1, float k2);
void launch_colorclip(hipStream_t st, fl_dim d, float4 *buf, float vib, float highpow, float gam, float lin, float lingam);
void launch_gamma_full_hi(hipStream_t st, fl_dim d, float4 *dst, const float4 *src);
void launch_smearclip(hipStream_t st, fl_dim d, float4 *buf, const float4 *smear, float gam_m_1, float lin, float lingam);
void launch_apply_gamma(hipStream_t st, fl_dim d, float *dst, const float4 *src, float gamma);
void launch_haloclip(hipStream_t st, fl_dim d, float4 *buf, const float *den, float gam_m_1);
void launch_plainclip(hipStream_t st, fl_dim d, float4 *buf, float gam_m_1, float lin, float lingam, float brightness);
void launch_logencode(hipStream_t st, fl_dim d, float4 *dst, const float4 *src, float degamma);

// de.hip
// tone filters that ride along with the last DE direction (filters.py default chains: DE -> logscale -> colorclip)
struct DeTail { int do_log; float k1, k2; int do_clip; float vib, highpow, gam, lin, lingam; int order; };
void launch_de_dir(hipStream_t st, fl_dim d, int pattern, float4 *Nout, const float4 *N, const float *coefs7,
                   float sstd, float cstd, float dstd, float dpow, float gspeed, int in_mode = 1, const DeTail *tail = nullptr,
                   int order_override = -1);
// (pattern 0 normalises the raw accumulator as it stages it — in_mode 1, or 2: after yuv -> rgb —; pattern 7 un-normalises and
// applies `tail`'s tone filters as it stores; round 5 removed the separate normalise / finish kernels, the persistent and the
// overlapped eight-direction launches of round 4 (de_chain.hip: git history, commit 58f1875) and round 1's blur + packed-math pair)

// de_adaptive.hip: the `de` filter (FL_FILT_DE), in place on buf; stage_c / stage_a / tmax are scratch of nbins float4 /
// nbins float / de_adaptive_tiles() words, sinv the 16 * FL_DE_MAX_RADIUS + 1 normalisers of de_adaptive_norms()
void launch_de_adaptive(hipStream_t st, fl_dim d, float4 *buf, float4 *stage_c, float *stage_a, uint32_t *tmax,
                        const float *sinv, float R, float Rmin, float curve);
size_t de_adaptive_tiles(fl_dim d);
void de_adaptive_norms(float *out);

// bloom.hip: the `bloom` filter (FL_FILT_BLOOM), in place on front; side is scratch of nbins float4; taps[0 .. R] the centre tap and
// one side of the symmetric kernel, R <= FL_BLOOM_MAX_REACH (fl_filter checks).  The taps travel as kernel arguments: `taps` is
// free again when the call returns.
void launch_bloom(hipStream_t st, fl_dim d, float4 *front, float4 *side, const float *taps, int R, float thr, float strength);

// resample.hip: flam3's spatial filter + supersample decimation, src laid out as din (the ss-fold frame) -> dst laid out as dout;
// ntaps in [ss, ss + 2 * FL_GUTTER] of the same parity as ss (fl_resample checks)
void launch_resample(hipStream_t st, fl_dim din, fl_dim dout, int ss, float4 *dst, const float4 *src, const float *taps, int ntaps);

// resize.hip: Lanczos downscale (fl_resize), src laid out as din -> dst laid out as dout (dout.w <= din.w, dout.h <= din.h); side is
// scratch of din's nbins float4.  The tables are DEVICE arrays: xfirst[dout.w], xtaps[dout.w][nxt], yfirst[dout.h], ytaps[dout.h][nyt],
// nxt, nyt <= FL_RESIZE_MAX_TAPS, every window inside the source (fl_resize checks).  resize_rows_fit (host arrays): the x windows of
// every FL_RESIZE_XSEG neighbouring output columns span at most FL_RESIZE_XSPAN source bins, which is what k_resize_rows stages per wave
// (a downscale of ratio <= 8 spans at most 63 * 8 + 1 + 50 = 555).
#define FL_RESIZE_XSEG 64
#define FL_RESIZE_XSPAN 576
bool resize_rows_fit(const int32_t *xfirst, uint32_t w2, uint32_t nxt);
void launch_resize(hipStream_t st, fl_dim din, fl_dim dout, float4 *dst, float4 *side, const float4 *src,
                   const int32_t *xfirst, const float *xtaps, int nxt, const int32_t *yfirst, const float *ytaps, int nyt);

// output.hip
void launch_f32_to_rgba(hipStream_t st, fl_dim d, const float4 *src, fl_mwc *rng, uint32_t nrng, int fmt, void *dst);

// jpeg.hip: baseline JPEG from u8 [3][h][w] Y/Cb/Cr planes.  `scratch` holds jpeg_layout().words words; the 16-byte record, the header and
// the stream go to `out`, of which nothing at or beyond `cap` (>= 16 + FL_JPEG_HEADER_BYTES) is touched.  sampling: FL_JPEG_444 or
// FL_JPEG_420 (the chroma planes are averaged 2 x 2 on load).  ri: MCUs per restart interval, 1..21 in 4:4:4 and 1..10 in 4:2:0.
#define FL_JPEG_RI 8u      // the default: how it was chosen is in DESIGN.md §4.8 (a wave codes one interval, a lane one block, so 3 * ri <= 64)
#define FL_JPEG_RI_420 4u  // the default in 4:2:0 (6 * ri <= 64): the 24 working lanes of the 4:4:4 default; the sweep of DESIGN.md §4.10 does not separate 2 .. 10
#define FL_JPEG_RI_420_MAX 10u
// optimize: the Huffman tables are built from the frame's own symbol counts; the frame has at most FL_JPEG_OPT_MAX_BLOCKS blocks.
#define FL_JPEG_OPT_MAX_BLOCKS (1u << 24)      // 63 symbols a block at frequency 2 * count + 2: the builder's 32-bit sums hold them
struct JpegLayout { uint32_t mw, nmcu, nint; size_t coef, offs, lens, acbits, info, counts, huff, words; };      // MCUs per row / in all, intervals; word offsets into the scratch
JpegLayout jpeg_layout(uint32_t w, uint32_t h, uint32_t ri, int sampling);
void launch_jpeg_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int quality, uint32_t ri, int sampling, bool optimize,
                        uint32_t *scratch, unsigned char *out, size_t cap);
// encode_device.h's place_pieces and store_offsets in a kernel of their own (fl_debug_place): offs[i] = front + lens[0] + .. + lens[i - 1]
void launch_debug_place(hipStream_t st, const uint32_t *lens, uint32_t n, u64 front, u64 *offs, u64 *total);

// png.hip: truecolour PNG of 8 or 16 bits a sample from u8 or u16 [h][w][4] (channels 3: the alpha sample is left out).  `scratch` holds
// png_layout().words words; the 16-byte record, signature + IHDR, one IDAT per segment and IEND go to `out`, of which nothing at or
// beyond `cap` (>= 16 + FL_PNG_HEADER_BYTES) is touched.  seg: filtered bytes per segment, a multiple of 16 in [8192, 32768].
// flags: FL_PNG_ADAPTIVE chooses every row's filter type (the table of types is the layout's last part); without it every row is Paeth.
#define FL_PNG_SEG 32768u      // the default: the largest whose bit buffer leaves a workgroup under 64 KiB of LDS
struct PngLayout { uint32_t rowlen, nseg, stride, per; uint64_t F; size_t filt, segbuf, offs, lens, adl, info, types, words; };      // bytes per filtered row, segments, bytes between coded segments, bytes per lane, filtered bytes; word offsets into the scratch
uint32_t png_segment_bytes();      // FL_PNG_SEG, or FLAME_PNG_SEG (measurements only)
PngLayout png_layout(uint32_t w, uint32_t h, int channels, uint32_t seg, int bits, unsigned flags);
void launch_png_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int channels, int bits, unsigned flags, uint32_t seg,
                       uint32_t *scratch, unsigned char *out, size_t cap);
// One frame of an APNG: the record (its fourth word the number of chunks) and the frame's chunks alone go to `out`
// (cap >= 16), with no signature, IHDR or IEND.  seq == FL_APNG_IDAT: the IDATs of launch_png_encode, byte for byte; any other seq:
// chunk i is an fdAT with seq + i in front of the same data (the caller refuses a seq whose last number would pass 0xfffffffe).
void launch_apng_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int channels, int bits, unsigned flags, uint32_t seg,
                        uint32_t seq, uint32_t *scratch, unsigned char *out, size_t cap);

// The same coder for streams that stand alone (tiff.hip): ntiles pieces of tile_bytes bytes (a multiple of 16 in [8192, 32768]) at `bytes`,
// each one final block — dynamic, or stored when that is no smaller — at segbuf + i * stride; lens[i] its bytes (at most tile_bytes + 5),
// adl[i] the Adler-32 of the piece.
void launch_deflate_tiles(hipStream_t st, const unsigned char *bytes, uint32_t tile_bytes, uint32_t ntiles, unsigned char *segbuf, uint32_t stride,
                          uint32_t *lens, uint32_t *adl);

// tiff.hip: tiled little-endian TIFF, Adobe deflate with the horizontal predictor, from the same sources as the PNG.
// `scratch` holds tiff_layout().words words; the 16-byte record, header + IFD + arrays and the tiles go to `out`, of which nothing at or
// beyond `cap` (>= 16 + tiff_layout().H) is touched.  The tile's size is the format's (64 rows of 128 or 64 pixels), not FLAME_PNG_SEG's.
#define FL_TIFF_TILE_LENGTH 64u
struct TiffLayout { uint32_t tw, tiles_x, nt, tile_bytes, stride, entries, fixed; uint64_t H, F; size_t tiled, segbuf, offs, lens, adl, info, words; };      // tile width, tiles per row / in all, bytes per tile, bytes between coded tiles, IFD entries, bytes before the arrays, before the tiles, of the tiled stream; word offsets into the scratch
TiffLayout tiff_layout(uint32_t w, uint32_t h, int channels, int bits);
void launch_tiff_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int channels, int bits, uint32_t *scratch,
                        unsigned char *out, size_t cap);

// The coder once more for pieces of unequal length (exr.hip): piece i is the lens[i] bytes (1 .. tile_bytes) at bytes + i * tile_bytes;
// lens[i] comes back as the block's bytes (at most the piece's + 5).
void launch_deflate_pieces(hipStream_t st, const unsigned char *bytes, uint32_t tile_bytes, uint32_t ntiles, unsigned char *segbuf, uint32_t stride,
                           uint32_t *lens, uint32_t *adl);

// exr.hip: tiled OpenEXR, ZIP, HALF or FLOAT samples, from f32 [h][src_stride][4].  `scratch` holds exr_layout().words
// words; the 16-byte record, the header, the offset table and the chunks go to `out`, of which nothing at or beyond `cap`
// (>= 16 + exr_layout().H) is touched.  Tiles are 64 pixels wide and 64 (HALF) or 32 (FLOAT) rows high, cropped to the image.
#define FL_EXR_TILE_WIDTH 64u
#define FL_EXR_TILE_ROWS_HALF 64u
#define FL_EXR_TILE_ROWS_FLOAT 32u
struct ExrLayout { uint32_t th, tiles_x, nt, tile_bytes, stride, header; uint64_t H, raw; size_t staged, segbuf, offs, lens, adl, info, words; };      // tile rows, tiles per row / in all, bytes of a full tile, bytes between coded tiles, bytes of the header; bytes before the chunks, of all samples; word offsets into the scratch
ExrLayout exr_layout(uint32_t w, uint32_t h, int channels, int pixel);
void launch_exr_encode(hipStream_t st, const float4 *src, uint32_t src_stride, uint32_t w, uint32_t h, int channels, int pixel, uint32_t *scratch,
                       unsigned char *out, size_t cap);

// gif.hip: one GIF frame block — image descriptor, local colour table, LZW data — from u8 [h][w][4] (the alpha byte is ignored): median
// cut by population over a histogram of 32768 cells, an inverse colour map, ordered dither, LZW in segments that each begin with a
// clear code.  `scratch` holds gif_layout().words words; the 16-byte record and the block go to `out`, of which nothing
// at or beyond `cap` (>= 16 + FL_GIF_HEADER_BYTES) is touched.  colors 2..256, amp 0..64, w * h <= 2^24; seg: pixels per segment, 256..3584.
#define FL_GIF_SEG 1024u       // the default
#define FL_GIF_LZW_TABLE_BYTES 32768u      // hash tables of one LZW workgroup: 4 segments a wave at the default, 16 at 256 pixels, 1 at 3584
struct GifLayout { uint32_t npix, seg, nseg, stride, slots_log2, lanes; size_t hist, ccnt, pal, lut, idx, segbuf, offs, lens, info, words; };      // pixels, pixels per segment, segments, bytes between coded segments, log2 of a hash table's slots, segments per LZW workgroup; word offsets into the scratch
uint32_t gif_segment_pixels();      // FL_GIF_SEG, or FLAME_GIF_SEG (measurements only)
GifLayout gif_layout(uint32_t w, uint32_t h, uint32_t seg);
void launch_gif_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int colors, int amp, uint32_t seg, uint32_t *scratch,
                       unsigned char *out, size_t cap);

// webp.hip: one lossless WebP frame block — a whole `VP8L` chunk — from u8 [h][w][4] (channels 3: every alpha reads 255): subtract green,
// a predictor mode per 16 x 16 tile, five prefix codes per 64 x 64 tile, no back references.  `scratch` holds
// webp_layout().words words; the 16-byte record and the block go to `out`, of which nothing at or beyond `cap` (>= 16 + FL_WEBP_HEADER_BYTES)
// is touched.  bound: fl_webp_bound of the frame.  w and h are 1..16384.
struct WebpLayout { uint32_t ptx, pty, gx, gy, G, NR, subwords; size_t asmwords, modes, codes, hdr, cnt, off, sub, subinfo, info, asmb, words; };      // predictor tiles, entropy tiles per row / column / in all, runs, words of the staged beginning and of the assembly buffer; word offsets into the scratch
uint64_t webp_bound_bits(uint32_t w, uint32_t h);      // no payload has more bits (fl_webp_bound)
WebpLayout webp_layout(uint32_t w, uint32_t h);
void launch_webp_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int channels, uint32_t *scratch, unsigned char *out,
                        size_t cap, size_t bound);

int launch_measure_copy(size_t nbytes, int iters, float *ms);      // the device's streaming copy rate (fl_measure_copy)

// sort.hip: one stable radix pass (nbits <= 10 at lo_bit) over n keys; hist = scratch of
// sort_scratch_words() words, chunk_tot = *chunk_words words (the last one receives the number of keys kept)
int launch_sort_pass(hipStream_t st, uint32_t *dst, const uint32_t *src, uint32_t n, uint32_t lo_bit, uint32_t nbits,
                     int ignore_max, uint32_t *hist, uint32_t *chunk_tot, uint32_t *total_dev);
size_t sort_scratch_words(uint32_t n, uint32_t nbits, size_t *chunk_words);
