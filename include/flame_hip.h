/*
 * flame_hip.h — C ABI of the MI355X-native fractal-flame hot path (libflame_hip.so).
 *
 * Drop-in boundary for cuburn's device path.  Each entry point cites the reference
 * interface (file:line in stevenrobertson/cuburn) it replaces.  Plain C types only:
 * no C++ / torch / HIP types cross this boundary (streams and device pointers travel
 * as void* / uint64_t).
 *
 * Status codes: 0 = ok; negative = error (FL_E_*); fl_last_error() gives text.
 * Threading: one fl_ctx per GPU per thread; calls on one ctx are not re-entrant
 * (cuburn/render.py:401-402 makes the same statement for RenderManager).
 */
#ifndef FLAME_HIP_H
#define FLAME_HIP_H

#ifndef __HIPCC_RTC__      /* hipRTC (run-time specialised iterate kernel) has no system headers; the includer typedefs */
#include <stdint.h>
#include <stddef.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define FL_ABI_VERSION 1

enum {
    FL_OK = 0,
    FL_E_INVAL = -1,      /* bad argument / malformed program                      */
    FL_E_NOMEM = -2,      /* hipErrorOutOfMemory; ctx stays usable (render.py:140-147) */
    FL_E_HIP = -3,        /* any other HIP runtime error                            */
    FL_E_NODEV = -4,      /* no usable gfx950 device                                */
    FL_E_UNSUPPORTED = -5 /* variation id / filter id not implemented               */
};

/* ------------------------------------------------------------------------------------
 * Formats that cross the boundary
 * ------------------------------------------------------------------------------------
 *
 * (1) Dimensions — cuburn/render.py:79-89 (Framebuffers.calc_dim): gutter 12,
 *     aw = w + 24, astride = ceil32(aw), ah = ceil16(h + 24).
 */
typedef struct fl_dim {
    uint32_t w, h, aw, ah, astride;
} fl_dim;

/* (2) MWC RNG state — cuburn/code/mwc.py:49-55 (mwc_st), 3 x u32, array-of-structs. */
typedef struct fl_mwc {
    uint32_t mul, state, carry;
} fl_mwc;

/* (3) Packed accumulator cell — cuburn/code/interp.py:428-429 (writer),
 *     cuburn/code/iter.py:385-389,464-468 (reader).  64-bit cell:
 *        hi[31:22] count (10 b) | hi[21:4] sum Y (18 b) | {hi[3:0],lo[31:18]} sum U (18 b)
 *        | lo[17:0] sum V (18 b)
 *     A palette entry is pre-packed as hi = (1<<22)|(y<<4), lo = (u<<18)|v, y,u,v in 0..255.
 *
 * (4) Spline rows — cuburn/code/interp.py:207-232 (GenomePacker.pack): per genome
 *     parameter one row of FL_KNOTS (=32) knot times (padded 1e9) and FL_KNOTS knot
 *     values; normalisation per cuburn/genome/use.py:129-158.  The evaluation reads the two knots either side of the
 *     sample (interp.py:326-334), so a row of all 32 real knots evaluated after its 31st takes its fourth support point
 *     (time and value) from word 0 of the FOLLOWING row, as the reference does; behind the last row the library keeps one
 *     row of padding (1e9 / 0) of its own, so the last row takes it from there.  Rows of up to 31 knots never leave
 *     themselves.
 */
#define FL_KNOTS 32
#define FL_NTEMPORAL 1024   /* cuburn/render.py:207 ntemporal_samples = the minimum number of temporal samples here: one per
                               walker slot (fl_ctx_create nslots >= 1024), or two / four per slot of 512 8-wave / 256 16-wave slots, see fl_interp */
#define FL_PAL_W 256        /* cuburn/render.py:201-202 palette surface 256 x 64 */
#define FL_PAL_H 64
#define FL_GUTTER 12        /* cuburn/render.py:77 */

/* (5) Xform program + parameter block — replaces the per-genome generated CUDA of
 *     cuburn/code/iter.py:121-149,559-575 with data interpreted by one precompiled kernel.
 *     The genome's STRUCTURE (which variations, post affines, final xform) is laid out in the
 *     parameter block itself with fixed strides, so that the kernel reaches everything about
 *     the chosen xform with ONE level of address arithmetic (no pointer chasing).
 *
 *     program header (int32 x 8):
 *       prog[0]  FL_PROG_MAGIC
 *       prog[1]  nxf        number of selectable xforms (string-sorted key order,
 *                            cuburn/genome/use.py:88-91)
 *       prog[2]  has_final  0/1 (cuburn/code/iter.py:303-307)
 *       prog[3]  pstride    floats per temporal-sample parameter block
 *       prog[4]  cdf_off    block offset of CDF[nxf] (cuburn/code/iter.py:12-30; entry
 *                            nxf-1 is stored too and is >= 1)
 *       prog[5]  xf_off     block offset of xform record 0
 *       prog[6]  xf_stride  floats per xform record (multiple of 4)
 *       prog[7]  var_stride floats per variation record (>= 2)
 *     a genome with chaos (flam3 xaos) has a ninth word; programs of 8 words mean what they always meant:
 *       prog[8]  chaos_off  block offset of an nxf x nxf matrix of floats behind the last xform record (every other
 *                            offset keeps its value); row p = the cumulative densities of the step that FOLLOWS xform p
 *                            (FL_OP_CHAOS_CDF below; same form as CDF[nxf], last word 2.0).  nxf <= FL_CHAOS_MAX_XFORMS.
 *     parameter block (32-bit words; floats unless noted):
 *       [0..5]   camera xx,xy,xo,yx,yy,yo (cuburn/code/iter.py:56-79)
 *       xform record i (i = nxf is the final xform) at xf_off + i * xf_stride:
 *         [0..5]  pre affine xx,xy,xo,yx,yy,yo (cuburn/code/iter.py:81-95)
 *         [6..11] post affine (same six; unused unless the flag below says so)
 *         [12] color   [13] color_speed
 *         [14] INT: nvar | (has_post << 8) | (has_opacity << 9)
 *         [15] plot probability q of the xform's samples (FL_OP_OPACITY below); read only where bit 9 of [14] is
 *              set, selectable xforms only.  A sample produced by the xform in a write-enabled round is plotted
 *              with probability q and hidden otherwise; the walk goes on from it either way.  q == 1 and q == 0
 *              draw no random number for the decision, 0 < q < 1 draws one (u = next uniform in [0, 1], plotted
 *              iff u <= q) right after the xform.  Programs without bit 9 run exactly as before.
 *         variation j (sorted-name order, cuburn/code/iter.py:132) at 16 + j * var_stride:
 *           [0] INT flam3 variation number (cuburn/genome/variations.py:28-127)
 *           [1] weight   [2..] the variation's genome parameters in sorted-name order,
 *                              then its precalculated values (cuburn_amd/genome/variations.py)
 *
 *     Contract of a chaos kernel (programs of 9 words; the CHAOS form of the walk, csrc/iter.hip).  The SAMPLE carries
 *     the index of its next xform, `next` in [0, nxf): through the swap as a fourth plane of the swap buffer (+2 KB of
 *     LDS per 256 walkers; kernels of 8-word programs keep their LDS), and between launches and frames in points[].w as
 *     (float)next (other kernels keep writing 0).  On load it is clamped to nxf - 1 and a non-finite w counts as 0 — the
 *     buffer may last have served another genome; an index past the records never reaches an address.
 *     What a lane draws in one round, fuse rounds included, in order: (1) the reseed, three draws, only for a bad point;
 *     (2) only after a reseed, one draw u that picks `next` from CDF[nxf]; (3) the variations of xform p = next; (4) the
 *     opacity decision, as above; (5) the chaos draw, one u per lane every round: next = the smallest n with
 *     u <= row p [n], else nxf - 1; (6) the swap; (7) the final xform; (8) the atomic back-end's roulette.  The wave's
 *     selector (lane 0's draw of the other kernels) is NOT drawn.  A wave runs the arm of every xform present among its
 *     lanes under that xform's lane mask; counters, the sort, both accumulate back-ends and the final xform are unchanged.
 */
#define FL_PROG_MAGIC 0x464c5032 /* 'FLP2' */
#define FL_PROG_HDR 8
#define FL_MAX_XFORMS 64
#define FL_CHAOS_MAX_XFORMS 32 /* selectable xforms of a program with chaos */
#define FL_MAX_PSTRIDE 4096
#define FL_XF_HDR 16      /* words of an xform record before its first variation */

/* (6) Interpolation op list (int32 x 4 per op) — replaces the generated
 *     interp_iter_params kernel body (cuburn/code/interp.py:234-272) and the precalc
 *     snippets registered through PrecalcWrapper._code.  op = {kind, dst, a, b}:
 */
enum {
    FL_OP_SPLINE = 0,     /* dst <- catmull_rom(row a)        (interp.py:318-355)        */
    FL_OP_SPLINE_MAG = 1, /* dst <- catmull_rom_mag(row a)    (interp.py:299-316,339-353)*/
    FL_OP_CAMERA = 2,     /* dst[0..5] <- camera precalc; rows a..a+3 = rotation,
                             center.x, center.y, scale(mag)   (iter.py:56-79)            */
    FL_OP_AFFINE = 3,     /* dst[0..5] <- affine precalc; rows a..a+5 = angle, spread,
                             magnitude.x(mag), magnitude.y(mag), offset.x, offset.y
                             (iter.py:81-95)                                             */
    FL_OP_CDF = 4,        /* dst[0..b-1] <- cumulative density; rows a..a+b-1 = xform
                             weights (iter.py:12-30)                                     */
    FL_OP_RATIO2 = 5,     /* dst <- row a / (2 * row b)   julian/juliascope cn
                             (variations.py:292-294); a = dist(mag), b = power(mag)      */
    FL_OP_INVSQ = 6,      /* dst <- 1/(v*v + 1e-20), v = row a  (waves, variations.py:136-140) */
    FL_OP_PERSP = 7,      /* dst[0..2] <- mdist, sin, cos; row a = angle, row b = dist(mag)
                             (variations.py:267-273)                                     */
    FL_OP_INVSQ_MAX = 8,  /* dst <- 1/max(1e-20, v*v), v = row a (mag)  (curve, variations.py:630-634) */
    FL_OP_CONST = 9,      /* dst <- the 32 bits of a (structure words: variation numbers, counts) */
    FL_OP_OPACITY = 10,   /* dst <- q(p), p = clamp(row a (mag), 0, 1): q = 0 for p <= 0, 1 for p >= 1 - 1e-6, else
                             10^(log2 p) = p^3.3219281 (flam3's visibility curve), flushed to 0 below 2^-32.
                             dst must be word 15 of a selectable xform record whose word 14 has bit 9 */
    FL_OP_CHAOS_CDF = 11, /* dst[0..nxf-1] <- row p of the chaos matrix, dst = chaos_off + p * nxf (programs of 9 words only,
                             one op per row).  a = the first of the nxf weight rows FL_OP_CDF reads; b = nxf | (r << 8),
                             r = the first of nxf consecutive rows c_p0 .. c_p,nxf-1 (chaos entries, linear splines).
                             d_n = w_n * max(c_pn, 0), s = sum d_n; if !(s > 0): d_n = w_n (an xform without a permitted
                             successor falls back to the plain weights); dst[n] = running sum of d_n * (1 / s) in
                             float32, FL_OP_CDF's order of operations; dst[nxf-1] = 2 (iter.py:32-54, precalc_chaos) */
};

/* ------------------------------------------------------------------------------------
 * Entry points
 * ------------------------------------------------------------------------------------ */

typedef struct fl_ctx fl_ctx;       /* RenderManager + Framebuffers state (render.py:40-170,253-262) */
typedef struct fl_genome fl_genome; /* Renderer's compiled module + packer layout (render.py:225-251) */

int fl_abi_version(void);
const char *fl_last_error(void);

/* cuburn/render.py:79-89 Framebuffers.calc_dim */
void fl_calc_dim(uint32_t w, uint32_t h, fl_dim *out);

/* cuburn/render.py:253-262 RenderManager.__init__ + :91-104 Framebuffers.__init__:
 * device, streams, walker/RNG state (persistent across frames, render.py:95-104).
 * `seeds` = nseeds x {mul,state,carry} as built by make_seeds (mwc.py:30-47);
 * nseeds must be nslots * 64 * NW + FL_PAL_H * 256 + 65536, where NW = 4, 8 or 16 is the number of
 * waves per iterate workgroup (the table's size selects it): walkers, then the palette kernel's
 * states, then the output dither's.  nslots: a multiple of 256 in [1024, 16384] — one temporal sample per
 * slot — or 512 with NW = 8 / 256 with NW = 16: every four waves of a workgroup then walk a temporal sample of
 * their own (1024 in all, 256 walkers each: the reference's geometry, cuburn/render.py:207), sharing one sort batch.  stream = a hipStream_t to run everything on (single lane), or NULL:
 * the context then owns two streams and alternates consecutive frames between them so that the
 * drain / filter / output work of frame k overlaps the iteration of frame k+1
 * (cuburn/render.py:432-433 swaps stream_a / stream_b the same way). */
int fl_ctx_create(int device, void *stream, const fl_mwc *seeds, uint32_t nseeds, uint32_t nslots, fl_ctx **out);
void fl_ctx_destroy(fl_ctx *ctx);
int fl_ctx_sync(fl_ctx *ctx);

/* cuburn/render.py:232-251 Renderer.compile/load: takes the xform program (5) and the
 * interpolation op list (6) instead of generated source. */
int fl_genome_create(fl_ctx *ctx, const int32_t *prog, uint32_t nprog,
                     const int32_t *ops, uint32_t nops, uint32_t nrows, fl_genome **out);
void fl_genome_destroy(fl_genome *g);

/* cuburn/render.py:264-285 RenderManager._copy: upload packed splines and palettes.
 * times/knots: nrows x FL_KNOTS floats; pal_rgba: npal x 256 x 4 floats;
 * pal_times: FL_KNOTS floats padded 1e9. */
int fl_genome_upload(fl_ctx *ctx, fl_genome *g, const float *times, const float *knots,
                     const float *pal_rgba, const float *pal_times, uint32_t npal);

/* cuburn/render.py:289-307 RenderManager._interp: interp_palette_flat + interp_iter_params
 * for the frame window [ts, ts+td).  The reference evaluates 1024 temporal samples and runs one
 * block column per sample (grid (1024, n), render.py:343-346), so every sample gets the same number
 * of iterations.  Here the number of temporal samples equals the number of walker slots (twice that
 * / four times that for 512 slots of 8 waves / 256 of 16): block s (s < n) is evaluated at ts + s*td/n and iterated
 * by slot s (by sub-block s % k of slot s / k), palette row r (of 64) at ts + r*td/64 is used by slots
 * [r*nslots/64, (r+1)*nslots/64) — equal weights for any nslots. */
int fl_interp(fl_ctx *ctx, fl_genome *g, uint32_t w, uint32_t h, float ts, float td);

/* Accumulation back-ends for fl_iterate. */
enum {
    FL_ACCUM_ATOMIC = 0, /* 64-bit packed global atomics, as cuburn/code/iter.py:331-411 */
    FL_ACCUM_BINNED = 1  /* LDS-staged tile binning, then packed adds per tile          */
};

/* cuburn/render.py:316-372 RenderManager._iter: clears, fuse, iteration rounds, flushes.
 * nsamples = write-enabled chaos-game iterations requested (spp*w*h, render.py:331);
 * the count actually run (rounded up to whole launches) is returned in *nsamples_run.
 * fuse = write-disabled iterations per walker at frame start (reference: 256). */
int fl_iterate(fl_ctx *ctx, fl_genome *g, uint32_t w, uint32_t h, double nsamples,
               uint32_t fuse, int accum_mode, uint64_t *nsamples_run);

/* cuburn/filters.py:45-53,56-95,98-108,138-174 Filter.apply — one call per filter, result
 * left in the front buffer (filters.py:29-35).  params are the host-derived scalars. */
enum {
    FL_FILT_YUV = 0,       /* yuv_to_rgb       code/filters.py:71-77   params: none                 */
    FL_FILT_BILATERAL = 1, /* DE chain         filters.py:62-95        sstd,cstd,dstd,dpow,gspeed   */
    FL_FILT_LOGSCALE = 2,  /* logscale         code/filters.py:41-53   k1,k2                        */
    FL_FILT_COLORCLIP = 3, /* colorclip        code/filters.py:354-412 vib,highpow,gam,lin,lingam   */
    FL_FILT_SMEARCLIP = 4, /* smearclip chain  filters.py:142-163      width,gam_m_1,lin,lingam     */
    FL_FILT_HALOCLIP = 5,  /* haloclip chain   filters.py:113-130      gam_m_1                      */
    FL_FILT_PLAINCLIP = 6, /* plainclip        code/filters.py:332-350 gam_m_1,lin,lingam,brightness*/
    FL_FILT_LOGENCODE = 7, /* logencode        code/filters.py:81-90   degamma                      */
    FL_FILT_DE = 8,        /* adaptive DE      DESIGN.md §4 (flam3)    R,Rmin,curve (R <= 96, curve > 0) */
    FL_FILT_BLOOM = 9      /* Gaussian glare   DESIGN.md §4.18         threshold,strength,tap_0..tap_R (below) */
};
#define FL_DE_MAX_RADIUS 96    /* FL_FILT_DE: the largest R in px, and so the filter's reach */
/* FL_FILT_BLOOM: front += strength * blur(E), E = (w - threshold) / w * (r, g, b, w) where w > threshold and 0 elsewhere, blurred
 * along x then y over the whole padded buffer (sources outside it count as zero) with the symmetric kernel of 2R + 1 taps whose
 * centre and one side are tap_0 .. tap_R: nparams = 3 + R, R <= FL_BLOOM_MAX_REACH.  The taps are used as given (not renormalised).
 * FL_E_INVAL, before anything is queued: fewer than 3 parameters, R above the limit, a non-finite threshold, strength or tap, a
 * negative threshold.  Never part of a deferred chain: deferred steps run first. */
#define FL_BLOOM_MAX_REACH 384 /* FL_FILT_BLOOM: the largest R in bins (769 taps), and so the filter's reach */
int fl_filter(fl_ctx *ctx, int filter_id, uint32_t w, uint32_t h, const float *params, uint32_t nparams);

/* flam3's spatial filter + supersample decimation: front (laid out for ss*w x ss*h) -> front (laid out for w x h).
 * The reference has no such step (its accumulator has the output's size; cuburn/genome/convert.py:196 carries flam3's
 * `filter` radius as camera.dither_width and nothing reads it).  After flam3_create_spatial_filter, Gaussian shape only:
 * `taps` = ntaps weights t[0..ntaps-1] of a separable filter, ntaps in [ss, ss + 2 * FL_GUTTER] with ntaps - ss even,
 * g = (ntaps - ss) / 2 the source bins the footprint overhangs on either side.  For EVERY bin of the result's padded buffer,
 * 0 <= X < astride(w), 0 <= Y < ah(h):
 *     out[Y][X] = sum_j sum_i t[j] * t[i] * src[12 + ss*(Y-12) - g + j][12 + ss*(X-12) - g + i]
 * with source coordinates outside [0, astride(ss*w)) x [0, ah(ss*h)) contributing exactly zero (they are not read; the weights
 * are not renormalised), all four channels alike.  Inside the picture every tap is in range; the result's gutter fades to zero.
 * ss in 1..4; ss = 1 is the plain spatial filter.  Deferred filter steps (a `yuv`, the DE's end) run first, at the source's
 * size.  Recorded with the filters in fl_timings / fl_timings_detail[3].  FL_E_INVAL for anything else, non-finite taps included. */
#define FL_RESAMPLE_MAX_SS 4
#define FL_RESAMPLE_MAX_TAPS (FL_RESAMPLE_MAX_SS + 2 * FL_GUTTER)
int fl_resample(fl_ctx *ctx, uint32_t w, uint32_t h, uint32_t ss, const float *taps, uint32_t ntaps);

/* A downscale of the float frame to an arbitrary smaller size: front (laid out for w x h) -> front (laid out
 * for w2 x h2), w2 <= w, h2 <= h.  The filter is separable and arrives as one table per axis; the caller decides its shape
 * (filters.resize_tables: Lanczos-3 with Pillow's taps).  Output i of an axis with n_in source samples is the sum of nt source
 * samples from first[i] on, 0 <= first[i] and first[i] + nt <= n_in, weighted by taps[i][0 .. nt-1].  x first, then y:
 *     out[12 + Y][12 + X] = sum_j ytaps[Y][j] * (sum_i xtaps[X][i] * src[12 + yfirst[Y] + j][12 + xfirst[X] + i])
 * for 0 <= X < w2, 0 <= Y < h2, all four channels alike, the inner sum rounded to float32.  Only the source's picture area is
 * read, never its gutter or padding; every bin of the result's padded buffer outside its picture area is written as +0.
 * Nothing is clamped.  xtaps is [w2][nxt], ytaps is [h2][nyt]; the arrays are the caller's again when the call returns: the
 * lane keeps device copies of the tables of the last few (w, h, w2, h2) it has seen, found again by a hash of their contents.
 * Deferred filter steps (a `yuv`, the DE's end) run first, at the source's size.  Recorded with the filters in fl_timings /
 * fl_timings_detail[3].
 * FL_E_INVAL, before anything is queued or timed: a null pointer or a zero size, w2 > w or h2 > h, nxt or nyt outside
 * 1 .. FL_RESIZE_MAX_TAPS or above the source's size, a first below 0 or with first + nt past the source, a non-finite tap,
 * x windows that are not a downscale's: those of 64 neighbouring output columns span more than 576 source bins (ratio 8, the
 * largest FL_RESIZE_MAX_TAPS serves, spans 555). */
#define FL_RESIZE_MAX_TAPS 50
int fl_resize(fl_ctx *ctx, uint32_t w, uint32_t h, uint32_t w2, uint32_t h2,
              const int32_t *xfirst, const float *xtaps, uint32_t nxt,
              const int32_t *yfirst, const float *ytaps, uint32_t nyt);

/* cuburn/output.py:83-88,120-125,150-158,212-219,323-338 (convert + copy of every Output class):
 * f32 -> pixel format with dither (cuburn/code/output.py:7-236), gutter cropped; async D2H into
 * host_out (or device copy when dev_out != 0).  fl_output_bytes gives the frame's size. */
enum {
    FL_OUT_RGBA8 = 0,     /* f32_to_rgba_u8    code/output.py:20-44    u8  [h][w][4]                        */
    FL_OUT_RGBA16 = 1,    /* f32_to_rgba_u16   code/output.py:47-71    u16 [h][w][4]                        */
    FL_OUT_YUV444P = 2,   /* f32_to_yuv444p    code/output.py:75-102   u8  [3][h][w], JPEG full range       */
    FL_OUT_YUV444P10 = 3, /* f32_to_yuv444p10  code/output.py:106-134  u16 [3][h][w], peak 1023             */
    FL_OUT_YUV420P10 = 4, /* f32_to_yuv420p10  code/output.py:138-190  u16 Y[h][w] Cb[h/2][w/2] Cr[h/2][w/2]; w, h even */
    FL_OUT_YUV444P12 = 5  /* f32_to_yuv444p12  code/output.py:194-221  u16 [3][h][w], Rec.709 studio swing  */
};
size_t fl_output_bytes(uint32_t w, uint32_t h, int fmt);   /* 0 for an unknown format */
int fl_output(fl_ctx *ctx, uint32_t w, uint32_t h, int fmt, void *host_out, uint64_t dev_out);

/* Baseline JPEG stills encoded on the device: SOF0, 8 bit, JFIF 1.01, components 1, 2, 3 = Y, Cb, Cr all sampled
 * 1x1 in one interleaved scan, the Huffman tables of ITU T.81 Annex K.3-K.6, the quantisation tables of Annex K.1 / K.2 scaled
 * the libjpeg way for quality 1..100 (100: all ones), restart intervals (DRI) of a length the library chooses.  Partial blocks
 * replicate the last column / row.  The same planes, quality and size give the same bytes.
 * The result, in host_out and / or at dev_out (capacity `cap` bytes each): a 16-byte record u32 nbytes, u32 status,
 * u32 restart_interval, u32 0, and behind it the stream.  status 0: the nbytes bytes behind the record are the file.  status 1:
 * the file needs nbytes bytes and cap - 16 is less; nothing behind the record is valid.  No byte at or beyond cap is touched.
 * A host_out from fl_host_alloc (any pinned memory) is written by the kernels themselves, so that only the record and nbytes bytes
 * cross the bus; other host memory receives an asynchronous copy of min(cap, fl_jpeg_bound) bytes.
 * fl_jpeg_bound: what no stream of that size can exceed, record and header included (0 for w or h of 0 or above 65535).
 * fl_jpeg_encode: src_dev = u8 [3][h][w] as FL_OUT_YUV444P writes them; queued on the current lane's stream.
 * fl_output_jpeg: fl_output(FL_OUT_YUV444P) into the lane's pixel buffer (same draws, same dither states afterwards), then the
 * encode; closes the frame as fl_output does.
 * FL_E_INVAL, before anything is queued: quality outside 1..100, w or h of 0 or above 65535, a null src_dev,
 * cap < 16 + FL_JPEG_HEADER_BYTES, host_out and dev_out both null. */
#define FL_JPEG_HEADER_BYTES 629   /* SOI, APP0, DQT x2, SOF0, DHT x4, DRI, SOS */
size_t fl_jpeg_bound(uint32_t w, uint32_t h);
int fl_jpeg_encode(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, int quality, void *host_out, uint64_t dev_out, size_t cap);
int fl_output_jpeg(fl_ctx *ctx, uint32_t w, uint32_t h, int quality, void *host_out, uint64_t dev_out, size_t cap);

/* The same with the chroma sampling chosen.  FL_JPEG_444: the three entry points above, byte for byte.
 * FL_JPEG_420: SOF0 declares Y as 2x2 and Cb, Cr as 1x1; an MCU covers 16x16 pixels and holds six blocks, Y00 Y01 Y10 Y11 Cb Cr.
 * The source is still the full-resolution planes of FL_OUT_YUV444P (fl_output_jpeg_s makes the draws of fl_output_jpeg and
 * leaves the same dither states): the encoder takes each chroma sample as (a + b + c + d + 2) >> 2 over its 2x2 full-resolution
 * samples, whose coordinates are clamped to w - 1, h - 1 first, so odd sizes and partial MCUs replicate the last column / row
 * before the average.  The Y predictor runs through the four Y blocks of an MCU and on into the next MCU; all three restart
 * with every interval.  The header keeps its FL_JPEG_HEADER_BYTES bytes; the record is the same.
 * fl_jpeg_bound_s: 0 as fl_jpeg_bound, and for an unknown sampling.  Any other call with an unknown sampling is FL_E_INVAL. */
enum { FL_JPEG_444 = 0, FL_JPEG_420 = 1 };
size_t fl_jpeg_bound_s(uint32_t w, uint32_t h, int sampling);
int fl_jpeg_encode_s(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, int quality, int sampling,
                     void *host_out, uint64_t dev_out, size_t cap);
int fl_output_jpeg_s(fl_ctx *ctx, uint32_t w, uint32_t h, int quality, int sampling,
                     void *host_out, uint64_t dev_out, size_t cap);

/* The same with flags.  flags = 0: the three entry points above, byte for byte.
 * FL_JPEG_OPTIMIZE: the same coefficients coded with Huffman tables built from the frame's own symbol counts (libjpeg's
 * "optimize"), on the device and on the lane's stream.  The header keeps its FL_JPEG_HEADER_BYTES bytes and its marker order:
 * only BITS / HUFFVAL inside the four DHT segments and the scan's bits differ.  Every table lists all its legal symbols (DC:
 * the categories 0..11; AC: 0x00, 0xF0 and run 0..15 x size 1..10), used or not.  For each table count[s] is how often the
 * scan emits s; freq[s] = 2 * count[s] + 2, and 1 for one pseudo-symbol behind the alphabet, which therefore takes a longest
 * code and keeps the all-ones codeword unassigned; the lengths are Huffman's for those frequencies (ranked by (frequency, symbol),
 * a tie between a leaf and an inner node takes the leaf), cut at 16 bits with the Kraft sum repaired, the rarest symbols taking
 * the longest codes; HUFFVAL orders the legal symbols by (length, symbol) and the codes follow T.81 Annex C.  A table that
 * does not cost the frame fewer code bits (sum count * length) than the Annex K table of its kind is that Annex K table, which
 * obeys the same rules: on a frame of a few symbols all four can be, and the file is then the file of flags = 0.  The same planes,
 * quality and size give the same bytes.  The record is the same.
 * fl_jpeg_bound_f: with FL_JPEG_OPTIMIZE a DC code can take 12 bits, so 4:2:0 allows 2494 bytes per MCU (4:4:4: 1248 as before);
 * 0 as fl_jpeg_bound_s, for an unknown flag bit, and with FL_JPEG_OPTIMIZE for a frame of more than 2^24 blocks (the counts must
 * fit 32-bit sums).  Any other call is FL_E_INVAL for an unknown flag bit and FL_E_UNSUPPORTED for such a frame, after every
 * refusal of the entry points above and before anything is queued. */
enum { FL_JPEG_OPTIMIZE = 1 };
size_t fl_jpeg_bound_f(uint32_t w, uint32_t h, int sampling, unsigned flags);
int fl_jpeg_encode_f(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, int quality, int sampling, unsigned flags,
                     void *host_out, uint64_t dev_out, size_t cap);
int fl_output_jpeg_f(fl_ctx *ctx, uint32_t w, uint32_t h, int quality, int sampling, unsigned flags,
                     void *host_out, uint64_t dev_out, size_t cap);

/* PNG stills encoded on the device: 8-bit truecolour (16-bit, and a filter type per row: the _f entry points
 * below), colour type 2 (channels 3) or 6 (channels 4), not interlaced:
 * the signature, IHDR, one IDAT per segment, IEND; no ancillary chunk.  The IDATs hold one zlib stream (header 78 01, deflate
 * blocks, Adler-32).  Every row is filtered with Paeth (filter byte 4).  The filtered bytes are cut into segments of segment_bytes
 * bytes (the library's choice; the last may be shorter), each coded with no reference before its own start as one block: dynamic
 * Huffman (type 2) holding literals and matches of distance 1 and length 3..258, code lengths limited to 15 (7 for the code-length
 * code), or stored (type 0) whenever the dynamic form would not be smaller.  Every segment but the last ends on a byte boundary
 * (an empty stored block behind a dynamic one); only the last block has BFINAL set.  CRC-32s and Adler-32 are computed on the
 * device.  The same pixels, size and channel count give the same bytes.
 * The result, in host_out and / or at dev_out (capacity `cap` bytes each): a 16-byte record u32 nbytes, u32 status,
 * u32 segment_bytes, u32 0, and behind it the file.  status 0: the nbytes bytes behind the record are the file.  status 1: the
 * file needs nbytes bytes and cap - 16 is less; nothing behind the record is valid.  No byte at or beyond cap is touched.
 * A host_out from fl_host_alloc (any pinned memory) is written by the kernels themselves; other host memory receives an
 * asynchronous copy of min(cap, fl_png_bound) bytes.
 * fl_png_bound: the all-stored worst case — record, header, 17 bytes per segment (5 of the stored block, 12 of the IDAT), the
 * zlib header and Adler-32, IEND; 0 for w or h of 0 or above 65535, channels other than 3 or 4, or a result beyond 2^32 - 1.
 * fl_png_encode: src_dev = u8 [h][w][4] as FL_OUT_RGBA8 writes them (channels 3 leaves the alpha byte out of the file); queued on
 * the current lane's stream.
 * fl_output_png: fl_output(FL_OUT_RGBA8) into the lane's pixel buffer (same draws, same dither states afterwards), then the
 * encode; closes the frame as fl_output does.
 * FL_E_INVAL, before anything is queued: channels other than 3 or 4, w or h of 0 or above 65535, a frame whose fl_png_bound is 0,
 * a null src_dev, cap < 16 + FL_PNG_HEADER_BYTES, host_out and dev_out both null. */
#define FL_PNG_HEADER_BYTES 33            /* signature + IHDR */
size_t fl_png_bound(uint32_t w, uint32_t h, int channels);
int fl_png_encode(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, int channels, void *host_out, uint64_t dev_out, size_t cap);
int fl_output_png(fl_ctx *ctx, uint32_t w, uint32_t h, int channels, void *host_out, uint64_t dev_out, size_t cap);

/* The same with a sample depth and flags.  bits = 8, flags = 0: the three entry points above, byte for byte.
 * With bpp = channels * bits / 8 (3, 4, 6 or 8): IHDR's bit depth is `bits`; a row of the filtered stream is one filter byte
 * and w * bpp residual bytes; all five PNG filters work on bytes at distance bpp (a and c are 0 for a row's first bpp bytes, b
 * and c are 0 in row 0).  Everything else of the file is as above.
 * bits = 16: the source is u16 [h][w][4] as FL_OUT_RGBA16 writes them, in native byte order (channels 3 leaves the alpha
 * sample out); the file holds each sample most significant byte first.
 * FL_PNG_ADAPTIVE: every row takes the filter type t in 0..4 (None, Sub, Up, Average with floor((a + b) / 2), Paeth) whose
 * cost — the sum over the row's residual bytes r of min(r, 256 - r) — is least, the smallest such t on a tie (libpng's
 * minimum sum of absolute differences).  Without the flag every row is type 4.
 * The same pixels, size, channels, bits and flags give the same bytes.  The record is the same.
 * fl_png_bound_f: fl_png_bound with rows of 1 + w * bpp bytes; 0 as fl_png_bound, for bits other than 8 or 16, for an unknown
 * flag bit and for a result beyond 2^32 - 1.
 * fl_output_png_f with bits = 16: fl_output(FL_OUT_RGBA16) into the lane's pixel buffer (same draws, same dither states
 * afterwards), then the encode; closes the frame as fl_output does.
 * Any other call is FL_E_INVAL for bits other than 8 or 16, an unknown flag bit or a frame whose fl_png_bound_f is 0, after
 * every refusal of the entry points above and before anything is queued. */
enum { FL_PNG_ADAPTIVE = 1 };
size_t fl_png_bound_f(uint32_t w, uint32_t h, int channels, int bits, unsigned flags);
int fl_png_encode_f(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, int channels, int bits, unsigned flags,
                    void *host_out, uint64_t dev_out, size_t cap);
int fl_output_png_f(fl_ctx *ctx, uint32_t w, uint32_t h, int channels, int bits, unsigned flags,
                    void *host_out, uint64_t dev_out, size_t cap);

/* Animations as APNG: one frame's chunks, encoded on the device.  A frame block is the chunks of one frame and
 * nothing else — no signature, no IHDR, no IEND —, one chunk per segment of the frame's own zlib stream, as the PNG encoder above
 * cuts, codes and checksums it for the same pixels, size, channels, bits and flags.
 * seq == FL_APNG_IDAT: the chunks are the IDATs of fl_png_encode_f's file, byte for byte (its bytes from offset 33 up to the 12
 * of IEND): the frame that a reader which knows no animation shows.
 * Any other seq: chunk i (from 0) is an fdAT.  Its length field is dlen + 4 and its data is seq + i as four bytes, most significant
 * first, then the dlen bytes of IDAT i (the first chunk holds the zlib header, the last the Adler-32); its CRC-32, computed on the
 * device, covers the tag, the number and the data.
 * The record is the PNG encoder's with its fourth word used: u32 nbytes, u32 status, u32 segment_bytes, u32 nchunks; status, the
 * capacity rule and the destinations are the PNG encoder's, with cap >= 16.  The file around the blocks — signature, IHDR, acTL,
 * an fcTL in front of every block, IEND — is the host's (cuburn_amd/encoders.py, APNGOutput).
 * fl_apng_chunks: the chunks of a frame, ceil(h * (1 + w * channels * bits / 8) / segment_bytes): the same for every frame of a
 * shape in a process, so the next frame's numbers are known before this one has finished; 0 where fl_png_bound_f is 0.
 * fl_apng_bound: fl_png_bound_f - 33 - 12 + 4 * fl_apng_chunks (every chunk an fdAT); 0 where fl_png_bound_f is 0.
 * fl_apng_encode: the source and flags of fl_png_encode_f; queued on the current lane's stream.
 * fl_output_apng: the conversion, draws and dither states of fl_output_png_f, then the encode; closes the frame as fl_output does.
 * FL_E_INVAL, before anything is queued: every refusal of fl_png_encode_f (with cap < 16 in place of its capacity rule), and a
 * seq other than FL_APNG_IDAT whose last number, seq + fl_apng_chunks - 1, would pass 0xfffffffe. */
enum { FL_APNG_IDAT = 0xffffffffu };
uint32_t fl_apng_chunks(uint32_t w, uint32_t h, int channels, int bits);
size_t fl_apng_bound(uint32_t w, uint32_t h, int channels, int bits, unsigned flags);
int fl_apng_encode(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, int channels, int bits, unsigned flags, uint32_t seq,
                   void *host_out, uint64_t dev_out, size_t cap);
int fl_output_apng(fl_ctx *ctx, uint32_t w, uint32_t h, int channels, int bits, unsigned flags, uint32_t seq,
                   void *host_out, uint64_t dev_out, size_t cap);

/* TIFF stills encoded on the device: classic little-endian TIFF with one IFD, tiled; Compression 8 (Adobe
 * deflate), Predictor 2, PlanarConfiguration 1, Photometric 2; samples of `bits` = 8 or 16, `channels` = 3 or 4 (4 adds
 * ExtraSamples = 2, unassociated alpha).  TileLength is 64, TileWidth 128 at 8 bits and 64 at 16: a tile holds
 * TileWidth * 64 * channels * bits / 8 = 24576 or 32768 bytes.  Tiles run row-major, nt = ceil(w / TileWidth) * ceil(h / 64)
 * of them; a tile sample at (x, y) outside the image is the source sample at (min(x, w - 1), min(y, h - 1)).  Within a tile
 * row the first pixel is stored as is and every later sample is (s[x] - s[x - 1]) mod 2^bits against the same channel of the pixel
 * to its left in the tile (16-bit word arithmetic at 16 bits); 16-bit values are stored low byte first.
 * The source is u8 / u16 [h][w][4] as FL_OUT_RGBA8 / FL_OUT_RGBA16 write them (channels 3 leaves the alpha sample out).
 * A tile's data: 78 01, one deflate block with BFINAL set — dynamic Huffman holding literals and matches of distance 1, coded as
 * the PNG encoder codes a last segment, or stored when the dynamic form would not be smaller —, then the Adler-32 of the tile's
 * predicted bytes, most significant byte first.  Tiles share no history.
 * The file: bytes 0..7 (II, 42, 8); the entry count, the entries in ascending tag order (256 ImageWidth, 257 ImageLength,
 * 258 BitsPerSample, 259 Compression, 262 Photometric, 277 SamplesPerPixel, 284 PlanarConfiguration, 317 Predictor, 322 TileWidth,
 * 323 TileLength, 324 TileOffsets, 325 TileByteCounts, and 338 ExtraSamples with channels 4; widths, lengths, offsets and counts
 * are LONGs, the rest SHORTs) and a next-IFD of 0; the BitsPerSample array; only when nt > 1 TileOffsets and TileByteCounts, nt
 * LONGs each (with nt = 1 both values sit in their entries); the tiles in order, each at an even offset: one zero byte follows
 * a tile of odd length, except the last.  The same pixels, size, channels and bits give the same bytes.
 * The result, in host_out and / or at dev_out (capacity `cap` bytes each): a 16-byte record u32 nbytes, u32 status, u32 the
 * bytes of a tile, u32 0, and behind it the file; status, the capacity rule and the destinations are the PNG encoder's.
 * fl_tiff_bound: the all-stored worst case — 16 for the record, H, and nt * (tile bytes + 5 + 6 + 1), where the header H is
 * 8 + 2 + 12 * entries + 4 + 2 * channels, plus 8 * nt when nt > 1; 0 for w or h of 0 or above 65535, channels other than 3 or
 * 4, bits other than 8 or 16, or a result beyond 2^32 - 1.
 * fl_tiff_encode: queued on the current lane's stream.
 * fl_output_tiff: fl_output(FL_OUT_RGBA16), or FL_OUT_RGBA8 for bits = 8, into the lane's pixel buffer (same draws, same dither
 * states afterwards), then the encode; closes the frame as fl_output does.
 * FL_E_INVAL, before anything is queued: any case in which fl_tiff_bound is 0, a null src_dev, host_out and dev_out both null,
 * cap < 16 + H. */
size_t fl_tiff_bound(uint32_t w, uint32_t h, int channels, int bits);
int fl_tiff_encode(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, int channels, int bits,
                   void *host_out, uint64_t dev_out, size_t cap);
int fl_output_tiff(fl_ctx *ctx, uint32_t w, uint32_t h, int channels, int bits, void *host_out, uint64_t dev_out, size_t cap);

/* OpenEXR stills encoded on the device: the float picture itself, not a display integer.  Single part, tiled,
 * one level, little-endian throughout; integers are 32-bit unless stated.
 * Bytes 0..7: 76 2f 31 01, then the version word 0x00000202 (version 2, the tiled bit 0x200).
 * The header: attributes `name\0 type\0 size value` in this order, then a single 00:
 *   channels / chlist: per channel in alphabetical order (A only with channels = 4, then B, G, R) name\0, the pixel type (1 HALF,
 *     2 FLOAT), pLinear u8 = 0, three zero bytes, xSampling 1, ySampling 1; a 00 ends the list (18 bytes a channel, and 1);
 *   compression / compression: one byte, 3 (ZIP);  dataWindow / box2i: 0, 0, w - 1, h - 1;  displayWindow / box2i: the same;
 *   lineOrder / lineOrder: one byte, 0 (increasing Y);  pixelAspectRatio / float: 1.0;  screenWindowCenter / v2f: 0.0, 0.0;
 *   screenWindowWidth / float: 1.0;  tiles / tiledesc: xSize u32 = 64, ySize u32 = TH, a mode byte 0 (one level, round down).
 *   That is 341 bytes with 3 channels and 359 with 4.
 * Tiles are 64 pixels wide and TH = 64 (HALF) or 32 (FLOAT) rows high: a full tile is 8192 * channels bytes at either depth.
 * nx = ceil(w / 64), ny = ceil(h / TH), nt = nx * ny.  Tile (tx, ty) covers columns 64 tx .. and rows TH ty .., cropped to the
 * image: tw = min(64, w - 64 tx) wide, th = min(TH, h - TH ty) high.  Nothing is padded.
 * Behind the header the offset table: nt u64, ty-major, the position in the file of each tile's chunk.  Then the chunks in the
 * same order with nothing between them: tileX, tileY, levelX = 0, levelY = 0, dataSize, and dataSize bytes.
 * A tile's raw bytes (n = th * tw * channels * bytes per sample): row by row; within a row channel by channel in the chlist's
 * order; within a channel the tw samples, low byte first.  R, G, B, A are .x, .y, .z, .w of the source's float4.
 * A tile's data is the smaller of (a) a zlib stream 78 01, one final deflate block coded as the TIFF encoder codes a tile, and the
 * Adler-32 of the block's input, most significant byte first, where that input d is the raw bytes after OpenEXR's two steps —
 * t = the even-indexed raw bytes followed by the odd-indexed ones; d[0] = t[0], d[i] = (t[i] - t[i-1] + 128) mod 256 — and (b),
 * whenever 2 + block + 4 >= n, the n raw bytes as they are.  A reader tells them apart by dataSize < n.
 * Samples.  FLOAT: the source's 32 bits (NaN, infinities and denormals kept).  HALF: finite values rounded to nearest, ties to
 * even, with gradual underflow; |x| >= 65520 and the infinities become +-65504 (7bff / fbff); NaN becomes 0000; -0 stays 8000.
 * The same samples, size, channels and pixel type give the same bytes.
 * The result, in host_out and / or at dev_out (capacity `cap` bytes each): a 16-byte record u32 nbytes, u32 status, u32
 * 8192 * channels, u32 0, and behind it the file; status, the capacity rule and the destinations are the PNG encoder's.
 * fl_exr_bound: every tile raw, which is exact for such a file — 16 + the header + 28 * nt + w * h * channels * bytes per
 * sample; 0 for w or h of 0 or above 65535, channels other than 3 or 4, an unknown pixel type, or a result beyond 2^32 - 1.
 * fl_exr_encode: src_dev = f32 [h][src_stride][4], src_stride in pixels and at least w; queued on the current lane's stream.
 * fl_output_exr: the lane's front buffer as the filter chain left it, read in place (FL_GUTTER rows and columns in), after the
 * deferred ends of the chain have run.  It draws no dither: the output RNG states stay as they are.  Closes the frame as
 * fl_output does.
 * FL_E_INVAL, before anything is queued: any case in which fl_exr_bound is 0, a null src_dev, src_stride < w, host_out and
 * dev_out both null, cap < 16 + the header + 8 * nt. */
enum { FL_EXR_HALF = 1, FL_EXR_FLOAT = 2 };
size_t fl_exr_bound(uint32_t w, uint32_t h, int channels, int pixel);
int fl_exr_encode(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, uint32_t src_stride, int channels, int pixel,
                  void *host_out, uint64_t dev_out, size_t cap);
int fl_output_exr(fl_ctx *ctx, uint32_t w, uint32_t h, int channels, int pixel, void *host_out, uint64_t dev_out, size_t cap);

/* GIF frames encoded on the device: one frame block with a palette of its own; the host writes the file around
 * the blocks (cuburn_amd/encoders.py, GIFOutput).  All arithmetic is integer arithmetic.
 * The source is u8 [h][w][4] as FL_OUT_RGBA8 writes them; the alpha byte is ignored.  w and h are 1..65535 and w * h <= 2^24, so
 * that a cell's channel sum fits 32 bits.
 * Histogram: a pixel's cell is (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3), 32768 cells; every cell keeps its pixel count and the
 * exact sums of r, g and b.
 * Median cut by population: box 0 holds every non-empty cell, nb = 1.  While nb < colors: among the boxes of more than one
 * non-empty cell the one of most pixels (a tie: the lowest index; none: stop); its axis is the one of largest extent, max - min of
 * the 5-bit coordinate over its non-empty cells (a tie: R, then G, then B); with pop the box's pixels and cum[c] those of
 * coordinate <= c on that axis, c is the smallest coordinate with 2 * cum[c] >= pop, clamped into [min, max - 1]; the cells of
 * coordinate > c become box nb, and nb += 1.
 * Palette: entry b is (sum + count / 2) / count per channel over box b; entries nb..255 are 0, 0, 0.  The local colour table always
 * has 256 entries and the LZW minimum code size is always 8.
 * Lookup: a non-empty cell's point is its own rounded mean (sum + count / 2) / count, an empty cell's its centre 8 * coord + 4;
 * the cell maps to the entry among 0..nb-1 of least squared distance to that point, the lowest index on a tie.
 * Dither: with B the 8 x 8 Bayer matrix (rows 0 32 8 40 2 34 10 42 / 48 16 56 24 50 18 58 26 / 12 44 4 36 14 46 6 38 /
 * 60 28 52 20 62 30 54 22 / 3 35 11 43 1 33 9 41 / 51 19 59 27 49 17 57 25 / 15 47 7 39 13 45 5 37 / 63 31 55 23 61 29 53 21)
 * and d = 2 * B[y & 7][x & 7] + 1 - 64, every channel becomes clamp(p + ((d * dither_amp) >> 7), 0, 255), the shift arithmetic;
 * the pixel's index is the lookup of the dithered value's cell.  Histogram and palette are taken from the undithered pixels.
 * LZW: the indices in raster order in segments of S pixels (the library's choice, FL_GIF_SEG = 1024 unless FLAME_GIF_SEG = 256..3584
 * was set when the context was created; the last may be shorter), codes packed least significant bit first.  Per segment:
 * width = 9, next = 258, CLEAR (256) in 9 bits; p = the first index; for every later index c: if the string (p, c) is in the
 * dictionary p becomes its code, otherwise p is emitted in width bits, (p, c) becomes code next, next += 1, width += 1 if
 * next > 1 << width and width < 12, and p = c.  After the last index p is emitted, then next += 1 and the width step once more
 * (the entry the decoder adds).  The last segment then emits END (257) in width bits and pads with zero bits to a byte; every
 * other one emits CLEAR in width bits and then CLEARs of 9 bits until the bit count is a multiple of 8.
 * The block: 2C, left 0, top 0, w, h as u16 little-endian, 87, the 768 palette bytes, 08 (FL_GIF_HEADER_BYTES so far), the
 * segments' bytes in sub-blocks — stream byte j at j + j / 255 + 1 behind the 08, a length byte min(255, total - 255 g) in front
 * of every 255 bytes —, 00.  The same pixels, size, colors, dither_amp and S give the same bytes.
 * The result, in host_out and / or at dev_out (capacity `cap` bytes each): a 16-byte record u32 nbytes, u32 status, u32 S, u32 0,
 * and behind it the block; status, the capacity rule and the destinations are the PNG encoder's.
 * fl_gif_bound: 16 + FL_GIF_HEADER_BYTES + T + ceil(T / 255) + 1 with T = ceil(3 n / 2) + 11 * ceil(n / 256), n = w * h: twelve
 * bits a pixel and 84 bits of framing a segment at the shortest S; 0 for w or h of 0 or above 65535 and for w * h > 2^24.
 * fl_gif_encode: queued on the current lane's stream.
 * fl_output_gif: fl_output(FL_OUT_RGBA8) into the lane's pixel buffer (same draws, same dither states afterwards), then the
 * encode; closes the frame as fl_output does.
 * FL_E_INVAL, before anything is queued: colors outside 2..256, dither_amp outside 0..64, a frame whose fl_gif_bound is 0, a null
 * src_dev, host_out and dev_out both null, cap < 16 + FL_GIF_HEADER_BYTES. */
#define FL_GIF_HEADER_BYTES 779           /* 2C, the descriptor, the colour table, the code size */
size_t fl_gif_bound(uint32_t w, uint32_t h);
int fl_gif_encode(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, int colors, int dither_amp,
                  void *host_out, uint64_t dev_out, size_t cap);
int fl_output_gif(fl_ctx *ctx, uint32_t w, uint32_t h, int colors, int dither_amp, void *host_out, uint64_t dev_out, size_t cap);

/* Lossless WebP frames encoded on the device: one frame block, a complete RIFF chunk `VP8L`, u32 payload length,
 * the payload, one zero byte if the length is odd; the host writes it verbatim into a still's or an animation's container
 * (cuburn_amd/encoders.py, WebPOutput).  All arithmetic is integer arithmetic.
 * The source is u8 [h][w][4] as FL_OUT_RGBA8 writes them, src_dev 4-byte aligned (a pixel is read as one word).  w and h are
 * 1..16384.  channels 3 reads every alpha as 255, channels 4 keeps alpha.  Bits are packed least significant first; prefix codes are canonical, as deflate's, and written bit-reversed.
 * The payload, in order: byte 2F; w - 1 and h - 1 in 14 bits each; alpha_is_used = (channels == 4); version 0 in 3 bits.
 * Transform present (1), type 2 (subtract green) in 2 bits: r and b become (r - g) mod 256 and (b - g) mod 256.  Transform present
 * (1), type 0 (predictor), the size field PB - 2 in 3 bits with PB = FL_WEBP_PB = 4 (16 x 16 tiles), then the mode sub-image of
 * ceil(w / 16) x ceil(h / 16) pixels, green = the tile's mode, red = blue = 0, alpha = 255.  No further transform (0), no colour
 * cache (0).  Meta prefix codes present (1), the size field EB - 2 in 3 bits with EB = FL_WEBP_EB = 6 (64 x 64 tiles), then the
 * entropy sub-image of ceil(w / 64) x ceil(h / 64) pixels: pixel i in raster order names group i, green = i & 255, red = i >> 8,
 * blue 0, alpha 255 (G = ceil(w / 64) * ceil(h / 64) groups, at most 65536; the bit is written even when G = 1).  Per group, in
 * order, five prefix codes: green (alphabet 280), red, blue, alpha (256 each), distance (40), built from the counts of that
 * tile's residuals (the distance code from no counts).  Then the pixels in raster order, each as its green, red, blue and alpha
 * symbol in the codes of its tile's group; a code of one symbol emits no bits.  Zero bits to the next byte.
 * Each sub-image is an entropy-coded image of its own: cache bit 0, one group of five codes from its own counts, its pixels.
 * Predictor: it works on the green-subtracted picture, never on residuals; the residual is (pixel - prediction) mod 256 per
 * channel.  Whatever the mode, (0, 0) is predicted as r, g, b, a = 0, 0, 0, 255, the rest of row 0 as L and the rest of column 0
 * as T.  TR of the last column is pixel (0, y) of the current row.  With avg2(a, b) = floor((a + b) / 2) per channel the modes
 * are 1: L; 2: T; 7: avg2(L, T); 10: avg2(avg2(L, TL), avg2(T, TR)); 11 (select): with e = L + T - TL per channel, signed, and
 * dL, dT the sums over the four channels of |e - L| and |e - T|, L if dL < dT, else T; 12: clamp(L + T - TL, 0, 255) per channel.
 * A tile takes the mode among {1, 2, 7, 10, 11, 12} of least cost, the lowest on a tie; the cost is the sum over the tile's
 * pixels inside the image and the four channels of min(r, 256 - r) of the residuals r the mode would give, fixed rules applied
 * (the measure of FL_PNG_ADAPTIVE).
 * Every prefix code, the sub-images' included: with at most one used symbol s (0 if none) the simple form, bits 1, 0,
 * is_first_8bits = (s > 1), s in 1 or 8 bits.  Otherwise bit 0 and the normal form: lengths limited to 15 — Huffman's (ties: the
 * lower count, then the lower symbol, leaves before inner nodes), depths cut at 15, Kraft's sum repaired by lengthening the
 * deepest code that can be, the rarest symbols longest.  The lengths 0 .. last used become tokens: a non-zero length is a
 * literal; a run of zeros takes 18 (11..138, 7 extra bits) while at least 11 remain, then 17 (3..10, 3 extra bits), then one or
 * two literal 0s; 16 is never used.  The token kinds get lengths by the same rule with limit 7; a lone kind gets one bit and so
 * does kind 0 (kind 1, if the lone kind is 0).  Written: num_code_lengths - 4 in 4 bits (at least 4, up to the last non-zero in
 * the order 17 18 0 1 2 3 4 5 16 6 7 8 9 10 11 12 13 14 15), those lengths in 3 bits each, bit 1, k - 1 in 3 bits and
 * ntokens - 2 in 2 k bits with k = max(1, ceil(bitlength(ntokens - 2) / 2)), then the tokens with their extra bits.
 * The same pixels, size and channels give the same bytes.
 * The result, in host_out and / or at dev_out (capacity `cap` bytes each): a 16-byte record u32 nbytes, u32 status,
 * u32 PB | EB << 8, u32 0, and behind it the block; status, the capacity rule and the destinations are the PNG encoder's (with
 * status 1 the record alone is written).
 * fl_webp_bound: 16 + 8 + ceil(B / 8) + 1 with B = 49 + (1 + Hg + 60 pt) + 6 + (1 + Hg + 60 G) + G Hg + 60 w h,
 * pt = ceil(w / 16) ceil(h / 16).  The proof: no code is longer than 15 bits, so a pixel of any image is at most 60; the fixed
 * fields are 49 bits in front of the mode sub-image and 6 between the sub-images, and each sub-image begins with its cache bit.
 * A normal code's header is 1 + 4 + 19 * 3 + 1 + 3 + 10 = 76 bits and its tokens: at most 256 of them (the last used symbol is
 * at most 255 in every image here, and no token stands for less than one length), each a code of at most 7 bits and at most 7
 * extra bits; the simple form is shorter; so Hc = 76 + 256 * 14 = 3660 and a group of four such codes and the distance code's
 * 4 bits is Hg = 4 Hc + 4.  The padding (at most 7 bits) is in the ceil, the chunk's pad byte is the + 1.  0 for w or h of 0 or
 * above 16384, channels other than 3 or 4, or a result beyond 2^32 - 1.
 * fl_webp_encode: queued on the current lane's stream.
 * fl_output_webp: fl_output(FL_OUT_RGBA8) into the lane's pixel buffer (same draws, same dither states afterwards), then the
 * encode; closes the frame as fl_output does.
 * FL_E_INVAL, before anything is queued: channels other than 3 or 4, w or h above 16384, a null src_dev, host_out and dev_out
 * both null, cap < 16 + FL_WEBP_HEADER_BYTES. */
#define FL_WEBP_PB 4                      /* predictor tiles of 16 x 16 pixels */
#define FL_WEBP_EB 6                      /* entropy tiles of 64 x 64 pixels */
#define FL_WEBP_HEADER_BYTES 8            /* `VP8L` and the payload's length */
size_t fl_webp_bound(uint32_t w, uint32_t h, int channels);
int fl_webp_encode(fl_ctx *ctx, uint32_t w, uint32_t h, uint64_t src_dev, int channels, void *host_out, uint64_t dev_out, size_t cap);
int fl_output_webp(fl_ctx *ctx, uint32_t w, uint32_t h, int channels, void *host_out, uint64_t dev_out, size_t cap);

/* cuburn/code/sort.py:443-504 Sorter.sort: one radix pass over n 32-bit keys on the device —
 * dst = src ordered by the `nbits` (1..10) bits from lo_bit up, keys with equal digits in their
 * original order (stable: passes from the low digit up compose into a full sort; the reference's
 * pass is not stable and its multi-pass sort is marked broken, sort.py:437-441,455-458).
 * ignore_max: keys equal to 0xffffffff are dropped (sort.py:449-452); *nvalid (optional, makes the
 * call synchronous) receives the number of keys written.  dst and src are device addresses and must
 * not overlap; every pass runs on the context's FIRST stream (the caller's, if one was given to
 * fl_ctx_create), so consecutive passes are ordered.  Not used by the render path — like
 * the reference's sorter (imported by render.py:19, never called). */
int fl_sort_u32(fl_ctx *ctx, uint64_t dst_dev, uint64_t src_dev, uint32_t n, uint32_t lo_bit, uint32_t nbits, int ignore_max,
                uint32_t *nvalid);

/* cuburn/render.py:404,430 timing_event / DurationEvent: fl_frame_begin opens a frame and returns
 * its id; fl_output closes it.  fl_frame_ms blocks until that frame is done and gives the ms
 * between the two (DurationEvent.time, render.py:26-38); fl_frame_query is DurationEvent.query
 * (1 done, 0 running).  Up to 4 frames may be in flight. */
int fl_frame_begin(fl_ctx *ctx, uint32_t *frame_id);
int fl_frame_ms(fl_ctx *ctx, uint32_t frame_id, float *ms);
int fl_frame_query(fl_ctx *ctx, uint32_t frame_id);

/* cuburn/render.py:93 PageLockedMemoryPool: pinned host memory for h_out so that the D2H copy of
 * fl_output is truly asynchronous. */
void *fl_host_alloc(size_t nbytes);
void fl_host_free(void *p);

/* ---- measurement taps (bench.py / tests only) ---- */
/* HIP-event times accumulated since the last fl_timings_reset: iterate kernels; drain kernels
 * (tile accumulate + flush); filter kernels; number of iterate launches.  Both calls sync. */
int fl_timings_reset(fl_ctx *ctx);
int fl_timings(fl_ctx *ctx, float *iter_ms, float *flush_ms, float *filter_ms, uint32_t *niter_launches);
/* The same, split further: ms[0] iterate kernels, [1] tile accumulate, [2] flush, [3] all fl_filter calls,
 * [4] the DE proper — the eight direction kernels, the first normalising the accumulator, the last un-normalising it with a
 * following logscale / colorclip riding along — recorded around the launches themselves, whichever call flushes them
 * (the colorclip that follows, another filter, fl_output, a debug tap); [5] the kernels of the device encoders (fl_jpeg_encode,
 * fl_output_jpeg, fl_png_encode, fl_output_png, fl_tiff_encode, fl_output_tiff, fl_exr_encode, fl_output_exr,
 * fl_gif_encode, fl_output_gif, fl_webp_encode, fl_output_webp, fl_apng_encode, fl_output_apng; 0 when none ran). */
int fl_timings_detail(fl_ctx *ctx, float ms[6]);
/* Which iterate kernel actually ran since the last fl_timings_reset: out[0] launches of the kernel compiled for the
 * genome's structure (hipRTC; the counterpart of the module the reference compiles per genome, cuburn/render.py:232-236),
 * out[1] launches of the precompiled interpreter kernel (the fallback); out[2] walker slots, out[3] waves per slot. */
int fl_launch_stats(fl_ctx *ctx, uint32_t out[4]);
/* The device's streaming ceiling as this library can reach it: a float4 copy of `nbytes` (read + write; at least 1 GiB each
 * way, so that the 256 MiB Infinity Cache does not serve it) with non-temporal loads and stores, `iters` launches between two HIP
 * events; *ms = milliseconds per copy.  The denominator of bench.py's "DE >= 60 % of measured HBM bandwidth" (BASELINE.json,
 * SURVEY.md 8d); the reference has no such measurement. */
int fl_measure_copy(int device, size_t nbytes, int iters, float *ms);

/* ---- debug taps (tests only): read/write device state ---- */
enum {
    FL_BUF_FRONT = 0,   /* float4[nbins]  accumulator / filter result (render.py:44-48)  */
    FL_BUF_BACK = 1,    /* float4[nbins]                                                   */
    FL_BUF_PARAMS = 2,  /* float[ntemporal * pstride] interpolated parameter blocks (one per temporal sample = per slot; two / four per slot of 512 8-wave / 256 16-wave slots) */
    FL_BUF_PALETTE = 3, /* u64[FL_PAL_H * FL_PAL_W] packed palette (interp.py:409-433)     */
    FL_BUF_POINTS = 4,  /* float4[nwalkers] walker points (render.py:102-104)              */
    FL_BUF_SEEDS = 5,   /* fl_mwc[nwalkers]                                                */
    FL_BUF_ATOM = 6,    /* u64[nbins] packed integer accumulator of the current side      */
    FL_BUF_HOT = 7,     /* u32[nbins/16] hot-pixel flags of the current side               */
    FL_BUF_SIDE = 8,    /* float4[nbins] side buffer                                       */
    FL_BUF_LOG = 9,     /* u32[] sample log, set 0 of the lane (the set of a frame's first binned launch; csrc/binned.hip) */
    FL_BUF_DIR = 10     /* u32[tiles][batches] its directory: (first record << 16) | count; both "not allocated yet" before a binned launch */
};
int fl_read_buffer(fl_ctx *ctx, fl_genome *g, int which, void *host_dst, size_t nbytes);
int fl_write_buffer(fl_ctx *ctx, fl_genome *g, int which, const void *host_src, size_t nbytes);

/* Device address and size of one of the buffers above (current frame's lane), after waiting for
 * all queued work of the context.  This is the hook for the one exchange step of sample-sharded
 * rendering of a single frame: every rank iterates its share of the samples,
 * the caller sums FL_BUF_FRONT across ranks with its own collective (RCCL all-reduce on its own
 * stream), synchronises that stream, and continues with fl_filter / fl_output.  The reference has
 * no such step (distribute.py:149-163 shards whole frames only). */
int fl_buffer_ptr(fl_ctx *ctx, fl_genome *g, int which, void **dev_ptr, size_t *nbytes);
/* The same without blocking the host (round 5): the address is handed out at once, and what the caller queues on a stream of its
 * own is ordered against the context's work with fl_stream_dependency.  The reference orders its two streams the same way —
 * an event recorded on one, stream.wait_for_event on the other, no host wait inside a frame (cuburn/render.py:358-364,419-430;
 * distribute.py:107-122 is its double-buffered loop). */
int fl_buffer_ptr_async(fl_ctx *ctx, fl_genome *g, int which, void **dev_ptr, size_t *nbytes);
/* Order the context's current lane and a caller's HIP stream (`stream`: a hipStream_t, e.g. torch's current stream, on which the
 * caller runs a collective over buffers obtained above) without a host wait.  ctx_waits = 0: everything queued on the lane so far
 * (deferred filter steps included) happens before whatever the caller queues on `stream` next; ctx_waits = 1: everything queued
 * on `stream` so far happens before whatever the context queues on the lane next. */
int fl_stream_dependency(fl_ctx *ctx, void *stream, int ctx_waits);
/* Make the current lane's frame buffers large enough for a w x h image now (they only ever grow; what they held is lost when
 * they do, so: before a frame's fl_iterate).  The sample-sharded path reserves the height that makes the accumulator's rows a
 * multiple of the rank count: its reduce-scatter then runs on the accumulator where it lies (the rows behind the frame's own are
 * summed and never looked at) instead of on a zero-padded copy per frame.  The reference's accumulator is allocated once, for the
 * largest frame (cuburn/render.py:44-48, :107-113). */
int fl_reserve(fl_ctx *ctx, uint32_t w, uint32_t h);

/* Single-launch taps for bit-exact tests: run `nrounds` rounds (first `fuse` write-disabled)
 * for every slot with the given global round counter, no clears, no flush. */
int fl_debug_iter_launch(fl_ctx *ctx, fl_genome *g, uint32_t w, uint32_t h, uint32_t round0,
                         uint32_t nrounds, uint32_t fuse, int accum_mode);
int fl_debug_flush(fl_ctx *ctx, uint32_t w, uint32_t h);
int fl_debug_clear(fl_ctx *ctx, uint32_t w, uint32_t h, int reset_points);
int fl_debug_clear_hot(fl_ctx *ctx, uint32_t w, uint32_t h);
/* Accumulate tap: run the tile accumulate of the binned mode (csrc/binned.hip) on a sample log and directory the caller built, exactly
 * as a binned iterate launch runs it on its own — the lane's palette (FL_BUF_PALETTE), packed cells and front buffer; no clear
 * before, no flush after.  The log goes into set 0 (FL_BUF_LOG / FL_BUF_DIR).  Geometry: the w x h frame in 128x64 tiles (wide = 0)
 * or 256x64 tiles (wide = 1); nbatch_total batches (slot-major: batch / (nbatch_total / nslots) is the slot, its palette row
 * slot * 64 / nslots) of batch_records records — three 21-bit records per 64-bit word in regions of fl_pack3_words words (128x64
 * tiles), one 22-bit record per 32-bit word (256x64) —, log_words = nbatch_total * region + 8, dir_words = tiles * nbatch_total;
 * nparts workgroups per tile.  Slots of the log no run owns may hold anything.
 * The kernels trust their input, so the call refuses with FL_E_INVAL, on the host and before anything reaches the device: an
 * nslots fl_ctx_create refuses; nbatch_total that is zero or no multiple of nslots; batch_records outside 1..16384 (or, 128x64
 * tiles, regions of fewer than 60 words); nparts outside 1..64; wide = 0 for a frame of more than 2047 narrow tiles; sizes other
 * than the above; a run with first + count > batch_records; runs of a batch that are not contiguous and ascending by tile
 * (first[t + 1] == first[t] + count[t]); a record owned by a run whose cell lies outside astride x aheight (256x64 tiles: or with
 * bits above its 22).  fl_debug_accum_check is the gate alone: it needs no context and no device. */
int fl_debug_accum(fl_ctx *ctx, uint32_t w, uint32_t h, const uint32_t *log, size_t log_words, const uint32_t *dir, size_t dir_words,
                   uint32_t nbatch_total, uint32_t batch_records, uint32_t nslots, uint32_t nparts, int wide);
int fl_debug_accum_check(uint32_t w, uint32_t h, const uint32_t *log, size_t log_words, const uint32_t *dir, size_t dir_words,
                         uint32_t nbatch_total, uint32_t batch_records, uint32_t nslots, uint32_t nparts, int wide);
/* Point-shuffle tap: out[dst_thread] = src_thread after one swap with round counter `round`. */
int fl_debug_shuffle(fl_ctx *ctx, uint32_t round, uint32_t *out256);
/* Xform tap: apply xform `xfi` (nxf = the final xform) of temporal sample `ts` once to n points
 * {x, y, color, unused} with one RNG state each; results overwrite the inputs. */
int fl_debug_apply_xf(fl_ctx *ctx, fl_genome *g, uint32_t ts, int xfi, uint32_t n, float *xyzw, fl_mwc *rng);
/* Math tap: out_bits[i] = the raw 32 bits of device helper `fn` applied to a[i] (and b[i]; unary helpers ignore b, which must
 * still point at n floats), compiled with the iterate kernels' flags.  The helpers are those of csrc/flame_device.h and
 * csrc/variations.h: ATAN2 is v_atan2(a, b), FMOD v_fmod(a, b), POW fpow(a, b), DIV fdiv(a, b); TRUNCA returns its integer;
 * HW_SIN / HW_COS are the bare sine / cosine instructions on an argument in revolutions, without the range reduction. */
enum {
    FL_MATH_RCP = 0, FL_MATH_DIV, FL_MATH_SQRT, FL_MATH_EXP2, FL_MATH_LOG2, FL_MATH_EXP, FL_MATH_LOG, FL_MATH_POW,
    FL_MATH_SIN, FL_MATH_COS, FL_MATH_TAN,
    FL_MATH_ATAN2, FL_MATH_SINH, FL_MATH_COSH, FL_MATH_FMOD, FL_MATH_FMOD_PI,
    FL_MATH_TRUNCA,
    FL_MATH_HW_SIN, FL_MATH_HW_COS,
    FL_MATH_COUNT
};
int fl_debug_math(fl_ctx *ctx, int fn, uint32_t n, const float *a, const float *b, uint32_t *out_bits);
/* The encoders' placement helper in a kernel of its own (one workgroup): offs_out[i] = front + lens[0] + .. + lens[i - 1] for the
 * n >= 1 pieces, *total_out = the sum of all lens (without front), in 64 bits.  Host pointers; synchronous. */
int fl_debug_place(fl_ctx *ctx, const uint32_t *lens, uint32_t n, uint64_t front, uint64_t *offs_out, uint64_t *total_out);
/* Bilateral DE tap: ONE direction (pattern 0..7, csrc/de.hip) of the eight FL_FILT_BILATERAL chains, on the lane's buffers, in the
 * instantiation the chain itself uses — the front buffer is the input, the result ends in the front buffer (a deferred `yuv` or
 * chain runs first).  Pattern 0 reads the raw accumulator (in_mode 1) or the raw YUV accumulator (in_mode 2) and writes the
 * normalised image (x / w, y / w, z / w, w); patterns 1..6 read and write the normalised image; pattern 7 reads it and writes raw
 * pixels (no tone filter rides along).  in_mode is ignored for patterns 1..7.  scalars = sstd, cstd, dstd, dpow, gspeed as
 * fl_filter takes them; the blur coefficients are fl_filter's.  order: -1 = the tile order the launch would take by itself
 * (FLAME_DE_ORDER, else the per-direction table), 0 / 1 / 2 = that order.  The destination is filled with NaN (all bits set)
 * before the launch: a pixel of the padded frame that the kernel does not write shows.  FL_E_INVAL, with nothing queued: a
 * pattern outside 0..7, an order outside -1..2, pattern 0 with an in_mode other than 1 or 2, an empty frame, null pointers. */
int fl_debug_de_dir(fl_ctx *ctx, uint32_t w, uint32_t h, int pattern, const float scalars[5], int in_mode, int order);
/* Compile (only) the iterate kernel specialised for a genome structure, as fl_iterate does on a genome's
 * first launch — the counterpart of cuburn/render.py:232-236 Renderer.compile.  Needs libhiprtc but no
 * GPU; FL_E_UNSUPPORTED if hipRTC is not installed.  nw = 4 | 8 | 16, acc = 0 (atomic), 1 / 3 (binned narrow / wide);
 * count: bit 0 = the sample counters, bit 1 = a temporal sample per four waves (nw = 8 / 16: two / four per workgroup). */
int fl_rtc_compile_check(const int32_t *prog, uint32_t nprog, const int32_t *ops, uint32_t nops, int nw, int count, int acc,
                         char *log, size_t log_bytes);
/* Get the per-genome kernel that fl_iterate would launch for a w x h frame in `accum_mode` before the frame needs it.  With
 * FLAME_RTC_ASYNC=1 the compile is queued for the library's worker thread and the call returns at once; otherwise the kernel is
 * compiled now.  Nothing happens with FLAME_RTC=0.  A failed compile is reported as fl_iterate reports it: one line on stderr,
 * and the genome stays on the interpreter kernel.  The reference compiles in Renderer's constructor (cuburn/render.py:232-236). */
int fl_genome_prepare(fl_ctx *ctx, fl_genome *g, uint32_t w, uint32_t h, int accum_mode);
/* Return when no compile job of a kernel this genome asked for (fl_genome_prepare, fl_iterate) is unfinished and the finished
 * kernels are loaded: the genome's next launches run them.  FL_E_INVAL while the worker is held and a job is outstanding. */
int fl_rtc_wait(fl_ctx *ctx, fl_genome *g);
/* Process-wide counters of the per-genome kernels; needs no device.  out[0] compiler runs; the disk cache (FLAME_RTC_CACHE):
 * out[1] hits, out[2] misses (no file), out[3] files written, out[4] files rejected (short, damaged, another key's); out[5] jobs
 * queued for the worker thread; iterate launches: out[6] on the interpreter kernel while a job of their kernel was unfinished,
 * out[7] on a per-genome kernel. */
int fl_rtc_stats(uint64_t out[8]);
/* Tests only: while held (on != 0) the worker thread leaves queued jobs alone, so a test decides which kernel runs a frame
 * instead of racing the compiler.  A job that is already running finishes. */
int fl_debug_rtc_hold(int on);
/* Counters of the last iterate: accepted (written) samples, out-of-frame, dropped, spills.  "Dropped" are the samples thinned
 * by the hot-pixel roulette (atomic accumulate) and the samples hidden by their xform's opacity; a hidden sample is counted
 * there and nowhere else (it is tested before the frame bounds), so accepted + out-of-frame + dropped is the number of
 * write-enabled samples run. */
int fl_debug_counters(fl_ctx *ctx, uint64_t out4[4]);

/* ---- run-time switches (environment; read when a context is created / a kernel is first launched) ----
 * Every switch is an A/B lever of a documented measurement, none changes results beyond float summation order:
 *   FLAME_LANES=n            stream lanes, 1..4 (default 2: consecutive frames alternate; 1 for kernel timing — profiles/ are taken with it;
 *                            3 and 4 measure the same as 2, profiles/r05_lanes.txt)
 *   FLAME_NO_INTRA_OVERLAP=1 the launches of a multi-launch frame strictly in series on one stream
 *   FLAME_RTC=0              always the precompiled interpreter iterate kernel (no hipRTC per-genome kernel)
 *   FLAME_RTC_FLAGS=...      extra options for the hipRTC compile; FLAME_RTC_DUMP=<dir> keeps its source / assembly
 *   FLAME_RTC_CACHE=<dir>    keep the compiled per-genome kernels in <dir> (made if missing) and load them from there: a process
 *                            compiles only what no earlier process has (csrc/rtc_cache.h; never evicted)
 *   FLAME_RTC_ASYNC=1        compile per-genome kernels on a worker thread; launches run the interpreter kernel until theirs is there
 *   FLAME_BIN_ROUNDS=n       rounds per sorted batch of the sample log (default 16)
 *   FLAME_BIN_PARTS=n        workgroups per tile of the tile accumulate (default: by image size)
 *   FLAME_BIN_GANG=n         adjacent tiles per XCD gang of the tile accumulate (default 32 above 512 tiles, else 0 = off)
 *   FLAME_BIN_WIDE=1         256x64 accumulate tiles for every image size
 *   FLAME_LAUNCH_ROUNDS=n    most write-enabled rounds per binned iterate launch, 16..4096 (default: the reference's growing batches
 *                            capped at 1024 rounds, or at 2304 when that saves the frame a launch)
 *   FLAME_DE_ORDER=d|dddddddd tile order of the DE kernels, one digit for all or one per direction (0 per-XCD column-major runs,
 *                            1 row-major, 2 row-major in runs per XCD; default: by direction and image size, de.hip)
 * The two compile-time timing builds (-DDE_X_TAPSONLY, -DDE_X_STOP_AFTER=n) produce wrong pictures and exist only in the
 * libraries that tools/de_slot_budget.sh builds. */

#ifdef __cplusplus
}
#endif
#endif /* FLAME_HIP_H */
