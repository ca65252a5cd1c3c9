// flame_abi.hip — host side of libflame_hip.so: the C ABI of include/flame_hip.h.
//
// Holds what cuburn's RenderManager / Framebuffers / Renderer hold on the CUDA side
// (cuburn/render.py:40-170, 225-262): device buffers, the stream, persistent walker and
// RNG state, and the per-frame launch sequences of render.py:289-372 and filters.py.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <atomic>
#include <vector>
#include <algorithm>
#include <array>
#include "kernels.h"
#include "flame_device.h"
#include "launch_plan.h"

static thread_local std::string g_err;
static int fail(int code, const char *what, const char *file, int line, hipError_t e = hipSuccess)
{
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    else snprintf(buf, sizeof buf, "%s (%s:%d)", what, file, line);
    g_err = buf;
    return code;
}
static int fail_hip(hipError_t e, const char *what, const char *file, int line)
{
    return fail(e == hipErrorOutOfMemory ? FL_E_NOMEM : FL_E_HIP, what, file, line, e);
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail_hip(e_, #x, __FILE__, __LINE__); } while (0)
#define REQUIRE(c, msg) do { if (!(c)) return fail(FL_E_INVAL, msg, __FILE__, __LINE__); } while (0)

// A grow-only device buffer and its one owner.  reserve(n) keeps memory that is large enough; otherwise it frees it (after `quiesce`
// has waited for whatever may still use it) and allocates n elements anew: contents are not kept.
template <class T> struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;                   // elements
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    operator T *() const { return p; }
    size_t bytes() const { return cap * sizeof(T); }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    template <class Quiesce> int reserve(size_t n, const char *what, Quiesce quiesce)
    {
        if (n <= cap) return FL_OK;
        if (int rc = quiesce()) return rc;
        release();
        const hipError_t e = hipMalloc(&p, n * sizeof(T));
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return fail_hip(e, what, __FILE__, __LINE__); }
        cap = n;
        return FL_OK;
    }
    int reserve(size_t n, const char *what) { return reserve(n, what, [] { return (int)FL_OK; }); }
    friend void swap(DevBuf &a, DevBuf &b) { std::swap(a.p, b.p); std::swap(a.cap, b.cap); }
};

struct EvPair { hipEvent_t a, b; };

// The bilateral DE's scalars (cuburn/filters.py:62-95) and the 7 coefficients of its blur, as fl_filter received them.
struct Bilateral { float sstd, cstd, dstd, dpow, gspeed, k7[7]; };

// Deferred ends of the filter chain.  fl_filter defers two cheap per-pixel steps so that the NEXT call can take them
// along in one pass (cuburn's default chains are yuv -> bilateral -> logscale -> colorclip /
// smearclip): `yuv` directly in front of `bilateral` becomes part of the DE's first direction,
// and the DE's last, un-normalising direction takes a following `logscale` and `colorclip` with it.
// Anything else that looks at the buffers (another filter, output, the debug taps, the next
// frame) first runs what is pending (flush_pending), so the observable behaviour is that of the separate kernels
// (the fused kernels run the same per-pixel device functions in the same order).
struct Pending {
    bool yuv = false, de = false;     // a `yuv` that has not run yet / the DE, all eight directions
    int in_mode = 0;                  // what the DE's first direction normalises: 1 the raw accumulator, 2 the raw YUV one
    Bilateral bl = {};
    DeTail tail = {};                 // what its last direction applies on the way
    fl_dim dim = {0, 0, 0, 0, 0};
    void clear() { yuv = de = false; }
    void defer_yuv(const fl_dim &d) { yuv = true; dim = d; }
    // (a pending `yuv` becomes the first direction's input form)
    void defer_bilateral(const fl_dim &d, const Bilateral &b) { in_mode = yuv ? 2 : 1; yuv = false; de = true; bl = b; tail = {}; dim = d; }
    // A logscale (once) or a colorclip directly behind the deferred DE rides along with its last direction.  A colorclip ends
    // the tail: the caller flushes at once.
    bool try_take(int id, const float *p)
    {
        if (!de || yuv || (id == FL_FILT_LOGSCALE && tail.do_log)) return false;
        if (id == FL_FILT_LOGSCALE) { tail.do_log = 1; tail.k1 = p[0]; tail.k2 = p[1]; }
        else { tail.do_clip = 1; tail.vib = p[0]; tail.highpow = p[1]; tail.gam = p[2]; tail.lin = p[3]; tail.lingam = p[4]; }
        return true;
    }
};

// fl_resize's tables on the device: one entry per (w, h, w2, h2, nxt, nyt) and content hash.  `first` holds xfirst then yfirst,
// `taps` xtaps then ytaps.
struct ResizeTables {
    uint32_t key[6] = {0, 0, 0, 0, 0, 0};
    uint64_t hash = 0, used = 0;      // used 0: empty; otherwise the serial of the last call that took it (the smallest leaves first)
    DevBuf<int32_t> first;
    DevBuf<float> taps;
};

// One "lane" = a stream with its own framebuffers, sample log and per-frame parameter buffers.
// Consecutive frames alternate between two lanes so that the drain + filter + output kernels of
// frame k (bandwidth / TA bound) overlap the iterate kernel of frame k+1 (issue / latency bound),
// the role of stream_a / stream_b in the reference (cuburn/render.py:253-262,432-433).
struct Lane {
    hipStream_t stream = nullptr;
    // the framebuffers: allocated together, for one image size (ensure_fb)
    DevBuf<float4> d_front, d_back, d_side;         // [nbins]
    DevBuf<float> d_blur;                           // 1-channel scratch [nbins]
    DevBuf<u64> d_atom;
    DevBuf<uint32_t> d_hot;
    DevBuf<unsigned char> d_outpix;                 // w*h*8 bytes
    DevBuf<uint32_t> d_de_tmax;                     // FL_FILT_DE: largest 16h per 64 x 16 tile [nbins / 256 + 64]
    DevBuf<float> d_de_sinv;                        // FL_FILT_DE: 1 / S(m / 16) for m = 0 .. 16 * FL_DE_MAX_RADIUS (de_adaptive_norms)
    // The still encoders (encode_on) share one scratch and one staging buffer: their kernels are queued on `stream`, which orders one
    // encode's use behind the other's, and a regrow first waits for the stream (quiesce).
    DevBuf<uint32_t> d_enc;                         // the encoder's working set (jpeg_layout / png_layout / tiff_layout)
    DevBuf<unsigned char> d_enc_out;                // the file on its way to host memory that is not pinned
    size_t nbins() const { return d_front.cap; }
    // binned accumulate: sample log + directory.  Two sets: in a frame of several launches the tile
    // accumulate + flush of launch k run on `aux` while launch k+1 iterates on `stream` into the other set
    // (the role of the reference's alternating streams inside a frame, cuburn/render.py:340-369)
    DevBuf<uint32_t> d_log[2], d_dir[2];
    hipStream_t aux = nullptr;
    hipEvent_t ev_it[2] = {nullptr, nullptr}, ev_ac[2] = {nullptr, nullptr};   // iterate k queued / drains of launch k done
    DevBuf<float> d_params;           // [nslots * pstride] one block per temporal sample = per walker slot
    uint64_t params_serial = 0;       // serial of the genome whose parameters the blocks hold (0: none / just allocated)
    DevBuf<u64> d_palette;            // [FL_PAL_H * FL_PAL_W]
    // cross-lane ordering of the state both lanes share
    hipEvent_t ev_interp_done = nullptr;   // genome staging buffers + palette RNG states
    hipEvent_t ev_iter_done = nullptr;     // walkers + their RNG states
    hipEvent_t ev_out_done = nullptr;      // output-dither RNG states
    bool interp_rec = false, iter_rec = false, out_rec = false;
    Pending pend;
    static const int kResizeTables = 4;             // fl_resize: the tables of the last few sizes (a master and its proxies)
    ResizeTables rz[kResizeTables];
    uint64_t rz_serial = 0;

    std::array<hipEvent_t *, 7> events() { return {&ev_interp_done, &ev_iter_done, &ev_out_done, &ev_it[0], &ev_ac[0], &ev_it[1], &ev_ac[1]}; }
    int quiesce(bool with_aux)
    {
        HIPCHK(hipStreamSynchronize(stream));
        if (with_aux) HIPCHK(hipStreamSynchronize(aux));
        return FL_OK;
    }
    void release_fb()
    {
        d_front.release(); d_back.release(); d_side.release(); d_blur.release(); d_atom.release();
        d_hot.release(); d_outpix.release(); d_de_tmax.release(); d_de_sinv.release();
        pend.clear();                 // whatever was deferred dies with the buffers
    }
    // everything but `stream`, which may be the caller's (fl_ctx::own_stream)
    void release()
    {
        release_fb();
        d_params.release(); d_palette.release(); d_enc.release(); d_enc_out.release();
        for (ResizeTables &t : rz) { t.first.release(); t.taps.release(); t.used = 0; }
        for (int k = 0; k < 2; ++k) { d_log[k].release(); d_dir[k].release(); }
        if (aux) hipStreamDestroy(aux);
        for (hipEvent_t *ev : events()) if (*ev) hipEventDestroy(*ev);
    }
};

#define FL_NOUT 65536u                // RNG states reserved for the output dither kernel

struct fl_ctx {
    int device = 0;
    bool own_stream = false;
    static const int kMaxLanes = 4;
    int nlanes = 2, cur = 0;          // FLAME_LANES (1..4; default 2): consecutive frames go round the lanes
    Lane lanes[kMaxLanes];
    Lane &lane() { return lanes[cur]; }
    Lane &prev_lane() { return lanes[(cur + nlanes - 1) % nlanes]; }      // the previous frame's lane: it touched the shared state last
    uint32_t nslots = 0;
    uint32_t sub_log2 = 0;                        // 512 slots of 8 waves / 256 of 16: 2 / 4 temporal samples per workgroup (iter.hip "Sub-blocks of four waves")
    uint32_t ntemporal() const { return nslots << sub_log2; }      // temporal samples = parameter blocks per frame (>= FL_NTEMPORAL)
    int nw = 4;                       // waves per iterate workgroup
    uint32_t npoints() const { return nslots * (uint32_t)nw * 64u; }      // walkers
    DevBuf<fl_mwc> d_rng;             // three tables: walkers [npoints] | palette rows [FL_PAL_H * 256] | output dither [FL_NOUT]
    fl_mwc *rng_walk() const { return d_rng.p; }
    fl_mwc *rng_pal() const { return d_rng.p + npoints(); }
    fl_mwc *rng_out() const { return rng_pal() + FL_PAL_H * 256; }
    DevBuf<float4> d_points;          // [npoints]
    DevBuf<u64> d_counters;
    DevBuf<uint32_t> d_sort;          // radix sort scratch: digit counts + chunk totals
    uint32_t bin_rounds = 16, bin_parts = 0;      // bin_parts 0: chosen per image (accum_parts)
    uint32_t launch_rounds = 0;                   // FLAME_LAUNCH_ROUNDS: write-enabled rounds per binned launch (0: FL_BIN_MAX_ROUNDS) — the sample log of a launch is nslots x 256 x rounds x 4 bytes
    uint32_t round_counter = 0;
    static const uint32_t kFrames = 8;            // frames that may be in flight (reference: 2)
    hipEvent_t ev_begin_[kFrames] = {}, ev_end_[kFrames] = {};
    uint32_t frame_lane[kFrames] = {};
    uint32_t frame_seq = 0;                        // id of the current frame = frame_seq - 1
    std::vector<EvPair> pool, iter_ev, accum_ev, flush_ev, filt_ev, de_ev, enc_ev;
    size_t pool_used = 0;
    bool timing = true;
    static const uint32_t kDepEvents = 16;
    hipEvent_t dep_ev[kDepEvents] = {};           // fl_stream_dependency
    uint32_t dep_next = 0;
    // environment switches, read once when the context is created (listed in include/flame_hip.h)
    bool env_bin_wide = false, env_no_intra = false;
    bool use_rtc = true;                    // FLAME_RTC=0: always the interpreter kernel
    bool rtc_async = false;                 // FLAME_RTC_ASYNC=1: per-genome kernels are compiled by a worker thread; the interpreter kernel runs until they are there
    uint32_t jpeg_ri = FL_JPEG_RI;          // FLAME_JPEG_RI (1..21): MCUs per JPEG restart interval
    uint32_t jpeg_ri_420 = FL_JPEG_RI_420;  // ... in 4:2:0, where a value above 10 means 10
    uint32_t gif_seg = FL_GIF_SEG;          // FLAME_GIF_SEG (256..3584): pixels per LZW segment of the GIF encoder
    uint32_t n_spec_launch = 0, n_interp_launch = 0;      // iterate launches by kernel since fl_timings_reset (fl_launch_stats)
    BinLayout layout(const fl_dim &d) const { return bin_layout(d, nw, bin_rounds, env_bin_wide); }
};

struct fl_genome {
    uint64_t serial = 0;                    // unique per created genome (a lane remembers whose parameters its blocks hold)
    std::vector<int32_t> prog;
    IterSpec spec;                          // structure for the run-time specialised iterate kernel (rtc.hip)
    hipFunction_t rtc_fn[5][2][4] = {};     // [nw 4 / 8 / 16 / 8 in halves / 16 in quarters][count][acc] once compiled
    unsigned rtc_epoch = 0;                 // module-cache epoch the handles above belong to
    bool rtc_failed = false;                // compile / load failed once: stay on the interpreter kernel
    bool rtc_want[5][2][4] = {};            // variants asked for while their job was unfinished (FLAME_RTC_ASYNC): what fl_rtc_wait waits for
    uint32_t nops = 0, nrows = 0, pstride = 0;
    int32_t *d_prog = nullptr, *d_ops = nullptr;
    float *d_times = nullptr, *d_knots = nullptr, *d_ptimes = nullptr;
    float4 *d_pals = nullptr;
    uint32_t npal = 0;
    // pinned staging for asynchronous uploads: a small ring so that packing frame k+1 on the
    // host never overwrites bytes a queued copy of frame k still has to read
    static const int kStage = 4;
    unsigned char *h_stage[kStage] = {};
    hipEvent_t ev_stage[kStage] = {};
    size_t stage_bytes = 0;
    int stage_next = 0;
};

static const int kKnownVars[] = {0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,30,31,32,33,
    34,35,36,37,38,39,40,41,42,43,44,45,46,48,49,50,51,52,53,54,55,56,57,58,59,60,61,62,63,64,65,66,67,68,69,70,71,72,73,
    74,75,76,77,80,81,82,83,84,85,86,87,88,89,90,91,92,93,94,95,97,98};

// Kernel timing keeps one event pair per launch since the last fl_timings_reset(); a long render
// that never asks for timings stops recording after kMaxTimed launches instead of growing forever.
static const size_t kMaxTimed = 8192;

// A pair from the pool, entered in `list`; nothing recorded yet (null: timing is off, or the pool is spent).
static EvPair *ev_acquire(fl_ctx *c, std::vector<EvPair> &list)
{
    if (!c->timing || c->pool_used >= kMaxTimed) return nullptr;
    if (c->pool.capacity() < kMaxTimed) c->pool.reserve(kMaxTimed);      // pointers into the pool are held across nested pairs: never reallocate
    if (c->pool_used == c->pool.size()) {
        EvPair p;
        if (hipEventCreate(&p.a) != hipSuccess || hipEventCreate(&p.b) != hipSuccess) return nullptr;
        c->pool.push_back(p);
    }
    list.push_back(c->pool[c->pool_used++]);
    return &c->pool[c->pool_used - 1];
}
static EvPair *ev_begin_on(fl_ctx *c, std::vector<EvPair> &list, hipStream_t st)
{
    EvPair *p = ev_acquire(c, list);
    if (p) hipEventRecord(p->a, st);
    return p;
}
static void ev_end_on(EvPair *p, hipStream_t st) { if (p) hipEventRecord(p->b, st); }
static EvPair *ev_begin(fl_ctx *c, std::vector<EvPair> &list) { return ev_begin_on(c, list, c->lane().stream); }
static void ev_end(fl_ctx *c, EvPair *p) { ev_end_on(p, c->lane().stream); }

#pragma GCC visibility push(default)
extern "C" {

int fl_abi_version(void) { return FL_ABI_VERSION; }
const char *fl_last_error(void) { return g_err.c_str(); }

void fl_calc_dim(uint32_t w, uint32_t h, fl_dim *o) { *o = calc_dim(w, h); }

// the normalisers of the `de` filter depend on nothing but the quantised radius: computed once per process
static const float *de_norms()
{
    static const std::vector<float> t = [] { std::vector<float> v(16 * FL_DE_MAX_RADIUS + 1); de_adaptive_norms(v.data()); return v; }();
    return t.data();
}

// cuburn/render.py:121-161 Framebuffers.alloc / set_dim: grow-only; on OOM free everything
// and report FL_E_NOMEM so the caller survives an oversize frame.
static int ensure_fb(Lane &ln, uint32_t w, uint32_t h, fl_dim *dim)
{
    const fl_dim d = *dim = calc_dim(w, h);
    const size_t nbins = (size_t)d.ah * d.astride, ob = (size_t)d.w * d.h * 8, nsinv = 16 * FL_DE_MAX_RADIUS + 1;
    if (ln.nbins() >= nbins && ln.d_outpix.cap >= ob) return FL_OK;
    hipStreamSynchronize(ln.stream);
    ln.release_fb();
    const char *what = "framebuffer allocation";
    int rc;
    if (!(rc = ln.d_front.reserve(nbins, what)) && !(rc = ln.d_back.reserve(nbins, what)) && !(rc = ln.d_side.reserve(nbins, what)) &&
        !(rc = ln.d_blur.reserve(nbins, what)) && !(rc = ln.d_atom.reserve(nbins, what)) && !(rc = ln.d_hot.reserve(nbins / 16, what)) &&
        !(rc = ln.d_outpix.reserve(ob, what)) && !(rc = ln.d_de_tmax.reserve(nbins / 256 + 64, what)) && !(rc = ln.d_de_sinv.reserve(nsinv, what))) {
        const hipError_t e = hipMemcpyAsync(ln.d_de_sinv, de_norms(), 4 * nsinv, hipMemcpyHostToDevice, ln.stream);
        if (e != hipSuccess) { (void)hipGetLastError(); rc = fail_hip(e, what, __FILE__, __LINE__); }
    }
    if (rc) ln.release_fb();
    return rc;
}

static bool env_on(const char *name) { const char *e = getenv(name); return e && *e && strcmp(e, "0") != 0; }

int fl_ctx_create(int device, void *stream, const fl_mwc *seeds, uint32_t nseeds, uint32_t nslots, fl_ctx **out)
{
    REQUIRE(out && seeds, "null argument");
    REQUIRE(nslots_valid(nslots),
            "nslots must be a multiple of 256 in [1024, 16384] (or 512 slots of 8 waves / 256 of 16: two / four temporal samples per workgroup)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(FL_E_NODEV, "no HIP device", __FILE__, __LINE__);
    REQUIRE(device >= 0 && device < ndev, "bad device index");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(FL_E_NODEV, "device is not gfx950 (kernels are built for MI355X only)", __FILE__, __LINE__);
    // waves per iterate workgroup (4, 8 or 16) follow from the size of the seed table
    int nw = 0;
    {
        const uint32_t fixed = FL_PAL_H * 256 + FL_NOUT;
        const uint32_t per_wave = nslots * 64u;
        if (nseeds == fixed + 16u * per_wave) nw = 16;
        else if (nseeds == fixed + 8u * per_wave) nw = 8;
        else if (nseeds == fixed + 4u * per_wave) nw = 4;
        else return fail(FL_E_INVAL, "nseeds must be nslots*64*NW + 64*256 + 65536 with NW = 4, 8 or 16", __FILE__, __LINE__);
    }
    if (nslots < FL_NTEMPORAL && (uint32_t)nw * nslots != 4u * FL_NTEMPORAL)
        return fail(FL_E_INVAL, "512 slots need 8-wave workgroups, 256 slots 16-wave ones (a temporal sample per four waves: 1024 in all)", __FILE__, __LINE__);
    fl_ctx *c = new fl_ctx;
    c->device = device;
    c->nw = nw;
    c->nslots = nslots;
    c->sub_log2 = nslots >= FL_NTEMPORAL ? 0u : nw == 8 ? 1u : 2u;
    if (const char *e = getenv("FLAME_LANES")) { const int v = atoi(e); c->nlanes = v >= 1 && v <= fl_ctx::kMaxLanes ? v : 2; }
    if (const char *e = getenv("FLAME_BIN_ROUNDS")) { int v = atoi(e); if (v >= 1 && v <= FL_BIN_R_MAX) c->bin_rounds = (uint32_t)v; }
    if (const char *e = getenv("FLAME_BIN_PARTS")) { int v = atoi(e); if (v >= 1 && v <= 64) c->bin_parts = (uint32_t)v; }
    c->env_bin_wide = env_on("FLAME_BIN_WIDE");
    if (const char *e = getenv("FLAME_RTC")) c->use_rtc = strcmp(e, "0") != 0;
    c->rtc_async = env_on("FLAME_RTC_ASYNC");
    c->gif_seg = gif_segment_pixels();
    if (const char *e = getenv("FLAME_JPEG_RI")) { const int v = atoi(e); if (v >= 1 && v <= 21) { c->jpeg_ri = (uint32_t)v; c->jpeg_ri_420 = std::min((uint32_t)v, FL_JPEG_RI_420_MAX); } }
    c->env_no_intra = env_on("FLAME_NO_INTRA_OVERLAP");      // launches of a frame strictly in series on one stream
    if (const char *e = getenv("FLAME_LAUNCH_ROUNDS")) { int v = atoi(e); if (v >= 16 && v <= 4096) c->launch_rounds = (uint32_t)(v / 16 * 16); }
    if (stream) { c->lanes[0].stream = (hipStream_t)stream; c->own_stream = false; c->nlanes = 1; }   // caller's stream: one lane
    else c->own_stream = true;
    // every failure below leaves through fl_ctx_destroy, which frees whatever exists so far
    const size_t nrng = (size_t)c->npoints() + FL_PAL_H * 256 + FL_NOUT;
    const char *what = "context allocation";
    const auto hip = [what](hipError_t e) { return e == hipSuccess ? (int)FL_OK : fail_hip(e, what, __FILE__, __LINE__); };
    int rc = FL_OK;
    for (int i = 0; i < c->nlanes && c->own_stream && !rc; ++i) rc = hip(hipStreamCreateWithFlags(&c->lanes[i].stream, hipStreamNonBlocking));
    if (!rc && !(rc = c->d_rng.reserve(nrng, what)) && !(rc = c->d_points.reserve(c->npoints(), what))) rc = c->d_counters.reserve(4, what);
    for (int i = 0; i < c->nlanes && !rc; ++i) {
        Lane &ln = c->lanes[i];
        if ((rc = ln.d_palette.reserve(FL_PAL_H * FL_PAL_W, what)) || (rc = hip(hipStreamCreateWithFlags(&ln.aux, hipStreamNonBlocking)))) break;
        for (hipEvent_t *ev : ln.events()) if ((rc = hip(hipEventCreateWithFlags(ev, hipEventDisableTiming)))) break;
    }
    if (!rc && !(rc = hip(hipMemcpy(c->d_rng, seeds, c->d_rng.bytes(), hipMemcpyHostToDevice))) &&
        !(rc = hip(hipMemsetD32(c->d_points, 0x7fc00000, (size_t)c->npoints() * 4)))) rc = hip(hipMemset(c->d_counters, 0, 32));
    for (uint32_t i = 0; i < fl_ctx::kFrames && !rc; ++i)
        if (!(rc = hip(hipEventCreate(&c->ev_begin_[i])))) rc = hip(hipEventCreate(&c->ev_end_[i]));
    if (rc) {
        fl_ctx_destroy(c);
        (void)hipGetLastError();
        return rc;
    }
    *out = c;
    return FL_OK;
}

static void sync_all(fl_ctx *c)
{
    for (int i = 0; i < c->nlanes; ++i) { hipStreamSynchronize(c->lanes[i].stream); if (c->lanes[i].aux) hipStreamSynchronize(c->lanes[i].aux); }
}

void fl_ctx_destroy(fl_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    for (uint32_t i = 0; i < fl_ctx::kDepEvents; ++i) if (c->dep_ev[i]) hipEventDestroy(c->dep_ev[i]);
    for (Lane &ln : c->lanes) {
        if (ln.stream) hipStreamSynchronize(ln.stream);
        if (ln.aux) hipStreamSynchronize(ln.aux);
    }
    for (Lane &ln : c->lanes) {
        ln.release();
        if (c->own_stream && ln.stream) hipStreamDestroy(ln.stream);
    }
    for (auto &p : c->pool) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
    for (uint32_t i = 0; i < fl_ctx::kFrames; ++i) {
        if (c->ev_begin_[i]) hipEventDestroy(c->ev_begin_[i]);
        if (c->ev_end_[i]) hipEventDestroy(c->ev_end_[i]);
    }
    delete c;                          // (with the context's own buffers)
    (void)hipGetLastError();
}

int fl_ctx_sync(fl_ctx *c) { REQUIRE(c, "null ctx"); sync_all(c); return FL_OK; }

// Make the current lane's stream wait for what the previous frame's lane last did to state both share.
static int wait_other(fl_ctx *c, int what)
{
    if (c->nlanes < 2) return FL_OK;
    Lane &ln = c->lane(), &o = c->prev_lane();
    if (what == 0 && o.interp_rec) HIPCHK(hipStreamWaitEvent(ln.stream, o.ev_interp_done, 0));
    if (what == 1 && o.iter_rec) HIPCHK(hipStreamWaitEvent(ln.stream, o.ev_iter_done, 0));
    if (what == 2 && o.out_rec) HIPCHK(hipStreamWaitEvent(ln.stream, o.ev_out_done, 0));
    return FL_OK;
}

// Validate the program header before any kernel trusts it (the reference traps on device,
// cuburn/code/iter.py:254-257).  Variation numbers live in the parameter block as FL_OP_CONST
// ops and are checked with the op list.
static int check_prog(const int32_t *p, uint32_t n)
{
    REQUIRE(n >= FL_PROG_HDR && p[0] == FL_PROG_MAGIC, "bad program header");
    int nxf = p[1], hf = p[2], ps = p[3], cdf = p[4], xo = p[5], xs = p[6], vs = p[7];
    REQUIRE(nxf >= 1 && nxf <= FL_MAX_XFORMS && (hf == 0 || hf == 1), "bad xform count");
    REQUIRE(ps >= 6 + nxf && ps <= FL_MAX_PSTRIDE, "bad pstride");
    REQUIRE(cdf >= 6 && cdf + nxf <= xo, "bad cdf offset");
    REQUIRE(xs >= FL_XF_HDR + vs && (xs % 4) == 0 && vs >= 2 && vs <= 64, "bad record strides");
    REQUIRE(xo + (nxf + hf) * xs <= ps, "xform records exceed the block");
    if (n > FL_PROG_HDR) {      // a chaos program: word 8 = block offset of the nxf x nxf matrix, behind the records
        const int co = p[FL_PROG_HDR];
        REQUIRE(nxf <= FL_CHAOS_MAX_XFORMS, "too many xforms for a genome with chaos");
        REQUIRE(co >= xo + (nxf + hf) * xs && co <= ps && nxf * nxf <= ps - co, "bad chaos offset");
    }
    return FL_OK;
}

// What an op may do to the structure of the xform records (prog passed check_prog): an opacity op writes word 15 of a selectable
// record (the final xform has no opacity); a structure word — FL_OP_CONST: xform word 14 (nvar | post << 8 | opacity << 9) or a
// variation number — lies inside the records, and word 14 carries nothing above bit 9 and no opacity flag on the final xform.
// iter_spec() relies on this.
static int check_structure_op(const int32_t *prog, const int32_t *o)
{
    const int xs = prog[6], nxf = prog[1], nrec = nxf + prog[2], rel = o[1] - prog[5];
    if (o[0] == FL_OP_OPACITY) REQUIRE(rel >= 0 && rel / xs < nxf && rel % xs == 15, "opacity op must write word 15 of a selectable xform record");
    if (o[0] != FL_OP_CONST) return FL_OK;
    REQUIRE(rel >= 0 && rel / xs < nrec, "structure word outside the xform records");
    if (rel % xs == 14) {
        REQUIRE((o[2] >> 10) == 0, "bad structure word");
        REQUIRE(((o[2] >> 9) & 1) == 0 || rel / xs < nxf, "the final xform has no opacity");
    }
    return FL_OK;
}

// Structure tables of the per-genome kernel (rtc.hip) from a program and its op list: per record the variation count, post and
// opacity flags of its structure word (14) and its variation numbers in order (-1: no op names one).  The callers have checked
// every op with check_structure_op.
static IterSpec iter_spec(const int32_t *prog, uint32_t nprog, const int32_t *ops, uint32_t nops)
{
    const int xo = prog[5], xs = prog[6], vs = prog[7], nrec = prog[1] + prog[2];
    const bool has_chaos = nprog > FL_PROG_HDR;
    IterSpec spec;
    spec.nxf = prog[1]; spec.has_final = prog[2]; spec.pstride = prog[3]; spec.cdf_off = prog[4];
    spec.xf_off = xo; spec.xf_stride = xs; spec.var_stride = vs;
    spec.chaos = has_chaos ? 1 : 0; spec.chaos_off = has_chaos ? prog[FL_PROG_HDR] : 0;
    spec.nvar.assign(nrec, 0); spec.post.assign(nrec, 0); spec.opac.assign(nrec, 0); spec.vids.assign(nrec, std::vector<int>());
    for (int pass = 0; pass < 2; ++pass)          // the structure words first: they size the variation lists
        for (uint32_t i = 0; i < nops; ++i) {
            const int32_t *o = ops + 4 * i;
            if (o[0] != FL_OP_CONST) continue;
            const int rel = o[1] - xo, rec = rel / xs, w = rel % xs;
            if (pass == 0 && w == 14) {
                spec.nvar[rec] = o[2] & 0xff; spec.post[rec] = (o[2] >> 8) & 1; spec.opac[rec] = (o[2] >> 9) & 1;
                spec.vids[rec].assign(spec.nvar[rec], -1);
            } else if (pass == 1 && w != 14) {
                const int j = (w - FL_XF_HDR) / vs;
                if (j >= 0 && j < spec.nvar[rec]) spec.vids[rec][j] = o[2];
            }
        }
    return spec;
}

static bool known_var(int id)
{
    for (int k : kKnownVars) if (k == id) return true;
    return false;
}

int fl_genome_create(fl_ctx *c, const int32_t *prog, uint32_t nprog, const int32_t *ops, uint32_t nops,
                     uint32_t nrows, fl_genome **out)
{
    REQUIRE(c && prog && ops && out, "null argument");
    int rc = check_prog(prog, nprog);
    if (rc) return rc;
    REQUIRE(nrows >= 1 && nrows <= 4096 && nops >= 1, "bad row / op count");
    uint32_t ps = prog[3];
    const int xo = prog[5], xs = prog[6], vs = prog[7], nrec = prog[1] + prog[2];
    std::vector<int> nvar_seen(nrec, -1), opac_seen(nrec, 0), opac_ops(nrec, 0);
    const bool has_chaos = nprog > FL_PROG_HDR;
    std::vector<int> chaos_ops(has_chaos ? prog[1] : 0, 0);
    for (uint32_t i = 0; i < nops; ++i) {
        const int32_t *o = ops + 4 * i;
        REQUIRE(o[0] >= FL_OP_SPLINE && o[0] <= FL_OP_CHAOS_CDF, "bad op kind");
        REQUIRE(o[1] >= 0 && (uint32_t)o[1] < ps, "op destination out of range");
        if ((rc = check_structure_op(prog, o))) return rc;
        const int rel = o[1] - xo;
        if (o[0] != FL_OP_CONST) {
            // every word an op writes and every spline row it reads must lie inside the block / row table
            uint32_t ndst = 1, nsrc = 1;
            switch (o[0]) {
            case FL_OP_CAMERA: ndst = 6; nsrc = 4; break;
            case FL_OP_AFFINE: ndst = 6; nsrc = 6; break;
            case FL_OP_CDF:
                REQUIRE(o[3] >= 1 && o[3] <= FL_MAX_XFORMS, "bad CDF length");
                ndst = nsrc = (uint32_t)o[3];
                break;
            case FL_OP_PERSP: ndst = 3; break;
            case FL_OP_CHAOS_CDF: {     // row p of the chaos matrix, from the nxf weight rows and nxf chaos rows
                REQUIRE(has_chaos, "chaos op in a program without a chaos matrix");
                const int nx = prog[1], crel = o[1] - prog[FL_PROG_HDR];
                REQUIRE(o[3] >= 0 && (o[3] & 0xff) == nx, "bad chaos row length");
                REQUIRE(crel >= 0 && crel < nx * nx && crel % nx == 0, "chaos op must write a row of the chaos matrix");
                REQUIRE((uint32_t)(o[3] >> 8) + (uint32_t)nx <= nrows, "op row out of range");
                ++chaos_ops[crel / nx];
                ndst = nsrc = (uint32_t)nx;
            } break;
            default: break;
            }
            REQUIRE((uint32_t)o[1] + ndst <= ps, "op destination out of range");
            REQUIRE(o[2] >= 0 && (uint32_t)o[2] + nsrc <= nrows, "op row out of range");
            if (o[0] == FL_OP_RATIO2 || o[0] == FL_OP_PERSP) REQUIRE(o[3] >= 0 && (uint32_t)o[3] < nrows, "op row out of range");
            if (o[0] == FL_OP_OPACITY) ++opac_ops[rel / xs];
            continue;
        }
        // structure words, beyond check_structure_op: the variations fit the record, every variation is a known one
        const int w = rel % xs;
        if (w == 14) {
            const int nv = o[2] & 0xff;
            REQUIRE(FL_XF_HDR + nv * vs <= xs, "bad variation count");
            nvar_seen[rel / xs] = nv;
            opac_seen[rel / xs] = (o[2] >> 9) & 1;
        } else {
            REQUIRE(w >= FL_XF_HDR && (w - FL_XF_HDR) % vs == 0, "misplaced structure word");
            if (!known_var(o[2])) return fail(FL_E_UNSUPPORTED, "unknown variation id", __FILE__, __LINE__);
        }
    }
    for (int i = 0; i < nrec; ++i) REQUIRE(nvar_seen[i] >= 0, "xform record without a variation count");
    for (int i = 0; i < nrec; ++i) REQUIRE(opac_ops[i] == opac_seen[i], "opacity flag and opacity op do not match");
    for (int n : chaos_ops) REQUIRE(n == 1, "every row of the chaos matrix needs exactly one chaos op");
    const IterSpec spec = iter_spec(prog, nprog, ops, nops);
    for (int i = 0; i < nrec; ++i)
        for (int j = 0; j < spec.nvar[i]; ++j) REQUIRE(spec.vids[i][j] >= 0, "variation record without a variation number");
    HIPCHK(hipSetDevice(c->device));
    fl_genome *g = new fl_genome;
    { static std::atomic<uint64_t> next_serial{1}; g->serial = next_serial.fetch_add(1); }
    g->spec = spec;
    g->prog.assign(prog, prog + nprog);
    g->nops = nops; g->nrows = nrows; g->pstride = ps;
    g->stage_bytes = 2 * 4 * (size_t)nrows * FL_KNOTS + 16 * 256 * (FL_KNOTS - 1) + 4 * FL_KNOTS;
    hipError_t e = hipSuccess;
    do {        // a failure anywhere frees what exists so far (fl_genome_destroy tolerates a partial genome)
        if ((e = hipMalloc(&g->d_prog, 4 * nprog))) break;
        if ((e = hipMalloc(&g->d_ops, 16 * nops))) break;
        // One spare row behind the table, padding (times 1e9, knots 0) written once here and never by fl_genome_upload: a row
        // of FL_KNOTS real knots evaluated after its last-but-one reads word FL_KNOTS, the first of the following row
        // (catmull_rom, times[idx + 2]; include/flame_hip.h (4)), and behind the LAST row that word must exist.
        const size_t table = 4 * (size_t)nrows * FL_KNOTS;
        const std::vector<float> pad_times(FL_KNOTS, 1e9f);
        if ((e = hipMalloc(&g->d_times, table + 4 * FL_KNOTS))) break;
        if ((e = hipMalloc(&g->d_knots, table + 4 * FL_KNOTS))) break;
        if ((e = hipMemcpy((char *)g->d_times + table, pad_times.data(), 4 * FL_KNOTS, hipMemcpyHostToDevice))) break;
        if ((e = hipMemset((char *)g->d_knots + table, 0, 4 * FL_KNOTS))) break;
        if ((e = hipMalloc(&g->d_ptimes, 4 * FL_KNOTS))) break;
        if ((e = hipMalloc(&g->d_pals, 16 * 256 * FL_KNOTS))) break;
        if ((e = hipMemcpy(g->d_prog, prog, 4 * nprog, hipMemcpyHostToDevice))) break;
        if ((e = hipMemcpy(g->d_ops, ops, 16 * nops, hipMemcpyHostToDevice))) break;
        if ((e = hipMemset(g->d_pals, 0, 16 * 256 * FL_KNOTS))) break;
        for (int i = 0; i < fl_genome::kStage && e == hipSuccess; ++i) {
            if ((e = hipHostMalloc((void **)&g->h_stage[i], g->stage_bytes, hipHostMallocDefault))) break;
            e = hipEventCreateWithFlags(&g->ev_stage[i], hipEventDisableTiming);
        }
    } while (0);
    if (e != hipSuccess) {
        fl_genome_destroy(g);
        (void)hipGetLastError();
        return fail_hip(e, "genome allocation", __FILE__, __LINE__);
    }
    *out = g;
    return FL_OK;
}

void fl_genome_destroy(fl_genome *g)
{
    if (!g) return;
    hipFree(g->d_prog); hipFree(g->d_ops); hipFree(g->d_times); hipFree(g->d_knots);
    hipFree(g->d_ptimes); hipFree(g->d_pals);
    for (int i = 0; i < fl_genome::kStage; ++i) { if (g->h_stage[i]) hipHostFree(g->h_stage[i]); if (g->ev_stage[i]) hipEventDestroy(g->ev_stage[i]); }
    delete g;
}

int fl_genome_upload(fl_ctx *c, fl_genome *g, const float *times, const float *knots,
                     const float *pal_rgba, const float *pal_times, uint32_t npal)
{
    REQUIRE(c && g && times && knots && pal_rgba && pal_times, "null argument");
    REQUIRE(npal >= 1 && npal < FL_KNOTS, "bad palette count");
    HIPCHK(hipSetDevice(c->device));
    const size_t nb = 4 * (size_t)g->nrows * FL_KNOTS, pb = 16 * 256 * (size_t)npal, tb = 4 * FL_KNOTS;
    const int slot = g->stage_next;
    g->stage_next = (slot + 1) % fl_genome::kStage;
    HIPCHK(hipEventSynchronize(g->ev_stage[slot]));        // the copy that last used this slot is done
    unsigned char *h = g->h_stage[slot];
    memcpy(h, times, nb);
    memcpy(h + nb, knots, nb);
    memcpy(h + 2 * nb, pal_rgba, pb);
    memcpy(h + 2 * nb + pb, pal_times, tb);
    { int rc = wait_other(c, 0); if (rc) return rc; }     // the other lane's interp still reads these buffers
    hipStream_t st = c->lane().stream;
    HIPCHK(hipMemcpyAsync(g->d_times, h, nb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g->d_knots, h + nb, nb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g->d_pals, h + 2 * nb, pb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g->d_ptimes, h + 2 * nb + pb, tb, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(g->ev_stage[slot], st));
    g->npal = npal;
    return FL_OK;
}

int fl_frame_begin(fl_ctx *c, uint32_t *frame_id)
{
    REQUIRE(c && frame_id, "null argument");
    HIPCHK(hipSetDevice(c->device));
    const uint32_t id = c->frame_seq++;
    const uint32_t k = id % fl_ctx::kFrames;
    c->cur = (int)(id % (uint32_t)c->nlanes);             // consecutive frames go round the lanes
    c->frame_lane[k] = (uint32_t)c->cur;
    HIPCHK(hipEventRecord(c->ev_begin_[k], c->lane().stream));
    HIPCHK(hipEventRecord(c->ev_end_[k], c->lane().stream));       // moved forward by fl_output
    *frame_id = id;
    return FL_OK;
}

int fl_interp(fl_ctx *c, fl_genome *g, uint32_t w, uint32_t h, float ts, float td)
{
    REQUIRE(c && g && g->npal, "genome not uploaded");
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    const fl_dim d = calc_dim(w, h);
    // One parameter block per walker slot: slot s iterates temporal sample s of nslots, evaluated
    // at ts + s*td/nslots, so that every temporal sample receives the same number of iterations
    // whatever the slot count (the reference: one block column per each of its 1024 temporal
    // samples, cuburn/render.py:303-307,343-346; cuburn/code/iter.py:165,184).
    const size_t need = (size_t)c->ntemporal() * g->pstride;     // (workgroups in sub-blocks: two or four blocks per slot)
    if (need > ln.d_params.cap) ln.params_serial = 0;
    int rc = ln.d_params.reserve(need, "parameter blocks", [&ln] { return ln.quiesce(false); });
    if (rc) return rc;
    if ((rc = wait_other(c, 0))) return rc;                 // palette RNG states are shared
    launch_interp_palette(ln.stream, c->rng_pal(), g->d_ptimes, g->d_pals, ts, td / FL_PAL_H, ln.d_palette);
    launch_interp_params(ln.stream, ln.d_params, g->d_times, g->d_knots, g->d_ops, g->nops, g->pstride,
                         c->ntemporal(), ts, td / (float)c->ntemporal(), d, ln.params_serial != g->serial);
    ln.params_serial = g->serial;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ln.ev_interp_done, ln.stream));
    ln.interp_rec = true;
    return FL_OK;
}

static int do_clear(fl_ctx *c, Lane &ln, const fl_dim &d, bool reset_points)
{
    size_t nbins = (size_t)d.ah * d.astride;
    // cuburn/render.py:321-328
    launch_clear_frame(ln.stream, ln.d_front, ln.d_atom, ln.d_hot, c->d_counters, c->d_points, (uint32_t)nbins,
                       reset_points ? c->npoints() : 0u);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

// The log + directory set `buf` of the lane, large enough for a launch of `write_rounds` write-enabled rounds.
static int ensure_binned(fl_ctx *c, Lane &ln, const fl_dim &d, uint32_t write_rounds, int buf, BinLayout *layout, uint32_t *nbatch_total)
{
    const BinLayout b = *layout = c->layout(d);
    if (b.nbins > FL_MAX_BINS_WIDE) return fail(FL_E_UNSUPPORTED, "image too large for the binned accumulate (> 8191 tiles of 256x64)", __FILE__, __LINE__);
    const BinSet s = bin_set(b, write_rounds, c->bin_rounds, c->nslots);
    *nbatch_total = s.nbatch;
    const auto quiesce = [&ln] { return ln.quiesce(true); };
    if (int rc = ln.d_log[buf].reserve(s.log_words, "sample log", quiesce)) return rc;
    return ln.d_dir[buf].reserve(s.dir_words, "sample log directory", quiesce);
}

// The per-genome kernel of one variant (count, kernel accumulate mode) in the context's walker geometry, or null: the interpreter
// kernel runs.  `mode` (kernels.h): RTC_SYNC compiles a missing variant now; RTC_POLL queues it for the worker thread and
// reports *pending while its job is unfinished; RTC_WAIT waits for it.
static hipFunction_t rtc_variant(fl_ctx *c, fl_genome *g, bool count, int kacc, int mode, bool *pending)
{
    *pending = false;
    if (!c->use_rtc || g->rtc_failed || kacc == 2) return nullptr;
    const unsigned ep = rtc_epoch();
    if (g->rtc_epoch != ep) { memset(g->rtc_fn, 0, sizeof g->rtc_fn); g->rtc_epoch = ep; }     // the module cache was flushed
    // the walker geometry's row of rtc_fn: 4 / 8 / 16 waves, 8 in halves, 16 in quarters
    const int geom = c->sub_log2 ? 2 + (int)c->sub_log2 : c->nw == 16 ? 2 : c->nw == 8 ? 1 : 0;
    hipFunction_t &slot = g->rtc_fn[geom][count ? 1 : 0][kacc];
    if (!slot) {
        std::string err;
        const int rc = rtc_iter_kernel(c->device, g->spec, c->nw, c->nslots, count, kacc, &slot, &err, c->sub_log2, mode);
        if (rc < 0) {
            g->rtc_failed = true;
            slot = nullptr;
            fprintf(stderr, "libflame_hip: per-genome kernel not available (%s); using the interpreter kernel\n", err.c_str());
        } else if (rc > 0) {
            slot = nullptr;
            *pending = true;
        }
        g->rtc_want[geom][count ? 1 : 0][kacc] = rc > 0;
    }
    return slot;
}

// One iterate launch and (binned mode) its tile accumulate.  `buf` selects the log / directory set;
// `drain` is the stream the accumulate runs on: the lane's own stream, or its aux stream when the
// launches of a frame are pipelined (then the accumulate waits for this iterate through ev_it[buf]).
static int do_iter_launch(fl_ctx *c, Lane &ln, fl_genome *g, const fl_dim &d, uint32_t nrounds, uint32_t fuse, bool count, int acc = 0,
                          int buf = 0, hipStream_t drain = nullptr)
{
    if (!drain) drain = ln.stream;
    BinLayout bl = {};
    uint32_t nbatch_total = 0;
    if (acc == FL_ACCUM_BINNED) {
        if (nrounds <= fuse) return fail(FL_E_INVAL, "binned launch needs write-enabled rounds", __FILE__, __LINE__);
        int rc = ensure_binned(c, ln, d, nrounds - fuse, buf, &bl, &nbatch_total);
        if (rc) return rc;
    }
    EvPair *e = ev_acquire(c, c->iter_ev);      // recorded by the kernel launch itself (hipExtLaunchKernelGGL)
    const int kacc = acc == FL_ACCUM_BINNED && bl.wide ? 3 : acc;
    // the kernel specialised for this genome's structure (compiled on first use, rtc.hip); the
    // interpreter kernel if hipRTC is unavailable, switched off, the compile failed — or is still under way (FLAME_RTC_ASYNC)
    bool pending = false;
    const hipFunction_t fn = rtc_variant(c, g, count, kacc, c->rtc_async ? RTC_POLL : RTC_SYNC, &pending);
    (fn ? c->n_spec_launch : c->n_interp_launch) += 1;
    rtc_count_launch(fn != nullptr, pending);
    const IterLaunch il = {c->nw, count, kacc, c->nslots, g->d_prog, ln.d_params, ln.d_palette, c->rng_walk(), c->d_points,
                           ln.d_hot, ln.d_atom, (float *)ln.d_front.p, c->d_counters, d.astride, d.ah, c->round_counter, nrounds, fuse,
                           bl.tiles_x, bl.nbins, c->bin_rounds, nbatch_total, ln.d_log[buf], ln.d_dir[buf],
                           e ? e->a : nullptr, e ? e->b : nullptr, c->sub_log2, g->spec.chaos != 0};
    launch_iter(ln.stream, il, fn);
    c->round_counter += nrounds;
    HIPCHK(hipGetLastError());
    if (acc == FL_ACCUM_BINNED) {
        if (drain != ln.stream) {
            HIPCHK(hipEventRecord(ln.ev_it[buf], ln.stream));
            HIPCHK(hipStreamWaitEvent(drain, ln.ev_it[buf], 0));
        }
        EvPair *e2 = ev_begin_on(c, c->accum_ev, drain);
        launch_accum_tiles(drain, ln.d_log[buf], ln.d_dir[buf], ln.d_palette, ln.d_atom, (float *)ln.d_front.p, bl.tiles_x, bl.nbins,
                           accum_parts(bl.nbins, bl.wide, c->bin_parts), nbatch_total, c->bin_rounds * (uint32_t)c->nw * 64, c->nslots,
                           d.astride, d.ah, bl.wide);
        ev_end_on(e2, drain);
        HIPCHK(hipGetLastError());
    }
    return FL_OK;
}

static int do_flush(fl_ctx *c, Lane &ln, const fl_dim &d, bool use_hot = true, hipStream_t st = nullptr)
{
    if (!st) st = ln.stream;
    EvPair *e = ev_begin_on(c, c->flush_ev, st);
    launch_flush(st, ln.d_atom, ln.d_front, ln.d_hot, d.ah * d.astride, use_hot);
    ev_end_on(e, st);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

// Run what the filter chain deferred: the `yuv`, or the DE — its eight per-direction kernels (de.hip) are all queued here, now
// that the tail is known: the first normalises the accumulator in d_front as it stages it, the result goes through d_back and
// ends in d_front, un-normalised (+ the tail's tone filters) by the last.
static int flush_pending(fl_ctx *c, Lane &ln)
{
    Pending &pd = ln.pend;
    if (!pd.yuv && !pd.de) return FL_OK;
    if (pd.yuv) {
        launch_yuv_to_rgb(ln.stream, pd.dim, ln.d_back, ln.d_front);
        swap(ln.d_front, ln.d_back);
    }
    if (pd.de) {
        const Bilateral &b = pd.bl;
        const auto dir = [&](int pat, float4 *dst, const float4 *src, const DeTail *tail) {
            launch_de_dir(ln.stream, pd.dim, pat, dst, src, b.k7, b.sstd, b.cstd, b.dstd, b.dpow, b.gspeed, pd.in_mode, tail);
        };
        EvPair *e = ev_begin_on(c, c->de_ev, ln.stream);            // the DE proper: fl_timings_detail[4], whoever flushes it
        float4 *Na = ln.d_back, *Nb = ln.d_front;
        dir(0, Na, Nb, nullptr);
        for (int pat = 1; pat < 7; ++pat) { dir(pat, Nb, Na, nullptr); std::swap(Na, Nb); }
        dir(7, ln.d_front, Na, &pd.tail);
        ev_end_on(e, ln.stream);
    }
    pd.clear();
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_iterate(fl_ctx *c, fl_genome *g, uint32_t w, uint32_t h, double nsamples, uint32_t fuse,
               int accum_mode, uint64_t *nsamples_run)
{
    REQUIRE(c && g, "null argument");
    REQUIRE(accum_mode == FL_ACCUM_ATOMIC || accum_mode == FL_ACCUM_BINNED || accum_mode == 2, "bad accumulation mode");
    Lane &ln = c->lane();
    REQUIRE(ln.d_params.cap >= (size_t)c->ntemporal() * g->pstride, "fl_interp has not run for this genome");
    HIPCHK(hipSetDevice(c->device));
    fl_dim d;
    int rc = ensure_fb(ln, w, h, &d);
    if (rc) return rc;
    if ((rc = flush_pending(c, ln))) return rc;
    if ((rc = wait_other(c, 1))) return rc;                 // walkers / RNG states are shared between lanes
    if ((rc = do_clear(c, ln, d, true))) return rc;
    const double per_round = (double)c->npoints();
    uint64_t rounds = (uint64_t)ceil(nsamples / per_round);
    if (rounds == 0) rounds = 1;
    if (nsamples_run) *nsamples_run = (uint64_t)(rounds * per_round);
    // The launches of the frame (launch_plan.h), each followed by a flush; the first also carries the fuse rounds.  The long cap
    // saves a launch but sizes the (grow-only) sample log and directory for the longest launch: it is taken only if what
    // would have to be allocated beyond the short cap's buffers fits the device's free memory with a margin — a frame that rendered
    // with 1024-round logs must not start failing on a shared or smaller device because a schedule saves it a flush.
    const bool binned = accum_mode == FL_ACCUM_BINNED;
    LaunchPlan plan = binned ? launch_schedule(rounds, c->sub_log2, c->nw, c->launch_rounds) : launch_schedule_under(rounds, c->sub_log2, FL_NO_CAP);
    if (binned && !c->launch_rounds && plan.cap > launch_cap(false, c->sub_log2, c->nw)) {
        const size_t need = bin_set(c->layout(d), std::min(rounds, plan.cap), c->bin_rounds, c->nslots).bytes();
        size_t grow = 0, mfree = 0, mtotal = 0;
        for (int b = 0; b < 2; ++b) {                                            // (two sets: launches of a frame are pipelined)
            const size_t have = ln.d_log[b].bytes() + ln.d_dir[b].bytes();
            if (need > have) grow += need - have;
        }
        if (grow && (hipMemGetInfo(&mfree, &mtotal) != hipSuccess || grow + (size_t(1) << 30) > mfree))
            plan = launch_schedule_under(rounds, c->sub_log2, launch_cap(false, c->sub_log2, c->nw));
    }
    // The reference alternates two streams so that flush k overlaps iter k+1 (render.py:358-369).  Here, when a binned frame
    // needs several launches, the iterate kernels stay on the lane's stream and the tile accumulate
    // + flush of each launch go to the lane's aux stream, with two log / directory sets: launch k+1
    // iterates while launch k drains.  (Both kernels want the whole chip, so this buys little —
    // DESIGN.md §4.1 — but it costs nothing and hides the drains' launch gaps.)
    const bool pipelined = binned && plan.rounds.size() > 1 && !c->env_no_intra;
    hipStream_t drain = pipelined ? ln.aux : ln.stream;
    uint32_t k = 0;
    for (const uint32_t n : plan.rounds) {
        const uint32_t f = k == 0 ? fuse : 0;
        const int buf = pipelined ? (int)(k & 1u) : 0;
        // the drains of launch k-2 read this log / directory set: they must be done before it is rewritten
        if (pipelined && k >= 2) HIPCHK(hipStreamWaitEvent(ln.stream, ln.ev_ac[buf], 0));
        if ((rc = do_iter_launch(c, ln, g, d, n + f, f, false, accum_mode, buf, drain))) return rc;
        if ((rc = do_flush(c, ln, d, !binned, drain))) return rc;
        if (pipelined) HIPCHK(hipEventRecord(ln.ev_ac[buf], drain));
        ++k;
    }
    // the walkers are free once the last iterate kernel has run (the drain kernels that follow
    // touch only this lane's buffers)
    HIPCHK(hipEventRecord(ln.ev_iter_done, ln.stream));
    ln.iter_rec = true;
    if (pipelined) {                    // whatever comes next on this lane's stream sees the finished accumulator
        HIPCHK(hipStreamWaitEvent(ln.stream, ln.ev_ac[(k - 1) & 1u], 0));
        if (k >= 2) HIPCHK(hipStreamWaitEvent(ln.stream, ln.ev_ac[k & 1u], 0));
    }
    return FL_OK;
}

static void gauss7(float stdev, float *c)      // cuburn/filters.py:11-16
{
    float s = 0.0f;
    for (int i = 0; i < 7; ++i) { float x = (float)(i - 3); c[i] = expf(x * x / (-2.0f * stdev * stdev)); s += c[i]; }
    for (int i = 0; i < 7; ++i) c[i] /= s;
}

// What fl_filter refuses, found before it touches anything: an unknown id, too few scalars (or none to read), a bad `de` radius / curve,
// a `bloom` whose reach is above the limit or whose scalars are not finite.
static int check_filter(int id, const float *p, uint32_t np)
{
    static const struct { uint32_t np; const char *msg; } need[] = {
        {0, ""}, {5, "bilateral needs sstd,cstd,dstd,dpow,gspeed"}, {2, "logscale needs k1,k2"},
        {5, "colorclip needs vib,highpow,gam,lin,lingam"}, {4, "smearclip needs width,gam_m_1,lin,lingam"}, {1, "haloclip needs gam_m_1"},
        {4, "plainclip needs gam_m_1,lin,lingam,brightness"}, {1, "logencode needs degamma"}, {3, "de needs R,Rmin,curve"},
        {3, "bloom needs threshold,strength,tap_0 (then tap_1 .. tap_R)"}};
    if (id < FL_FILT_YUV || id > FL_FILT_BLOOM) return fail(FL_E_UNSUPPORTED, "unknown filter id", __FILE__, __LINE__);
    REQUIRE(np >= need[id].np, need[id].msg);
    REQUIRE(p || !need[id].np, "null filter scalars");
    if (id == FL_FILT_DE) {
        REQUIRE(!(p[0] > (float)FL_DE_MAX_RADIUS), "de: R above 96 px");
        REQUIRE(p[2] > 0.0f, "de: curve must be > 0");
    }
    if (id == FL_FILT_BLOOM) {
        REQUIRE(np - 3 <= FL_BLOOM_MAX_REACH, "bloom: more than 384 taps per side");
        for (uint32_t i = 0; i < np; ++i) REQUIRE(std::isfinite(p[i]), "bloom: non-finite threshold, strength or tap");
        REQUIRE(p[0] >= 0.0f, "bloom: threshold must be >= 0");
    }
    return FL_OK;
}

int fl_filter(fl_ctx *c, int id, uint32_t w, uint32_t h, const float *p, uint32_t np)
{
    REQUIRE(c, "null ctx");
    int rc = check_filter(id, p, np);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    fl_dim d;
    if ((rc = ensure_fb(ln, w, h, &d))) return rc;
    hipStream_t st = ln.stream;
    float k7[7];
    EvPair *e = ev_begin(c, c->filt_ev);
    bool took = false;
    switch (id) {                        // what is pending either takes this step along, or runs first
    case FL_FILT_BILATERAL: if (ln.pend.de) rc = flush_pending(c, ln); break;      // (a pending `yuv` stays: defer_bilateral absorbs it)
    case FL_FILT_LOGSCALE: if (!(took = ln.pend.try_take(id, p))) rc = flush_pending(c, ln); break;
    case FL_FILT_COLORCLIP: took = ln.pend.try_take(id, p); rc = flush_pending(c, ln); break;      // taken or not, the chain runs now
    default: rc = flush_pending(c, ln); break;
    }
    if (!rc && !took) switch (id) {
    case FL_FILT_YUV: ln.pend.defer_yuv(d); break;                     // runs with the next call
    case FL_FILT_BILATERAL: {            // cuburn/filters.py:62-95; one kernel per direction (de.hip), all eight deferred
        Bilateral b = {p[0], p[1], p[2], p[3], p[4], {}};
        gauss7(1.0f, b.k7);
        ln.pend.defer_bilateral(d, b);
    } break;
    case FL_FILT_LOGSCALE: launch_logscale(st, d, ln.d_front, p[0], p[1]); break;
    case FL_FILT_COLORCLIP: launch_colorclip(st, d, ln.d_front, p[0], p[1], p[2], p[3], p[4]); break;
    case FL_FILT_SMEARCLIP:              // cuburn/filters.py:142-163
        gauss7(p[0], k7);
        launch_gamma_full_hi(st, d, ln.d_side, ln.d_front);
        launch_full_blur(st, d, ln.d_back, ln.d_side, 2, 0, k7);
        launch_full_blur(st, d, ln.d_side, ln.d_back, 3, 0, k7);
        launch_full_blur(st, d, ln.d_back, ln.d_side, 0, 0, k7);
        launch_full_blur(st, d, ln.d_side, ln.d_back, 1, 0, k7);
        launch_smearclip(st, d, ln.d_front, ln.d_side, p[1], p[2], p[3]);
        break;
    case FL_FILT_HALOCLIP:               // cuburn/filters.py:113-130
        gauss7(1.0f, k7);
        launch_apply_gamma(st, d, ln.d_blur, ln.d_front, 0.1f);
        launch_den_blur_1c(st, d, (float *)ln.d_side.p, ln.d_blur, 2, 0, k7);
        launch_den_blur_1c(st, d, ln.d_blur, (const float *)ln.d_side.p, 3, 0, k7);
        launch_haloclip(st, d, ln.d_front, ln.d_blur, p[0]);
        break;
    case FL_FILT_PLAINCLIP: launch_plainclip(st, d, ln.d_front, p[0], p[1], p[2], p[3]); break;
    case FL_FILT_LOGENCODE:
        launch_logencode(st, d, ln.d_back, ln.d_front, p[0]);
        swap(ln.d_front, ln.d_back);
        break;
    case FL_FILT_DE:                     // not part of the deferred bilateral chain
        if (!(p[0] > 0.0f)) break;       // R <= 0: every bin stays where it is
        // in place on d_front; d_back / d_blur hold the staged sources
        launch_de_adaptive(st, d, ln.d_front, ln.d_back, ln.d_blur, ln.d_de_tmax, ln.d_de_sinv,
                           p[0], std::min(std::max(p[1], 0.0f), p[0]), p[2]);
        break;
    case FL_FILT_BLOOM:                  // in place on d_front; d_side holds the excess blurred along x
        launch_bloom(st, d, ln.d_front, ln.d_side, p + 2, (int)np - 3, p[0], p[1]);
        break;
    }
    ev_end(c, e);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_resample(fl_ctx *c, uint32_t w, uint32_t h, uint32_t ss, const float *taps, uint32_t ntaps)
{
    REQUIRE(c && taps && w && h, "null argument");
    REQUIRE(ss >= 1 && ss <= FL_RESAMPLE_MAX_SS, "resample: ss must be 1..4");
    REQUIRE(ntaps >= ss && ntaps <= ss + 2 * FL_GUTTER && (ntaps - ss) % 2 == 0,
            "resample: ntaps must lie in [ss, ss + 24] and have the parity of ss");
    REQUIRE(w <= 0x7fffffffu / ss && h <= 0x7fffffffu / ss, "resample: source size overflows");
    for (uint32_t i = 0; i < ntaps; ++i) REQUIRE(std::isfinite(taps[i]), "resample: non-finite tap");
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    fl_dim din;
    const fl_dim dout = calc_dim(w, h);
    int rc = ensure_fb(ln, ss * w, ss * h, &din);
    if (rc) return rc;
    EvPair *e = ev_begin(c, c->filt_ev);
    if (!(rc = flush_pending(c, ln))) {                     // a deferred yuv / DE belongs to the source size
        launch_resample(ln.stream, din, dout, (int)ss, ln.d_back, ln.d_front, taps, (int)ntaps);
        swap(ln.d_front, ln.d_back);
    }
    ev_end(c, e);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return FL_OK;
}

// One axis of fl_resize's tables, checked on the host; folds the table into `hash` on the way.
static int check_resize_axis(const int32_t *first, const float *taps, uint32_t n_out, uint32_t nt, uint32_t n_in, uint64_t *hash)
{
    REQUIRE(nt >= 1 && nt <= FL_RESIZE_MAX_TAPS && nt <= n_in, "resize: taps per output must lie in 1..50 and within the source's size");
    uint64_t hsh = *hash;
    for (uint32_t i = 0; i < n_out; ++i) {
        REQUIRE(first[i] >= 0 && (uint64_t)first[i] + nt <= n_in, "resize: a window reaches outside the source");
        hsh = (hsh ^ (uint32_t)first[i]) * 0x100000001b3ull;
    }
    for (size_t i = 0, n = (size_t)n_out * nt; i < n; ++i) {
        REQUIRE(std::isfinite(taps[i]), "resize: non-finite tap");
        uint32_t bits;
        memcpy(&bits, taps + i, 4);
        hsh = (hsh ^ bits) * 0x100000001b3ull;
    }
    *hash = hsh;
    return FL_OK;
}

int fl_resize(fl_ctx *c, uint32_t w, uint32_t h, uint32_t w2, uint32_t h2, const int32_t *xfirst, const float *xtaps, uint32_t nxt,
              const int32_t *yfirst, const float *ytaps, uint32_t nyt)
{
    REQUIRE(c && xfirst && xtaps && yfirst && ytaps, "null argument");
    REQUIRE(w && h && w2 && h2, "resize: zero size");
    REQUIRE(w <= 0x3fffffffu && h <= 0x3fffffffu, "resize: source size overflows");
    REQUIRE(w2 <= w && h2 <= h, "resize: the result is larger than the source (enlarging is not supported)");
    uint64_t hash = 0xcbf29ce484222325ull;
    int rc;
    if ((rc = check_resize_axis(xfirst, xtaps, w2, nxt, w, &hash)) || (rc = check_resize_axis(yfirst, ytaps, h2, nyt, h, &hash))) return rc;
    REQUIRE(resize_rows_fit(xfirst, w2, nxt), "resize: the x windows of 64 neighbouring outputs span more than 576 source bins (not a downscale's table)");
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    fl_dim din;
    const fl_dim dout = calc_dim(w2, h2);
    if ((rc = ensure_fb(ln, w, h, &din))) return rc;
    // the lane's device copy of these tables, or the least recently used place for one
    const uint32_t key[6] = {w, h, w2, h2, nxt, nyt};
    ResizeTables *t = nullptr;
    for (ResizeTables &q : ln.rz) if (q.used && q.hash == hash && !memcmp(q.key, key, sizeof key)) t = &q;
    if (!t) {
        t = &ln.rz[0];
        for (ResizeTables &q : ln.rz) if (q.used < t->used) t = &q;
        // kernels queued earlier may still read what this entry held
        HIPCHK(hipStreamSynchronize(ln.stream));
        t->used = 0;
        const size_t nx = (size_t)w2 * nxt, ny = (size_t)h2 * nyt;
        if ((rc = t->first.reserve((size_t)w2 + h2, "resize tables")) || (rc = t->taps.reserve(nx + ny, "resize tables"))) return rc;
        HIPCHK(hipMemcpy(t->first.p, xfirst, 4 * (size_t)w2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t->first.p + w2, yfirst, 4 * (size_t)h2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t->taps.p, xtaps, 4 * nx, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t->taps.p + nx, ytaps, 4 * ny, hipMemcpyHostToDevice));
        memcpy(t->key, key, sizeof key);
        t->hash = hash;
    }
    t->used = ++ln.rz_serial;
    EvPair *e = ev_begin(c, c->filt_ev);
    if (!(rc = flush_pending(c, ln))) {                     // a deferred yuv / DE belongs to the source size
        launch_resize(ln.stream, din, dout, ln.d_back, ln.d_side, ln.d_front, t->first.p, t->taps.p, (int)nxt,
                      t->first.p + w2, t->taps.p + (size_t)w2 * nxt, (int)nyt);
        swap(ln.d_front, ln.d_back);
    }
    ev_end(c, e);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return FL_OK;
}

size_t fl_output_bytes(uint32_t w, uint32_t h, int fmt)
{
    const size_t n = (size_t)w * h;
    switch (fmt) {
    case FL_OUT_RGBA8: return 4 * n;
    case FL_OUT_RGBA16: return 8 * n;
    case FL_OUT_YUV444P: return 3 * n;
    case FL_OUT_YUV444P10: case FL_OUT_YUV444P12: return 6 * n;
    case FL_OUT_YUV420P10: return 3 * n;                    // (n + 2 * n/4) * 2 bytes
    default: return 0;
    }
}

// What fl_output and the encoding outputs begin with: the front buffer, dithered and converted to `fmt`, in dst (null: the lane's
// pixel buffer).
static int convert_front(fl_ctx *c, Lane &ln, uint32_t w, uint32_t h, int fmt, void *dst)
{
    fl_dim d;
    int rc = ensure_fb(ln, w, h, &d);
    if (rc) return rc;
    if ((rc = flush_pending(c, ln))) return rc;             // deferred ends of the filter chain
    if ((rc = wait_other(c, 2))) return rc;                 // the dither RNG states are shared between lanes
    launch_f32_to_rgba(ln.stream, d, ln.d_front, c->rng_out(), FL_NOUT, fmt, dst ? dst : (void *)ln.d_outpix.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ln.ev_out_done, ln.stream));
    ln.out_rec = true;
    return FL_OK;
}

// ... and end with, behind the encode and the copy to the host: the frame's end moves here (fl_frame_begin recorded it first)
static int close_frame(fl_ctx *c, Lane &ln)
{
    if (c->frame_seq) HIPCHK(hipEventRecord(c->ev_end_[(c->frame_seq - 1) % fl_ctx::kFrames], ln.stream));
    return FL_OK;
}

int fl_output(fl_ctx *c, uint32_t w, uint32_t h, int fmt, void *host_out, uint64_t dev_out)
{
    REQUIRE(c && fl_output_bytes(w, h, fmt) != 0, "bad argument");
    REQUIRE(fmt != FL_OUT_YUV420P10 || (w % 2 == 0 && h % 2 == 0), "4:2:0 needs even width and height");
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    void *dev = (void *)(uintptr_t)dev_out;
    if (int rc = convert_front(c, ln, w, h, fmt, dev)) return rc;
    if (host_out) HIPCHK(hipMemcpyAsync(host_out, dev ? dev : (void *)ln.d_outpix.p, fl_output_bytes(w, h, fmt), hipMemcpyDeviceToHost, ln.stream));
    return close_frame(c, ln);
}

// ---- files and frame blocks encoded on the device (jpeg.hip, png.hip, tiff.hip, exr.hip, gif.hip, webp.hip; DESIGN.md §4.8 and
// §4.9 .. §4.17): stills as JPEG, PNG, TIFF and OpenEXR, animations' frames as JPEG (Motion-JPEG), GIF, WebP and APNG blocks ----
static bool sides_ok(uint32_t w, uint32_t h, uint32_t max = 65535u) { return w >= 1 && h >= 1 && w <= max && h <= max; }

// What every encoder asks of a call: a context, a frame whose sides fit the formats' 16 bits, room for the record and the
// header (the placement kernel stores them whatever the status), and somewhere to put the file.  An encoder whose header's size
// comes from a layout (tiff, exr) calls check_sides itself before it asks for the layout: one of other sides means nothing.
static int check_sides(const char *enc, uint32_t w, uint32_t h)
{
    if (sides_ok(w, h)) return FL_OK;
    return fail(FL_E_INVAL, (std::string(enc) + ": width and height must be 1..65535").c_str(), __FILE__, __LINE__);
}
static int check_encode(const fl_ctx *c, const char *enc, uint32_t w, uint32_t h, size_t header, const void *host_out, uint64_t dev_out, size_t cap)
{
    REQUIRE(c, "null ctx");
    if (int rc = check_sides(enc, w, h)) return rc;
    const char *bad = cap < 16 + header ? "capacity below the record and the header" : !(host_out || dev_out) ? "no destination" : nullptr;
    if (!bad) return FL_OK;
    return fail(FL_E_INVAL, (std::string(enc) + ": " + bad).c_str(), __FILE__, __LINE__);
}

// The two shapes of an encoder's entry point.  check(): the encoder's own refusals, in its own order; encode(lane): its X_encode_on.
// From the caller's source: a null source is refused behind `check`, and `late()` holds what the entry point refuses behind that.
extern "C++" template <class Check, class Encode, class Late = int (*)()>
static int encode_source(fl_ctx *c, uint64_t src_dev, const char *no_source, Check check, Encode encode, Late late = +[] { return (int)FL_OK; })
{
    if (int rc = check()) return rc;
    REQUIRE(src_dev, no_source);
    if (int rc = late()) return rc;
    HIPCHK(hipSetDevice(c->device));
    return encode(c->lane());
}

// From the front buffer: source(lane) makes the encoder's source ready, and the frame's end moves behind the encode.
extern "C++" template <class Check, class Source, class Encode>
static int encode_front(fl_ctx *c, Check check, Source source, Encode encode)
{
    if (int rc = check()) return rc;
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    if (int rc = source(ln)) return rc;
    if (int rc = encode(ln)) return rc;
    return close_frame(c, ln);
}
// ... dithered and converted to `fmt` in the lane's pixel buffer, which is what encode(lane) then reads
extern "C++" template <class Check, class Encode>
static int encode_front(fl_ctx *c, uint32_t w, uint32_t h, int fmt, Check check, Encode encode)
{
    return encode_front(c, check, [=](Lane &ln) { return convert_front(c, ln, w, h, fmt, nullptr); }, encode);
}

// One encode, queued on the lane's stream (arguments checked).  Where the kernels store: the caller's device buffer; else the
// caller's host buffer through its device address when it is pinned; else the lane's staging buffer, copied to the host afterwards.
// bound: the encoder's fl_*_bound, so min(cap, bound) is what a fitting file can occupy; launch(scratch, dst) queues the kernels.
extern "C++" template <class Launch>                            // (inside the extern "C" block a template needs its own linkage)
static int encode_on(fl_ctx *c, Lane &ln, void *host_out, uint64_t dev_out, size_t cap, size_t bound, size_t scratch_words,
                     const char *what_out, const char *what_scratch, Launch launch)
{
    unsigned char *dst = (unsigned char *)(uintptr_t)dev_out;
    bool copy_back = host_out && dst;
    const size_t dcap = std::min(cap, bound);
    const auto quiesce = [&ln] { return ln.quiesce(false); };
    if (!dst) {
        hipPointerAttribute_t at = {};
        const hipError_t e = hipPointerGetAttributes(&at, host_out);
        if (e == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer) dst = (unsigned char *)at.devicePointer;
        else {
            (void)hipGetLastError();                            // (not a pointer the runtime knows: plain host memory)
            if (int rc = ln.d_enc_out.reserve(dcap, what_out, quiesce)) return rc;
            dst = ln.d_enc_out;
            copy_back = true;
        }
    }
    if (int rc = ln.d_enc.reserve(scratch_words, what_scratch, quiesce)) return rc;
    EvPair *e = ev_begin_on(c, c->enc_ev, ln.stream);           // (slot 5 of fl_timings_detail: every device encoder)
    launch(ln.d_enc.p, dst);
    ev_end_on(e, ln.stream);
    HIPCHK(hipGetLastError());
    if (copy_back) HIPCHK(hipMemcpyAsync(host_out, dst, dcap, hipMemcpyDeviceToHost, ln.stream));
    return FL_OK;
}

// ---- JPEG ----
// No stream can be longer: a block codes its DC difference in at most 11 + 11 bits (the longest code of table K.4, category 11)
// and each of its 63 AC coefficients in at most 16 + 10 (the longest code of K.5 / K.6, category 10; ZRL and EOB stand for
// coefficients that then cost nothing): 22 + 63 * 26 = 1660 bits, 4980 per MCU of three blocks, 623 bytes once padded.  Every one
// of those bytes can be 0xFF and take a stuffed zero with it, and the shortest restart interval — one MCU — puts a two-byte
// marker (RSTm, or EOI) behind each: 2 * 623 + 2 = 1248 bytes per MCU.  Longer intervals pad and mark less often.
// 4:2:0 by the same rule: an MCU of six blocks is 9960 bits, 1245 bytes, 2 * 1245 + 2 = 2492.
size_t fl_jpeg_bound_s(uint32_t w, uint32_t h, int sampling)
{
    if (!sides_ok(w, h) || (sampling != FL_JPEG_444 && sampling != FL_JPEG_420)) return 0;
    if (sampling == FL_JPEG_420) return 16 + FL_JPEG_HEADER_BYTES + (size_t)((w + 15u) / 16u) * ((h + 15u) / 16u) * 2492u;
    return 16 + FL_JPEG_HEADER_BYTES + (size_t)((w + 7u) / 8u) * ((h + 7u) / 8u) * 1248u;
}

size_t fl_jpeg_bound(uint32_t w, uint32_t h) { return fl_jpeg_bound_s(w, h, FL_JPEG_444); }

// FL_JPEG_OPTIMIZE, by the same rule with the longest codes a frame's own tables can have: a DC table of 13 leaves (the 12
// categories and the pseudo-symbol) has no code above 12 bits, an AC code is limited to 16: 12 + 11 + 63 * 26 = 1661 bits a block.
// 4:4:4: 4983 bits, 623 bytes, 1248 per MCU as before; 4:2:0: 9966 bits, 1246 bytes, 2 * 1246 + 2 = 2494.
// The symbol counts must fit the table builder's 32-bit sums: no more than FL_JPEG_OPT_MAX_BLOCKS blocks.
static uint64_t jpeg_blocks(uint32_t w, uint32_t h, int sampling)
{
    return sampling == FL_JPEG_420 ? (uint64_t)((w + 15u) / 16u) * ((h + 15u) / 16u) * 6u : (uint64_t)((w + 7u) / 8u) * ((h + 7u) / 8u) * 3u;
}

size_t fl_jpeg_bound_f(uint32_t w, uint32_t h, int sampling, unsigned flags)
{
    if (!flags) return fl_jpeg_bound_s(w, h, sampling);
    if (flags != FL_JPEG_OPTIMIZE || !fl_jpeg_bound_s(w, h, sampling) || jpeg_blocks(w, h, sampling) > FL_JPEG_OPT_MAX_BLOCKS) return 0;
    if (sampling == FL_JPEG_420) return 16 + FL_JPEG_HEADER_BYTES + (size_t)((w + 15u) / 16u) * ((h + 15u) / 16u) * 2494u;
    return 16 + FL_JPEG_HEADER_BYTES + (size_t)((w + 7u) / 8u) * ((h + 7u) / 8u) * 1248u;
}

static int check_jpeg(const fl_ctx *c, uint32_t w, uint32_t h, int quality, int sampling, unsigned flags, const void *host_out, uint64_t dev_out, size_t cap)
{
    if (int rc = check_encode(c, "jpeg", w, h, FL_JPEG_HEADER_BYTES, host_out, dev_out, cap)) return rc;
    REQUIRE(quality >= 1 && quality <= 100, "jpeg: quality must be 1..100");
    REQUIRE(sampling == FL_JPEG_444 || sampling == FL_JPEG_420, "jpeg: sampling must be FL_JPEG_444 or FL_JPEG_420");
    REQUIRE(!(flags & ~(unsigned)FL_JPEG_OPTIMIZE), "jpeg: unknown flag");
    if (flags && jpeg_blocks(w, h, sampling) > FL_JPEG_OPT_MAX_BLOCKS) return fail(FL_E_UNSUPPORTED, "jpeg: FL_JPEG_OPTIMIZE takes frames of at most 2^24 blocks", __FILE__, __LINE__);
    return FL_OK;
}

static int jpeg_encode_on(fl_ctx *c, Lane &ln, uint32_t w, uint32_t h, const unsigned char *src, int quality, int sampling, unsigned flags,
                          void *host_out, uint64_t dev_out, size_t cap)
{
    const uint32_t ri = sampling == FL_JPEG_420 ? c->jpeg_ri_420 : c->jpeg_ri;
    const bool optimize = flags & FL_JPEG_OPTIMIZE;
    return encode_on(c, ln, host_out, dev_out, cap, fl_jpeg_bound_f(w, h, sampling, flags), jpeg_layout(w, h, ri, sampling).words, "jpeg stream", "jpeg scratch",
                     [=, st = ln.stream](uint32_t *scratch, unsigned char *dst) { launch_jpeg_encode(st, src, w, h, quality, ri, sampling, optimize, scratch, dst, cap); });
}

int fl_jpeg_encode_f(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, int quality, int sampling, unsigned flags, void *host_out, uint64_t dev_out,
                     size_t cap)
{
    return encode_source(c, src_dev, "jpeg: null source planes", [&] { return check_jpeg(c, w, h, quality, sampling, flags, host_out, dev_out, cap); },
                         [&](Lane &ln) { return jpeg_encode_on(c, ln, w, h, (const unsigned char *)(uintptr_t)src_dev, quality, sampling, flags, host_out, dev_out, cap); });
}

int fl_jpeg_encode_s(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, int quality, int sampling, void *host_out, uint64_t dev_out, size_t cap)
{
    return fl_jpeg_encode_f(c, w, h, src_dev, quality, sampling, 0u, host_out, dev_out, cap);
}

int fl_jpeg_encode(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, int quality, void *host_out, uint64_t dev_out, size_t cap)
{
    return fl_jpeg_encode_s(c, w, h, src_dev, quality, FL_JPEG_444, host_out, dev_out, cap);
}

int fl_output_jpeg_f(fl_ctx *c, uint32_t w, uint32_t h, int quality, int sampling, unsigned flags, void *host_out, uint64_t dev_out, size_t cap)
{
    return encode_front(c, w, h, FL_OUT_YUV444P, [&] { return check_jpeg(c, w, h, quality, sampling, flags, host_out, dev_out, cap); },
                        [&](Lane &ln) { return jpeg_encode_on(c, ln, w, h, ln.d_outpix, quality, sampling, flags, host_out, dev_out, cap); });
}

int fl_output_jpeg_s(fl_ctx *c, uint32_t w, uint32_t h, int quality, int sampling, void *host_out, uint64_t dev_out, size_t cap)
{
    return fl_output_jpeg_f(c, w, h, quality, sampling, 0u, host_out, dev_out, cap);
}

int fl_output_jpeg(fl_ctx *c, uint32_t w, uint32_t h, int quality, void *host_out, uint64_t dev_out, size_t cap)
{
    return fl_output_jpeg_s(c, w, h, quality, FL_JPEG_444, host_out, dev_out, cap);
}

// ---- PNG ----
// No file can be longer: every segment stored is its bytes and 5 of block header, in an IDAT of 12; the first IDAT also holds the
// 2 bytes of the zlib header and the last the Adler-32; IEND is 12.  A dynamic segment is only chosen where it is smaller.
// Rows of 1 + w * channels * bits / 8 bytes; the filter choice changes no size.  (A frame over the limit at 8 bits is over it at 16.)
size_t fl_png_bound_f(uint32_t w, uint32_t h, int channels, int bits, unsigned flags)
{
    if (!sides_ok(w, h) || (channels != 3 && channels != 4)) return 0;
    if ((bits != 8 && bits != 16) || (flags & ~(unsigned)FL_PNG_ADAPTIVE)) return 0;
    const uint64_t F = (uint64_t)h * (1u + (uint64_t)w * (uint32_t)(channels * bits / 8)), seg = png_segment_bytes();
    const uint64_t n = 16u + FL_PNG_HEADER_BYTES + 2u + F + 17u * ((F + seg - 1u) / seg) + 4u + 12u;
    return n > 0xffffffffull ? 0 : (size_t)n;
}

size_t fl_png_bound(uint32_t w, uint32_t h, int channels) { return fl_png_bound_f(w, h, channels, 8, 0u); }

static int check_png(const fl_ctx *c, uint32_t w, uint32_t h, int channels, const void *host_out, uint64_t dev_out, size_t cap,
                     size_t header = FL_PNG_HEADER_BYTES)      // (a frame block of fl_apng_encode has none)
{
    if (int rc = check_encode(c, "png", w, h, header, host_out, dev_out, cap)) return rc;
    REQUIRE(channels == 3 || channels == 4, "png: channels must be 3 or 4");
    REQUIRE(fl_png_bound(w, h, channels) != 0, "png: the file could pass 2^32 - 1 bytes");
    return FL_OK;
}

// What the _f entry points refuse beyond check_png (and, in fl_png_encode_f, the null source), after those
static int check_png_f(uint32_t w, uint32_t h, int channels, int bits, unsigned flags)
{
    REQUIRE(bits == 8 || bits == 16, "png: bits must be 8 or 16");
    REQUIRE(!(flags & ~(unsigned)FL_PNG_ADAPTIVE), "png: unknown flag");
    REQUIRE(fl_png_bound_f(w, h, channels, bits, flags) != 0, "png: the file could pass 2^32 - 1 bytes");
    return FL_OK;
}

static int png_encode_on(fl_ctx *c, Lane &ln, uint32_t w, uint32_t h, const unsigned char *src, int channels, int bits, unsigned flags,
                         void *host_out, uint64_t dev_out, size_t cap)
{
    const uint32_t seg = png_segment_bytes();
    return encode_on(c, ln, host_out, dev_out, cap, fl_png_bound_f(w, h, channels, bits, flags), png_layout(w, h, channels, seg, bits, flags).words,
                     "png file", "png scratch", [=, st = ln.stream](uint32_t *scratch, unsigned char *dst) {
                         launch_png_encode(st, src, w, h, channels, bits, flags, seg, scratch, dst, cap);
                     });
}

int fl_png_encode_f(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, int channels, int bits, unsigned flags, void *host_out, uint64_t dev_out,
                    size_t cap)
{
    return encode_source(c, src_dev, "png: null source pixels", [&] { return check_png(c, w, h, channels, host_out, dev_out, cap); },
                         [&](Lane &ln) { return png_encode_on(c, ln, w, h, (const unsigned char *)(uintptr_t)src_dev, channels, bits, flags, host_out, dev_out, cap); },
                         [&] { return check_png_f(w, h, channels, bits, flags); });
}

int fl_png_encode(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, int channels, void *host_out, uint64_t dev_out, size_t cap)
{
    return fl_png_encode_f(c, w, h, src_dev, channels, 8, 0u, host_out, dev_out, cap);
}

int fl_output_png_f(fl_ctx *c, uint32_t w, uint32_t h, int channels, int bits, unsigned flags, void *host_out, uint64_t dev_out, size_t cap)
{
    return encode_front(c, w, h, bits == 16 ? FL_OUT_RGBA16 : FL_OUT_RGBA8,
                        [&] { const int rc = check_png(c, w, h, channels, host_out, dev_out, cap); return rc ? rc : check_png_f(w, h, channels, bits, flags); },
                        [&](Lane &ln) { return png_encode_on(c, ln, w, h, ln.d_outpix, channels, bits, flags, host_out, dev_out, cap); });
}

int fl_output_png(fl_ctx *c, uint32_t w, uint32_t h, int channels, void *host_out, uint64_t dev_out, size_t cap)
{
    return fl_output_png_f(c, w, h, channels, 8, 0u, host_out, dev_out, cap);
}

// ---- APNG frame blocks ----
// The PNG's chunks without the 33 bytes in front of them and the 12 of IEND, and 4 more per chunk where they are fdATs.
uint32_t fl_apng_chunks(uint32_t w, uint32_t h, int channels, int bits)
{
    if (!fl_png_bound_f(w, h, channels, bits, 0u)) return 0;
    const uint64_t F = (uint64_t)h * (1u + (uint64_t)w * (uint32_t)(channels * bits / 8)), seg = png_segment_bytes();
    return (uint32_t)((F + seg - 1u) / seg);
}

size_t fl_apng_bound(uint32_t w, uint32_t h, int channels, int bits, unsigned flags)
{
    const size_t png = fl_png_bound_f(w, h, channels, bits, flags);
    return png ? png - FL_PNG_HEADER_BYTES - 12u + 4u * (size_t)fl_apng_chunks(w, h, channels, bits) : 0;
}

// What a frame block refuses beyond check_png (with no header) and, in fl_apng_encode, the null source, after those
static int check_apng_f(uint32_t w, uint32_t h, int channels, int bits, unsigned flags, uint32_t seq)
{
    if (int rc = check_png_f(w, h, channels, bits, flags)) return rc;
    // the last chunk's number is seq + chunks - 1, and 0xffffffff is no number: it asks for IDATs
    REQUIRE(seq == FL_APNG_IDAT || fl_apng_chunks(w, h, channels, bits) - 1u <= 0xfffffffeu - seq, "apng: the frame's sequence numbers would pass 0xfffffffe");
    return FL_OK;
}

static int apng_encode_on(fl_ctx *c, Lane &ln, uint32_t w, uint32_t h, const unsigned char *src, int channels, int bits, unsigned flags,
                          uint32_t seq, void *host_out, uint64_t dev_out, size_t cap)
{
    const uint32_t seg = png_segment_bytes();
    return encode_on(c, ln, host_out, dev_out, cap, fl_apng_bound(w, h, channels, bits, flags), png_layout(w, h, channels, seg, bits, flags).words,
                     "apng frame block", "png scratch", [=, st = ln.stream](uint32_t *scratch, unsigned char *dst) {
                         launch_apng_encode(st, src, w, h, channels, bits, flags, seg, seq, scratch, dst, cap);
                     });
}

int fl_apng_encode(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, int channels, int bits, unsigned flags, uint32_t seq, void *host_out,
                   uint64_t dev_out, size_t cap)
{
    return encode_source(c, src_dev, "png: null source pixels", [&] { return check_png(c, w, h, channels, host_out, dev_out, cap, 0); },
                         [&](Lane &ln) { return apng_encode_on(c, ln, w, h, (const unsigned char *)(uintptr_t)src_dev, channels, bits, flags, seq, host_out, dev_out, cap); },
                         [&] { return check_apng_f(w, h, channels, bits, flags, seq); });
}

int fl_output_apng(fl_ctx *c, uint32_t w, uint32_t h, int channels, int bits, unsigned flags, uint32_t seq, void *host_out, uint64_t dev_out,
                   size_t cap)
{
    return encode_front(c, w, h, bits == 16 ? FL_OUT_RGBA16 : FL_OUT_RGBA8,
                        [&] { const int rc = check_png(c, w, h, channels, host_out, dev_out, cap, 0); return rc ? rc : check_apng_f(w, h, channels, bits, flags, seq); },
                        [&](Lane &ln) { return apng_encode_on(c, ln, w, h, ln.d_outpix, channels, bits, flags, seq, host_out, dev_out, cap); });
}

// ---- TIFF ----
// No file can be longer: every tile stored is its bytes and 5 of block header between the 2 bytes of its zlib header and the 4 of its
// Adler-32, and a pad byte; in front of them the header, the IFD, BitsPerSample and — with more than one tile — both arrays.
size_t fl_tiff_bound(uint32_t w, uint32_t h, int channels, int bits)
{
    if (!sides_ok(w, h) || (channels != 3 && channels != 4) || (bits != 8 && bits != 16)) return 0;
    const TiffLayout l = tiff_layout(w, h, channels, bits);
    const uint64_t n = 16u + l.H + (uint64_t)l.nt * (l.tile_bytes + 5u + 6u + 1u);
    return n > 0xffffffffull ? 0 : (size_t)n;
}

static int check_tiff(const fl_ctx *c, uint32_t w, uint32_t h, int channels, int bits, const void *host_out, uint64_t dev_out, size_t cap)
{
    REQUIRE(c, "null ctx");
    REQUIRE(channels == 3 || channels == 4, "tiff: channels must be 3 or 4");
    REQUIRE(bits == 8 || bits == 16, "tiff: bits must be 8 or 16");
    if (int rc = check_sides("tiff", w, h)) return rc;
    if (int rc = check_encode(c, "tiff", w, h, (size_t)tiff_layout(w, h, channels, bits).H, host_out, dev_out, cap)) return rc;
    REQUIRE(fl_tiff_bound(w, h, channels, bits) != 0, "tiff: the file could pass 2^32 - 1 bytes");
    return FL_OK;
}

static int tiff_encode_on(fl_ctx *c, Lane &ln, uint32_t w, uint32_t h, const unsigned char *src, int channels, int bits, void *host_out,
                          uint64_t dev_out, size_t cap)
{
    return encode_on(c, ln, host_out, dev_out, cap, fl_tiff_bound(w, h, channels, bits), tiff_layout(w, h, channels, bits).words, "tiff file",
                     "tiff scratch", [=, st = ln.stream](uint32_t *scratch, unsigned char *dst) {
                         launch_tiff_encode(st, src, w, h, channels, bits, scratch, dst, cap);
                     });
}

int fl_tiff_encode(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, int channels, int bits, void *host_out, uint64_t dev_out, size_t cap)
{
    return encode_source(c, src_dev, "tiff: null source pixels", [&] { return check_tiff(c, w, h, channels, bits, host_out, dev_out, cap); },
                         [&](Lane &ln) { return tiff_encode_on(c, ln, w, h, (const unsigned char *)(uintptr_t)src_dev, channels, bits, host_out, dev_out, cap); });
}

int fl_output_tiff(fl_ctx *c, uint32_t w, uint32_t h, int channels, int bits, void *host_out, uint64_t dev_out, size_t cap)
{
    return encode_front(c, w, h, bits == 16 ? FL_OUT_RGBA16 : FL_OUT_RGBA8, [&] { return check_tiff(c, w, h, channels, bits, host_out, dev_out, cap); },
                        [&](Lane &ln) { return tiff_encode_on(c, ln, w, h, ln.d_outpix, channels, bits, host_out, dev_out, cap); });
}

// ---- OpenEXR ----
// No file can be longer, and a file of noise is exactly this long: every tile raw behind the 20 bytes of its chunk's head and the
// 8 of its place in the offset table.  A zlib stream is only chosen where it is smaller.
size_t fl_exr_bound(uint32_t w, uint32_t h, int channels, int pixel)
{
    if (!sides_ok(w, h) || (channels != 3 && channels != 4) || (pixel != FL_EXR_HALF && pixel != FL_EXR_FLOAT)) return 0;
    const ExrLayout l = exr_layout(w, h, channels, pixel);
    const uint64_t n = 16u + l.H + 20ull * l.nt + l.raw;
    return n > 0xffffffffull ? 0 : (size_t)n;
}

static int check_exr(const fl_ctx *c, uint32_t w, uint32_t h, int channels, int pixel, const void *host_out, uint64_t dev_out, size_t cap)
{
    REQUIRE(c, "null ctx");
    REQUIRE(channels == 3 || channels == 4, "exr: channels must be 3 or 4");
    REQUIRE(pixel == FL_EXR_HALF || pixel == FL_EXR_FLOAT, "exr: pixel must be FL_EXR_HALF or FL_EXR_FLOAT");
    if (int rc = check_sides("exr", w, h)) return rc;
    if (int rc = check_encode(c, "exr", w, h, (size_t)exr_layout(w, h, channels, pixel).H, host_out, dev_out, cap)) return rc;
    REQUIRE(fl_exr_bound(w, h, channels, pixel) != 0, "exr: the file could pass 2^32 - 1 bytes");
    return FL_OK;
}

static int exr_encode_on(fl_ctx *c, Lane &ln, uint32_t w, uint32_t h, const float4 *src, uint32_t src_stride, int channels, int pixel,
                         void *host_out, uint64_t dev_out, size_t cap)
{
    return encode_on(c, ln, host_out, dev_out, cap, fl_exr_bound(w, h, channels, pixel), exr_layout(w, h, channels, pixel).words, "exr file",
                     "exr scratch", [=, st = ln.stream](uint32_t *scratch, unsigned char *dst) {
                         launch_exr_encode(st, src, src_stride, w, h, channels, pixel, scratch, dst, cap);
                     });
}

int fl_exr_encode(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, uint32_t src_stride, int channels, int pixel, void *host_out,
                  uint64_t dev_out, size_t cap)
{
    return encode_source(c, src_dev, "exr: null source pixels", [&] { return check_exr(c, w, h, channels, pixel, host_out, dev_out, cap); },
                         [&](Lane &ln) { return exr_encode_on(c, ln, w, h, (const float4 *)(uintptr_t)src_dev, src_stride, channels, pixel, host_out, dev_out, cap); },
                         [&]() -> int { REQUIRE(src_stride >= w, "exr: the source's stride is below the width"); return FL_OK; });
}

// The front buffer itself is the source: no conversion pass, no dither draw, so nothing of the state the lanes share is touched.
int fl_output_exr(fl_ctx *c, uint32_t w, uint32_t h, int channels, int pixel, void *host_out, uint64_t dev_out, size_t cap)
{
    fl_dim d;
    return encode_front(c, [&] { return check_exr(c, w, h, channels, pixel, host_out, dev_out, cap); },
                        [&](Lane &ln) { const int rc = ensure_fb(ln, w, h, &d); return rc ? rc : flush_pending(c, ln); },      // (deferred ends of the filter chain)
                        [&](Lane &ln) {
                            const float4 *src = (const float4 *)ln.d_front.p + (size_t)d.astride * FL_GUTTER + FL_GUTTER;
                            return exr_encode_on(c, ln, w, h, src, d.astride, channels, pixel, host_out, dev_out, cap);
                        });
}

// ---- GIF ----
// No block can be longer: a segment of n pixels is CLEAR in 9 bits, at most n codes of at most 12, the closing code in 12 and at most
// seven CLEARs of 9 as padding, 12 n + 84 bits, under 3 n / 2 + 11 bytes; segments are never shorter than 256 pixels but the last.
size_t fl_gif_bound(uint32_t w, uint32_t h)
{
    if (!sides_ok(w, h) || (uint64_t)w * h > (1ull << 24)) return 0;
    const uint64_t n = (uint64_t)w * h, T = (3u * n + 1u) / 2u + 11u * ((n + 255u) / 256u);
    return (size_t)(16u + FL_GIF_HEADER_BYTES + T + (T + 254u) / 255u + 1u);
}

static int check_gif(const fl_ctx *c, uint32_t w, uint32_t h, int colors, int amp, const void *host_out, uint64_t dev_out, size_t cap)
{
    if (int rc = check_encode(c, "gif", w, h, FL_GIF_HEADER_BYTES, host_out, dev_out, cap)) return rc;
    REQUIRE(colors >= 2 && colors <= 256, "gif: colors must be 2..256");
    REQUIRE(amp >= 0 && amp <= 64, "gif: dither_amp must be 0..64");
    REQUIRE(fl_gif_bound(w, h) != 0, "gif: the frame has more than 2^24 pixels");
    return FL_OK;
}

static int gif_encode_on(fl_ctx *c, Lane &ln, uint32_t w, uint32_t h, const unsigned char *src, int colors, int amp, void *host_out,
                         uint64_t dev_out, size_t cap)
{
    const uint32_t seg = c->gif_seg;
    return encode_on(c, ln, host_out, dev_out, cap, fl_gif_bound(w, h), gif_layout(w, h, seg).words, "gif block", "gif scratch",
                     [=, st = ln.stream](uint32_t *scratch, unsigned char *dst) { launch_gif_encode(st, src, w, h, colors, amp, seg, scratch, dst, cap); });
}

int fl_gif_encode(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, int colors, int dither_amp, void *host_out, uint64_t dev_out, size_t cap)
{
    return encode_source(c, src_dev, "gif: null source pixels", [&] { return check_gif(c, w, h, colors, dither_amp, host_out, dev_out, cap); },
                         [&](Lane &ln) { return gif_encode_on(c, ln, w, h, (const unsigned char *)(uintptr_t)src_dev, colors, dither_amp, host_out, dev_out, cap); });
}

int fl_output_gif(fl_ctx *c, uint32_t w, uint32_t h, int colors, int dither_amp, void *host_out, uint64_t dev_out, size_t cap)
{
    return encode_front(c, w, h, FL_OUT_RGBA8, [&] { return check_gif(c, w, h, colors, dither_amp, host_out, dev_out, cap); },
                        [&](Lane &ln) { return gif_encode_on(c, ln, w, h, ln.d_outpix, colors, dither_amp, host_out, dev_out, cap); });
}

// ---- WebP ----
// No block can be longer: the proof is with the declaration in include/flame_hip.h.
size_t fl_webp_bound(uint32_t w, uint32_t h, int channels)
{
    if (!sides_ok(w, h, 16384u) || (channels != 3 && channels != 4)) return 0;
    const uint64_t n = 16u + 8u + (webp_bound_bits(w, h) + 7u) / 8u + 1u;
    return n > 0xffffffffull ? 0 : (size_t)n;
}

static int check_webp(const fl_ctx *c, uint32_t w, uint32_t h, int channels, const void *host_out, uint64_t dev_out, size_t cap)
{
    if (int rc = check_encode(c, "webp", w, h, FL_WEBP_HEADER_BYTES, host_out, dev_out, cap)) return rc;
    REQUIRE(channels == 3 || channels == 4, "webp: channels must be 3 or 4");
    REQUIRE(sides_ok(w, h, 16384u), "webp: width and height must be 1..16384");
    REQUIRE(fl_webp_bound(w, h, channels) != 0, "webp: the block could pass 2^32 - 1 bytes");
    return FL_OK;
}

static int webp_encode_on(fl_ctx *c, Lane &ln, uint32_t w, uint32_t h, const unsigned char *src, int channels, void *host_out, uint64_t dev_out,
                          size_t cap)
{
    const size_t bound = fl_webp_bound(w, h, channels);
    return encode_on(c, ln, host_out, dev_out, cap, bound, webp_layout(w, h).words, "webp block", "webp scratch",
                     [=, st = ln.stream](uint32_t *scratch, unsigned char *dst) { launch_webp_encode(st, src, w, h, channels, scratch, dst, cap, bound); });
}

int fl_webp_encode(fl_ctx *c, uint32_t w, uint32_t h, uint64_t src_dev, int channels, void *host_out, uint64_t dev_out, size_t cap)
{
    return encode_source(c, src_dev, "webp: null source pixels", [&] { return check_webp(c, w, h, channels, host_out, dev_out, cap); },
                         [&](Lane &ln) { return webp_encode_on(c, ln, w, h, (const unsigned char *)(uintptr_t)src_dev, channels, host_out, dev_out, cap); });
}

int fl_output_webp(fl_ctx *c, uint32_t w, uint32_t h, int channels, void *host_out, uint64_t dev_out, size_t cap)
{
    return encode_front(c, w, h, FL_OUT_RGBA8, [&] { return check_webp(c, w, h, channels, host_out, dev_out, cap); },
                        [&](Lane &ln) { return webp_encode_on(c, ln, w, h, ln.d_outpix, channels, host_out, dev_out, cap); });
}

int fl_sort_u32(fl_ctx *c, uint64_t dst_dev, uint64_t src_dev, uint32_t n, uint32_t lo_bit, uint32_t nbits, int ignore_max,
                uint32_t *nvalid)
{
    REQUIRE(c && dst_dev && src_dev && dst_dev != src_dev, "null or aliased key arrays");
    REQUIRE(nbits >= 1 && nbits <= 10 && lo_bit + nbits <= 32, "a pass sorts 1..10 bits inside the 32-bit key");
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) { if (nvalid) *nvalid = 0; return FL_OK; }
    size_t chunk_words = 0;
    const size_t hist_words = sort_scratch_words(n, nbits, &chunk_words);
    // Every pass runs on lane 0's stream whatever lane the frame loop is on: consecutive passes of a
    // multi-pass sort stay ordered across frame boundaries, and the scratch has ONE user stream.
    hipStream_t sst = c->lanes[0].stream;
    // (nothing may still be using the old scratch)
    if (int rc = c->d_sort.reserve(hist_words + chunk_words, "sort scratch", [c] { sync_all(c); return (int)FL_OK; })) return rc;
    uint32_t *chunk_tot = c->d_sort + hist_words, *total_dev = chunk_tot + (chunk_words - 1);
    launch_sort_pass(sst, (uint32_t *)(uintptr_t)dst_dev, (const uint32_t *)(uintptr_t)src_dev, n, lo_bit, nbits,
                     ignore_max, c->d_sort, chunk_tot, total_dev);
    HIPCHK(hipGetLastError());
    if (nvalid) {                                           // the reference leaves this count on the device (sort.py:449-452)
        HIPCHK(hipMemcpyAsync(nvalid, total_dev, 4, hipMemcpyDeviceToHost, sst));
        HIPCHK(hipStreamSynchronize(sst));
    }
    return FL_OK;
}

int fl_frame_ms(fl_ctx *c, uint32_t frame_id, float *ms)
{
    REQUIRE(c && ms, "null argument");
    REQUIRE(frame_id < c->frame_seq && c->frame_seq - frame_id <= fl_ctx::kFrames, "frame id no longer tracked");
    const uint32_t k = frame_id % fl_ctx::kFrames;
    HIPCHK(hipEventSynchronize(c->ev_end_[k]));
    HIPCHK(hipEventElapsedTime(ms, c->ev_begin_[k], c->ev_end_[k]));
    return FL_OK;
}

int fl_frame_query(fl_ctx *c, uint32_t frame_id)
{
    REQUIRE(c, "null ctx");
    REQUIRE(frame_id < c->frame_seq && c->frame_seq - frame_id <= fl_ctx::kFrames, "frame id no longer tracked");
    hipError_t e = hipEventQuery(c->ev_end_[frame_id % fl_ctx::kFrames]);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
    return fail(FL_E_HIP, "hipEventQuery", __FILE__, __LINE__, e);
}

void *fl_host_alloc(size_t nbytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, nbytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

void fl_host_free(void *p) { if (p) hipHostFree(p); }

static float sum_ms(std::vector<EvPair> &v)
{
    float t = 0.0f;
    for (auto &p : v) { float ms = 0.0f; if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) t += ms; }
    return t;
}

int fl_timings_reset(fl_ctx *c)
{
    REQUIRE(c, "null ctx");
    sync_all(c);
    c->iter_ev.clear(); c->accum_ev.clear(); c->flush_ev.clear(); c->filt_ev.clear(); c->de_ev.clear(); c->enc_ev.clear(); c->pool_used = 0;
    c->n_spec_launch = c->n_interp_launch = 0;
    return FL_OK;
}

int fl_timings_detail(fl_ctx *c, float ms[6])
{
    REQUIRE(c && ms, "null argument");
    sync_all(c);
    ms[0] = sum_ms(c->iter_ev); ms[1] = sum_ms(c->accum_ev); ms[2] = sum_ms(c->flush_ev);
    ms[3] = sum_ms(c->filt_ev); ms[4] = sum_ms(c->de_ev); ms[5] = sum_ms(c->enc_ev);      // [4]: the DE's eight launches (fused ends included), recorded where they are queued; [5]: the JPEG, PNG and TIFF encodes
    return FL_OK;
}

int fl_launch_stats(fl_ctx *c, uint32_t out[4])
{
    REQUIRE(c && out, "null argument");
    out[0] = c->n_spec_launch; out[1] = c->n_interp_launch; out[2] = c->nslots; out[3] = (uint32_t)c->nw;
    return FL_OK;
}

int fl_measure_copy(int device, size_t nbytes, int iters, float *ms)
{
    REQUIRE(ms && iters > 0 && nbytes >= 16, "bad argument");
    HIPCHK(hipSetDevice(device));
    if (launch_measure_copy(nbytes, iters, ms)) return fail(FL_E_HIP, "copy measurement (allocation of 2 x nbytes, or the launch)", __FILE__, __LINE__);
    return FL_OK;
}

int fl_timings(fl_ctx *c, float *iter_ms, float *flush_ms, float *filter_ms, uint32_t *nlaunch)
{
    REQUIRE(c, "null ctx");
    sync_all(c);
    if (iter_ms) *iter_ms = sum_ms(c->iter_ev);
    if (flush_ms) *flush_ms = sum_ms(c->accum_ev) + sum_ms(c->flush_ev);
    if (filter_ms) *filter_ms = sum_ms(c->filt_ev);
    if (nlaunch) *nlaunch = (uint32_t)c->iter_ev.size();
    return FL_OK;
}

// A buffer of the debug taps: runs what the filter chain deferred, then names the buffer and its size in bytes.
static int buf_ptr(fl_ctx *c, int which, void **p, size_t *cap)
{
    Lane &ln = c->lane();
    if (int rc = flush_pending(c, ln)) return rc;
    const auto is = [&](auto &b) { *p = b.p; *cap = b.bytes(); };
    switch (which) {
    case FL_BUF_FRONT: is(ln.d_front); break;
    case FL_BUF_BACK: is(ln.d_back); break;
    case FL_BUF_SIDE: is(ln.d_side); break;
    case FL_BUF_PARAMS: is(ln.d_params); break;
    case FL_BUF_PALETTE: is(ln.d_palette); break;
    case FL_BUF_POINTS: is(c->d_points); break;
    case FL_BUF_SEEDS: is(c->d_rng); break;
    case FL_BUF_ATOM: is(ln.d_atom); break;
    case FL_BUF_HOT: is(ln.d_hot); break;
    case FL_BUF_LOG: is(ln.d_log[0]); break;
    case FL_BUF_DIR: is(ln.d_dir[0]); break;
    default: return fail(FL_E_INVAL, "unknown buffer", __FILE__, __LINE__);
    }
    if (!*p) return fail(FL_E_INVAL, "buffer not allocated yet", __FILE__, __LINE__);
    return FL_OK;
}

int fl_buffer_ptr_async(fl_ctx *c, fl_genome *g, int which, void **dev_ptr, size_t *nbytes)
{
    REQUIRE(c && dev_ptr && nbytes, "null argument");
    HIPCHK(hipSetDevice(c->device));
    return buf_ptr(c, which, dev_ptr, nbytes);
}

int fl_buffer_ptr(fl_ctx *c, fl_genome *g, int which, void **dev_ptr, size_t *nbytes)
{
    const int rc = fl_buffer_ptr_async(c, g, which, dev_ptr, nbytes);
    if (rc == FL_OK) sync_all(c);
    return rc;
}

// the host copies of the debug taps: everything queued has run before the bytes move
static int host_copy(fl_ctx *c, int which, void *host, size_t nbytes, bool to_device)
{
    REQUIRE(c && host, "null argument");
    HIPCHK(hipSetDevice(c->device));
    void *p; size_t cap;
    int rc = buf_ptr(c, which, &p, &cap);
    if (rc) return rc;
    REQUIRE(nbytes <= cap, to_device ? "write larger than buffer" : "read larger than buffer");
    sync_all(c);
    if (to_device) HIPCHK(hipMemcpy(p, host, nbytes, hipMemcpyHostToDevice));
    else HIPCHK(hipMemcpy(host, p, nbytes, hipMemcpyDeviceToHost));
    return FL_OK;
}

int fl_read_buffer(fl_ctx *c, fl_genome *g, int which, void *dst, size_t nbytes) { return host_copy(c, which, dst, nbytes, false); }

int fl_reserve(fl_ctx *c, uint32_t w, uint32_t h)
{
    REQUIRE(c && w && h, "bad argument");
    HIPCHK(hipSetDevice(c->device));
    fl_dim d;
    return ensure_fb(c->lane(), w, h, &d);
}

int fl_stream_dependency(fl_ctx *c, void *stream, int ctx_waits)
{
    REQUIRE(c, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    hipStream_t other = (hipStream_t)stream;
    // a small ring of events: an event may be re-recorded once the wait that used it has been queued
    hipEvent_t &ev = c->dep_ev[c->dep_next++ % fl_ctx::kDepEvents];
    if (!ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    if (ctx_waits) {
        HIPCHK(hipEventRecord(ev, other));
        HIPCHK(hipStreamWaitEvent(ln.stream, ev, 0));
    } else {
        if (int rc = flush_pending(c, ln)) return rc;        // deferred filter steps belong to "everything queued so far"
        HIPCHK(hipEventRecord(ev, ln.stream));
        HIPCHK(hipStreamWaitEvent(other, ev, 0));
    }
    return FL_OK;
}

int fl_write_buffer(fl_ctx *c, fl_genome *g, int which, const void *src, size_t nbytes)
{
    const int rc = host_copy(c, which, const_cast<void *>(src), nbytes, true);
    if (rc == FL_OK && which == FL_BUF_PARAMS) c->lane().params_serial = 0;       // whatever was written, the next fl_interp starts from zeroed blocks
    return rc;
}

int fl_debug_clear(fl_ctx *c, uint32_t w, uint32_t h, int reset_points)
{
    REQUIRE(c, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    fl_dim d;
    int rc = ensure_fb(ln, w, h, &d);
    if (rc) return rc;
    if ((rc = flush_pending(c, ln))) return rc;
    return do_clear(c, ln, d, reset_points != 0);
}

int fl_debug_iter_launch(fl_ctx *c, fl_genome *g, uint32_t w, uint32_t h, uint32_t round0,
                         uint32_t nrounds, uint32_t fuse, int accum_mode)
{
    REQUIRE(c && g && (accum_mode == FL_ACCUM_ATOMIC || accum_mode == FL_ACCUM_BINNED), "bad argument");
    Lane &ln = c->lane();
    REQUIRE(ln.d_params.cap >= (size_t)c->ntemporal() * g->pstride, "fl_interp has not run for this genome");
    HIPCHK(hipSetDevice(c->device));
    fl_dim d;
    int rc = ensure_fb(ln, w, h, &d);
    if (rc) return rc;
    c->round_counter = round0;
    HIPCHK(hipMemsetAsync(c->d_counters, 0, 32, ln.stream));
    return do_iter_launch(c, ln, g, d, nrounds, fuse, true, accum_mode);
}

int fl_debug_flush(fl_ctx *c, uint32_t w, uint32_t h)
{
    REQUIRE(c, "null ctx");
    Lane &ln = c->lane();
    fl_dim d;
    int rc = ensure_fb(ln, w, h, &d);
    if (rc) return rc;
    if ((rc = flush_pending(c, ln))) return rc;
    return do_flush(c, ln, d);
}

int fl_debug_accum_check(uint32_t w, uint32_t h, const uint32_t *log, size_t log_words, const uint32_t *dir, size_t dir_words,
                          uint32_t nbatch_total, uint32_t batch_records, uint32_t nslots, uint32_t nparts, int wide)
{
    fl_dim d;
    BinLayout b;
    const char *why = accum_log_check(w, h, log, log_words, dir, dir_words, nbatch_total, batch_records, nslots, nparts, wide, &d, &b);
    return why ? fail(FL_E_INVAL, why, __FILE__, __LINE__) : (int)FL_OK;
}

int fl_debug_accum(fl_ctx *c, uint32_t w, uint32_t h, const uint32_t *log, size_t log_words, const uint32_t *dir, size_t dir_words,
                   uint32_t nbatch_total, uint32_t batch_records, uint32_t nslots, uint32_t nparts, int wide)
{
    REQUIRE(c, "null ctx");
    // nothing reaches the device unless the kernels are written for it (launch_plan.h)
    fl_dim d;
    BinLayout bl;
    if (const char *why = accum_log_check(w, h, log, log_words, dir, dir_words, nbatch_total, batch_records, nslots, nparts, wide, &d, &bl))
        return fail(FL_E_INVAL, why, __FILE__, __LINE__);
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    int rc = ensure_fb(ln, w, h, &d);
    if (rc) return rc;
    if ((rc = flush_pending(c, ln))) return rc;
    const auto quiesce = [&ln] { return ln.quiesce(true); };
    if ((rc = ln.d_log[0].reserve(log_words, "sample log", quiesce))) return rc;
    if ((rc = ln.d_dir[0].reserve(dir_words, "sample log directory", quiesce))) return rc;
    if ((rc = quiesce())) return rc;                        // whatever still reads set 0
    HIPCHK(hipMemcpy(ln.d_log[0], log, 4 * log_words, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ln.d_dir[0], dir, 4 * dir_words, hipMemcpyHostToDevice));
    // do_iter_launch's call: the lane's palette, packed cells and front buffer; no clear in front of it, no flush behind it
    launch_accum_tiles(ln.stream, ln.d_log[0], ln.d_dir[0], ln.d_palette, ln.d_atom, (float *)ln.d_front.p, bl.tiles_x, bl.nbins,
                       nparts, nbatch_total, batch_records, nslots, d.astride, d.ah, bl.wide);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_debug_clear_hot(fl_ctx *c, uint32_t w, uint32_t h)
{
    REQUIRE(c && c->lane().d_hot, "null ctx");
    const fl_dim d = calc_dim(w, h);
    HIPCHK(hipMemsetAsync(c->lane().d_hot, 0, 4 * ((size_t)d.ah * d.astride / 16), c->lane().stream));
    return FL_OK;
}

int fl_debug_shuffle(fl_ctx *c, uint32_t round, uint32_t *out256)
{
    REQUIRE(c && out256, "null argument");
    HIPCHK(hipSetDevice(c->device));
    DevBuf<uint32_t> d; const size_t n = (size_t)c->nw * 64;
    if (int rc = d.reserve(n, "shuffle tap scratch")) return rc;
    launch_shuffle_tap(c->lane().stream, c->nw, d, round);
    HIPCHK(hipStreamSynchronize(c->lane().stream));
    HIPCHK(hipMemcpy(out256, d, 4 * n, hipMemcpyDeviceToHost));
    return FL_OK;
}

int fl_debug_apply_xf(fl_ctx *c, fl_genome *g, uint32_t ts, int xfi, uint32_t n, float *xyzw, fl_mwc *rng)
{
    REQUIRE(c && g && xyzw && rng && n > 0 && ts < c->ntemporal(), "bad argument");
    REQUIRE(xfi >= 0 && xfi < g->prog[1] + g->prog[2], "xform index out of range");
    Lane &ln = c->lane();
    REQUIRE(ln.d_params.cap >= (size_t)c->ntemporal() * g->pstride, "fl_interp has not run for this genome");
    HIPCHK(hipSetDevice(c->device));
    DevBuf<float4> dp; DevBuf<fl_mwc> dr;
    int rc;
    if ((rc = dp.reserve(n, "xform tap scratch")) || (rc = dr.reserve(n, "xform tap scratch"))) return rc;
    HIPCHK(hipMemcpy(dp, xyzw, dp.bytes(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dr, rng, dr.bytes(), hipMemcpyHostToDevice));
    launch_apply_xf_tap(ln.stream, g->d_prog, ln.d_params, ts, xfi, n, dp, dr);
    HIPCHK(hipStreamSynchronize(ln.stream));
    HIPCHK(hipMemcpy(xyzw, dp, dp.bytes(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(rng, dr, dr.bytes(), hipMemcpyDeviceToHost));
    return FL_OK;
}

int fl_debug_math(fl_ctx *c, int fn, uint32_t n, const float *a, const float *b, uint32_t *out_bits)
{
    REQUIRE(c && a && b && out_bits, "null argument");
    REQUIRE(n > 0, "no elements");
    REQUIRE(fn >= 0 && fn < FL_MATH_COUNT, "unknown math helper");
    Lane &ln = c->lane();
    HIPCHK(hipSetDevice(c->device));
    DevBuf<float> da, db; DevBuf<uint32_t> dout;
    int rc;
    if ((rc = da.reserve(n, "math tap scratch")) || (rc = db.reserve(n, "math tap scratch")) || (rc = dout.reserve(n, "math tap scratch"))) return rc;
    HIPCHK(hipMemcpy(da, a, da.bytes(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db, b, db.bytes(), hipMemcpyHostToDevice));
    launch_math_tap(ln.stream, fn, n, da, db, dout);
    HIPCHK(hipStreamSynchronize(ln.stream));
    HIPCHK(hipMemcpy(out_bits, dout, dout.bytes(), hipMemcpyDeviceToHost));
    return FL_OK;
}

int fl_debug_place(fl_ctx *c, const uint32_t *lens, uint32_t n, uint64_t front, uint64_t *offs_out, uint64_t *total_out)
{
    REQUIRE(c && lens && offs_out && total_out, "null argument");
    REQUIRE(n > 0, "no elements");
    Lane &ln = c->lane();
    HIPCHK(hipSetDevice(c->device));
    DevBuf<uint32_t> dl; DevBuf<u64> doffs;                     // (the total lies behind the n offsets)
    int rc;
    if ((rc = dl.reserve(n, "placement tap scratch")) || (rc = doffs.reserve((size_t)n + 1u, "placement tap scratch"))) return rc;
    HIPCHK(hipMemcpy(dl, lens, dl.bytes(), hipMemcpyHostToDevice));
    launch_debug_place(ln.stream, dl, n, front, doffs, doffs.p + n);
    HIPCHK(hipStreamSynchronize(ln.stream));
    HIPCHK(hipMemcpy(offs_out, doffs, 8 * (size_t)n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(total_out, doffs.p + n, 8, hipMemcpyDeviceToHost));
    return FL_OK;
}

int fl_debug_de_dir(fl_ctx *c, uint32_t w, uint32_t h, int pattern, const float *scalars, int in_mode, int order)
{
    REQUIRE(c && scalars, "null argument");
    REQUIRE(pattern >= 0 && pattern <= 7, "de direction must be 0..7");
    REQUIRE(order >= -1 && order <= 2, "tile order must be -1 (the table's) or 0..2");
    REQUIRE(pattern != 0 || in_mode == 1 || in_mode == 2, "direction 0 reads the raw accumulator: in_mode 1, or 2 (YUV)");
    REQUIRE(w && h, "empty frame");
    HIPCHK(hipSetDevice(c->device));
    Lane &ln = c->lane();
    fl_dim d;
    int rc = ensure_fb(ln, w, h, &d);
    if (rc) return rc;
    if ((rc = flush_pending(c, ln))) return rc;
    float k7[7];
    gauss7(1.0f, k7);                                       // fl_filter's (FL_FILT_BILATERAL)
    // a pixel the kernel does not write stays NaN (all bits set)
    HIPCHK(hipMemsetAsync(ln.d_back, 0xff, 16 * (size_t)d.ah * d.astride, ln.stream));
    const DeTail none = {};                                 // direction 7: un-normalise, no tone filter riding along
    launch_de_dir(ln.stream, d, pattern, ln.d_back, ln.d_front, k7, scalars[0], scalars[1], scalars[2], scalars[3], scalars[4],
                  in_mode, pattern == 7 ? &none : nullptr, order);
    swap(ln.d_front, ln.d_back);
    HIPCHK(hipGetLastError());
    return FL_OK;
}

int fl_rtc_compile_check(const int32_t *prog, uint32_t nprog, const int32_t *ops, uint32_t nops, int nw, int count, int acc,
                         char *log, size_t log_bytes)
{
    REQUIRE(prog && ops && nprog >= FL_PROG_HDR && (nw == 4 || nw == 8 || nw == 16) && acc >= 0 && acc <= 3, "bad argument");
    int rc = check_prog(prog, nprog);
    if (rc) return rc;
    for (uint32_t i = 0; i < nops; ++i) if ((rc = check_structure_op(prog, ops + 4 * i))) return rc;
    IterSpec spec = iter_spec(prog, nprog, ops, nops);
    for (std::vector<int> &v : spec.vids) for (int &id : v) if (id < 0) id = 0;      // (a variation without a number compiles as number 0 here; fl_genome_create refuses it)
    std::vector<char> code;
    std::string err;
    rc = rtc_compile(spec, nw, (count & 1) != 0, acc, &code, &err, nullptr, (count & 2) == 0 ? 0u : nw == 8 ? 1u : nw == 16 ? 2u : 0u);
    if (log && log_bytes) { snprintf(log, log_bytes, "%s", rc ? err.c_str() : "ok"); }
    if (rc) return fail(rtc_available() ? FL_E_HIP : FL_E_UNSUPPORTED, "per-genome kernel did not compile", __FILE__, __LINE__);
    return (int)(code.size() > 0 ? FL_OK : FL_E_HIP);
}

int fl_genome_prepare(fl_ctx *c, fl_genome *g, uint32_t w, uint32_t h, int accum_mode)
{
    REQUIRE(c && g, "null argument");
    REQUIRE(accum_mode == FL_ACCUM_ATOMIC || accum_mode == FL_ACCUM_BINNED || accum_mode == 2, "bad accumulation mode");
    HIPCHK(hipSetDevice(c->device));
    // the one variant fl_iterate launches for this size and mode (do_iter_launch): no counters; a binned frame of more tiles than
    // the 128x64 layout holds takes the wide kernel
    const int kacc = accum_mode == FL_ACCUM_BINNED && c->layout(calc_dim(w, h)).wide ? 3 : accum_mode;
    bool pending = false;
    (void)rtc_variant(c, g, false, kacc, c->rtc_async ? RTC_POLL : RTC_SYNC, &pending);
    return FL_OK;
}

int fl_rtc_wait(fl_ctx *c, fl_genome *g)
{
    REQUIRE(c && g, "null argument");
    HIPCHK(hipSetDevice(c->device));
    const int geom = c->sub_log2 ? 2 + (int)c->sub_log2 : c->nw == 16 ? 2 : c->nw == 8 ? 1 : 0;
    for (int count = 0; count < 2; ++count)
        for (int kacc = 0; kacc < 4; ++kacc) {
            if (!g->rtc_want[geom][count][kacc]) continue;
            REQUIRE(!rtc_held(), "the worker is held (fl_debug_rtc_hold): its jobs cannot finish");
            bool pending = false;
            (void)rtc_variant(c, g, count != 0, kacc, RTC_WAIT, &pending);
        }
    return FL_OK;
}

int fl_rtc_stats(uint64_t out[8])
{
    REQUIRE(out, "null argument");
    rtc_stats(out);
    return FL_OK;
}

int fl_debug_rtc_hold(int on) { rtc_hold(on != 0); return FL_OK; }

int fl_debug_counters(fl_ctx *c, uint64_t out4[4])
{
    REQUIRE(c && out4, "null argument");
    sync_all(c);
    HIPCHK(hipMemcpy(out4, c->d_counters, 32, hipMemcpyDeviceToHost));
    return FL_OK;
}

} // extern "C"
#pragma GCC visibility pop
