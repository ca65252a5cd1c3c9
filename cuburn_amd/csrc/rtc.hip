// rtc.hip — per-genome specialisation of the iterate kernel with hipRTC.
//
// The reference generates and compiles CUDA source for every genome (cuburn/render.py:232-236,
// cuburn/code/iter.py:559-575, Tempita + nvcc through PyCUDA, up to 20 modules cached,
// render.py:229-245).  Here one precompiled kernel interprets any genome; on top of it the STRUCTURE
// of a genome (xform count, variation numbers per xform, post affines, final xform, record strides)
// can be compiled into the same kernel source at run time: iter.hip is rebuilt by hipRTC with the
// structure as constexpr tables ("flame_spec.h", generated below), which removes the variation
// dispatch, the variation loop and the post / final tests from the round loop.  All VALUES (affine
// coefficients, weights, variation parameters) stay data in the parameter block, so an animation
// whose structure does not change compiles once.  Code objects are cached per process by
// (device, structure, walker geometry, accumulate mode).  libhiprtc is loaded with dlopen: without it
// (or with FLAME_RTC=0) the interpreter kernel runs — same results, bit for bit.
//
// Two opt-in switches.  FLAME_RTC_CACHE=<dir> keeps every code object in a file (rtc_cache.h), looked up before
// each compile: a warm cache walks the same budget chain and ends on the same kernel with no compiler run.  FLAME_RTC_ASYNC=1
// (read by fl_ctx_create) hands the compiles to one worker thread; until a variant's kernel is there its launches run the
// interpreter kernel.  The worker calls hipRTC and the cache's file I/O only — every hip* runtime call (module load, function
// lookup, register check) stays on the thread that asked.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "kernels.h"
#include "rtc_cache.h"
#include "flame_device.h"      // the compile-time switches the run-time build must share with this library (FL_LOG_PACK3)
#define FL_STR2(x) #x
#define FL_STR(x) FL_STR2(x)
#include "rtc_sources.inc"

namespace {

struct Api {
    bool ok = false;
    hiprtcResult (*create)(hiprtcProgram *, const char *, const char *, int, const char **, const char **) = nullptr;
    hiprtcResult (*compile)(hiprtcProgram, int, const char **) = nullptr;
    hiprtcResult (*log_size)(hiprtcProgram, size_t *) = nullptr;
    hiprtcResult (*log)(hiprtcProgram, char *) = nullptr;
    hiprtcResult (*code_size)(hiprtcProgram, size_t *) = nullptr;
    hiprtcResult (*code)(hiprtcProgram, char *) = nullptr;
    hiprtcResult (*destroy)(hiprtcProgram *) = nullptr;
    hiprtcResult (*version)(int *, int *) = nullptr;      // (optional: the cache key falls back to the HIP runtime's version)
};

Api load_api()
{
    Api a;
    void *h = nullptr;
    for (const char *name : {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"}) {
        h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
    }
    if (!h) return a;
#define SYM(field, sym) a.field = reinterpret_cast<decltype(a.field)>(dlsym(h, sym)); if (!a.field) return a
    SYM(create, "hiprtcCreateProgram"); SYM(compile, "hiprtcCompileProgram");
    SYM(log_size, "hiprtcGetProgramLogSize"); SYM(log, "hiprtcGetProgramLog");
    SYM(code_size, "hiprtcGetCodeSize"); SYM(code, "hiprtcGetCode"); SYM(destroy, "hiprtcDestroyProgram");
#undef SYM
    a.version = reinterpret_cast<decltype(a.version)>(dlsym(h, "hiprtcVersion"));
    a.ok = true;
    return a;
}

const Api &api() { static Api a = load_api(); return a; }

struct Entry { hipModule_t mod = nullptr; hipFunction_t fn = nullptr; };
std::mutex g_mu;
std::map<std::string, Entry> g_cache;           // key: device + generated header
unsigned g_epoch = 1;                           // bumped whenever modules are unloaded: handles held by callers expire
const size_t kMaxModules = 64;                  // (the reference keeps 20, render.py:229)

std::string spec_header(const IterSpec &s, int nw, bool count, int acc, uint32_t sub_log2)
{
    const int nrec = s.nxf + s.has_final;
    int maxv = 1;
    for (int i = 0; i < nrec; ++i) maxv = std::max(maxv, s.nvar[i]);
    std::string h = "// generated: structure of one genome (rtc.hip)\n";
    char buf[256];
#define DEF(name, val) snprintf(buf, sizeof buf, "#define %s %d\n", name, (int)(val)); h += buf
    DEF("FL_SPEC_NXF", s.nxf); DEF("FL_SPEC_FINAL", s.has_final); DEF("FL_SPEC_PSTRIDE", s.pstride);
    DEF("FL_SPEC_CDF_OFF", s.cdf_off); DEF("FL_SPEC_XF_OFF", s.xf_off); DEF("FL_SPEC_XF_STRIDE", s.xf_stride);
    DEF("FL_SPEC_VAR_STRIDE", s.var_stride); DEF("FL_SPEC_NW", nw); DEF("FL_SPEC_COUNT", count ? 1 : 0); DEF("FL_SPEC_ACC", acc);
    DEF("FL_SPEC_SUB_LOG2", sub_log2 != 0u && (4 << sub_log2) == nw ? (int)sub_log2 : 0);
    DEF("FL_SPEC_CHAOS", s.chaos ? 1 : 0); DEF("FL_SPEC_CHAOS_OFF", s.chaos ? s.chaos_off : 0);      // xaos: the divergent form of the walk (iter.hip CHAOS)
#undef DEF
    h += "constexpr int kSpecNvar[] = {";
    for (int i = 0; i < nrec; ++i) h += std::to_string(s.nvar[i]) + ",";
    h += "0};\nconstexpr int kSpecPost[] = {";
    for (int i = 0; i < nrec; ++i) h += std::to_string(s.post[i]) + ",";
    h += "0};\nconstexpr int kSpecOpac[] = {";
    for (int i = 0; i < nrec; ++i) h += std::to_string(i < (int)s.opac.size() ? s.opac[i] : 0) + ",";
    snprintf(buf, sizeof buf, "0};\nconstexpr int kSpecVid[][%d] = {", maxv);
    h += buf;
    for (int i = 0; i < nrec; ++i) {
        h += "{";
        for (int j = 0; j < maxv; ++j) h += std::to_string(j < s.nvar[i] ? s.vids[i][j] : 0) + ",";
        h += "},";
    }
    h += "{0}};\n";
    return h;
}

// process-wide counters (fl_rtc_stats, include/flame_hip.h): compiler runs; disk hits, misses, writes, rejects; jobs queued;
// iterate launches on the interpreter while a job was pending; iterate launches on a per-genome kernel
std::atomic<uint64_t> g_stats[8];
enum { ST_COMPILES, ST_HITS, ST_MISSES, ST_WRITES, ST_REJECTS, ST_QUEUED, ST_PENDING_LAUNCHES, ST_SPEC_LAUNCHES };

// One compile.  A job owns copies of everything it reads (the structure, the options, the architecture, the directories), so that
// the worker thread never follows a pointer into a genome or a context and never asks the HIP runtime or the environment anything.
struct Job {
    IterSpec spec;
    int nw = 4, acc = 0;
    bool count = false;
    uint32_t sub_log2 = 0;
    std::string header;                    // flame_spec.h, generated from the five fields above
    std::vector<std::string> opts;         // the complete option list, in order
    std::string arch;                      // the device's full architecture string (target features included): part of the cache key
    int64_t version = 0;                   // hipRTC's version: part of the cache key
    std::string cache_dir, dump_dir;       // FLAME_RTC_CACHE (empty: no cache, or the directory cannot be used), FLAME_RTC_DUMP
    // results
    std::vector<char> code;
    std::string err;
    int rc = 0;
    bool done = false;                     // (asynchronous jobs: guarded by the worker's mutex)
};

// hipRTC's version, or the HIP runtime's where libhiprtc does not export hiprtcVersion; asked once, on a calling thread
int64_t rtc_version()
{
    static const int64_t v = [] {
        int major = 0, minor = 0, rt = 0;
        if (api().version && api().version(&major, &minor) == HIPRTC_SUCCESS) return (int64_t)major * 1000000 + minor;
        if (hipRuntimeGetVersion(&rt) != hipSuccess) { (void)hipGetLastError(); rt = 0; }
        return -(int64_t)rt - 1;
    }();
    return v;
}

// FLAME_RTC_CACHE, if it names a directory that can hold the cache (made if missing); one warning per process if not
std::string cache_dir()
{
    const char *e = getenv("FLAME_RTC_CACHE");
    if (!e || !*e) return "";
    static std::mutex mu;
    static std::map<std::string, bool> seen;
    static bool warned = false;
    std::lock_guard<std::mutex> lock(mu);
    auto it = seen.find(e);
    if (it == seen.end()) {
        std::string why;
        const bool ok = rtc_cache::prepare_dir(e, &why);
        if (!ok && !warned) {
            warned = true;
            fprintf(stderr, "libflame_hip: FLAME_RTC_CACHE=%s cannot be used (%s); running without the kernel cache\n", e, why.c_str());
        }
        it = seen.emplace(e, ok).first;
    }
    return it->second ? std::string(e) : std::string();
}

std::shared_ptr<Job> make_job(const IterSpec &spec, int nw, bool count, int acc, const char *extra_opt, uint32_t sub_log2)
{
    std::shared_ptr<Job> j = std::make_shared<Job>();
    j->spec = spec; j->nw = nw; j->count = count; j->acc = acc; j->sub_log2 = sub_log2;
    j->header = spec_header(j->spec, nw, count, acc, sub_log2);
    if (!api().ok) return j;
    // same code generation options as the ahead-of-time build of iter.hip (csrc/Makefile); the target is the
    // current device's own architecture string (fl_ctx_create has refused anything that is not gfx950)
    std::string arch_opt = "--offload-arch=gfx950";
    j->arch = "gfx950";
    {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.gcnArchName[0]) {
            std::string name(prop.gcnArchName);
            arch_opt = "--offload-arch=" + name.substr(0, name.find(':'));
            j->arch = name;
        } else (void)hipGetLastError();
    }
    j->opts = {arch_opt, "-O3", "-std=c++20", "-ffp-contract=off", "-DFL_RTC=1",
               "-mllvm", "-structurizecfg-skip-uniform-regions=true",
               "-DFL_LOG_PACK3=" FL_STR(FL_LOG_PACK3),
               "-fno-slp-vectorize",
    };
    if (extra_opt) j->opts.push_back(extra_opt);
    // FLAME_RTC_FLAGS="-mllvm -x=y ...": extra options, e.g. the switches of iter.hip that tests/test_gpu_switches.py sets
    if (const char *e = getenv("FLAME_RTC_FLAGS")) {
        std::string w;
        for (const char *q = e;; ++q) {
            if (*q && *q != ' ') { w += *q; continue; }
            if (!w.empty()) { j->opts.push_back(w); w.clear(); }
            if (!*q) break;
        }
    }
    j->cache_dir = cache_dir();
    if (!j->cache_dir.empty()) j->version = rtc_version();
    if (const char *dir = getenv("FLAME_RTC_DUMP")) j->dump_dir = dir;
    return j;
}

// The job's code object: from the disk cache, or from the compiler (and then into the cache).  hipRTC and file I/O only.
void run_job(Job &j)
{
    const Api &a = api();
    if (!a.ok) { j.err = "libhiprtc not found"; j.rc = -1; return; }
    rtc_cache::Digest key = {};
    bool hit = false;
    if (!j.cache_dir.empty()) {
        rtc_cache::KeyInput k;
        k.src_iter = rtc_src_iter; k.src_variations = rtc_src_variations; k.src_device = rtc_src_device; k.src_abi = rtc_src_abi;
        k.spec_header = j.header; k.options = j.opts; k.arch = j.arch; k.version = j.version;
        key = rtc_cache::key_of(k);
        const rtc_cache::Result r = rtc_cache::read(j.cache_dir, key, &j.code);
        hit = r == rtc_cache::HIT;
        g_stats[hit ? ST_HITS : r == rtc_cache::MISS ? ST_MISSES : ST_REJECTS] += 1;
    }
    if (!hit) {
        hiprtcProgram prog = nullptr;
        const char *hdr_src[] = {rtc_src_variations, rtc_src_device, rtc_src_abi, j.header.c_str()};
        const char *hdr_name[] = {"variations.h", "flame_device.h", "flame_hip.h", "flame_spec.h"};
        if (a.create(&prog, rtc_src_iter, "iter.hip", 4, hdr_src, hdr_name) != HIPRTC_SUCCESS) { j.err = "hiprtcCreateProgram failed"; j.rc = -1; return; }
        std::vector<const char *> optv;
        for (const std::string &o : j.opts) optv.push_back(o.c_str());
        g_stats[ST_COMPILES] += 1;
        const hiprtcResult rc = a.compile(prog, (int)optv.size(), optv.data());
        if (rc != HIPRTC_SUCCESS) {
            size_t n = 0;
            a.log_size(prog, &n);
            std::string log(n, '\0');
            if (n) a.log(prog, &log[0]);
            j.err = "hiprtc compile failed: " + log.substr(0, 4000);
            a.destroy(&prog);
            j.rc = -1;
            return;
        }
        size_t n = 0;
        a.code_size(prog, &n);
        j.code.resize(n);
        a.code(prog, j.code.data());
        a.destroy(&prog);
        if (!j.cache_dir.empty() && rtc_cache::write(j.cache_dir, key, j.code.data(), j.code.size())) g_stats[ST_WRITES] += 1;
    }
    // FLAME_RTC_DUMP=<dir>: keep the generated header and the code object of the last compile, for
    // llvm-objdump -d (tools/dump_spec_kernel.py)
    if (!j.dump_dir.empty()) {
        const std::string &d = j.dump_dir;
        if (FILE *f = fopen((d + "/flame_spec.h").c_str(), "w")) { fwrite(j.header.data(), 1, j.header.size(), f); fclose(f); }
        if (FILE *f = fopen((d + "/k_iter_spec.co").c_str(), "wb")) { fwrite(j.code.data(), 1, j.code.size(), f); fclose(f); }
    }
}

// FLAME_RTC_ASYNC: one thread per process runs the queued jobs, the one asked about last first.  It is started by the first job and joined when
// the process ends (this object's destructor: no thread is left running in code that is being unloaded); jobs still queued
// then are dropped.  The object is constructed after api(), so it is destroyed before it — libhiprtc itself is never closed.
struct Worker {
    std::mutex mu;
    std::condition_variable cv;                   // the worker waits for a job or a release; callers wait for a job's end
    std::deque<std::shared_ptr<Job>> q;
    bool hold = false, quit = false;
    std::thread th;

    void queue(const std::shared_ptr<Job> &j)
    {
        std::lock_guard<std::mutex> lock(mu);
        q.push_back(j);
        g_stats[ST_QUEUED] += 1;
        if (!th.joinable()) th = std::thread([this] { loop(); });
        cv.notify_all();
    }
    // Is the job done (wait: once it is)?  Whoever asks moves a job that still waits to the head of the queue: the kernel
    // the frame loop is rendering without right now is compiled next, and the jobs of genomes nobody renders any more —
    // a walk over many one-frame genomes leaves them behind — sink to the end instead of holding it up.
    bool finished(const std::shared_ptr<Job> &j, bool wait)
    {
        std::unique_lock<std::mutex> lock(mu);
        if (!j->done) {
            auto it = std::find(q.begin(), q.end(), j);
            if (it != q.end() && it != q.begin()) { q.erase(it); q.push_front(j); }
        }
        if (wait) cv.wait(lock, [&] { return j->done; });
        return j->done;
    }
    void set_hold(bool on)
    {
        std::lock_guard<std::mutex> lock(mu);
        hold = on;
        cv.notify_all();
    }
    bool held() { std::lock_guard<std::mutex> lock(mu); return hold; }
    void loop()
    {
        std::unique_lock<std::mutex> lock(mu);
        for (;;) {
            cv.wait(lock, [&] { return quit || (!hold && !q.empty()); });
            if (quit) return;
            std::shared_ptr<Job> j = q.front();
            q.pop_front();
            lock.unlock();
            run_job(*j);
            // (whatever this compile made the compiler register for destruction is destroyed before ~Worker runs: a join
            // registered now comes before it — the warm-up in worker() covers the first compile, this every later one)
            atexit(join_at_exit);
            lock.lock();
            j->done = true;
            cv.notify_all();
        }
    }
    void shutdown()
    {
        { std::lock_guard<std::mutex> lock(mu); quit = true; }
        cv.notify_all();
        std::lock_guard<std::mutex> lock(join_mu);
        if (th.joinable()) th.join();
    }
    std::mutex join_mu;
    static void join_at_exit();
    ~Worker() { shutdown(); }
};

Worker &worker()
{
    (void)api();
    // libhiprtc loads the code object manager (the compiler proper) when it first compiles.  Loaded here instead, its global
    // objects exist before the worker does and are destroyed after the worker has been joined: a process that ends in the
    // middle of a compile waits for the compile, it does not pull the compiler's state from under it.  Never closed.
    static void *const comgr = [] {
        void *h = nullptr;
        for (const char *name : {"libamd_comgr.so.3", "libamd_comgr.so", "/opt/rocm/lib/libamd_comgr.so"})
            if ((h = dlopen(name, RTLD_LAZY | RTLD_LOCAL))) break;
        return h;
    }();
    (void)comgr;
    // ... and the compiler registers more of its state for destruction while it first works (found with a host program that
    // ends 50 ms into a compile: the worker faulted inside the code object manager while the exiting thread ran those
    // destructors, before it reached ~Worker).  So the first compile of the process is an empty kernel, here, on the calling
    // thread, before the worker exists: whatever that registered is destroyed after the join.
    static const bool warm = [] {
        const Api &a = api();
        if (!a.ok) return false;
        hiprtcProgram prog = nullptr;
        if (a.create(&prog, "extern \"C\" __global__ void k_warm() {}\n", "warm.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) return false;
        const char *opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++20"};
        const bool ok = a.compile(prog, 3, opts) == HIPRTC_SUCCESS;
        a.destroy(&prog);
        return ok;
    }();
    (void)warm;
    static Worker w;
    return w;
}

void Worker::join_at_exit() { worker().shutdown(); }

// A variant's walk down the budgets, kept between the calls of the asynchronous mode (guarded by g_mu): the budget in hand, its
// job, and the full-budget module that was over the register limit.  It belongs to the process, not to the genome or the context
// that started it — either may be destroyed while the job is queued or running; the next caller of the same key takes it up.
struct Chain { int b = 0; std::shared_ptr<Job> job; Entry first; bool have_first = false; };
std::map<std::string, Chain> g_pending;

}  // namespace

bool rtc_available() { return api().ok; }

int rtc_compile(const IterSpec &spec, int nw, bool count, int acc, std::vector<char> *code, std::string *err, const char *extra_opt, uint32_t sub_log2)
{
    const std::shared_ptr<Job> j = make_job(spec, nw, count, acc, extra_opt, sub_log2);
    run_job(*j);
    if (j->rc) { *err = j->err; return -1; }
    code->swap(j->code);
    return 0;
}

unsigned rtc_epoch() { std::lock_guard<std::mutex> lock(g_mu); return g_epoch; }

void rtc_stats(uint64_t out[8]) { for (int i = 0; i < 8; ++i) out[i] = g_stats[i].load(); }
void rtc_count_launch(bool spec, bool pending) { if (spec) g_stats[ST_SPEC_LAUNCHES] += 1; else if (pending) g_stats[ST_PENDING_LAUNCHES] += 1; }
void rtc_hold(bool on) { worker().set_hold(on); }
bool rtc_held() { return worker().held(); }

int rtc_iter_kernel(int device, const IterSpec &spec, int nw, uint32_t nslots, bool count, int acc, hipFunction_t *fn, std::string *err, uint32_t sub_log2, int mode)
{
    // vector registers a four-wave kernel may use before a workgroup per CU is lost: every slot is resident at once, nslots * 4
    // waves over 1024 SIMDs of 512 registers each — 128 at the 1024 slots of frames of up to 2^28 samples (four waves per SIMD),
    // 80 at 1536 (six; the allocation granule is 8).  Other geometries are bounded by LDS, not registers: no limit.
    const uint32_t wps = (nslots * 4u + 1023u) / 1024u;
    const int reg_limit = nw == 4 && wps >= 1u && wps <= 8u ? (int)(512u / wps / 8u * 8u) : 0;
    const std::string key = std::to_string(device) + "|" + std::to_string(reg_limit) + "|" + spec_header(spec, nw, count, acc, sub_log2);
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_cache.find(key);
    if (it != g_cache.end()) { *fn = it->second.fn; return 0; }
    // The kernel keeps wave-uniform operands of the round in vector registers (FL_HOIST_BUDGET, iter.hip); where that is what takes a
    // genome's kernel past the geometry's register limit, it is compiled again with a smaller budget — a sixth of the workgroups
    // waiting for a slot costs far more than the few instructions per round the registers save.  (Round 4 compared with 80 whatever
    // the geometry: kernels of 81-128 registers were recompiled up to three times for the 1024-slot geometry, for nothing.)
    // Synchronous: each budget's job runs here.  Asynchronous: it is queued for the worker, and this walk is taken up again by the
    // next call once the job has finished (RTC_POLL returns 1 until then; RTC_WAIT waits) — the same steps in the same order, so
    // both modes, and a warm disk cache, settle on the same kernel.
    Entry e;
    const char *budgets[] = {nullptr, "-DFL_HOIST_BUDGET=7", "-DFL_HOIST_BUDGET=5", "-DFL_HOIST_BUDGET=0"};
    Chain local;
    Chain &ch = mode == RTC_SYNC ? local : g_pending[key];
    for (;;) {
        if (!ch.job) {
            ch.job = make_job(spec, nw, count, acc, budgets[ch.b], sub_log2);
            if (mode == RTC_SYNC) run_job(*ch.job); else worker().queue(ch.job);
        }
        if (mode != RTC_SYNC && !worker().finished(ch.job, mode == RTC_WAIT)) return 1;
        const std::shared_ptr<Job> j = ch.job;
        ch.job.reset();
        Entry t;
        std::string why;
        if (j->rc) why = j->err;
        else if (hipModuleLoadData(&t.mod, j->code.data()) != hipSuccess) { (void)hipGetLastError(); why = "hipModuleLoadData failed"; }
        else if (hipModuleGetFunction(&t.fn, t.mod, "k_iter_spec") != hipSuccess) {
            (void)hipGetLastError(); (void)hipModuleUnload(t.mod); why = "k_iter_spec not found in the compiled module";
        }
        if (!why.empty()) {
            *err = why;
            if (ch.have_first) break;
            if (mode != RTC_SYNC) g_pending.erase(key);
            return -1;
        }
        int regs = 0;
        if (hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, t.fn) != hipSuccess) { (void)hipGetLastError(); regs = 0; }
        if (reg_limit == 0 || regs <= reg_limit) { if (ch.have_first) (void)hipModuleUnload(ch.first.mod); ch.have_first = false; e = t; break; }
        if (!ch.have_first) { ch.first = t; ch.have_first = true; } else (void)hipModuleUnload(t.mod);
        if (++ch.b == 4) break;
    }
    if (ch.have_first) e = ch.first;    // over the limit with every budget: the registers are not the hoisted operands — keep the full budget
    err->clear();                       // (a later budget's failure text must not outlive a successful result)
    if (mode != RTC_SYNC) g_pending.erase(key);
    if (g_cache.size() >= kMaxModules) {
        // simple bound: drop THIS device's modules (the current device is `device`: its queued kernels are
        // waited for first); modules of other devices held by the process stay loaded — their kernels may
        // still be queued and this thread cannot wait for them from here
        (void)hipDeviceSynchronize();
        const std::string prefix = std::to_string(device) + "|";
        for (auto kv = g_cache.begin(); kv != g_cache.end();) {
            if (kv->first.compare(0, prefix.size(), prefix) == 0) { (void)hipModuleUnload(kv->second.mod); kv = g_cache.erase(kv); }
            else ++kv;
        }
        ++g_epoch;
    }
    g_cache[key] = e;
    *fn = e.fn;
    return 0;
}

