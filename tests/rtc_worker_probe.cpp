// rtc_worker_probe.cpp — the compile thread of csrc/rtc.hip on its own, without a device: a host program built around rtc.hip
// itself (tests/test_cpu_rtc_worker.py builds it with hipcc and runs one named check per process).
//
//   rtc_worker_probe <check> <flame_spec.h>
//
//   exit_mid_compile   queue three compiles, return from main as soon as the compiler has been entered: the process must
//                      wait for the compile in flight and end with status 0 (it died of SIGSEGV inside the code object
//                      manager before the worker's join was ordered behind the compiler's own exit-time destructors)
//   held               while held, queued jobs are left alone; ending the process drops them
//   order              the job asked about last runs first
#include "rtc.hip"
#include <fstream>
#include <sstream>

static std::string g_header;

static std::shared_ptr<Job> job(const char *extra)
{
    std::shared_ptr<Job> j = std::make_shared<Job>();
    j->header = g_header;
    j->arch = "gfx950";
    j->opts = {"--offload-arch=gfx950", "-O3", "-std=c++20", "-ffp-contract=off", "-DFL_RTC=1", "-mllvm", "-structurizecfg-skip-uniform-regions=true",
               "-DFL_LOG_PACK3=" FL_STR(FL_LOG_PACK3), "-fno-slp-vectorize", extra};
    return j;
}

static uint64_t stat(int i) { uint64_t st[8]; rtc_stats(st); return st[i]; }

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: rtc_worker_probe <check> <flame_spec.h>\n"); return 2; }
    const std::string check = argv[1];
    std::ifstream f(argv[2]);
    std::stringstream ss;
    ss << f.rdbuf();
    g_header = ss.str();
    if (g_header.empty() || !rtc_available()) { printf("SKIP no header or no libhiprtc\n"); return 0; }
    if (check == "exit_mid_compile") {
        for (const char *b : {"-DFL_HOIST_BUDGET=12", "-DFL_HOIST_BUDGET=7", "-DFL_HOIST_BUDGET=5"}) worker().queue(job(b));
        while (stat(ST_COMPILES) == 0) std::this_thread::yield();
        printf("leaving main with %llu of 3 compiles entered\n", (unsigned long long)stat(ST_COMPILES));
        fflush(stdout);
        return 0;
    }
    if (check == "held") {
        rtc_hold(true);
        std::shared_ptr<Job> a = job("-DFL_HOIST_BUDGET=12"), b = job("-DFL_HOIST_BUDGET=7");
        worker().queue(a); worker().queue(b);
        for (int i = 0; i < 1000; ++i) std::this_thread::yield();
        const bool ok = !worker().finished(a, false) && !worker().finished(b, false) && stat(ST_COMPILES) == 0 && stat(ST_QUEUED) == 2 && rtc_held();
        printf("%s held: compiles %llu queued %llu\n", ok ? "ok" : "FAIL", (unsigned long long)stat(ST_COMPILES), (unsigned long long)stat(ST_QUEUED));
        return ok ? 0 : 1;                          // (still held: the two jobs are dropped)
    }
    if (check == "order") {
        rtc_hold(true);
        std::shared_ptr<Job> a = job("-DFL_HOIST_BUDGET=12"), b = job("-DFL_HOIST_BUDGET=7"), c = job("-DFL_HOIST_BUDGET=5");
        worker().queue(a); worker().queue(b); worker().queue(c);
        (void)worker().finished(b, false);          // asked about b: b, a, c
        rtc_hold(false);
        bool ok = worker().finished(b, true) && !worker().finished(c, false);
        const bool a_after_b = !a->done;            // (the single worker has just finished b: a cannot be done unless it ran first)
        ok = ok && a_after_b && worker().finished(a, true) && !worker().finished(c, false) && worker().finished(c, true);
        ok = ok && a->rc == 0 && b->rc == 0 && c->rc == 0 && !a->code.empty() && a->code != b->code && stat(ST_COMPILES) == 3;
        printf("%s order: a after b %d, rc %d %d %d, %zu bytes\n", ok ? "ok" : "FAIL", (int)a_after_b, a->rc, b->rc, c->rc, a->code.size());
        return ok ? 0 : 1;
    }
    fprintf(stderr, "unknown check %s\n", check.c_str());
    return 2;
}
