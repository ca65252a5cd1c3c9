// Prints what csrc/launch_plan.h computes for the cases named on the command line, one line per case
// (tests/test_cpu_launch_plan.py builds this with the host sanitizers and compares the lines with its own restatement):
//   L w h nw bin_rounds force_wide forced_parts write_rounds nslots
//       -> astride ah wide tile_w tiles_x nbins region parts nbatch log_words dir_words set_bytes
//   S rounds sub_log2 nw fixed_cap     -> cap_short cap_long cap n0 n1 ...   (the binned schedule before the free-memory test)
//   U rounds sub_log2                  -> n0 n1 ...                           (no cap: the atomic modes)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../cuburn_amd/csrc/launch_plan.h"

int main(int argc, char **argv)
{
    int i = 1;
    auto num = [&] { if (i >= argc) { fprintf(stderr, "missing argument\n"); exit(2); } return strtoull(argv[i++], nullptr, 10); };
    while (i < argc) {
        const char cmd = argv[i++][0];
        if (cmd == 'L') {
            const uint32_t w = num(), h = num(); const int nw = (int)num(); const uint32_t br = num(); const bool fw = num() != 0;
            const uint32_t forced = num(); const uint64_t wr = num(); const uint32_t nslots = num();
            const fl_dim d = calc_dim(w, h);
            const BinLayout b = bin_layout(d, nw, br, fw);
            const BinSet s = bin_set(b, wr, br, nslots);
            printf("L %u %u %d %u %u %u %zu %u %u %zu %zu %zu\n", d.astride, d.ah, (int)b.wide, b.tile_w, b.tiles_x, b.nbins, b.region,
                   accum_parts(b.nbins, b.wide, forced), s.nbatch, s.log_words, s.dir_words, s.bytes());
        } else if (cmd == 'S' || cmd == 'U') {
            const uint64_t rounds = num(); const uint32_t sub = num();
            LaunchPlan p;
            if (cmd == 'S') {
                const int nw = (int)num(); const uint32_t fixed = num();
                p = launch_schedule(rounds, sub, nw, fixed);
                printf("S %llu %llu %llu", (unsigned long long)launch_cap(false, sub, nw), (unsigned long long)launch_cap(true, sub, nw),
                       (unsigned long long)p.cap);
            } else {
                p = launch_schedule_under(rounds, sub, FL_NO_CAP);
                printf("U");
            }
            for (uint32_t n : p.rounds) printf(" %u", n);
            printf("\n");
        } else { fprintf(stderr, "unknown case %c\n", cmd); return 2; }
    }
    return 0;
}
