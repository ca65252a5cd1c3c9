// rtc_cache_probe.cpp — csrc/rtc_cache.h on its own: a host program (built with -fsanitize=address,undefined by
// tests/test_cpu_rtc_cache.py) that runs one named check in a scratch directory and exits 0 if it holds.
//
//   rtc_cache_probe <check> <dir>
//
// Every check prints what it saw; a line that starts with FAIL makes the exit status 1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iterator>
#include <map>
#include <string>
#include <vector>
#include "rtc_cache.h"

using namespace rtc_cache;

static int g_fail = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++g_fail; printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static KeyInput fixed_input()
{
    KeyInput k;
    k.src_iter = "__global__ void k_iter_spec() {}\n";
    k.src_variations = "// variations\n";
    k.src_device = "// device\n";
    k.src_abi = "// abi\n";
    k.spec_header = "#define FL_SPEC_NXF 3\n";
    k.options = {"--offload-arch=gfx950", "-O3", "-DFL_LOG_PACK3=1", "-DFL_HOIST_BUDGET=7"};
    k.arch = "gfx950:sramecc+:xnack-";
    k.version = 7000001;
    return k;
}

static std::vector<char> payload_of(size_t n, unsigned seed)
{
    std::vector<char> v(n);
    unsigned s = seed * 2654435761u + 1u;
    for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; v[i] = (char)(s >> 24); }
    return v;
}

static std::vector<char> slurp(const std::string &p)
{
    std::ifstream f(p, std::ios::binary);
    return std::vector<char>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static void spit(const std::string &p, const std::vector<char> &v, size_t n)
{
    std::ofstream f(p, std::ios::binary | std::ios::trunc);
    f.write(v.data(), (std::streamsize)n);
}

static void check_roundtrip(const std::string &dir)
{
    const size_t sizes[] = {0, 1, 15, 16, 17, 4096, 100003};
    unsigned seed = 1;
    for (size_t n : sizes) {
        KeyInput k = fixed_input();
        k.version += (int64_t)n;
        const Digest key = key_of(k);
        const std::vector<char> p = payload_of(n, seed++);
        std::vector<char> got(3, 'x');
        EXPECT(read(dir, key, &got) == MISS && got.empty(), "before the write, %zu bytes", n);
        EXPECT(write(dir, key, p.data(), p.size()), "write of %zu bytes", n);
        EXPECT(read(dir, key, &got) == HIT, "read of %zu bytes", n);
        EXPECT(got == p, "payload of %zu bytes differs", n);
        EXPECT(slurp(path_of(dir, key)).size() == kHeaderBytes + n, "file size for %zu bytes", n);
        EXPECT(write(dir, key, p.data(), p.size()) && read(dir, key, &got) == HIT && got == p, "written over, %zu bytes", n);
    }
    printf("roundtrip: %zu sizes\n", sizeof sizes / sizeof *sizes);
}

static void check_truncated(const std::string &dir)
{
    const Digest key = key_of(fixed_input());
    const std::vector<char> p = payload_of(777, 3);
    EXPECT(write(dir, key, p.data(), p.size()), "write");
    const std::vector<char> whole = slurp(path_of(dir, key));
    EXPECT(whole.size() == kHeaderBytes + p.size(), "size %zu", whole.size());
    std::vector<char> got;
    const size_t cuts[] = {0, 5, 8, 12, 20, 28, 36, 43, kHeaderBytes, kHeaderBytes + 1, whole.size() - 1};
    for (size_t n : cuts) {
        spit(path_of(dir, key), whole, n);
        EXPECT(read(dir, key, &got) == REJECT && got.empty(), "cut at %zu of %zu", n, whole.size());
    }
    std::vector<char> longer = whole;
    longer.push_back('\0');
    spit(path_of(dir, key), longer, longer.size());
    EXPECT(read(dir, key, &got) == REJECT, "one byte too many");
    spit(path_of(dir, key), whole, whole.size());
    EXPECT(read(dir, key, &got) == HIT && got == p, "the whole file again");
    // a rejected file is replaced by the write that follows the compile
    spit(path_of(dir, key), whole, 10);
    EXPECT(read(dir, key, &got) == REJECT, "cut again");
    EXPECT(write(dir, key, p.data(), p.size()) && read(dir, key, &got) == HIT && got == p, "replaced");
    printf("truncated: %zu cuts\n", sizeof cuts / sizeof *cuts);
}

static void check_flipped(const std::string &dir)
{
    const Digest key = key_of(fixed_input());
    const std::vector<char> p = payload_of(1000, 4);
    EXPECT(write(dir, key, p.data(), p.size()), "write");
    const std::vector<char> whole = slurp(path_of(dir, key));
    std::vector<char> got;
    // every byte of the header (magic 0-7, version 8-11, digest 12-27, length 28-35, checksum 36-43), and the payload's first, a middle and last byte
    std::vector<size_t> where;
    for (size_t i = 0; i < kHeaderBytes; ++i) where.push_back(i);
    where.push_back(kHeaderBytes); where.push_back(kHeaderBytes + 500); where.push_back(whole.size() - 1);
    for (size_t i : where)
        for (int bit : {0, 7}) {
            std::vector<char> bad = whole;
            bad[i] = (char)(bad[i] ^ (1 << bit));
            spit(path_of(dir, key), bad, bad.size());
            EXPECT(read(dir, key, &got) == REJECT && got.empty(), "byte %zu bit %d flipped", i, bit);
        }
    spit(path_of(dir, key), whole, whole.size());
    EXPECT(read(dir, key, &got) == HIT && got == p, "the whole file again");
    printf("flipped: %zu bytes x 2 bits\n", where.size());
}

static void check_other_key(const std::string &dir)
{
    KeyInput a = fixed_input(), b = fixed_input();
    b.arch = "gfx950:sramecc-:xnack-";
    const Digest ka = key_of(a), kb = key_of(b);
    EXPECT(!(ka == kb), "two keys");
    const std::vector<char> p = payload_of(300, 5);
    EXPECT(write(dir, kb, p.data(), p.size()), "write");
    const std::vector<char> other = slurp(path_of(dir, kb));
    spit(path_of(dir, ka), other, other.size());             // a complete, valid file — of another key — under this key's name
    std::vector<char> got;
    EXPECT(read(dir, ka, &got) == REJECT && got.empty(), "another key's file");
    EXPECT(read(dir, kb, &got) == HIT && got == p, "its own name");
    printf("other_key: ok\n");
}

static void check_leftover_tmp(const std::string &dir)
{
    const Digest key = key_of(fixed_input());
    const std::vector<char> p = payload_of(200, 6), junk = payload_of(50, 7);
    // what a writer that died half-way leaves behind, under the names this process would choose next and under a foreign one
    char name[64];
    for (unsigned i = 0; i < 4; ++i) {
        snprintf(name, sizeof name, ".tmp.%ld.%u", (long)getpid(), i);
        spit(path_of(dir, key) + name, junk, junk.size());
    }
    spit(path_of(dir, key) + ".tmp.1.0", junk, junk.size());
    std::vector<char> got;
    EXPECT(read(dir, key, &got) == MISS, "temporary files are not the entry");
    EXPECT(write(dir, key, p.data(), p.size()), "write beside leftovers (taken names are skipped)");
    EXPECT(read(dir, key, &got) == HIT && got == p, "read beside leftovers");
    EXPECT(slurp(path_of(dir, key) + ".tmp.1.0") == junk, "a foreign temporary file is left alone");
    printf("leftover_tmp: ok\n");
}

static void check_digest_inputs(const std::string &)
{
    const KeyInput base = fixed_input();
    std::map<std::string, std::function<void(KeyInput &)>> changes = {
        {"src_iter", [](KeyInput &k) { k.src_iter += " "; }},
        {"src_variations", [](KeyInput &k) { k.src_variations += " "; }},
        {"src_device", [](KeyInput &k) { k.src_device += " "; }},
        {"src_abi", [](KeyInput &k) { k.src_abi += " "; }},
        {"spec_header", [](KeyInput &k) { k.spec_header[k.spec_header.size() - 2] = '4'; }},
        {"option_0", [](KeyInput &k) { k.options[0] = "--offload-arch=gfx942"; }},
        {"option_1", [](KeyInput &k) { k.options[1] = "-O2"; }},
        {"option_2", [](KeyInput &k) { k.options[2] = "-DFL_LOG_PACK3=0"; }},
        {"option_3_budget", [](KeyInput &k) { k.options[3] = "-DFL_HOIST_BUDGET=5"; }},
        {"option_added", [](KeyInput &k) { k.options.push_back("-DX"); }},
        {"option_dropped", [](KeyInput &k) { k.options.pop_back(); }},
        {"option_order", [](KeyInput &k) { std::swap(k.options[1], k.options[2]); }},
        {"option_split", [](KeyInput &k) { k.options[1] = "-O"; k.options.insert(k.options.begin() + 2, "3"); }},
        {"field_boundary", [](KeyInput &k) { k.src_device += k.src_abi[0]; k.src_abi.erase(0, 1); }},
        {"arch", [](KeyInput &k) { k.arch = "gfx950:sramecc+:xnack+"; }},
        {"arch_features_dropped", [](KeyInput &k) { k.arch = "gfx950"; }},
        {"version", [](KeyInput &k) { k.version += 1; }},
    };
    std::map<std::string, std::string> seen = {{hex(key_of(base)), "base"}};
    for (auto &c : changes) {
        KeyInput k = base;
        c.second(k);
        const std::string h = hex(key_of(k));
        EXPECT(!seen.count(h), "%s gives the digest of %s", c.first.c_str(), seen[h].c_str());
        seen[h] = c.first;
    }
    EXPECT(key_of(base) == key_of(fixed_input()), "the same input twice");
    printf("digest_inputs: %zu changes, %zu digests\n", changes.size(), seen.size());
}

static void check_digest(const std::string &)
{
    // the digest of one fixed input, for the literal in tests/test_cpu_rtc_cache.py; and MurmurHash3_x64_128's digest of nothing
    printf("digest %s\n", hex(key_of(fixed_input())).c_str());
    printf("empty %s\n", hex(murmur3_128("", 0, 0)).c_str());
    printf("hello %s\n", hex(murmur3_128("hello", 5, 0)).c_str());
    printf("pangram %s\n", hex(murmur3_128("The quick brown fox jumps over the lazy dog", 43, 0)).c_str());
    printf("format %u header %zu\n", kFormatVersion, kHeaderBytes);
}

static void check_dir(const std::string &dir)
{
    std::string why;
    EXPECT(prepare_dir(dir, &why), "an existing directory: %s", why.c_str());
    EXPECT(prepare_dir(dir + "/made", &why) && prepare_dir(dir + "/made", &why), "one missing level is made: %s", why.c_str());
    EXPECT(!prepare_dir(dir + "/a/b", &why), "two missing levels are not");
    spit(dir + "/file", payload_of(4, 1), 4);
    EXPECT(!prepare_dir(dir + "/file", &why), "a regular file");
    EXPECT(!prepare_dir(dir + "/file/sub", &why), "below a regular file");
    EXPECT(!prepare_dir("", &why), "the empty path");
    std::vector<char> got;
    EXPECT(read(dir + "/file/sub", key_of(fixed_input()), &got) != HIT, "a read there is a miss");
    EXPECT(!write(dir + "/file/sub", key_of(fixed_input()), "x", 1), "a write there fails");
    printf("dir: ok\n");
}

int main(int argc, char **argv)
{
    const std::map<std::string, void (*)(const std::string &)> checks = {
        {"roundtrip", check_roundtrip}, {"truncated", check_truncated}, {"flipped", check_flipped}, {"other_key", check_other_key},
        {"leftover_tmp", check_leftover_tmp}, {"digest_inputs", check_digest_inputs}, {"digest", check_digest}, {"dir", check_dir}};
    if (argc != 3 || !checks.count(argv[1])) {
        fprintf(stderr, "usage: rtc_cache_probe <check> <dir>\n");
        return 2;
    }
    checks.at(argv[1])(argv[2]);
    return g_fail ? 1 : 0;
}
