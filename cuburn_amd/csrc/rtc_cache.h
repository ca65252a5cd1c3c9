// rtc_cache.h — the per-genome kernels' code objects kept on disk (FLAME_RTC_CACHE=<dir>, rtc.hip).
//
// Host only: no HIP header, so a plain C++ program can include it (tests/rtc_cache_probe.cpp does).  Three things live here:
//
//   * the KEY: a 128-bit digest (MurmurHash3 x64 128, written out below) over everything that determines a code object —
//     the four embedded sources, the generated flame_spec.h, the complete option list in order, the device's full
//     architecture string and the hipRTC version.  Every field goes in behind its length, so no two inputs share a byte string.
//   * the FILE: <dir>/<32 hex digits>.co =
//         magic "FLRTCCO\0" (8) | format version u32 | digest (16) | payload length u64 | payload checksum u64 | payload
//     little-endian, 44 bytes of header.  The checksum is the first half of the same hash over the payload, seeded differently.
//   * read and write.  A file is written under a unique temporary name in the same directory and renamed into place, so a
//     reader sees a complete file or none, whoever else writes the same key.  A reader checks every field and the file's
//     length: anything wrong is a miss (REJECT), never an error; the compile that follows replaces the file.
//
// A change to the key function or the layout is a change of kFormatVersion (tests/test_cpu_rtc_cache.py pins one digest).
// Nothing is ever evicted.
#pragma once
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

namespace rtc_cache {

const uint32_t kFormatVersion = 1;
const char kMagic[8] = {'F', 'L', 'R', 'T', 'C', 'C', 'O', '\0'};
const size_t kHeaderBytes = 8 + 4 + 16 + 8 + 8;
const uint32_t kSeedKey = 0x464c4b31u, kSeedPayload = 0x464c5031u;

struct Digest {
    uint8_t b[16];
    bool operator==(const Digest &o) const { return memcmp(b, o.b, 16) == 0; }
};

// MurmurHash3_x64_128 (Austin Appleby, public domain), bytes read little-endian whatever the host
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t fmix64(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}
inline uint64_t load_le64(const uint8_t *p)
{
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = v << 8 | p[i];
    return v;
}
inline void store_le(uint8_t *p, uint64_t v, int n) { for (int i = 0; i < n; ++i) p[i] = (uint8_t)(v >> (8 * i)); }

inline Digest murmur3_128(const void *data, size_t len, uint32_t seed)
{
    const uint8_t *p = static_cast<const uint8_t *>(data);
    const size_t nblocks = len / 16;
    uint64_t h1 = seed, h2 = seed;
    const uint64_t c1 = 0x87c37b91114253d5ull, c2 = 0x4cf5ad432745937full;
    for (size_t i = 0; i < nblocks; ++i) {
        uint64_t k1 = load_le64(p + 16 * i), k2 = load_le64(p + 16 * i + 8);
        k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
        h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
        h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    const uint8_t *tail = p + 16 * nblocks;
    uint64_t k1 = 0, k2 = 0;
    const size_t rest = len & 15;
    for (size_t i = rest; i > 8; --i) k2 = k2 << 8 | tail[i - 1];
    if (rest > 8) { k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2; }
    for (size_t i = rest < 8 ? rest : 8; i > 0; --i) k1 = k1 << 8 | tail[i - 1];
    if (rest > 0) { k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1; }
    h1 ^= (uint64_t)len; h2 ^= (uint64_t)len;
    h1 += h2; h2 += h1;
    h1 = fmix64(h1); h2 = fmix64(h2);
    h1 += h2; h2 += h1;
    Digest d;
    store_le(d.b, h1, 8); store_le(d.b + 8, h2, 8);
    return d;
}

inline uint64_t payload_checksum(const char *data, size_t n) { return load_le64(murmur3_128(data, n, kSeedPayload).b); }

// Everything that determines a code object.
struct KeyInput {
    std::string src_iter, src_variations, src_device, src_abi;      // the embedded sources
    std::string spec_header;                                        // the generated flame_spec.h
    std::vector<std::string> options;                               // the complete option list, in order
    std::string arch;                                               // the device's full architecture string, target features included
    int64_t version = 0;                                            // hipRTC's version
};

inline Digest key_of(const KeyInput &k)
{
    std::string s;
    const auto num = [&s](uint64_t v) { uint8_t b[8]; store_le(b, v, 8); s.append(reinterpret_cast<const char *>(b), 8); };
    const auto field = [&](const std::string &f) { num(f.size()); s += f; };
    num(kFormatVersion);
    field(k.src_iter); field(k.src_variations); field(k.src_device); field(k.src_abi);
    field(k.spec_header);
    num(k.options.size());
    for (const std::string &o : k.options) field(o);
    field(k.arch);
    num((uint64_t)k.version);
    return murmur3_128(s.data(), s.size(), kSeedKey);
}

inline std::string hex(const Digest &d)
{
    static const char *digits = "0123456789abcdef";
    std::string s;
    for (uint8_t v : d.b) { s += digits[v >> 4]; s += digits[v & 15]; }
    return s;
}

inline std::string path_of(const std::string &dir, const Digest &key) { return dir + "/" + hex(key) + ".co"; }

// The directory, made if it is missing (one level only).  False with the reason in *why if it cannot hold the cache.
inline bool prepare_dir(const std::string &dir, std::string *why)
{
    struct stat st;
    if (dir.empty()) { *why = "empty path"; return false; }
    if (stat(dir.c_str(), &st) != 0) {
        if (mkdir(dir.c_str(), 0777) != 0 && errno != EEXIST) { *why = std::string("mkdir: ") + strerror(errno); return false; }
        if (stat(dir.c_str(), &st) != 0) { *why = std::string("stat: ") + strerror(errno); return false; }
    }
    if (!S_ISDIR(st.st_mode)) { *why = "not a directory"; return false; }
    if (access(dir.c_str(), R_OK | W_OK | X_OK) != 0) { *why = std::string("access: ") + strerror(errno); return false; }
    return true;
}

enum Result { HIT = 0, MISS = 1, REJECT = 2 };      // MISS: no such file; REJECT: a file that is short, damaged or another key's

inline Result read(const std::string &dir, const Digest &key, std::vector<char> *payload)
{
    payload->clear();
    FILE *f = fopen(path_of(dir, key).c_str(), "rb");
    if (!f) return errno == ENOENT ? MISS : REJECT;
    Result res = REJECT;
    uint8_t h[kHeaderBytes];
    do {
        if (fread(h, 1, kHeaderBytes, f) != kHeaderBytes) break;
        if (memcmp(h, kMagic, 8) != 0) break;
        uint32_t version = 0;
        for (int i = 3; i >= 0; --i) version = version << 8 | h[8 + i];
        if (version != kFormatVersion) break;
        if (memcmp(h + 12, key.b, 16) != 0) break;
        const uint64_t len = load_le64(h + 28), sum = load_le64(h + 36);
        struct stat st;
        if (fstat(fileno(f), &st) != 0 || !S_ISREG(st.st_mode) || (uint64_t)st.st_size != kHeaderBytes + len) break;      // (bounds len before anything is allocated)
        payload->resize((size_t)len);
        if (len && fread(payload->data(), 1, (size_t)len, f) != len) break;
        if (payload_checksum(payload->data(), payload->size()) != sum) break;
        res = HIT;
    } while (0);
    fclose(f);
    if (res != HIT) payload->clear();
    return res;
}

// Complete under a name of its own, then renamed into place: whoever else writes the same key, <key>.co is always whole.
inline bool write(const std::string &dir, const Digest &key, const char *data, size_t n)
{
    static unsigned serial = 0;
    const std::string dst = path_of(dir, key);
    std::string tmp;
    int fd = -1;
    for (int attempt = 0; attempt < 16 && fd < 0; ++attempt) {
        char suffix[64];
        snprintf(suffix, sizeof suffix, ".tmp.%ld.%u", (long)getpid(), __atomic_fetch_add(&serial, 1u, __ATOMIC_RELAXED));
        tmp = dst + suffix;
        fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
        if (fd < 0 && errno != EEXIST) return false;
    }
    if (fd < 0) return false;
    uint8_t h[kHeaderBytes];
    memcpy(h, kMagic, 8);
    store_le(h + 8, kFormatVersion, 4);
    memcpy(h + 12, key.b, 16);
    store_le(h + 28, n, 8);
    store_le(h + 36, payload_checksum(data, n), 8);
    bool ok = true;
    const auto put = [&](const void *p, size_t len) {
        const char *q = static_cast<const char *>(p);
        while (ok && len) {
            const ssize_t w = ::write(fd, q, len);
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) { ok = false; break; }
            q += w; len -= (size_t)w;
        }
    };
    put(h, kHeaderBytes);
    put(data, n);
    if (close(fd) != 0) ok = false;
    if (ok && rename(tmp.c_str(), dst.c_str()) != 0) ok = false;
    if (!ok) unlink(tmp.c_str());
    return ok;
}

}  // namespace rtc_cache
