// jpeg.hip — baseline JPEG (SOF0, 8 bit, 4:4:4 or 4:2:0, one interleaved scan, restart intervals) from u8 planar Y/Cb/Cr on the
// device.  DESIGN.md §4.8 (4:4:4) and §4.10 (4:2:0: the same kernels, instantiated for an MCU of six blocks).  Four launches per
// frame, no host wait between them:
//   k_jpeg_dct          one lane per 8x8 block: load (edge replicated), level shift, float32 DCT, quantise, zigzag -> int16, and the
//                       bit length of the block's AC symbols
//   k_jpeg_entropy<S,0> one wave per restart interval: DC differences, prefix sum of the blocks' bit lengths, bits packed in LDS,
//                       0xFF counted -> the interval's byte length (stuffing and marker included)
//   k_jpeg_scan         one workgroup: exclusive scan of the intervals' byte lengths, the 16-byte record and the header
//   k_jpeg_entropy<S,1> the same packing again, stuffed in LDS, stored at the interval's place with dword stores
// The intervals are byte aligned and independent (the DC predictor restarts), which is what makes the scan parallel; nothing is
// stored at or beyond `cap`: the last pass stores nothing when the stream does not fit.
// With `optimize` the frame's own Huffman tables take the place of Annex K's, three launches more:
//   k_jpeg_hist         one lane per block: how often the scan will emit every symbol of the four tables
//   k_jpeg_tables       a workgroup per table: the four length-limited codes (build_lengths), the symbol table the entropy kernel reads,
//                       and BITS / HUFFVAL into the header's DHT segments
//   k_jpeg_acbits       one lane per block: the bit length of the block's AC symbols under the new lengths
// and k_jpeg_entropy<S, *, true> and k_jpeg_scan<true>, which read those tables and leave the DHT bodies alone.
#include "kernels.h"
#include "encode_device.h"

namespace {

// ITU T.81 Annex K.3-K.6: the "typical" Huffman tables (BITS, HUFFVAL)
constexpr uint8_t kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
// Annex K.1 / K.2: the base quantisation tables, row-major
constexpr uint8_t kQLum[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                               14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kQChr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                               47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// zigzag position -> row-major index (v * 8 + u, u the horizontal frequency)
constexpr uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// code | length << 16 by symbol: [0, 16) DC luminance, [16, 32) DC chrominance, [32, 288) AC luminance, [288, 544) AC chrominance
enum { kDcLum = 0, kDcChr = 16, kAcLum = 32, kAcChr = 288, kHuffWords = 544 };
struct HuffTabs { uint32_t e[kHuffWords]; };
constexpr void huff_fill(uint32_t *dst, const uint8_t *bits, const uint8_t *vals)      // T.81 Annex C: codes in order of length
{
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) dst[vals[k++]] = code++ | (uint32_t)len << 16;
        code <<= 1;
    }
}
constexpr HuffTabs make_huff()
{
    HuffTabs t = {};
    huff_fill(t.e + kDcLum, kDcLumBits, kDcVals);
    huff_fill(t.e + kDcChr, kDcChrBits, kDcVals);
    huff_fill(t.e + kAcLum, kAcLumBits, kAcLumVals);
    huff_fill(t.e + kAcChr, kAcChrBits, kAcChrVals);
    return t;
}
__device__ const HuffTabs g_huff = make_huff();

// 0.5 * C(u) * cos((2x + 1) u pi / 16), C(0) = 1 / sqrt(2): the T.81 normalisation, one factor per axis
struct DctTab { float c[8][8]; };
constexpr DctTab make_dct()
{
    constexpr double cs[9] = {1.0, 0.98078528040323044913, 0.92387953251128675613, 0.83146961230254523708, 0.70710678118654752440,
                              0.55557023301960222474, 0.38268343236508977173, 0.19509032201612826785, 0.0};
    DctTab t = {};
    for (int u = 0; u < 8; ++u)
        for (int x = 0; x < 8; ++x) {
            int m = (2 * x + 1) * u % 32;
            if (m > 16) m = 32 - m;
            const double c = m > 8 ? -cs[16 - m] : cs[m];
            t.c[u][x] = (float)(0.5 * (u == 0 ? cs[4] : 1.0) * c);
        }
    return t;
}
constexpr DctTab kDct = make_dct();

struct JpegQuant { float q[2][64]; };                     // divisors by row-major index: luminance, chrominance
struct JpegHeaderArg { unsigned char b[640]; };           // FL_JPEG_HEADER_BYTES bytes, as a kernel argument: no copy to order

__device__ __forceinline__ int nbits_of(int v) { const int a = v < 0 ? -v : v; return 32 - __clz(a); }      // magnitude category (0 for 0)

// The sampling is a compile-time parameter S of every kernel (FL_JPEG_444 / FL_JPEG_420).  An MCU holds NB blocks, `slot` counting
// them in the order of the scan: 4:4:4 Y, Cb, Cr of 8 x 8 pixels; 4:2:0 Y00, Y01, Y10, Y11, Cb, Cr of 16 x 16 pixels.
template <int S> struct Mcu {
    static constexpr uint32_t NB = S ? 6u : 3u;               // blocks
    static constexpr uint32_t BITS = NB * 1660u;              // worst case of a block: DC 11 + 11 bits, 63 AC of 16 + 10 bits = 1660 bits
    static constexpr uint32_t BITS_OPT = NB * 1661u;          // ... with a frame's own tables: a DC code of 13 leaves can take 12 bits
    __host__ __device__ static constexpr uint32_t bits(bool opt) { return opt ? BITS_OPT : BITS; }
    __host__ __device__ static constexpr uint32_t comp(uint32_t slot) { return S ? (slot < 4u ? 0u : slot - 3u) : slot; }
    // how many blocks back the component's previous block lies: 4:2:0 Y runs through the MCU's four blocks and on into the next
    // MCU (Y00 follows the Y11 three blocks before it), Cb and Cr run MCU to MCU
    __host__ __device__ static constexpr uint32_t back(uint32_t slot) { return S ? (slot == 0u ? 3u : slot < 4u ? 1u : 6u) : 3u; }
};

// ---- load + DCT + quantise -------------------------------------------------------------------------------------------
// grid (ceil(nmcu / 256), NB): blockIdx.y is the block's slot in the MCU, so the quantiser table is wave-uniform.
// coef[(NB * mcu + slot) * 64 + k] in zigzag order (the order of the scan); acbits[NB * mcu + slot] = bits of the block's AC symbols.
// 4:2:0 chroma: a sample is (a + b + c + d + 2) >> 2 over the 2 x 2 full-resolution samples, their coordinates clamped first.
template <int S>
__global__ void __launch_bounds__(256)
k_jpeg_dct(const unsigned char *__restrict__ src, uint32_t w, uint32_t h, uint32_t mw, uint32_t nmcu, JpegQuant Q,
           short *__restrict__ coef, unsigned short *__restrict__ acbits)
{
    __shared__ unsigned char s_len[256];
    const uint32_t slot = blockIdx.y, comp = Mcu<S>::comp(slot);
    s_len[threadIdx.x] = (unsigned char)(g_huff.e[(comp ? kAcChr : kAcLum) + threadIdx.x] >> 16);
    __syncthreads();
    const uint32_t mcu = blockIdx.x * 256u + threadIdx.x;
    if (mcu >= nmcu) return;
    const uint32_t bx = mcu % mw, by = mcu / mw;
    const unsigned char *plane = src + (size_t)comp * w * h;
    float f[64];
    if (S && comp) {
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const unsigned char *r0 = plane + (size_t)min(by * 16u + 2u * y, h - 1u) * w;
            const unsigned char *r1 = plane + (size_t)min(by * 16u + 2u * y + 1u, h - 1u) * w;
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                const uint32_t x0 = min(bx * 16u + 2u * x, w - 1u), x1 = min(bx * 16u + 2u * x + 1u, w - 1u);
                f[y * 8 + x] = (float)(((uint32_t)r0[x0] + r0[x1] + r1[x0] + r1[x1] + 2u) >> 2) - 128.0f;
            }
        }
    } else {
        const uint32_t ox = S ? bx * 16u + (slot & 1u) * 8u : bx * 8u, oy = S ? by * 16u + (slot >> 1) * 8u : by * 8u;
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            const uint32_t yy = min(oy + y, h - 1u);              // the last row / column is replicated into partial blocks
            const unsigned char *row = plane + (size_t)yy * w;
#pragma unroll
            for (int x = 0; x < 8; ++x) f[y * 8 + x] = (float)row[min(ox + x, w - 1u)] - 128.0f;
        }
    }
    float t[64];
#pragma unroll
    for (int y = 0; y < 8; ++y)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float s = kDct.c[u][0] * f[y * 8];
#pragma unroll
            for (int x = 1; x < 8; ++x) s += kDct.c[u][x] * f[y * 8 + x];
            t[y * 8 + u] = s;
        }
    const float *q = Q.q[comp ? 1 : 0];
    short z[64];                                              // row-major
#pragma unroll
    for (int v = 0; v < 8; ++v)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            float s = kDct.c[v][0] * t[u];
#pragma unroll
            for (int y = 1; y < 8; ++y) s += kDct.c[v][y] * t[y * 8 + u];
            // |AC| < 925 and |DC| <= 1024 for 8-bit samples: the clamp only keeps the symbol tables' index in range whatever the bytes
            z[v * 8 + u] = (short)fminf(fmaxf(rintf(s / q[v * 8 + u]), v + u ? -1023.0f : -2047.0f), v + u ? 1023.0f : 2047.0f);
        }
    const uint32_t blk = Mcu<S>::NB * mcu + slot;
    uint4 *dst = (uint4 *)(coef + (size_t)blk * 64);
    uint32_t bits = 0, run = 0;
#pragma unroll
    for (int k8 = 0; k8 < 8; ++k8) {
        uint32_t pk[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k8 * 8 + 2 * j;
            pk[j] = (uint32_t)(unsigned short)z[kZigzag[k]] | (uint32_t)(unsigned short)z[kZigzag[k + 1]] << 16;
        }
        dst[k8] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k8 * 8 + j;
            if (k == 0) continue;
            const int v = z[kZigzag[k]];
            if (v == 0) { ++run; continue; }
            bits += (run >> 4) * s_len[0xf0];                 // ZRL per 16 zeros
            const int s = nbits_of(v);
            bits += s_len[(run & 15u) << 4 | s] + s;
            run = 0;
        }
    }
    if (run) bits += s_len[0];                                // EOB
    acbits[blk] = (unsigned short)bits;
}

// ---- entropy coding of one restart interval per wave -------------------------------------------------------------------
// Worst case of an MCU: Mcu<S>::BITS, 4980 bits in 4:4:4 and 9960 in 4:2:0.
struct Bits {                         // a lane's writer into the interval's bit buffer (big-endian 32-bit words; a word may be shared with the neighbouring lanes' blocks)
    uint32_t *words; uint32_t w; u64 acc; uint32_t n;
    __device__ __forceinline__ void put(uint32_t code, uint32_t len)       // 1 <= len <= 26, n < 32
    {
        acc |= (u64)code << (64u - n - len);
        n += len;
        if (n >= 32u) { atomicOr(&words[w++], (uint32_t)(acc >> 32)); acc <<= 32; n -= 32u; }
    }
    __device__ __forceinline__ void flush() { if (n) atomicOr(&words[w], (uint32_t)(acc >> 32)); }
};

// One workgroup of one wave per interval of `ri` MCUs (NB * ri <= 64: a lane per block).  WRITE = false: lens[interval] = bytes of the
// interval, stuffing and the RSTm / EOI marker behind it included.  WRITE = true: the bytes go to out + base + offs[interval],
// unless info[kInfoStatus] (the status the scan left) says that the stream does not fit.
// LDS, sized for the worst case of ri MCUs whatever the input (launch_jpeg_kernels): the symbol tables | bit buffer of
// ceil(ri * BITS / 32) + 2 words | stuffed bytes, 2 * ceil(ri * BITS / 8) + 2 and 8 of padding
// OPT: the symbol tables are the frame's own, read from `huff` (k_jpeg_tables wrote them), and BITS is BITS_OPT.
template <int S, bool WRITE, bool OPT = false>
__global__ void __launch_bounds__(64)
k_jpeg_entropy(const short *__restrict__ coef, const unsigned short *__restrict__ acbits, uint32_t nmcu, uint32_t ri, uint32_t nint,
               uint32_t *__restrict__ lens, const u64 *__restrict__ offs, const uint32_t *__restrict__ info,
               unsigned char *__restrict__ out, uint32_t base, const uint32_t *__restrict__ huff)
{
    extern __shared__ uint32_t s_mem[];
    uint32_t *s_huff = s_mem, *s_bits = s_mem + kHuffWords;
    constexpr uint32_t NB = Mcu<S>::NB;
    const uint32_t nbw = (ri * Mcu<S>::bits(OPT) + 31u) / 32u + 2u;
    unsigned char *s_out = (unsigned char *)(s_bits + nbw);
    const uint32_t lane = threadIdx.x, it = blockIdx.x;
    if (WRITE && info[kInfoStatus]) return;
    for (uint32_t i = lane; i < kHuffWords; i += 64) s_huff[i] = OPT ? huff[i] : g_huff.e[i];
    const uint32_t mcu0 = it * ri, nb = NB * min(ri, nmcu - mcu0);
    const bool live = lane < nb;
    const uint32_t slot = lane % NB, comp = Mcu<S>::comp(slot), back = Mcu<S>::back(slot);
    const size_t blk = (size_t)NB * mcu0 + lane;
    const uint4 *cp = (const uint4 *)(coef + blk * 64);
    uint4 cw[8];
    int diff = 0;
    uint32_t mybits = 0;
    if (live) {
#pragma unroll
        for (int j = 0; j < 8; ++j) cw[j] = cp[j];
        const int dc = (short)(cw[0].x & 0xffffu);
        const int pred = lane >= back ? (int)coef[(blk - back) * 64] : 0;  // the previous block of the component; 0 at the interval's start
        diff = dc - pred;
        mybits = acbits[blk] + (uint32_t)nbits_of(diff);                   // (the DC code's length is added below, from the table)
    }
    __syncthreads();                                                       // the tables are in LDS
    const uint32_t *dctab = s_huff + (comp ? kDcChr : kDcLum), *actab = s_huff + (comp ? kAcChr : kAcLum);
    const int ds = nbits_of(diff);
    if (live) mybits += dctab[ds] >> 16;
    const uint32_t incl = wave_incl_scan(mybits, lane);
    const uint32_t T = __shfl(incl, 63, 64);
    const uint32_t pad = (8u - (T & 7u)) & 7u, N = (T + pad) >> 3, nw = (N + 3u) >> 2;      // N bytes before stuffing, nw words
    for (uint32_t i = lane; i <= nw; i += 64) s_bits[i] = 0;
    __syncthreads();
    if (live) {
        const uint32_t start = incl - mybits;
        Bits b = {s_bits, start >> 5, 0, start & 31u};
        b.put(dctab[ds] & 0xffffu, dctab[ds] >> 16);
        if (ds) b.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << ds) - 1u), (uint32_t)ds);
        uint32_t run = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t wd[4] = {cw[j].x, cw[j].y, cw[j].z, cw[j].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (j == 0 && e == 0) continue;
                const int v = (short)(wd[e >> 1] >> ((e & 1) * 16) & 0xffffu);
                if (v == 0) { ++run; continue; }
                for (; run > 15u; run -= 16u) b.put(actab[0xf0] & 0xffffu, actab[0xf0] >> 16);
                const int s = nbits_of(v);
                const uint32_t sym = actab[run << 4 | (uint32_t)s];
                b.put(sym & 0xffffu, sym >> 16);
                b.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u), (uint32_t)s);
                run = 0;
            }
        }
        if (run) b.put(actab[0] & 0xffffu, actab[0] >> 16);
        if (lane == nb - 1u && pad) b.put((1u << pad) - 1u, pad);          // the interval is padded to a byte with 1-bits
        b.flush();
    }
    __syncthreads();
    // stuffing: every lane takes `per` consecutive words; a prefix sum of their 0xFF counts places each lane's bytes
    const uint32_t per = (nw + 63u) / 64u, lo = min(lane * per, nw), hi = min(lo + per, nw);
    uint32_t nff = 0;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t wd = s_bits[i];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) nff += (4u * i + k < N && (wd >> (24u - 8u * k) & 0xffu) == 0xffu) ? 1u : 0u;
    }
    const uint32_t ffincl = wave_incl_scan(nff, lane);
    const uint32_t L = N + __shfl(ffincl, 63, 64) + 2u;                    // + the marker
    if (!WRITE) {
        if (lane == 0) lens[it] = L;
        return;
    }
    uint32_t o = 4u * lo + (ffincl - nff);
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t wd = s_bits[i];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t byte = wd >> (24u - 8u * k) & 0xffu;
            if (4u * i + k < N) {
                s_out[o++] = (unsigned char)byte;
                if (byte == 0xffu) s_out[o++] = 0;
            }
        }
    }
    if (lane == 0) {
        s_out[L - 2u] = 0xff;
        s_out[L - 1u] = it + 1u == nint ? 0xd9 : (unsigned char)(0xd0u + (it & 7u));      // EOI behind the last interval, RSTm behind the others
    }
    __syncthreads();
    store_bytes<64>(out + (size_t)base + offs[it], s_bits + nbw, L, lane);      // (s_out, with the 8 bytes of padding behind it)
}

// ---- where the intervals go ------------------------------------------------------------------------------------------
// One workgroup: offs[i] = sum of lens[0 .. i), info as encode_device.h lays it out; the record and the header go to `out`.
// OPT: but for BITS and HUFFVAL of the four DHT segments, which k_jpeg_tables has written there.
// Where they lie in the header: SOI 2, APP0 18, DQT 2 x 69, SOF0 19 = 177, then FFC4, the length and the class / id in front of each.
enum { kDhtDcLum = 177 + 5, kDhtAcLum = kDhtDcLum + 28 + 5, kDhtDcChr = kDhtAcLum + 178 + 5, kDhtAcChr = kDhtDcChr + 28 + 5 };
static_assert(kDhtAcChr + 178 + 6 + 14 == FL_JPEG_HEADER_BYTES, "header layout");
__host__ __device__ constexpr bool in_dht_body(uint32_t t)
{
    return (t >= kDhtDcLum && t < kDhtDcLum + 28u) || (t >= kDhtAcLum && t < kDhtAcLum + 178u) || (t >= kDhtDcChr && t < kDhtDcChr + 28u) ||
           (t >= kDhtAcChr && t < kDhtAcChr + 178u);
}
template <bool OPT>
__global__ void __launch_bounds__(1024)
k_jpeg_scan(const uint32_t *__restrict__ lens, uint32_t nint, u64 *__restrict__ offs, uint32_t *__restrict__ info,
            unsigned char *__restrict__ out, u64 cap, uint32_t ri, JpegHeaderArg hdr)
{
    __shared__ u64 s_sum[1024];
    const uint32_t t = threadIdx.x;
    const auto len = [&](uint32_t i) { return lens[i]; };
    const Placement p = place_pieces(s_sum, nint, t, 0ull, len);
    store_offsets(offs, p, len);
    finish_placement(info, out, (u64)FL_JPEG_HEADER_BYTES + p.total, cap, ri, 0u, t);      // (the header's bytes and the stream's lie behind the record)
    if (t < FL_JPEG_HEADER_BYTES && !(OPT && in_dht_body(t))) out[16u + t] = hdr.b[t];      // (cap >= 16 + the header: the callers checked)
}

// ---- a frame's own Huffman tables (`optimize`) --------------------------------------------------------
// The legal symbols of a table, all of which its DHT lists whether the frame uses them or not (the header keeps its length):
// the DC categories 0..11; EOB, ZRL and run 0..15 x size 1..10.
__device__ __forceinline__ bool legal_symbol(bool ac, uint32_t s) { return ac ? s == 0u || s == 0xf0u || ((s & 15u) >= 1u && (s & 15u) <= 10u) : s < 12u; }

// f(symbol) for every AC symbol the scan emits for the block whose coefficients are cw, in the order of the scan
template <class Fn>
__device__ __forceinline__ void for_ac_symbols(const uint4 (&cw)[8], Fn &&f)
{
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t wd[4] = {cw[j].x, cw[j].y, cw[j].z, cw[j].w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (j == 0 && e == 0) continue;
            const int v = (short)(wd[e >> 1] >> ((e & 1) * 16) & 0xffffu);
            if (v == 0) { ++run; continue; }
            for (; run > 15u; run -= 16u) f(0xf0u);
            f(run << 4 | (uint32_t)nbits_of(v));
            run = 0;
        }
    }
    if (run) f(0u);
}

// One lane per block (nblk = NB * nmcu <= 2^24 of them): counts[] += how often the scan emits each symbol, laid out as the symbol
// tables are (kDcLum ..).  The DC difference is the entropy kernel's: the predictor is the component's previous block, 0 at the
// start of every interval of ri MCUs.  A workgroup counts in LDS and adds what it found to the frame's counts, which the caller
// cleared; integer sums, so the order does not matter.
template <int S>
__global__ void __launch_bounds__(256)
k_jpeg_hist(const short *__restrict__ coef, uint32_t nblk, uint32_t ri, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t s_cnt[kHuffWords];
    constexpr uint32_t NB = Mcu<S>::NB;
    const uint32_t t = threadIdx.x, blk = blockIdx.x * 256u + t;
    for (uint32_t i = t; i < kHuffWords; i += 256u) s_cnt[i] = 0;
    __syncthreads();
    if (blk < nblk) {
        const uint32_t mcu = blk / NB, slot = blk - mcu * NB, comp = Mcu<S>::comp(slot), back = Mcu<S>::back(slot);
        const uint32_t pos = (mcu % ri) * NB + slot;                       // the block's lane in its interval
        const uint4 *cp = (const uint4 *)(coef + (size_t)blk * 64);
        uint4 cw[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) cw[j] = cp[j];
        const int dc = (short)(cw[0].x & 0xffffu);
        const int pred = pos >= back ? (int)coef[(size_t)(blk - back) * 64] : 0;
        atomicAdd(&s_cnt[(comp ? kDcChr : kDcLum) + (uint32_t)nbits_of(dc - pred)], 1u);      // (a category is at most 12 < 16)
        uint32_t *ac = s_cnt + (comp ? kAcChr : kAcLum);
        for_ac_symbols(cw, [&](uint32_t sym) { atomicAdd(&ac[sym], 1u); });
    }
    __syncthreads();
    for (uint32_t i = t; i < kHuffWords; i += 256u) { const uint32_t c = s_cnt[i]; if (c) atomicAdd(&counts[i], c); }
}

// Four workgroups of 256 threads, one per table in the order of the file: freq = 2 * count + 2 for the legal symbols and 1 for a
// pseudo-symbol behind them (strictly the rarest: it takes a longest code, which keeps the all-ones codeword unassigned, as
// T.81 demands), build_lengths with the limit 16, codes as in T.81 Annex C.  huff[] = code | length << 16 by symbol, the table
// k_jpeg_entropy<.., true> reads; BITS and HUFFVAL (the legal symbols by (length, symbol)) go into the header at out + 16.
// Listing every legal symbol has a price on frames of a few dozen symbols: where sum count * length is not below what Annex K's
// table of the same kind costs, the table keeps Annex K's lengths.  Those tables too list their symbols by (length, symbol), so the
// steps that follow write Annex K's BITS, HUFFVAL and codes; with all four kept the file is the one without `optimize`.
__global__ void __launch_bounds__(256)
k_jpeg_tables(const uint32_t *__restrict__ counts, uint32_t *__restrict__ huff, unsigned char *__restrict__ out)
{
    __shared__ HuffTmp T;
    __shared__ uint32_t s_freq[kSymPad], s_n[17], s_first[17], s_pos[17];
    __shared__ unsigned char s_lens[kSymPad];
    __shared__ unsigned long long s_cost[2];                               // code bits of the frame's symbols: with the new lengths, with Annex K's
    const uint32_t t = threadIdx.x, tab = blockIdx.x;
    const bool ac = tab & 1u;
    const uint32_t base = tab == 0 ? kDcLum : tab == 1u ? kAcLum : tab == 2u ? kDcChr : kAcChr;
    const uint32_t body = tab == 0 ? kDhtDcLum : tab == 1u ? kDhtAcLum : tab == 2u ? kDhtDcChr : kDhtAcChr;
    const uint32_t pseudo = ac ? 256u : 12u, nwords = ac ? 256u : 16u;
    for (uint32_t i = t; i < kSymPad; i += 256u) s_freq[i] = i < pseudo ? (legal_symbol(ac, i) ? 2u * counts[base + i] + 2u : 0u) : i == pseudo ? 1u : 0u;
    if (t < 17u) s_n[t] = 0;
    if (t < 2u) s_cost[t] = 0;
    __syncthreads();
    build_lengths(s_freq, pseudo + 1u, 16u, s_lens, T);
    for (uint32_t i = t; i < pseudo; i += 256u) {
        const uint32_t c = legal_symbol(ac, i) ? counts[base + i] : 0u;
        if (c) {
            atomicAdd(&s_cost[0], (unsigned long long)c * s_lens[i]);
            atomicAdd(&s_cost[1], (unsigned long long)c * (g_huff.e[base + i] >> 16));
        }
    }
    __syncthreads();
    if (s_cost[0] >= s_cost[1])
        for (uint32_t i = t; i < pseudo; i += 256u) if (legal_symbol(ac, i)) s_lens[i] = (unsigned char)(g_huff.e[base + i] >> 16);
    __syncthreads();
    for (uint32_t i = t; i < pseudo; i += 256u) if (legal_symbol(ac, i)) atomicAdd(&s_n[s_lens[i]], 1u);
    __syncthreads();
    if (t == 0) {
        uint32_t code = 0, k = 0;
        for (uint32_t l = 1; l <= 16u; ++l) { s_first[l] = code; s_pos[l] = k; code = (code + s_n[l]) << 1; k += s_n[l]; }
    }
    __syncthreads();
    unsigned char *dht = out + 16u + body;
    if (t < 16u) dht[t] = (unsigned char)s_n[t + 1u];
    for (uint32_t i = t; i < nwords; i += 256u) {
        uint32_t e = 0;
        if (legal_symbol(ac, i)) {
            const uint32_t l = s_lens[i];
            uint32_t r = 0;                                            // (the other symbols have length 0, the pseudo-symbol lies behind)
#pragma unroll 8
            for (uint32_t j = 0; j < i; ++j) r += s_lens[j] == l ? 1u : 0u;
            e = (s_first[l] + r) | l << 16;
            dht[16u + s_pos[l] + r] = (unsigned char)i;
        }
        huff[base + i] = e;
    }
}

// One lane per block: acbits[] of k_jpeg_dct again, with the lengths of the frame's own AC tables
template <int S>
__global__ void __launch_bounds__(256)
k_jpeg_acbits(const short *__restrict__ coef, uint32_t nblk, const uint32_t *__restrict__ huff, unsigned short *__restrict__ acbits)
{
    __shared__ unsigned char s_len[512];                                   // luminance | chrominance
    static_assert(kAcChr == kAcLum + 256, "the AC tables are adjacent");
    const uint32_t t = threadIdx.x, blk = blockIdx.x * 256u + t;
    s_len[t] = (unsigned char)(huff[kAcLum + t] >> 16);
    s_len[256u + t] = (unsigned char)(huff[kAcLum + 256u + t] >> 16);
    __syncthreads();
    if (blk >= nblk) return;
    const unsigned char *len = s_len + (Mcu<S>::comp(blk % Mcu<S>::NB) ? 256u : 0u);
    const uint4 *cp = (const uint4 *)(coef + (size_t)blk * 64);
    uint4 cw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cw[j] = cp[j];
    uint32_t bits = 0;
    for_ac_symbols(cw, [&](uint32_t sym) { bits += len[sym] + (sym & 15u); });      // (ZRL and EOB: no value bits, and their low nibble is 0)
    acbits[blk] = (unsigned short)bits;
}

void put16(unsigned char *&p, uint32_t v) { *p++ = (unsigned char)(v >> 8); *p++ = (unsigned char)v; }
void put_dht(unsigned char *&p, int cls_id, const uint8_t *bits, const uint8_t *vals, int nvals)
{
    put16(p, 0xffc4); put16(p, 2 + 1 + 16 + nvals);
    *p++ = (unsigned char)cls_id;
    for (int i = 0; i < 16; ++i) *p++ = bits[i];
    for (int i = 0; i < nvals; ++i) *p++ = vals[i];
}

} // namespace

// Annex K.1 / K.2 scaled the libjpeg way (jpeg_quality_scaling, jpeg_add_quant_table with force_baseline)
static void jpeg_quant_table(int quality, int chroma, unsigned char q[64])
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int v = ((chroma ? kQChr[i] : kQLum[i]) * s + 50) / 100;
        q[i] = (unsigned char)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

// SOI, APP0 (JFIF 1.01), DQT x2, SOF0, DHT x4, DRI, SOS: FL_JPEG_HEADER_BYTES bytes
static void jpeg_header(unsigned char *out, uint32_t w, uint32_t h, int quality, uint32_t ri, int sampling)
{
    unsigned char *p = out, q[64];
    put16(p, 0xffd8);
    put16(p, 0xffe0); put16(p, 16);
    for (const unsigned char c : {'J', 'F', 'I', 'F', '\0'}) *p++ = c;
    *p++ = 1; *p++ = 1; *p++ = 0; put16(p, 1); put16(p, 1); *p++ = 0; *p++ = 0;        // 1.01, no units, 1:1, no thumbnail
    for (int tab = 0; tab < 2; ++tab) {
        jpeg_quant_table(quality, tab, q);
        put16(p, 0xffdb); put16(p, 67); *p++ = (unsigned char)tab;
        for (int k = 0; k < 64; ++k) *p++ = q[kZigzag[k]];
    }
    put16(p, 0xffc0); put16(p, 17); *p++ = 8; put16(p, h); put16(p, w); *p++ = 3;
    for (int c = 0; c < 3; ++c) { *p++ = (unsigned char)(c + 1); *p++ = sampling == FL_JPEG_420 && !c ? 0x22 : 0x11; *p++ = c ? 1 : 0; }
    put_dht(p, 0x00, kDcLumBits, kDcVals, 12);
    put_dht(p, 0x10, kAcLumBits, kAcLumVals, 162);
    put_dht(p, 0x01, kDcChrBits, kDcVals, 12);
    put_dht(p, 0x11, kAcChrBits, kAcChrVals, 162);
    put16(p, 0xffdd); put16(p, 4); put16(p, ri);
    put16(p, 0xffda); put16(p, 12); *p++ = 3;
    for (int c = 0; c < 3; ++c) { *p++ = (unsigned char)(c + 1); *p++ = c ? 0x11 : 0x00; }
    *p++ = 0; *p++ = 63; *p++ = 0;
    static_assert(FL_JPEG_HEADER_BYTES == 2 + 18 + 2 * 69 + 19 + 2 * 33 + 2 * 183 + 6 + 14, "header layout");
}

JpegLayout jpeg_layout(uint32_t w, uint32_t h, uint32_t ri, int sampling)
{
    JpegLayout l;
    const uint32_t pix = sampling == FL_JPEG_420 ? 16u : 8u, nb = sampling == FL_JPEG_420 ? 6u : 3u;
    l.mw = (w + pix - 1u) / pix;
    const uint64_t nmcu = (uint64_t)l.mw * ((h + pix - 1u) / pix);     // <= 8192^2
    l.nmcu = (uint32_t)nmcu;
    l.nint = (uint32_t)((nmcu + ri - 1u) / ri);
    // words: coefficients (int16 x 64 per block) | offsets (u64) | lengths | AC bits (u16 per block) | info | `optimize`: symbol counts | symbol tables
    l.coef = 0;
    l.offs = l.coef + (size_t)nmcu * nb * 32u;
    l.lens = l.offs + 2u * (size_t)l.nint;
    l.acbits = l.lens + l.nint;
    l.info = l.acbits + ((size_t)nmcu * nb + 1u) / 2u;
    l.counts = l.info + 4u;
    l.huff = l.counts + kHuffWords;
    l.words = l.huff + kHuffWords;
    return l;
}

template <int S, bool OPT>
static void launch_jpeg_kernels(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, uint32_t ri, const JpegLayout &l,
                                const JpegQuant &Q, const JpegHeaderArg &hdr, uint32_t *scratch, unsigned char *out, size_t cap)
{
    short *coef = (short *)(scratch + l.coef);
    u64 *offs = (u64 *)(scratch + l.offs);
    uint32_t *lens = scratch + l.lens, *info = scratch + l.info;
    unsigned short *acbits = (unsigned short *)(scratch + l.acbits);
    uint32_t *counts = scratch + l.counts, *huff = OPT ? scratch + l.huff : nullptr;
    constexpr uint32_t BITS = Mcu<S>::bits(OPT);
    const uint32_t nbw = (ri * BITS + 31u) / 32u + 2u;
    const size_t lds = 4 * (size_t)(kHuffWords + nbw) + 2 * (size_t)((ri * BITS + 7u) / 8u) + 2 + 8 + 4;
    if (OPT) (void)hipMemsetAsync(counts, 0, 4 * kHuffWords, st);      // (an error stays the runtime's last error, which the caller reads)
    hipLaunchKernelGGL(k_jpeg_dct<S>, dim3((l.nmcu + 255u) / 256u, Mcu<S>::NB), dim3(256), 0, st, src, w, h, l.mw, l.nmcu, Q, coef, acbits);
    if (OPT) {
        const uint32_t nblk = Mcu<S>::NB * l.nmcu;                         // <= 2^24: the callers refuse larger frames
        hipLaunchKernelGGL(k_jpeg_hist<S>, dim3((nblk + 255u) / 256u), dim3(256), 0, st, coef, nblk, ri, counts);
        hipLaunchKernelGGL(k_jpeg_tables, dim3(4), dim3(256), 0, st, counts, huff, out);
        hipLaunchKernelGGL(k_jpeg_acbits<S>, dim3((nblk + 255u) / 256u), dim3(256), 0, st, coef, nblk, huff, acbits);
    }
    hipLaunchKernelGGL((k_jpeg_entropy<S, false, OPT>), dim3(l.nint), dim3(64), lds, st, coef, acbits, l.nmcu, ri, l.nint, lens, offs, info, out,
                       16u + FL_JPEG_HEADER_BYTES, huff);
    hipLaunchKernelGGL(k_jpeg_scan<OPT>, dim3(1), dim3(1024), 0, st, lens, l.nint, offs, info, out, (u64)cap, ri, hdr);
    hipLaunchKernelGGL((k_jpeg_entropy<S, true, OPT>), dim3(l.nint), dim3(64), lds, st, coef, acbits, l.nmcu, ri, l.nint, lens, offs, info, out,
                       16u + FL_JPEG_HEADER_BYTES, huff);
}

// ri: 1 .. 21 in 4:4:4, 1 .. 10 in 4:2:0 (the callers clamp it).  optimize: the frame's own Huffman tables (at most 2^24 blocks).
void launch_jpeg_encode(hipStream_t st, const unsigned char *src, uint32_t w, uint32_t h, int quality, uint32_t ri, int sampling, bool optimize,
                        uint32_t *scratch, unsigned char *out, size_t cap)
{
    const JpegLayout l = jpeg_layout(w, h, ri, sampling);
    JpegQuant Q;
    unsigned char q[64];
    for (int tab = 0; tab < 2; ++tab) {
        jpeg_quant_table(quality, tab, q);
        for (int i = 0; i < 64; ++i) Q.q[tab][i] = (float)q[i];
    }
    JpegHeaderArg hdr = {};
    jpeg_header(hdr.b, w, h, quality, ri, sampling);
    if (sampling == FL_JPEG_420) {
        if (optimize) launch_jpeg_kernels<FL_JPEG_420, true>(st, src, w, h, ri, l, Q, hdr, scratch, out, cap);
        else launch_jpeg_kernels<FL_JPEG_420, false>(st, src, w, h, ri, l, Q, hdr, scratch, out, cap);
    } else {
        if (optimize) launch_jpeg_kernels<FL_JPEG_444, true>(st, src, w, h, ri, l, Q, hdr, scratch, out, cap);
        else launch_jpeg_kernels<FL_JPEG_444, false>(st, src, w, h, ri, l, Q, hdr, scratch, out, cap);
    }
}

// ---- the placement helpers alone (fl_debug_place) ------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
k_debug_place(const uint32_t *__restrict__ lens, uint32_t n, u64 front, u64 *__restrict__ offs, u64 *__restrict__ total)
{
    __shared__ u64 s_sum[1024];
    const auto len = [&](uint32_t i) { return lens[i]; };
    const Placement p = place_pieces(s_sum, n, threadIdx.x, front, len);
    store_offsets(offs, p, len);
    if (threadIdx.x == 0) *total = p.total;
}

void launch_debug_place(hipStream_t st, const uint32_t *lens, uint32_t n, u64 front, u64 *offs, u64 *total)
{
    hipLaunchKernelGGL(k_debug_place, dim3(1), dim3(1024), 0, st, lens, n, front, offs, total);
}
