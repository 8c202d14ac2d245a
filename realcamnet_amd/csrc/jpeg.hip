// JPEG output at the back of the path (include/realcam_hip.h, rc_jpeg_*): the network's planar sRGB result (B,3,H,W) -> one baseline JFIF
// file per frame, coded on the device in three launches with no host sync.
//
// jpeg_interval_kernel<TI, SUB, WRITE>: one wave (a 64-thread block) per restart interval, walking its MCUs; nothing but the source
// samples and the stuffed bytes touches memory.
//   samples   4:2:0: lane l holds the 2x2 quad (l >> 3, l & 7) of the 16x16 MCU -- four Y codes and exactly one Cb and one Cr sample;
//             4:4:4: lane l holds pixel (l >> 3, l & 7) of the 8x8 MCU.  The codes (minus 128) go to LDS, one 64-sample image per block.
//             The source is fetched per MCU (a quad's two pixels of a row in one access where they are adjacent and aligned).
//   DCT       per block, lane (y, u) = (l >> 3, l & 7) forms R'[y][u] from its row of samples (two ds_read_b128) and its row of M (8
//             registers), through LDS; then lane k forms F of the coefficient at ZIGZAG position k from its column of R' (8 ds_read_b32)
//             and its row of M (8 more registers).  Lane = coefficient in coding order from here on.
//   quantise  q = sign(F) ((|F| + (Q << 18)) div (Q << 19)) = sign(F) (((|F| + (Q << 18)) >> 19) div Q); the dividend is below 4096 and
//             Q below 256, so the division is one multiply by ceil(2^20 / Q) and a shift, exact (checked for every pair on the host).
//             A lane reads its two Q from the DQT segment of the header on the device: the tables the decoder will use.
//   code      __ballot(q != 0) is the block's non-zero mask; a lane's run is a bit scan of the mask below itself; its ZRLs, Huffman word
//             (an LDS table) and magnitude bits are at most 59 bits, lane-local; a wave prefix sum gives its bit offset; the lanes OR
//             their bits into an LDS bit buffer (ds_or_b32), MSB first.  Lane 0 codes the DC difference, lane 63 the EOB.
//   stuff     after each block the buffer's complete bytes are taken 64 at a time: __ballot(byte == 0xFF) and a population count give
//             each byte its place; the (up to 7) bits left over start the next block's buffer.
// WRITE = false stores only the interval's stuffed byte count (4 bytes of scratch per interval); jpeg_scan_kernel turns the counts of a
// frame into byte offsets in place, writes `lengths`, the header, the RST markers and EOI; WRITE = true codes again and stores straight to
// the final offsets.  Every store to the frame is clipped to `capacity`.  No workgroup waits on another.
#include <atomic>

#include "bitpack.hpp"
#include "ycc_code.hpp"

namespace rc {

// ---- the constants of the format (ITU-T T.81) ---------------------------------------------------------------------------------------------
constexpr uint8_t kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3.3: BITS (codes per length 1 .. 16) and HUFFVAL of the typical tables, in DHT order: DC luma, DC chroma, AC luma, AC chroma.
constexpr uint8_t kBitsDcL[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kBitsDcC[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kValsDc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kBitsAcL[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t kValsAcL[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t kBitsAcC[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t kValsAcC[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// M[u][x] = rint(2^14 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2 (tests/test_jpeg_host.py regenerates it from this formula).
constexpr int kJpegM[64] = {5793, 5793,  5793,  5793,  5793,  5793,  5793,  5793,  8035, 6811,  4551,  1598,  -1598, -4551, -6811, -8035,
                            7568, 3135,  -3135, -7568, -7568, -3135, 3135,  7568,  6811, -1598, -8035, -4551, 4551,  8035,  1598,  -6811,
                            5793, -5793, -5793, 5793,  5793,  -5793, -5793, 5793,  4551, -8035, 1598,  6811,  -6811, -1598, 8035,  -4551,
                            3135, -7568, 7568,  -3135, -3135, 7568,  -7568, 3135,  1598, -4551, 6811,  -8035, 8035,  -6811, 4551,  -1598};

// Byte offsets in the header rc_jpeg_header writes: SOI 2, APP0 18, DQT 4 + 65 + 65, SOF0 19, DHT 4 + 29 + 29 + 179 + 179, DRI 6, SOS 14.
constexpr int kJpegHeaderBytes = 2 + 18 + 134 + 19 + 420 + 6 + 14;
constexpr int kJpegQLuma = 2 + 18 + 4 + 1, kJpegQChroma = kJpegQLuma + 65;       // the 64 zigzag entries of table 0 and of table 1
static_assert(kJpegHeaderBytes == 613, "header layout");

// What the kernel keeps in constant memory: M (step 2 of the header), the zigzag order, and the four Huffman tables as (length << 16) | code:
// DC luma at [category], DC chroma at [16 + category], AC luma at [32 + (run << 4 | category)], AC chroma at [288 + ...].
constexpr int kJpegTab = 32 + 2 * 256;
struct JpegConst {
    int m[64];
    uint8_t zigzag[64];
    uint32_t tab[kJpegTab];
};
constexpr void jpeg_huff(uint32_t* t, const uint8_t* bits, const uint8_t* vals) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) t[vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}
constexpr JpegConst jpeg_const() {
    JpegConst c{};
    for (int i = 0; i < 64; ++i) {
        c.m[i] = kJpegM[i];
        c.zigzag[i] = kZigzag[i];
    }
    jpeg_huff(c.tab, kBitsDcL, kValsDc);
    jpeg_huff(c.tab + 16, kBitsDcC, kValsDc);
    jpeg_huff(c.tab + 32, kBitsAcL, kValsAcL);
    jpeg_huff(c.tab + 288, kBitsAcC, kValsAcC);
    return c;
}
__device__ const JpegConst kJpegDev = jpeg_const();

constexpr int kJpegBitWords = 72;       // the bit buffer of one block: at most 7 carried bits + 22 (DC) + 63 x 26 (AC) + 7 pad bits = 1674 bits < 64 words

struct JpegArgs {
    int H, W, h, w;
    int mcols, nmcu, restart, nint;     // MCU columns, MCUs per frame, MCUs per interval, intervals per frame
    int vec;                            // two adjacent source elements at an even column are one aligned access
    long long capacity;
    LumaChroma c;
};

// Two adjacent elements of a row.
template <typename TI>
__device__ __forceinline__ void jpeg_pair(const TI* p, float& a, float& b) {
    if constexpr (sizeof(TI) == 4) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        a = v.x; b = v.y;
    } else {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
        a = lo16<TI>(v); b = hi16<TI>(v);
    }
}

template <typename TI, int SUB, bool WRITE>
__global__ void __launch_bounds__(64) jpeg_interval_kernel(JpegArgs a, const TI* __restrict__ src, const uint8_t* __restrict__ hdr, uint32_t* __restrict__ scratch,
                                                           uint8_t* __restrict__ dst) {
    constexpr int NB = SUB == RC_JPEG_420 ? 6 : 3;
    __shared__ uint32_t tab[kJpegTab];
    __shared__ __attribute__((aligned(16))) int smp[NB * 64];
    __shared__ int rp[64];
    __shared__ uint32_t bb[kJpegBitWords];

    const int lane = threadIdx.x, iv = blockIdx.x, b = blockIdx.y;
    for (int i = lane; i < kJpegTab; i += 64) tab[i] = kJpegDev.tab[i];
    for (int i = lane; i < kJpegBitWords; i += 64) bb[i] = 0u;
    const int nat = kJpegDev.zigzag[lane], ucol = nat & 7;           // this lane's coefficient: row nat >> 3, column nat & 7
    int mr[8], mc[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        mr[x] = kJpegDev.m[(lane & 7) * 8 + x];                      // the row pass: lane (y, u) needs M[u][.]
        mc[x] = kJpegDev.m[(nat >> 3) * 8 + x];                      // the column pass: lane k needs M[v][.]
    }
    const uint32_t q_l = hdr[kJpegQLuma + lane], q_c = hdr[kJpegQChroma + lane];
    const uint32_t rcp_l = ((1u << 20) + q_l - 1u) / q_l, rcp_c = ((1u << 20) + q_c - 1u) / q_c;
    const uint64_t below = (1ull << lane) - 1ull;

    const size_t plane = (size_t)a.H * a.W;
    const TI* frame_src = src + (size_t)b * 3 * plane;
    uint8_t* frame = dst + (size_t)b * (size_t)a.capacity;
    const uint64_t cap = (uint64_t)a.capacity;
    const size_t slot = (size_t)b * a.nint + iv;
    const uint64_t base = WRITE ? (uint64_t)scratch[slot] : 0ull;
    uint32_t out = 0u;                   // stuffed bytes of this interval so far
    int carry = 0;                       // bits of the last incomplete byte, at the top of bb[0]
    int pred0 = 0, pred1 = 0, pred2 = 0;
    const int m_begin = iv * a.restart, m_end = min(m_begin + a.restart, a.nmcu);
    __syncthreads();

    for (int m = m_begin; m < m_end; ++m) {
        const int my = m / a.mcols, mx = m - my * a.mcols;
        // ---- samples ----
        if constexpr (SUB == RC_JPEG_420) {
            const int qy = lane >> 3, qx = lane & 7;
            const int x0 = min(mx * 16 + 2 * qx, a.w - 1), x1 = min(mx * 16 + 2 * qx + 1, a.w - 1);
            const bool pair = a.vec && x1 == x0 + 1;
            float hb[2], hr[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int y = min(my * 16 + 2 * qy + r, a.h - 1);
                const TI* p = frame_src + (size_t)y * a.W;
                float px[3][2];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (pair) {
                        jpeg_pair<TI>(p + c * plane + x0, px[c][0], px[c][1]);
                    } else {
                        px[c][0] = to_f32(p[c * plane + x0]);
                        px[c][1] = to_f32(p[c * plane + x1]);
                    }
                }
                float yv[2], cb[2], cr[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    ycc(a.c, px[0][k], px[1][k], px[2][k], yv[k], cb[k], cr[k]);
                    const int yy = 2 * qy + r, xx = 2 * qx + k;
                    smp[((yy >> 3) * 2 + (xx >> 3)) * 64 + (yy & 7) * 8 + (xx & 7)] = (int)code(yv[k], 255.f, 0.f, 0.f, 255.f) - 128;
                }
                hb[r] = __fadd_rn(cb[0], cb[1]);
                hr[r] = __fadd_rn(cr[0], cr[1]);
            }
            smp[4 * 64 + lane] = (int)code(__fmul_rn(__fadd_rn(hb[0], hb[1]), 0.25f), 255.f, 128.f, 0.f, 255.f) - 128;
            smp[5 * 64 + lane] = (int)code(__fmul_rn(__fadd_rn(hr[0], hr[1]), 0.25f), 255.f, 128.f, 0.f, 255.f) - 128;
        } else {
            const int y = min(my * 8 + (lane >> 3), a.h - 1), x = min(mx * 8 + (lane & 7), a.w - 1);
            const TI* p = frame_src + (size_t)y * a.W + x;
            float yv, cb, cr;
            ycc(a.c, to_f32(p[0]), to_f32(p[plane]), to_f32(p[2 * plane]), yv, cb, cr);
            smp[lane] = (int)code(yv, 255.f, 0.f, 0.f, 255.f) - 128;
            smp[64 + lane] = (int)code(cb, 255.f, 128.f, 0.f, 255.f) - 128;
            smp[128 + lane] = (int)code(cr, 255.f, 128.f, 0.f, 255.f) - 128;
        }
        __syncthreads();

#pragma unroll 1
        for (int blk = 0; blk < NB; ++blk) {
            const int comp = SUB == RC_JPEG_420 ? (blk < 4 ? 0 : blk - 3) : blk;
            // ---- DCT ----
            {
                const int4* row = reinterpret_cast<const int4*>(smp + blk * 64 + (lane & ~7));
                const int4 s0 = row[0], s1 = row[1];
                const int r = mr[0] * s0.x + mr[1] * s0.y + mr[2] * s0.z + mr[3] * s0.w + mr[4] * s1.x + mr[5] * s1.y + mr[6] * s1.z + mr[7] * s1.w;
                rp[lane] = (r + 256) >> 9;
            }
            __syncthreads();
            int f = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) f += mc[y] * rp[y * 8 + ucol];
            // ---- quantise ----
            const uint32_t qq = comp ? q_c : q_l, rcp = comp ? rcp_c : rcp_l;
            const uint32_t aq = ((((uint32_t)(f < 0 ? -f : f) + (qq << 18)) >> 19) * rcp) >> 20;
            const int q = f < 0 ? -(int)aq : (int)aq;
            // ---- code ----
            const int dcq = __shfl(q, 0);
            const int pred = comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2);
            if (comp == 0) pred0 = dcq; else if (comp == 1) pred1 = dcq; else pred2 = dcq;
            const uint64_t nzm = __ballot(q != 0) | 1ull;              // bit 0 stands for the DC position: runs are counted behind it
            const uint32_t* dc = tab + (comp ? 16 : 0);
            const uint32_t* ac = tab + (comp ? 288 : 32);
            uint64_t bits = 0ull;
            int n = 0;
            if (lane == 0) {
                const int d = dcq - pred;
                const int cat = 32 - __clz(d < 0 ? -d : d);
                const uint32_t e = dc[cat];
                bits = ((uint64_t)(e & 0xffffu) << cat) | (uint32_t)((d < 0 ? d - 1 : d) & ((1 << cat) - 1));
                n = (int)(e >> 16) + cat;
            } else if (q != 0) {
                const int run = lane - (63 - __clzll(nzm & below)) - 1;
                const int cat = 32 - __clz(aq);
                const uint32_t e = ac[((run & 15) << 4) | cat];
                bits = ((uint64_t)(e & 0xffffu) << cat) | (uint32_t)((q < 0 ? q - 1 : q) & ((1 << cat) - 1));
                n = (int)(e >> 16) + cat;
                const uint32_t zrl = ac[0xf0];
                for (int z = run >> 4; z > 0; --z) {                    // at most 3, in front of the word
                    bits |= (uint64_t)(zrl & 0xffffu) << n;
                    n += (int)(zrl >> 16);
                }
            } else if (lane == 63) {                                    // coefficient 63 is zero: the block ends with EOB
                const uint32_t e = ac[0];
                bits = e & 0xffffu;
                n = (int)(e >> 16);
            }
            const int incl = wave_scan_incl(n, lane);
            int total = carry + __shfl(incl, 63);
            if (n) bits_or(bb, kJpegBitWords, carry + incl - n, bits, n);
            if (m == m_end - 1 && blk == NB - 1) total = bits_pad_ones(bb, total, lane);      // the interval ends: pad the last byte with 1-bits
            __syncthreads();
            // ---- stuff and store (bitpack.hpp) ----
            carry = bits_flush<WRITE>(bb, kJpegBitWords, total, lane, frame, cap, base, out);
        }
    }
    if (!WRITE && lane == 0) scratch[slot] = out;
}

// One block per frame: the intervals' byte counts -> their byte offsets in the file (in place, saturated at 2^32 - 1: a store beyond
// `capacity` is dropped anyway), the file's length, its header, the marker behind each interval (RSTm, or EOI behind the last).
constexpr int kJpegScanThreads = 256;
__global__ void __launch_bounds__(kJpegScanThreads) jpeg_scan_kernel(int nint, int hdr_bytes, long long capacity, const uint8_t* __restrict__ hdr,
                                                                     uint32_t* __restrict__ scratch, uint8_t* __restrict__ dst, long long* __restrict__ lengths) {
    __shared__ unsigned long long wave_sum[kJpegScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
    uint32_t* cnt = scratch + (size_t)b * nint;
    uint8_t* frame = dst + (size_t)b * (size_t)capacity;
    const unsigned long long cap = (unsigned long long)capacity;
    for (int i = tid; i < hdr_bytes && (unsigned long long)i < cap; i += kJpegScanThreads) frame[i] = hdr[i];
    unsigned long long run = (unsigned long long)hdr_bytes;
    for (int i0 = 0; i0 < nint; i0 += kJpegScanThreads) {
        const int i = i0 + tid;
        const unsigned long long c = i < nint ? (unsigned long long)cnt[i] + 2ull : 0ull;     // the interval and the marker behind it
        unsigned long long v = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        if (lane == 63) wave_sum[wv] = v;
        __syncthreads();
        unsigned long long before = 0ull, chunk = 0ull;
#pragma unroll
        for (int k = 0; k < kJpegScanThreads / 64; ++k) {
            const unsigned long long s = wave_sum[k];
            if (k < wv) before += s;
            chunk += s;
        }
        if (i < nint) {
            const unsigned long long start = run + before + v - c, mark = start + c - 2ull;
            cnt[i] = start > 0xffffffffull ? 0xffffffffu : (uint32_t)start;
            if (mark < cap) frame[mark] = 0xff;
            if (mark + 1ull < cap) frame[mark + 1ull] = i == nint - 1 ? 0xd9 : (uint8_t)(0xd0 + (i & 7));
        }
        run += chunk;
        __syncthreads();
    }
    if (tid == 0) lengths[b] = (long long)run;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
static std::atomic<int> g_jpeg_passes{7};       // rc_debug_jpeg_passes: measurement only

static const char* jpeg_plan(const rc_jpeg_desc* d, int h, int w, rc_jpeg_plan_info* p) {
    if (!d) return "null description";
    if (d->quality < 1 || d->quality > 100) return "quality must be 1 .. 100";
    if (d->subsampling != RC_JPEG_420 && d->subsampling != RC_JPEG_444) return "unknown subsampling";
    if (d->restart < 1 || d->restart > 65535) return "restart must be 1 .. 65535 MCUs";
    for (int r : d->reserved)
        if (r) return "reserved fields must be zero";
    if (h < 1 || w < 1 || h > 65535 || w > 65535) return "a JPEG frame has 1 .. 65535 rows and columns";
    const long long mcu = d->subsampling == RC_JPEG_420 ? 16 : 8;
    p->header_bytes = kJpegHeaderBytes;
    p->mcu_cols = (w + mcu - 1) / mcu;
    p->mcu_rows = (h + mcu - 1) / mcu;
    p->intervals = (p->mcu_cols * p->mcu_rows + d->restart - 1) / d->restart;
    const long long area = p->mcu_cols * mcu * p->mcu_rows * mcu;
    p->capacity = p->header_bytes + (d->subsampling == RC_JPEG_420 ? 3 * area / 2 : 3 * area) + 2 * p->intervals + 2;
    p->scratch_bytes = 4 * p->intervals;
    return nullptr;
}

static void jpeg_tables(int quality, uint8_t* luma, uint8_t* chroma) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        const int l = (kBaseLuma[i] * s + 50) / 100, c = (kBaseChroma[i] * s + 50) / 100;
        luma[i] = (uint8_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
        chroma[i] = (uint8_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_jpeg_desc_size(void) { return sizeof(rc_jpeg_desc); }

int rc_debug_jpeg_passes(int mask) {
    g_jpeg_passes.store(mask & 7, std::memory_order_relaxed);
    return RC_OK;
}

int rc_jpeg_tables(int quality, uint8_t* luma, uint8_t* chroma) {
    RC_REQUIRE(luma && chroma, "rc_jpeg_tables: null pointer");
    RC_REQUIRE(quality >= 1 && quality <= 100, "rc_jpeg_tables: quality must be 1 .. 100");
    jpeg_tables(quality, luma, chroma);
    return RC_OK;
}

int rc_jpeg_plan(const rc_jpeg_desc* desc, int h, int w, rc_jpeg_plan_info* plan) {
    RC_REQUIRE(plan, "rc_jpeg_plan: null pointer");
    const char* err = jpeg_plan(desc, h, w, plan);
    if (err) return fail(RC_ERR_INVALID, std::string("rc_jpeg_plan: ") + err);
    return RC_OK;
}

int rc_jpeg_header(const rc_jpeg_desc* desc, int h, int w, uint8_t* buf, size_t cap, size_t* len) {
    RC_REQUIRE(buf && len, "rc_jpeg_header: null pointer");
    rc_jpeg_plan_info p;
    const char* err = jpeg_plan(desc, h, w, &p);
    if (err) return fail(RC_ERR_INVALID, std::string("rc_jpeg_header: ") + err);
    RC_REQUIRE(cap >= (size_t)kJpegHeaderBytes, "rc_jpeg_header: the buffer is shorter than the header (rc_jpeg_plan's header_bytes)");
    uint8_t* o = buf;
    auto put = [&](int v) { *o++ = (uint8_t)v; };
    auto put16 = [&](int v) { put(v >> 8); put(v & 0xff); };
    put16(0xffd8);                                                                   // SOI
    put16(0xffe0); put16(16);                                                        // APP0: JFIF 1.01, no units, aspect 1:1, no thumbnail
    for (int c : {0x4a, 0x46, 0x49, 0x46, 0, 1, 1, 0}) put(c);                       // "JFIF\0", version 1.01, units 0
    put16(1); put16(1); put(0); put(0);
    uint8_t ql[64], qc[64];
    jpeg_tables(desc->quality, ql, qc);
    put16(0xffdb); put16(2 + 65 + 65);                                               // DQT: tables 0 and 1, 8 bit, zigzag order
    put(0x00);
    for (int k = 0; k < 64; ++k) put(ql[kZigzag[k]]);
    put(0x01);
    for (int k = 0; k < 64; ++k) put(qc[kZigzag[k]]);
    put16(0xffc0); put16(17); put(8); put16(h); put16(w); put(3);                    // SOF0
    put(1); put(desc->subsampling == RC_JPEG_420 ? 0x22 : 0x11); put(0);
    put(2); put(0x11); put(1);
    put(3); put(0x11); put(1);
    put16(0xffc4); put16(2 + 2 * (17 + 12) + 2 * (17 + 162));                        // DHT: the four K.3.3 tables
    auto table = [&](int tc_th, const uint8_t* bits, const uint8_t* vals, int n) {
        put(tc_th);
        for (int i = 0; i < 16; ++i) put(bits[i]);
        for (int i = 0; i < n; ++i) put(vals[i]);
    };
    table(0x00, kBitsDcL, kValsDc, 12);
    table(0x01, kBitsDcC, kValsDc, 12);
    table(0x10, kBitsAcL, kValsAcL, 162);
    table(0x11, kBitsAcC, kValsAcC, 162);
    put16(0xffdd); put16(4); put16(desc->restart);                                   // DRI
    put16(0xffda); put16(12); put(3);                                                // SOS
    put(1); put(0x00); put(2); put(0x11); put(3); put(0x11);
    put(0); put(63); put(0);
    if (o - buf != kJpegHeaderBytes) return fail(RC_ERR_INVALID, "rc_jpeg_header: internal: header layout");
    *len = (size_t)kJpegHeaderBytes;
    return RC_OK;
}

int rc_jpeg_encode(const void* d_src, int src_dtype, const rc_jpeg_desc* desc, const void* d_header, void* d_scratch, void* d_dst, void* d_lengths,
                   int batch, int H, int W, int h, int w, long long capacity, void* stream) {
    RC_REQUIRE(d_src && desc && d_header && d_scratch && d_dst && d_lengths, "rc_jpeg_encode: null pointer");
    RgbSide src;
    if (int e = rgb_source("rc_jpeg_encode", d_src, src_dtype, batch, H, W, h, w, &src)) return e;
    rc_jpeg_plan_info p;
    const char* err = jpeg_plan(desc, h, w, &p);
    if (err) return fail(RC_ERR_INVALID, std::string("rc_jpeg_encode: ") + err);
    RC_REQUIRE(capacity >= 1, "rc_jpeg_encode: capacity must be at least one byte");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_scratch) % 4 == 0 && reinterpret_cast<uintptr_t>(d_lengths) % 8 == 0, "rc_jpeg_encode: scratch or lengths misaligned");
    RC_REQUIRE(batch <= 65535, "rc_jpeg_encode: more than 65535 frames");
    RC_REQUIRE(p.intervals <= 0x7fffffffLL && p.mcu_cols * p.mcu_rows <= 0x7fffffffLL - 65535, "rc_jpeg_encode: too many restart intervals");

    JpegArgs a;
    a.H = H; a.W = W; a.h = h; a.w = w;
    a.mcols = (int)p.mcu_cols; a.nmcu = (int)(p.mcu_cols * p.mcu_rows); a.restart = desc->restart; a.nint = (int)p.intervals;
    a.vec = reinterpret_cast<uintptr_t>(d_src) % (2 * src.esize) == 0 && W % 2 == 0;
    a.capacity = capacity;
    a.c = rgb_coef(RC_MATRIX_BT601);
    const dim3 grid(a.nint, batch);
    hipStream_t s = as_stream(stream);
    by_source(src_dtype, [&](auto ti) {
        typedef typename decltype(ti)::type TI;
        auto pass = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(64), 0, s, a, static_cast<const TI*>(d_src), static_cast<const uint8_t*>(d_header), static_cast<uint32_t*>(d_scratch),
                               static_cast<uint8_t*>(d_dst));
        };
        const bool s420 = desc->subsampling == RC_JPEG_420;
        const int passes = g_jpeg_passes.load(std::memory_order_relaxed);
        if (passes & 1) pass(s420 ? jpeg_interval_kernel<TI, RC_JPEG_420, false> : jpeg_interval_kernel<TI, RC_JPEG_444, false>);
        if (passes & 2)
            hipLaunchKernelGGL(jpeg_scan_kernel, dim3(batch), dim3(kJpegScanThreads), 0, s, a.nint, kJpegHeaderBytes, capacity, static_cast<const uint8_t*>(d_header),
                               static_cast<uint32_t*>(d_scratch), static_cast<uint8_t*>(d_dst), static_cast<long long*>(d_lengths));
        if (passes & 4) pass(s420 ? jpeg_interval_kernel<TI, RC_JPEG_420, true> : jpeg_interval_kernel<TI, RC_JPEG_444, true>);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
