// Defective-pixel correction on the mosaic (include/realcam_hip.h, rc_raw_defects): the sensor frame as rc_raw_ingest_fmt reads it (any
// storage, padded lines) -> the corrected, unpacked mosaic (B, 2h, 2w) and, optionally, (B, 3) counts.  The one stage of the family that
// is a stencil: every sample looks at the eight nearest samples of its own colour, two rows / columns away.
//
// raw_defects_kernel: grid (pairs of strips, bands of 64 rows, frames), four waves per block.
//   lane map   a STRIP is 248 columns.  Lane l of a wave holds the 4 consecutive samples 248 s - 4 + 4 l .. + 3 of a row: lanes 1 .. 62
//              correct and store theirs, lanes 0 and 63 only load (the strip's halo: 8 of 256 columns are read twice, out of L2).  Every
//              lane's first column is a multiple of 4: one 4 / 8 / 16-byte load per lane and row for u8 / 16-bit / fp32 samples, 5 bytes of
//              a RAW10 line, 6 of a RAW12 line (whole dwords, as the ingest reads them); ragged frames (a base or pitch that is no multiple
//              of 4 samples, the last two columns of a width that is 2 mod 4) go sample by sample.
//   columns    x - 2 and x + 2 are the lane's own registers or the neighbouring lane's (six lane shifts per row: four values, and the
//              four good / bad bits to either side), never a reload.
//   rows       waves 0, 2 of a block walk the even rows of the band DOWNWARDS, waves 1, 3 the odd rows (waves 0, 1: the block's first
//              strip; 2, 3: its second): a wave keeps rows y - 2, y, y + 2 (8 values + 8 bits each) and loads one new row per step -- the
//              raw bytes of the row after it are already in flight.  Two rows above and below a band are read twice (4 / 64, out of L2).
//   map        the lane's 4 bits are one nibble of one dword (8 lanes share a dword: one request); a position outside the frame counts as
//              mapped, so the frame's edges need no case of their own.
//   counts     per lane in registers, per wave by lane exchange, per block in LDS, then one 64-bit atomic per block and counter.
// No division per sample, no LDS tile, no scratch.  The arithmetic is step for step the header's.
#include "common.hpp"

#include <cmath>

namespace rc {

constexpr int kDfPx = 4, kDfWaves = 4, kDfThreads = 64 * kDfWaves;
constexpr int kDfSpan = 62 * kDfPx;             // columns a wave corrects
constexpr int kDfStrips = kDfWaves / 2;         // strips per block
constexpr int kDfRows = 64;                     // rows per block

enum { kDfElem = 0, kDfMipi10 = 1, kDfMipi12 = 2 };     // how a mosaic row is stored (raw_format.hip's three forms)

struct DefectArgs {
    const uint8_t* src;        // mosaic row r of frame b starts at src + (b * H + r) * line_bytes
    const uint32_t* map;       // or null
    uint8_t* dst;
    unsigned long long* counts;    // or null
    int H, W;                  // the mosaic's rows and columns (2h, 2w)
    int line_bytes, map_pitch_dw, dst_pitch;
    int vec_in, vec_out;       // every lane's 4 samples start on a 4-sample boundary of the source / the destination
    int hot, cold;
    float hot_abs, hot_rel, cold_abs, cold_rel;
    float black[4];            // CFA-position order
};

struct DfRaw { uint32_t d[4]; uint32_t map; };          // a row's bytes as loaded (or, sample by sample, its 4 values) and its map dword
struct DfRow { float v[8]; uint32_t bad; };             // columns x0 - 2 .. x0 + 5 and, per column, "mapped or outside the frame"

// raw_format.hip's load_window: bytes [s, s + nb) (nb <= 6) of a 4-byte aligned buffer as a little-endian 64-bit window, whole dwords only
__device__ __forceinline__ void df_window(const uint8_t* base, size_t s, int nb, uint32_t* out) {
    const uint32_t* d = reinterpret_cast<const uint32_t*>(base + (s & ~(size_t)3));
    const int sh = (int)(s & 3), ndw = (sh + nb + 3) >> 2;
    const uint32_t w0 = d[0];
    const uint32_t w1 = ndw > 1 ? d[1] : 0u;
    const uint32_t w2 = ndw > 2 ? d[2] : 0u;
    const uint64_t lo = ((uint64_t)w1 << 32) | w0;
    const uint64_t g = sh ? (lo >> (8 * sh)) | ((uint64_t)w2 << (64 - 8 * sh)) : lo;
    out[0] = (uint32_t)g;
    out[1] = (uint32_t)(g >> 32);
}

// Row y of the frame at columns x0 .. x0 + 3 (n of them inside the frame; `full`: n == 4 and the lane may use one vector load).  A row
// outside the frame, or a lane with n = 0, reads nothing.
template <int ST, typename TI>
__device__ __forceinline__ DfRaw df_load(const DefectArgs& a, size_t frame_row, int y, int x0, int n, bool full) {
    DfRaw r = {{0u, 0u, 0u, 0u}, 0u};
    if (y < 0 || y >= a.H || n <= 0) return r;
    const size_t off = (frame_row + (size_t)y) * (size_t)a.line_bytes;
    if constexpr (ST == kDfElem) {
        const TI* p = reinterpret_cast<const TI*>(a.src + off) + x0;
        if (full) {
            if constexpr (sizeof(TI) == 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(p);
                r.d[0] = q.x; r.d[1] = q.y; r.d[2] = q.z; r.d[3] = q.w;
            } else if constexpr (sizeof(TI) == 2) {
                const uint2 q = *reinterpret_cast<const uint2*>(p);
                r.d[0] = q.x; r.d[1] = q.y;
            } else {
                r.d[0] = *reinterpret_cast<const uint32_t*>(p);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kDfPx; ++k) r.d[k] = k < n ? __float_as_uint(to_f32(p[k])) : 0u;
        }
    } else if constexpr (ST == kDfMipi10) {                     // W % 4 == 0: always a whole 5-byte group
        df_window(a.src, off + (size_t)(x0 >> 2) * 5, 5, r.d);
    } else {                                                    // two 3-byte groups, or one at the end of a row of 2 mod 4 samples
        df_window(a.src, off + (size_t)(x0 >> 1) * 3, n == 4 ? 6 : 3, r.d);
    }
    if (a.map) r.map = a.map[(size_t)y * (size_t)a.map_pitch_dw + (size_t)(x0 >> 5)];
    return r;
}

template <int ST, typename TI>
__device__ __forceinline__ void df_decode(const DfRaw& r, int n, bool full, float* v) {
    if constexpr (ST == kDfElem) {
        if (!full) {
#pragma unroll
            for (int k = 0; k < kDfPx; ++k) v[k] = __uint_as_float(r.d[k]);
        } else if constexpr (__is_same(TI, float)) {
#pragma unroll
            for (int k = 0; k < kDfPx; ++k) v[k] = __uint_as_float(r.d[k]);
        } else if constexpr (__is_same(TI, bf16_t)) {
#pragma unroll
            for (int j = 0; j < 2; ++j) { v[2 * j] = __uint_as_float(r.d[j] << 16); v[2 * j + 1] = __uint_as_float(r.d[j] & 0xffff0000u); }
        } else if constexpr (__is_same(TI, f16_t)) {
#pragma unroll
            for (int j = 0; j < 2; ++j) { v[2 * j] = Vec16<f16_t>::lo(r.d[j]); v[2 * j + 1] = Vec16<f16_t>::hi(r.d[j]); }
        } else if constexpr (sizeof(TI) == 2) {
#pragma unroll
            for (int j = 0; j < 2; ++j) { v[2 * j] = (float)(r.d[j] & 0xffffu); v[2 * j + 1] = (float)(r.d[j] >> 16); }
        } else {
#pragma unroll
            for (int k = 0; k < kDfPx; ++k) v[k] = (float)((r.d[0] >> (8 * k)) & 0xffu);
        }
    } else if constexpr (ST == kDfMipi10) {
        const uint32_t lsb = r.d[1] & 0xffu;
#pragma unroll
        for (int k = 0; k < kDfPx; ++k) v[k] = (float)((((r.d[0] >> (8 * k)) & 0xffu) << 2) | ((lsb >> (2 * k)) & 3u));
    } else {
        const uint64_t g = ((uint64_t)r.d[1] << 32) | r.d[0];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t b0 = (uint32_t)(g >> (24 * j)) & 0xffu, b1 = (uint32_t)(g >> (24 * j + 8)) & 0xffu, b2 = (uint32_t)(g >> (24 * j + 16)) & 0xffu;
            const bool live = j == 0 || n == 4;
            v[2 * j] = live ? (float)((b0 << 4) | (b2 & 15u)) : 0.f;
            v[2 * j + 1] = live ? (float)((b1 << 4) | (b2 >> 4)) : 0.f;
        }
    }
}

// The lane's row with its two columns to either side.  Called by the whole wave: the lane shifts need every lane.  Lane 0's left and lane
// 63's right columns are its own values: those lanes store nothing.
template <int ST, typename TI>
__device__ __forceinline__ DfRow df_row(const DefectArgs& a, const DfRaw& raw, int y, int x0, int n, bool full) {
    float v[kDfPx];
    df_decode<ST, TI>(raw, n, full, v);
    const uint32_t inside = n >= 4 ? 15u : n > 0 ? 3u : 0u;                       // W is even and x0 a multiple of 4: n is 0, 2 or 4
    const uint32_t nib = (y >= 0 && y < a.H) ? (((raw.map >> (x0 & 31)) & inside) | (15u & ~inside)) : 15u;
    DfRow r;
#pragma unroll
    for (int k = 0; k < kDfPx; ++k) r.v[2 + k] = v[k];
    r.v[0] = __shfl_up(v[2], 1); r.v[1] = __shfl_up(v[3], 1);
    r.v[6] = __shfl_down(v[0], 1); r.v[7] = __shfl_down(v[1], 1);
    const uint32_t nl = __shfl_up(nib, 1), nr = __shfl_down(nib, 1);
    r.bad = ((nl >> 2) & 3u) | (nib << 2) | ((nr & 3u) << 6);
    return r;
}

struct DfParams { int hot, cold; float hot_abs, hot_rel, cold_abs, cold_rel; };

// Sample k of the lane in row `cu` (steps 1 and 2 of the header); n[0..2] count what was replaced.
template <int K>
__device__ __forceinline__ float df_sample(const DfRow& up, const DfRow& cu, const DfRow& dn, const DfParams& p, float black, uint32_t* n) {
    const float v = cu.v[K + 2];
    // the ring in the order W, E, N, S, NW, NE, SW, SE
    const float r[8] = {cu.v[K], cu.v[K + 4], up.v[K + 2], dn.v[K + 2], up.v[K], up.v[K + 4], dn.v[K], dn.v[K + 4]};
    const uint32_t bad = ((cu.bad >> K) & 1u) | (((cu.bad >> (K + 4)) & 1u) << 1) | (((up.bad >> (K + 2)) & 1u) << 2) | (((dn.bad >> (K + 2)) & 1u) << 3) |
                         (((up.bad >> K) & 1u) << 4) | (((up.bad >> (K + 4)) & 1u) << 5) | (((dn.bad >> K) & 1u) << 6) | (((dn.bad >> (K + 4)) & 1u) << 7);
    const uint32_t good = ~bad & 0xffu;
    float out = v;
    if ((cu.bad >> (K + 2)) & 1u) {
        constexpr int pa[4] = {0, 2, 4, 5}, pb[4] = {1, 3, 7, 6};                // H, V, D1, D2
        bool have = false;
        float best = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool whole = ((good >> pa[i]) & (good >> pb[i]) & 1u) != 0u;
            const float d = fabsf(__fsub_rn(r[pa[i]], r[pb[i]]));
            if (whole && (!have || d < best)) {
                best = d;
                out = __fmul_rn(__fadd_rn(r[pa[i]], r[pb[i]]), 0.5f);
                have = true;
            }
        }
        if (!have) {
#pragma unroll
            for (int i = 7; i >= 0; --i)
                if ((good >> i) & 1u) { out = r[i]; have = true; }
        }
        n[0] += have ? 1u : 0u;
    } else if (good) {
        float hi = -INFINITY, lo = INFINITY;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const bool g = ((good >> i) & 1u) != 0u;
            hi = fmaxf(hi, g ? r[i] : -INFINITY);
            lo = fminf(lo, g ? r[i] : INFINITY);
        }
        bool done = false;
        if (p.hot) {
            const float t = __fadd_rn(p.hot_abs, __fmul_rn(p.hot_rel, fmaxf(__fsub_rn(hi, black), 0.f)));
            if (__fsub_rn(v, hi) > t) { out = hi; done = true; n[1] += 1u; }
        }
        if (!done && p.cold) {
            const float t = __fadd_rn(p.cold_abs, __fmul_rn(p.cold_rel, fmaxf(__fsub_rn(lo, black), 0.f)));
            if (__fsub_rn(lo, v) > t) { out = lo; n[2] += 1u; }
        }
    }
    return out;
}

template <typename TO>
__device__ __forceinline__ uint32_t df_bits(float v) {                             // step 3, as the low bits of a word
    if constexpr (__is_same(TO, uint16_t)) return (uint32_t)rintf(v);              // half to even; 0 .. 65535 by construction
    else if constexpr (__is_same(TO, float)) return __float_as_uint(v);
    else return (uint32_t)__builtin_bit_cast(uint16_t, from_f32<TO>(v));           // round to nearest even
}

template <typename TO>
__device__ __forceinline__ void df_store(TO* o, const float* v, int n, bool full) {
    if (full) {
        if constexpr (sizeof(TO) == 4) {
            *reinterpret_cast<uint4*>(o) = make_uint4(df_bits<TO>(v[0]), df_bits<TO>(v[1]), df_bits<TO>(v[2]), df_bits<TO>(v[3]));
        } else {
            *reinterpret_cast<uint2*>(o) = make_uint2(df_bits<TO>(v[0]) | (df_bits<TO>(v[1]) << 16), df_bits<TO>(v[2]) | (df_bits<TO>(v[3]) << 16));
        }
    } else {
#pragma unroll
        for (int k = 0; k < kDfPx; ++k) {
            if (k < n) {
                if constexpr (sizeof(TO) == 4) reinterpret_cast<uint32_t*>(o)[k] = df_bits<TO>(v[k]);
                else reinterpret_cast<uint16_t*>(o)[k] = (uint16_t)df_bits<TO>(v[k]);
            }
        }
    }
}

template <int ST, typename TI, typename TO>
__global__ void __launch_bounds__(kDfThreads) raw_defects_kernel(DefectArgs a) {
    __shared__ uint32_t total[3];                                                  // at most 256 x 64 x 4 per block
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid < 3) total[tid] = 0u;
    __syncthreads();
    const int par = wv & 1, strip = blockIdx.x * kDfStrips + (wv >> 1), frame = blockIdx.z;
    const int x0 = strip * kDfSpan + (lane - 1) * kDfPx;
    const int n = x0 < 0 ? 0 : min(max(a.W - x0, 0), kDfPx);                       // the lane's columns inside the frame: 0, 2 or 4
    const bool writer = lane >= 1 && lane <= 62 && n > 0;
    const bool full_in = n == kDfPx && a.vec_in, full_out = n == kDfPx && a.vec_out;
    const int r0 = blockIdx.y * kDfRows, r1 = min(r0 + kDfRows, a.H);
    const size_t frame_row = (size_t)frame * (size_t)a.H;
    const DfParams p = {a.hot, a.cold, a.hot_abs, a.hot_rel, a.cold_abs, a.cold_rel};
    const float black0 = a.black[2 * par], black1 = a.black[2 * par + 1];          // r0 is even: y & 1 = par; x0 % 4 = 0: x & 1 = k & 1
    uint32_t cnt[3] = {0u, 0u, 0u};
    if (strip * kDfSpan < a.W) {                                                   // wave-uniform
        int y = r0 + par;
        DfRow up = df_row<ST, TI>(a, df_load<ST, TI>(a, frame_row, y - 2, x0, n, full_in), y - 2, x0, n, full_in);
        DfRow cu = df_row<ST, TI>(a, df_load<ST, TI>(a, frame_row, y, x0, n, full_in), y, x0, n, full_in);
        DfRaw ahead = df_load<ST, TI>(a, frame_row, y + 2, x0, n, full_in);
        for (; y < r1; y += 2) {
            const DfRaw raw = ahead;
            if (y + 2 < r1) ahead = df_load<ST, TI>(a, frame_row, y + 4, x0, n, full_in);      // in flight while this row is worked on
            const DfRow dn = df_row<ST, TI>(a, raw, y + 2, x0, n, full_in);
            if (writer) {
                float o[kDfPx];
                o[0] = df_sample<0>(up, cu, dn, p, black0, cnt);
                o[1] = df_sample<1>(up, cu, dn, p, black1, cnt);
                if (n == kDfPx) {
                    o[2] = df_sample<2>(up, cu, dn, p, black0, cnt);
                    o[3] = df_sample<3>(up, cu, dn, p, black1, cnt);
                } else {
                    o[2] = o[3] = 0.f;
                }
                TO* dst = reinterpret_cast<TO*>(a.dst + (frame_row + (size_t)y) * (size_t)a.dst_pitch) + x0;
                df_store<TO>(dst, o, n, full_out);
            }
            up = cu;
            cu = dn;
        }
    }
    if (a.counts) {                                                                // block-uniform
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t s = cnt[c];
#pragma unroll
            for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
            if (lane == 0 && s) atomicAdd(&total[c], s);
        }
        __syncthreads();
        if (tid < 3 && total[tid]) atomicAdd(&a.counts[(size_t)frame * 3 + tid], (unsigned long long)total[tid]);
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_defect_desc_size(void) { return sizeof(rc_defect_desc); }

int rc_raw_defects(const void* d_src, const rc_raw_format* fmt, const rc_defect_desc* desc, const void* d_map, int map_pitch_bytes,
                   void* d_dst, int dst_pitch_bytes, long long* d_counts, int batch, int h, int w, void* stream) {
    RC_REQUIRE(d_src && fmt && desc && d_dst, "rc_raw_defects: null pointer");
    RC_REQUIRE(batch >= 1 && batch <= 65535 && h >= 1 && w >= 1 && h <= (1 << 20) && w <= (1 << 24), "rc_raw_defects: bad shape (empty, more than 65535 frames, or too large)");
    const int st = fmt->storage;
    RC_REQUIRE(st >= RC_RAW_F32 && st <= RC_RAW_MIPI12, "rc_raw_defects: unknown storage");
    RC_REQUIRE(fmt->cfa >= RC_CFA_RGGB && fmt->cfa <= RC_CFA_GBRG, "rc_raw_defects: unknown cfa");
    RC_REQUIRE(fmt->reserved[0] == 0 && fmt->reserved[1] == 0 && fmt->reserved[2] == 0 && fmt->reserved[3] == 0,
               "rc_raw_defects: the format's reserved fields must be zero");
    RC_REQUIRE(desc->reserved[0] == 0 && desc->reserved[1] == 0 && desc->reserved[2] == 0, "rc_raw_defects: reserved fields must be zero");
    RC_REQUIRE((desc->flags & ~(RC_DEFECT_HOT | RC_DEFECT_COLD)) == 0, "rc_raw_defects: unknown flags");
    RC_REQUIRE(desc->flags != 0 || d_map, "rc_raw_defects: nothing enabled (no map, no hot test, no cold test)");
    const float thr[4] = {desc->hot_abs, desc->hot_rel, desc->cold_abs, desc->cold_rel};
    for (int k = 0; k < 4; ++k) RC_REQUIRE(std::isfinite(thr[k]) && thr[k] >= 0.f, "rc_raw_defects: thresholds must be finite and >= 0");
    RC_REQUIRE(fmt->width == 0 || fmt->width == 2 * w, "rc_raw_defects: width must be 0 or the mosaic width 2w");
    const bool mipi = st == RC_RAW_MIPI10 || st == RC_RAW_MIPI12;
    RC_REQUIRE(st != RC_RAW_MIPI10 || (2 * w) % 4 == 0, "rc_raw_defects: RAW10 needs a mosaic width 2w divisible by 4");
    const int esize = st == RC_RAW_F32 ? 4 : st == RC_RAW_U8 ? 1 : 2;
    const long long need = st == RC_RAW_MIPI10 ? 2LL * w * 10 / 8 : st == RC_RAW_MIPI12 ? 2LL * w * 12 / 8 : 2LL * w * esize;
    const long long lb = fmt->line_bytes ? fmt->line_bytes : need;
    RC_REQUIRE(lb >= need && lb <= 0x7fffffffLL, "rc_raw_defects: line_bytes shorter than one mosaic row");
    RC_REQUIRE(mipi || lb % esize == 0, "rc_raw_defects: line_bytes must be a multiple of the sample size");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_src) % (mipi ? 4 : esize) == 0, "rc_raw_defects: source misaligned (MIPI: 4 bytes, else one sample)");
    const int osize = st == RC_RAW_F32 ? 4 : 2;
    const long long dp = dst_pitch_bytes ? dst_pitch_bytes : 2LL * w * osize;
    RC_REQUIRE(dp >= 2LL * w * osize && dp <= 0x7fffffffLL && dp % osize == 0, "rc_raw_defects: dst pitch shorter than one row or no multiple of the sample size");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_dst) % osize == 0, "rc_raw_defects: dst misaligned");
    if (d_map) {
        RC_REQUIRE(map_pitch_bytes % 4 == 0 && map_pitch_bytes >= 4 * ceil_div(2 * w, 32), "rc_raw_defects: the map pitch must be a multiple of 4 and hold 2w bits");
        RC_REQUIRE(reinterpret_cast<uintptr_t>(d_map) % 4 == 0, "rc_raw_defects: the map must be 4-byte aligned");
    }
    RC_REQUIRE(!d_counts || reinterpret_cast<uintptr_t>(d_counts) % 8 == 0, "rc_raw_defects: counts must be 8-byte aligned");

    DefectArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.map = static_cast<const uint32_t*>(d_map);
    a.dst = static_cast<uint8_t*>(d_dst);
    a.counts = reinterpret_cast<unsigned long long*>(d_counts);
    a.H = 2 * h; a.W = 2 * w;
    a.line_bytes = (int)lb; a.map_pitch_dw = d_map ? map_pitch_bytes / 4 : 0; a.dst_pitch = (int)dp;
    a.vec_in = !mipi && reinterpret_cast<uintptr_t>(d_src) % (kDfPx * esize) == 0 && lb % (kDfPx * esize) == 0;
    a.vec_out = reinterpret_cast<uintptr_t>(d_dst) % (kDfPx * osize) == 0 && dp % (kDfPx * osize) == 0;
    a.hot = (desc->flags & RC_DEFECT_HOT) != 0; a.cold = (desc->flags & RC_DEFECT_COLD) != 0;
    a.hot_abs = desc->hot_abs; a.hot_rel = desc->hot_rel; a.cold_abs = desc->cold_abs; a.cold_rel = desc->cold_rel;
    for (int k = 0; k < 4; ++k) a.black[k] = fmt->black[k];
    const hipStream_t s = as_stream(stream);
    if (d_counts) RC_HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)batch * 3 * sizeof(long long), s));
    const dim3 grid((unsigned)ceil_div(ceil_div(a.W, kDfSpan), kDfStrips), (unsigned)ceil_div(a.H, kDfRows), (unsigned)batch), block(kDfThreads);
#define LAUNCH(ST, TI, TO) hipLaunchKernelGGL((raw_defects_kernel<ST, TI, TO>), grid, block, 0, s, a)
    switch (st) {
        case RC_RAW_F32: LAUNCH(kDfElem, float, float); break;
        case RC_RAW_BF16: LAUNCH(kDfElem, bf16_t, bf16_t); break;
        case RC_RAW_F16: LAUNCH(kDfElem, f16_t, f16_t); break;
        case RC_RAW_U16: LAUNCH(kDfElem, uint16_t, uint16_t); break;
        case RC_RAW_U8: LAUNCH(kDfElem, uint8_t, uint16_t); break;
        case RC_RAW_MIPI10: LAUNCH(kDfMipi10, uint8_t, uint16_t); break;
        default: LAUNCH(kDfMipi12, uint8_t, uint16_t); break;
    }
#undef LAUNCH
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
