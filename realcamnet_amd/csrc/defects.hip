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
#include "raw_row.hpp"

#include <cmath>

namespace rc {

constexpr int kDfPx = 4, kDfWaves = 4, kDfThreads = 64 * kDfWaves;
constexpr int kDfSpan = 62 * kDfPx;             // columns a wave corrects
constexpr int kDfStrips = kDfWaves / 2;         // strips per block
constexpr int kDfRows = 64;                     // rows per block
static_assert(kDfPx == kRowPx, "a lane holds the row reader's 4 samples");

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

struct DfRaw { RowRaw row; uint32_t map; };             // a row's 4 samples as loaded and its map dword
struct DfRow { float v[8]; uint32_t bad; };             // columns x0 - 2 .. x0 + 5 and, per column, "mapped or outside the frame"

// Row y of the frame at columns x0 .. x0 + 3 (n of them inside the frame; `full`: n == 4 and the lane may use one vector load).  A row
// outside the frame, or a lane with n = 0, reads nothing.
template <int ST, typename TI>
__device__ __forceinline__ DfRaw df_load(const DefectArgs& a, size_t frame_row, int y, int x0, int n, bool full) {
    DfRaw r = {{{0u, 0u, 0u, 0u}}, 0u};
    if (y < 0 || y >= a.H || n <= 0) return r;
    r.row = row_load<ST, TI>(a.src, (frame_row + (size_t)y) * (size_t)a.line_bytes, x0, n, full);
    if (a.map) r.map = a.map[(size_t)y * (size_t)a.map_pitch_dw + (size_t)(x0 >> 5)];
    return r;
}

// The lane's row with its two columns to either side.  Called by the whole wave: the lane shifts need every lane.  Lane 0's left and lane
// 63's right columns are its own values: those lanes store nothing.
template <int ST, typename TI>
__device__ __forceinline__ DfRow df_row(const DefectArgs& a, const DfRaw& raw, int y, int x0, int n, bool full) {
    float v[kDfPx];
    row_decode<ST, TI>(raw.row, n, full, v);
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
                row_store<TO>(dst, o, n, full_out);
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
    if (const int e = raw_frames("rc_raw_defects", batch, h, w)) return e;
    RawSource rs;
    if (const int e = raw_source("rc_raw_defects", d_src, fmt, w, &rs)) return e;
    RC_REQUIRE(all_zero(desc->reserved), "rc_raw_defects: reserved fields must be zero");
    RC_REQUIRE((desc->flags & ~(RC_DEFECT_HOT | RC_DEFECT_COLD)) == 0, "rc_raw_defects: unknown flags");
    RC_REQUIRE(desc->flags != 0 || d_map, "rc_raw_defects: nothing enabled (no map, no hot test, no cold test)");
    const float thr[4] = {desc->hot_abs, desc->hot_rel, desc->cold_abs, desc->cold_rel};
    for (int k = 0; k < 4; ++k) RC_REQUIRE(std::isfinite(thr[k]) && thr[k] >= 0.f, "rc_raw_defects: thresholds must be finite and >= 0");
    long long dp;
    if (const int e = raw_pitch("rc_raw_defects", "dst", d_dst, dst_pitch_bytes, 2LL * w * rs.usize, rs.usize, &dp)) return e;
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
    a.line_bytes = (int)rs.line_bytes; a.map_pitch_dw = d_map ? map_pitch_bytes / 4 : 0; a.dst_pitch = (int)dp;
    a.vec_in = rs.vec; a.vec_out = raw_vec(d_dst, dp, rs.usize);
    a.hot = (desc->flags & RC_DEFECT_HOT) != 0; a.cold = (desc->flags & RC_DEFECT_COLD) != 0;
    a.hot_abs = desc->hot_abs; a.hot_rel = desc->hot_rel; a.cold_abs = desc->cold_abs; a.cold_rel = desc->cold_rel;
    for (int k = 0; k < 4; ++k) a.black[k] = fmt->black[k];
    const hipStream_t s = as_stream(stream);
    if (d_counts) RC_HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)batch * 3 * sizeof(long long), s));
    const dim3 grid((unsigned)ceil_div(ceil_div(a.W, kDfSpan), kDfStrips), (unsigned)ceil_div(a.H, kDfRows), (unsigned)batch), block(kDfThreads);
    by_storage(fmt->storage, [&](auto sg) {
        typedef typename decltype(sg)::type TI;
        hipLaunchKernelGGL((raw_defects_kernel<decltype(sg)::ST, TI, unpacked_t<TI>>), grid, block, 0, s, a);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
