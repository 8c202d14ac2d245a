// Motion-compensated temporal noise reduction on the mosaic (include/realcam_hip.h, rc_raw_motion_pyramid and rc_raw_temporal_mc): the
// 8-bit luma proxy of a mosaic and its pyramid, for rc_motion_search, and rc_raw_temporal's filter against the state displaced by the
// block vectors that search returns.  Two kernels; no LDS memory, no atomics, no device state.
//
// raw_pyramid_kernel: one launch, the frame read once -- motion.hip's pyramid map on Bayer cells.  A lane owns a 4 x 4 tile of cells (8 rows
//   of 8 samples: two of the row reader's 4-sample loads per row, all sixteen issued before the first is decoded): sixteen level-0 bytes,
//   four level-1 bytes, one level-2 byte; a wave is 16 x 4 lanes (64 x 16 cells), so the level-3 byte of a 2 x 2 group of lanes is two lane
//   exchanges (lane ^ 1, lane ^ 16) and the lane with both bits clear stores it.  A block is four waves side by side (256 x 16 cells).
//   Level 0 goes out as one dword per row and lane, level 1 as one 16-bit store per row where the level's rows keep that alignment, bytes
//   otherwise.  Everything after q is integer.
//
// temporal_mc_kernel: temporal.hip's raw_temporal_kernel -- the same grid, lane map, overlapping strips, row parity per wave, rolling
//   three-row window and lane shifts (see there) -- with another fetch of the state and nothing else changed:
//   vectors    a lane's 4 samples are two cells of one block column (x0 % 4 = 0, the block is even), so it holds one (dx, dy) in registers and
//              reloads it, one 8-byte load, when the block row of the row it is about to read changes: wave-uniform (y is), once per `block`
//              rows; a halo row above or below a band belongs to the neighbouring block row and takes that row's vector.
//   state      row 2 clamp(cy + dy) + par, from cell column cx + dx on: one 16-byte load where neither cell's column is clamped (an address
//              that is 8-byte aligned, not always 16: global loads take it), one 8-byte pair per cell where one is; a state whose base or
//              pitch is no multiple of 8 bytes goes sample by sample.  A whole-cell displacement keeps every sample on its CFA position.
//   e          |c - p| is formed per lane from its own displaced state, so the taps that come from the neighbouring lanes and rows carry
//              their own block's displacement, as the header's step 3 asks.
// One correctly rounded division per sample, 32-bit offsets below a 64-bit frame base (the entry point checks), no scratch.  The arithmetic
// is step for step the header's: every product, sum and quotient rounded on its own.
#include "raw_row.hpp"

#include <cmath>

namespace rc {

// ---- the luma proxy and its pyramid ---------------------------------------------------------------------------------------------------------
constexpr int kRpMaxLevels = 4;
constexpr int kRpWaves = 4, kRpThreads = 64 * kRpWaves, kRpLanesX = 16, kRpTile = 4;                 // a lane's tile: 4 x 4 cells
constexpr int kRpBlockW = kRpWaves * kRpLanesX * kRpTile, kRpBlockH = (64 / kRpLanesX) * kRpTile;  // cells per block
static_assert(kRpTile == kRowPx, "a tile row of 4 cells is 8 samples: two of the row reader's loads");

struct RawPyramidArgs {
    const uint8_t* src;        // row r of frame b starts at src + (b * H + r) * line_bytes
    const float* gain;         // (1 or B) on the device, or null: g below
    uint8_t* lv[kRpMaxLevels];
    int levels;
    int H, W, h, w;            // samples (2h, 2w) and cells
    int line_bytes, vec_in;
    int vec0, vec1;            // level 0: every row starts on a dword; level 1: every row starts on a 16-bit boundary
    int has_gain, gain_stride;
    float black[4];            // CFA-position order
    float inv, g;
};

// q in 0 .. 65025 -> floor(sqrt(q)), exactly: whatever the float square root rounds to is corrected in integers.
__device__ __forceinline__ uint32_t proxy_isqrt(int q) {
    int r = (int)sqrtf((float)q);
    if (r * r > q) --r;
    else if ((r + 1) * (r + 1) <= q) ++r;
    return (uint32_t)r;
}

template <int ST, typename TI>
__global__ void __launch_bounds__(kRpThreads) raw_pyramid_kernel(RawPyramidArgs a) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, frame = blockIdx.z;
    const int tx = (blockIdx.x * kRpWaves + wv) * kRpLanesX + (lane & (kRpLanesX - 1));       // the lane's tile: cells 4 tx .., 4 ty ..
    const int ty = blockIdx.y * (64 / kRpLanesX) + (lane >> 4);
    const int x0 = tx * kRpTile, y0 = ty * kRpTile, cnt = a.w - x0;                         // cnt <= 0: the tile is right of the frame
    const uint32_t line_bytes = (uint32_t)a.line_bytes;
    const uint8_t* src = a.src + (size_t)frame * (size_t)a.H * (size_t)line_bytes;
    // the samples 2 x0 .. 2 x0 + 7 of a row as two loads of 4; a load holds 4, 2 or 0 samples inside the frame (W is even)
    const int sx[2] = {2 * x0, 2 * x0 + kRowPx};
    int n[2];
    bool full[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        n[j] = sx[j] < a.W ? min(a.W - sx[j], kRowPx) : 0;
        full[j] = n[j] == kRowPx && a.vec_in;
    }
    const float g = a.gain ? a.gain[frame * a.gain_stride] : a.g;                             // uniform over the frame
    const bool has_gain = a.has_gain != 0;

    RowRaw raw[2 * kRpTile][2];
#pragma unroll
    for (int r = 0; r < 2 * kRpTile; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            raw[r][j] = RowRaw{{0u, 0u, 0u, 0u}};
            if (2 * y0 + r < a.H && n[j] > 0) raw[r][j] = row_load<ST, TI>(src + (uint32_t)(2 * y0 + r) * line_bytes, sx[j], n[j], full[j]);
        }

    uint32_t q[kRpTile][kRpTile];                                                             // level-0 codes; 0 outside the frame (never stored)
#pragma unroll
    for (int r = 0; r < kRpTile; ++r) {
        float v[2][2 * kRpTile];                                                              // the cell row's two sample rows
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < 2; ++j) row_decode<ST, TI>(raw[2 * r + p][j], n[j], full[j], v[p] + kRowPx * j);
#pragma unroll
        for (int k = 0; k < kRpTile; ++k) {
            const float d0 = __fsub_rn(v[0][2 * k], a.black[0]), d1 = __fsub_rn(v[0][2 * k + 1], a.black[1]);
            const float d2 = __fsub_rn(v[1][2 * k], a.black[2]), d3 = __fsub_rn(v[1][2 * k + 1], a.black[3]);
            const float m = __fmul_rn(__fadd_rn(__fadd_rn(d0, d1), __fadd_rn(d2, d3)), 0.25f);
            float t = __fmul_rn(m, a.inv);
            if (has_gain) t = __fmul_rn(t, g);
            t = t > 0.f ? (t < 1.f ? t : 1.f) : 0.f;                                          // NaN compares false: 0
            const int qq = (int)rintf(__fmul_rn(65025.f, t));                                 // half to even
            q[r][k] = y0 + r < a.h && k < cnt ? proxy_isqrt(qq) : 0u;
        }
    }
    {   // level 0: (B, h, w)
        uint8_t* o = a.lv[0] + ((size_t)frame * a.h + y0) * a.w + x0;
#pragma unroll
        for (int r = 0; r < kRpTile; ++r) {
            if (y0 + r < a.h && cnt > 0) {
                uint8_t* p = o + (size_t)r * a.w;
                if (a.vec0 && cnt >= kRpTile) {
                    *reinterpret_cast<uint32_t*>(p) = q[r][0] | (q[r][1] << 8) | (q[r][2] << 16) | (q[r][3] << 24);
                } else {
#pragma unroll
                    for (int k = 0; k < kRpTile; ++k)
                        if (k < cnt) p[k] = (uint8_t)q[r][k];
                }
            }
        }
    }
    if (a.levels < 2) return;
    uint32_t q1[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) q1[r][k] = (q[2 * r][2 * k] + q[2 * r][2 * k + 1] + q[2 * r + 1][2 * k] + q[2 * r + 1][2 * k + 1] + 2u) >> 2;
    {   // level 1: (B, h >> 1, w >> 1); a pixel that exists has its four sources inside the frame
        const int h1 = a.h >> 1, w1 = a.w >> 1, c1 = w1 - 2 * tx;
        uint8_t* o = a.lv[1] + ((size_t)frame * h1 + 2 * ty) * w1 + 2 * tx;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (2 * ty + r < h1 && c1 > 0) {
                uint8_t* p = o + (size_t)r * w1;
                if (a.vec1 && c1 >= 2) {
                    *reinterpret_cast<uint16_t*>(p) = (uint16_t)(q1[r][0] | (q1[r][1] << 8));
                } else {
                    p[0] = (uint8_t)q1[r][0];
                    if (c1 >= 2) p[1] = (uint8_t)q1[r][1];
                }
            }
        }
    }
    if (a.levels < 3) return;
    const uint32_t q2 = (q1[0][0] + q1[0][1] + q1[1][0] + q1[1][1] + 2u) >> 2;
    {
        const int h2 = a.h >> 2, w2 = a.w >> 2;
        if (ty < h2 && tx < w2) a.lv[2][((size_t)frame * h2 + ty) * w2 + tx] = (uint8_t)q2;
    }
    if (a.levels < 4) return;                                                                 // uniform: every lane reaches the exchanges
    uint32_t s = q2 + (uint32_t)__shfl_xor((int)q2, 1);
    s += (uint32_t)__shfl_xor((int)s, kRpLanesX);
    {
        const int h3 = a.h >> 3, w3 = a.w >> 3;
        if (!(lane & 1) && !(lane & kRpLanesX) && (ty >> 1) < h3 && (tx >> 1) < w3)
            a.lv[3][((size_t)frame * h3 + (ty >> 1)) * w3 + (tx >> 1)] = (uint8_t)((s + 2u) >> 2);
    }
}

// ---- the filter against the displaced state -------------------------------------------------------------------------------------------------
constexpr int kTmcPx = 4, kTmcWaves = 4, kTmcThreads = 64 * kTmcWaves;
constexpr int kTmcSpan = 64 * kTmcPx;             // columns a wave loads
constexpr int kTmcOut = kTmcSpan - 2 * kTmcPx;    // columns it produces inside a row: strips start this far apart
constexpr int kTmcStrips = kTmcWaves / 2;         // strips per block
constexpr int kTmcRows = 32;                      // rows per block
static_assert(kTmcPx == kRowPx, "a lane holds the row reader's 4 samples");
static_assert(kTmcRows % 2 == 0, "a band starts on an even row: a wave's row parity is its CFA row");

struct TmcArgs {
    const uint8_t* src;        // row r of frame b starts at src + (b * H + r) * line_bytes
    const uint8_t* prev;       // the state, fp32: row r of frame b at prev + (b * H + r) * prev_pitch; null with reset
    const float* gain;         // (1 or B) on the device, or null: g below
    const int* vec;            // (B, by, bx, 4): slots 0, 1 are (dx, dy) in cells; null with reset
    uint8_t* dst;
    int H, W;                  // 2h, 2w
    int line_bytes, prev_pitch, dst_pitch;
    int vec_in, pair_prev, vec_out;    // every lane's 4 samples start on a 4-sample boundary of the source / the destination; every cell of
                                       // the state (2 samples of a row) starts on an 8-byte boundary
    int reset, has_gain, gain_stride;  // gain_stride: 0 (one value for every frame) or 1
    int by, bx, blk_log2;      // the vector grid; a node covers (1 << blk_log2)^2 cells
    float black[4];            // CFA-position order
    float n_abs, n_rel, alpha, ramp, slope, g;
};

struct TmcRow { float c[kTmcPx], p[kTmcPx], e[kTmcPx], l[2], r[2]; };          // temporal.hip's TnrRow

struct __attribute__((packed, aligned(8))) TmcQuad { uint32_t v[4]; };         // 16 bytes at an 8-byte aligned address

__device__ __forceinline__ int tmc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int ST, typename TI>
__global__ void __launch_bounds__(kTmcThreads) temporal_mc_kernel(TmcArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int par = wv & 1, strip = blockIdx.x * kTmcStrips + (wv >> 1), frame = blockIdx.z;
    const int xs = strip * kTmcOut;
    if (strip > 0 && xs + 2 * kTmcPx >= a.W) return;                               // wave-uniform: the strip before holds the row's end
    const int x0 = xs + lane * kTmcPx;
    const int n = x0 < a.W ? min(a.W - x0, kTmcPx) : 0;                            // W is even and x0 a multiple of 4: 0, 2 or 4
    const bool act = n > 0, wide = n == kTmcPx;
    const bool first = x0 == 0, more = x0 + kTmcPx < a.W;                          // no columns to the left / columns to the right
    const bool owns = act && (lane > 0 || first) && (lane < 63 || !more);          // this lane's results are stored
    const bool full_in = wide && a.vec_in, full_out = wide && a.vec_out;
    const int r0 = blockIdx.y * kTmcRows, r1 = min(r0 + kTmcRows, a.H);
    const int y_first = r0 + par;
    if (y_first >= r1) return;
    const uint32_t line_bytes = (uint32_t)a.line_bytes, prev_pitch = (uint32_t)a.prev_pitch, dst_pitch = (uint32_t)a.dst_pitch;
    const uint8_t* src = a.src + (size_t)frame * (size_t)a.H * (size_t)line_bytes;
    uint8_t* dst = a.dst + (size_t)frame * (size_t)a.H * (size_t)dst_pitch;
    auto load_c = [&](int y) { RowRaw r = {{0u, 0u, 0u, 0u}}; if (act) r = row_load<ST, TI>(src + (uint32_t)y * line_bytes, x0, n, full_in); return r; };

    if (a.reset) {                                                                 // wave-uniform: out = c; neither the state nor the field is read
        RowRaw ahead = load_c(y_first);
        for (int y = y_first; y < r1; y += 2) {
            const RowRaw raw = ahead;
            if (y + 2 < r1) ahead = load_c(y + 2);
            float v[kTmcPx];
            row_decode<ST, TI>(raw, n, full_in, v);
            if (owns) row_store<float>(reinterpret_cast<float*>(dst + (uint32_t)y * dst_pitch) + x0, v, n, full_out);
        }
        return;
    }

    // 0'. the displaced state.  The lane's cells cx0 and cx0 + 1 lie in block column bi; the block row follows the row that is read
    const uint8_t* prev = a.prev + (size_t)frame * (size_t)a.H * (size_t)prev_pitch;
    const int hc = a.H >> 1, wc = a.W >> 1, cx0 = x0 >> 1;
    const int* node = a.vec + ((size_t)frame * (size_t)a.by * (size_t)a.bx + (size_t)min(cx0 >> a.blk_log2, a.bx - 1)) * 4;
    const bool pairs = a.pair_prev != 0;
    int bj_held = -1, dx = 0, dy = 0;
    auto load_p = [&](int y) {                                                     // the state's bits at the lane's 4 displaced samples
        RowRaw r = {{0u, 0u, 0u, 0u}};
        const int cy = y >> 1, bj = min(cy >> a.blk_log2, a.by - 1);               // wave-uniform
        if (bj != bj_held) {
            bj_held = bj;
            if (act) {                                                             // device data is not trusted: clamped before it is used
                const int2 v = *reinterpret_cast<const int2*>(node + (size_t)bj * (size_t)a.bx * 4);
                dx = tmc_clamp(v.x, -32768, 32767);
                dy = tmc_clamp(v.y, -32768, 32767);
            }
        }
        if (!act) return r;
        const uint8_t* row = prev + (uint32_t)(2 * tmc_clamp(cy + dy, 0, hc - 1) + par) * prev_pitch;
        const int ca = cx0 + dx;                                                   // the second cell's column is ca + 1
        if (wide && pairs && ca >= 0 && ca + 1 < wc) {
            const TmcQuad q = *reinterpret_cast<const TmcQuad*>(row + (uint32_t)ca * 8u);
            r.d[0] = q.v[0]; r.d[1] = q.v[1]; r.d[2] = q.v[2]; r.d[3] = q.v[3];
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j == 0 || wide) {
                    const uint8_t* cell = row + (uint32_t)tmc_clamp(ca + j, 0, wc - 1) * 8u;
                    if (pairs) {
                        const uint2 q = *reinterpret_cast<const uint2*>(cell);
                        r.d[2 * j] = q.x; r.d[2 * j + 1] = q.y;
                    } else {
                        r.d[2 * j] = reinterpret_cast<const uint32_t*>(cell)[0];
                        r.d[2 * j + 1] = reinterpret_cast<const uint32_t*>(cell)[1];
                    }
                }
            }
        }
        return r;
    };
    // r0 is even: y & 1 = par for every row this wave reads; x0 % 4 = 0: x & 1 = k & 1.  The wave's two positions are 2 par and 2 par + 1
    const float black[2] = {a.black[2 * par], a.black[2 * par + 1]};
    const float g = a.gain ? a.gain[frame * a.gain_stride] : a.g;                  // wave-uniform
    const bool has_gain = a.has_gain != 0;
    const float ninth = (float)(1.0 / 9.0);

    // the rows this wave reads: y_first - 2 (when the frame has it) .. y_last + 2 (when the frame has it)
    const int y_last = y_first + ((r1 - 1 - y_first) & ~1);
    const int y_end = y_last + 2 < a.H ? y_last + 2 : y_last;
    int yr = y_first >= 2 ? y_first - 2 : y_first;
    const bool top_row = yr < y_first;
    RowRaw ahead_c = load_c(yr), ahead_p = load_p(yr);

    auto next_row = [&](TmcRow& o) {                                               // every lane of the wave runs this: the shifts need them all
        const RowRaw rc = ahead_c, rp = ahead_p;
        yr += 2;
        if (yr <= y_end) { ahead_c = load_c(yr); ahead_p = load_p(yr); }           // in flight while this row is worked on
        row_decode<ST, TI>(rc, n, full_in, o.c);
#pragma unroll
        for (int k = 0; k < kTmcPx; ++k) {
            const float b = black[k & 1], s = __uint_as_float(rp.d[k]);
            o.p[k] = has_gain ? __fadd_rn(b, __fmul_rn(__fsub_rn(s, b), g)) : s;
            o.e[k] = fabsf(__fsub_rn(o.c[k], o.p[k]));
        }
        const float l2 = __shfl_up(o.e[2], 1), l3 = __shfl_up(o.e[3], 1), r0_ = __shfl_down(o.e[0], 1), r1_ = __shfl_down(o.e[1], 1);
        o.l[0] = first ? o.e[0] : l2; o.l[1] = first ? o.e[1] : l3;
        o.r[0] = more ? r0_ : o.e[2]; o.r[1] = more ? r1_ : o.e[3];
    };
    // the taps of sample k of a row at columns x - 2 and x + 2 (x + 2 of k = 0, 1 is past the frame where the lane holds two samples only)
    auto tap_l = [&](const TmcRow& m, int k) { return k < 2 ? m.l[k] : m.e[k - 2]; };
    auto tap_r = [&](const TmcRow& m, int k) { return k < 2 ? (wide ? m.e[k + 2] : m.e[k]) : m.r[k - 2]; };
    auto prefix = [&](const TmcRow& m, float* h) {                                 // the row above: its three taps, summed in the header's order
#pragma unroll
        for (int k = 0; k < kTmcPx; ++k) h[k] = __fadd_rn(__fadd_rn(tap_l(m, k), m.e[k]), tap_r(m, k));
    };
    auto emit = [&](int y, const float* h, const TmcRow& m, const TmcRow& bt) {
        float o[kTmcPx];
#pragma unroll
        for (int k = 0; k < kTmcPx; ++k) {
            float A = h[k];
            A = __fadd_rn(A, tap_l(m, k)); A = __fadd_rn(A, m.e[k]); A = __fadd_rn(A, tap_r(m, k));
            A = __fadd_rn(A, tap_l(bt, k)); A = __fadd_rn(A, bt.e[k]); A = __fadd_rn(A, tap_r(bt, k));
            const float av = __fmul_rn(A, ninth);
            const float t = __fadd_rn(a.n_abs, __fmul_rn(a.n_rel, fmaxf(__fsub_rn(m.p[k], black[k & 1]), 0.f)));
            const float u = __fdiv_rn(av, t);
            const float d = __fsub_rn(m.c[k], m.p[k]);
            const float kk = u <= 1.f ? a.alpha : __fadd_rn(a.alpha, __fmul_rn(__fsub_rn(u, 1.f), a.slope));
            o[k] = u >= a.ramp ? m.c[k] : __fadd_rn(m.p[k], __fmul_rn(kk, d));
        }
        if (owns) row_store<float>(reinterpret_cast<float*>(dst + (uint32_t)y * dst_pitch) + x0, o, n, full_out);
    };

    TmcRow cur, nxt;
    float h[kTmcPx];
    next_row(cur);
    prefix(cur, h);                                                                // the row above, or row y itself where the frame has none
    if (top_row) next_row(cur);
    for (int y = y_first;; y += 2) {
        const bool below = y + 2 <= y_end;                                         // wave-uniform
        if (below) next_row(nxt);
        else nxt = cur;                                                            // the frame's last rows: the row below is row y itself
        emit(y, h, cur, nxt);
        if (y + 2 >= r1) break;                                                    // then `below` held: y + 2 < r1 <= H
        prefix(cur, h);
        cur = nxt;
    }
}

// What rc_raw_temporal requires of its gain, for both entries here.
inline int tmc_gain(const std::string& who, bool host_gain, float host_value, const float* d_gain, int gain_batch, int batch) {
    RC_REQUIRE(!(host_gain && d_gain), who + ": the gain is given both ways (a host gain and d_gain)");
    if (d_gain) {
        RC_REQUIRE(gain_batch == 1 || gain_batch == batch, who + ": gain_batch must be 1 or the batch");
        RC_REQUIRE(reinterpret_cast<uintptr_t>(d_gain) % 4 == 0, who + ": the gain must be 4-byte aligned");
    } else {
        RC_REQUIRE(gain_batch == 0, who + ": gain_batch without d_gain must be 0");
        if (host_gain) RC_REQUIRE(std::isfinite(host_value) && host_value > 0.f, who + ": the gain must be finite and > 0");
    }
    return RC_OK;
}

}  // namespace rc

using namespace rc;

extern "C" {

int rc_raw_motion_pyramid(const void* d_src, const rc_raw_format* fmt, float gain, const float* d_gain, int gain_batch, int levels,
                          void* const* d_levels, int batch, int h, int w, void* stream) {
    RC_REQUIRE(d_src && fmt && d_levels, "rc_raw_motion_pyramid: null pointer");
    if (const int e = raw_frames("rc_raw_motion_pyramid", batch, h, w)) return e;
    RawSource rs;
    if (const int e = raw_source("rc_raw_motion_pyramid", d_src, fmt, w, &rs)) return e;
    const long long lb = rs.line_bytes;
    if (const int e = raw_blacks_finite("rc_raw_motion_pyramid", fmt)) return e;
    const double span = (double)fmt->white - ((double)fmt->black[0] + (double)fmt->black[1] + (double)fmt->black[2] + (double)fmt->black[3]) / 4.0;
    RC_REQUIRE(std::isfinite(fmt->white) && span > 0.0 && std::isfinite((float)(1.0 / span)),
               "rc_raw_motion_pyramid: white must be finite and above the mean black level");
    const bool host_gain = !(gain == 1.f);                                          // NaN is a gain, and refused
    if (const int e = tmc_gain("rc_raw_motion_pyramid", host_gain, gain, d_gain, gain_batch, batch)) return e;
    RC_REQUIRE(levels >= 1 && levels <= kRpMaxLevels, "rc_raw_motion_pyramid: levels must lie in 1 .. 4");
    RC_REQUIRE((h >> (levels - 1)) >= 1 && (w >> (levels - 1)) >= 1,
               "rc_raw_motion_pyramid: the coarsest level is empty (h >> (levels - 1) or w >> (levels - 1) is 0)");
    RC_REQUIRE(2LL * h * lb <= 0x7fffffffLL, "rc_raw_motion_pyramid: a frame (rows x line_bytes) must stay below 2 GiB");
    RawPyramidArgs a = {};
    for (int k = 0; k < levels; ++k) {
        RC_REQUIRE(d_levels[k], "rc_raw_motion_pyramid: null level pointer");
        a.lv[k] = static_cast<uint8_t*>(d_levels[k]);
    }
    a.src = static_cast<const uint8_t*>(d_src);
    a.gain = d_gain;
    a.levels = levels; a.H = 2 * h; a.W = 2 * w; a.h = h; a.w = w;
    a.line_bytes = (int)lb; a.vec_in = rs.vec;
    a.vec0 = reinterpret_cast<uintptr_t>(a.lv[0]) % 4 == 0 && w % 4 == 0;
    a.vec1 = levels > 1 && reinterpret_cast<uintptr_t>(a.lv[1]) % 2 == 0 && (w >> 1) % 2 == 0;
    a.has_gain = host_gain || d_gain;
    a.gain_stride = d_gain && gain_batch > 1 ? 1 : 0;
    for (int p = 0; p < 4; ++p) a.black[p] = fmt->black[p];
    a.inv = (float)(1.0 / span);
    a.g = gain;
    const dim3 grid((unsigned)ceil_div(w, kRpBlockW), (unsigned)ceil_div(h, kRpBlockH), (unsigned)batch), block(kRpThreads);
    const hipStream_t s = as_stream(stream);
    by_storage(fmt->storage, [&](auto sg) { hipLaunchKernelGGL((raw_pyramid_kernel<decltype(sg)::ST, typename decltype(sg)::type>), grid, block, 0, s, a); });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_raw_temporal_mc(const void* d_src, const rc_raw_format* fmt, const rc_temporal_desc* desc, const float* d_prev, int prev_pitch_bytes,
                       const float* d_gain, int gain_batch, void* d_dst, int dst_pitch_bytes, int batch, int h, int w,
                       const int* d_vec, int by, int bx, int block, void* stream) {
    RC_REQUIRE(d_src && fmt && desc && d_dst, "rc_raw_temporal_mc: null pointer");
    if (const int e = raw_frames("rc_raw_temporal_mc", batch, h, w)) return e;
    RawSource rs;
    if (const int e = raw_source("rc_raw_temporal_mc", d_src, fmt, w, &rs)) return e;
    const long long lb = rs.line_bytes;
    if (const int e = raw_blacks_finite("rc_raw_temporal_mc", fmt)) return e;
    RC_REQUIRE(all_zero(desc->reserved), "rc_raw_temporal_mc: reserved fields must be zero");
    RC_REQUIRE((desc->flags & ~(RC_TNR_RESET | RC_TNR_GAIN)) == 0, "rc_raw_temporal_mc: unknown flags");
    const bool reset = (desc->flags & RC_TNR_RESET) != 0, host_gain = (desc->flags & RC_TNR_GAIN) != 0;
    // the parameters
    RC_REQUIRE(std::isfinite(desc->noise_abs) && desc->noise_abs > 0.f && std::isfinite(desc->noise_rel) && desc->noise_rel >= 0.f,
               "rc_raw_temporal_mc: noise_abs must be finite and > 0, noise_rel finite and >= 0");
    RC_REQUIRE(desc->alpha > 0.f && desc->alpha <= 1.f, "rc_raw_temporal_mc: alpha must lie in (0, 1]");
    RC_REQUIRE(std::isfinite(desc->ramp) && desc->ramp > 1.f, "rc_raw_temporal_mc: ramp must be finite and > 1");
    if (const int e = tmc_gain("rc_raw_temporal_mc", host_gain, desc->gain, d_gain, gain_batch, batch)) return e;
    // the field
    RC_REQUIRE(block == 8 || block == 16 || block == 32, "rc_raw_temporal_mc: block must be 8, 16 or 32");
    RC_REQUIRE(by >= 1 && bx >= 1, "rc_raw_temporal_mc: the vector grid needs by, bx >= 1");
    RC_REQUIRE(reset || d_vec, "rc_raw_temporal_mc: no vectors (d_vec is null) and no RC_TNR_RESET");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_vec) % 16 == 0, "rc_raw_temporal_mc: the vectors must be 16-byte aligned");
    // the state and the destination
    const long long row = 2LL * w * 4, rows = (long long)batch * 2LL * h;
    long long dp, pp = prev_pitch_bytes ? prev_pitch_bytes : row;                  // pp without a state: not looked at
    if (const int e = raw_pitch("rc_raw_temporal_mc", "dst", d_dst, dst_pitch_bytes, row, 4, &dp)) return e;
    RC_REQUIRE(reset || d_prev, "rc_raw_temporal_mc: no state (d_prev is null) and no RC_TNR_RESET");
    if (d_prev) {
        if (const int e = raw_pitch("rc_raw_temporal_mc", "prev", d_prev, prev_pitch_bytes, row, 4, &pp)) return e;
        const uintptr_t p0 = reinterpret_cast<uintptr_t>(d_prev), p1 = p0 + (uintptr_t)((rows - 1) * pp + row);
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_dst), o1 = o0 + (uintptr_t)((rows - 1) * dp + row);
        RC_REQUIRE(p1 <= o0 || o1 <= p0, "rc_raw_temporal_mc: dst overlaps prev (displaced rows and a row's neighbours are read after it is written)");
    }
    // a frame's byte offsets are formed in 32 bits
    RC_REQUIRE(2LL * h * lb <= 0x7fffffffLL && 2LL * h * dp <= 0x7fffffffLL && (!d_prev || 2LL * h * pp <= 0x7fffffffLL),
               "rc_raw_temporal_mc: a frame (rows x pitch: source, state, destination) must stay below 2 GiB");

    TmcArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.prev = reset ? nullptr : reinterpret_cast<const uint8_t*>(d_prev);
    a.gain = reset ? nullptr : d_gain;
    a.vec = reset ? nullptr : d_vec;
    a.dst = static_cast<uint8_t*>(d_dst);
    a.H = 2 * h; a.W = 2 * w;
    a.line_bytes = (int)lb; a.prev_pitch = (int)pp; a.dst_pitch = (int)dp;
    a.vec_in = rs.vec; a.pair_prev = d_prev && reinterpret_cast<uintptr_t>(d_prev) % 8 == 0 && pp % 8 == 0; a.vec_out = raw_vec(d_dst, dp, 4);
    a.reset = reset;
    a.has_gain = !reset && (host_gain || d_gain);
    a.gain_stride = d_gain && gain_batch > 1 ? 1 : 0;
    a.by = by; a.bx = bx; a.blk_log2 = block == 8 ? 3 : block == 16 ? 4 : 5;
    for (int p = 0; p < 4; ++p) a.black[p] = fmt->black[p];
    a.n_abs = desc->noise_abs; a.n_rel = desc->noise_rel; a.alpha = desc->alpha; a.ramp = desc->ramp;
    a.slope = (float)((1.0 - (double)desc->alpha) / ((double)desc->ramp - 1.0));
    a.g = host_gain ? desc->gain : 1.f;
    const hipStream_t s = as_stream(stream);
    const int strips = 1 + (a.W > kTmcSpan ? ceil_div(a.W - kTmcSpan, kTmcOut) : 0);
    const dim3 grid((unsigned)ceil_div(strips, kTmcStrips), (unsigned)ceil_div(a.H, kTmcRows), (unsigned)batch), blk(kTmcThreads);
    by_storage(fmt->storage, [&](auto sg) { hipLaunchKernelGGL((temporal_mc_kernel<decltype(sg)::ST, typename decltype(sg)::type>), grid, blk, 0, s, a); });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
