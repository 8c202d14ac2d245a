// The temporal filter on the mosaic, once, for rc_raw_temporal (temporal.hip: raw_temporal_kernel) and rc_raw_temporal_mc (temporal_mc.hip:
// temporal_mc_kernel): the lane map's constants, the arguments, the kernels' body and the entries' checks.  One sensor frame as delivered
// (any storage, padded lines) and the last filtered frame (B, 2h, 2w) fp32 -> the filtered frame (B, 2h, 2w) fp32 in the frame's code
// units.  A motion-adaptive recursive filter: the weight of the new frame rises with the mean |frame - state| over the same-colour 3x3
// neighbourhood (rows y - 2, y, y + 2, columns x - 2, x, x + 2), measured against the noise expected at the sample's level.  No LDS memory,
// no atomics.  The two kernels differ in how a lane fetches its 4 samples of the state (MC, below) and in nothing else.
//
// temporal_body: grid (pairs of strips, bands of 32 rows, frames), four waves per block -- calibrate.hip's map with a halo.
//   lane map   lane l of a wave holds the 4 consecutive samples xs + 4 l .. + 3 of a row, of the frame and of the state: a load of 4 / 8 / 16
//              bytes for u8 / 16-bit / fp32 samples (5 bytes of a RAW10 line, 6 of a RAW12 line) and one of 16 bytes, one 16-byte store;
//              ragged frames (a base or pitch that is no multiple of 4 samples, the last two columns of a width that is 2 mod 4) go sample by
//              sample.
//   columns    the columns x0 - 2, x0 - 1, x0 + 4, x0 + 5 of |frame - state| come from lanes l - 1 and l + 1 (four lane shifts per row, in
//              registers).  At a strip's two ends there is no such lane, so STRIPS OVERLAP: a wave loads 256 columns and produces the 248 of
//              lanes 1 .. 62; lane 0 produces only at the frame's left edge and lane 63 only where the row ends in it (the taps past the
//              frame fall back to the sample's own column).  64 / 62 = 1.032 x the loads and the arithmetic, no halo load, no second path.
//   rows       waves 0, 2 of a block walk the even rows of the band downwards, waves 1, 3 the odd rows (waves 0, 1: the block's first strip;
//              2, 3: its second), so a wave sees two CFA positions only, and the rows y - 2, y, y + 2 of the stencil are the rows it visits
//              in turn.  It keeps the row above as its three-tap prefix sums (4 registers) and the centre row's c, p, |c - p| and edge taps
//              (16), decodes the row below once, produces row y and moves on: every row's c, p and |c - p| are computed once per wave.  The
//              bytes of the row after that are in flight meanwhile.
//   bands      a band's first two rows need the row above the band and its last two the row below: a wave reads 1 + 16 + 1 rows for 16, a
//              block 36 for 32 -- 1.125 x the reads, 1.075 x the traffic of a u16 frame (2 + 4 bytes read, 4 written per sample).
//   reset      (RC_TNR_RESET) a wave-uniform branch: decode, store, nothing else is read.  The gain is wave-uniform too.
// MC: the state is read displaced by the block vectors rc_motion_search returns.
//   vectors    a lane's 4 samples are two cells of one block column (x0 % 4 = 0, the block is even), so it holds one (dx, dy) in registers and
//              reloads it, one 8-byte load, when the block row of the row it is about to read changes: wave-uniform (y is), once per `block`
//              rows; a halo row above or below a band belongs to the neighbouring block row and takes that row's vector.
//   state      row 2 clamp(cy + dy) + par, from cell column cx + dx on: one 16-byte load where neither cell's column is clamped (an address
//              that is 8-byte aligned, not always 16: global loads take it), one 8-byte pair per cell where one is; a state whose base or
//              pitch is no multiple of 8 bytes goes sample by sample.  A whole-cell displacement keeps every sample on its CFA position.
//   e          |c - p| is formed per lane from its own displaced state, so the taps that come from the neighbouring lanes and rows carry
//              their own block's displacement, as the header's step 3 asks.
// One correctly rounded division per sample (v_div_scale / v_rcp / v_div_fmas / v_div_fixup, denormals on), 32-bit offsets below a 64-bit
// frame base (the entry point checks), no scratch.  The arithmetic is step for step the header's: every product, sum and quotient rounded
// on its own.
#pragma once
#include <type_traits>

#include "raw_row.hpp"

namespace rc {

constexpr int kTnrPx = 4, kTnrWaves = 4, kTnrThreads = 64 * kTnrWaves;
constexpr int kTnrSpan = 64 * kTnrPx;             // columns a wave loads
constexpr int kTnrOut = kTnrSpan - 2 * kTnrPx;    // columns it produces inside a row: strips start this far apart
constexpr int kTnrStrips = kTnrWaves / 2;         // strips per block
constexpr int kTnrRows = 32;                      // rows per block
static_assert(kTnrPx == kRowPx, "a lane holds the row reader's 4 samples");
static_assert(kTnrRows % 2 == 0, "a band starts on an even row: a wave's row parity is its CFA row");

struct TnrArgs {
    const uint8_t* src;        // row r of frame b starts at src + (b * H + r) * line_bytes
    const uint8_t* prev;       // the state, fp32: row r of frame b at prev + (b * H + r) * prev_pitch; null with reset
    const float* gain;         // (1 or B) on the device, or null: g below
    uint8_t* dst;
    int H, W;                  // 2h, 2w
    int line_bytes, prev_pitch, dst_pitch;
    int vec_in, vec_prev, vec_out;     // every lane's 4 samples start on a 4-sample boundary of the source / the state / the destination; MC:
                                       // vec_prev asks less, every cell of the state (2 samples of a row) starts on an 8-byte boundary
    int reset, has_gain, gain_stride;  // gain_stride: 0 (one value for every frame) or 1
    float black[4];            // CFA-position order
    float n_abs, n_rel, alpha, ramp, slope, g;
};

struct TmcArgs : TnrArgs {     // behind the plain kernel's arguments, which keep their places
    const int* vec;            // (B, by, bx, 4): slots 0, 1 are (dx, dy) in cells; null with reset
    int by, bx, blk_log2;      // the vector grid; a node covers (1 << blk_log2)^2 cells
};

// A row as a wave holds it: the frame's samples, the (gained) state, e = |c - p|, and the taps that lie in the neighbouring lanes, with the
// fallback at the frame's edges already taken: l[k] is the tap at column x0 + k - 2 (k = 0, 1), r[k] the one at x0 + 4 + k.
struct TnrRow { float c[kTnrPx], p[kTnrPx], e[kTnrPx], l[2], r[2]; };

struct __attribute__((packed, aligned(8))) TmcQuad { uint32_t v[4]; };         // 16 bytes at an 8-byte aligned address

__device__ __forceinline__ int tmc_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int ST, typename TI, bool MC>
__device__ __forceinline__ void temporal_body(const typename std::conditional<MC, TmcArgs, TnrArgs>::type& a) {
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int par = wv & 1, strip = blockIdx.x * kTnrStrips + (wv >> 1), frame = blockIdx.z;
    const int xs = strip * kTnrOut;
    if (strip > 0 && xs + 2 * kTnrPx >= a.W) return;                               // wave-uniform: the strip before holds the row's end
    const int x0 = xs + lane * kTnrPx;
    const int n = x0 < a.W ? min(a.W - x0, kTnrPx) : 0;                            // W is even and x0 a multiple of 4: 0, 2 or 4
    const bool act = n > 0, wide = n == kTnrPx;
    const bool first = x0 == 0, more = x0 + kTnrPx < a.W;                          // no columns to the left / columns to the right
    const bool owns = act && (lane > 0 || first) && (lane < 63 || !more);          // this lane's results are stored
    const bool full_in = wide && a.vec_in, full_prev = wide && a.vec_prev, full_out = wide && a.vec_out;
    const int r0 = blockIdx.y * kTnrRows, r1 = min(r0 + kTnrRows, a.H);
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
            float v[kTnrPx];
            row_decode<ST, TI>(raw, n, full_in, v);
            if (owns) row_store<float>(reinterpret_cast<float*>(dst + (uint32_t)y * dst_pitch) + x0, v, n, full_out);
        }
        return;
    }

    // The state's bits at the lane's 4 samples of row y, fp32 as they lie.  MC: the displaced samples.  The lane's cells cx0 and cx0 + 1 lie
    // in one block column, whose nodes start at `node`; the block row follows the row that is read
    const uint8_t* prev = a.prev + (size_t)frame * (size_t)a.H * (size_t)prev_pitch;
    const int hc = a.H >> 1, wc = a.W >> 1, cx0 = x0 >> 1;
    const int* node = nullptr;
    if constexpr (MC) node = a.vec + ((size_t)frame * (size_t)a.by * (size_t)a.bx + (size_t)min(cx0 >> a.blk_log2, a.bx - 1)) * 4;
    int bj_held = -1, dx = 0, dy = 0;
    auto load_p = [&](int y) {
        RowRaw r = {{0u, 0u, 0u, 0u}};
        if constexpr (MC) {
            const int cy = y >> 1, bj = min(cy >> a.blk_log2, a.by - 1);           // wave-uniform
            if (bj != bj_held) {
                bj_held = bj;
                if (act) {                                                         // device data is not trusted: clamped before it is used
                    const int2 v = *reinterpret_cast<const int2*>(node + (size_t)bj * (size_t)a.bx * 4);
                    dx = tmc_clamp(v.x, -32768, 32767);
                    dy = tmc_clamp(v.y, -32768, 32767);
                }
            }
            if (!act) return r;
            const uint8_t* row = prev + (uint32_t)(2 * tmc_clamp(cy + dy, 0, hc - 1) + par) * prev_pitch;
            const int ca = cx0 + dx;                                               // the second cell's column is ca + 1
            if (full_prev && ca >= 0 && ca + 1 < wc) {
                const TmcQuad q = *reinterpret_cast<const TmcQuad*>(row + (uint32_t)ca * 8u);
                r.d[0] = q.v[0]; r.d[1] = q.v[1]; r.d[2] = q.v[2]; r.d[3] = q.v[3];
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j == 0 || wide) {
                        const uint8_t* cell = row + (uint32_t)tmc_clamp(ca + j, 0, wc - 1) * 8u;
                        if (a.vec_prev) {
                            const uint2 q = *reinterpret_cast<const uint2*>(cell);
                            r.d[2 * j] = q.x; r.d[2 * j + 1] = q.y;
                        } else {
                            r.d[2 * j] = reinterpret_cast<const uint32_t*>(cell)[0];
                            r.d[2 * j + 1] = reinterpret_cast<const uint32_t*>(cell)[1];
                        }
                    }
                }
            }
        } else {
            if (act) r = row_load<kElem, float>(prev + (uint32_t)y * prev_pitch, x0, n, full_prev);
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

    auto next_row = [&](TnrRow& o) {                                               // every lane of the wave runs this: the shifts need them all
        const RowRaw rc = ahead_c, rp = ahead_p;
        yr += 2;
        if (yr <= y_end) { ahead_c = load_c(yr); ahead_p = load_p(yr); }           // in flight while this row is worked on
        row_decode<ST, TI>(rc, n, full_in, o.c);
#pragma unroll
        for (int k = 0; k < kTnrPx; ++k) {
            const float b = black[k & 1], s = __uint_as_float(rp.d[k]);
            o.p[k] = has_gain ? __fadd_rn(b, __fmul_rn(__fsub_rn(s, b), g)) : s;
            o.e[k] = fabsf(__fsub_rn(o.c[k], o.p[k]));
        }
        const float l2 = __shfl_up(o.e[2], 1), l3 = __shfl_up(o.e[3], 1), r0_ = __shfl_down(o.e[0], 1), r1_ = __shfl_down(o.e[1], 1);
        o.l[0] = first ? o.e[0] : l2; o.l[1] = first ? o.e[1] : l3;
        o.r[0] = more ? r0_ : o.e[2]; o.r[1] = more ? r1_ : o.e[3];
    };
    // the taps of sample k of a row at columns x - 2 and x + 2 (x + 2 of k = 0, 1 is past the frame where the lane holds two samples only)
    auto tap_l = [&](const TnrRow& m, int k) { return k < 2 ? m.l[k] : m.e[k - 2]; };
    auto tap_r = [&](const TnrRow& m, int k) { return k < 2 ? (wide ? m.e[k + 2] : m.e[k]) : m.r[k - 2]; };
    auto prefix = [&](const TnrRow& m, float* h) {                                 // the row above: its three taps, summed in the header's order
#pragma unroll
        for (int k = 0; k < kTnrPx; ++k) h[k] = __fadd_rn(__fadd_rn(tap_l(m, k), m.e[k]), tap_r(m, k));
    };
    auto emit = [&](int y, const float* h, const TnrRow& m, const TnrRow& bt) {
        float o[kTnrPx];
#pragma unroll
        for (int k = 0; k < kTnrPx; ++k) {
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

    TnrRow cur, nxt;
    float h[kTnrPx];
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

// ---- the host half ----------------------------------------------------------------------------------------------------------------------------
struct TnrField { const int* d_vec; int by, bx, block; };                          // rc_raw_temporal_mc's vectors

// What both entries require of their arguments (`field`: null for rc_raw_temporal), the kernel's arguments and its grid of kTnrThreads.
inline int temporal_args(const char* who, const void* d_src, const rc_raw_format* fmt, const rc_temporal_desc* desc, const float* d_prev, int prev_pitch_bytes,
                         const float* d_gain, int gain_batch, void* d_dst, int dst_pitch_bytes, int batch, int h, int w, const TnrField* field,
                         TmcArgs* out, dim3* grid) {
    TmcArgs& a = *out;
    const std::string at = std::string(who) + ": ";
    RC_REQUIRE(d_src && fmt && desc && d_dst, at + "null pointer");
    if (const int e = raw_frames(who, batch, h, w)) return e;
    RawSource rs;
    if (const int e = raw_source(who, d_src, fmt, w, &rs)) return e;
    const long long lb = rs.line_bytes;
    if (const int e = raw_blacks_finite(who, fmt)) return e;
    RC_REQUIRE(all_zero(desc->reserved), at + "reserved fields must be zero");
    RC_REQUIRE((desc->flags & ~(RC_TNR_RESET | RC_TNR_GAIN)) == 0, at + "unknown flags");
    const bool reset = (desc->flags & RC_TNR_RESET) != 0, host_gain = (desc->flags & RC_TNR_GAIN) != 0;
    // the parameters
    RC_REQUIRE(std::isfinite(desc->noise_abs) && desc->noise_abs > 0.f && std::isfinite(desc->noise_rel) && desc->noise_rel >= 0.f,
               at + "noise_abs must be finite and > 0, noise_rel finite and >= 0");
    RC_REQUIRE(desc->alpha > 0.f && desc->alpha <= 1.f, at + "alpha must lie in (0, 1]");
    RC_REQUIRE(std::isfinite(desc->ramp) && desc->ramp > 1.f, at + "ramp must be finite and > 1");
    if (const int e = raw_gain(who, field ? "a host gain" : "RC_TNR_GAIN", host_gain, desc->gain, d_gain, gain_batch, batch)) return e;
    if (field) {
        RC_REQUIRE(field->block == 8 || field->block == 16 || field->block == 32, at + "block must be 8, 16 or 32");
        RC_REQUIRE(field->by >= 1 && field->bx >= 1, at + "the vector grid needs by, bx >= 1");
        RC_REQUIRE(reset || field->d_vec, at + "no vectors (d_vec is null) and no RC_TNR_RESET");
        RC_REQUIRE(reinterpret_cast<uintptr_t>(field->d_vec) % 16 == 0, at + "the vectors must be 16-byte aligned");
    }
    // the state and the destination
    const long long row = 2LL * w * 4, rows = (long long)batch * 2LL * h;
    long long dp, pp = prev_pitch_bytes ? prev_pitch_bytes : row;                  // pp without a state: not looked at
    if (const int e = raw_pitch(who, "dst", d_dst, dst_pitch_bytes, row, 4, &dp)) return e;
    RC_REQUIRE(reset || d_prev, at + "no state (d_prev is null) and no RC_TNR_RESET");
    if (d_prev) {
        if (const int e = raw_pitch(who, "prev", d_prev, prev_pitch_bytes, row, 4, &pp)) return e;
        const uintptr_t p0 = reinterpret_cast<uintptr_t>(d_prev), p1 = p0 + (uintptr_t)((rows - 1) * pp + row);
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_dst), o1 = o0 + (uintptr_t)((rows - 1) * dp + row);
        RC_REQUIRE(p1 <= o0 || o1 <= p0, at + "dst overlaps prev (" + (field ? "displaced rows and " : "") + "a row's neighbours are read after it is written)");
    }
    // a frame's byte offsets are formed in 32 bits
    RC_REQUIRE(2LL * h * lb <= 0x7fffffffLL && 2LL * h * dp <= 0x7fffffffLL && (!d_prev || 2LL * h * pp <= 0x7fffffffLL),
               at + "a frame (rows x pitch: source, state, destination) must stay below 2 GiB");

    a = TmcArgs{};
    a.src = static_cast<const uint8_t*>(d_src);
    a.prev = reset ? nullptr : reinterpret_cast<const uint8_t*>(d_prev);
    a.gain = reset ? nullptr : d_gain;
    a.dst = static_cast<uint8_t*>(d_dst);
    a.H = 2 * h; a.W = 2 * w;
    a.line_bytes = (int)lb; a.prev_pitch = (int)pp; a.dst_pitch = (int)dp;
    a.vec_in = rs.vec; a.vec_prev = d_prev && (field ? reinterpret_cast<uintptr_t>(d_prev) % 8 == 0 && pp % 8 == 0 : raw_vec(d_prev, pp, 4)); a.vec_out = raw_vec(d_dst, dp, 4);
    a.reset = reset;
    a.has_gain = !reset && (host_gain || d_gain);
    a.gain_stride = d_gain && gain_batch > 1 ? 1 : 0;
    for (int p = 0; p < 4; ++p) a.black[p] = fmt->black[p];
    a.n_abs = desc->noise_abs; a.n_rel = desc->noise_rel; a.alpha = desc->alpha; a.ramp = desc->ramp;
    a.slope = (float)((1.0 - (double)desc->alpha) / ((double)desc->ramp - 1.0));
    a.g = host_gain ? desc->gain : 1.f;
    if (field) {
        a.vec = reset ? nullptr : field->d_vec;
        a.by = field->by; a.bx = field->bx; a.blk_log2 = field->block == 8 ? 3 : field->block == 16 ? 4 : 5;
    }
    const int strips = 1 + (a.W > kTnrSpan ? ceil_div(a.W - kTnrSpan, kTnrOut) : 0);
    *grid = dim3((unsigned)ceil_div(strips, kTnrStrips), (unsigned)ceil_div(a.H, kTnrRows), (unsigned)batch);
    return RC_OK;
}

}  // namespace rc
