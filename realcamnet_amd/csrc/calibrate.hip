// Sensor calibration on the mosaic (include/realcam_hip.h, rc_raw_calibrate): the sensor frame as rc_raw_defects reads it (any storage,
// padded lines) -> the linearised, normalised, flat-fielded, white-balanced mosaic (B, 2h, 2w) as fp32 / bf16 / fp16, unpacked.  Pointwise:
// no halo, no LDS tile, no atomics.
//
// raw_calibrate_kernel: grid (pairs of strips, bands of 16 rows, frames), four waves per block.
//   lane map   a STRIP is 256 columns.  Lane l of a wave holds the 4 consecutive samples 256 s + 4 l .. + 3 of a row.  Every lane's first
//              column is a multiple of 4: one 4 / 8 / 16-byte load per lane and row for u8 / 16-bit / fp32 samples, 5 bytes of a RAW10
//              line, 6 of a RAW12 line (whole dwords, as the ingest reads them), one 8- or 16-byte store; ragged frames (a base or pitch
//              that is no multiple of 4 samples, the last two columns of a width that is 2 mod 4) go sample by sample.
//   rows       waves 0, 2 of a block walk the even rows of the band downwards, waves 1, 3 the odd rows (waves 0, 1: the block's first
//              strip; 2, 3: its second), so a wave sees two CFA positions only: its blacks, divisors and gains are six values read once.
//              The raw bytes of the wave's next row are in flight while it works on this one.  Eight rows per wave: bands of 32 and 64
//              rows measured slower.
//   gain map   the lane's 4 samples are 2 plane columns X, X + 1 (X even) of each of the wave's two positions; a cell is >= 8 plane
//              columns, so they share one node column.  When the node row changes (at most every 16 mosaic rows) the lane fetches the
//              eight nodes (two positions x four corners; lanes of a cell ask for the same words, out of L2) and forms `top` and `bot` of
//              its 2 x 2 (position, column) pairs; down the rows only g = top + fy (bot - top) is left.
//   curve      the knots ride in the kernel's argument block; wave 0 lays them out in LDS once per block (16 slots of x_j, y_j, s_j; x_j of
//              the unused slots is +inf) and every sample bisects them branch-free: at most four compares, then one 16-byte LDS read.
// No division, no 64-bit address arithmetic per sample (a frame's offsets fit 32 bits: the entry point checks), no scratch.  The arithmetic
// is step for step the header's: every product and sum rounded on its own.
#include "raw_row.hpp"

#include <cmath>

namespace rc {

constexpr int kCalPx = 4, kCalWaves = 4, kCalThreads = 64 * kCalWaves;
constexpr int kCalSpan = 64 * kCalPx;             // columns of a strip
constexpr int kCalStrips = kCalWaves / 2;         // strips per block
constexpr int kCalRows = 16;                      // rows per block
constexpr int kCalKnots = RC_CALIB_MAX_KNOTS;
static_assert(kCalPx == kRowPx, "a lane holds the row reader's 4 samples");

struct CalArgs {
    const uint8_t* src;        // mosaic row r of frame b starts at src + (b * H + r) * line_bytes
    const float* map;          // (4, Gh, Gw) or null
    const float* wb;           // (1 or B, 4) or null
    uint8_t* dst;
    int H, W;                  // the mosaic's rows and columns (2h, 2w)
    int line_bytes, dst_pitch;
    int vec_in, vec_out;       // every lane's 4 samples start on a 4-sample boundary of the source / the destination
    int nseg;                  // curve segments (knots - 1), 0: no curve
    int cell_log2, Gw, plane;  // gain map: log2(cell), nodes per row, nodes per position
    int wb_stride;             // 0 (one row for every frame) or 4
    int gains, clip;           // host gains on / clip on
    float black[4], inv[4], gain[4];   // CFA-position order
    float lo, hi;
    float cx[kCalKnots], cy[kCalKnots], cs[kCalKnots];     // segment j: x_j, y_j and its slope; cx[j] = +inf past the last segment
};

// Step 1 of the header: segment j is the last one whose x_j <= c (segment 0 below x_1), then l = y_j + (c - x_j) s_j.  kx[j] = x_j, +inf past
// the last segment, so the bisect over 16 slots needs no bound; seg[j] = (x_j, y_j, s_j, 0).  The steps a short curve cannot need are skipped
// (wave-uniform: nseg is an argument).
__device__ __forceinline__ float cal_curve(const float* kx, const float4* seg, int nseg, float c) {
    int j = 0;
    if (nseg > 7) j = c >= kx[8] ? 8 : 0;
    if (nseg > 3) j = c >= kx[j + 4] ? j + 4 : j;
    if (nseg > 1) {
        j = c >= kx[j + 2] ? j + 2 : j;
        j = c >= kx[j + 1] ? j + 1 : j;
    }
    const float4 q = seg[j];
    return __fadd_rn(q.y, __fmul_rn(__fsub_rn(c, q.x), q.z));
}

template <int ST, typename TI, typename TO>
__global__ void __launch_bounds__(kCalThreads) raw_calibrate_kernel(CalArgs a) {
    __shared__ float4 seg[kCalKnots];                                              // the curve: 320 bytes, read per sample by its own index
    __shared__ float kx[kCalKnots];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (a.nseg) {                                                                  // block-uniform
        if (wv == 0) {                                                             // every lane writes the same 16 slots: no indexed read of the arguments
#pragma unroll
            for (int j = 0; j < kCalKnots; ++j) {
                seg[j] = make_float4(a.cx[j], a.cy[j], a.cs[j], 0.f);
                kx[j] = a.cx[j];
            }
        }
        __syncthreads();
    }
    const int par = wv & 1, strip = blockIdx.x * kCalStrips + (wv >> 1), frame = blockIdx.z;
    const int x0 = strip * kCalSpan + lane * kCalPx;
    if (x0 >= a.W) return;                                                         // no barrier and no lane exchange below
    const int n = min(a.W - x0, kCalPx);                                           // W is even and x0 a multiple of 4: 2 or 4
    const bool full_in = n == kCalPx && a.vec_in, full_out = n == kCalPx && a.vec_out;
    const int r0 = blockIdx.y * kCalRows, r1 = min(r0 + kCalRows, a.H);
    const uint8_t* src = a.src + (size_t)frame * (size_t)a.H * (size_t)a.line_bytes;
    uint8_t* dst = a.dst + (size_t)frame * (size_t)a.H * (size_t)a.dst_pitch;
    // r0 is even: y & 1 = par; x0 % 4 = 0: x & 1 = k & 1.  The wave's two positions are 2 par and 2 par + 1
    const float black[2] = {a.black[2 * par], a.black[2 * par + 1]}, inv[2] = {a.inv[2 * par], a.inv[2 * par + 1]};
    float wb[2] = {a.gain[2 * par], a.gain[2 * par + 1]};
    const bool use_wb = a.wb != nullptr || a.gains;
    if (a.wb) {
        const float* row = a.wb + frame * a.wb_stride;
        wb[0] = row[2 * par]; wb[1] = row[2 * par + 1];
    }
    const int k = a.cell_log2, cmask = (1 << k) - 1;
    const float step = __uint_as_float((uint32_t)(127 - k) << 23);                 // 2^-k
    const int X0 = x0 >> 1;                                                        // even: X0 and X0 + 1 lie in one cell
    const float fx[2] = {__fmul_rn((float)(X0 & cmask), step), __fmul_rn((float)((X0 + 1) & cmask), step)};
    const uint32_t node0 = (uint32_t)(X0 >> k);
    float top[2][2] = {{1.f, 1.f}, {1.f, 1.f}}, bot[2][2] = {{1.f, 1.f}, {1.f, 1.f}};     // [position][column]
    int node_row = -1;

    int y = r0 + par;
    if (y >= r1) return;
    const uint32_t line_bytes = (uint32_t)a.line_bytes;
    RowRaw ahead = row_load<ST, TI>(src + (uint32_t)y * line_bytes, x0, n, full_in);
    for (; y < r1; y += 2) {
        const RowRaw raw = ahead;
        if (y + 2 < r1) ahead = row_load<ST, TI>(src + (uint32_t)(y + 2) * line_bytes, x0, n, full_in);     // in flight while this row is worked on
        float v[kCalPx];
        row_decode<ST, TI>(raw, n, full_in, v);
        float fy = 0.f;
        if (a.map) {                                                               // wave-uniform
            const int Y = y >> 1, j0 = Y >> k;
            fy = __fmul_rn((float)(Y & cmask), step);
            if (j0 != node_row) {                                                  // wave-uniform: at most every 16 rows
                node_row = j0;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const float* g = a.map + ((uint32_t)(2 * par + p) * (uint32_t)a.plane + (uint32_t)j0 * (uint32_t)a.Gw + node0);
                    const float g00 = g[0], g01 = g[1], g10 = g[a.Gw], g11 = g[a.Gw + 1];
                    const float dt = __fsub_rn(g01, g00), db = __fsub_rn(g11, g10);
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        top[p][c] = __fadd_rn(g00, __fmul_rn(fx[c], dt));
                        bot[p][c] = __fadd_rn(g10, __fmul_rn(fx[c], db));
                    }
                }
            }
        }
        float o[kCalPx];
#pragma unroll
        for (int s = 0; s < kCalPx; ++s) {
            const int p = s & 1, c = s >> 1;
            float m = v[s];
            if (a.nseg) m = cal_curve(kx, seg, a.nseg, m);
            m = __fmul_rn(__fsub_rn(m, black[p]), inv[p]);
            if (a.map) m = __fmul_rn(m, __fadd_rn(top[p][c], __fmul_rn(fy, __fsub_rn(bot[p][c], top[p][c]))));
            if (use_wb) m = __fmul_rn(m, wb[p]);
            if (a.clip) m = fminf(fmaxf(m, a.lo), a.hi);
            o[s] = m;
        }
        row_store<TO>(reinterpret_cast<TO*>(dst + (uint32_t)y * (uint32_t)a.dst_pitch) + x0, o, n, full_out);
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_calib_desc_size(void) { return sizeof(rc_calib_desc); }

int rc_raw_calibrate(const void* d_src, const rc_raw_format* fmt, const rc_calib_desc* desc, const float* d_gain_map, const float* d_frame_gains,
                     int frame_gains_batch, void* d_dst, int dst_dtype, int dst_pitch_bytes, int batch, int h, int w, void* stream) {
    RC_REQUIRE(d_src && fmt && desc && d_dst, "rc_raw_calibrate: null pointer");
    if (const int e = raw_frames("rc_raw_calibrate", batch, h, w)) return e;
    RawSource rs;
    if (const int e = raw_source("rc_raw_calibrate", d_src, fmt, w, &rs)) return e;
    const long long lb = rs.line_bytes;
    RC_REQUIRE(dst_dtype == RC_F32 || dst_dtype == RC_BF16 || dst_dtype == RC_F16, "rc_raw_calibrate: dst dtype must be RC_F32, RC_BF16 or RC_F16");
    RC_REQUIRE(all_zero(desc->reserved), "rc_raw_calibrate: reserved fields must be zero");
    RC_REQUIRE((desc->flags & ~(RC_CALIB_GAINS | RC_CALIB_CLIP)) == 0, "rc_raw_calibrate: unknown flags");
    for (int p = 0; p < 4; ++p)
        RC_REQUIRE(std::isfinite(fmt->black[p]) && std::isfinite(fmt->white) && fmt->white > fmt->black[p], "rc_raw_calibrate: white must exceed every black level (all finite)");
    // the curve
    const int K = desc->knots;
    RC_REQUIRE(K == 0 || (K >= 2 && K <= RC_CALIB_MAX_KNOTS), "rc_raw_calibrate: a curve has 2 to 16 knots (0: no curve)");
    for (int j = 0; j < K; ++j) {
        RC_REQUIRE(std::isfinite(desc->curve_x[j]) && std::isfinite(desc->curve_y[j]), "rc_raw_calibrate: knots must be finite");
        RC_REQUIRE(j == 0 || (desc->curve_x[j] > desc->curve_x[j - 1] && desc->curve_y[j] >= desc->curve_y[j - 1]),
                   "rc_raw_calibrate: knots out of order (x strictly increasing, y non-decreasing)");
    }
    // the gain map
    const int cell = desc->cell;
    RC_REQUIRE(cell == 0 || cell == 8 || cell == 16 || cell == 32 || cell == 64 || cell == 128, "rc_raw_calibrate: cell must be 8, 16, 32, 64 or 128 (0: no gain map)");
    RC_REQUIRE((cell != 0) == (d_gain_map != nullptr), "rc_raw_calibrate: a gain map needs both its pointer and its cell");
    RC_REQUIRE(!d_gain_map || reinterpret_cast<uintptr_t>(d_gain_map) % 4 == 0, "rc_raw_calibrate: the gain map must be 4-byte aligned");
    // the gains
    const bool host_gains = (desc->flags & RC_CALIB_GAINS) != 0;
    RC_REQUIRE(!(host_gains && d_frame_gains), "rc_raw_calibrate: gains given twice (RC_CALIB_GAINS and d_frame_gains)");
    if (host_gains)
        for (int p = 0; p < 4; ++p) RC_REQUIRE(std::isfinite(desc->gains[p]) && desc->gains[p] >= 0.f, "rc_raw_calibrate: gains must be finite and >= 0");
    if (d_frame_gains) {
        RC_REQUIRE(frame_gains_batch == 1 || frame_gains_batch == batch, "rc_raw_calibrate: frame_gains_batch must be 1 or the batch");
        RC_REQUIRE(reinterpret_cast<uintptr_t>(d_frame_gains) % 4 == 0, "rc_raw_calibrate: the frame gains must be 4-byte aligned");
    } else {
        RC_REQUIRE(frame_gains_batch == 0, "rc_raw_calibrate: frame_gains_batch without d_frame_gains must be 0");
    }
    const bool clip = (desc->flags & RC_CALIB_CLIP) != 0;
    if (clip) RC_REQUIRE(std::isfinite(desc->clip_lo) && std::isfinite(desc->clip_hi) && desc->clip_lo < desc->clip_hi, "rc_raw_calibrate: clip needs finite lo < hi");
    RC_REQUIRE(K || cell || host_gains || d_frame_gains || clip, "rc_raw_calibrate: nothing enabled (no curve, no gain map, no gains, no clip)");
    // the destination
    const int osize = (int)dtype_size(dst_dtype);
    long long dp;
    if (const int e = raw_pitch("rc_raw_calibrate", "dst", d_dst, dst_pitch_bytes, 2LL * w * osize, osize, &dp)) return e;
    // a frame's byte offsets are formed in 32 bits
    RC_REQUIRE(2LL * h * lb <= 0x7fffffffLL && 2LL * h * dp <= 0x7fffffffLL, "rc_raw_calibrate: a frame (rows x pitch) must stay below 2 GiB");

    CalArgs a;
    a.src = static_cast<const uint8_t*>(d_src);
    a.map = d_gain_map;
    a.wb = d_frame_gains;
    a.dst = static_cast<uint8_t*>(d_dst);
    a.H = 2 * h; a.W = 2 * w;
    a.line_bytes = (int)lb; a.dst_pitch = (int)dp;
    a.vec_in = rs.vec; a.vec_out = raw_vec(d_dst, dp, osize);
    a.nseg = K ? K - 1 : 0;
    a.cell_log2 = 0; a.Gw = 0; a.plane = 0;
    if (cell) {
        while ((1 << a.cell_log2) < cell) ++a.cell_log2;
        const int gh = ceil_div(h, cell) + 1;
        a.Gw = ceil_div(w, cell) + 1;
        a.plane = gh * a.Gw;                                     // h w < 2^29 (the 2 GiB bound), cell >= 8: four planes fit 32 bits with room
    }
    a.wb_stride = d_frame_gains && frame_gains_batch > 1 ? 4 : 0;
    a.gains = host_gains; a.clip = clip;
    for (int p = 0; p < 4; ++p) {
        a.black[p] = fmt->black[p];
        a.inv[p] = 1.f / (fmt->white - fmt->black[p]);           // rc_raw_ingest_fmt's divisor: (v - black) * (1 / (white - black))
        a.gain[p] = host_gains ? desc->gains[p] : 1.f;
    }
    a.lo = clip ? desc->clip_lo : 0.f; a.hi = clip ? desc->clip_hi : 0.f;
    for (int j = 0; j < kCalKnots; ++j) {
        const bool live = j < a.nseg;
        a.cx[j] = live ? desc->curve_x[j] : INFINITY;
        a.cy[j] = live ? desc->curve_y[j] : 0.f;
        a.cs[j] = live ? (float)(((double)desc->curve_y[j + 1] - (double)desc->curve_y[j]) / ((double)desc->curve_x[j + 1] - (double)desc->curve_x[j])) : 0.f;
    }
    const hipStream_t s = as_stream(stream);
    const dim3 grid((unsigned)ceil_div(ceil_div(a.W, kCalSpan), kCalStrips), (unsigned)ceil_div(a.H, kCalRows), (unsigned)batch), block(kCalThreads);
    by_storage(fmt->storage, [&](auto sg) {
        by_dtype(dst_dtype, [&](auto to) {
            hipLaunchKernelGGL((raw_calibrate_kernel<decltype(sg)::ST, typename decltype(sg)::type, typename decltype(to)::type>), grid, block, 0, s, a);
        });
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
