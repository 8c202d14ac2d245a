// Motion-compensated temporal noise reduction on the mosaic (include/realcam_hip.h, rc_raw_motion_pyramid and rc_raw_temporal_mc): the
// 8-bit luma proxy of a mosaic and its pyramid, for rc_motion_search, and rc_raw_temporal's filter against the state displaced by the
// block vectors that search returns.  Two kernels; no LDS memory, no atomics, no device state.
//
// raw_pyramid_kernel: one launch, the frame read once -- pyramid_tail.hpp's map on Bayer cells.  A lane owns a 4 x 4 tile of cells (8 rows
//   of 8 samples: two of the row reader's 4-sample loads per row, all sixteen issued before the first is decoded) and forms its sixteen
//   level-0 codes; the levels' reductions and stores are pyramid_tail.hpp's.  Everything after q is integer.
//
// temporal_mc_kernel: temporal_kernel.hpp's filter, shared with temporal.hip's raw_temporal_kernel -- the same grid, lane map, overlapping
//   strips, row parity per wave, rolling three-row window and lane shifts -- with the displaced fetch of the state (MC there).
#include "pyramid_tail.hpp"
#include "temporal_kernel.hpp"

namespace rc {

// ---- the luma proxy and its pyramid ---------------------------------------------------------------------------------------------------------
static_assert(kPyrTile == kRowPx, "a tile row of 4 cells is 8 samples: two of the row reader's loads");

struct RawPyramidArgs {
    const uint8_t* src;        // row r of frame b starts at src + (b * H + r) * line_bytes
    const float* gain;         // (1 or B) on the device, or null: g below
    uint8_t* lv[RC_MOTION_MAX_LEVELS];
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
__global__ void __launch_bounds__(kPyrThreads) raw_pyramid_kernel(RawPyramidArgs a) {
    const int lane = threadIdx.x & 63, frame = blockIdx.z;
    const int tx = pyramid_tx(lane), ty = pyramid_ty(lane);                                   // the lane's tile: cells 4 tx .., 4 ty ..
    const int x0 = tx * kPyrTile, y0 = ty * kPyrTile, cnt = a.w - x0;                         // cnt <= 0: the tile is right of the frame
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

    RowRaw raw[2 * kPyrTile][2];
#pragma unroll
    for (int r = 0; r < 2 * kPyrTile; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            raw[r][j] = RowRaw{{0u, 0u, 0u, 0u}};
            if (2 * y0 + r < a.H && n[j] > 0) raw[r][j] = row_load<ST, TI>(src + (uint32_t)(2 * y0 + r) * line_bytes, sx[j], n[j], full[j]);
        }

    uint32_t q[kPyrTile][kPyrTile];                                                           // level-0 codes; 0 outside the frame (never stored)
#pragma unroll
    for (int r = 0; r < kPyrTile; ++r) {
        float v[2][2 * kPyrTile];                                                             // the cell row's two sample rows
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int j = 0; j < 2; ++j) row_decode<ST, TI>(raw[2 * r + p][j], n[j], full[j], v[p] + kRowPx * j);
#pragma unroll
        for (int k = 0; k < kPyrTile; ++k) {
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
    pyramid_tail(a, frame, lane, tx, ty, q);
}

// ---- the filter against the displaced state -------------------------------------------------------------------------------------------------
template <int ST, typename TI>
__global__ void __launch_bounds__(kTnrThreads) temporal_mc_kernel(TmcArgs a) { temporal_body<ST, TI, true>(a); }

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
    if (const int e = raw_gain("rc_raw_motion_pyramid", "a host gain", host_gain, gain, d_gain, gain_batch, batch)) return e;
    RC_REQUIRE(levels >= 1 && levels <= RC_MOTION_MAX_LEVELS, "rc_raw_motion_pyramid: levels must lie in 1 .. 4");
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
    const dim3 grid((unsigned)ceil_div(w, kPyrBlockW), (unsigned)ceil_div(h, kPyrBlockH), (unsigned)batch), block(kPyrThreads);
    const hipStream_t s = as_stream(stream);
    by_storage(fmt->storage, [&](auto sg) { hipLaunchKernelGGL((raw_pyramid_kernel<decltype(sg)::ST, typename decltype(sg)::type>), grid, block, 0, s, a); });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

int rc_raw_temporal_mc(const void* d_src, const rc_raw_format* fmt, const rc_temporal_desc* desc, const float* d_prev, int prev_pitch_bytes,
                       const float* d_gain, int gain_batch, void* d_dst, int dst_pitch_bytes, int batch, int h, int w,
                       const int* d_vec, int by, int bx, int block, void* stream) {
    const TnrField field = {d_vec, by, bx, block};
    TmcArgs a;
    dim3 grid;
    if (const int e = temporal_args("rc_raw_temporal_mc", d_src, fmt, desc, d_prev, prev_pitch_bytes, d_gain, gain_batch, d_dst, dst_pitch_bytes, batch, h, w,
                                    &field, &a, &grid)) return e;
    const hipStream_t s = as_stream(stream);
    by_storage(fmt->storage, [&](auto sg) { hipLaunchKernelGGL((temporal_mc_kernel<decltype(sg)::ST, typename decltype(sg)::type>), grid, dim3(kTnrThreads), 0, s, a); });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
