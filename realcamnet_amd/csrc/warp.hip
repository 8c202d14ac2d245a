// Geometric correction in front of the scaler (include/realcam_hip.h, rc_warp): the planar result (B,3,H,W), cropped to the frame (h,w),
// resampled through a coarse mesh of source positions -> (B,3,oh,ow) planar.  Replaces F.grid_sample on the float result: no dense grid
// in HBM, no fp32 copy of the frame.
//
// warp_kernel (the gather form): a lane owns kWarpPx = 4 consecutive output pixels of one row; a block is 64 such strips (one wave) x 4
// rows, the grid is (column tiles, row tiles, frames), so no index is ever divided.  A strip starts on a multiple of 4 and a cell is at
// least 8 wide: the four pixels share one cell, whose four nodes are four 8-byte loads that the lanes of the same cell (2 to 16 of them)
// share through L1.  Per pixel the tap indices are clamped into the frame first, then every tap load is issued -- all 12 of a bilinear
// pixel (the strip's 48 together), all 48 of a bicubic pixel (one pixel at a time) -- before the first weighted sum needs one; CONSTANT
// replaces a tap that was outside by the fill after the load, so the loads never depend on the border rule.  One vector store per plane
// where every strip starts on a vector boundary; otherwise (odd widths, a row's last partial strip) element stores of the same values.
// Taps are read through L1 / L2 from global memory: no LDS, no scratch.
// Arithmetic: fp32, every product, sum and difference rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn: no contraction whatever the
// compile flags say), so the vector path, the element path and a plain elementwise restatement give the same bits.
#include "rgb_strip.hpp"

#include <cmath>

namespace rc {

constexpr int kWarpPx = kRgbPx, kWarpStrips = 64, kWarpRows = 4;

struct WarpArgs {
    int H, W, h, w;            // source plane, the frame inside it
    int oh, ow;                // output plane
    int cell_log2, gw;         // nodes per mesh row
    long long mesh_stride;     // nodes from one frame's mesh to the next (0: one mesh for every frame)
    float inv_cell;            // 1 / cell, exact
    float xmax, ymax;          // float(w + 1), float(h + 1): the guard's upper ends
    float fill[3];
    int vec_dst;               // every destination strip starts on a vector boundary
};

__device__ __forceinline__ float warp_lerp(float a, float b, float t, float omt) { return __fadd_rn(__fmul_rn(omt, a), __fmul_rn(t, b)); }

// Step 2: NaN -> -2, then into [-2, hi].
__device__ __forceinline__ float warp_guard(float s, float hi) {
    s = s == s ? s : -2.f;
    return fminf(fmaxf(s, -2.f), hi);
}

__device__ __forceinline__ float warp_c1(float x) { return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(1.25f, x), 2.25f), x), x), 1.f); }
__device__ __forceinline__ float warp_c2(float x) {
    return __fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(-0.75f, x), 3.75f), x), 6.f), x), 3.f);
}

// One axis of steps 3 and 4: the NT weights, the NT indices clamped into [0, n), and bit k of `in` set when tap k was inside.
template <int NT>
__device__ __forceinline__ void warp_axis(float s, int n, float* wt, int* idx, unsigned& in) {
    const float fl = floorf(s);
    const int i0 = (int)fl;                                                        // s lies in [-2, n + 1]: the conversion is exact
    const float t = __fsub_rn(s, fl);
    int first;
    if constexpr (NT == 2) {
        first = i0;
        wt[0] = __fsub_rn(1.f, t);
        wt[1] = t;
    } else {
        first = i0 - 1;
        wt[0] = warp_c2(__fadd_rn(t, 1.f));
        wt[1] = warp_c1(t);
        wt[2] = warp_c1(__fsub_rn(1.f, t));
        wt[3] = warp_c2(__fsub_rn(2.f, t));
    }
    in = 0;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const int i = first + k;
        idx[k] = min(max(i, 0), n - 1);
        in |= (unsigned)(i == idx[k]) << k;
    }
}

// One output pixel at column x of a row whose fraction is v: steps 1 to 5 -> px[3].  NT taps per axis: 2 bilinear, 4 bicubic.  CONSTANT: a tap
// outside the frame is the fill, else it reads the clamped index.
template <typename TI, int NT, bool CONSTANT>
__device__ __forceinline__ void warp_pixel(const WarpArgs& a, const TI* __restrict__ s, size_t splane, float2 m00, float2 m10, float2 m01, float2 m11, float v, float omv,
                                           int x, float* px) {
    const float u = __fmul_rn((float)(x & ((1 << a.cell_log2) - 1)), a.inv_cell), omu = __fsub_rn(1.f, u);
    const float sx = warp_guard(warp_lerp(warp_lerp(m00.x, m10.x, u, omu), warp_lerp(m01.x, m11.x, u, omu), v, omv), a.xmax);
    const float sy = warp_guard(warp_lerp(warp_lerp(m00.y, m10.y, u, omu), warp_lerp(m01.y, m11.y, u, omu), v, omv), a.ymax);
    float wx[NT], wy[NT];
    int ix[NT], iy[NT];
    unsigned inx, iny;
    warp_axis<NT>(sx, a.w, wx, ix, inx);
    warp_axis<NT>(sy, a.h, wy, iy, iny);
    // byte offsets inside a plane: below 2^31 (a plane holds at most 2^29 - 1 samples, checked by rc_warp), so a tap's address is the
    // plane's uniform base and one 32-bit register
    unsigned row[NT], col[NT];
#pragma unroll
    for (int r = 0; r < NT; ++r) row[r] = (unsigned)(iy[r] * a.W) * (unsigned)sizeof(TI);
#pragma unroll
    for (int q = 0; q < NT; ++q) col[q] = (unsigned)ix[q] * (unsigned)sizeof(TI);
    TI raw[3][NT][NT];                                                             // every tap load of the pixel, then the sums
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const char* plane = reinterpret_cast<const char*>(s + c * splane);
#pragma unroll
        for (int r = 0; r < NT; ++r)
#pragma unroll
            for (int q = 0; q < NT; ++q) raw[c][r][q] = *reinterpret_cast<const TI*>(plane + (row[r] + col[q]));
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float o = 0.f;
#pragma unroll
        for (int r = 0; r < NT; ++r) {
            float rr = 0.f;
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                float t = to_f32(raw[c][r][q]);
                if constexpr (CONSTANT) t = ((inx >> q) & (iny >> r) & 1u) ? t : a.fill[c];
                const float p = __fmul_rn(wx[q], t);
                rr = q == 0 ? p : __fadd_rn(rr, p);
            }
            const float p = __fmul_rn(wy[r], rr);
            o = r == 0 ? p : __fadd_rn(o, p);
        }
        px[c] = o;
    }
}

template <typename TI, typename TO, int NT, bool CONSTANT>
__global__ void __launch_bounds__(kWarpStrips * kWarpRows) warp_kernel(WarpArgs a, const TI* __restrict__ src, TO* __restrict__ dst, const float2* __restrict__ mesh) {
    const int x0 = (blockIdx.x * kWarpStrips + threadIdx.x) * kWarpPx, y = blockIdx.y * kWarpRows + threadIdx.y;
    if (x0 >= a.ow || y >= a.oh) return;
    const int frame = blockIdx.z, cnt = min(a.ow - x0, kWarpPx);
    const size_t splane = (size_t)a.H * a.W, dplane = (size_t)a.oh * a.ow;
    const TI* s = src + (size_t)frame * 3 * splane;
    TO* d = dst + (size_t)frame * 3 * dplane + (size_t)y * a.ow + x0;

    // step 1: the cell's four nodes (i + 1 <= Gw - 1 and j + 1 <= Gh - 1 by the mesh's size) and the row's fraction
    const int i = x0 >> a.cell_log2, j = y >> a.cell_log2;
    const float2* m = mesh + (size_t)frame * a.mesh_stride + (size_t)j * a.gw + i;
    const float2 m00 = m[0], m10 = m[1], m01 = m[a.gw], m11 = m[a.gw + 1];
    const float v = __fmul_rn((float)(y & ((1 << a.cell_log2) - 1)), a.inv_cell), omv = __fsub_rn(1.f, v);

    // a pixel past the row's end is computed (its cell is the strip's and its reads are in bounds) and dropped
    float o[3][kWarpPx] = {};
    if constexpr (NT == 2) {                                                       // bilinear: the four pixels' 48 loads in flight together
#pragma unroll
        for (int k = 0; k < kWarpPx; ++k) {
            float px[3];
            warp_pixel<TI, NT, CONSTANT>(a, s, splane, m00, m10, m01, m11, v, omv, x0 + k, px);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c][k] = px[c];
        }
    } else {                                                                       // bicubic: one pixel's 48 loads at a time, or the registers run out
#pragma unroll 1
        for (int k = 0; k < kWarpPx; ++k) {
            float px[3];
            warp_pixel<TI, NT, CONSTANT>(a, s, splane, m00, m10, m01, m11, v, omv, x0 + k, px);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int e = 0; e < kWarpPx; ++e) o[c][e] = e == k ? px[c] : o[c][e];      // k is uniform: selects, no indexed registers
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb_store<TO>(d + c * dplane, a.vec_dst && cnt == kWarpPx, cnt, o[c]);
}

template <typename TI, typename TO>
static void warp_launch(const WarpArgs& a, int interp, int border, dim3 grid, hipStream_t st, const void* d_src, void* d_dst, const float* d_mesh) {
    const dim3 block(kWarpStrips, kWarpRows);
    const TI* src = static_cast<const TI*>(d_src);
    TO* dst = static_cast<TO*>(d_dst);
    const float2* mesh = reinterpret_cast<const float2*>(d_mesh);
    if (interp == RC_WARP_BILINEAR) {
        if (border == RC_WARP_CLAMP) hipLaunchKernelGGL((warp_kernel<TI, TO, 2, false>), grid, block, 0, st, a, src, dst, mesh);
        else hipLaunchKernelGGL((warp_kernel<TI, TO, 2, true>), grid, block, 0, st, a, src, dst, mesh);
    } else {
        if (border == RC_WARP_CLAMP) hipLaunchKernelGGL((warp_kernel<TI, TO, 4, false>), grid, block, 0, st, a, src, dst, mesh);
        else hipLaunchKernelGGL((warp_kernel<TI, TO, 4, true>), grid, block, 0, st, a, src, dst, mesh);
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

int rc_warp(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, const float* d_mesh, int mesh_batch, int cell_log2, int interp,
            int border, float fill_r, float fill_g, float fill_b, int batch, int H, int W, int h, int w, int oh, int ow, void* stream) {
    RC_REQUIRE(interp == RC_WARP_BILINEAR || interp == RC_WARP_BICUBIC, "rc_warp: bad interp (bilinear or bicubic)");
    RC_REQUIRE(border == RC_WARP_CLAMP || border == RC_WARP_CONSTANT, "rc_warp: bad border (clamp or constant)");
    RC_REQUIRE(cell_log2 >= RC_WARP_MIN_CELL_LOG2 && cell_log2 <= RC_WARP_MAX_CELL_LOG2, "rc_warp: bad cell (8, 16, 32 or 64: cell_log2 3 .. 6)");
    RC_REQUIRE(std::isfinite(fill_r) && std::isfinite(fill_g) && std::isfinite(fill_b), "rc_warp: the fill must be finite");
    RC_REQUIRE(d_src && d_dst && d_mesh, "rc_warp: null pointer");
    RgbSide src, dst;
    if (int e = rgb_source("rc_warp", d_src, src_dtype, batch, H, W, h, w, &src)) return e;
    if (int e = rgb_dest("rc_warp", d_dst, dst_dtype, src_dtype, ow, &dst)) return e;
    RC_REQUIRE(oh >= 1 && ow >= 1, "rc_warp: bad shape (an empty output)");
    RC_REQUIRE(H <= RC_WARP_MAX_DIM && W <= RC_WARP_MAX_DIM && oh <= RC_WARP_MAX_DIM && ow <= RC_WARP_MAX_DIM && (long long)H * W < (1LL << 29),
               "rc_warp: bad shape (a dimension above 2^23 or a source plane of 2^29 samples or more)");
    RC_REQUIRE(mesh_batch == 1 || mesh_batch == batch, "rc_warp: mesh_batch must be 1 or the batch");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_mesh) % 8 == 0, "rc_warp: the mesh must be 8-byte aligned");
    const int cell = 1 << cell_log2;
    WarpArgs a;
    a.H = H; a.W = W; a.h = h; a.w = w; a.oh = oh; a.ow = ow;
    a.cell_log2 = cell_log2;
    a.gw = ceil_div(ow, cell) + 1;
    a.mesh_stride = mesh_batch == 1 ? 0 : (long long)a.gw * (ceil_div(oh, cell) + 1);
    a.inv_cell = 1.f / (float)cell;
    a.xmax = (float)(w + 1); a.ymax = (float)(h + 1);
    a.fill[0] = fill_r; a.fill[1] = fill_g; a.fill[2] = fill_b;
    a.vec_dst = dst.vec;
    const dim3 grid(ceil_div(ow, kWarpStrips * kWarpPx), ceil_div(oh, kWarpRows), (unsigned)batch);
    RC_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "rc_warp: more than 65535 frames or 262140 output rows");
    const hipStream_t st = as_stream(stream);
    by_source_dest(src_dtype, dst_dtype, [&](auto ti, auto to) {
        warp_launch<typename decltype(ti)::type, typename decltype(to)::type>(a, interp, border, grid, st, d_src, d_dst, d_mesh);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
