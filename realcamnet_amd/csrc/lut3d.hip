// Colour looks between the scaler and the encoders (include/realcam_hip.h, rc_lut3d): the planar result (B,3,H,W), cropped to (h,w),
// through a 3D LUT of n x n x n nodes with tetrahedral interpolation -> (B,3,h,w) planar.
//
// lut3d_kernel: a lane owns kLutPx = 4 consecutive pixels of one row; a block is 64 such strips (one wave) x 4 rows, the grid is
// (column tiles, row tiles, frames), so no index is ever divided.  A lane loads its 4 pixels of each plane as one vector (8 bytes of a
// 16-bit source, 16 of fp32), works out the four vertices of each pixel's tetrahedron, issues all 16 vertex gathers -- one 16-byte load
// each, the table holds R,G,B and a pad float per node -- before the first weighted sum needs one, and stores one vector per plane.
// Rows that do not start on a vector boundary (odd widths, odd crops) and a row's last partial strip take element loads / stores with
// the same values.  The table is read through L1 / L2 from global memory: no LDS, no scratch.
//
// lut3d_lds_kernel (n <= kLutLdsMax = 17: the table is at most 78.6 KB): the same strip, bit for bit, with the table in LDS.  One block of
// 16 waves per CU copies the table in once and then walks tiles of 256 strips x 4 rows (one division per tile, none per pixel); a
// vertex is one ds_read of 12 bytes.  Measured against the gather form in the same interleaved run: 0.77 of its time on
// a network output, 0.34 on uniform-random data.
// Arithmetic: fp32, every product and every sum rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn: no contraction whatever the
// compile flags say), so the vector path, the element path and a plain elementwise restatement give the same bits.  The node indices
// are clamped to [0, n - 2] after the NaN rule: no input makes the kernel read outside the table.
#include "rgb_strip.hpp"

namespace rc {

constexpr int kLutPx = kRgbPx, kLutStrips = 64, kLutRows = 4, kLutThreads = kLutStrips * kLutRows;
constexpr int kLutLdsMax = 17, kLutLdsStrips = 256, kLutLdsThreads = kLutLdsStrips * kLutRows;     // the LDS form: tables up to 17^3 x 16 bytes, blocks of 16 waves

struct Lut3dArgs {
    int H, W, h, w;            // source plane, cropped / output plane
    int n;                     // nodes per axis
    float scale;               // float(n - 1)
    int vec_src, vec_dst;      // every source row segment / every destination strip starts on a vector boundary
};

// One channel's node index and fraction: p = c (n - 1), i = min(int(floor(p)), n - 2), f = p - i (exact).
__device__ __forceinline__ void lut_cell(float c, const Lut3dArgs& a, int& i, float& f) {
    const float p = __fmul_rn(rgb_unit(c), a.scale);
    i = min((int)p, a.n - 2);                                                      // p >= 0: truncation is floor
    f = __fsub_rn(p, (float)i);
}

// rgb_strip.hpp's load, except that an fp32 vector is read in place: copied into words first (rgb_load), the two fp32 kernels wait twice
// more for memory and run 9 % slower on 1080p and 720p fp32 frames (profiles/output_strip_refactor.md).
template <typename TI>
__device__ __forceinline__ void lut_load(const TI* p, bool vec, int cnt, float* f) {
    if constexpr (sizeof(TI) == 4) {
        if (vec) {
            const float4& v = *reinterpret_cast<const float4*>(p);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
            return;
        }
    }
    rgb_load<TI>(p, vec, cnt, f);
}

template <typename TI, typename TO>
__device__ __forceinline__ void lut3d_strip(const Lut3dArgs& a, const TI* __restrict__ src, TO* __restrict__ dst, const float4* lut, int x0, int y, int frame) {
    const int cnt = min(a.w - x0, kLutPx);
    const size_t splane = (size_t)a.H * a.W, dplane = (size_t)a.h * a.w;
    const TI* s = src + (size_t)frame * 3 * splane + (size_t)y * a.W + x0;
    TO* d = dst + (size_t)frame * 3 * dplane + (size_t)y * a.w + x0;

    float px[3][kLutPx];
#pragma unroll
    for (int c = 0; c < 3; ++c) lut_load<TI>(s + c * splane, a.vec_src && cnt == kLutPx, cnt, px[c]);

    const int sg = a.n, sb = a.n * a.n;                                            // node (ir, ig, ib) is entry ir + n (ig + n ib)
    float4 v[kLutPx][4];
    float wt[kLutPx][4];
#pragma unroll
    for (int k = 0; k < kLutPx; ++k) {                                             // a pixel past the row's end is 0: node 0, read and dropped
        int ir, ig, ib;
        float fr, fg, fb;
        lut_cell(px[0][k], a, ir, fr);
        lut_cell(px[1][k], a, ig, fg);
        lut_cell(px[2][k], a, ib, fb);
        // the axes in the order of their fractions, ties as the header fixes them: f1 >= f2 >= f3, o1 / o2 the steps to V1 / V2
        float f1, f2, f3;
        int o1, o2;
        if (fr >= fg) {
            if (fg >= fb)      { f1 = fr; f2 = fg; f3 = fb; o1 = 1;  o2 = 1 + sg; }     // r, g, b
            else if (fr >= fb) { f1 = fr; f2 = fb; f3 = fg; o1 = 1;  o2 = 1 + sb; }     // r, b, g
            else               { f1 = fb; f2 = fr; f3 = fg; o1 = sb; o2 = sb + 1; }     // b, r, g
        } else {
            if (fb >= fg)      { f1 = fb; f2 = fg; f3 = fr; o1 = sb; o2 = sb + sg; }    // b, g, r
            else if (fb >= fr) { f1 = fg; f2 = fb; f3 = fr; o1 = sg; o2 = sg + sb; }    // g, b, r
            else               { f1 = fg; f2 = fr; f3 = fb; o1 = sg; o2 = sg + 1; }     // g, r, b
        }
        const int i0 = ir + a.n * (ig + a.n * ib);
        v[k][0] = lut[i0];
        v[k][1] = lut[i0 + o1];
        v[k][2] = lut[i0 + o2];
        v[k][3] = lut[i0 + 1 + sg + sb];
        wt[k][0] = __fsub_rn(1.f, f1);
        wt[k][1] = __fsub_rn(f1, f2);
        wt[k][2] = __fsub_rn(f2, f3);
        wt[k][3] = f3;
    }

    float o[3][kLutPx];
#pragma unroll
    for (int k = 0; k < kLutPx; ++k) {
#define RC_LUT_MIX(m) __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(wt[k][0], v[k][0].m), __fmul_rn(wt[k][1], v[k][1].m)), __fmul_rn(wt[k][2], v[k][2].m)), __fmul_rn(wt[k][3], v[k][3].m))
        o[0][k] = RC_LUT_MIX(x);
        o[1][k] = RC_LUT_MIX(y);
        o[2][k] = RC_LUT_MIX(z);
#undef RC_LUT_MIX
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb_store<TO>(d + c * dplane, a.vec_dst && cnt == kLutPx, cnt, o[c]);
}

template <typename TI, typename TO>
__global__ void __launch_bounds__(kLutThreads) lut3d_kernel(Lut3dArgs a, const TI* __restrict__ src, TO* __restrict__ dst, const float4* __restrict__ lut) {
    const int x0 = (blockIdx.x * kLutStrips + threadIdx.x) * kLutPx, y = blockIdx.y * kLutRows + threadIdx.y;
    if (x0 >= a.w || y >= a.h) return;
    lut3d_strip<TI, TO>(a, src, dst, lut, x0, y, blockIdx.z);
}

// The table in LDS: a persistent block per CU, tiles of kLutLdsStrips strips x kLutRows rows in the order (frame, row tile, column tile).
template <typename TI, typename TO>
__global__ void __launch_bounds__(kLutLdsThreads) lut3d_lds_kernel(Lut3dArgs a, int ctiles, int per_frame, int total, const TI* __restrict__ src, TO* __restrict__ dst,
                                                                   const float4* __restrict__ lut) {
    extern __shared__ float4 lut_lds[];
    const int n3 = a.n * a.n * a.n;
    for (int i = threadIdx.y * kLutLdsStrips + threadIdx.x; i < n3; i += kLutLdsThreads) lut_lds[i] = lut[i];
    __syncthreads();
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const int f = t / per_frame, r = t - f * per_frame, rt = r / ctiles, ct = r - rt * ctiles;
        const int x0 = (ct * kLutLdsStrips + threadIdx.x) * kLutPx, y = rt * kLutRows + threadIdx.y;
        if (x0 < a.w && y < a.h) lut3d_strip<TI, TO>(a, src, dst, lut_lds, x0, y, f);
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

int rc_lut3d(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, const float* d_lut, int n, int batch, int H, int W, int h, int w, void* stream) {
    RC_REQUIRE(n >= RC_LUT3D_MIN_SIZE && n <= RC_LUT3D_MAX_SIZE, "rc_lut3d: table size outside 2 .. 65");
    RC_REQUIRE(d_src && d_dst && d_lut, "rc_lut3d: null pointer");
    RgbSide src, dst;
    if (int e = rgb_source("rc_lut3d", d_src, src_dtype, batch, H, W, h, w, &src)) return e;
    if (int e = rgb_dest("rc_lut3d", d_dst, dst_dtype, src_dtype, w, &dst)) return e;
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_lut) % 16 == 0, "rc_lut3d: the table must be 16-byte aligned");
    Lut3dArgs a;
    a.H = H; a.W = W; a.h = h; a.w = w; a.n = n; a.scale = (float)(n - 1);
    a.vec_src = src.vec; a.vec_dst = dst.vec;
    const dim3 grid(ceil_div(w, kLutStrips * kLutPx), ceil_div(h, kLutRows), (unsigned)batch);
    RC_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "rc_lut3d: more than 65535 frames or 262140 rows");
    const float4* lut = reinterpret_cast<const float4*>(d_lut);
    const long long ctiles = ceil_div(w, kLutLdsStrips * kLutPx), per_frame = ctiles * grid.y, total = per_frame * batch;
    const bool in_lds = n <= kLutLdsMax && total <= 0x7fffffffLL;
    return by_source_dest(src_dtype, dst_dtype, [&](auto ti, auto to) {
        typedef typename decltype(ti)::type TI;
        typedef typename decltype(to)::type TO;
        const TI* s = static_cast<const TI*>(d_src);
        TO* d = static_cast<TO*>(d_dst);
        if (in_lds) {
            const dim3 lgrid((unsigned)(total < device_cu_count() ? total : device_cu_count())), lblock(kLutLdsStrips, kLutRows);
            return launch_lds<&lut3d_lds_kernel<TI, TO>>(lgrid, lblock, n * n * n * (int)sizeof(float4), as_stream(stream), a, (int)ctiles, (int)per_frame, (int)total, s, d, lut);
        }
        hipLaunchKernelGGL((lut3d_kernel<TI, TO>), grid, dim3(kLutStrips, kLutRows), 0, as_stream(stream), a, s, d, lut);
        RC_HIP_CHECK(hipGetLastError());
        return (int)RC_OK;
    });
}

}  // extern "C"
