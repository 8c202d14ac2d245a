// Scaled and cropped renditions of the network's result (include/realcam_hip.h, rc_resize_taps / rc_resize): a separable downscale of a
// window of the planar (B,3,H,W) result to (B,3,h,w), between the tail and the encoders.
//
// rc_resize_taps (host): per output index of one axis the first source index and a short list of non-negative weights that sum to 1
// ("area": fractional coverage; "bilinear": the antialiased triangle), computed in double without contraction and rounded to fp32 once.
//
// resize_kernel: a block owns kRsRows x kRsCols outputs of one plane of one frame.  Pass 1 writes the horizontal sums of the source rows
// the tile needs -- straight from global memory -- into a static LDS array t[row][column] of fp32; pass 2 sums t down the rows.  In both
// passes a wave's 64 lanes are 64 neighbouring output columns, so every LDS access is one dword per lane at consecutive addresses
// (conflict free), and the vertical weights are wave uniform.  Neighbouring row tiles recompute the rows their windows share.
// Arithmetic: fp32, every product and every sum rounded on its own (__fmul_rn / __fadd_rn), in list order; the zero weights that pad a
// list to the axis's longest are skipped, not multiplied (0 x inf would be NaN).
#include <cmath>
#include <vector>

#include "rgb_strip.hpp"

namespace rc {

constexpr int kRsCols = 64, kRsRows = 8, kRsWaves = 4, kRsThreads = kRsCols * kRsWaves, kRsBatch = 4;
constexpr int kRsWindow = kRsRows * RC_RESIZE_MAX_RATIO + RC_RESIZE_MAX_TAPS;      // source rows under 8 output rows: (8 - 1) ratio + 1 + taps <= this

struct ResizeArgs {
    int H, W, h, w;            // source plane, output plane
    int ty, tx;                // padded list lengths
};

// Taps k and k + 1 of kRsBatch source rows: all 2 x kRsBatch loads are issued before the first sum needs one.
template <typename TI, bool FIRST>
__device__ __forceinline__ void row_taps(const ResizeArgs& a, const float (*wxs)[kRsCols], int lane, int fx, int k, const TI* const* line, float* s) {
    const float w0 = wxs[k][lane], w1 = k + 1 < a.tx ? wxs[k + 1][lane] : 0.f;
    const int c0 = min(max(fx + k, 0), a.W - 1), c1 = min(max(fx + k + 1, 0), a.W - 1);
    float x0[kRsBatch], x1[kRsBatch];
#pragma unroll
    for (int u = 0; u < kRsBatch; ++u) {
        x0[u] = to_f32(line[u][c0]);
        x1[u] = to_f32(line[u][c1]);
    }
#pragma unroll
    for (int u = 0; u < kRsBatch; ++u) {
        const float p0 = __fmul_rn(w0, x0[u]), p1 = __fmul_rn(w1, x1[u]);
        const float s0 = FIRST ? p0 : (w0 != 0.f ? __fadd_rn(s[u], p0) : s[u]);
        s[u] = w1 != 0.f ? __fadd_rn(s0, p1) : s0;
    }
}

template <typename TI, typename TO>
__global__ void __launch_bounds__(kRsThreads) resize_kernel(ResizeArgs a, const TI* __restrict__ src, TO* __restrict__ dst, const int* __restrict__ first_y,
                                                            const float* __restrict__ wy, const int* __restrict__ first_x, const float* __restrict__ wx) {
    __shared__ float t[kRsWindow][kRsCols];
    __shared__ float wxs[RC_RESIZE_MAX_TAPS][kRsCols];
    const int lane = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(threadIdx.y);      // a wave is one threadIdx.y: its table reads are scalar loads
    const int j = blockIdx.x * kRsCols + lane, i0 = blockIdx.y * kRsRows;
    const bool col = j < a.w;
    const int i1 = min(i0 + kRsRows, a.h) - 1;                                    // the tile's last output row
    const int row0 = first_y[i0];
    const int nrow = min(first_y[i1] + a.ty - row0, kRsWindow);                   // its window of source rows (the tail may be padding only)
    const int fx = col ? first_x[j] : 0;
    for (int k = wave; k < a.tx; k += kRsWaves) wxs[k][lane] = col ? wx[(size_t)j * a.tx + k] : 0.f;
    __syncthreads();

    // Indices are clamped into the plane / the window: tables from rc_resize_taps never need it for a tap that counts, a padding tap's
    // operand is loaded from the clamped place and dropped, and tables that are not from rc_resize_taps cannot make the kernel read
    // outside its buffers.
    // pass 1: t[r][lane] = (..((w0 x0) + (w1 x1)) + ..) of source row row0 + r, kRsBatch rows of a wave at a time: their loads are
    // independent, so a wave has kRsBatch of them in flight per tap instead of one (the pass is bound by load latency otherwise)
    const TI* plane = src + (size_t)blockIdx.z * a.H * a.W;
    if (col) {
        for (int rb = wave * kRsBatch; rb < nrow; rb += kRsWaves * kRsBatch) {
            const TI* line[kRsBatch];
            float s[kRsBatch];
#pragma unroll
            for (int u = 0; u < kRsBatch; ++u)
                line[u] = plane + (size_t)min(max(row0 + rb + u, 0), a.H - 1) * a.W;      // past the plane or the window: a valid line, and a sum nothing uses
            row_taps<TI, true>(a, wxs, lane, fx, 0, line, s);                             // the sum starts as the first product, not as 0 + it
            for (int k = 2; k < a.tx; k += 2) row_taps<TI, false>(a, wxs, lane, fx, k, line, s);
#pragma unroll
            for (int u = 0; u < kRsBatch; ++u)
                if (rb + u < nrow) t[rb + u][lane] = s[u];
        }
    }
    __syncthreads();

    // pass 2: the same sum down the rows of t
    if (col) {
        for (int i = i0 + wave; i <= i1; i += kRsWaves) {
            const float* w = wy + (size_t)i * a.ty;
            const int r0 = first_y[i] - row0;
            float s = __fmul_rn(w[0], t[min(max(r0, 0), kRsWindow - 1)][lane]);
#pragma unroll 4
            for (int k = 1; k < a.ty; ++k) {
                const float wk = w[k];
                const float v = __fadd_rn(s, __fmul_rn(wk, t[min(max(r0 + k, 0), kRsWindow - 1)][lane]));
                s = wk != 0.f ? v : s;
            }
            dst[((size_t)blockIdx.z * a.h + i) * a.w + j] = from_f32<TO>(s);
        }
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

int rc_resize_taps(int filter, int n, int off, int m, int* first, float* weights, int* taps) {
#pragma clang fp contract(off)
    RC_REQUIRE(first && weights && taps, "rc_resize_taps: null pointer");
    RC_REQUIRE(filter == RC_FILTER_AREA || filter == RC_FILTER_BILINEAR, "rc_resize_taps: unknown filter");
    RC_REQUIRE(n >= 1 && m >= 1 && off >= 0, "rc_resize_taps: bad lengths");
    RC_REQUIRE(m <= n, "rc_resize_taps: upscaling (the stage downscales or keeps the size: ratio >= 1)");
    RC_REQUIRE((long long)n <= (long long)RC_RESIZE_MAX_RATIO * m, "rc_resize_taps: ratio above the limit of 8");
    const double s = (double)n / (double)m;
    std::vector<double> w((size_t)m * RC_RESIZE_MAX_TAPS, 0.0);
    std::vector<int> cnt(m);
    int longest = 0;
    for (int i = 0; i < m; ++i) {
        double v[4 * RC_RESIZE_MAX_TAPS];
        int k0, k1;                                                               // source indices k0 .. k1 - 1, inside [0, n)
        if (filter == RC_FILTER_AREA) {
            const double lo = (double)i * s, hi = (double)(i + 1) * s;
            k0 = (int)std::floor(lo);
            k1 = (int)std::ceil(hi);
            if (k1 > n) k1 = n;
            RC_REQUIRE(k1 - k0 <= 4 * RC_RESIZE_MAX_TAPS, "rc_resize_taps: list longer than 20 taps");
            for (int k = k0; k < k1; ++k) {
                const double c = std::fmin((double)(k + 1), hi) - std::fmax((double)k, lo);
                v[k - k0] = std::fmax(0.0, c);
            }
        } else {
            const double c = s * ((double)i + 0.5);
            k0 = (int)(c - s + 0.5);
            if (k0 < 0) k0 = 0;
            k1 = (int)(c + s + 0.5);
            if (k1 > n) k1 = n;
            RC_REQUIRE(k1 - k0 <= 4 * RC_RESIZE_MAX_TAPS, "rc_resize_taps: list longer than 20 taps");
            for (int k = k0; k < k1; ++k) v[k - k0] = std::fmax(0.0, 1.0 - std::fabs(((double)k - c + 0.5) / s));
        }
        while (k1 > k0 && v[k1 - 1 - k0] == 0.0) --k1;                            // zero weights at either end are dropped
        int lead = 0;
        while (k0 + lead < k1 && v[lead] == 0.0) ++lead;
        const int c = k1 - k0 - lead;
        RC_REQUIRE(c >= 1, "rc_resize_taps: an output index without a source");
        RC_REQUIRE(c <= RC_RESIZE_MAX_TAPS, "rc_resize_taps: list longer than 20 taps");
        double sum = 0.0;
        for (int k = 0; k < c; ++k) sum += v[lead + k];
        for (int k = 0; k < c; ++k) w[(size_t)i * RC_RESIZE_MAX_TAPS + k] = v[lead + k] / sum;
        first[i] = off + k0 + lead;
        cnt[i] = c;
        if (c > longest) longest = c;
    }
    for (int i = 0; i < m; ++i)
        for (int k = 0; k < longest; ++k) weights[(size_t)i * longest + k] = k < cnt[i] ? (float)w[(size_t)i * RC_RESIZE_MAX_TAPS + k] : 0.f;
    *taps = longest;
    return RC_OK;
}

int rc_resize(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, int batch, int H, int W, int h, int w, const int* d_first_y, const float* d_wy,
              int taps_y, const int* d_first_x, const float* d_wx, int taps_x, void* stream) {
    RC_REQUIRE(d_src && d_dst && d_first_y && d_wy && d_first_x && d_wx, "rc_resize: null pointer");
    RgbSide src, dst;                                                             // the stage downscales or keeps the size: its output is a crop's size
    if (int e = rgb_source("rc_resize", d_src, src_dtype, batch, H, W, h, w, &src)) return e;
    if (int e = rgb_dest("rc_resize", d_dst, dst_dtype, src_dtype, w, &dst)) return e;
    RC_REQUIRE(taps_y >= 1 && taps_x >= 1 && taps_y <= RC_RESIZE_MAX_TAPS && taps_x <= RC_RESIZE_MAX_TAPS, "rc_resize: tap length outside 1 .. 20");
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_first_y) % 4 == 0 && reinterpret_cast<uintptr_t>(d_wy) % 4 == 0 &&
               reinterpret_cast<uintptr_t>(d_first_x) % 4 == 0 && reinterpret_cast<uintptr_t>(d_wx) % 4 == 0, "rc_resize: misaligned pointer");
    const dim3 grid(ceil_div(w, kRsCols), ceil_div(h, kRsRows), (unsigned)batch * 3u);
    RC_REQUIRE(grid.y <= 65535u && batch <= 21845, "rc_resize: more than 21845 frames or 524280 output rows");
    ResizeArgs a;
    a.H = H; a.W = W; a.h = h; a.w = w; a.ty = taps_y; a.tx = taps_x;
    by_source_dest(src_dtype, dst_dtype, [&](auto ti, auto to) {
        typedef typename decltype(ti)::type TI;
        typedef typename decltype(to)::type TO;
        hipLaunchKernelGGL((resize_kernel<TI, TO>), grid, dim3(kRsCols, kRsWaves), 0, as_stream(stream), a, static_cast<const TI*>(d_src), static_cast<TO*>(d_dst), d_first_y, d_wy, d_first_x, d_wx);
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
