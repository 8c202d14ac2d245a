// Output sharpening between the look and the encoders (include/realcam_hip.h, rc_sharpen): the planar result (B,3,H,W), cropped to (h,w),
// -> (B,3,h,w) planar with its luma detail amplified: an unsharp mask on the luma (3x3 or 5x5 binomial), cored, limited to the range of
// the 3x3 neighbourhood, and added to R, G and B alike.  A streaming stencil: no LDS memory, no atomics, no scratch.
//
// sharpen_kernel: grid (groups of 4 strips, bands of 32 rows, frames), four waves per block, one strip each -- temporal.hip's map.
//   lane map   lane l of a wave holds the 4 consecutive pixels xs + 4 l .. + 3 of a row, of each plane: one load of 8 bytes (16-bit source)
//              or 16 (fp32) per plane and row, one store of 8 / 16 bytes per plane and row.  Rows that start off a vector boundary (a
//              plane width or crop width that is no multiple of 4, a misaligned base) and a row's last partial quad go element by element.
//   columns    the luma at columns x0 - 2, x0 - 1, x0 + 4, x0 + 5 comes from lanes l - 1 and l + 1 (four lane shifts per row, in
//              registers).  At a strip's two ends there is no such lane, so STRIPS OVERLAP: a wave loads 256 columns and produces the 248 of
//              lanes 1 .. 62; lane 0 produces only at the crop's left edge and lane 63 only where the row ends in it.  A lane fills the
//              pixels it holds past the crop's last column with that column's luma, so a neighbour's shift and its own taps see the
//              replicated border without a second path.  64 / 62 = 1.032 x the loads and the arithmetic, no halo load.
//   rows       a wave walks its band downwards and keeps a window of 2 radius + 1 rows in registers: of every row the horizontal binomial
//              sums S (4 registers), of the rows y - 1 .. y + radius the horizontal minimum and maximum of the luma over three columns (8),
//              and of the rows y .. y + radius the luma (4) and THE SOURCE WORDS of r, g, b (6 for a 16-bit source, 12 for fp32), which
//              step 6 decodes a second time when the row has become the centre: nothing is loaded twice by a wave (loading them a second
//              time instead frees 11 to 55 registers and measured 26 to 42 % slower: DESIGN.md 4.p).  The words of the row
//              after the window are in flight while a row is worked on.  Rows above row 0 and below row h - 1 are copies of those rows
//              (a register move, no load).
//   bands      a wave reads radius + 32 + radius rows for 32: 1.125 x the reads at radius 2, 1.0625 x at radius 1.
// 32-bit element offsets below a 64-bit frame base (the entry point checks).  The arithmetic is step for step the header's: every product,
// sum and difference rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn: no contraction whatever the compile flags say), so the vector
// path, the element path and a plain elementwise restatement give the same bits.  Every tap is clamped to the crop: nothing outside
// (h, w) is ever read.
#include "rgb_strip.hpp"

#include <cmath>

namespace rc {

constexpr int kShPx = 4, kShWaves = 4, kShThreads = 64 * kShWaves;
static_assert(kShPx == kRgbPx, "a lane holds one rgb_strip.hpp strip");
constexpr int kShSpan = 64 * kShPx;               // columns a wave loads
constexpr int kShOut = kShSpan - 2 * kShPx;       // columns it produces inside a row: strips start this far apart
constexpr int kShRows = 32;                       // rows per band

struct SharpenArgs {
    int H, W, h, w;            // source plane, cropped / output plane
    int vec_src, vec_dst;      // every source row segment / every destination quad starts on a vector boundary
    Luma k;
    float amount, core, over;
};

// The source words of a lane's 4 pixels of the three planes, as loaded (rgb_strip.hpp) ...
template <typename TI> struct ShPx { RgbRaw<TI> c[3]; };

// ... and step 1 of them: float(src), NaN -> 0, clamped to [0, 1].
template <typename TI>
__device__ __forceinline__ void sh_decode(const ShPx<TI>& px, float (*f)[kShPx]) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int k = 0; k < kShPx; ++k) f[p][k] = rgb_unit(rgb_pixel<TI>(px.c[p], k));
    }
}

// A row as a wave holds it.  Which fields of which window row are live is in the header comment; the rest is dead and costs no register.
template <typename TI> struct ShRow { float S[kShPx], L[kShPx], mn[kShPx], mx[kShPx]; ShPx<TI> px; };

// The binomial of five (radius 2) or three (radius 1) values in the header's order of additions; m is the centre.
template <int R>
__device__ __forceinline__ float sh_binomial(float m2, float m1, float m, float p1, float p2) {
    if constexpr (R == 1) {
        return __fadd_rn(__fadd_rn(m1, p1), __fmul_rn(2.f, m));
    } else {
        return __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(m2, p2), __fmul_rn(2.f, m)), __fmul_rn(4.f, m)), __fmul_rn(4.f, __fadd_rn(m1, p1)));
    }
}

template <typename TI, typename TO, int R>
__global__ void __launch_bounds__(kShThreads) sharpen_kernel(SharpenArgs a, const TI* __restrict__ src, TO* __restrict__ dst) {
    constexpr int kWin = 2 * R + 1;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int strip = blockIdx.x * kShWaves + wv, frame = blockIdx.z;
    const int xs = strip * kShOut;
    if (strip > 0 && xs + 2 * kShPx >= a.w) return;                                // wave-uniform: the strip before holds the row's end
    const int x0 = xs + lane * kShPx;
    const int n = x0 < a.w ? min(a.w - x0, kShPx) : 0;
    const bool act = n > 0, wide = n == kShPx;
    const bool first = x0 == 0, more = x0 + kShPx < a.w;                           // no columns to the left / columns to the right
    const bool owns = act && (lane > 0 || first) && (lane < 63 || !more);          // this lane's results are stored
    const bool vin = wide && a.vec_src, vout = wide && a.vec_dst;
    const int r0 = blockIdx.y * kShRows, r1 = min(r0 + kShRows, a.h);              // r0 < h: the grid has ceil(h / kShRows) bands
    const uint32_t splane = (uint32_t)a.H * (uint32_t)a.W, dplane = (uint32_t)a.h * (uint32_t)a.w;
    const TI* s = src + (size_t)frame * 3 * (size_t)splane;
    TO* d = dst + (size_t)frame * 3 * (size_t)dplane;

    auto load = [&](int y) {
        ShPx<TI> r = {};
        if (act) {
            const uint32_t o = (uint32_t)y * (uint32_t)a.W + (uint32_t)x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) r.c[c] = rgb_words<TI>(s + (c * splane + o), vin, n);
        }
        return r;
    };

    // the rows this wave reads: r0 - R .. r1 - 1 + R, clamped to the crop
    const int y_end = min(r1 - 1 + R, a.h - 1);
    int yr = max(r0 - R, 0);                                                       // the row whose words are in flight
    ShPx<TI> ahead = load(yr);

    auto next_row = [&](ShRow<TI>& o) {                                            // every lane of the wave runs this: the shifts need them all
        o.px = ahead;
        ++yr;
        if (yr <= y_end) ahead = load(yr);                                         // in flight while this row is worked on
        float c[3][kShPx];
        sh_decode<TI>(o.px, c);
#pragma unroll
        for (int k = 0; k < kShPx; ++k) o.L[k] = rgb_luma(a.k, c[0][k], c[1][k], c[2][k]);
#pragma unroll
        for (int k = 1; k < kShPx; ++k) o.L[k] = k < n ? o.L[k] : o.L[k - 1];     // past the crop's last column: that column
        const float l2 = __shfl_up(o.L[2], 1), l3 = __shfl_up(o.L[3], 1), q0 = __shfl_down(o.L[0], 1), q1 = __shfl_down(o.L[1], 1);
        float e[kShPx + 4];                                                        // the luma at columns x0 - 2 .. x0 + 5, clamped to the crop
        e[0] = first ? o.L[0] : l2; e[1] = first ? o.L[0] : l3;
#pragma unroll
        for (int k = 0; k < kShPx; ++k) e[2 + k] = o.L[k];
        e[6] = more ? q0 : o.L[3]; e[7] = more ? q1 : o.L[3];
#pragma unroll
        for (int k = 0; k < kShPx; ++k) {
            o.S[k] = sh_binomial<R>(e[k], e[k + 1], e[k + 2], e[k + 3], e[k + 4]);
            o.mn[k] = fminf(fminf(e[k + 1], e[k + 2]), e[k + 3]);
            o.mx[k] = fmaxf(fmaxf(e[k + 1], e[k + 2]), e[k + 3]);
        }
    };

    const float norm = R == 1 ? 0.0625f : 0.00390625f;
    auto emit = [&](int y, const ShRow<TI>* w) {
        const ShRow<TI>& m = w[R];
        float c[3][kShPx], o[3][kShPx];
        sh_decode<TI>(m.px, c);
#pragma unroll
        for (int k = 0; k < kShPx; ++k) {
            const float T = sh_binomial<R>(w[0].S[k], w[R - 1].S[k], m.S[k], w[R + 1].S[k], w[kWin - 1].S[k]);
            const float blur = __fmul_rn(T, norm);
            const float lo = fminf(fminf(w[R - 1].mn[k], m.mn[k]), w[R + 1].mn[k]);
            const float hi = fmaxf(fmaxf(w[R - 1].mx[k], m.mx[k]), w[R + 1].mx[k]);
            const float L = m.L[k];
            const float dd = __fsub_rn(L, blur);
            const float cc = fmaxf(__fsub_rn(fabsf(dd), a.core), 0.f);
            const float e = __fmul_rn(a.amount, copysignf(cc, dd));
            float t = __fadd_rn(L, e);
            t = fminf(t, __fadd_rn(hi, a.over));
            t = fmaxf(t, __fsub_rn(lo, a.over));
            const float e2 = __fsub_rn(t, L);
#pragma unroll
            for (int p = 0; p < 3; ++p) o[p][k] = fminf(fmaxf(__fadd_rn(c[p][k], e2), 0.f), 1.f);
        }
        if (owns) {
            const uint32_t off = (uint32_t)y * (uint32_t)a.w + (uint32_t)x0;
#pragma unroll
            for (int p = 0; p < 3; ++p) rgb_store<TO>(d + (p * dplane + off), vout, n, o[p]);
        }
    };

    // the window of row r0: rows r0 - R .. r0 + R, clamped; a row that the clamp repeats is a copy of the one before it
    ShRow<TI> w[kWin];
    next_row(w[0]);
#pragma unroll
    for (int k = 1; k < kWin; ++k) {
        const int want = min(max(r0 - R + k, 0), a.h - 1);                         // wave-uniform
        if (want >= yr) next_row(w[k]);                                            // yr - 1 is the last row worked out
        else w[k] = w[k - 1];
    }
    for (int y = r0;; ++y) {
        emit(y, w);
        if (y + 1 >= r1) break;
#pragma unroll
        for (int k = 0; k + 1 < kWin; ++k) w[k] = w[k + 1];
        if (min(y + 1 + R, a.h - 1) >= yr) next_row(w[kWin - 1]);                  // else the crop's last row again: w[kWin - 1] stays
    }
}

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_sharpen_desc_size(void) { return sizeof(rc_sharpen_desc); }

int rc_sharpen(const void* d_src, int src_dtype, void* d_dst, int dst_dtype, const rc_sharpen_desc* desc, int batch, int H, int W, int h, int w, void* stream) {
    RC_REQUIRE(d_src && d_dst && desc, "rc_sharpen: null pointer");
    RgbSide src, dst;
    if (int e = rgb_source("rc_sharpen", d_src, src_dtype, batch, H, W, h, w, &src)) return e;
    if (int e = rgb_dest("rc_sharpen", d_dst, dst_dtype, src_dtype, w, &dst)) return e;
    RC_REQUIRE(desc->radius == 1 || desc->radius == 2, "rc_sharpen: radius must be 1 or 2");
    RC_REQUIRE(desc->matrix >= 0 && desc->matrix <= 2, "rc_sharpen: bad matrix");
    RC_REQUIRE(std::isfinite(desc->amount) && desc->amount >= 0.f && desc->amount <= 8.f, "rc_sharpen: amount must be finite and lie in [0, 8]");
    RC_REQUIRE(std::isfinite(desc->core) && desc->core >= 0.f && desc->core <= 1.f, "rc_sharpen: core must be finite and lie in [0, 1]");
    RC_REQUIRE(std::isfinite(desc->overshoot) && desc->overshoot >= 0.f && desc->overshoot <= 1.f, "rc_sharpen: overshoot must be finite and lie in [0, 1]");
    const long long ss = (long long)src.esize, ds = (long long)dst.esize;
    // a frame's element offsets are formed in 32 bits
    RC_REQUIRE(3LL * H * W * ss <= 0x7fffffffLL && 3LL * h * w * ds <= 0x7fffffffLL, "rc_sharpen: a frame's three planes (source, destination) must stay below 2 GiB");
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), s1 = s0 + (uintptr_t)(3LL * H * W * ss * batch);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_dst), o1 = o0 + (uintptr_t)(3LL * h * w * ds * batch);
    RC_REQUIRE(s1 <= o0 || o1 <= s0, "rc_sharpen: dst overlaps src (a pixel's neighbours are read after it is written)");

    SharpenArgs a;
    a.H = H; a.W = W; a.h = h; a.w = w;
    a.vec_src = src.vec; a.vec_dst = dst.vec;
    a.k = rgb_coef(desc->matrix).k;
    a.amount = desc->amount; a.core = desc->core; a.over = desc->overshoot;
    const int strips = 1 + (w > kShSpan ? ceil_div(w - kShSpan, kShOut) : 0);
    const dim3 grid((unsigned)ceil_div(strips, kShWaves), (unsigned)ceil_div(h, kShRows), (unsigned)batch), block(kShThreads);
    RC_REQUIRE(grid.y <= 65535u && grid.z <= 65535u, "rc_sharpen: more than 65535 frames or 2097120 rows");
    const hipStream_t st = as_stream(stream);
    by_source_dest(src_dtype, dst_dtype, [&](auto ti, auto to) {
        typedef typename decltype(ti)::type TI;
        typedef typename decltype(to)::type TO;
        if (desc->radius == 1) hipLaunchKernelGGL((sharpen_kernel<TI, TO, 1>), grid, block, 0, st, a, static_cast<const TI*>(d_src), static_cast<TO*>(d_dst));
        else hipLaunchKernelGGL((sharpen_kernel<TI, TO, 2>), grid, block, 0, st, a, static_cast<const TI*>(d_src), static_cast<TO*>(d_dst));
    });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
