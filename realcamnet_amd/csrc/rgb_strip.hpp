// How a lane reads and writes its pixels of a planar RGB frame, and nothing else: the one reader and writer of the output-stage kernels
// behind the network -- rc_tone_* (tone.hip), rc_lut3d (lut3d.hip), rc_sharpen (sharpen.hip), rc_warp (warp.hip), rc_frame_stats
// (frame_stats.hip), rc_yuv_encode (yuv_encode.hip) and rc_resize (resize.hip).  A frame is (B,3,H,W) of TI = fp32 / bf16 / fp16, planar,
// cropped to (h,w); a result is fp32 or the source's type.  A lane works on kRgbPx consecutive pixels of one row of one plane.  `vec`: the
// lane's kRgbPx elements are one 8- or 16-byte access (the host's vec_src / vec_dst and all kRgbPx inside the row); otherwise the first
// `cnt` elements are accessed one by one, and a load gives 0 for the rest.  Both paths give the same values.  A new output stage includes
// this header: rgb_source / rgb_dest for its checks, by_source / by_source_dest for its launch, rgb_load / rgb_store in its kernel.
#pragma once
#include "common.hpp"

namespace rc {

constexpr int kRgbPx = 4;                        // pixels of a row per lane

__device__ __forceinline__ float rgb_unit(float v) { return v > 0.f ? (v < 1.f ? v : 1.f) : 0.f; }    // into [0, 1]; NaN compares false: 0

// ---- a lane's 4 pixels of one plane, as loaded and as floats ----------------------------------------------------------------------------
template <typename TI> struct RgbRaw { uint32_t w[sizeof(TI) == 4 ? 4 : 2]; };     // the source words: a kernel that needs a row twice keeps these

template <typename TI>
__device__ __forceinline__ RgbRaw<TI> rgb_words(const TI* p, bool vec, int cnt) {
    RgbRaw<TI> r;
    if constexpr (sizeof(TI) == 4) {
        if (vec) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            r.w[0] = v.x; r.w[1] = v.y; r.w[2] = v.z; r.w[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < kRgbPx; ++k) r.w[k] = k < cnt ? __float_as_uint(p[k]) : 0u;
        }
    } else {
        if (vec) {
            const uint2 v = *reinterpret_cast<const uint2*>(p);
            r.w[0] = v.x; r.w[1] = v.y;
        } else {
            const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
            uint32_t e[kRgbPx];
#pragma unroll
            for (int k = 0; k < kRgbPx; ++k) e[k] = k < cnt ? (uint32_t)q[k] : 0u;
            r.w[0] = e[0] | (e[1] << 16); r.w[1] = e[2] | (e[3] << 16);
        }
    }
    return r;
}

template <typename TI>
__device__ __forceinline__ float rgb_pixel(const RgbRaw<TI>& r, int k) {           // pixel k of the words; k is a constant where it is called
    if constexpr (sizeof(TI) == 4) return __uint_as_float(r.w[k]);
    else return (k & 1) ? hi16<TI>(r.w[k >> 1]) : lo16<TI>(r.w[k >> 1]);
}

template <typename TI>
__device__ __forceinline__ void rgb_decode(const RgbRaw<TI>& r, float* f) {
#pragma unroll
    for (int k = 0; k < kRgbPx; ++k) f[k] = rgb_pixel<TI>(r, k);
}

// The two in one step, for a kernel that needs the row once; the element path converts each element as it is.
template <typename TI>
__device__ __forceinline__ void rgb_load(const TI* p, bool vec, int cnt, float* f) {
    if (vec) {
        rgb_decode<TI>(rgb_words<TI>(p, true, kRgbPx), f);
    } else {
#pragma unroll
        for (int k = 0; k < kRgbPx; ++k) f[k] = k < cnt ? to_f32(p[k]) : 0.f;
    }
}

// ---- a lane's 4 results of one plane ----------------------------------------------------------------------------------------------------
template <typename TO>
__device__ __forceinline__ void rgb_store(TO* p, bool vec, int cnt, const float* f) {          // 16-bit results: round to nearest even
    if (vec) {
        if constexpr (sizeof(TO) == 4) {
            *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
            *reinterpret_cast<uint2*>(p) = make_uint2(Vec16<TO>::rne(f[0]) | (Vec16<TO>::rne(f[1]) << 16), Vec16<TO>::rne(f[2]) | (Vec16<TO>::rne(f[3]) << 16));
        }
    } else {
#pragma unroll
        for (int k = 0; k < kRgbPx; ++k)
            if (k < cnt) p[k] = from_f32<TO>(f[k]);
    }
}

// ---- the luma of an RC_MATRIX_* ---------------------------------------------------------------------------------------------------------
struct Luma { float kr, kg, kb; };
struct LumaChroma { Luma k; float sb, sr; };     // and the Cb / Cr scales 0.5 / (1 - Kb), 0.5 / (1 - Kr), which only rc_yuv_encode uses

// Y = ((Kr r) + (Kg g)) + (Kb b), every product and every sum rounded on its own.
__device__ __forceinline__ float rgb_luma(const Luma& k, float r, float g, float b) {
    return __fadd_rn(__fadd_rn(__fmul_rn(k.kr, r), __fmul_rn(k.kg, g)), __fmul_rn(k.kb, b));
}

// Kr, Kb -> Kg, sb, sr in double, each rounded to fp32 once.  The caller has checked the matrix.
inline LumaChroma rgb_coef(int matrix) {
    static const double kKrKb[3][2] = RC_YUV_KR_KB;
    const double kr = kKrKb[matrix][0], kb = kKrKb[matrix][1];
    return {{(float)kr, (float)(1.0 - kr - kb), (float)kb}, (float)(0.5 / (1.0 - kb)), (float)(0.5 / (1.0 - kr))};
}

// ---- the host's dispatch over the element types -----------------------------------------------------------------------------------------
// f(Elem<TI>()) for a checked source dtype; its result is returned (common.hpp's by_dtype, under the name the stages use).
template <typename F>
inline auto by_source(int src_dtype, F&& f) { return by_dtype(src_dtype, f); }

// f(Elem<TI>(), Elem<TO>()) for a checked pair: TO is float or TI.
template <typename F>
inline auto by_source_dest(int src_dtype, int dst_dtype, F&& f) {
    return by_source(src_dtype, [&](auto ti) { return dst_dtype == RC_F32 ? f(ti, Elem<float>()) : f(ti, ti); });
}

// ---- the host's checks of a source and of a destination ---------------------------------------------------------------------------------
struct RgbSide {
    size_t esize;              // bytes per element
    bool vec;                  // the base on a kRgbPx-element boundary and rows of a multiple of kRgbPx: every plane and every row starts on a vector
};

inline RgbSide rgb_side(const void* d, int dtype, int row) {
    const size_t es = dtype_size(dtype);
    return {es, reinterpret_cast<uintptr_t>(d) % (kRgbPx * es) == 0 && row % kRgbPx == 0};
}

// What every entry point that reads `batch` frames (3,H,W) at d_src cropped to (h,w) requires of them; `who` names it in the messages.
// RC_OK, or the error as RC_REQUIRE reports it (a message is formed only for a refusal).  Limits that differ between the entries (frame counts, plane sizes) stay with them.
inline int rgb_source(const char* who, const void* d_src, int src_dtype, int batch, int H, int W, int h, int w, RgbSide* out) {
    RC_REQUIRE(src_dtype == RC_F32 || src_dtype == RC_BF16 || src_dtype == RC_F16, std::string(who) + ": bad source dtype");
    RC_REQUIRE(batch >= 1 && h >= 1 && w >= 1, std::string(who) + ": bad shape (an empty frame)");
    RC_REQUIRE(h <= H && w <= W, std::string(who) + ": bad shape (the crop exceeds the source)");
    *out = rgb_side(d_src, src_dtype, W);
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_src) % out->esize == 0, std::string(who) + ": source misaligned");
    return RC_OK;
}

// The same of the frames written at d_dst, rows of `row` elements: fp32 or the (checked) source's type.
inline int rgb_dest(const char* who, void* d_dst, int dst_dtype, int src_dtype, int row, RgbSide* out) {
    RC_REQUIRE(dst_dtype == RC_F32 || dst_dtype == src_dtype, std::string(who) + ": bad output dtype (fp32 or the source's)");
    *out = rgb_side(d_dst, dst_dtype, row);
    RC_REQUIRE(reinterpret_cast<uintptr_t>(d_dst) % out->esize == 0, std::string(who) + ": destination misaligned");
    return RC_OK;
}

}  // namespace rc
