// The sample step the encoders behind the network share (include/realcam_hip.h, rc_yuv_encode): r,g,b -> unquantised Y', Cb, Cr and a value
// -> its integer code.  rc_yuv_encode (yuv_encode.hip) and rc_jpeg_encode (jpeg.hip) both form their samples with these two functions, so a
// JPEG's samples are the I420 / BT.601 / full-range / centre-sited surface's samples bit for bit.
#pragma once
#include "rgb_strip.hpp"

namespace rc {

__device__ __forceinline__ uint32_t code(float v, float s, float o, float lo, float hi) {
    float q = rintf(__fadd_rn(__fmul_rn(v, s), o));             // round half to even
    q = q < lo ? lo : (q > hi ? hi : q);
    return (uint32_t)q;
}

__device__ __forceinline__ void ycc(const LumaChroma& c, float r, float g, float b, float& y, float& cb, float& cr) {
    r = rgb_unit(r); g = rgb_unit(g); b = rgb_unit(b);
    y = rgb_luma(c.k, r, g, b);
    cb = __fmul_rn(__fsub_rn(b, y), c.sb);
    cr = __fmul_rn(__fsub_rn(r, y), c.sr);
}

}  // namespace rc
