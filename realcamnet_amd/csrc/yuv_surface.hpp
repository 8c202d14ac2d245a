// The professional video surfaces of rc_yuv_encode (include/realcam_hip.h, the layouts from RC_YUV_NV16 on): what yuv_encode.hip's entry
// points call for them.  The kernels and the surface plan are in yuv_surface.hip.
#pragma once
#include "rgb_strip.hpp"

namespace rc {

inline bool yuv_surface_layout(int layout) { return layout >= RC_YUV_NV16 && layout <= RC_YUV_V210; }

// nullptr and the bytes of one (h, w) frame, or what is wrong with the format.
const char* yuv_surface_plan(const rc_out_format* f, int h, int w, long long* frame_bytes);

// rc_yuv_encode for these layouts; the caller has checked the pointers and the source (rgb_source).
int yuv_surface_encode(const void* d_src, int src_dtype, const rc_out_format* fmt, void* d_dst, int batch, int H, int W, int h, int w, void* stream);

}  // namespace rc
