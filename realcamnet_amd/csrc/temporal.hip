// Temporal noise reduction on the mosaic (include/realcam_hip.h, rc_raw_temporal): one sensor frame as delivered (any storage, padded lines) and
// the last filtered frame (B, 2h, 2w) fp32 -> the filtered frame (B, 2h, 2w) fp32 in the frame's code units.  The filter -- its lane map,
// strips, bands, arithmetic and the entry's checks -- is temporal_kernel.hpp's, shared with temporal_mc.hip; this kernel reads the state
// where it lies.  No LDS memory, no atomics.
#include "temporal_kernel.hpp"

namespace rc {

template <int ST, typename TI>
__global__ void __launch_bounds__(kTnrThreads) raw_temporal_kernel(TnrArgs a) { temporal_body<ST, TI, false>(a); }

}  // namespace rc

using namespace rc;

extern "C" {

size_t rc_temporal_desc_size(void) { return sizeof(rc_temporal_desc); }

int rc_raw_temporal(const void* d_src, const rc_raw_format* fmt, const rc_temporal_desc* desc, const float* d_prev, int prev_pitch_bytes,
                    const float* d_gain, int gain_batch, void* d_dst, int dst_pitch_bytes, int batch, int h, int w, void* stream) {
    TmcArgs args;
    dim3 grid;
    if (const int e = temporal_args("rc_raw_temporal", d_src, fmt, desc, d_prev, prev_pitch_bytes, d_gain, gain_batch, d_dst, dst_pitch_bytes, batch, h, w,
                                    nullptr, &args, &grid)) return e;
    const TnrArgs a = args;                                                        // no field: the plain part
    const hipStream_t s = as_stream(stream);
    by_storage(fmt->storage, [&](auto sg) { hipLaunchKernelGGL((raw_temporal_kernel<decltype(sg)::ST, typename decltype(sg)::type>), grid, dim3(kTnrThreads), 0, s, a); });
    RC_HIP_CHECK(hipGetLastError());
    return RC_OK;
}

}  // extern "C"
