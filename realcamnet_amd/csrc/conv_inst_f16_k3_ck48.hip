// Instantiations of the MFMA conv kernels: f16_t, 3x3, 48-channel Cin chunks (one file per chunk width so they build in parallel).
#include "conv_kernel.hpp"
namespace rc {
int conv_f16_k3_ck48(int nt, const ConvArgs& a, hipStream_t s) {
    if (nt == 1) return launch_conv<ConvCfg<f16_t, 48, 1, 3>>(a, s);
    if (nt == 3) return launch_conv<ConvCfg<f16_t, 48, 3, 3>>(a, s);
    if (nt == 4) return launch_conv<ConvCfg<f16_t, 48, 4, 3>>(a, s);
    return fail(RC_ERR_UNSUPPORTED, "conv: no kernel instantiation for this cout tile width");
}
}  // namespace rc
