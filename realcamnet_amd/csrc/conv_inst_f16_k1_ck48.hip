// Instantiations of the MFMA conv kernels: f16_t, 1x1, 48-channel Cin chunks (no 80-wide cout tiles: those serve the GroupMix Linears, which have no fp16 form).
#include "conv_kernel.hpp"
namespace rc {
int conv_f16_k1_ck48(int nt, const ConvArgs& a, hipStream_t s) {
    if (nt == 1) return launch_conv<ConvCfg<f16_t, 48, 1, 1>>(a, s);
    if (nt == 3) return launch_conv<ConvCfg<f16_t, 48, 3, 1>>(a, s);
    if (nt == 4) return launch_conv<ConvCfg<f16_t, 48, 4, 1>>(a, s);
    return fail(RC_ERR_UNSUPPORTED, "conv: no kernel instantiation for this cout tile width");
}
}  // namespace rc
