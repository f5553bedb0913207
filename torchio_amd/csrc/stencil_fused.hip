// stencil_fused.hip — the fused J + K instantiations of conv_march_kernel (stencil_march.hpp), alone in a translation
// unit because they are compiled without the SLP vectoriser (see the Makefile): paired into v_pk_fma_f32, the K taps at odd
// window offsets and the taps held in scalar registers cost register-pair moves, and the kernels spilled scalar registers.
// The source, the arithmetic and the tap order are those of every other instantiation; the launcher in intensity.hip
// (plan_conv) decides what is launched and calls in here with its decision.
#include "stencil_march.hpp"

namespace tio {

void launch_conv_march_fused(int radius_class, int post_noise, bool fma, dim3 grid, size_t lds, hipStream_t stream, const ConvArgs& a) {
#define TIO_FUSED_VARIANT_F(RR, FM)                                                                                              \
  {                                                                                                                              \
    if (post_noise == 2) hipLaunchKernelGGL((conv_march_kernel<RR, true, false, 2, FM>), grid, dim3(kBlock), lds, stream, a);     \
    else if (post_noise != 0) hipLaunchKernelGGL((conv_march_kernel<RR, true, false, 1, FM>), grid, dim3(kBlock), lds, stream, a); \
    else hipLaunchKernelGGL((conv_march_kernel<RR, true, false, 0, FM>), grid, dim3(kBlock), lds, stream, a);                     \
  }
#define TIO_FUSED_VARIANT(RR)                                                          \
  {                                                                                    \
    if (fma) { TIO_FUSED_VARIANT_F(RR, true) } else { TIO_FUSED_VARIANT_F(RR, false) } \
  }
  switch (radius_class) {
    case 1: TIO_FUSED_VARIANT(1) break;
    case 2: TIO_FUSED_VARIANT(2) break;
    case 3: TIO_FUSED_VARIANT(3) break;
    case 4: TIO_FUSED_VARIANT(4) break;
    case 5: TIO_FUSED_VARIANT(5) break;
    case 6: TIO_FUSED_VARIANT(6) break;
    case 7: TIO_FUSED_VARIANT(7) break;
    default: TIO_FUSED_VARIANT(8) break;
  }
#undef TIO_FUSED_VARIANT
#undef TIO_FUSED_VARIANT_F
}

}  // namespace tio
