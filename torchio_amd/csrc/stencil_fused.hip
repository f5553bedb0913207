// stencil_fused.hip — the fused J + K instantiations of conv_march_kernel and of its streaming form conv_stream_march_kernel
// (stencil_march.hpp), alone in a translation unit because they are compiled without the SLP vectoriser (see the Makefile):
// paired into v_pk_fma_f32, the K taps at odd window offsets and the taps held in scalar registers cost register-pair moves, and
// the kernels spilled scalar registers.  The source, the arithmetic and the tap order are those of every other instantiation;
// the launcher in stencil.hip (plan_conv, launch_streams) decides what is launched and calls in here with its decision.
#include "stencil_march.hpp"

namespace tio {

void launch_conv_march_fused(int radius_class, int post_noise, bool fma, bool stream_policy, dim3 grid, size_t lds, hipStream_t stream, const ConvArgs& a) {
  with_march_radius(radius_class, [&](auto radius_tag) {
    with_bools([&](auto fm) {
      constexpr int R = decltype(radius_tag)::value;
      constexpr bool FM = decltype(fm)::value;
      if (stream_policy) {
        if (post_noise == 2) hipLaunchKernelGGL((conv_stream_march_kernel<R, true, false, 2, FM>), grid, dim3(kBlock), lds, stream, a);
        else if (post_noise != 0) hipLaunchKernelGGL((conv_stream_march_kernel<R, true, false, 1, FM>), grid, dim3(kBlock), lds, stream, a);
        else hipLaunchKernelGGL((conv_stream_march_kernel<R, true, false, 0, FM>), grid, dim3(kBlock), lds, stream, a);
      } else {
        if (post_noise == 2) hipLaunchKernelGGL((conv_march_kernel<R, true, false, 2, FM>), grid, dim3(kBlock), lds, stream, a);
        else if (post_noise != 0) hipLaunchKernelGGL((conv_march_kernel<R, true, false, 1, FM>), grid, dim3(kBlock), lds, stream, a);
        else hipLaunchKernelGGL((conv_march_kernel<R, true, false, 0, FM>), grid, dim3(kBlock), lds, stream, a);
      }
    }, fma);
  });
}

}  // namespace tio
