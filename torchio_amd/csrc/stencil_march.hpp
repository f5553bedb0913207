// stencil_march.hpp - the register-window marching kernel of the separable stencil (axes I and J, radii <= 8) and its
// argument block.  A header because the kernel's two families are compiled in two translation units with different code
// generation (see the Makefile): stencil.hip holds the plain I / J and the bias-on-load instantiations and every other
// stencil kernel, stencil_fused.hip the fused J + K ones.  The launcher in stencil.hip decides; this file decides nothing.
#pragma once

#include "common.hpp"
#include "philox_normal.hpp"

namespace tio {

constexpr int kBlock = 256;

struct ConvArgs {
  const void* src;
  void* dst;
  const void* x_orig;  // the original input (skip rows are copied from it bit-exactly)
  const float* taps;
  const uint8_t* skip;
  int I, J, K;
  int channels;
  int axis, radius;
  int taps_batched, tap_stride;
  int orig_dtype;
  int last_pass;
  int tiles_a;  // tiles along the stencil axis (axes I, J) / row groups (axis K)
  int bcs;      // B * C (register-window marching kernel: strips are enumerated per wave)
  int radius_k;  // > 0: the J pass also applies the K taps to every row it produces (fused J+K)
  // tio_blur_fused: BiasField folded into the loads of the I pass, Noise into the stores of the last pass
  const float* bias_coarse;          // (B, C, ci, cj, ck) or nullptr
  int bias_ci, bias_cj, bias_ck;
  float bias_si, bias_sj, bias_sk;   // ATen lerp scales of the coarse grid
  int noise_on, noise_batched;
  float noise_mean, noise_std;
  const float* noise_mean_b;
  const float* noise_std_b;
  uint64_t noise_seed;
  const float* noise_base;  // noise_on == 2: the normal draws of every element, laid out like the data (the reference's seeded stream)
  // tio_blur_fused(fast_math = 1): the taps of the marching kernel accumulate with fused multiply-adds (one rounding per
  // tap instead of the reference's two: results within float rounding, ~1e-7 relative — the J+K pass is bound by vector
  // instructions, not by memory, and the taps are two thirds of them)
  int fma;
};

// ---- float32 fast path for radii <= 8: the stencil window lives in registers ---------------
// Along I or J a lane only ever needs ITS OWN column's history, so nothing has to be shared:
// every wave marches alone down one (other, b, c) strip of 256 K positions (one float4 per
// lane) with the last 2R+1 rows in VGPRs.  The marching loop is unrolled by the window length,
// which turns the rotating window into compile-time register names (no moves, no LDS ring, no
// block barrier); two rows of 16-byte loads are in flight per lane.  Arithmetic and tap order
// are those of the generic kernels.  LDS is only used by the fused K stage (one row per wave).
constexpr int kMarchMaxRadius = 8;
#ifndef TIO_MARCH_AHEAD
#define TIO_MARCH_AHEAD 2
#endif
constexpr int kMarchAhead = TIO_MARCH_AHEAD;

// (the fused J + K instantiations of the usual radii are held to 128 registers — four waves per SIMD: with explicit draws the
// R = 6 one needed 130, one wave per SIMD less)
// FMA (tio_blur_fused(fast_math = 1)) is a template parameter: as a block-uniform branch both forms of every tap sat in the
// W-times unrolled loop — 12 600 lines of assembly, more than the instruction cache holds.
// STREAM (the launcher's cache policy, launch_streams in common.hpp): the rows this pass reads and the rows it writes go by once —
// at volumes no cache holds, the consumer of a row comes by after the Infinity Cache has turned over.  Row loads and row
// stores then carry the nontemporal policy (`nt`: the lines are first to be evicted); the taps, the coarse bias field and
// everything else keep the default.  ONE text (stencil_march_kernel.inc), two __global__ families that differ in this constant
// alone.  Not a __device__ function template called from both: built that way — by reference and by value, always inlined —
// eleven of the eighty non-streaming instantiations came out with other register counts than before the policy existed
// (<3, false, true, 0, *> 130 -> 132 VGPRs, beyond what tests/test_stencil_kernel_resources.py allows), and the policy's promise
// is that a launch below the threshold runs the code it ran before.  Included as text, conv_march_kernel is token for token what
// it was, and tests/test_cache_policy_resources.py holds every instantiation of both families to the same registers.
#define TIO_MARCH_KERNEL conv_march_kernel
#define TIO_MARCH_STREAM false
#include "stencil_march_kernel.inc"
#undef TIO_MARCH_KERNEL
#undef TIO_MARCH_STREAM
#define TIO_MARCH_KERNEL conv_stream_march_kernel
#define TIO_MARCH_STREAM true
#include "stencil_march_kernel.inc"
#undef TIO_MARCH_KERNEL
#undef TIO_MARCH_STREAM

// run-time radius class -> template argument: f is called with std::integral_constant<int, R> for radius_class R = 1 .. 7,
// and with R = kMarchMaxRadius for every other value (both launchers instantiate all eight: the boolean template arguments
// go through with_bools, common.hpp)
template <typename F>
void with_march_radius(int radius_class, F f) {
  switch (radius_class) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, kMarchMaxRadius>{}); break;
  }
}

// The fused J + K instantiations <R, true, false, post_noise, fma> (stencil_fused.hip): radius_class 1 .. 8, post_noise 0 / 1 / 2.
void launch_conv_march_fused(int radius_class, int post_noise, bool fma, bool stream_policy, dim3 grid, size_t lds, hipStream_t stream, const ConvArgs& a);

}  // namespace tio
