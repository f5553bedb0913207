// philox_normal.hpp — the fast-mode normal stream (Philox4x32-10 + Box-Muller), shared by intensity.hip (tio_add_noise,
// tio_philox_normal), the stencil (stencil_march.hpp, stencil.hip: the fused noise) and labels_to_image.hip: one definition, one stream.
#pragma once

#include "common.hpp"

namespace tio {

// =============================================================================
// Philox4x32-10 + Box-Muller (fast noise mode; definition in oracle/tio_oracle.c)
// =============================================================================
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; round++) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c[0];
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c[2];
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = static_cast<uint32_t>(p1);
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = static_cast<uint32_t>(p0);
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// sin and cos of 2 pi u, u in (0, 1), in plain IEEE float32 operations (the oracle runs the SAME sequence: bit-identical).
// Round 5: the hardware units (v_sin_f32 / v_cos_f32, argument in revolutions) are good to ~1e-6 absolute; times the radius
// and the noise's std that is a few 1e-7 of the intensity range — the size of the north-star bar READ PER VOXEL at a voxel
// whose value the noise has brought close to zero (1e-4 x 1e-3 range): scripts/r5_headline_error_budget.py measured the whole
// pipeline without Noise at 4.5e-7 of that bar and with it at 1.02, whatever the resampler and the stencil did.  Quadrant
// q = rint(4 u), f = 4 u - q in [-1/2, 1/2] (both exact), Taylor polynomials of sin / cos(pi/2 f) through f^9 / f^8
// (truncation 1.7e-9 / 2.5e-8): 8.6e-8 absolute against the true value over all 2^24 arguments.
__device__ __forceinline__ void sincos_rev(float u, float& sn, float& cs) {
  const float t = __fmul_rn(u, 4.0f);
  const float q = rintf(t);
  const float f = __fsub_rn(t, q);
  const float w = __fmul_rn(f, f);
  float p = __builtin_fmaf(0.00016044118478735982f, w, -0.004681754135318688f);
  p = __builtin_fmaf(p, w, 0.07969262624616704f);
  p = __builtin_fmaf(p, w, -0.6459640975062462f);
  p = __builtin_fmaf(p, w, 1.5707963267948966f);
  const float s0 = __fmul_rn(p, f);
  float c = __builtin_fmaf(0.0009192602748394263f, w, -0.020863480763352960f);
  c = __builtin_fmaf(c, w, 0.25366950790104797f);
  c = __builtin_fmaf(c, w, -1.2337005501361697f);
  c = __builtin_fmaf(c, w, 1.0f);
  const int qi = static_cast<int>(q) & 3;
  const float a = (qi & 1) ? c : s0, b = (qi & 1) ? s0 : c;
  sn = (qi & 2) ? -a : a;
  cs = ((qi + 1) & 2) ? -b : b;
}

__device__ __forceinline__ void philox_normal4(uint64_t seed, int stream_id, uint64_t q, float z[4]) {
  uint32_t c[4] = {static_cast<uint32_t>(q), static_cast<uint32_t>(q >> 32), static_cast<uint32_t>(stream_id), 0u};
  philox4x32_10(c, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float u1 = __fmul_rn(__fadd_rn(static_cast<float>(c[2 * h] >> 8), 0.5f), 1.0f / 16777216.0f);
    const float u2 = __fmul_rn(__fadd_rn(static_cast<float>(c[2 * h + 1] >> 8), 0.5f), 1.0f / 16777216.0f);
    // -2 ln(u1) through the hardware log2 / sqrt units (u1 in (0, 1): no special cases; one ulp each: the radius is
    // within ~2e-7 relative of libm's)
    const float nl = __fmul_rn(-1.3862943611198906f, __builtin_amdgcn_logf(u1));  // -2 ln 2 * log2(u1)
    const float radius = __builtin_amdgcn_sqrtf(fmaxf(nl, 0.0f));
    float cs, sn;
    sincos_rev(u2, sn, cs);
    z[2 * h] = __fmul_rn(radius, cs);
    z[2 * h + 1] = __fmul_rn(radius, sn);
  }
}

}  // namespace tio
