// resample_coords.hpp — the pieces of the reference's float32 coordinate chain that the exact resampling kernels share: the correctly
// rounded division, the normalise round trip (plain: resample_kernel, exact_voxel_coords; folded: resample_tile_kernel, the lean
// exact-coordinate kernels, resample_nearest_exact_kernel), the control-point lerps, the affine row and ATen's corner weights.
// NOT here, each site its own text: the composition ladder, the in-bounds weight, resample_kernel's corner weights.
#pragma once
#include "common.hpp"

namespace tio {

// IEEE-754 correctly rounded n / d from r = RN(1/d): q0 = RN(n r), two Markstein
// refinements (each: exact remainder by FMA, correction by FMA).  Checked
// bit-for-bit against the hardware division on 1.9e9 operands (integer
// divisors 1..2100, spacings in [0.05, 20], exact-multiple neighbourhoods).
__device__ __forceinline__ float exact_div(float n, float d, float r) {
  float q = __fmul_rn(n, r);
  float e = __builtin_fmaf(-d, q, n);
  q = __builtin_fmaf(e, r, q);
  e = __builtin_fmaf(-d, q, n);
  return __builtin_fmaf(e, r, q);
}

// g = 2 v / max(S-1,1) - 1 (spatial.py:1638-1646) followed by ATen's
// grid_sampler_unnormalize(align_corners=True): ((g + 1) / 2) * (S - 1).
__device__ __forceinline__ float normalise_roundtrip(float v, float den, float rden, float size_m1) {
  const float g = __fsub_rn(exact_div(__fmul_rn(2.0f, v), den, rden), 1.0f);
  return __fmul_rn(__fmul_rn(__fadd_rn(g, 1.0f), 0.5f), size_m1);
}

// The same round trip with the two exact scalings folded into the constants: v / (den/2) is the same real quotient as
// 2v / den, and (t * 0.5) * h == t * (0.5 h) because t * 0.5 is exact.  short_div: one
// Markstein refinement is already correctly rounded for every divisor k/2, k <= 8192
// (exhaustive over all mantissas: tests/native/divtest.c).
template <bool SHORT>
__device__ __forceinline__ float normalise_roundtrip_folded(float v, float dh, float rdh, float half_h) {
  float q = __fmul_rn(v, rdh);
  float e = __builtin_fmaf(-dh, q, v);
  q = __builtin_fmaf(e, rdh, q);
  if constexpr (!SHORT) {
    e = __builtin_fmaf(-dh, q, v);
    q = __builtin_fmaf(e, rdh, q);
  }
  const float g = __fsub_rn(q, 1.0f);
  return __fmul_rn(__fadd_rn(g, 1.0f), half_h);
}
// block-uniform choice at run time (the compiler turns it into a select over both results;
// the hot loops branch once outside instead and call the template)
__device__ __forceinline__ float normalise_roundtrip_folded(float v, float dh, float rdh, float half_h, bool short_div) {
  return short_div ? normalise_roundtrip_folded<true>(v, dh, rdh, half_h) : normalise_roundtrip_folded<false>(v, dh, rdh, half_h);
}

// trilinear lookup of the three displacement components from the (ni,nj,nk,3)
// field; nesting and rounding exactly as ATen's upsample_trilinear3d (K innermost)
struct Disp {
  float i, j, k;
};

__device__ __forceinline__ Disp cp_trilerp3(const float* __restrict__ cp, int s_i, int s_j, const Lerp1D& li,
                                            const Lerp1D& lj, const Lerp1D& lk) {
  const float* p00 = cp + li.i0 * s_i + lj.i0 * s_j;
  const float* p01 = cp + li.i0 * s_i + lj.i1 * s_j;
  const float* p10 = cp + li.i1 * s_i + lj.i0 * s_j;
  const float* p11 = cp + li.i1 * s_i + lj.i1 * s_j;
  const int k0 = lk.i0 * 3, k1 = lk.i1 * 3;
  float r[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float a00 = lerp2(p00[k0 + c], lk.l0, p00[k1 + c], lk.l1);
    const float a01 = lerp2(p01[k0 + c], lk.l0, p01[k1 + c], lk.l1);
    const float a10 = lerp2(p10[k0 + c], lk.l0, p10[k1 + c], lk.l1);
    const float a11 = lerp2(p11[k0 + c], lk.l0, p11[k1 + c], lk.l1);
    const float b0 = lerp2(a00, lj.l0, a01, lj.l1);
    const float b1 = lerp2(a10, lj.l0, a11, lj.l1);
    r[c] = lerp2(b0, li.l0, b1, li.l1);
  }
  return Disp{r[0], r[1], r[2]};
}

// one control plane of the displacement field for this thread's (j, k) column:
// the two inner lerps of ATen's upsample_trilinear3d (K innermost, then J)
__device__ __forceinline__ void cp_plane(const float* __restrict__ cp, int ii, int s_i, int s_j, const Lerp1D& lj,
                                         const Lerp1D& lk, float (&P)[3]) {
  const float* p0 = cp + ii * s_i + lj.i0 * s_j;
  const float* p1 = cp + ii * s_i + lj.i1 * s_j;
  const int k0 = lk.i0 * 3, k1 = lk.i1 * 3;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float a0 = lerp2(p0[k0 + c], lk.l0, p0[k1 + c], lk.l1);
    const float a1 = lerp2(p1[k0 + c], lk.l0, p1[k1 + c], lk.l1);
    P[c] = lerp2(a0, lj.l0, a1, lj.l1);
  }
}

// [c,1] @ M^T per row: a*m0, then fma(b,m1,.), fma(c,m2,.), fma(1,m3,.) — the rounding sequence of MKL sgemm (K = 4), pinned against
// the reference.  A macro: a function evaluates its operands in another order, which reorders instructions in 14 kernels.
#define TIO_AFFINE_ROW(M0, M1, M2, M3, A, B, C) \
  __builtin_fmaf(1.0f, M3, __builtin_fmaf(C, M2, __builtin_fmaf(B, M1, __fmul_rn(A, M0))))

// ATen grid_sampler_3d: the eight corner weights in its tap order (bit0 = x+1, bit1 = y+1, bit2 = z+1); operands by reference: by value
// they are read in another order, which reorders instructions in resample_tile_kernel<FAST>
__device__ __forceinline__ void corner_weights(const float& wx0, const float& wx1, const float& wy0, const float& wy1, const float& wz0, const float& wz1, float (&w)[8]) {
  w[0] = __fmul_rn(__fmul_rn(wx0, wy0), wz0);
  w[1] = __fmul_rn(__fmul_rn(wx1, wy0), wz0);
  w[2] = __fmul_rn(__fmul_rn(wx0, wy1), wz0);
  w[3] = __fmul_rn(__fmul_rn(wx1, wy1), wz0);
  w[4] = __fmul_rn(__fmul_rn(wx0, wy0), wz1);
  w[5] = __fmul_rn(__fmul_rn(wx1, wy0), wz1);
  w[6] = __fmul_rn(__fmul_rn(wx0, wy1), wz1);
  w[7] = __fmul_rn(__fmul_rn(wx1, wy1), wz1);
}

}  // namespace tio
