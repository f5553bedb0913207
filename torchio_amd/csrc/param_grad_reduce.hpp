// param_grad_reduce.hpp — the reduction skeleton of intensity_param_grad.hip: per-lane float64 accumulators -> wave (shuffles) ->
// block (LDS, fixed order) -> one float64 hardware atomic per value and block into the caller's workspace -> a finishing kernel
// that sums the workspace slots in a fixed order and rounds ONCE to float32.  (resample_geometry_grad.hip's structure, with the
// wave level in float64 as well.)
#pragma once

#include "common.hpp"

namespace tio {

constexpr int kPgBlock = 256;   // threads per block of every parameter-gradient kernel
constexpr int kPgWaves = kPgBlock / 64;
constexpr int kPgSpread = 16;   // workspace slots per output group: block partials of one group queue on 16 cache lines, not one
constexpr int kPgMaxBlocks = 1024;  // blocks per batch element (grid-stride loops): bounds the atomics per output value

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) v += __shfl_xor(v, offset, 64);
  return v;
}

// The block's sums of acc[0 .. n_used) are added to slot[0 .. n_used): one atomic per non-zero value.  Every thread of the block
// calls this (it holds a barrier).
template <int N>
__device__ __forceinline__ void block_sum_to_workspace(const double (&acc)[N], int n_used, double* slot) {
  __shared__ double s_part[kPgWaves][N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < N; t++) {
    if (t < n_used) {  // (uniform)
      const double total = wave_sum_f64(acc[t]);
      if (lane == 0) s_part[wave][t] = total;
    }
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < n_used) {
    double total = 0.0;
    for (int w = 0; w < kPgWaves; w++) total += s_part[w][threadIdx.x];
    if (total != 0.0) unsafeAtomicAdd(slot + threadIdx.x, total);
  }
}

// out[g * out_stride + e] = float32(sum over s < spread of ws[(g * spread + s) * slot_doubles + e]), g < groups, e < n
__global__ void param_grad_finish_kernel(const double* __restrict__ ws, float* __restrict__ out, int64_t groups, int64_t n, int spread,
                                         int64_t slot_doubles, int64_t out_stride) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= groups * n) return;
  const int64_t g = t / n, e = t - g * n;
  const double* p = ws + g * spread * slot_doubles + e;
  double total = 0.0;
  for (int s = 0; s < spread; s++) total += p[s * slot_doubles];
  out[g * out_stride + e] = static_cast<float>(total);
}

inline void launch_param_grad_finish(const double* ws, float* out, int64_t groups, int64_t n, int spread, int64_t slot_doubles,
                                     int64_t out_stride, hipStream_t s) {
  const int64_t threads = groups * n;
  if (threads <= 0) return;
  hipLaunchKernelGGL(param_grad_finish_kernel, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, ws, out, groups, n, spread,
                     slot_doubles, out_stride);
}

}  // namespace tio
