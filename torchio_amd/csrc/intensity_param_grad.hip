// intensity_param_grad.hip — the gradients of the intensity transforms with respect to their PARAMETERS:
//   tio_bias_field_grad              d / d(coarse grid)     of tio_bias_field_apply   (bias_field.py:237-244 under autograd)
//   tio_gamma_grad                   d / d(gamma)           of tio_gamma_pow          (sign(x) |x|^gamma)
//   tio_noise_grad                   d / d(mean), d / d(std) of tio_add_noise         (x + (mean + std z); Rician)
//   tio_separable_conv3d_taps_grad   d / d(taps)            of tio_separable_conv3d   (blur.py:157-252)
// Every one is a reduction of the volume into a handful of numbers: one read of x and of the incoming gradient, no per-voxel
// intermediate in memory (the tap gradient keeps the two scratch volumes of the stencil passes it needs).
//
// Common to the four.  gy is float32, shaped like the forward's output.  Each term is formed in float32 from the forward's own
// float32 values (y before its store rounds it, the same lerp weights, the same expf / powf); float64 data takes the forward's
// float64 expressions where the forward has them (gamma, noise) and is narrowed once where the term is a product (bias, taps).
// A term is widened to float64 as soon as it exists and summed in float64: per lane, across the wave by shuffles, across the
// block through LDS, across blocks by float64 hardware atomics into the caller's workspace (param_grad_reduce.hpp); a finishing
// kernel rounds once to float32.  Two runs differ at most in the last float32 rounding of an output.  Flagged rows add exactly
// zero; parameters shared across the batch receive the sum over the batch; outputs are fully overwritten.
#include <stdint.h>

#include <type_traits>

#include "param_grad_reduce.hpp"
#include "philox_normal.hpp"

namespace tio {
namespace {

constexpr int kSlotDoubles = 16;  // gamma (1 used) and noise (2 used): one 128-byte line per slot

// =============================================================================
// BiasField: d_coarse[b,c,n] = s * sum_v gy[v] * y[v] * W(n; v)
// =============================================================================
// The block shape is bias_kernel's: 64 lanes along K, one wave per J row, kBiasTileI slabs.  i / j nodes and weights are the
// wave's, so per k node the K-lerp is reduced across the wave (float64 shuffles) before 4 lanes apply the (2 x 2) I / J weights and
// add into the block's float64 LDS box of the nodes its tile can touch; the box is flushed once, non-zero entries only.  A tile
// whose box exceeds kBoxDoubles, or that spans more than kMaxWaveNodes k nodes (a coarse grid nearly as fine as the volume), adds
// its eight values per voxel to the workspace directly.
constexpr int kBiasTileI = 8;
constexpr int kBiasRows = 4;
constexpr int kBoxDoubles = 1536;   // 12 KiB
constexpr int kMaxWaveNodes = 8;    // k nodes per 64-lane tile on the box road: one wave reduction each

struct BiasGradArgs {
  const void* x;
  const float* gy;
  const float* coarse;
  double* ws;  // (B * C, ci * cj * ck)
  const uint8_t* skip;
  int channels, I, J, K, ci, cj, ck, divide, tiles_i;
  float scale_i, scale_j, scale_k;
};

template <int DT>
__global__ __launch_bounds__(kPgBlock) void bias_grad_kernel(const BiasGradArgs a) {
  __shared__ double s_box[kBoxDoubles];
  const int it = blockIdx.z % a.tiles_i;
  const int bc = blockIdx.z / a.tiles_i;
  const int b = bc / a.channels;
  if (a.skip != nullptr && a.skip[b] != 0) return;  // block-uniform: the forward copied this element
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int j_raw = blockIdx.y * kBiasRows + wave, k_raw = blockIdx.x * 64 + lane;
  const bool active = j_raw < a.J && k_raw < a.K;
  const int j = min(j_raw, a.J - 1), k = min(k_raw, a.K - 1);  // idle threads shadow a voxel of the volume and add zeros
  const int i_begin = it * kBiasTileI, i_end = min(i_begin + kBiasTileI, a.I);
  const int nc = a.ci * a.cj * a.ck;
  const float* fg = a.coarse + static_cast<int64_t>(bc) * nc;
  double* ws = a.ws + static_cast<int64_t>(bc) * nc;

  // the block's box of coarse nodes (lerp_index is monotone in its voxel: the first and the last voxel of each axis bound it)
  const int j_first = blockIdx.y * kBiasRows, j_last = min(j_first + kBiasRows, a.J) - 1;
  const int k_first = blockIdx.x * 64, k_last = min(k_first + 64, a.K) - 1;
  const int bi0 = lerp_index(i_begin, a.ci, a.I, a.scale_i).i0, bni = lerp_index(i_end - 1, a.ci, a.I, a.scale_i).i1 - bi0 + 1;
  const int bj0 = lerp_index(j_first, a.cj, a.J, a.scale_j).i0, bnj = lerp_index(j_last, a.cj, a.J, a.scale_j).i1 - bj0 + 1;
  const int bk0 = lerp_index(k_first, a.ck, a.K, a.scale_k).i0, bnk = lerp_index(k_last, a.ck, a.K, a.scale_k).i1 - bk0 + 1;
  const bool box = bnk <= kMaxWaveNodes && static_cast<int64_t>(bni) * bnj * bnk <= kBoxDoubles;
  if (box) {
    for (int t = threadIdx.x; t < bni * bnj * bnk; t += blockDim.x) s_box[t] = 0.0;
  }
  __syncthreads();

  const Lerp1D lj = lerp_index(j, a.cj, a.J, a.scale_j);
  const Lerp1D lk = lerp_index(k, a.ck, a.K, a.scale_k);
  const int s_i = a.cj * a.ck, s_j = a.ck;
  const int64_t n = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t row = static_cast<int64_t>(bc) * n + static_cast<int64_t>(j) * a.K + k;
  const int64_t slab = static_cast<int64_t>(a.J) * a.K;
  auto coarse_plane = [&](int ii) -> float {  // bias_kernel's: the K-lerp, then the J-lerp
    const int o0 = ii * s_i + lj.i0 * s_j, o1 = ii * s_i + lj.i1 * s_j;
    return lerp2(lerp2(fg[o0 + lk.i0], lk.l0, fg[o0 + lk.i1], lk.l1), lj.l0, lerp2(fg[o1 + lk.i0], lk.l0, fg[o1 + lk.i1], lk.l1), lj.l1);
  };
  for (int i = i_begin; i < i_end; i++) {
    const Lerp1D li = lerp_index(i, a.ci, a.I, a.scale_i);
    const float field = expf(lerp2(coarse_plane(li.i0), li.l0, coarse_plane(li.i1), li.l1));
    const int64_t idx = row + i * slab;
    const float v = Elem<DT>::load(a.x, idx);
    const float y = a.divide ? __fdiv_rn(v, field) : __fmul_rn(v, field);
    float term = active ? __fmul_rn(a.gy[idx], y) : 0.0f;
    if (a.divide) term = -term;
    if (box) {
      for (int kk = bk0; kk < bk0 + bnk; kk++) {
        const float wk = (lk.i0 == kk ? lk.l0 : 0.0f) + (lk.i1 == kk ? lk.l1 : 0.0f);
        const double along_k = wave_sum_f64(static_cast<double>(__fmul_rn(wk, term)));
        if (lane < 4 && along_k != 0.0) {
          const float wi = (lane & 1) ? li.l1 : li.l0, wj = (lane & 2) ? lj.l1 : lj.l0;
          const int ii = (lane & 1) ? li.i1 : li.i0, jj = (lane & 2) ? lj.i1 : lj.i0;
          const float wij = __fmul_rn(wi, wj);
          if (wij != 0.0f) atomicAdd(&s_box[((ii - bi0) * bnj + (jj - bj0)) * bnk + (kk - bk0)], along_k * static_cast<double>(wij));
        }
      }
    } else if (term != 0.0f) {
#pragma unroll
      for (int corner = 0; corner < 8; corner++) {
        const float wi = (corner & 1) ? li.l1 : li.l0, wj = (corner & 2) ? lj.l1 : lj.l0, wk = (corner & 4) ? lk.l1 : lk.l0;
        const int ii = (corner & 1) ? li.i1 : li.i0, jj = (corner & 2) ? lj.i1 : lj.i0, kk = (corner & 4) ? lk.i1 : lk.i0;
        const float wij = __fmul_rn(wi, wj);
        const float value = __fmul_rn(wk, term);
        if (wij != 0.0f && value != 0.0f)
          unsafeAtomicAdd(ws + (static_cast<int64_t>(ii) * a.cj + jj) * a.ck + kk, static_cast<double>(value) * static_cast<double>(wij));
      }
    }
  }
  if (box) {
    __syncthreads();
    for (int t = threadIdx.x; t < bni * bnj * bnk; t += blockDim.x) {
      const double value = s_box[t];
      if (value == 0.0) continue;
      const int kk = t % bnk, jj = (t / bnk) % bnj, ii = t / (bnk * bnj);
      unsafeAtomicAdd(ws + (static_cast<int64_t>(ii + bi0) * a.cj + (jj + bj0)) * a.ck + (kk + bk0), value);
    }
  }
}

// =============================================================================
// Gamma: d_gamma[b] = sum_{x != 0} gy * y * log|x|,  y = sign(x) |x|^gamma
// =============================================================================
template <int DT>
__global__ __launch_bounds__(kPgBlock) void gamma_grad_kernel(const void* __restrict__ x, const float* __restrict__ gy, int64_t n_per_element,
                                                              float gamma, const float* __restrict__ gamma_b, int params_batched,
                                                              double* __restrict__ ws) {
  const int b = blockIdx.y;
  const float gm = gamma_b != nullptr ? gamma_b[params_batched ? b : 0] : gamma;  // (a shared exponent may live on the device too)
  const int64_t base = static_cast<int64_t>(b) * n_per_element;
  double acc[1] = {0.0};
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_per_element; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float g = gy[base + i];
    if constexpr (DT == TIO_F64) {  // the forward's float64 expression
      const double v = static_cast<const double*>(x)[base + i];
      if (v != 0.0) {
        const double s = static_cast<double>((v > 0) - (v < 0));
        acc[0] += (static_cast<double>(g) * (s * pow(fabs(v), static_cast<double>(gm)))) * log(fabs(v));
      }
    } else {
      const float v = Elem<DT>::load(x, base + i);
      if (v != 0.0f) {  // ATen's rule for d pow / d exponent at base 0
        const float s = static_cast<float>((v > 0.0f) - (v < 0.0f));
        const float y = __fmul_rn(s, powf(fabsf(v), gm));
        acc[0] += static_cast<double>(__fmul_rn(__fmul_rn(g, y), logf(fabsf(v))));
      }
    }
  }
  block_sum_to_workspace(acc, 1, ws + (static_cast<int64_t>(params_batched ? b : 0) * kPgSpread + blockIdx.x % kPgSpread) * kSlotDoubles);
}

// =============================================================================
// Noise: thread = 4 consecutive elements (one Philox block), as noise_kernel
// =============================================================================
template <int DT>
__global__ __launch_bounds__(kPgBlock) void noise_grad_kernel(const void* __restrict__ x, const float* __restrict__ gy, int64_t n_per_element,
                                                              float mean, float std, const float* __restrict__ mean_b,
                                                              const float* __restrict__ std_b, int params_batched, int rician,
                                                              const float* __restrict__ base1, const float* __restrict__ base2, uint64_t seed,
                                                              const uint8_t* __restrict__ keep, double* __restrict__ ws) {
  const int b = blockIdx.y;
  if (keep != nullptr && keep[b] == 0) return;  // block-uniform: the forward copied this element
  const int64_t base = static_cast<int64_t>(b) * n_per_element;
  const float mu = mean_b != nullptr ? mean_b[params_batched ? b : 0] : mean;  // (shared values may live on the device too)
  const float sd = std_b != nullptr ? std_b[params_batched ? b : 0] : std;
  using R = typename std::conditional<DT == TIO_F64, double, float>::type;  // the type the forward computes y in
  double acc[2] = {0.0, 0.0};
  const int64_t quads = (n_per_element + 3) / 4;
  for (int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; q < quads; q += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t e0 = 4 * q;
    const int cnt = static_cast<int>(min(static_cast<int64_t>(4), n_per_element - e0));
    float z1[4] = {0.f, 0.f, 0.f, 0.f}, z2[4] = {0.f, 0.f, 0.f, 0.f};
    if (base1 != nullptr) {
      for (int t = 0; t < cnt; t++) {
        z1[t] = base1[base + e0 + t];
        if (rician) z2[t] = base2[base + e0 + t];
      }
    } else if (((base + e0) & 3) == 0) {  // Philox blocks are indexed by the GLOBAL element index, as in noise_kernel
      philox_normal4(seed, 0, static_cast<uint64_t>((base + e0) >> 2), z1);
      if (rician) philox_normal4(seed, 1, static_cast<uint64_t>((base + e0) >> 2), z2);
    } else {
      for (int t = 0; t < cnt; t++) {
        float z[4];
        const int64_t g = base + e0 + t;
        philox_normal4(seed, 0, static_cast<uint64_t>(g >> 2), z);
        z1[t] = z[g & 3];
        if (rician) {
          philox_normal4(seed, 1, static_cast<uint64_t>(g >> 2), z);
          z2[t] = z[g & 3];
        }
      }
    }
    for (int t = 0; t < cnt; t++) {
      const int64_t idx = base + e0 + t;
      const float g = gy[idx];
      if (!rician) {  // y = x + (mean + std z)
        acc[0] += static_cast<double>(g);
        acc[1] += static_cast<double>(__fmul_rn(g, z1[t]));
        continue;
      }
      // y = sqrt(a^2 + n2^2), a = x + n1: d y / d mean = (a + n2) / y, d y / d std = (a z1 + n2 z2) / y   (-ffp-contract=off: every
      // operation below rounds on its own, in R)
      const R n1 = static_cast<R>(__fadd_rn(mu, __fmul_rn(sd, z1[t]))), n2 = static_cast<R>(__fadd_rn(mu, __fmul_rn(sd, z2[t])));
      R v;
      if constexpr (DT == TIO_F64) v = static_cast<const double*>(x)[idx];
      else v = Elem<DT>::load(x, idx);
      const R s = v + n1;
      const R y = sqrt(s * s + n2 * n2);
      if (y != static_cast<R>(0)) {
        const R slope = static_cast<R>(g) / y;
        acc[0] += static_cast<double>(slope * (s + n2));
        acc[1] += static_cast<double>(slope * (s * static_cast<R>(z1[t]) + n2 * static_cast<R>(z2[t])));
      }
    }
  }
  block_sum_to_workspace(acc, 2, ws + (static_cast<int64_t>(params_batched ? b : 0) * kPgSpread + blockIdx.x % kPgSpread) * kSlotDoubles);
}

// =============================================================================
// Taps: the clamped tap correlation  d[t] = sum_v g[v] * a[clamp(v + (t - r) e_axis)],  t = 0 .. 2 r
// =============================================================================
constexpr int kTapsMaxRadius = 16;
constexpr int kTapSlotDoubles = 40;  // 2 * 16 + 1 = 33 used

struct TapCorrArgs {
  const float* g;   // (B, C, I, J, K) float32
  const void* a;    // the same shape, dtype DT
  const uint8_t* skip;
  double* ws;       // (groups, kPgSpread, kTapSlotDoubles)
  int64_t n_spatial, stride;
  int channels, extent, r, axis, taps_batched, J, K;
};

template <int DT, int RMAX>
__global__ __launch_bounds__(kPgBlock) void tap_correlation_kernel(const TapCorrArgs a) {
  const int bc = blockIdx.y;
  const int b = bc / a.channels;
  if (a.skip != nullptr && a.skip[b] != 0) return;  // block-uniform: the forward copied this element
  const int64_t base = static_cast<int64_t>(bc) * a.n_spatial;
  const int r = a.r, last = a.extent - 1;
  double acc[2 * RMAX + 1];
#pragma unroll
  for (int t = 0; t < 2 * RMAX + 1; t++) acc[t] = 0.0;
  for (int64_t v = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; v < a.n_spatial; v += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int m = a.axis == 2 ? static_cast<int>(v % a.K) : (a.axis == 1 ? static_cast<int>((v / a.K) % a.J) : static_cast<int>(v / (static_cast<int64_t>(a.K) * a.J)));
    const float g = a.g[base + v];
    const int64_t line = base + v - static_cast<int64_t>(m) * a.stride;  // the voxel of this line at coordinate 0
#pragma unroll
    for (int t = 0; t < 2 * RMAX + 1; t++) {
      if (t <= 2 * r) {  // (uniform)
        const int p = min(max(m + t - r, 0), last);
        acc[t] += static_cast<double>(__fmul_rn(g, Elem<DT>::load(a.a, line + static_cast<int64_t>(p) * a.stride)));
      }
    }
  }
  block_sum_to_workspace(acc, 2 * r + 1, a.ws + (static_cast<int64_t>(a.taps_batched ? b : 0) * kPgSpread + blockIdx.x % kPgSpread) * kTapSlotDoubles);
}

template <int DT>
__global__ __launch_bounds__(kPgBlock) void widen_kernel(const void* __restrict__ x, float* __restrict__ y, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    y[i] = Elem<DT>::load(x, i);
}

unsigned capped_blocks(int64_t items) {
  const int64_t want = (items + kPgBlock - 1) / kPgBlock;
  return static_cast<unsigned>(want < 1 ? 1 : (want < kPgMaxBlocks ? want : kPgMaxBlocks));
}

// null / size / alignment check of a workspace and its clearing; 0 = go on
int prepare_workspace(const char* what, void* workspace, int64_t workspace_bytes, int64_t needed, hipStream_t s) {
  if (workspace == nullptr || workspace_bytes < needed)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: the workspace holds %lld bytes, %lld are needed", what, static_cast<long long>(workspace_bytes),
                static_cast<long long>(needed));
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: the workspace must be 8-byte aligned", what);
  if (needed > 0 && hipMemsetAsync(workspace, 0, static_cast<size_t>(needed), s) != hipSuccess)
    return fail(TIO_ERR_LAUNCH, "%s: cannot clear the workspace", what);
  return TIO_OK;
}

int zero_output(const char* what, float* out, int64_t n, hipStream_t s) {
  if (out != nullptr && n > 0 && hipMemsetAsync(out, 0, static_cast<size_t>(n) * sizeof(float), s) != hipSuccess)
    return fail(TIO_ERR_LAUNCH, "%s: cannot clear an output", what);
  return TIO_OK;
}

int64_t scalar_groups(int32_t batch, int32_t params_batched) { return params_batched ? (batch > 0 ? batch : 0) : 1; }

}  // namespace
}  // namespace tio

using namespace tio;

// -----------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t tio_bias_field_grad_workspace_bytes(int32_t batch, int32_t channels, const int32_t coarse_shape[3]) {
  if (coarse_shape == nullptr || batch < 0 || channels < 1 || coarse_shape[0] < 1 || coarse_shape[1] < 1 || coarse_shape[2] < 1) {
    fail(TIO_ERR_INVALID_ARGUMENT, "tio_bias_field_grad_workspace_bytes: bad argument");
    return 0;
  }
  return static_cast<int64_t>(batch) * channels * coarse_shape[0] * coarse_shape[1] * coarse_shape[2] * static_cast<int64_t>(sizeof(double));
}

extern "C" int tio_bias_field_grad(const void* x, const float* gy, int32_t dtype, int32_t batch, int32_t channels, const int32_t shape[3],
                                   const float* coarse_dev, const int32_t coarse_shape[3], int32_t divide, const uint8_t* skip_dev,
                                   float* d_coarse, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* what = "tio_bias_field_grad";
  if (batch == 0) return TIO_OK;  // (no output values either)
  if (x == nullptr || gy == nullptr || shape == nullptr || coarse_dev == nullptr || coarse_shape == nullptr || d_coarse == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null argument", what);
  if (!is_float_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", what, dtype);
  for (int d = 0; d < 3; d++)
    if (shape[d] < 1 || coarse_shape[d] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: bad shape", what);
  if (batch < 0 || channels < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: bad batch/channels", what);
  const int64_t nc = static_cast<int64_t>(coarse_shape[0]) * coarse_shape[1] * coarse_shape[2];
  if (nc > 0x7FFFFFFF) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: coarse grid too large", what);
  const int tiles_i = (shape[0] + kBiasTileI - 1) / kBiasTileI;
  const dim3 grid(static_cast<unsigned>((shape[2] + 63) / 64), static_cast<unsigned>((shape[1] + kBiasRows - 1) / kBiasRows),
                  static_cast<unsigned>(tiles_i) * batch * channels);
  if (grid.z > 65535u || grid.y > 65535u) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: volume too large for one launch", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t values = static_cast<int64_t>(batch) * channels * nc;
  if (const int st = prepare_workspace(what, workspace, workspace_bytes, values * static_cast<int64_t>(sizeof(double)), s)) return st;
  BiasGradArgs a{};
  a.x = x; a.gy = gy; a.coarse = coarse_dev; a.ws = static_cast<double*>(workspace); a.skip = skip_dev;
  a.channels = channels; a.I = shape[0]; a.J = shape[1]; a.K = shape[2];
  a.ci = coarse_shape[0]; a.cj = coarse_shape[1]; a.ck = coarse_shape[2]; a.divide = divide != 0; a.tiles_i = tiles_i;
  a.scale_i = lerp_scale(a.ci, a.I); a.scale_j = lerp_scale(a.cj, a.J); a.scale_k = lerp_scale(a.ck, a.K);
  const bool known = dispatch_float_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL(bias_grad_kernel<decltype(dt)::value>, grid, dim3(kPgBlock), 0, s, a); });
  if (!known) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", what, dtype);
  launch_param_grad_finish(a.ws, d_coarse, 1, values, 1, values, values, s);
  return check_launch(what);
}

// -----------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t tio_gamma_grad_workspace_bytes(int32_t batch, int32_t params_batched) {
  return scalar_groups(batch, params_batched) * kPgSpread * kSlotDoubles * static_cast<int64_t>(sizeof(double));
}

extern "C" int tio_gamma_grad(const void* x, const float* gy, int32_t dtype, int32_t batch, int64_t n_per_element, float gamma,
                              const float* gamma_dev, int32_t params_batched, float* d_gamma, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  const char* what = "tio_gamma_grad";
  if (d_gamma == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null d_gamma", what);
  if (batch < 0 || n_per_element < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", what);
  if (!is_float_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", what, dtype);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t groups = scalar_groups(batch, params_batched);
  if (batch == 0 || n_per_element == 0) return zero_output(what, d_gamma, groups, s);
  if (x == nullptr || gy == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null argument", what);
  if (params_batched && gamma_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null gamma_dev", what);
  if (batch > 65535) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: batch too large for one launch", what);
  if (const int st = prepare_workspace(what, workspace, workspace_bytes, tio_gamma_grad_workspace_bytes(batch, params_batched), s)) return st;
  double* ws = static_cast<double*>(workspace);
  const dim3 grid(capped_blocks(n_per_element), static_cast<unsigned>(batch));
  const bool known = dispatch_float_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(gamma_grad_kernel<decltype(dt)::value>, grid, dim3(kPgBlock), 0, s, x, gy, n_per_element, gamma, gamma_dev, params_batched, ws);
  });
  if (!known) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", what, dtype);
  launch_param_grad_finish(ws, d_gamma, groups, 1, kPgSpread, kSlotDoubles, 1, s);
  return check_launch(what);
}

// -----------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t tio_noise_grad_workspace_bytes(int32_t batch, int32_t params_batched) {
  return scalar_groups(batch, params_batched) * kPgSpread * kSlotDoubles * static_cast<int64_t>(sizeof(double));
}

extern "C" int tio_noise_grad(const void* x, const float* gy, int32_t dtype, int32_t batch, int64_t n_per_element, float mean, float std,
                              const float* mean_dev, const float* std_dev, int32_t params_batched, int32_t rician, const float* base1_dev,
                              const float* base2_dev, uint64_t philox_seed, const uint8_t* keep_dev, float* d_mean, float* d_std,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  const char* what = "tio_noise_grad";
  if (d_mean == nullptr && d_std == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: neither d_mean nor d_std is wanted", what);
  if (batch < 0 || n_per_element < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", what);
  if (!is_float_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", what, dtype);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t groups = scalar_groups(batch, params_batched);
  if (batch == 0 || n_per_element == 0) {
    if (const int st = zero_output(what, d_mean, groups, s)) return st;
    return zero_output(what, d_std, groups, s);
  }
  if (gy == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null gy", what);
  if (rician && x == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: rician needs x", what);
  if (params_batched && (mean_dev == nullptr || std_dev == nullptr))
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: params_batched needs mean_dev and std_dev", what);
  if (base1_dev != nullptr && rician && base2_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: rician with base1_dev needs base2_dev", what);
  if (batch > 65535) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: batch too large for one launch", what);
  if (const int st = prepare_workspace(what, workspace, workspace_bytes, tio_noise_grad_workspace_bytes(batch, params_batched), s)) return st;
  double* ws = static_cast<double*>(workspace);
  const dim3 grid(capped_blocks((n_per_element + 3) / 4), static_cast<unsigned>(batch));
  const bool known = dispatch_float_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(noise_grad_kernel<decltype(dt)::value>, grid, dim3(kPgBlock), 0, s, x, gy, n_per_element, mean, std, mean_dev, std_dev,
                       params_batched, rician, base1_dev, base2_dev, philox_seed, keep_dev, ws);
  });
  if (!known) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", what, dtype);
  if (d_mean != nullptr) launch_param_grad_finish(ws, d_mean, groups, 1, kPgSpread, kSlotDoubles, 1, s);
  if (d_std != nullptr) launch_param_grad_finish(ws + 1, d_std, groups, 1, kPgSpread, kSlotDoubles, 1, s);
  return check_launch(what);
}

// -----------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t tio_separable_conv3d_taps_grad_workspace_bytes(int32_t batch, int32_t taps_batched) {
  return 3 * scalar_groups(batch, taps_batched) * kPgSpread * kTapSlotDoubles * static_cast<int64_t>(sizeof(double));
}

extern "C" int tio_separable_conv3d_taps_grad(const void* x, int32_t dtype, const float* gy, float* scratch, int32_t batch, int32_t channels,
                                              const int32_t shape[3], const float* taps_dev, int32_t taps_batched, int32_t tap_stride,
                                              const int32_t radius[3], const uint8_t* skip_dev, float* d_taps, void* workspace,
                                              int64_t workspace_bytes, void* stream) {
  const char* what = "tio_separable_conv3d_taps_grad";
  if (shape == nullptr || radius == nullptr || d_taps == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null argument", what);
  if (!is_float_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", what, dtype);
  if (batch < 0 || channels < 1 || shape[0] < 1 || shape[1] < 1 || shape[2] < 1 || tap_stride < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: bad shape", what);
  int n_active = 0;
  for (int a = 0; a < 3; a++) {
    if (radius[a] < 0 || 2 * radius[a] + 1 > tap_stride)
      return fail(TIO_ERR_INVALID_ARGUMENT, "%s: radius[%d]=%d does not fit tap_stride=%d", what, a, radius[a], tap_stride);
    if (radius[a] > kTapsMaxRadius) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: radius[%d]=%d exceeds %d", what, a, radius[a], kTapsMaxRadius);
    if (radius[a] > 0) n_active++;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t groups = scalar_groups(batch, taps_batched);
  if (batch == 0 || n_active == 0) return zero_output(what, d_taps, groups * 3 * tap_stride, s);
  if (x == nullptr || gy == nullptr || taps_dev == nullptr || scratch == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null argument", what);
  const int64_t n = static_cast<int64_t>(shape[0]) * shape[1] * shape[2];
  const int64_t bcs = static_cast<int64_t>(batch) * channels, total = bcs * n;
  if (bcs > 65535) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: batch x channels too large for one launch", what);
  if (const int st = prepare_workspace(what, workspace, workspace_bytes, tio_separable_conv3d_taps_grad_workspace_bytes(batch, taps_batched), s)) return st;
  if (const int st = zero_output(what, d_taps, groups * 3 * tap_stride, s)) return st;
  double* ws = static_cast<double*>(workspace);
  float* s0 = scratch;
  float* s1 = scratch + total;

  // one single-axis pass of the forward / of its transpose through the existing launchers (the other radii zeroed)
  auto forward_axis = [&](const float* src, float* dst, int axis) {
    int32_t one[3] = {0, 0, 0};
    one[axis] = radius[axis];
    return tio_separable_conv3d(src, dst, nullptr, TIO_F32, batch, channels, shape, taps_dev, taps_batched, tap_stride, one, skip_dev, stream);
  };
  auto adjoint_axis = [&](const float* src, float* dst, int axis) {
    int32_t one[3] = {0, 0, 0};
    one[axis] = radius[axis];
    return tio_separable_conv3d_adjoint(src, dst, nullptr, batch, channels, shape, taps_dev, taps_batched, tap_stride, one, skip_dev, stream);
  };
  auto widen = [&](float* dst) -> const float* {  // x as float32 (exact): the stencil's intermediates are float32
    if (dtype == TIO_F32) return static_cast<const float*>(x);
    (void)dispatch_float_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL(widen_kernel<decltype(dt)::value>, dim3(capped_blocks(total)), dim3(kPgBlock), 0, s, x, dst, total); });
    return dst;
  };
  auto correlate = [&](const float* g, const void* a, int a_dtype, int axis) {
    TapCorrArgs t{};
    t.g = g; t.a = a; t.skip = skip_dev; t.ws = ws + static_cast<int64_t>(axis) * groups * kPgSpread * kTapSlotDoubles;
    t.n_spatial = n; t.stride = axis == 0 ? static_cast<int64_t>(shape[1]) * shape[2] : (axis == 1 ? shape[2] : 1);
    t.channels = channels; t.extent = shape[axis]; t.r = radius[axis]; t.axis = axis; t.taps_batched = taps_batched != 0; t.J = shape[1]; t.K = shape[2];
    const dim3 grid(capped_blocks(n), static_cast<unsigned>(bcs));
    (void)dispatch_float_dtype(a_dtype, [&](auto dt) {
      if (t.r <= 4) hipLaunchKernelGGL((tap_correlation_kernel<decltype(dt)::value, 4>), grid, dim3(kPgBlock), 0, s, t);
      else hipLaunchKernelGGL((tap_correlation_kernel<decltype(dt)::value, kTapsMaxRadius>), grid, dim3(kPgBlock), 0, s, t);
    });
    // d_taps[(group * 3 + axis) * tap_stride + t]
    launch_param_grad_finish(t.ws, d_taps + static_cast<int64_t>(axis) * tap_stride, groups, 2 * t.r + 1, kPgSpread, kTapSlotDoubles,
                             3 * static_cast<int64_t>(tap_stride), s);
  };

  // y = A_K A_J A_I x.  P1 = A_I x, P2 = A_J P1, Q1 = A_K^T gy, Q2 = A_J^T Q1; an inactive axis is the identity.
  const void* p1 = x;
  int p1_dtype = dtype;
  if (radius[0] > 0) {
    if (const int st = forward_axis(widen(s1), s0, 0)) return st;
    p1 = s0; p1_dtype = TIO_F32;
  }
  const void* p2 = p1;
  int p2_dtype = p1_dtype;
  if (radius[1] > 0 && radius[2] > 0) {  // (P2 is read by the K correlation only)
    const float* src = p1_dtype == TIO_F32 ? static_cast<const float*>(p1) : widen(s0);  // (radius[0] == 0: s0 is free)
    if (const int st = forward_axis(src, s1, 1)) return st;
    p2 = s1; p2_dtype = TIO_F32;
  }
  if (radius[2] > 0) correlate(gy, p2, p2_dtype, 2);  // dW_K[t] = sum gy * (A_J A_I x)[clamp]
  const float* q1 = gy;
  if (radius[2] > 0 && (radius[1] > 0 || radius[0] > 0)) {
    if (const int st = adjoint_axis(gy, s1, 2)) return st;
    q1 = s1;
  }
  if (radius[1] > 0) correlate(q1, p1, p1_dtype, 1);  // dW_J[t] = sum (A_K^T gy) * (A_I x)[clamp]
  const float* q2 = q1;
  if (radius[1] > 0 && radius[0] > 0) {
    if (const int st = adjoint_axis(q1, s0, 1)) return st;  // (P1 in s0 has been read)
    q2 = s0;
  }
  if (radius[0] > 0) correlate(q2, x, dtype, 0);  // dW_I[t] = sum (A_J^T A_K^T gy) * x[clamp]
  return check_launch(what);
}
