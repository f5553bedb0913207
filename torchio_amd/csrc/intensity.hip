// intensity.hip — the pointwise intensity kernels for gfx950 (the separable stencil: stencil.hip):
//   tio_bias_field_apply  (BiasField;                 bias_field.py:201-341)
//   tio_add_noise         (Noise;                     noise.py:98-178)
//   tio_philox_normal     (the fast-mode normal stream of tio_add_noise)
//   tio_gamma_pow         (Gamma;                     gamma.py:80-142)
//   tio_channel_min       (default_pad_value="minimum"; spatial.py:2054-2095)
// All are HBM-bound elementwise passes: one read + one write of the volume per op
// (tio_channel_min: one read).  No MFMA.
#include <mutex>
#include <vector>

#include "common.hpp"
#include "philox_normal.hpp"

namespace tio {

constexpr int kBlock = 256;

// =============================================================================
// BiasField
// =============================================================================
constexpr int kMaxCoarseLds = 8192;  // floats (32 KiB)

// grid: x = K tiles (64 lanes), y = J tiles (4 rows, one per wave), z = I tiles * (B*C);
// each thread walks kBiasTileI slabs so the j/k lerp terms are computed once.
constexpr int kBiasTileI = 8;

template <int DT>
__global__ __launch_bounds__(kBlock) void bias_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                      int channels, int I, int J, int K,
                                                      const float* __restrict__ coarse, int ci, int cj, int ck,
                                                      float scale_i, float scale_j, float scale_k, int divide,
                                                      const uint8_t* __restrict__ skip, int tiles_i) {
  extern __shared__ __attribute__((aligned(16))) float s_coarse[];
  const int it = blockIdx.z % tiles_i;
  const int bc = blockIdx.z / tiles_i;
  const int b = bc / channels;
  const int64_t n = static_cast<int64_t>(I) * J * K;
  const int64_t base = static_cast<int64_t>(bc) * n;
  const bool skipped = skip != nullptr && skip[b] != 0;
  const int nc = ci * cj * ck;
  const float* fg = coarse + static_cast<int64_t>(bc) * nc;
  const bool in_lds = !skipped && nc <= kMaxCoarseLds;
  if (in_lds) {
    for (int t = threadIdx.x; t < nc; t += blockDim.x) s_coarse[t] = fg[t];
    __syncthreads();
  }
  const int k = blockIdx.x * 64 + (threadIdx.x & 63);
  const int j = blockIdx.y * (kBlock / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= K || j >= J) return;
  const int i_begin = it * kBiasTileI, i_end = min(i_begin + kBiasTileI, I);
  using T = typename Elem<DT>::type;
  const int64_t row = base + static_cast<int64_t>(j) * K + k;
  const int64_t slab = static_cast<int64_t>(J) * K;
  if (skipped) {  // std == 0 rows restored bit-exactly (bias_field.py:247-253)
    for (int i = i_begin; i < i_end; i++) static_cast<T*>(y)[row + i * slab] = static_cast<const T*>(x)[row + i * slab];
    return;
  }
  const Lerp1D lj = lerp_index(j, cj, J, scale_j);
  const Lerp1D lk = lerp_index(k, ck, K, scale_k);
  const int s_i = cj * ck, s_j = ck;
  // all loads of the i-tile are issued before the first use: 8 independent HBM requests in flight per lane
  float v[kBiasTileI];
  double vd[DT == TIO_F64 ? kBiasTileI : 1];
#pragma unroll
  for (int u = 0; u < kBiasTileI; u++) {
    const int i = i_begin + u;
    if (i < i_end) {
      if constexpr (DT == TIO_F64) vd[u] = static_cast<const double*>(x)[row + i * slab];
      else v[u] = Elem<DT>::load(x, row + i * slab);
    }
  }
  // The K- and J-lerps of a coarse plane are invariants of this thread's (j, k) column
  // (ATen nests K innermost, then J, then I), so they are redone only when the walk
  // along I enters a new coarse cell — a block-uniform event.
  auto coarse_plane = [&](int ii) -> float {
    const int o0 = ii * s_i + lj.i0 * s_j, o1 = ii * s_i + lj.i1 * s_j;
    float c00, c01, c10, c11;
    if (in_lds) {
      c00 = s_coarse[o0 + lk.i0]; c01 = s_coarse[o0 + lk.i1]; c10 = s_coarse[o1 + lk.i0]; c11 = s_coarse[o1 + lk.i1];
    } else {
      c00 = fg[o0 + lk.i0]; c01 = fg[o0 + lk.i1]; c10 = fg[o1 + lk.i0]; c11 = fg[o1 + lk.i1];
    }
    return lerp2(lerp2(c00, lk.l0, c01, lk.l1), lj.l0, lerp2(c10, lk.l0, c11, lk.l1), lj.l1);
  };
  int cur0 = -1, cur1 = -1;
  float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
  for (int u = 0; u < kBiasTileI; u++) {
    const int i = i_begin + u;
    if (i >= i_end) break;
    const Lerp1D li = lerp_index(i, ci, I, scale_i);
    if (li.i0 != cur0) {
      p0 = (li.i0 == cur1) ? p1 : coarse_plane(li.i0);
      cur0 = li.i0;
    }
    if (li.i1 != cur1) {
      p1 = (li.i1 == cur0) ? p0 : coarse_plane(li.i1);
      cur1 = li.i1;
    }
    const float field = expf(lerp2(p0, li.l0, p1, li.l1));  // bias_field.py:341
    const int64_t idx = row + i * slab;
    if constexpr (DT == TIO_F64) {  // f64 data (x) f32 field promotes to f64
      static_cast<double*>(y)[idx] = divide ? vd[u] / static_cast<double>(field) : vd[u] * static_cast<double>(field);
    } else {
      Elem<DT>::store(y, idx, divide ? __fdiv_rn(v[u], field) : __fmul_rn(v[u], field));
    }
  }
}

__global__ __launch_bounds__(kBlock) void philox_normal_kernel(float* __restrict__ out, int64_t n, uint64_t seed,
                                                               int stream_id) {
  const int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (4 * q >= n) return;
  float z[4];
  philox_normal4(seed, stream_id, static_cast<uint64_t>(q), z);
  // (one 16-byte store where `out` allows it: a caller's dense view may start anywhere on an element boundary)
  if (4 * q + 3 < n && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
    *reinterpret_cast<float4*>(out + 4 * q) = make_float4(z[0], z[1], z[2], z[3]);
  } else {
    for (int t = 0; t < 4; t++)
      if (4 * q + t < n) out[4 * q + t] = z[t];
  }
}

// =============================================================================
// Noise: thread = 4 consecutive elements (one Philox block / one 16-B access)
// =============================================================================
template <int DT>
__global__ __launch_bounds__(kBlock) void noise_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                       int64_t n_per_element, float mean, float std,
                                                       const float* __restrict__ mean_b,
                                                       const float* __restrict__ std_b, int params_batched,
                                                       int rician, const float* __restrict__ base1,
                                                       const float* __restrict__ base2, uint64_t seed,
                                                       const uint8_t* __restrict__ keep) {
  const int b = blockIdx.y;
  const int64_t q = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t e0 = 4 * q;
  if (e0 >= n_per_element) return;
  const int64_t base = static_cast<int64_t>(b) * n_per_element;
  const float mu = params_batched ? mean_b[b] : mean;
  const float sd = params_batched ? std_b[b] : std;
  const bool kept = keep == nullptr || keep[b] != 0;
  using T = typename Elem<DT>::type;
  const int cnt = static_cast<int>(min(static_cast<int64_t>(4), n_per_element - e0));
  if (!kept) {  // gated-out rows restored bit-exactly (noise.py:126-146)
    for (int t = 0; t < cnt; t++) static_cast<T*>(y)[base + e0 + t] = static_cast<const T*>(x)[base + e0 + t];
    return;
  }
  float z1[4], z2[4] = {0.f, 0.f, 0.f, 0.f};
  if (base1 != nullptr) {
    for (int t = 0; t < cnt; t++) {
      z1[t] = base1[base + e0 + t];
      if (rician) z2[t] = base2[base + e0 + t];
    }
  } else {
    // Philox blocks are indexed by the GLOBAL element index (base + e0) >> 2 so
    // that the stream equals tio_philox_normal over the whole tensor; rows are
    // 4-aligned whenever n_per_element % 4 == 0, otherwise take the slow path.
    if (((base + e0) & 3) == 0) {
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
  }
  if constexpr (DT == TIO_F32) {
    // whole, 16-byte aligned quad: one vector load and one vector store per thread
    if (cnt == 4 && (((base + e0) & 3) == 0) && !rician &&
        (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0)) {
      const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + base + e0);
      float4 o;
      o.x = __fadd_rn(v.x, __fadd_rn(mu, __fmul_rn(sd, z1[0])));  // noise.py:178, :119
      o.y = __fadd_rn(v.y, __fadd_rn(mu, __fmul_rn(sd, z1[1])));
      o.z = __fadd_rn(v.z, __fadd_rn(mu, __fmul_rn(sd, z1[2])));
      o.w = __fadd_rn(v.w, __fadd_rn(mu, __fmul_rn(sd, z1[3])));
      *reinterpret_cast<float4*>(static_cast<float*>(y) + base + e0) = o;
      return;
    }
  }
  for (int t = 0; t < cnt; t++) {
    const int64_t idx = base + e0 + t;
    const float n1 = __fadd_rn(mu, __fmul_rn(sd, z1[t]));  // noise.py:178
    if constexpr (DT == TIO_F64) {
      const double v = static_cast<const double*>(x)[idx];
      if (rician) {
        const double n2 = static_cast<double>(__fadd_rn(mu, __fmul_rn(sd, z2[t])));
        const double s = v + static_cast<double>(n1);
        static_cast<double*>(y)[idx] = sqrt(s * s + n2 * n2);
      } else {
        static_cast<double*>(y)[idx] = v + static_cast<double>(n1);
      }
    } else {
      const float v = Elem<DT>::load(x, idx);
      float r;
      if (rician) {  // noise.py:117
        const float n2 = __fadd_rn(mu, __fmul_rn(sd, z2[t]));
        const float s = __fadd_rn(v, n1);
        r = sqrtf(__fadd_rn(__fmul_rn(s, s), __fmul_rn(n2, n2)));
      } else {
        r = __fadd_rn(v, n1);  // noise.py:119
      }
      Elem<DT>::store(y, idx, r);
    }
  }
}

// =============================================================================
// Gamma
// =============================================================================
template <int DT>
__global__ __launch_bounds__(kBlock) void gamma_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                       int64_t n_per_element, float gamma,
                                                       const float* __restrict__ gamma_b, int params_batched) {
  const int b = blockIdx.y;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n_per_element) return;
  const int64_t idx = static_cast<int64_t>(b) * n_per_element + i;
  const float gm = params_batched ? gamma_b[b] : gamma;
  if constexpr (DT == TIO_F64) {
    const double v = static_cast<const double*>(x)[idx];
    const double s = static_cast<double>((v > 0) - (v < 0));
    static_cast<double*>(y)[idx] = s * pow(fabs(v), static_cast<double>(gm));
  } else {
    const float v = Elem<DT>::load(x, idx);
    const float s = static_cast<float>((v > 0.0f) - (v < 0.0f));
    Elem<DT>::store(y, idx, __fmul_rn(s, powf(fabsf(v), gm)));  // gamma.py:90
  }
}

// =============================================================================
// Per-channel minimum of the first batch element (device-resident result)
// =============================================================================
// (float_to_key / key_to_float: common.hpp)

// keys (all ones) + tickets (zero) of tio_channel_min, one pair of arrays per (device, stream): set up once, every
// launch restores them.  Calls on one stream are ordered; different streams get different arrays.
uint32_t* min_workspace(hipStream_t s, int entries, int* cap_out, int kind) {
  struct Slot { int device; hipStream_t stream; int kind; uint32_t* ptr; int cap; };
  static std::mutex mu;
  static std::vector<Slot> slots;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  Slot* found = nullptr;
  for (Slot& sl : slots)
    if (sl.device == device && sl.stream == s && sl.kind == kind) found = &sl;
  if (found != nullptr && found->cap >= entries) {
    *cap_out = found->cap;
    return found->ptr;
  }
  const int cap = entries < 1024 ? 1024 : entries;
  uint32_t* ptr = nullptr;
  if (hipMalloc(&ptr, sizeof(uint32_t) * 2 * cap) != hipSuccess) return nullptr;
  if (hipMemset(ptr, 0xFF, sizeof(uint32_t) * cap) != hipSuccess || hipMemset(ptr + cap, 0, sizeof(uint32_t) * cap) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {  // (the memsets run on the null stream: finished before any launch on `s` reads them)
    (void)hipFree(ptr);
    return nullptr;
  }
  if (found != nullptr) {
    // the predecessor is NOT freed: a concurrent caller on this stream may hold it and launch with it after we return
    found->ptr = ptr; found->cap = cap;
  } else {
    slots.push_back(Slot{device, s, kind, ptr, cap});
  }
  *cap_out = cap;
  return ptr;
}

// One launch: every block folds its minimum into keys[c] (ordered-integer image of the float), takes a ticket, and the
// block that draws the last ticket of its channel decodes the result into out[c] and leaves keys[c] / tickets[c] as it
// found them (all ones / zero) for the next call on this stream — no init launch before, no decode launch after.
template <int DT>
__global__ __launch_bounds__(kBlock) void min_reduce_kernel(const void* __restrict__ x, int64_t n_spatial,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ tickets,
                                                            float* __restrict__ out) {
  const int c = blockIdx.y;
  const int64_t base = static_cast<int64_t>(c) * n_spatial;
  uint32_t best = 0xFFFFFFFFu;
  bool vectorised = false;
  if constexpr (DT == TIO_F32) {
    // 16-byte loads, four independent ones in flight per lane (a 64 MiB channel in ~15 us)
    const float* p = static_cast<const float*>(x) + base;
    if ((n_spatial & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      vectorised = true;
      const int64_t n4 = n_spatial >> 2, step = static_cast<int64_t>(gridDim.x) * blockDim.x;
      const float4* p4 = reinterpret_cast<const float4*>(p);
      int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
      for (; i + 7 * step < n4; i += 8 * step) {  // (eight loads in flight per lane: what a 512^3 volume needs to keep HBM busy from 2 - 4 blocks per CU)
        const float4 a0 = p4[i], a1 = p4[i + step], a2 = p4[i + 2 * step], a3 = p4[i + 3 * step];
        const float4 a4 = p4[i + 4 * step], a5 = p4[i + 5 * step], a6 = p4[i + 6 * step], a7 = p4[i + 7 * step];
        best = min(best, min(min(float_to_key(a0.x), float_to_key(a0.y)), min(float_to_key(a0.z), float_to_key(a0.w))));
        best = min(best, min(min(float_to_key(a1.x), float_to_key(a1.y)), min(float_to_key(a1.z), float_to_key(a1.w))));
        best = min(best, min(min(float_to_key(a2.x), float_to_key(a2.y)), min(float_to_key(a2.z), float_to_key(a2.w))));
        best = min(best, min(min(float_to_key(a3.x), float_to_key(a3.y)), min(float_to_key(a3.z), float_to_key(a3.w))));
        best = min(best, min(min(float_to_key(a4.x), float_to_key(a4.y)), min(float_to_key(a4.z), float_to_key(a4.w))));
        best = min(best, min(min(float_to_key(a5.x), float_to_key(a5.y)), min(float_to_key(a5.z), float_to_key(a5.w))));
        best = min(best, min(min(float_to_key(a6.x), float_to_key(a6.y)), min(float_to_key(a6.z), float_to_key(a6.w))));
        best = min(best, min(min(float_to_key(a7.x), float_to_key(a7.y)), min(float_to_key(a7.z), float_to_key(a7.w))));
      }
      for (; i + 3 * step < n4; i += 4 * step) {
        const float4 a0 = p4[i], a1 = p4[i + step], a2 = p4[i + 2 * step], a3 = p4[i + 3 * step];
        best = min(best, min(min(float_to_key(a0.x), float_to_key(a0.y)), min(float_to_key(a0.z), float_to_key(a0.w))));
        best = min(best, min(min(float_to_key(a1.x), float_to_key(a1.y)), min(float_to_key(a1.z), float_to_key(a1.w))));
        best = min(best, min(min(float_to_key(a2.x), float_to_key(a2.y)), min(float_to_key(a2.z), float_to_key(a2.w))));
        best = min(best, min(min(float_to_key(a3.x), float_to_key(a3.y)), min(float_to_key(a3.z), float_to_key(a3.w))));
      }
      for (; i < n4; i += step) {
        const float4 a0 = p4[i];
        best = min(best, min(min(float_to_key(a0.x), float_to_key(a0.y)), min(float_to_key(a0.z), float_to_key(a0.w))));
      }
    }
  }
  if (!vectorised) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n_spatial;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
      best = min(best, float_to_key(Elem<DT>::load(x, base + i)));
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) best = min(best, static_cast<uint32_t>(__shfl_xor(static_cast<int>(best), s)));
  __shared__ uint32_t s_best[kBlock / 64];
  if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t m = s_best[0];
    for (int w = 1; w < kBlock / 64; w++) m = min(m, s_best[w]);
    // (no fence: the ticket is drawn after the minimum's atomic has returned, both at agent scope — a `__threadfence()`
    // per block is an L2 write-back each and made this kernel 50 % slower)
    const uint32_t seen = __hip_atomic_fetch_min(&keys[c], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("" ::"v"(seen) : "memory");
    if (__hip_atomic_fetch_add(&tickets[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {  // all the others have published
      out[c] = key_to_float(__hip_atomic_exchange(&keys[c], 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      __hip_atomic_exchange(&tickets[c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace tio

using namespace tio;

extern "C" int tio_bias_field_apply(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels,
                                    const int32_t shape[3], const float* coarse_dev,
                                    const int32_t coarse_shape[3], int32_t divide, const uint8_t* skip_dev,
                                    void* stream) {
  if (batch == 0) return TIO_OK;
  if (x == nullptr || y == nullptr || shape == nullptr || coarse_dev == nullptr || coarse_shape == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_bias_field_apply: null argument");
  if (!is_float_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_bias_field_apply: dtype %d", dtype);
  for (int d = 0; d < 3; d++)
    if (shape[d] < 1 || coarse_shape[d] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_bias_field_apply: bad shape");
  if (batch < 0 || channels < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_bias_field_apply: bad batch/channels");
  if (batch == 0) return TIO_OK;
  const int nc = coarse_shape[0] * coarse_shape[1] * coarse_shape[2];
  const size_t lds = nc <= kMaxCoarseLds ? static_cast<size_t>(nc) * sizeof(float) : 0;
  const int tiles_i = (shape[0] + kBiasTileI - 1) / kBiasTileI;
  const dim3 grid(static_cast<unsigned>((shape[2] + 63) / 64), static_cast<unsigned>((shape[1] + 3) / 4),
                  static_cast<unsigned>(tiles_i) * batch * channels);
  if (grid.z > 65535u || grid.y > 65535u) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_bias_field_apply: volume too large for one launch");
  const bool known = dispatch_float_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(bias_kernel<decltype(dt)::value>, grid, dim3(kBlock), lds, static_cast<hipStream_t>(stream), x, y, channels,
                       shape[0], shape[1], shape[2], coarse_dev, coarse_shape[0], coarse_shape[1], coarse_shape[2],
                       lerp_scale(coarse_shape[0], shape[0]), lerp_scale(coarse_shape[1], shape[1]),
                       lerp_scale(coarse_shape[2], shape[2]), divide, skip_dev, tiles_i);
  });
  return known ? check_launch("tio_bias_field_apply") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_bias_field_apply: dtype %d", dtype);
}

extern "C" int tio_add_noise(const void* x, void* y, int32_t dtype, int32_t batch, int64_t n_per_element,
                             float mean, float std, const float* mean_dev, const float* std_dev,
                             int32_t params_batched, int32_t rician, const float* base1_dev,
                             const float* base2_dev, uint64_t philox_seed, const uint8_t* keep_dev, void* stream) {
  if (batch == 0 || n_per_element == 0) return TIO_OK;
  if (x == nullptr || y == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_add_noise: null argument");
  if (!is_float_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_add_noise: dtype %d", dtype);
  if (batch < 0 || n_per_element < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_add_noise: negative size");
  if (params_batched && (mean_dev == nullptr || std_dev == nullptr))
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_add_noise: params_batched needs mean_dev and std_dev");
  if (base1_dev != nullptr && rician && base2_dev == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_add_noise: rician with base1_dev needs base2_dev");
  if (batch == 0 || n_per_element == 0) return TIO_OK;
  const int64_t quads = (n_per_element + 3) / 4;
  const dim3 grid(static_cast<unsigned>((quads + kBlock - 1) / kBlock), static_cast<unsigned>(batch));
  const bool known = dispatch_float_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(noise_kernel<decltype(dt)::value>, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), x, y,
                       n_per_element, mean, std, mean_dev, std_dev, params_batched, rician, base1_dev, base2_dev,
                       philox_seed, keep_dev);
  });
  return known ? check_launch("tio_add_noise") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_add_noise: dtype %d", dtype);
}

extern "C" int tio_philox_normal(float* out_dev, int64_t n, uint64_t philox_seed, int32_t stream_id, void* stream) {
  if (out_dev == nullptr || n < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_philox_normal: bad argument");
  if (n == 0) return TIO_OK;
  const int64_t quads = (n + 3) / 4;
  hipLaunchKernelGGL(philox_normal_kernel, dim3(static_cast<unsigned>((quads + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), out_dev, n, philox_seed, stream_id);
  return check_launch("tio_philox_normal");
}

extern "C" int tio_gamma_pow(const void* x, void* y, int32_t dtype, int32_t batch, int64_t n_per_element,
                             float gamma, const float* gamma_dev, int32_t params_batched, void* stream) {
  if (batch == 0 || n_per_element == 0) return TIO_OK;
  if (x == nullptr || y == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_gamma_pow: null argument");
  if (!is_float_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_gamma_pow: dtype %d", dtype);
  if (batch < 0 || n_per_element < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_gamma_pow: negative size");
  if (params_batched && gamma_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_gamma_pow: null gamma_dev");
  if (batch == 0 || n_per_element == 0) return TIO_OK;
  const dim3 grid(static_cast<unsigned>((n_per_element + kBlock - 1) / kBlock), static_cast<unsigned>(batch));
  const bool known = dispatch_float_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(gamma_kernel<decltype(dt)::value>, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), x, y,
                       n_per_element, gamma, gamma_dev, params_batched);
  });
  return known ? check_launch("tio_gamma_pow") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_gamma_pow: dtype %d", dtype);
}

extern "C" int tio_channel_min(const void* x, int32_t dtype, int32_t channels, int64_t n_spatial, float* out_dev,
                               void* stream) {
  if (x == nullptr || out_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_channel_min: null argument");
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_channel_min: dtype %d", dtype);
  if (channels < 1 || n_spatial < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_channel_min: empty input");
  hipStream_t s = static_cast<hipStream_t>(stream);
  int ws_cap = 0;
  uint32_t* keys = min_workspace(s, channels, &ws_cap);
  if (keys == nullptr) return fail(TIO_ERR_LAUNCH, "tio_channel_min: cannot allocate the reduction workspace");
  uint32_t* tickets = keys + ws_cap;
  const int64_t want = (n_spatial + kBlock - 1) / kBlock;
  int64_t cap = 512;  // two blocks per CU: measured 18 us per 64 MiB channel (2048 blocks: 34 us, the atomics and block tails add up)
  const unsigned gx = static_cast<unsigned>(want < cap ? want : cap);
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(min_reduce_kernel<decltype(dt)::value>, dim3(gx, static_cast<unsigned>(channels)), dim3(kBlock), 0, s, x, n_spatial, keys, tickets, out_dev);
  });
  return known ? check_launch("tio_channel_min") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_channel_min: dtype %d", dtype);
}
