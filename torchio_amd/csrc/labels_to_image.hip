// labels_to_image.hip — LabelsToImage (reference transforms/intensity/labels_to_image.py:182-290) for gfx950:
//   tio_labels_to_image   the synthetic image of a label map in ONE pass.  The reference loops over the labels and runs, per
//                         label, a full-volume randn_like, a multiply, an add, a `==` mask, a cast, another multiply and an
//                         accumulate; the masks are disjoint, so every voxel receives exactly one draw with the mean and the
//                         deviation of its own label: one label read, one table lookup, one float32 store per voxel.
// Thread = four consecutive voxels of the FLAT output = one Philox block (the stream of tio_philox_normal over the whole
// output), whatever the row length: a row that starts off a quad shares its first and last block with its neighbours and
// each of them writes its own part.
#include "common.hpp"
#include "label_keys.hpp"
#include "philox_normal.hpp"

namespace tio {
namespace {

constexpr int kThreads = 256;
constexpr int kLdsKeys = 2048;      // at most 32 KiB per block: 16 bytes per key (the key, its mean, its deviation)
constexpr int kBlocksPerRow = 512;  // a block stages its table once and then strides over its row

// the label of voxels [lo, hi) of the quad that starts at `p` (p itself may lie in front of the row when lo > 0): one vector
// load of the four elements where the quad is whole and `vec` says that it is aligned, element by element otherwise
template <typename T>
__device__ __forceinline__ void load_quad(const T* p, bool vec, int lo, int hi, T e[4]) {
  if (vec && lo == 0 && hi == 4) {
    if constexpr (sizeof(T) == 8) {
      const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
      __builtin_memcpy(e, &a, 16);
      __builtin_memcpy(e + 2, &b, 16);
    } else if constexpr (sizeof(T) == 4) {
      const uint4 a = *reinterpret_cast<const uint4*>(p);
      __builtin_memcpy(e, &a, 16);
    } else if constexpr (sizeof(T) == 2) {
      const uint2 a = *reinterpret_cast<const uint2*>(p);
      __builtin_memcpy(e, &a, 8);
    } else {
      const uint32_t a = *reinterpret_cast<const uint32_t*>(p);
      __builtin_memcpy(e, &a, 4);
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < 4; t++)
    if (t >= lo && t < hi) e[t] = p[t];
}

__device__ __forceinline__ void store_quad(float* p, bool vec, int lo, int hi, const float v[4]) {
  if (vec && lo == 0 && hi == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    return;
  }
#pragma unroll
  for (int t = 0; t < 4; t++)
    if (t >= lo && t < hi) p[t] = v[t];
}

// What every thread of a block shares: the row of batch element blockIdx.y in quads of the flat output.
struct Row {
  int64_t g0;      // flat index of the row's first output voxel
  int64_t q0;      // the Philox block that holds it
  int64_t quads;   // blocks the row touches
  int64_t label0;  // element index of the row's first label (channel 0 of the element)
  bool vec_labels, vec_out, vec_base;
};

template <typename T>
__device__ __forceinline__ Row make_row(const T* labels, int channels, int64_t n, const float* out, const float* base) {
  Row r;
  const int64_t b = blockIdx.y;
  r.g0 = b * n;
  r.q0 = r.g0 >> 2;
  r.quads = ((r.g0 + n + 3) >> 2) - r.q0;
  r.label0 = b * channels * n;
  // a whole quad starts at flat index 4 q: its label at element label0 - g0 + 4 q, so one test serves the row
  constexpr uintptr_t kLabelAlign = sizeof(T) >= 4 ? 16 : 4 * sizeof(T);
  r.vec_labels = (reinterpret_cast<uintptr_t>(labels) + static_cast<uintptr_t>(r.label0 - r.g0) * sizeof(T)) % kLabelAlign == 0;
  r.vec_out = reinterpret_cast<uintptr_t>(out) % 16 == 0;
  r.vec_base = reinterpret_cast<uintptr_t>(base) % 16 == 0;
  return r;
}

enum { kByteTable = 0, kSearchLds = 1, kSearchGlobal = 2 };

// Fused mode: out[b, v] = mean[k] + std[k] * z, k the key of labels[b, 0, v]; +0.0 where the label is no key.
template <int DT, int MODE>
__global__ __launch_bounds__(kThreads) void labels_to_image_kernel(const typename Lab<DT>::T* __restrict__ labels, int channels, int64_t n,
                                                                   const double* __restrict__ keys, int n_keys,
                                                                   const float* __restrict__ mean, const float* __restrict__ std,
                                                                   int params_batched, float* __restrict__ out, uint64_t seed) {
  using T = typename Lab<DT>::T;
  // (mean, std) per byte value (static, 2 KiB), or the keys and then (mean, std) per key (dynamic: 16 bytes per key)
  __shared__ float2 lds_table[MODE == kByteTable ? 256 : 1];
  extern __shared__ double lds_keys[];
  float2* lds_params = MODE == kByteTable ? lds_table : reinterpret_cast<float2*>(lds_keys + n_keys);
  const int64_t param0 = params_batched ? static_cast<int64_t>(blockIdx.y) * n_keys : 0;
  // a key whose mean and deviation are both zero is the reference's `continue`: +0.0 whatever the signs of the zeros
  auto params_of = [&](int j) {
    const float m = mean[param0 + j], s = std[param0 + j];
    return (m == 0.0f && s == 0.0f) ? make_float2(0.0f, 0.0f) : make_float2(m, s);
  };
  if constexpr (MODE == kByteTable) {
    lds_params[threadIdx.x] = make_float2(0.0f, 0.0f);
    __syncthreads();
    constexpr double kLow = DT == TIO_I8 ? -128.0 : 0.0, kHigh = DT == TIO_I8 ? 127.0 : 255.0;
    for (int j = threadIdx.x; j < n_keys; j += kThreads) {
      const double key = keys[j];
      if (!(key >= kLow && key <= kHigh)) continue;
      const T as_t = static_cast<T>(key);
      if (static_cast<double>(as_t) == key) lds_params[static_cast<uint8_t>(as_t)] = params_of(j);
    }
    __syncthreads();
  } else if constexpr (MODE == kSearchLds) {
    for (int j = threadIdx.x; j < n_keys; j += kThreads) {
      lds_keys[j] = keys[j];
      lds_params[j] = params_of(j);
    }
    __syncthreads();
  }
  const Row r = make_row<T>(labels, channels, n, out, nullptr);
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; t < r.quads; t += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int64_t q = r.q0 + t, first = 4 * q;
    const int lo = first < r.g0 ? static_cast<int>(r.g0 - first) : 0;
    const int hi = first + 4 > r.g0 + n ? static_cast<int>(r.g0 + n - first) : 4;
    T e[4];
    load_quad<T>(labels + (r.label0 - r.g0 + first), r.vec_labels, lo, hi, e);
    float z[4], v[4];
    philox_normal4(seed, 0, static_cast<uint64_t>(q), z);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (u < lo || u >= hi) continue;
      float2 p;
      if constexpr (MODE == kByteTable) {
        p = lds_params[static_cast<uint8_t>(e[u])];
      } else if constexpr (MODE == kSearchLds) {
        const int j = find_key(lds_keys, n_keys, Lab<DT>::to_double(e[u]));
        p = j >= 0 ? lds_params[j] : make_float2(0.0f, 0.0f);
      } else {
        const int j = find_key(keys, n_keys, Lab<DT>::to_double(e[u]));
        p = j >= 0 ? params_of(j) : make_float2(0.0f, 0.0f);
      }
      v[u] = __fadd_rn(p.x, __fmul_rn(p.y, z[u]));  // labels_to_image.py:215, :287 (0 + (+-0) = +0.0 for a voxel without a key)
    }
    store_quad(out + first, r.vec_out, lo, hi, v);
  }
}

// One-label mode: where the label is keys[base_key], out = mean + std * base (the caller's draw); other voxels are not touched.
template <int DT>
__global__ __launch_bounds__(kThreads) void labels_one_label_kernel(const typename Lab<DT>::T* __restrict__ labels, int channels, int64_t n,
                                                                    const double* __restrict__ keys, int n_keys,
                                                                    const float* __restrict__ mean, const float* __restrict__ std,
                                                                    int params_batched, float* __restrict__ out,
                                                                    const float* __restrict__ base, int base_key) {
  using T = typename Lab<DT>::T;
  const double key = keys[base_key];
  const int64_t at = (params_batched ? static_cast<int64_t>(blockIdx.y) * n_keys : 0) + base_key;
  const float m = mean[at], s = std[at];
  const Row r = make_row<T>(labels, channels, n, out, base);
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; t < r.quads; t += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int64_t first = 4 * (r.q0 + t);
    const int lo = first < r.g0 ? static_cast<int>(r.g0 - first) : 0;
    const int hi = first + 4 > r.g0 + n ? static_cast<int>(r.g0 + n - first) : 4;
    T e[4];
    load_quad<T>(labels + (r.label0 - r.g0 + first), r.vec_labels, lo, hi, e);
    bool any = false;
#pragma unroll
    for (int u = 0; u < 4; u++) any |= u >= lo && u < hi && Lab<DT>::to_double(e[u]) == key;
    if (!any) continue;  // (most quads of most labels: neither the draws nor the output are read)
    float z[4];
    load_quad<float>(base + first, r.vec_base, lo, hi, z);
#pragma unroll
    for (int u = 0; u < 4; u++) {
      if (u < lo || u >= hi || !(Lab<DT>::to_double(e[u]) == key)) continue;
      // randn * std + mean, then `* mask` and `result +=` onto the zeros (labels_to_image.py:214-216, :286-288): the sum with
      // +0.0 changes a -0.0 tissue only
      out[first + u] = __fadd_rn(__fadd_rn(__fmul_rn(z[u], s), m), 0.0f);
    }
  }
}

template <int DT>
void launch(const void* labels, int channels, int64_t n, const double* keys, int n_keys, const float* mean, const float* std, int params_batched,
            float* out, uint64_t seed, const float* base, int base_key, dim3 grid, hipStream_t s) {
  using T = typename Lab<DT>::T;
  const T* x = static_cast<const T*>(labels);
  if (base != nullptr) {
    hipLaunchKernelGGL(labels_one_label_kernel<DT>, grid, dim3(kThreads), 0, s, x, channels, n, keys, n_keys, mean, std, params_batched, out, base, base_key);
  } else if constexpr (DT == TIO_U8 || DT == TIO_I8) {
    hipLaunchKernelGGL((labels_to_image_kernel<DT, kByteTable>), grid, dim3(kThreads), 0, s, x, channels, n, keys, n_keys, mean, std, params_batched, out, seed);
  } else if (n_keys <= kLdsKeys) {
    hipLaunchKernelGGL((labels_to_image_kernel<DT, kSearchLds>), grid, dim3(kThreads), static_cast<size_t>(n_keys) * 16, s, x, channels, n, keys, n_keys, mean, std, params_batched, out, seed);
  } else {
    hipLaunchKernelGGL((labels_to_image_kernel<DT, kSearchGlobal>), grid, dim3(kThreads), 0, s, x, channels, n, keys, n_keys, mean, std, params_batched, out, seed);
  }
}

}  // namespace
}  // namespace tio

extern "C" int tio_labels_to_image(const void* labels, int32_t dtype, int32_t batch, int32_t channels, int64_t n_spatial, const double* keys_dev,
                                   int32_t n_keys, const float* mean_dev, const float* std_dev, int32_t params_batched, float* out,
                                   uint64_t philox_seed, const float* base_dev, int32_t base_key, void* stream) {
  using namespace tio;
  const char* who = "tio_labels_to_image";
  const int es = dtype_size(dtype);
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: unknown dtype %d", who, dtype);
  if (batch < 0 || channels < 0 || n_spatial < 0 || n_keys < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", who);
  if (n_keys > TIO_REMAP_MAX_PAIRS) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: n_keys %d beyond %d", who, n_keys, TIO_REMAP_MAX_PAIRS);
  if (batch > 65535) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 65535 batch elements", who);
  if (base_dev != nullptr && n_keys == 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: one-label mode without keys", who);
  if (base_dev != nullptr && (base_key < 0 || base_key >= n_keys)) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: base_key %d outside [0, %d)", who, base_key, n_keys);
  if (batch == 0 || n_spatial == 0) return TIO_OK;
  if (channels == 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: a label map without channels", who);
  if (labels == nullptr || out == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null labels or output", who);
  if (n_keys > 0 && (keys_dev == nullptr || mean_dev == nullptr || std_dev == nullptr)) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null keys, means or deviations", who);
  if (n_spatial > (int64_t{1} << 40) / batch / channels) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 elements", who);
  if (reinterpret_cast<uintptr_t>(labels) % es != 0 || reinterpret_cast<uintptr_t>(out) % 4 != 0 || reinterpret_cast<uintptr_t>(base_dev) % 4 != 0 ||
      reinterpret_cast<uintptr_t>(keys_dev) % 8 != 0 || reinterpret_cast<uintptr_t>(mean_dev) % 4 != 0 || reinterpret_cast<uintptr_t>(std_dev) % 4 != 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: a pointer is not aligned to its element", who);
  const uintptr_t l0 = reinterpret_cast<uintptr_t>(labels), l1 = l0 + static_cast<uintptr_t>(batch) * channels * n_spatial * es;
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + static_cast<uintptr_t>(batch) * n_spatial * 4;
  if (l0 < o1 && o0 < l1) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: the output overlaps the labels", who);
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(base_dev);
  if (base_dev != nullptr && b0 < o1 && o0 < b0 + (o1 - o0)) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: the output overlaps the draws", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_keys == 0) {  // no key: every voxel is +0.0
    if (hipMemsetAsync(out, 0, static_cast<size_t>(batch) * n_spatial * 4, s) != hipSuccess) return fail(TIO_ERR_LAUNCH, "%s: clearing the output failed", who);
    return TIO_OK;
  }
  const int64_t blocks = (n_spatial / 4 + 2 + kThreads - 1) / kThreads;  // (a row off the quad touches up to n / 4 + 2 blocks)
  const dim3 grid(static_cast<unsigned>(blocks > kBlocksPerRow ? kBlocksPerRow : blocks), static_cast<unsigned>(batch));
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    launch<decltype(dt)::value>(labels, channels, n_spatial, keys_dev, n_keys, mean_dev, std_dev, params_batched != 0, out, philox_seed, base_dev, base_key, grid, s);
  });
  return known ? check_launch(who) : fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: unknown dtype %d", who, dtype);
}
