// label_keys.hpp — a label map's element as the double the reference compares (`data == python_int`) and the search in
// a strictly ascending key list, shared by label_ops.hip and labels_to_image.hip.
#pragma once

#include "common.hpp"

namespace tio {

// ---- element <-> double (the comparisons of the reference are `data == python_int`: exact in double for every dtype
// but int64 beyond 2^53) ---------------------------------------------------------------------------------------------
template <int DT>
struct Lab {
  using T = typename Elem<DT>::type;
  static __device__ __forceinline__ double to_double(T v) { return static_cast<double>(v); }
  static __device__ __forceinline__ T from_double(double d) { return static_cast<T>(d); }
};
template <>
struct Lab<TIO_BF16> {
  using T = uint16_t;
  static __device__ __forceinline__ double to_double(T v) { return static_cast<double>(bf16_bits_to_float(v)); }
  static __device__ __forceinline__ T from_double(double d) { return float_to_bf16_bits(static_cast<float>(d)); }
};

// first index whose key is not below v, then the equality: -1 when v is no key (NaN compares false everywhere: -1)
__device__ __forceinline__ int find_key(const double* keys, int n, double v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && keys[lo] == v) ? lo : -1;
}

}  // namespace tio
