// intensity_stats.hip — intensity preprocessing (reference transforms/intensity/normalize.py, standardize.py, clamp.py,
// mask.py) with the statistics computed on the device:
//   tio_intensity_moments    masked count / mean / unbiased standard deviation: float64 accumulation, per-block partials in
//                            fixed slots merged in a fixed order (bitwise reproducible, no float atomics);
//   tio_intensity_quantiles  exact order statistics by a three-pass radix select (11 / 11 / 10 bits) over an order-preserving
//                            32-bit key of the float32 value, the rank arithmetic on the device;
//   tio_intensity_multi_quantiles  np.percentile for up to 32 fractions and every batch element, left on the device (four passes);
//   tio_histogram_standardize      HistogramStandardization's table and map from those percentiles;
//   tio_intensity_map        the four linear maps, every step a separately rounded float32 operation, IEEE division;
//   tio_intensity_clamp      torch.clamp(min=, max=) with Python-float bounds;
//   tio_intensity_mask       torch.where(mask, x, python_float), the mask broadcast over batch and channels.
// Every kernel reads every dtype code and converts to float32 first, as `.float()` does.
#include "common.hpp"

#include <math.h>
#include <string.h>

#include <type_traits>

namespace tio {
namespace {

// ---- the optional mask: nonzero means inside (`.bool()`: -0.0 is outside, NaN inside) ---------------------------------
struct MaskView {
  const void* data;   // nullptr: every element is inside
  int element_size;   // 1, 2, 4, 8
  int is_float;       // the sign bit does not count
  int64_t period;     // elements of the mask: the data index modulo this is the mask index
};

__device__ __forceinline__ bool mask_nonzero(const MaskView& m, int64_t i) {
  switch (m.element_size) {
    case 1: return static_cast<const uint8_t*>(m.data)[i] != 0;
    case 2: {
      const uint16_t bits = static_cast<const uint16_t*>(m.data)[i];
      return (m.is_float ? (bits & 0x7FFFu) : bits) != 0;
    }
    case 4: {
      const uint32_t bits = static_cast<const uint32_t*>(m.data)[i];
      return (m.is_float ? (bits & 0x7FFFFFFFu) : bits) != 0;
    }
    default: {
      const uint64_t bits = static_cast<const uint64_t*>(m.data)[i];
      return (m.is_float ? (bits & 0x7FFFFFFFFFFFFFFFull) : bits) != 0;
    }
  }
}

// f(float) for every inside element of x[0 : n], 16 bytes of x per load where x allows (the elements in front of the first
// 16-byte boundary and behind the last whole vector go one by one).  The order in which ONE thread sees its elements is a
// function of n, the grid and the pointer's offset from a 16-byte boundary alone.
template <int DT, typename F>
__device__ __forceinline__ void for_each_inside(const void* x_, int64_t n, const MaskView& mask, F f) {
  using T = typename Elem<DT>::type;
  constexpr int PER = 16 / sizeof(T);
  const T* x = static_cast<const T*>(x_);
  int64_t head = static_cast<int64_t>(((16 - reinterpret_cast<uintptr_t>(x) % 16) % 16) / sizeof(T));
  if (head > n) head = n;
  const int64_t vectors = (n - head) / PER;
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x, threads = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const uint4* xv = reinterpret_cast<const uint4*>(x + head);
  for (int64_t v = tid; v < vectors; v += threads) {
    const uint4 raw = xv[v];
    T e[PER];
    __builtin_memcpy(e, &raw, 16);
    const int64_t base = head + v * PER;
    if (mask.data == nullptr) {
#pragma unroll
      for (int j = 0; j < PER; j++) f(Elem<DT>::load(e, j));
    } else {
      int64_t at = base % mask.period;
#pragma unroll
      for (int j = 0; j < PER; j++) {
        if (mask_nonzero(mask, at)) f(Elem<DT>::load(e, j));
        if (++at == mask.period) at = 0;
      }
    }
  }
  const int64_t behind = head + vectors * PER;
  for (int64_t i = tid; i < head + (n - behind); i += threads) {
    const int64_t at = i < head ? i : behind + (i - head);
    if (mask.data == nullptr || mask_nonzero(mask, at % mask.period)) f(Elem<DT>::load(x, at));
  }
}

unsigned reduce_blocks(int64_t n, int cap) {
  const int64_t blocks = (n + 256 * 16 - 1) / (256 * 16);  // 16 elements per thread before a second block pays
  return static_cast<unsigned>(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// ---- masked moments --------------------------------------------------------------------------------------------------
// (count, mean, M2 = sum of squared deviations from the mean) in float64.  A thread sums (x - K) and (x - K)^2 with K its
// first value — a sample of the distribution, so the squares are of the spread's size and `ss - s^2 / n` cancels nothing
// that matters —; threads, then blocks, then the block partials are merged pairwise (Chan et al.) in an order that depends
// on the launch geometry alone.  Infinities and NaN come out as torch has them: a mean of +-inf (NaN when both signs or a NaN
// are present) and a NaN deviation.
constexpr int kMomentBlocks = 1024;

struct Moments {
  double n, mean, m2;
};

__device__ __forceinline__ Moments merge(const Moments& a, const Moments& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Moments r;
  r.n = a.n + b.n;
  const double delta = b.mean - a.mean;
  if (!(fabs(delta) <= 1.7976931348623157e308)) {  // an infinite or NaN mean on a side: inf + finite = inf, inf - inf = NaN
    r.mean = a.mean + b.mean;
    r.m2 = __longlong_as_double(0x7FF8000000000000ll);
    return r;
  }
  r.mean = a.mean + delta * (b.n / r.n);
  r.m2 = a.m2 + b.m2 + delta * delta * (a.n * (b.n / r.n));
  return r;
}

__device__ __forceinline__ Moments block_merge(Moments mine, Moments* lds) {
  lds[threadIdx.x] = mine;
  __syncthreads();
  for (int stride = 128; stride > 0; stride >>= 1) {
    if (static_cast<int>(threadIdx.x) < stride) lds[threadIdx.x] = merge(lds[threadIdx.x], lds[threadIdx.x + stride]);
    __syncthreads();
  }
  return lds[0];
}

template <int DT>
__global__ __launch_bounds__(256) void moments_partial_kernel(const void* __restrict__ x, int64_t n, MaskView mask, Moments* __restrict__ partial) {
  __shared__ Moments lds[256];
  double count = 0.0, shift = 0.0, s = 0.0, ss = 0.0;
  bool shifted = false;
  for_each_inside<DT>(x, n, mask, [&](float v) {
    if (!shifted && fabsf(v) <= 3.4028234663852886e38f) {  // the first FINITE value (inf - inf would make a NaN of an infinite mean)
      shift = static_cast<double>(v);
      shifted = true;
      // (what was summed before is infinite or NaN and stays so whatever the shift)
    }
    const double d = static_cast<double>(v) - shift;
    count += 1.0;
    s += d;
    ss += d * d;
  });
  Moments mine = {0.0, 0.0, 0.0};
  if (count > 0.0) {
    mine.n = count;
    mine.mean = shift + s / count;
    mine.m2 = ss - s * (s / count);
  }
  const Moments all = block_merge(mine, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = all;
}

struct MomentsRecord {
  int64_t count;
  float mean, std;
};

__global__ __launch_bounds__(256) void moments_final_kernel(const Moments* __restrict__ partial, int n_partials, MomentsRecord* __restrict__ record) {
  __shared__ Moments lds[256];
  Moments mine = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n_partials; i += 256) mine = merge(mine, partial[i]);
  const Moments all = block_merge(mine, lds);
  if (threadIdx.x == 0) {
    record->count = static_cast<int64_t>(all.n);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    // torch: the mean of nothing and the unbiased deviation of one value are NaN.  Only a finite negative m2 (rounding) is
    // clamped: a NaN m2 — a NaN or an infinity among the values — must stay NaN (fmax would return the other operand)
    const double mean = all.n > 0.0 ? all.mean : nan;
    const double m2 = all.m2 < 0.0 ? 0.0 : all.m2;
    const double variance = all.n > 1.0 ? m2 / (all.n - 1.0) : nan;
    record->mean = static_cast<float>(mean);          // the one rounding to float32
    record->std = static_cast<float>(sqrt(variance));
  }
}

// ---- exact selection -------------------------------------------------------------------------------------------------
// key: ascending unsigned order = ascending float order, -0 directly below +0, every NaN at the top (torch.kthvalue sorts
// NaN last).
__device__ __forceinline__ uint32_t select_key(float f) {
  if (f != f) return 0xFFFFFFFFu;
  const uint32_t bits = __float_as_uint(f);
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float select_value(uint32_t key) {
  if (key == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

constexpr int kSelectBins = 2048, kSelectRanks = 4, kSelectBlocks = 2048;

struct SelectState {
  unsigned long long n;                    // inside elements (pass 1's total)
  unsigned long long rank[kSelectRanks];   // 0-based rank of distinct rank r among the elements that share prefix[r]
  uint32_t prefix[kSelectRanks];           // the key bits resolved so far
  int32_t n_ranks;                         // distinct ranks, 0 when n == 0
  int32_t slot[kSelectRanks];              // (q0 lower, q0 upper, q1 lower, q1 upper) -> distinct rank
};

struct QuantileRecord {
  float lower, upper;
  int64_t n;
};

// Equal digits in a row become one LDS atomic: a constant volume or a block of exact zeros sends every element of a
// thread to the same bin, and 64 lanes adding to one address go through the LDS one after the other.
struct RunAdd {
  int digit = -1;
  unsigned count = 0;
  __device__ __forceinline__ void add(unsigned* hist, int d) {
    if (d == digit) {
      count++;
    } else {
      if (count) atomicAdd(hist + digit, count);
      digit = d;
      count = 1;
    }
  }
  __device__ __forceinline__ void flush(unsigned* hist) {
    if (count) atomicAdd(hist + digit, count);
    count = 0;
  }
};

// PASS 1: the top 11 bits of every inside element (one histogram); PASS 2 / 3: the next 11 / the last 10 bits of the
// elements whose higher bits are a rank's prefix, one histogram per distinct rank.
template <int DT, int PASS>
__global__ __launch_bounds__(256) void select_histogram_kernel(const void* __restrict__ x, int64_t n, MaskView mask,
                                                               const SelectState* __restrict__ state, unsigned long long* __restrict__ hist) {
  constexpr int HISTS = PASS == 1 ? 1 : kSelectRanks;
  constexpr int SHIFT = PASS == 1 ? 21 : (PASS == 2 ? 10 : 0);   // the digit's position
  constexpr int ABOVE = PASS == 2 ? 21 : 10;                     // bits below the prefix of passes 2 and 3
  constexpr uint32_t DIGIT_MASK = PASS == 3 ? 0x3FFu : 0x7FFu;
  __shared__ unsigned lds[HISTS * kSelectBins];
  const int n_ranks = PASS == 1 ? 1 : state->n_ranks;
  for (int i = threadIdx.x; i < n_ranks * kSelectBins; i += 256) lds[i] = 0u;
  uint32_t prefix[kSelectRanks] = {0u, 0u, 0u, 0u};
  if (PASS != 1) {
#pragma unroll
    for (int r = 0; r < kSelectRanks; r++) prefix[r] = r < n_ranks ? state->prefix[r] : 0u;
  }
  __syncthreads();
  if (n_ranks == 0) return;  // (uniform: nothing is inside)
  RunAdd run[HISTS];
  for_each_inside<DT>(x, n, mask, [&](float v) {
    const uint32_t key = select_key(v);
    if (PASS == 1) {
      run[0].add(lds, static_cast<int>(key >> SHIFT));
    } else {
#pragma unroll
      for (int r = 0; r < HISTS; r++)
        if (r < n_ranks && ((key ^ prefix[r]) >> ABOVE) == 0u) run[r].add(lds + r * kSelectBins, static_cast<int>((key >> SHIFT) & DIGIT_MASK));
    }
  });
#pragma unroll
  for (int r = 0; r < HISTS; r++) run[r].flush(lds + r * kSelectBins);
  __syncthreads();
  for (int i = threadIdx.x; i < n_ranks * kSelectBins; i += 256)
    if (lds[i]) atomicAdd(hist + i, static_cast<unsigned long long>(lds[i]));  // integer sums: the order does not matter
}

// Inside one block of 256 threads: each owns 8 consecutive bins of a 2048-bin histogram.  scan_bins leaves the thread's bins in
// `mine` and the sum of all bins in front of them in `*before` (scan[255] is the histogram's total afterwards); find_bin has the
// thread whose bins hold `rank` (0-based, below the total) write the bin and the rank inside it.
constexpr int kOwnBins = kSelectBins / 256;

__device__ __forceinline__ void scan_bins(const unsigned long long* hist, unsigned long long* scan, unsigned long long mine[kOwnBins],
                                          unsigned long long* before) {
  unsigned long long sum = 0ull;
#pragma unroll
  for (int j = 0; j < kOwnBins; j++) {
    mine[j] = hist[threadIdx.x * kOwnBins + j];
    sum += mine[j];
  }
  __syncthreads();  // (the previous user of `scan` has read it)
  scan[threadIdx.x] = sum;
  __syncthreads();
  for (int offset = 1; offset < 256; offset <<= 1) {
    const unsigned long long add = static_cast<int>(threadIdx.x) >= offset ? scan[threadIdx.x - offset] : 0ull;
    __syncthreads();
    scan[threadIdx.x] += add;
    __syncthreads();
  }
  *before = scan[threadIdx.x] - sum;
}

__device__ __forceinline__ void find_bin(unsigned long long rank, const unsigned long long mine[kOwnBins], unsigned long long before,
                                         int* found_bin, unsigned long long* found_rank) {
#pragma unroll
  for (int j = 0; j < kOwnBins; j++) {
    if (rank >= before && rank < before + mine[j]) {
      *found_bin = static_cast<int>(threadIdx.x) * kOwnBins + j;
      *found_rank = rank - before;
    }
    before += mine[j];
  }
  __syncthreads();
}

// One block after each data pass: narrows every rank's prefix, zeroes the histograms the pass has used for the next pass, and
// — after pass 3 — writes the records.  Pass 1 also turns the fractions into ranks: lower = floor(q * (n - 1)) with the two
// float64 operations of the reference's compute_quantile, upper = min(lower + 1, n - 1).
template <int PASS>
__global__ __launch_bounds__(256) void select_scan_kernel(SelectState* state, unsigned long long* hist, double q0, double q1, int n_q,
                                                          QuantileRecord* __restrict__ record) {
  __shared__ unsigned long long scan[256];
  __shared__ int found_bin;
  __shared__ unsigned long long found_rank;
  __shared__ unsigned long long want[kSelectRanks];
  __shared__ int n_want;
  unsigned long long mine[kOwnBins], before;
  int n_ranks;
  if (PASS == 1) {
    scan_bins(hist, scan, mine, &before);  // the one histogram of pass 1 serves every rank
    if (threadIdx.x == 0) {
      const unsigned long long n = scan[255];
      state->n = n;
      int distinct = 0;
      if (n > 0ull) {
        for (int k = 0; k < 2 * n_q; k++) {
          const double q = k < 2 ? q0 : q1;
          const double index = q * static_cast<double>(n - 1ull);
          unsigned long long rank = static_cast<unsigned long long>(floor(index));
          if (k & 1) rank = rank + 1ull < n ? rank + 1ull : n - 1ull;
          int at = 0;
          while (at < distinct && want[at] != rank) at++;
          if (at == distinct) want[distinct++] = rank;
          state->slot[k] = at;
        }
      }
      n_want = distinct;
      state->n_ranks = distinct;
    }
    __syncthreads();
    n_ranks = n_want;
  } else {
    n_ranks = state->n_ranks;
  }
  for (int r = 0; r < n_ranks; r++) {
    if (PASS != 1) scan_bins(hist + r * kSelectBins, scan, mine, &before);
    find_bin(PASS == 1 ? want[r] : state->rank[r], mine, before, &found_bin, &found_rank);
    if (threadIdx.x == 0) {
      const uint32_t digit = static_cast<uint32_t>(found_bin);
      state->prefix[r] = PASS == 1 ? digit << 21 : (PASS == 2 ? state->prefix[r] | (digit << 10) : state->prefix[r] | digit);
      state->rank[r] = found_rank;
    }
    __syncthreads();
  }
  // what this pass's data kernel has added to: pass 1 one histogram, pass 2 one per rank; after pass 3 nothing reads them again
  if (PASS != 3)
    for (int i = threadIdx.x; i < (PASS == 1 ? 1 : n_ranks) * kSelectBins; i += 256) hist[i] = 0ull;
  if (PASS == 3 && static_cast<int>(threadIdx.x) < n_q) {
    QuantileRecord out;
    out.n = static_cast<int64_t>(state->n);
    if (n_ranks == 0) {
      out.lower = out.upper = __uint_as_float(0x7FC00000u);
    } else {
      out.lower = select_value(state->prefix[state->slot[2 * threadIdx.x]]);
      out.upper = select_value(state->prefix[state->slot[2 * threadIdx.x + 1]]);
    }
    record[threadIdx.x] = out;
  }
}

constexpr int64_t kSelectHistBytes = static_cast<int64_t>(kSelectRanks) * kSelectBins * sizeof(unsigned long long);
constexpr int64_t kStatsWorkspaceBytes = kSelectHistBytes + 256;  // the histograms, then the state
static_assert(kStatsWorkspaceBytes >= static_cast<int64_t>(kMomentBlocks * sizeof(Moments)), "the moments' partials share the workspace");
static_assert(sizeof(SelectState) <= 256, "the state's place in the workspace");

// ---- elementwise streams: y[i] = f(x[i], i), TI in, TO out, 16 bytes per access on the narrower side where both pointers
// allow it (a group of G elements: 16 bytes of the narrower type); otherwise element by element ------------------------
template <typename TI, typename TO, typename F>
__device__ __forceinline__ void stream_convert(const TI* x, TO* y, int64_t n, F f) {
  constexpr int NARROW = sizeof(TI) < sizeof(TO) ? sizeof(TI) : sizeof(TO);
  constexpr int G = 16 / NARROW;
  constexpr int AI = G * sizeof(TI) < 16 ? G * sizeof(TI) : 16, AO = G * sizeof(TO) < 16 ? G * sizeof(TO) : 16;
  const uintptr_t ax = reinterpret_cast<uintptr_t>(x), ay = reinterpret_cast<uintptr_t>(y);
  int64_t head = n;  // no common boundary: everything goes one by one
  for (int h = 0; h < G; h++) {
    if ((ax + h * sizeof(TI)) % AI == 0 && (ay + h * sizeof(TO)) % AO == 0) {
      head = h < n ? h : n;
      break;
    }
  }
  const int64_t groups = (n - head) / G;
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x, threads = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t g = tid; g < groups; g += threads) {
    const int64_t base = head + g * G;
    TI in[G];
    TO out[G];
    __builtin_memcpy(in, __builtin_assume_aligned(x + base, AI), G * sizeof(TI));
#pragma unroll
    for (int j = 0; j < G; j++) out[j] = f(in[j], base + j);
    __builtin_memcpy(__builtin_assume_aligned(y + base, AO), out, G * sizeof(TO));
  }
  const int64_t behind = head + groups * G;
  for (int64_t i = tid; i < head + (n - behind); i += threads) {
    const int64_t at = i < head ? i : behind + (i - head);
    y[at] = f(x[at], at);
  }
}

unsigned stream_blocks(int64_t n) {
  const int64_t blocks = (n / 4 + 255) / 256;
  return static_cast<unsigned>(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
}

// ---- the linear maps -------------------------------------------------------------------------------------------------
struct MapParams {
  int mode;
  float in_min, in_max, in_range, out_min, out_range;
  const float* out_min_dev;    // (B,) or nullptr: the scalars
  const float* out_range_dev;
  int64_t n_per_element;
};

// torch.clamp: a NaN stays a NaN, the bounds are applied as min(max(x, lo), hi)
__device__ __forceinline__ float clip(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

template <int DT>
__global__ __launch_bounds__(256) void map_kernel(const typename Elem<DT>::type* __restrict__ x, float* __restrict__ y, int64_t n, MapParams p) {
  using T = typename Elem<DT>::type;
  int64_t lo = 0, hi = 0;  // the batch element of the last index seen: its range of indices and its parameters
  float out_min = p.out_min, out_range = p.out_range;
  stream_convert<T, float>(x, y, n, [&](T raw, int64_t i) {
    const float v = Elem<DT>::load(&raw, 0);
    if (p.out_min_dev != nullptr && (i < lo || i >= hi)) {
      const int64_t b = i / p.n_per_element;
      lo = b * p.n_per_element;
      hi = lo + p.n_per_element;
      out_min = p.out_min_dev[b];
      out_range = p.out_range_dev[b];
    }
    // (-ffp-contract=off: each operation below rounds to float32 on its own, the division is IEEE)
    switch (p.mode) {
      case TIO_MAP_RESCALE_CLIP: return (clip(v, p.in_min, p.in_max) - p.in_min) / p.in_range * out_range + out_min;
      case TIO_MAP_RESCALE:
        if (p.out_min_dev != nullptr && out_range == 0.0f) return v;  // _RescaleInverse: such an element stays
        return (v - out_min) / out_range * p.in_range + p.in_min;
      case TIO_MAP_SUB_DIV: return (v - p.in_min) / p.in_range;
      default: return v * p.in_range + p.in_min;
    }
  });
}

// ---- clamp and mask: the result dtype of torch's type promotion with a Python float ------------------------------------
//   float64 stays float64 (compared in float64), float16 / bfloat16 / float32 stay (the scalar is cast to the dtype; the
//   comparison of two such values in float32 is the comparison in the dtype), every integer dtype becomes float32.
template <int DT>
struct Promoted {
  using Out = float;
  using Work = float;
  static __device__ __forceinline__ Work load(typename Elem<DT>::type v) { return Elem<DT>::load(&v, 0); }
  static __device__ __forceinline__ Out store(Work v) { return v; }
};
template <>
struct Promoted<TIO_F64> {
  using Out = double;
  using Work = double;
  static __device__ __forceinline__ Work load(double v) { return v; }
  static __device__ __forceinline__ Out store(Work v) { return v; }
};
template <>
struct Promoted<TIO_F16> {
  using Out = _Float16;
  using Work = float;
  static __device__ __forceinline__ Work load(_Float16 v) { return static_cast<float>(v); }
  static __device__ __forceinline__ Out store(Work v) { return static_cast<_Float16>(v); }  // (v is a float16 value: exact)
};
template <>
struct Promoted<TIO_BF16> {
  using Out = uint16_t;
  using Work = float;
  static __device__ __forceinline__ Work load(uint16_t v) { return bf16_bits_to_float(v); }
  static __device__ __forceinline__ Out store(Work v) { return float_to_bf16_bits(v); }  // (exact likewise)
};

template <int DT>
__global__ __launch_bounds__(256) void clamp_kernel(const typename Elem<DT>::type* __restrict__ x, typename Promoted<DT>::Out* __restrict__ y, int64_t n,
                                                    int has_min, double lo_, int has_max, double hi_) {
  using P = Promoted<DT>;
  using W = typename P::Work;
  const W lo = static_cast<W>(lo_), hi = static_cast<W>(hi_);
  stream_convert<typename Elem<DT>::type, typename P::Out>(x, y, n, [&](typename Elem<DT>::type raw, int64_t) {
    W v = P::load(raw);
    if (v == v) {
      if (has_min) v = v < lo ? lo : v;
      if (has_max) v = v > hi ? hi : v;
    }
    return P::store(v);
  });
}

template <int DT>
__global__ __launch_bounds__(256) void mask_kernel(const typename Elem<DT>::type* __restrict__ x, typename Promoted<DT>::Out* __restrict__ y, int64_t n,
                                                   MaskView mask, double outside_) {
  using P = Promoted<DT>;
  const typename P::Out outside = P::store(static_cast<typename P::Work>(outside_));
  int64_t last = -2, at = 0;  // consecutive indices walk the mask without a division
  stream_convert<typename Elem<DT>::type, typename P::Out>(x, y, n, [&](typename Elem<DT>::type raw, int64_t i) {
    if (i != last + 1) at = i % mask.period;
    else if (++at == mask.period) at = 0;
    last = i;
    return mask_nonzero(mask, at) ? P::store(P::load(raw)) : outside;
  });
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// the pass number of a selection kernel, handed to a generic lambda as a compile-time constant
template <int N>
using Pass = std::integral_constant<int, N>;

// a Python float as the dtype's scalar (c10::Scalar::to<T>: through float32 for the 16-bit floats), back as a double
double scalar_in_dtype(double v, int dtype) {
  if (dtype == TIO_F64) return v;
  float f = static_cast<float>(v);
  if (dtype == TIO_F16) f = static_cast<float>(static_cast<_Float16>(f));
  if (dtype == TIO_BF16 && f == f) {
    uint32_t bits;
    memcpy(&bits, &f, 4);
    bits += 0x7FFFu + ((bits >> 16) & 1u);
    bits &= 0xFFFF0000u;
    memcpy(&f, &bits, 4);
  }
  return static_cast<double>(f);
}

// the checks the two statistics share; *n is channels * n_spatial
int check_stats_arguments(const char* who, const void* x, int dtype, int channels, int64_t n_spatial, const void* mask, int mask_dtype,
                          int mask_channels, const void* record, const void* workspace, int64_t workspace_bytes, MaskView* view, int64_t* n) {
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: unknown dtype %d", who, dtype);
  if (mask != nullptr && !is_known_dtype(mask_dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: unknown mask dtype %d", who, mask_dtype);
  if (channels < 0 || n_spatial < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", who);
  if (mask != nullptr && mask_channels != 1 && mask_channels != channels)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: %d mask channels for %d data channels (1 or as many)", who, mask_channels, channels);
  if (record == nullptr || workspace == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null record or workspace", who);
  if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0 || reinterpret_cast<uintptr_t>(record) % 8 != 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: the workspace must be 16-byte aligned, the record 8-byte", who);
  if (workspace_bytes < kStatsWorkspaceBytes)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: workspace of %lld bytes is too small", who, static_cast<long long>(workspace_bytes));
  if (channels > 0 && n_spatial > (int64_t{1} << 40) / channels) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 elements", who);
  *n = static_cast<int64_t>(channels) * n_spatial;
  if (*n > 0 && x == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null data", who);
  view->data = *n > 0 ? mask : nullptr;
  view->element_size = mask != nullptr ? dtype_size(mask_dtype) : 1;
  view->is_float = mask != nullptr && is_float_dtype(mask_dtype);
  view->period = mask != nullptr && mask_channels * n_spatial > 0 ? mask_channels * n_spatial : 1;
  return TIO_OK;
}

// ---- selection for many ranks and every batch element (HistogramStandardization) ----------------------------------------
// The same key as above, for up to 32 fractions and each batch element on its own, finished on the device as np.percentile
// finishes it.  Four data passes of 11 / 7 / 7 / 7 bits.  Pass 1 is one histogram per element, common to all ranks.  In the
// later passes the ranks that share a prefix share a histogram (they count the same elements): an element looks its top digit
// up in a table in LDS, finds the group with its prefix, if any, and adds to that group's 128-bin histogram IN LDS.  Why not
// wider digits behind global atomics: a percentile lies where the data is dense, so most elements of a smooth distribution
// still match a group in pass 2 (measured on 8 x 256^3 white noise: 2.3 ms for that pass with 11-bit digits in global memory,
// 0.36 ms here), and discrete data matches in every pass.  With 7-bit digits all 65 groups fit in LDS (512 bytes each) and no
// pass depends on what the data looks like; the price is a fourth read.
constexpr int kMultiFractions = 32, kMultiRanks = 2 * kMultiFractions + 1;  // a lower and an upper rank per fraction, and the top rank: a NaN sorts last
constexpr int kMultiBins = 128;                                             // passes 2 to 4

struct MultiState {  // one per batch element
  unsigned long long n;
  unsigned long long rank[kMultiRanks];  // distinct, ascending; from pass 1 on the rank among the elements that share the prefix
  double gamma[kMultiFractions];
  uint32_t prefix[kMultiRanks];
  uint32_t group_prefix[kMultiRanks];    // distinct, ascending
  int32_t group[kMultiRanks];            // rank -> group
  int32_t lower[kMultiFractions], upper[kMultiFractions];  // fraction -> rank slot
  int32_t top, n_ranks, n_groups, pad;
};
constexpr int64_t kMultiStateBytes = 2048;
static_assert(sizeof(MultiState) <= kMultiStateBytes && sizeof(MultiState) % 4 == 0, "the state's place in the workspace");

struct MultiFractions {
  double q[kMultiFractions];
};

// bits below the prefix that passes 2, 3 and 4 match; their digit is the 7 bits below that
__host__ __device__ constexpr int multi_above(int pass) { return 35 - 7 * pass; }

// grid (blocks, batch).  hist1: [batch][2048]; hist_groups: [batch][ranks_cap][128].  Dynamic LDS: ranks_cap * 128 counters
// (passes 2 to 4).
template <int DT, int PASS>
__global__ __launch_bounds__(256) void multi_histogram_kernel(const void* __restrict__ x_, int64_t n, MaskView mask, const MultiState* __restrict__ states,
                                                              unsigned long long* __restrict__ hist1, unsigned long long* __restrict__ hist_groups,
                                                              int ranks_cap) {
  using T = typename Elem<DT>::type;
  __shared__ unsigned lds[kSelectBins];  // pass 1: the histogram; later: top digit -> first group | groups << 16
  __shared__ uint32_t group_prefix[kMultiRanks];
  extern __shared__ unsigned group_hist[];
  const int b = blockIdx.y;
  const void* x = static_cast<const T*>(x_) + static_cast<int64_t>(b) * n;
  for (int i = threadIdx.x; i < kSelectBins; i += 256) lds[i] = 0u;
  if (PASS == 1) {
    __syncthreads();
    RunAdd run;
    for_each_inside<DT>(x, n, mask, [&](float v) { run.add(lds, static_cast<int>(select_key(v) >> 21)); });
    run.flush(lds);
    __syncthreads();
    for (int i = threadIdx.x; i < kSelectBins; i += 256)
      if (lds[i]) atomicAdd(hist1 + static_cast<int64_t>(b) * kSelectBins + i, static_cast<unsigned long long>(lds[i]));
    return;
  }
  constexpr int ABOVE = multi_above(PASS), SHIFT = ABOVE - 7;
  const MultiState& state = states[b];
  const int n_groups = state.n_groups;
  if (n_groups == 0) return;  // (uniform: nothing is inside)
  for (int i = threadIdx.x; i < n_groups * kMultiBins; i += 256) group_hist[i] = 0u;
  if (static_cast<int>(threadIdx.x) < n_groups) group_prefix[threadIdx.x] = state.group_prefix[threadIdx.x];
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < n_groups) {  // the first group of each top digit counts its followers
    const int g = threadIdx.x;
    const uint32_t digit = group_prefix[g] >> 21;
    if (g == 0 || (group_prefix[g - 1] >> 21) != digit) {
      int count = 1;
      while (g + count < n_groups && (group_prefix[g + count] >> 21) == digit) count++;
      lds[digit] = static_cast<unsigned>(g) | (static_cast<unsigned>(count) << 16);
    }
  }
  __syncthreads();
  RunAdd run;
  for_each_inside<DT>(x, n, mask, [&](float v) {
    const uint32_t key = select_key(v);
    const unsigned entry = lds[key >> 21];
    if (entry == 0u) return;
    // the groups' prefixes ascend: the one that equals the key's, if any, among those that share its top digit
    int lo = static_cast<int>(entry & 0xFFFFu), hi = lo + static_cast<int>(entry >> 16) - 1;
    const uint32_t want = key >> ABOVE;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((group_prefix[mid] >> ABOVE) < want) lo = mid + 1;
      else hi = mid;
    }
    if ((group_prefix[lo] >> ABOVE) == want) run.add(group_hist, lo * kMultiBins + static_cast<int>((key >> SHIFT) & 0x7Fu));
  });
  run.flush(group_hist);
  __syncthreads();
  unsigned long long* hist = hist_groups + static_cast<int64_t>(b) * ranks_cap * kMultiBins;
  for (int i = threadIdx.x; i < n_groups * kMultiBins; i += 256)
    if (group_hist[i]) atomicAdd(hist + i, static_cast<unsigned long long>(group_hist[i]));  // integer sums: the order does not matter
}

// the exclusive prefix sums of a 2048-bin histogram into cum (each of 256 threads owns 8 bins); returns the total
__device__ __forceinline__ unsigned long long cumulate(const unsigned long long* hist, unsigned long long* scan, unsigned long long* cum) {
  unsigned long long mine[kOwnBins], before;
  scan_bins(hist, scan, mine, &before);
#pragma unroll
  for (int j = 0; j < kOwnBins; j++) {
    cum[threadIdx.x * kOwnBins + j] = before;
    before += mine[j];
  }
  __syncthreads();
  return scan[255];
}

// the bin that holds `rank` (below the total): the last bin whose exclusive prefix sum is <= rank
__device__ __forceinline__ int bin_of_rank(const unsigned long long* cum, unsigned long long rank) {
  int lo = 0, hi = kSelectBins - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cum[mid] <= rank) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ranks ascend, so their prefixes do: equal prefixes are neighbours
__device__ __forceinline__ void regroup(MultiState& st) {
  int groups = 0;
  for (int r = 0; r < st.n_ranks; r++) {
    if (r == 0 || st.prefix[r] != st.prefix[r - 1]) st.group_prefix[groups++] = st.prefix[r];
    st.group[r] = groups - 1;
  }
  st.n_groups = groups;
}

// One block per batch element after each data pass.  Pass 1 turns the fractions into ranks by numpy's rule
// (_function_base_impl.py: virtual = q * (n - 1) with q = (100 q) / 100 as the reference passes it, lower = floor(virtual),
// gamma = virtual - lower); every pass narrows each rank's prefix (and zeroes the group histograms it has read, for the next
// pass); pass 4 writes np.percentile's values:
//   _lerp: d = b - a in the array's dtype (float32), then in float64 a + d * gamma, or b - d * (1 - gamma) for gamma >= 0.5;
//   a NaN anywhere (the top rank tells) or n == 0: NaN.
template <int PASS>
__global__ __launch_bounds__(256) void multi_scan_kernel(MultiState* __restrict__ states, const unsigned long long* __restrict__ hist1,
                                                         unsigned long long* __restrict__ hist_groups, int ranks_cap, MultiFractions fractions, int n_fractions,
                                                         double* __restrict__ out, int64_t* __restrict__ counts) {
  __shared__ unsigned long long scan[256];
  __shared__ unsigned long long cum[kSelectBins];
  __shared__ MultiState st;
  const int b = blockIdx.x;
  uint32_t* st_words = reinterpret_cast<uint32_t*>(&st);
  uint32_t* global_words = reinterpret_cast<uint32_t*>(states + b);
  constexpr int kWords = sizeof(MultiState) / 4;
  if (PASS == 1) {
    const unsigned long long n = cumulate(hist1 + static_cast<int64_t>(b) * kSelectBins, scan, cum);
    if (threadIdx.x == 0) {
      st.n = n;
      st.n_ranks = st.n_groups = 0;
      st.top = 0;
      if (n > 0ull) {
        unsigned long long wanted[kMultiRanks];
        int n_wanted = 0;
        for (int f = 0; f < n_fractions; f++) {
          const double q = 100.0 * fractions.q[f] / 100.0;
          const double virtual_index = q * static_cast<double>(n - 1ull);
          unsigned long long lower = static_cast<unsigned long long>(floor(virtual_index));
          if (lower > n - 1ull) lower = n - 1ull;
          st.gamma[f] = virtual_index - static_cast<double>(lower);
          wanted[n_wanted++] = lower;
          wanted[n_wanted++] = lower + 1ull < n ? lower + 1ull : n - 1ull;
        }
        wanted[n_wanted++] = n - 1ull;
        int distinct = 0;
        for (int k = 0; k < n_wanted; k++) {  // insert into the ascending list
          int at = 0;
          while (at < distinct && st.rank[at] < wanted[k]) at++;
          if (at < distinct && st.rank[at] == wanted[k]) continue;
          for (int m = distinct; m > at; m--) st.rank[m] = st.rank[m - 1];
          st.rank[at] = wanted[k];
          distinct++;
        }
        for (int k = 0; k < n_wanted; k++) {
          int at = 0;
          while (st.rank[at] != wanted[k]) at++;
          if (k == n_wanted - 1) st.top = at;
          else if (k & 1) st.upper[k >> 1] = at;
          else st.lower[k >> 1] = at;
        }
        st.n_ranks = distinct;
      }
    }
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < st.n_ranks) {
      const int digit = bin_of_rank(cum, st.rank[threadIdx.x]);
      st.prefix[threadIdx.x] = static_cast<uint32_t>(digit) << 21;
      st.rank[threadIdx.x] -= cum[digit];
    }
  } else {
    for (int i = threadIdx.x; i < kWords; i += 256) st_words[i] = global_words[i];
    __syncthreads();
    unsigned long long* hist = hist_groups + static_cast<int64_t>(b) * ranks_cap * kMultiBins;
    if (static_cast<int>(threadIdx.x) < st.n_ranks) {  // a rank walks the 128 bins of its group
      const unsigned long long* mine = hist + st.group[threadIdx.x] * kMultiBins;
      unsigned long long rank = st.rank[threadIdx.x];
      int digit = 0;
      while (digit < kMultiBins - 1 && rank >= mine[digit]) rank -= mine[digit++];
      st.prefix[threadIdx.x] |= static_cast<uint32_t>(digit) << (multi_above(PASS) - 7);
      st.rank[threadIdx.x] = rank;
    }
    __syncthreads();
    if (PASS != 4)
      for (int i = threadIdx.x; i < st.n_groups * kMultiBins; i += 256) hist[i] = 0ull;
  }
  __syncthreads();
  if (PASS != 4) {
    if (threadIdx.x == 0) regroup(st);
    __syncthreads();
    for (int i = threadIdx.x; i < kWords; i += 256) global_words[i] = st_words[i];
    return;
  }
  if (threadIdx.x == 0) counts[b] = static_cast<int64_t>(st.n);
  if (static_cast<int>(threadIdx.x) < n_fractions) {
    double result = __longlong_as_double(0x7FF8000000000000ll);
    if (st.n > 0ull) {
      const float top = select_value(st.prefix[st.top]);
      if (top == top) {
        const float lower = select_value(st.prefix[st.lower[threadIdx.x]]), upper = select_value(st.prefix[st.upper[threadIdx.x]]);
        const double difference = static_cast<double>(upper - lower);  // (rounded to float32 first)
        const double gamma = st.gamma[threadIdx.x];
        result = gamma >= 0.5 ? static_cast<double>(upper) - difference * (1.0 - gamma) : static_cast<double>(lower) + difference * gamma;
      }
    }
    out[static_cast<int64_t>(b) * n_fractions + threadIdx.x] = result;
  }
}

int64_t multi_workspace_bytes(int64_t batch, int n_fractions) {
  const int64_t ranks_cap = 2 * n_fractions + 1;
  return batch * ((kSelectBins + ranks_cap * kMultiBins) * static_cast<int64_t>(sizeof(unsigned long long)) + kMultiStateBytes);
}

// ---- HistogramStandardization: the table, then the map (histogram_standardization.py:276-303) ---------------------------
constexpr int kMaxLandmarks = kMultiFractions;

// table: [batch][3][kMaxLandmarks] float32 — slopes, intercepts, inner edges.  Every step is a float32 operation of its own.
__global__ __launch_bounds__(256) void standardize_table_kernel(const double* __restrict__ percentiles, const float* __restrict__ landmarks, int n_landmarks,
                                                                int batch, float* __restrict__ table) {
  for (int b = threadIdx.x; b < batch; b += 256) {
    float* slopes = table + static_cast<int64_t>(b) * 3 * kMaxLandmarks;
    float *intercepts = slopes + kMaxLandmarks, *edges = intercepts + kMaxLandmarks;
    const double* mine = percentiles + static_cast<int64_t>(b) * n_landmarks;
    for (int i = 0; i + 1 < n_landmarks; i++) {
      const float low = static_cast<float>(mine[i]), high = static_cast<float>(mine[i + 1]);  // torch.as_tensor(pv, dtype=float32)
      float diff_input = high - low;
      const float diff_landmarks = landmarks[i + 1] - landmarks[i];
      if (fabsf(diff_input) < 1e-5f) diff_input = __uint_as_float(0x7F800000u);  // a flat segment: slope 0
      const float slope = diff_landmarks / diff_input;
      slopes[i] = slope;
      intercepts[i] = landmarks[i] - slope * low;
      if (i > 0) edges[i - 1] = low;
    }
  }
}

template <int DT>
__device__ __forceinline__ typename Elem<DT>::type value_in_dtype(float v) {
  typename Elem<DT>::type out;
  Elem<DT>::store(&out, 0, v);
  return out;
}

// grid (blocks, batch): bin = the number of inner edges below x (torch.bucketize, right=False), y = slope[bin] * x + intercept[bin]
template <int DT>
__global__ __launch_bounds__(256) void standardize_apply_kernel(const typename Elem<DT>::type* __restrict__ x, typename Elem<DT>::type* __restrict__ y,
                                                                int64_t n_per_element, const float* __restrict__ table, int n_landmarks) {
  using T = typename Elem<DT>::type;
  __shared__ float lds[3 * kMaxLandmarks];
  const int b = blockIdx.y;
  if (threadIdx.x < 3 * kMaxLandmarks) lds[threadIdx.x] = table[static_cast<int64_t>(b) * 3 * kMaxLandmarks + threadIdx.x];
  __syncthreads();
  const float *slopes = lds, *intercepts = lds + kMaxLandmarks, *edges = lds + 2 * kMaxLandmarks;
  const int n_edges = n_landmarks - 2;
  stream_convert<T, T>(x + static_cast<int64_t>(b) * n_per_element, y + static_cast<int64_t>(b) * n_per_element, n_per_element, [&](T raw, int64_t) {
    const float v = Elem<DT>::load(&raw, 0);
    int bin = 0;
    if (v != v) {
      bin = n_edges;  // (bucketize puts a NaN behind every edge; the product is NaN whatever the bin)
    } else {
      for (int e = 0; e < n_edges; e++) bin += edges[e] < v ? 1 : 0;
    }
    return value_in_dtype<DT>(slopes[bin] * v + intercepts[bin]);  // (-ffp-contract=off: a product, then a sum)
  });
}

}  // namespace
}  // namespace tio

extern "C" int64_t tio_intensity_stats_workspace_bytes(void) { return tio::kStatsWorkspaceBytes; }

extern "C" int tio_intensity_moments(const void* x, int32_t dtype, int32_t channels, int64_t n_spatial, const void* mask, int32_t mask_dtype,
                                     int32_t mask_channels, void* record_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  using namespace tio;
  MaskView view;
  int64_t n = 0;
  if (const int rc = check_stats_arguments("tio_intensity_moments", x, dtype, channels, n_spatial, mask, mask_dtype, mask_channels, record_dev,
                                           workspace_dev, workspace_bytes, &view, &n))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  Moments* partial = static_cast<Moments*>(workspace_dev);
  const unsigned blocks = reduce_blocks(n, kMomentBlocks);
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(moments_partial_kernel<decltype(dt)::value>, dim3(blocks), dim3(256), 0, s, x, n, view, partial);
  });
  if (!known) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_intensity_moments: unknown dtype %d", dtype);
  if (const int rc = check_launch("tio_intensity_moments (partials)")) return rc;
  hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(256), 0, s, partial, static_cast<int>(blocks), static_cast<MomentsRecord*>(record_dev));
  return check_launch("tio_intensity_moments");
}

extern "C" int tio_intensity_quantiles(const void* x, int32_t dtype, int32_t channels, int64_t n_spatial, const void* mask, int32_t mask_dtype,
                                       int32_t mask_channels, const double* fractions, int32_t n_fractions, void* record_dev,
                                       void* workspace_dev, int64_t workspace_bytes, void* stream) {
  using namespace tio;
  if (fractions == nullptr || n_fractions < 1 || n_fractions > 2)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_quantiles: one or two fractions, got %d", n_fractions);
  for (int k = 0; k < n_fractions; k++)
    if (!(fractions[k] >= 0.0 && fractions[k] <= 1.0))
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_quantiles: fraction %g outside [0, 1]", fractions[k]);
  MaskView view;
  int64_t n = 0;
  if (const int rc = check_stats_arguments("tio_intensity_quantiles", x, dtype, channels, n_spatial, mask, mask_dtype, mask_channels, record_dev,
                                           workspace_dev, workspace_bytes, &view, &n))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* hist = static_cast<unsigned long long*>(workspace_dev);
  SelectState* state = reinterpret_cast<SelectState*>(static_cast<char*>(workspace_dev) + kSelectHistBytes);
  QuantileRecord* record = static_cast<QuantileRecord*>(record_dev);
  // (the workspace may hold anything: zeroed once here; between the passes the scan kernels zero what the pass has used)
  if (hipMemsetAsync(hist, 0, kSelectHistBytes, s) != hipSuccess) return fail(TIO_ERR_LAUNCH, "tio_intensity_quantiles: memset failed");
  const dim3 grid(reduce_blocks(n, kSelectBlocks)), block(256);
  const double q0 = fractions[0], q1 = n_fractions > 1 ? fractions[1] : fractions[0];
  const auto histogram = [&](auto pass, const char* what) {
    const bool known = dispatch_dtype(dtype, [&](auto dt) {
      hipLaunchKernelGGL((select_histogram_kernel<decltype(dt)::value, decltype(pass)::value>), grid, block, 0, s, x, n, view, state, hist);
    });
    return known ? check_launch(what) : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_intensity_quantiles: unknown dtype %d", dtype);
  };
  if (const int rc = histogram(Pass<1>{}, "tio_intensity_quantiles (pass 1)")) return rc;
  hipLaunchKernelGGL(select_scan_kernel<1>, dim3(1), block, 0, s, state, hist, q0, q1, n_fractions, record);
  if (const int rc = check_launch("tio_intensity_quantiles (scan 1)")) return rc;
  if (const int rc = histogram(Pass<2>{}, "tio_intensity_quantiles (pass 2)")) return rc;
  hipLaunchKernelGGL(select_scan_kernel<2>, dim3(1), block, 0, s, state, hist, q0, q1, n_fractions, record);
  if (const int rc = check_launch("tio_intensity_quantiles (scan 2)")) return rc;
  if (const int rc = histogram(Pass<3>{}, "tio_intensity_quantiles (pass 3)")) return rc;
  hipLaunchKernelGGL(select_scan_kernel<3>, dim3(1), block, 0, s, state, hist, q0, q1, n_fractions, record);
  return check_launch("tio_intensity_quantiles");
}

extern "C" int tio_intensity_map(const void* x, float* y, int32_t dtype, int32_t batch, int64_t n_per_element, int32_t mode, float in_min,
                                 float in_max, float in_range, float out_min, float out_range, const float* out_min_dev,
                                 const float* out_range_dev, void* stream) {
  using namespace tio;
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_intensity_map: unknown dtype %d", dtype);
  if (batch < 0 || n_per_element < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_map: negative size");
  if (mode < TIO_MAP_RESCALE_CLIP || mode > TIO_MAP_MUL_ADD) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_map: unknown mode %d", mode);
  if ((out_min_dev == nullptr) != (out_range_dev == nullptr))
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_map: per-element out_min and out_range come together");
  if (out_min_dev != nullptr && mode != TIO_MAP_RESCALE_CLIP && mode != TIO_MAP_RESCALE)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_map: mode %d takes no per-element parameters", mode);
  if (batch > 0 && n_per_element > (int64_t{1} << 40) / batch) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "tio_intensity_map: more than 2^40 elements");
  const int64_t n = static_cast<int64_t>(batch) * n_per_element;
  if (n == 0) return TIO_OK;
  if (x == nullptr || y == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_map: null argument");
  const MapParams p = {mode, in_min, in_max, in_range, out_min, out_range, out_min_dev, out_range_dev, n_per_element};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(stream_blocks(n)), block(256);
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL(map_kernel<DT>, grid, block, 0, s, static_cast<const typename Elem<DT>::type*>(x), y, n, p);
  });
  return known ? check_launch("tio_intensity_map") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_intensity_map: unknown dtype %d", dtype);
}

extern "C" int tio_intensity_clamp(const void* x, void* y, int32_t dtype, int64_t n, int32_t has_min, double out_min, int32_t has_max,
                                   double out_max, void* stream) {
  using namespace tio;
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_intensity_clamp: unknown dtype %d", dtype);
  if (n < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_clamp: negative size");
  if (!has_min && !has_max) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_clamp: at least one of the bounds");
  if ((has_min && out_min != out_min) || (has_max && out_max != out_max)) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_clamp: a bound is NaN");
  if (n == 0) return TIO_OK;
  if (x == nullptr || y == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_clamp: null argument");
  const double lo = scalar_in_dtype(out_min, dtype), hi = scalar_in_dtype(out_max, dtype);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(stream_blocks(n)), block(256);
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL(clamp_kernel<DT>, grid, block, 0, s, static_cast<const typename Elem<DT>::type*>(x), static_cast<typename Promoted<DT>::Out*>(y), n,
                       has_min, lo, has_max, hi);
  });
  return known ? check_launch("tio_intensity_clamp") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_intensity_clamp: unknown dtype %d", dtype);
}

extern "C" int tio_intensity_mask(const void* x, void* y, int32_t dtype, int64_t n, const void* mask, int32_t mask_dtype, int64_t mask_n,
                                  double outside_value, void* stream) {
  using namespace tio;
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_intensity_mask: unknown dtype %d", dtype);
  if (!is_known_dtype(mask_dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_intensity_mask: unknown mask dtype %d", mask_dtype);
  if (n < 0 || mask_n < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_mask: negative size");
  if (n == 0) return TIO_OK;
  if (mask_n == 0 || n % mask_n != 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_mask: %lld data elements are no multiple of %lld mask elements", static_cast<long long>(n),
                static_cast<long long>(mask_n));
  if (x == nullptr || y == nullptr || mask == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_intensity_mask: null argument");
  const MaskView view = {mask, dtype_size(mask_dtype), is_float_dtype(mask_dtype) ? 1 : 0, mask_n};
  const double outside = scalar_in_dtype(outside_value, is_float_dtype(dtype) ? dtype : TIO_F32);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(stream_blocks(n)), block(256);
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    hipLaunchKernelGGL(mask_kernel<DT>, grid, block, 0, s, static_cast<const typename Elem<DT>::type*>(x), static_cast<typename Promoted<DT>::Out*>(y), n, view,
                       outside);
  });
  return known ? check_launch("tio_intensity_mask") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_intensity_mask: unknown dtype %d", dtype);
}

extern "C" int64_t tio_intensity_multi_quantiles_workspace_bytes(int32_t batch, int32_t n_fractions) {
  if (batch < 0 || n_fractions < 1 || n_fractions > tio::kMultiFractions) return 0;
  return tio::multi_workspace_bytes(batch, n_fractions);
}

extern "C" int tio_intensity_multi_quantiles(const void* x, int32_t dtype, int32_t batch, int32_t channels, int64_t n_spatial, const void* mask,
                                             int32_t mask_dtype, int32_t mask_channels, const double* fractions, int32_t n_fractions,
                                             double* values_dev, int64_t* counts_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  using namespace tio;
  const char* who = "tio_intensity_multi_quantiles";
  if (fractions == nullptr || n_fractions < 1 || n_fractions > kMultiFractions)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: 1 to %d fractions, got %d", who, kMultiFractions, n_fractions);
  MultiFractions q;
  for (int k = 0; k < kMultiFractions; k++) q.q[k] = k < n_fractions ? fractions[k] : 0.0;
  for (int k = 0; k < n_fractions; k++)
    if (!(q.q[k] >= 0.0 && q.q[k] <= 1.0)) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: fraction %g outside [0, 1]", who, q.q[k]);
  if (batch < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", who);
  if (counts_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null record or workspace", who);
  MaskView view;
  int64_t n = 0;
  // (the workspace's size is checked below: the shared check knows the single-element selection's only)
  if (const int rc = check_stats_arguments(who, x, dtype, channels, n_spatial, mask, mask_dtype, mask_channels, values_dev, workspace_dev,
                                           kStatsWorkspaceBytes, &view, &n))
    return rc;
  const int64_t needed = multi_workspace_bytes(batch, n_fractions);
  if (workspace_bytes < needed)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: workspace of %lld bytes is too small (%lld)", who, static_cast<long long>(workspace_bytes),
                static_cast<long long>(needed));
  if (batch > 0 && n > (int64_t{1} << 40) / batch) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 elements", who);
  if (batch > 65535) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 65535 batch elements", who);
  if (batch == 0) return TIO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int ranks_cap = 2 * n_fractions + 1;
  unsigned long long* hist1 = static_cast<unsigned long long*>(workspace_dev);
  unsigned long long* hist_groups = hist1 + static_cast<int64_t>(batch) * kSelectBins;
  MultiState* states = reinterpret_cast<MultiState*>(hist_groups + static_cast<int64_t>(batch) * ranks_cap * kMultiBins);
  // (the workspace may hold anything: the histograms are zeroed here; the scans zero what the next pass adds to again)
  if (hipMemsetAsync(hist1, 0, static_cast<size_t>(batch) * (kSelectBins + ranks_cap * kMultiBins) * sizeof(unsigned long long), s) != hipSuccess)
    return fail(TIO_ERR_LAUNCH, "%s: memset failed", who);
  const dim3 grid(reduce_blocks(n, kSelectBlocks), batch), block(256), one(batch);
  const size_t group_lds = static_cast<size_t>(ranks_cap) * kMultiBins * sizeof(unsigned);  // at most 33 280 bytes
  const auto histogram = [&](auto pass, const char* what) {
    constexpr int PASS = decltype(pass)::value;
    const bool known = dispatch_dtype(dtype, [&](auto dt) {
      hipLaunchKernelGGL((multi_histogram_kernel<decltype(dt)::value, PASS>), grid, block, PASS == 1 ? 0 : group_lds, s, x, n, view, states, hist1,
                         hist_groups, ranks_cap);
    });
    return known ? check_launch(what) : fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: unknown dtype %d", who, dtype);
  };
  const auto scan = [&](auto pass) {
    hipLaunchKernelGGL(multi_scan_kernel<decltype(pass)::value>, one, block, 0, s, states, hist1, hist_groups, ranks_cap, q, n_fractions, values_dev, counts_dev);
  };
  if (const int rc = histogram(Pass<1>{}, "tio_intensity_multi_quantiles (pass 1)")) return rc;
  scan(Pass<1>{});
  if (const int rc = check_launch("tio_intensity_multi_quantiles (scan 1)")) return rc;
  if (const int rc = histogram(Pass<2>{}, "tio_intensity_multi_quantiles (pass 2)")) return rc;
  scan(Pass<2>{});
  if (const int rc = check_launch("tio_intensity_multi_quantiles (scan 2)")) return rc;
  if (const int rc = histogram(Pass<3>{}, "tio_intensity_multi_quantiles (pass 3)")) return rc;
  scan(Pass<3>{});
  if (const int rc = check_launch("tio_intensity_multi_quantiles (scan 3)")) return rc;
  if (const int rc = histogram(Pass<4>{}, "tio_intensity_multi_quantiles (pass 4)")) return rc;
  scan(Pass<4>{});
  return check_launch(who);
}

extern "C" int tio_histogram_standardize(const void* x, void* y, int32_t dtype, int32_t batch, int64_t n_per_element, const double* percentiles_dev,
                                         const float* landmarks_dev, int32_t n_landmarks, float* table_dev, void* stream) {
  using namespace tio;
  const char* who = "tio_histogram_standardize";
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: unknown dtype %d", who, dtype);
  if (batch < 0 || n_per_element < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", who);
  if (n_landmarks < 2 || n_landmarks > kMaxLandmarks) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: 2 to %d landmarks, got %d", who, kMaxLandmarks, n_landmarks);
  if (batch > 0 && n_per_element > (int64_t{1} << 40) / batch) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 elements", who);
  if (batch > 65535) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 65535 batch elements", who);
  if (batch == 0 || n_per_element == 0) return TIO_OK;
  if (x == nullptr || y == nullptr || percentiles_dev == nullptr || landmarks_dev == nullptr || table_dev == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null argument", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(standardize_table_kernel, dim3(1), dim3(256), 0, s, percentiles_dev, landmarks_dev, n_landmarks, batch, table_dev);
  if (const int rc = check_launch("tio_histogram_standardize (table)")) return rc;
  const dim3 grid(stream_blocks(n_per_element), batch), block(256);
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    using T = typename Elem<decltype(dt)::value>::type;
    hipLaunchKernelGGL(standardize_apply_kernel<decltype(dt)::value>, grid, block, 0, s, static_cast<const T*>(x), static_cast<T*>(y), n_per_element, table_dev,
                       n_landmarks);
  });
  return known ? check_launch(who) : fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: unknown dtype %d", who, dtype);
}
