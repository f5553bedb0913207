// patch_feed.hip — the feeding side of patch-based training on the device (reference data/sampler.py:252-274 WeightedSampler,
// :320-360 LabelSampler; the cutting of :54-67).
//
//   tio_centre_law_sums   one pass over the weight source: the float64 total of every segment of TIO_CENTRE_SEGMENT
//                         consecutive flat voxels (border mask applied from the coordinates, the masked map never stored),
//                         then ONE block turns the totals into inclusive prefix sums, one addition after the other.
//   tio_centre_draw       N draws: t = u * total, binary search of the prefixes, one scan of the segment found.
//   tio_patch_gather      (C, I, J, K) -> (N, C, pi, pj, pk), corners read from device memory.
//
// Nothing here is atomic in floating point, no block waits for another block, and the only loops whose trip count depends
// on data are the binary search (at most 41 steps: 2^40 voxels) and the scan of one segment.
//
// A voxel's weight is a pure function of the source and its flat index (segment_weights), evaluated the same way by the
// sums and by the draw; a segment's total is added in one fixed order (each thread its 8 voxels tid, tid + 256, ... in
// float64, then a stride-halving tree over the 256 threads), so the prefixes depend neither on the grid nor on timing.
#include "common.hpp"
#include "philox_normal.hpp"

namespace tio {
namespace {

constexpr int SEG = TIO_CENTRE_SEGMENT;
constexpr int THREADS = 256;
constexpr int PER_THREAD = SEG / THREADS;
constexpr int SCAN_CHUNK = 4096;  // doubles in LDS per round of the scan (32 KiB)
static_assert(SEG % THREADS == 0 && SEG >= 256, "a segment is a whole number of rounds of the block");

struct LawSource {
  const void* data;
  int32_t type;        // tio_dtype of the source
  int32_t label_mode;  // 0: the source holds the weights; 1: labels looked up in the table
  int32_t n_labels;
  int32_t shape[3], half[3], patch[3];
  int64_t n_voxels;
  double label_values[TIO_CENTRE_MAX_LABELS];
  float label_weights[TIO_CENTRE_MAX_LABELS];
};

__device__ __forceinline__ double load_as_double(const void* p, int type, int64_t i) {
  switch (type) {
    case TIO_F64: return static_cast<const double*>(p)[i];
    case TIO_I64: return static_cast<double>(static_cast<const int64_t*>(p)[i]);
    case TIO_I32: return static_cast<double>(static_cast<const int32_t*>(p)[i]);
    default: return static_cast<double>(load_as_float(p, type, i));  // (float32 holds every value of the narrower types)
  }
}

// `.float()` of the map, or the reference's loop of `weights[labels == label] = weight` (later pairs win); no table: label > 0
__device__ __forceinline__ float raw_weight(const LawSource& s, int64_t flat) {
  if (!s.label_mode) return load_as_float(s.data, s.type, flat);
  const double v = load_as_double(s.data, s.type, flat);
  if (s.n_labels == 0) return v > 0.0 ? 1.0f : 0.0f;
  float w = 0.0f;
  for (int q = 0; q < s.n_labels; q++)
    if (v == s.label_values[q]) w = s.label_weights[q];
  return w;
}

// a patch centred here stays inside the volume (CentreLaw / the reference's _mask_borders): half <= pos < shape - half
__device__ __forceinline__ bool centre_allowed(const LawSource& s, int i, int j, int k) {
  return (s.half[0] == 0 || (i >= s.half[0] && i < s.shape[0] - s.half[0])) && (s.half[1] == 0 || (j >= s.half[1] && j < s.shape[1] - s.half[1])) &&
         (s.half[2] == 0 || (k >= s.half[2] && k < s.shape[2] - s.half[2]));
}

// The masked weights of this thread's voxels of segment `seg`: voxel seg * SEG + q * THREADS + tid for q = 0 .. PER_THREAD - 1
// (0 beyond the volume).  `bad`: an unmasked weight that is negative, infinite or NaN.
__device__ __forceinline__ void segment_weights(const LawSource& s, int64_t seg, float w[PER_THREAD], bool& bad) {
  const int64_t start = seg * SEG;
  const int64_t plane = static_cast<int64_t>(s.shape[1]) * s.shape[2];
  const int64_t i0 = start / plane;  // (uniform in the block)
  const uint32_t rest = static_cast<uint32_t>(start - i0 * plane);
  const uint32_t j0 = rest / static_cast<uint32_t>(s.shape[2]), k0 = rest % static_cast<uint32_t>(s.shape[2]);
  const uint32_t J = static_cast<uint32_t>(s.shape[1]), K = static_cast<uint32_t>(s.shape[2]);
#pragma unroll
  for (int q = 0; q < PER_THREAD; q++) {
    const uint32_t off = static_cast<uint32_t>(q * THREADS) + threadIdx.x;
    const int64_t flat = start + off;
    w[q] = 0.0f;
    if (flat >= s.n_voxels) continue;
    const uint32_t kk = k0 + off, jj = j0 + kk / K;  // (k0 < K <= 2^31 - 1 and off < SEG: no overflow)
    const int64_t i = i0 + jj / J;
    if (!centre_allowed(s, static_cast<int>(i), static_cast<int>(jj % J), static_cast<int>(kk % K))) continue;
    const float v = raw_weight(s, flat);
    bad = bad || !(v >= 0.0f) || v == __builtin_inff();
    w[q] = v;
  }
}

__global__ __launch_bounds__(THREADS) void law_sums_kernel(LawSource s, double* __restrict__ sums, int64_t n_segments, tio_centre_record* record) {
  __shared__ double part[THREADS];
  for (int64_t seg = blockIdx.x; seg < n_segments; seg += gridDim.x) {
    float w[PER_THREAD];
    bool bad = false;
    segment_weights(s, seg, w, bad);
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < PER_THREAD; q++) acc += static_cast<double>(w[q]);
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int stride = THREADS / 2; stride > 0; stride >>= 1) {
      if (static_cast<int>(threadIdx.x) < stride) part[threadIdx.x] += part[threadIdx.x + stride];
      __syncthreads();
    }
    if (threadIdx.x == 0) sums[seg] = part[0];
    if (bad) atomicOr(&record->invalid, 1);  // (an integer flag: the one atomic of this file)
    __syncthreads();                          // part[] is written again by the next segment
  }
}

// One block; the additions are made by ONE thread in ascending order, so prefix[s] = fl(prefix[s - 1] + sum[s]) holds for
// every s and the prefixes never decrease where the sums are not negative — what the binary search and the remainder
// t - prefix[s - 1] of the draw rely on.  The other threads only move the values between memory and LDS.
__global__ __launch_bounds__(THREADS) void law_scan_kernel(double* __restrict__ sums, int64_t n_segments, tio_centre_record* record) {
  __shared__ double buffer[SCAN_CHUNK];
  __shared__ double carry;
  if (threadIdx.x == 0) carry = 0.0;
  __syncthreads();
  for (int64_t base = 0; base < n_segments; base += SCAN_CHUNK) {
    const int len = static_cast<int>(n_segments - base < SCAN_CHUNK ? n_segments - base : SCAN_CHUNK);
    for (int q = threadIdx.x; q < len; q += THREADS) buffer[q] = sums[base + q];
    __syncthreads();
    if (threadIdx.x == 0) {
      double running = carry;
      for (int q = 0; q < len; q++) {
        running += buffer[q];
        buffer[q] = running;
      }
      carry = running;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < len; q += THREADS) sums[base + q] = buffer[q];
    __syncthreads();
  }
  if (threadIdx.x == 0) record->total = carry;
}

// this package's uniform stream: Philox4x32-10, counter {n lo, n hi, 2, 0}, key {seed lo, seed hi}; 53 bits of c[0], c[1]
__device__ __forceinline__ double centre_uniform(uint64_t seed, uint64_t n) {
  uint32_t c[4] = {static_cast<uint32_t>(n), static_cast<uint32_t>(n >> 32), 2u, 0u};
  philox4x32_10(c, static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  const uint64_t bits = (static_cast<uint64_t>(c[0] >> 5) << 26) | static_cast<uint64_t>(c[1] >> 6);
  return static_cast<double>(bits) * 0x1.0p-53;  // (both steps exact: bits < 2^53)
}

__global__ __launch_bounds__(THREADS) void centre_draw_kernel(LawSource s, const double* __restrict__ prefix, int64_t n_segments,
                                                              const tio_centre_record* __restrict__ record, int64_t n_draws, uint64_t seed,
                                                              const double* __restrict__ uniforms, double* __restrict__ uniforms_out,
                                                              int64_t* __restrict__ centres, int32_t* __restrict__ corners) {
  __shared__ float weights[SEG];
  const double total = record->total;
  for (int64_t n = blockIdx.x; n < n_draws; n += gridDim.x) {  // (everything up to the weights is uniform in the block)
    const double u = uniforms != nullptr ? uniforms[n] : centre_uniform(seed, static_cast<uint64_t>(n));
    const double t = u * total;
    int64_t lo = 0, hi = n_segments;  // first segment whose inclusive prefix exceeds t
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (prefix[mid] > t) hi = mid;
      else lo = mid + 1;
    }
    const int64_t seg = lo < n_segments ? lo : n_segments - 1;  // (t >= total after rounding, or a total that is no number)
    float w[PER_THREAD];
    bool bad = false;
    segment_weights(s, seg, w, bad);
#pragma unroll
    for (int q = 0; q < PER_THREAD; q++) weights[q * THREADS + threadIdx.x] = w[q];
    __syncthreads();
    if (threadIdx.x == 0) {
      const double remainder = t - (seg > 0 ? prefix[seg - 1] : 0.0);
      const int64_t left = s.n_voxels - seg * SEG;
      const int len = static_cast<int>(left < SEG ? left : SEG);
      double running = 0.0;
      int pick = -1, last_positive = -1;
      for (int v = 0; v < len; v++) {  // flat order
        const float wv = weights[v];
        running += static_cast<double>(wv);
        if (wv > 0.0f) {
          last_positive = v;
          if (running > remainder) {
            pick = v;
            break;
          }
        }
      }
      if (pick < 0) pick = last_positive;  // rounding left none: the segment's last voxel of positive weight
      int64_t centre = -1;
      int32_t corner[3] = {0, 0, 0};
      if (pick >= 0) {
        centre = seg * SEG + pick;
        const int64_t plane = static_cast<int64_t>(s.shape[1]) * s.shape[2];
        const int64_t i = centre / plane, rest = centre - i * plane;
        const int32_t at[3] = {static_cast<int32_t>(i), static_cast<int32_t>(rest / s.shape[2]), static_cast<int32_t>(rest % s.shape[2])};
        for (int a = 0; a < 3; a++) corner[a] = min(max(at[a] - s.half[a], 0), s.shape[a] - s.patch[a]);
      }
      centres[n] = centre;  // -1: no voxel of positive weight (total 0, or weights that are no numbers)
      corners[3 * n] = corner[0], corners[3 * n + 1] = corner[1], corners[3 * n + 2] = corner[2];
      if (uniforms_out != nullptr) uniforms_out[n] = u;
    }
    __syncthreads();  // weights[] is written again by the next draw
  }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------
struct GatherGeom {
  int32_t shape[3], patch[3];
  int32_t channels;
  int64_t volumes;        // patches * channels
  uint32_t patch_voxels;  // < 2^31 - 256
};

constexpr int GATHER_ROUNDS = 4;  // 16-byte groups per thread

// 16 bytes from an address that is a multiple of ES only: the widest loads its low bits allow
template <int ES>
__device__ __forceinline__ uint4 load_16_bytes(const char* p) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  union {
    uint4 q;
    uint2 d[2];
    uint32_t w[4];
    uint16_t h[8];
    uint8_t b[16];
  } r;
  if ((a & 15) == 0) {
    r.q = *reinterpret_cast<const uint4*>(p);
  } else if ((a & 7) == 0) {
    r.d[0] = reinterpret_cast<const uint2*>(p)[0], r.d[1] = reinterpret_cast<const uint2*>(p)[1];
  } else if (ES >= 4 || (a & 3) == 0) {
#pragma unroll
    for (int e = 0; e < 4; e++) r.w[e] = reinterpret_cast<const uint32_t*>(p)[e];
  } else if (ES >= 2 || (a & 1) == 0) {
#pragma unroll
    for (int e = 0; e < 8; e++) r.h[e] = reinterpret_cast<const uint16_t*>(p)[e];
  } else {
#pragma unroll
    for (int e = 0; e < 16; e++) r.b[e] = reinterpret_cast<const uint8_t*>(p)[e];
  }
  return r.q;
}

// grid.y walks the (patch, channel) pairs, grid.x the 16-byte groups of one patch volume of y, cut at y's own 16-byte
// boundaries: every full group is ONE aligned 16-byte store.  Its source is 16 / ES consecutive elements of one row of x at an
// arbitrary k — one load as wide as that address allows — or, where the group spans the end of a patch row, single elements.
template <int ES>
__global__ __launch_bounds__(256) void patch_gather_kernel(const char* __restrict__ x, char* __restrict__ y, const int32_t* __restrict__ corners,
                                                           GatherGeom g) {
  using T = typename RawBits<ES>::type;
  constexpr int V = 16 / ES;
  const uint32_t pj = static_cast<uint32_t>(g.patch[1]), pk = static_cast<uint32_t>(g.patch[2]);
  const int64_t J = g.shape[1], K = g.shape[2];
  const T* xs = reinterpret_cast<const T*>(x);
  for (int64_t nc = blockIdx.y; nc < g.volumes; nc += gridDim.y) {  // (uniform in the block)
    const int64_t n = nc / g.channels, c = nc - n * g.channels;
    int32_t corner[3];
    for (int a = 0; a < 3; a++) corner[a] = min(max(corners[3 * n + a], 0), g.shape[a] - g.patch[a]);  // whatever the array holds
    const int64_t origin = ((c * g.shape[0] + corner[0]) * J + corner[1]) * K + corner[2];
    T* dst = reinterpret_cast<T*>(y) + nc * g.patch_voxels;
    const uint32_t lead = static_cast<uint32_t>((reinterpret_cast<uintptr_t>(dst) / ES) % V);  // elements since the last 16-byte boundary
    const uint32_t groups = (g.patch_voxels + lead + V - 1) / V;
#pragma unroll
    for (int round = 0; round < GATHER_ROUNDS; round++) {
      const uint32_t group = (blockIdx.x * GATHER_ROUNDS + round) * 256 + threadIdx.x;
      if (group >= groups) continue;
      const int64_t first = static_cast<int64_t>(group) * V - lead;  // element of the patch volume; negative in the first group
      if (first >= 0 && first + V <= static_cast<int64_t>(g.patch_voxels)) {
        const uint32_t v = static_cast<uint32_t>(first);
        uint32_t k = v % pk, row = v / pk;
        uint32_t j = row % pj, i = row / pj;
        uint4 value;
        if (k + V <= pk) {
          value = load_16_bytes<ES>(reinterpret_cast<const char*>(xs + origin + (i * J + j) * K + k));
        } else {
          union {
            uint4 q;
            T e[V];
          } packed;
#pragma unroll
          for (int e = 0; e < V; e++) {
            packed.e[e] = xs[origin + (i * J + j) * K + k];
            if (++k == pk) {
              k = 0;
              if (++j == pj) j = 0, ++i;
            }
          }
          value = packed.q;
        }
        *reinterpret_cast<uint4*>(dst + first) = value;
      } else {
#pragma unroll
        for (int e = 0; e < V; e++) {
          const int64_t at = first + e;
          if (at < 0 || at >= static_cast<int64_t>(g.patch_voxels)) continue;
          const uint32_t v = static_cast<uint32_t>(at);
          const uint32_t k = v % pk, row = v / pk;
          dst[at] = xs[origin + ((row / pj) * J + row % pj) * K + k];
        }
      }
    }
  }
}

int fill_source(const char* who, LawSource& s, const void* weights, int32_t element_type, int32_t label_mode, const double* label_values,
                const float* label_weights, int32_t n_labels, const int32_t shape[3], const int32_t patch[3]) {
  if (!is_known_dtype(element_type)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: unknown element type code %d", who, element_type);
  if (shape == nullptr || patch == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null shape or patch", who);
  if (label_mode != 0 && label_mode != 1) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: label_mode %d (0 or 1)", who, label_mode);
  if (n_labels < 0 || n_labels > TIO_CENTRE_MAX_LABELS || (!label_mode && n_labels != 0))
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: %d table entries (0 .. %d, and none in map mode)", who, n_labels, TIO_CENTRE_MAX_LABELS);
  if (n_labels > 0 && (label_values == nullptr || label_weights == nullptr)) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null label table", who);
  for (int a = 0; a < 3; a++) {
    if (shape[a] < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", who);
    if (patch[a] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: patch size %d along axis %d (at least 1)", who, patch[a], a);
  }
  const int64_t limit = int64_t{1} << 40;
  const int64_t plane = static_cast<int64_t>(shape[1]) * shape[2];
  if (plane > limit || (shape[0] > 0 && plane > limit / shape[0])) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 voxels", who);
  s.data = weights;
  s.type = element_type;
  s.label_mode = label_mode;
  s.n_labels = n_labels;
  for (int a = 0; a < 3; a++) s.shape[a] = shape[a], s.patch[a] = patch[a], s.half[a] = patch[a] / 2;
  s.n_voxels = plane * shape[0];
  for (int q = 0; q < TIO_CENTRE_MAX_LABELS; q++) {
    s.label_values[q] = q < n_labels ? label_values[q] : 0.0;
    s.label_weights[q] = q < n_labels ? label_weights[q] : 0.0f;
  }
  if (s.n_voxels > 0 && weights == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null weights", who);
  if (reinterpret_cast<uintptr_t>(weights) % dtype_size(element_type) != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: weights not aligned to their element", who);
  return TIO_OK;
}

}  // namespace
}  // namespace tio

extern "C" int tio_centre_law_sums(const void* weights, int32_t element_type, int32_t label_mode, const double* label_values,
                                   const float* label_weights, int32_t n_labels, const int32_t shape[3], const int32_t patch[3],
                                   double* prefix_dev, tio_centre_record* record_dev, void* stream) {
  using namespace tio;
  const char* who = "tio_centre_law_sums";
  LawSource s;
  const int status = fill_source(who, s, weights, element_type, label_mode, label_values, label_weights, n_labels, shape, patch);
  if (status != TIO_OK) return status;
  if (record_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null record", who);
  if (reinterpret_cast<uintptr_t>(record_dev) % 8 != 0 || reinterpret_cast<uintptr_t>(prefix_dev) % 8 != 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: prefix sums or record not 8-byte aligned", who);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(record_dev, 0, sizeof(tio_centre_record), st) != hipSuccess) return fail(TIO_ERR_LAUNCH, "%s: clearing the record failed", who);
  const int64_t n_segments = (s.n_voxels + SEG - 1) / SEG;
  if (n_segments == 0) return TIO_OK;
  if (prefix_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null prefix sums", who);
  const dim3 grid(static_cast<unsigned>(n_segments < (1 << 20) ? n_segments : (1 << 20))), block(THREADS);
  hipLaunchKernelGGL(law_sums_kernel, grid, block, 0, st, s, prefix_dev, n_segments, record_dev);
  hipLaunchKernelGGL(law_scan_kernel, dim3(1), block, 0, st, prefix_dev, n_segments, record_dev);
  return check_launch(who);
}

extern "C" int tio_centre_draw(const void* weights, int32_t element_type, int32_t label_mode, const double* label_values, const float* label_weights,
                               int32_t n_labels, const int32_t shape[3], const int32_t patch[3], const double* prefix_dev,
                               const tio_centre_record* record_dev, int64_t n_draws, uint64_t seed, const double* uniforms_dev,
                               double* uniforms_out_dev, int64_t* centres_dev, int32_t* corners_dev, void* stream) {
  using namespace tio;
  const char* who = "tio_centre_draw";
  LawSource s;
  const int status = fill_source(who, s, weights, element_type, label_mode, label_values, label_weights, n_labels, shape, patch);
  if (status != TIO_OK) return status;
  if (n_draws < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative number of draws", who);
  if (n_draws > (int64_t{1} << 40)) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 draws", who);
  if (n_draws == 0) return TIO_OK;
  if (s.n_voxels == 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: draws from an empty volume", who);
  if (prefix_dev == nullptr || record_dev == nullptr || centres_dev == nullptr || corners_dev == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null prefix sums, record or outputs", who);
  if (reinterpret_cast<uintptr_t>(prefix_dev) % 8 != 0 || reinterpret_cast<uintptr_t>(record_dev) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(uniforms_dev) % 8 != 0 || reinterpret_cast<uintptr_t>(uniforms_out_dev) % 8 != 0 ||
      reinterpret_cast<uintptr_t>(centres_dev) % 8 != 0 || reinterpret_cast<uintptr_t>(corners_dev) % 4 != 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: an array is not aligned to its element", who);
  const int64_t n_segments = (s.n_voxels + SEG - 1) / SEG;
  const dim3 grid(static_cast<unsigned>(n_draws < (1 << 20) ? n_draws : (1 << 20))), block(THREADS);
  hipLaunchKernelGGL(centre_draw_kernel, grid, block, 0, static_cast<hipStream_t>(stream), s, prefix_dev, n_segments, record_dev, n_draws,
                     static_cast<uint64_t>(seed), uniforms_dev, uniforms_out_dev, centres_dev, corners_dev);
  return check_launch(who);
}

extern "C" int tio_patch_gather(const void* x, void* y, int32_t element_bytes, int32_t channels, const int32_t shape[3], const int32_t patch[3],
                                const int32_t* corners_dev, int32_t n_patches, void* stream) {
  using namespace tio;
  const char* who = "tio_patch_gather";
  if (element_bytes != 1 && element_bytes != 2 && element_bytes != 4 && element_bytes != 8)
    return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: elements of %d bytes (1, 2, 4 or 8)", who, element_bytes);
  if (shape == nullptr || patch == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null shape or patch", who);
  if (channels < 0 || n_patches < 0 || shape[0] < 0 || shape[1] < 0 || shape[2] < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", who);
  for (int a = 0; a < 3; a++) {
    if (patch[a] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: patch size %d along axis %d (at least 1)", who, patch[a], a);
    if (patch[a] > shape[a])
      return fail(TIO_ERR_INVALID_ARGUMENT, "%s: patch (%d, %d, %d) cannot be larger than the volume (%d, %d, %d)", who, patch[0], patch[1],
                  patch[2], shape[0], shape[1], shape[2]);
  }
  const int64_t limit = int64_t{1} << 40;
  const int64_t plane = static_cast<int64_t>(shape[1]) * shape[2];
  if (plane > limit || plane > limit / shape[0]) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 voxels", who);
  const int64_t n_spatial = plane * shape[0];
  if (channels > 0 && n_spatial > limit / channels) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 elements", who);
  const int64_t patch_voxels = static_cast<int64_t>(patch[0]) * patch[1] * patch[2];
  if (patch_voxels >= (int64_t{1} << 31) - 256) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: a patch of 2^31 voxels or more", who);
  const int64_t volumes = static_cast<int64_t>(n_patches) * channels;
  if (volumes > 0 && patch_voxels > limit / volumes) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 output elements", who);
  if (volumes == 0) return TIO_OK;
  if (x == nullptr || y == nullptr || corners_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null data or corners", who);
  const uintptr_t ax = reinterpret_cast<uintptr_t>(x), ay = reinterpret_cast<uintptr_t>(y);
  const int64_t in_bytes = channels * n_spatial * element_bytes, out_bytes = volumes * patch_voxels * element_bytes;
  if (ax < ay + out_bytes && ay < ax + in_bytes) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: the destination overlaps the source", who);
  if (ax % element_bytes != 0 || ay % element_bytes != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: data not aligned to its element", who);
  if (reinterpret_cast<uintptr_t>(corners_dev) % 4 != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: corners not aligned to their element", who);
  GatherGeom g;
  for (int a = 0; a < 3; a++) g.shape[a] = shape[a], g.patch[a] = patch[a];
  g.channels = channels;
  g.volumes = volumes;
  g.patch_voxels = static_cast<uint32_t>(patch_voxels);
  const int per_group = 16 / element_bytes;
  const int64_t groups = (patch_voxels + 2 * (per_group - 1)) / per_group;  // (the most any destination alignment makes of it)
  const int64_t per_block = 256 * GATHER_ROUNDS;
  const dim3 grid(static_cast<unsigned>((groups + per_block - 1) / per_block), static_cast<unsigned>(volumes < 65535 ? volumes : 65535)), block(256);
  const bool known = dispatch_element_size(element_bytes, [&](auto size) {
    constexpr int ES = decltype(size)::value;
    hipLaunchKernelGGL(patch_gather_kernel<ES>, grid, block, 0, static_cast<hipStream_t>(stream), static_cast<const char*>(x), static_cast<char*>(y),
                       corners_dev, g);
  });
  return known ? check_launch(who) : fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: elements of %d bytes (1, 2, 4 or 8)", who, element_bytes);
}
