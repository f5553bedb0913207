// channel_pca.hip — PCA over the channel axis (reference transforms/intensity/pca.py: _pca_single :83-140).
//
// The reference centres the (voxels, C) matrix, runs torch.pca_lowrank on it (a randomised range finder: a second
// centring, three QR factorisations and about six products over the whole matrix) and projects.  Here the data is read
// twice: tio_channel_scatter makes the channel means and the C x C scatter matrix in float64, the caller takes the
// eigenvectors of that small matrix, and tio_channel_project centres, projects, scales, shifts and clips in one pass.
//
// Scatter.  One wave per block.  A block owns a chunk of voxels of one batch element and a group of up to 8 tile pairs
// (ti, tj0 .. tj0 + G - 1) of one tile row, a tile being 16 channels; it accumulates D_ti D_tj^T over its voxels on the
// float64 matrix cores (v_mfma_f64_16x16x4_f64), D = x - p with the pivot p[c] = x[c, 0] taken in double.  Operand maps
// of that instruction: A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15], one double per lane, so with A = 16 channels x 4
// voxels the B operand of the pair (ti, tj) is the A operand of tile tj and a diagonal pair uses one register for both.
// Any assignment of voxels to k is right as long as A and B share it: lane l loads the four consecutive voxels
// 4 (l >> 4) .. + 3 of its channel at once and feeds four MFMAs, MFMA j taking element j.  The result map is
// col = l & 15, row = (l >> 4) + 4 reg — NOT the row formula of the float32 forms.
// Rows start at x + c V: they share no 16-byte phase, and a voxel must sit in the same k for every channel, so the four
// voxels are read through a 4-byte-aligned vector type and the compiler picks the instruction; the last, partial step of
// a row is read element by element.  Voxels past the end and channels past C enter as d = 0.
// The same lanes add up d per channel (tiles on the diagonal only) for the mean.
// Every block writes its accumulators to its own slot of the workspace.  Above 64 chunks channel_scatter_reduce_kernel
// first adds 64 slots into one (one block adding 2048 slots serially took twenty times as long as the accumulation);
// channel_scatter_finish_kernel adds what is left, forms delta = mean - p and writes S = A - V delta delta^T to both
// triangles.  Every sum runs in ascending slot order and nothing is atomic: two calls give the same bits.
//
// Projection.  Plain VALU, memory bound: a thread owns four consecutive voxels and up to 8 components; per channel it
// reads its voxels (coalesced over the lanes), subtracts the float32 mean, and does one fma per component with a
// weight that is uniform over the block (scalar loads).  More than 8 components: further launches that re-read x.
#include "common.hpp"

namespace tio {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
// four floats at any 4-byte boundary
struct __attribute__((packed, aligned(4))) Float4U {
  float v[4];
};

constexpr int kTile = 16;             // channels per tile
constexpr int kStep = 16;             // voxels per wave step: 4 per lane quarter
constexpr int kMaxGroup = 8;          // tile pairs per block: 8 x 4 doubles = 64 accumulator registers per lane
constexpr int64_t kMinChunk = 512;    // voxels: 32 steps amortise a block's pivot loads and its 2 KiB per pair of partials
constexpr int64_t kTargetBlocks = 8192;  // one wave each: what 256 CUs hold at 8 waves per SIMD
constexpr int kFan = 64;              // chunks one thread adds up: more chunks than this are first reduced kFan to one

struct ScatterPlan {
  int32_t tiles, group, groups, chunks;
  int32_t reduced;       // slots per batch element after the first reduction, 0 when the chunks are few enough to skip it
  int64_t chunk_voxels;
  int64_t slot_doubles;  // one (chunk, batch element): tiles^2 x 256 accumulators, then tiles x 16 sums
};

inline int group_size(int tiles) { return tiles >= 8 ? 8 : tiles > 2 ? 4 : tiles; }

inline int groups_of(int tiles, int group) {
  int n = 0;
  for (int ti = 0; ti < tiles; ti++) n += (tiles - ti + group - 1) / group;
  return n;
}

ScatterPlan make_plan(int32_t batch, int32_t channels, int64_t voxels) {
  ScatterPlan p;
  p.tiles = (channels + kTile - 1) / kTile;
  p.group = group_size(p.tiles);
  p.groups = groups_of(p.tiles, p.group);
  const int64_t per_chunk = static_cast<int64_t>(p.groups) * (batch > 0 ? batch : 1);
  int64_t chunks = (kTargetBlocks + per_chunk - 1) / per_chunk;
  const int64_t most = (voxels + kMinChunk - 1) / kMinChunk;
  if (chunks > most) chunks = most;
  if (chunks < 1) chunks = 1;
  p.chunk_voxels = ((voxels + chunks - 1) / chunks + kStep - 1) / kStep * kStep;
  p.chunks = static_cast<int32_t>((voxels + p.chunk_voxels - 1) / p.chunk_voxels);
  p.reduced = p.chunks > kFan ? (p.chunks + kFan - 1) / kFan : 0;
  p.slot_doubles = static_cast<int64_t>(p.tiles) * p.tiles * 256 + static_cast<int64_t>(p.tiles) * kTile;
  return p;
}

inline int64_t workspace_doubles(const ScatterPlan& p, int32_t batch) { return p.slot_doubles * (p.chunks + p.reduced) * batch; }

// the four voxels v .. v + 3 of one row minus the pivot, 0 past `end` or for a padding channel
__device__ __forceinline__ void load_centred(const float* __restrict__ row, bool channel_ok, int64_t v, int64_t end, double pivot, double d[4]) {
  d[0] = d[1] = d[2] = d[3] = 0.0;
  if (!channel_ok) return;
  if (v + 3 < end) {
    const Float4U q = *reinterpret_cast<const Float4U*>(row + v);
#pragma unroll
    for (int j = 0; j < 4; j++) d[j] = static_cast<double>(q.v[j]) - pivot;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (v + j < end) d[j] = static_cast<double>(row[v + j]) - pivot;
  }
}

// The body of the chunk runs U whole steps at a time: every load of the U steps is issued before the first conversion,
// and the MFMAs go voxel by voxel across the pairs, so that consecutive ones write different accumulators.  One or two
// pairs per block leave too few of those: there the U steps keep a set of accumulators each, added at the end, and the
// loads run one iteration ahead of the arithmetic (these blocks are the memory-bound ones).
template <int G>
__global__ __launch_bounds__(64, (G >= 8 ? 2 : 4)) void channel_scatter_kernel(const float* __restrict__ x, double* __restrict__ workspace, int32_t channels,
                                                             int64_t voxels, ScatterPlan plan) {
  constexpr int U = G >= 4 ? 1 : 2;  // steps in flight (4 and 8 pairs: 20 and 36 floats per lane and step as it is)
  constexpr int S = G <= 2 ? U : 1;  // accumulator sets
  constexpr bool P = G <= 2;         // the next U steps are loaded before this iteration's MFMAs (the registers are there)
  const int lane = threadIdx.x, ch = lane & 15, quarter = lane >> 4;
  int64_t rest = blockIdx.x;
  const int group = static_cast<int>(rest % plan.groups);
  rest /= plan.groups;
  const int chunk = static_cast<int>(rest % plan.chunks);
  const int64_t b = rest / plan.chunks;
  // the group's tile row and first column: rows are laid out one after the other, ceil((T - ti) / G) groups each
  int ti = 0, tj0 = 0;
  for (int g = group; ti < plan.tiles; ti++) {
    const int in_row = (plan.tiles - ti + G - 1) / G;
    if (g < in_row) {
      tj0 = ti + g * G;
      break;
    }
    g -= in_row;
  }
  const float* __restrict__ xb = x + b * channels * voxels;
  const int64_t begin = static_cast<int64_t>(chunk) * plan.chunk_voxels;
  const int64_t end = begin + plan.chunk_voxels < voxels ? begin + plan.chunk_voxels : voxels;

  // a padding channel reads row 0 of the element (memory that exists) and enters as 0
  const int ca = ti * kTile + ch;
  const bool a_ok = ca < channels;
  const float* __restrict__ row_a = xb + static_cast<int64_t>(a_ok ? ca : 0) * voxels;
  const double pivot_a = a_ok ? static_cast<double>(row_a[0]) : 0.0;
  const bool diagonal_first = tj0 == ti;  // (only the first pair of a row's first group can be the diagonal one)
  const float* row_b[G];
  double pivot_b[G];
  bool b_ok[G], live[G], loads[G];
#pragma unroll
  for (int g = 0; g < G; g++) {
    const int cb = (tj0 + g) * kTile + ch;
    live[g] = tj0 + g < plan.tiles;               // (uniform)
    loads[g] = live[g] && !(g == 0 && diagonal_first);  // (uniform: the diagonal pair takes A's registers)
    b_ok[g] = live[g] && cb < channels;
    row_b[g] = xb + static_cast<int64_t>(b_ok[g] ? cb : 0) * voxels;
    pivot_b[g] = b_ok[g] ? static_cast<double>(row_b[g][0]) : 0.0;
  }

  f64x4 acc[S][G];
#pragma unroll
  for (int s = 0; s < S; s++)
#pragma unroll
    for (int g = 0; g < G; g++) acc[s][g] = f64x4{0.0, 0.0, 0.0, 0.0};
  double sum = 0.0;
  const int64_t whole_end = begin + (end - begin) / (U * kStep) * (U * kStep);
  auto load_steps = [&](int64_t v, Float4U(&qa)[U], Float4U(&qb)[G][U]) {
#pragma unroll
    for (int u = 0; u < U; u++) qa[u] = *reinterpret_cast<const Float4U*>(row_a + v + u * kStep);
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (!loads[g]) continue;
#pragma unroll
      for (int u = 0; u < U; u++) qb[g][u] = *reinterpret_cast<const Float4U*>(row_b[g] + v + u * kStep);
    }
  };
  Float4U qa[U], qb[G][U];
  if (P && begin < whole_end) load_steps(begin + 4 * quarter, qa, qb);
  for (int64_t base = begin; base < whole_end; base += U * kStep) {  // (uniform)
    Float4U next_a[U], next_b[G][U];
    if (P) {
      if (base + U * kStep < whole_end) load_steps(base + U * kStep + 4 * quarter, next_a, next_b);
    } else {
      load_steps(base + 4 * quarter, qa, qb);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      double a[4];
#pragma unroll
      for (int j = 0; j < 4; j++) a[j] = a_ok ? static_cast<double>(qa[u].v[j]) - pivot_a : 0.0;
      if (diagonal_first) sum += (a[0] + a[1]) + (a[2] + a[3]);
      double d[G][4];
#pragma unroll
      for (int g = 0; g < G; g++) {
        if (!live[g]) continue;
#pragma unroll
        for (int j = 0; j < 4; j++) d[g][j] = !loads[g] ? a[j] : b_ok[g] ? static_cast<double>(qb[g][u].v[j]) - pivot_b[g] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int g = 0; g < G; g++) {
          if (!live[g]) continue;
          acc[S == 1 ? 0 : u][g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], d[g][j], acc[S == 1 ? 0 : u][g], 0, 0, 0);
        }
      }
    }
    if (P) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        qa[u] = next_a[u];
#pragma unroll
        for (int g = 0; g < G; g++) qb[g][u] = next_b[g][u];
      }
    }
  }
  // what is left of the chunk: fewer than U whole steps and the partial one, element by element where a step ends early
  for (int64_t v = whole_end + 4 * quarter; v - 4 * quarter < end; v += kStep) {
    double a[4];
    load_centred(row_a, a_ok, v, end, pivot_a, a);
    if (diagonal_first) sum += (a[0] + a[1]) + (a[2] + a[3]);
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (!live[g]) continue;
      double d[4];
      if (!loads[g]) {
#pragma unroll
        for (int j = 0; j < 4; j++) d[j] = a[j];
      } else {
        load_centred(row_b[g], b_ok[g], v, end, pivot_b[g], d);
      }
#pragma unroll
      for (int j = 0; j < 4; j++) acc[0][g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], d[j], acc[0][g], 0, 0, 0);
    }
  }

  double* __restrict__ mine = workspace + (b * plan.chunks + chunk) * plan.slot_doubles;
#pragma unroll
  for (int g = 0; g < G; g++) {
    if (!live[g]) continue;
    double* __restrict__ tile = mine + (static_cast<int64_t>(ti) * plan.tiles + tj0 + g) * 256;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      double value = acc[0][g][r];
#pragma unroll
      for (int s = 1; s < S; s++) value += acc[s][g][r];
      tile[r * 64 + lane] = value;
    }
  }
  if (diagonal_first) {
    // the four quarters of a channel, in the order 0 1 2 3
    const double s1 = __shfl(sum, ch + 16), s2 = __shfl(sum, ch + 32), s3 = __shfl(sum, ch + 48);
    if (quarter == 0) mine[static_cast<int64_t>(plan.tiles) * plan.tiles * 256 + ti * kTile + ch] = ((sum + s1) + s2) + s3;
  }
}

// More than kFan chunks: slot r of the second part of the workspace becomes the sum of the chunks r kFan .. r kFan + kFan - 1,
// in ascending order.  grid (slot_doubles / 256, reduced, batch); the tiles below the diagonal are nobody's and are skipped.
__global__ __launch_bounds__(256) void channel_scatter_reduce_kernel(const double* __restrict__ workspace, double* __restrict__ reduced, ScatterPlan plan) {
  const int64_t at = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (at >= plan.slot_doubles) return;
  const int64_t tile = at / 256;
  if (tile < static_cast<int64_t>(plan.tiles) * plan.tiles && tile / plan.tiles > tile % plan.tiles) return;
  const int r = blockIdx.y;
  const int64_t b = blockIdx.z;
  const int last = (r + 1) * kFan < plan.chunks ? (r + 1) * kFan : plan.chunks;
  const double* __restrict__ from = workspace + b * plan.chunks * plan.slot_doubles + at;
  double total = 0.0;
#pragma unroll 8
  for (int k = r * kFan; k < last; k++) total += from[k * plan.slot_doubles];
  reduced[(b * plan.reduced + r) * plan.slot_doubles + at] = total;
}

// One block per (batch element, tile pair ti <= tj): the `count` slots of every accumulator in ascending order, then the
// pivot correction.  Thread t < 256 holds accumulator register t >> 6 of lane t & 63: row (lane >> 4) + 4 reg, column lane & 15.
__global__ __launch_bounds__(320) void channel_scatter_finish_kernel(const float* __restrict__ x, const double* __restrict__ partials, int32_t count,
                                                                     double* __restrict__ mean, double* __restrict__ scatter, int32_t channels,
                                                                     int64_t voxels, ScatterPlan plan) {
  __shared__ double delta[2][kTile];
  const int pairs = plan.tiles * (plan.tiles + 1) / 2;
  const int pair = blockIdx.x % pairs;
  const int64_t b = blockIdx.x / pairs;
  int ti = 0, tj = 0;
  for (int p = pair; ti < plan.tiles; ti++) {
    if (p < plan.tiles - ti) {
      tj = ti + p;
      break;
    }
    p -= plan.tiles - ti;
  }
  const double* __restrict__ first = partials + b * count * plan.slot_doubles;
  const int t = threadIdx.x;
  double total = 0.0;
  if (t >= 256) {  // the fifth wave: the two tiles' channel sums, while the other four add up the accumulators
    const int u = t - 256;
    if (u < 2 * kTile) {
      const int c = (u < kTile ? ti : tj) * kTile + (u & 15);
#pragma unroll 8
      for (int k = 0; k < count; k++) total += first[k * plan.slot_doubles + static_cast<int64_t>(plan.tiles) * plan.tiles * 256 + c];
      const double d = total / static_cast<double>(voxels);
      delta[u >> 4][u & 15] = d;
      if (u < kTile && ti == tj && c < channels) mean[b * channels + c] = static_cast<double>(x[(b * channels + c) * voxels]) + d;
    }
  } else {
    const int64_t at = (static_cast<int64_t>(ti) * plan.tiles + tj) * 256 + t;
#pragma unroll 8
    for (int k = 0; k < count; k++) total += first[k * plan.slot_doubles + at];
  }
  __syncthreads();
  if (t >= 256) return;
  const int lane = t & 63, reg = t >> 6;
  const int row = (lane >> 4) + 4 * reg, col = lane & 15;
  const int i = ti * kTile + row, j = tj * kTile + col;
  if (i >= channels || j >= channels) return;
  const double value = total - static_cast<double>(voxels) * (delta[0][row] * delta[1][col]);
  double* __restrict__ s = scatter + b * channels * channels;
  s[static_cast<int64_t>(i) * channels + j] = value;
  if (ti != tj) s[static_cast<int64_t>(j) * channels + i] = value;
}

// y[b, k0 + k, v] = sum_c W[b, k0 + k, c] (x[b, c, v] - m[b, c]) + o[b, k0 + k] for K components and four voxels per thread
template <int K>
__global__ __launch_bounds__(256) void channel_project_kernel(const float* __restrict__ x, const float* __restrict__ centre,
                                                              const float* __restrict__ weights, const float* __restrict__ offset,
                                                              float* __restrict__ y, int32_t channels, int32_t components, int32_t k0,
                                                              int64_t voxels, int32_t clip) {
  const int64_t b = blockIdx.y;
  const int64_t v = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 4;
  if (v >= voxels) return;
  const float* __restrict__ xb = x + b * channels * voxels + v;
  const float* __restrict__ m = centre + b * channels;
  const float* __restrict__ w = weights + (b * components + k0) * channels;
  const bool whole = v + 3 < voxels;
  float acc[K][4];
#pragma unroll
  for (int k = 0; k < K; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0.0f;
#pragma unroll 4
  for (int c = 0; c < channels; c++) {
    const float* __restrict__ row = xb + static_cast<int64_t>(c) * voxels;
    float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (whole) {
      const Float4U q = *reinterpret_cast<const Float4U*>(row);
#pragma unroll
      for (int j = 0; j < 4; j++) d[j] = q.v[j] - m[c];
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (v + j < voxels) d[j] = row[j] - m[c];
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
      const float wk = w[static_cast<int64_t>(k) * channels + c];
#pragma unroll
      for (int j = 0; j < 4; j++) acc[k][j] = __builtin_fmaf(wk, d[j], acc[k][j]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; k++) {
    const float o = offset[b * components + k0 + k];
    Float4U out;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float r = acc[k][j] + o;
      if (clip) r = r < 0.0f ? 0.0f : (r > 1.0f ? 1.0f : r);  // (both comparisons are false for NaN: it stays, as in torch.clamp)
      out.v[j] = r;
    }
    float* __restrict__ to = y + (b * components + k0 + k) * voxels + v;
    if (whole) {
      *reinterpret_cast<Float4U*>(to) = out;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (v + j < voxels) to[j] = out.v[j];
    }
  }
}

// sizes every entry point of this file refuses; 0 when they are fine
int check_sizes(const char* who, int32_t batch, int32_t channels, int64_t voxels) {
  if (batch < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative batch", who);
  if (channels < 1 || channels > TIO_PCA_MAX_CHANNELS)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: %d channels (1 to %d)", who, channels, TIO_PCA_MAX_CHANNELS);
  if (voxels < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: %lld voxels per channel (at least 1)", who, static_cast<long long>(voxels));
  const int64_t limit = int64_t{1} << 40;
  if (voxels > limit / channels || (batch > 0 && voxels * channels > limit / batch))
    return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 elements", who);
  return TIO_OK;
}

bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace
}  // namespace tio

extern "C" int tio_channel_scatter_plan(int32_t batch, int32_t channels, int64_t voxels, int32_t out[4]) {
  using namespace tio;
  const char* who = "tio_channel_scatter_plan";
  if (out == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null out", who);
  if (const int status = check_sizes(who, batch, channels, voxels)) return status;
  const ScatterPlan p = make_plan(batch, channels, voxels);
  const int64_t grid = static_cast<int64_t>(p.chunks) * p.groups * batch;
  if (p.chunk_voxels > INT32_MAX || grid > INT32_MAX) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: the plan does not fit 32 bits", who);
  out[0] = p.chunks;
  out[1] = static_cast<int32_t>(p.chunk_voxels);
  out[2] = p.group;
  out[3] = static_cast<int32_t>(grid);
  return TIO_OK;
}

extern "C" int64_t tio_channel_scatter_workspace_bytes(int32_t batch, int32_t channels, int64_t voxels) {
  using namespace tio;
  if (check_sizes("tio_channel_scatter_workspace_bytes", batch, channels, voxels) != TIO_OK) return -1;
  const ScatterPlan p = make_plan(batch, channels, voxels);
  return workspace_doubles(p, batch) * static_cast<int64_t>(sizeof(double));
}

extern "C" int tio_channel_scatter(const float* x, int32_t batch, int32_t channels, int64_t voxels, double* mean, double* scatter,
                                   void* workspace_dev, int64_t workspace_bytes, void* stream) {
  using namespace tio;
  const char* who = "tio_channel_scatter";
  if (const int status = check_sizes(who, batch, channels, voxels)) return status;
  if (batch == 0) return TIO_OK;
  if (batch > 65535) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: a batch of more than 65535", who);
  if (x == nullptr || mean == nullptr || scatter == nullptr || workspace_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
  if (!aligned4(x)) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: data not aligned to its element", who);
  if (reinterpret_cast<uintptr_t>(mean) % 8 != 0 || reinterpret_cast<uintptr_t>(scatter) % 8 != 0 || reinterpret_cast<uintptr_t>(workspace_dev) % 8 != 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: mean, scatter and workspace must be 8-byte aligned", who);
  const ScatterPlan p = make_plan(batch, channels, voxels);
  const int64_t need = workspace_doubles(p, batch) * static_cast<int64_t>(sizeof(double));
  if (workspace_bytes < need)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: workspace of %lld bytes, %lld needed", who, static_cast<long long>(workspace_bytes), static_cast<long long>(need));
  const int64_t grid = static_cast<int64_t>(p.chunks) * p.groups * batch;
  const int64_t finish_grid = static_cast<int64_t>(p.tiles) * (p.tiles + 1) / 2 * batch;
  if (grid > INT32_MAX || finish_grid > INT32_MAX) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^31 blocks", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* ws = static_cast<double*>(workspace_dev);
  const dim3 blocks(static_cast<unsigned>(grid)), wave(64);
  switch (p.group) {
    case 1: hipLaunchKernelGGL(channel_scatter_kernel<1>, blocks, wave, 0, s, x, ws, channels, voxels, p); break;
    case 2: hipLaunchKernelGGL(channel_scatter_kernel<2>, blocks, wave, 0, s, x, ws, channels, voxels, p); break;
    case 4: hipLaunchKernelGGL(channel_scatter_kernel<4>, blocks, wave, 0, s, x, ws, channels, voxels, p); break;
    default: hipLaunchKernelGGL(channel_scatter_kernel<kMaxGroup>, blocks, wave, 0, s, x, ws, channels, voxels, p); break;
  }
  if (const int status = check_launch(who)) return status;
  const double* partials = ws;
  int32_t count = p.chunks;
  if (p.reduced > 0) {
    double* reduced = ws + p.slot_doubles * p.chunks * batch;
    const dim3 reduce_grid(static_cast<unsigned>((p.slot_doubles + 255) / 256), static_cast<unsigned>(p.reduced), static_cast<unsigned>(batch));
    hipLaunchKernelGGL(channel_scatter_reduce_kernel, reduce_grid, dim3(256), 0, s, ws, reduced, p);
    if (const int status = check_launch(who)) return status;
    partials = reduced;
    count = p.reduced;
  }
  hipLaunchKernelGGL(channel_scatter_finish_kernel, dim3(static_cast<unsigned>(finish_grid)), dim3(320), 0, s, x, partials, count, mean, scatter, channels,
                     voxels, p);
  return check_launch(who);
}

extern "C" int tio_channel_project(const float* x, int32_t batch, int32_t channels, int64_t voxels, const float* center_dev,
                                   const float* weights_dev, const float* offset_dev, int32_t components, int32_t clip, float* y, void* stream) {
  using namespace tio;
  const char* who = "tio_channel_project";
  if (const int status = check_sizes(who, batch, channels, voxels)) return status;
  if (components < 1 || components > channels) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: %d components of %d channels (1 to the channels)", who, components, channels);
  if (batch == 0) return TIO_OK;
  if (x == nullptr || y == nullptr || center_dev == nullptr || weights_dev == nullptr || offset_dev == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
  if (!aligned4(x) || !aligned4(y) || !aligned4(center_dev) || !aligned4(weights_dev) || !aligned4(offset_dev))
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: data not aligned to its element", who);
  if (batch > 65535) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: a batch of more than 65535", who);
  const int64_t in_bytes = static_cast<int64_t>(batch) * channels * voxels * 4, out_bytes = static_cast<int64_t>(batch) * components * voxels * 4;
  const uintptr_t ax = reinterpret_cast<uintptr_t>(x), ay = reinterpret_cast<uintptr_t>(y);
  if (ax < ay + out_bytes && ay < ax + in_bytes) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: the destination overlaps the source", who);
  const int64_t blocks = (voxels + 1023) / 1024;
  if (blocks > INT32_MAX) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^41 voxels per channel", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(batch)), block(256);
  for (int32_t k0 = 0; k0 < components; k0 += 8) {
    const int32_t n = components - k0 < 8 ? components - k0 : 8;
#define TIO_PROJECT(K) \
  case K: hipLaunchKernelGGL(channel_project_kernel<K>, grid, block, 0, s, x, center_dev, weights_dev, offset_dev, y, channels, components, k0, voxels, clip); break;
    switch (n) {
      TIO_PROJECT(1) TIO_PROJECT(2) TIO_PROJECT(3) TIO_PROJECT(4) TIO_PROJECT(5) TIO_PROJECT(6) TIO_PROJECT(7)
      default: hipLaunchKernelGGL(channel_project_kernel<8>, grid, block, 0, s, x, center_dev, weights_dev, offset_dev, y, channels, components, k0, voxels, clip); break;
    }
#undef TIO_PROJECT
    if (const int status = check_launch(who)) return status;
  }
  return TIO_OK;
}
