// label_ops.hip — the label-map transforms (reference transforms/label/*.py) as integer-exact kernels:
//   tio_label_remap             RemapLabels / RemoveLabels / SequentialLabels: every pair in ONE pass (the reference runs
//                               a full-volume compare and a masked write per pair);
//   tio_label_one_hot           OneHot: the input is read once, num_classes float32 streams are written;
//   tio_label_contour           Contour: the 3x3x3 minimum as a march along I over a J x K tile in LDS;
//   tio_keep_largest_component  KeepLargestComponent: connected components of all listed labels at once, on the device
//                               (the reference copies one mask per label and element to the host for SimpleITK).
#include "common.hpp"
#include "label_keys.hpp"

namespace tio {
namespace {

// y[i] = f(x[i]) with 16-byte loads and stores wherever x and y share their offset from a 16-byte boundary (the
// elements in front of the first boundary and behind the last whole vector go one by one); x == y is allowed: every
// element is read and written by the same thread.
template <typename T, typename F>
__device__ __forceinline__ void stream_map(const T* x, T* y, int64_t n, F f) {
  constexpr int PER = 16 / sizeof(T);
  const uintptr_t ax = reinterpret_cast<uintptr_t>(x), ay = reinterpret_cast<uintptr_t>(y);
  int64_t head = static_cast<int64_t>(((16 - ax % 16) % 16) / sizeof(T));
  if (ay % 16 != ax % 16 || head > n) head = n;
  const int64_t vectors = (n - head) / PER;
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x, threads = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const uint4* xv = reinterpret_cast<const uint4*>(x + head);
  uint4* yv = reinterpret_cast<uint4*>(y + head);
  for (int64_t i = tid; i < vectors; i += threads) {
    uint4 raw = xv[i];
    T e[PER];
    __builtin_memcpy(e, &raw, 16);
#pragma unroll
    for (int j = 0; j < PER; j++) e[j] = f(e[j]);
    __builtin_memcpy(&raw, e, 16);
    yv[i] = raw;
  }
  const int64_t behind = head + vectors * PER;
  for (int64_t i = tid; i < head + (n - behind); i += threads) {
    const int64_t at = i < head ? i : behind + (i - head);
    y[at] = f(x[at]);
  }
}

// ---- remap ----------------------------------------------------------------------------------------------------------
constexpr int kRemapLdsPairs = 2048;  // 32 KiB of keys and values per block

// 8-bit data: the whole map is a 256-entry table in LDS, indexed by the byte
template <int DT>
__global__ __launch_bounds__(256) void remap_byte_kernel(const typename Lab<DT>::T* x, typename Lab<DT>::T* y, int64_t n,
                                                         const double* __restrict__ keys, const double* __restrict__ values, int n_pairs,
                                                         int keep, double constant) {
  using T = typename Lab<DT>::T;
  __shared__ T table[256];
  table[threadIdx.x] = keep ? static_cast<T>(static_cast<uint8_t>(threadIdx.x)) : Lab<DT>::from_double(constant);
  __syncthreads();
  for (int j = threadIdx.x; j < n_pairs; j += 256) {
    const double key = keys[j];
    const T as_t = Lab<DT>::from_double(key >= -128.0 && key <= 255.0 ? key : 0.0);
    if (Lab<DT>::to_double(as_t) == key) table[static_cast<uint8_t>(as_t)] = Lab<DT>::from_double(values[j]);
  }
  __syncthreads();
  stream_map<T>(x, y, n, [&](T v) { return table[static_cast<uint8_t>(v)]; });
}

// int16 data: a 65536-entry table in global memory (it stays in L2; a label map touches a few lines of it), made by
// one block in front of the streaming launch
__global__ __launch_bounds__(1024) void remap_build_table_kernel(int16_t* __restrict__ table, const double* __restrict__ keys,
                                                                 const double* __restrict__ values, int n_pairs, int keep, double constant) {
  const int16_t fill = static_cast<int16_t>(constant);
  for (int i = threadIdx.x; i < 65536; i += 1024) table[i] = keep ? static_cast<int16_t>(static_cast<uint16_t>(i)) : fill;
  __syncthreads();  // (one block: its own stores are ordered for it by the barrier)
  for (int j = threadIdx.x; j < n_pairs; j += 1024) {
    const double key = keys[j];
    const int16_t as_t = static_cast<int16_t>(key >= -32768.0 && key <= 32767.0 ? key : 0.0);
    if (static_cast<double>(as_t) == key) table[static_cast<uint16_t>(as_t)] = static_cast<int16_t>(values[j]);
  }
}

__global__ __launch_bounds__(256) void remap_table_kernel(const int16_t* x, int16_t* y, int64_t n, const int16_t* __restrict__ table) {
  stream_map<int16_t>(x, y, n, [&](int16_t v) { return table[static_cast<uint16_t>(v)]; });
}

// every other dtype: binary search in the ascending keys, from LDS when they fit
template <int DT, bool IN_LDS>
__global__ __launch_bounds__(256) void remap_search_kernel(const typename Lab<DT>::T* x, typename Lab<DT>::T* y, int64_t n,
                                                           const double* __restrict__ keys, const double* __restrict__ values, int n_pairs,
                                                           int keep, double constant) {
  using T = typename Lab<DT>::T;
  const T fill = Lab<DT>::from_double(constant);
  if constexpr (IN_LDS) {
    __shared__ double lds_keys[kRemapLdsPairs];
    __shared__ double lds_values[kRemapLdsPairs];
    for (int j = threadIdx.x; j < n_pairs; j += 256) {
      lds_keys[j] = keys[j];
      lds_values[j] = values[j];
    }
    __syncthreads();
    stream_map<T>(x, y, n, [&](T v) {
      const int j = find_key(lds_keys, n_pairs, Lab<DT>::to_double(v));
      return j >= 0 ? Lab<DT>::from_double(lds_values[j]) : (keep ? v : fill);
    });
  } else {
    stream_map<T>(x, y, n, [&](T v) {
      const int j = find_key(keys, n_pairs, Lab<DT>::to_double(v));
      return j >= 0 ? Lab<DT>::from_double(values[j]) : (keep ? v : fill);
    });
  }
}

unsigned stream_blocks(int64_t n, int element_size) {
  int64_t blocks = (n / (16 / element_size) + 255) / 256;
  return static_cast<unsigned>(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
}

// ---- one-hot --------------------------------------------------------------------------------------------------------
// One thread per group of four voxels of one batch element: four input elements, then one 16-byte store per class.
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void one_hot_kernel(const typename Lab<DT>::T* __restrict__ x, float* __restrict__ y, int batch,
                                                      int64_t n_spatial, int num_classes, int* __restrict__ status) {
  using T = typename Lab<DT>::T;
  const int64_t groups = (n_spatial + 3) / 4, total = groups * batch;
  bool bad = false;
  for (int64_t g = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; g < total; g += static_cast<int64_t>(gridDim.x) * 256) {
    const int64_t b = g / groups, s = (g - b * groups) * 4;
    const int count = n_spatial - s < 4 ? static_cast<int>(n_spatial - s) : 4;
    const T* src = x + b * n_spatial + s;
    T e[4] = {};
    if (VEC) __builtin_memcpy(e, __builtin_assume_aligned(src, 4 * sizeof(T)), 4 * sizeof(T));  // (VEC: n_spatial % 4 == 0)
    else
      for (int j = 0; j < count; j++) e[j] = src[j];
    int cls[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const double d = Lab<DT>::to_double(e[j]);
      const bool ok = d >= 0.0 && d < static_cast<double>(num_classes) && d == floor(d);
      cls[j] = ok ? static_cast<int>(d) : -1;
      bad |= !ok && j < count;
    }
    float* dst = y + b * num_classes * n_spatial + s;
    for (int c = 0; c < num_classes; c++, dst += n_spatial) {
      const float4 out = make_float4(cls[0] == c ? 1.0f : 0.0f, cls[1] == c ? 1.0f : 0.0f, cls[2] == c ? 1.0f : 0.0f, cls[3] == c ? 1.0f : 0.0f);
      if (VEC) *reinterpret_cast<float4*>(dst) = out;
      else {
        const float o[4] = {out.x, out.y, out.z, out.w};
        for (int j = 0; j < count; j++) dst[j] = o[j];
      }
    }
  }
  if (bad) atomicOr(status, 1);
}

// ---- contour --------------------------------------------------------------------------------------------------------
// A block owns an 8 x 64 (J x K) column of one volume and marches along I.  Per plane: the tile and its one-voxel halo
// (-1 outside the volume) go to LDS as float32, every thread takes the 3 x 3 minimum around its voxel, and the minimum of
// three consecutive planes' 3 x 3 minima is the 27-point minimum of the middle one.
constexpr int kContourTJ = 8, kContourTK = 64;

template <int DT>
__global__ __launch_bounds__(kContourTJ * kContourTK) void contour_kernel(const void* __restrict__ x, float* __restrict__ y, int ni, int nj, int nk,
                                                                          int tiles_j, int tiles_k) {
  constexpr int TJ = kContourTJ, TK = kContourTK, HJ = TJ + 2, HK = TK + 2;
  __shared__ float tile[2][HJ][HK + 1];
  int block = blockIdx.x;
  const int tk = block % tiles_k;
  block /= tiles_k;
  const int tj = block % tiles_j;
  const int64_t volume = block / tiles_j;
  const int tx = threadIdx.x % TK, ty = threadIdx.x / TK;
  const int j = tj * TJ + ty, k = tk * TK + tx;
  const bool inside = j < nj && k < nk;
  const int64_t plane = static_cast<int64_t>(nj) * nk, base = volume * ni * plane;
  float min_before = -1.0f, min_here = -1.0f, centre_here = 0.0f;  // planes i - 2 and i - 1 (plane -1 lies outside: -1)
  for (int i = 0; i <= ni; i++) {
    float min_next = -1.0f, centre_next = 0.0f;  // plane i (plane ni lies outside)
    if (i < ni) {
      float(*t)[HK + 1] = tile[i & 1];
      for (int cell = threadIdx.x; cell < HJ * HK; cell += TJ * TK) {
        const int r = cell / HK, c = cell % HK, jj = tj * TJ + r - 1, kk = tk * TK + c - 1;
        const bool in_volume = jj >= 0 && jj < nj && kk >= 0 && kk < nk;
        t[r][c] = in_volume ? Elem<DT>::load(x, base + i * plane + static_cast<int64_t>(jj) * nk + kk) : -1.0f;
      }
      __syncthreads();  // (the other buffer was last read before the previous iteration's barrier)
      float rows[3];
#pragma unroll
      for (int r = 0; r < 3; r++) rows[r] = fminf(fminf(t[ty + r][tx], t[ty + r][tx + 1]), t[ty + r][tx + 2]);
      min_next = fminf(fminf(rows[0], rows[1]), rows[2]);
      centre_next = t[ty + 1][tx + 1];
    }
    if (i >= 1 && inside) {
      const float eroded = fminf(fminf(min_before, min_here), min_next);
      y[base + (i - 1) * plane + static_cast<int64_t>(j) * nk + k] = eroded != centre_here ? 1.0f : 0.0f;
    }
    min_before = min_here;
    min_here = min_next;
    centre_here = centre_next;
  }
}

// ---- connected components -------------------------------------------------------------------------------------------
// Union-find over voxel indices (int32), every listed label at once: only neighbours of EQUAL value are united, so the
// components of different labels never meet.  parent[v] = -1 for a voxel whose value is not listed.  The root of a
// component is its smallest voxel index (a union hangs the larger root under the smaller), i.e. its first voxel in C order.
//   init:    a wave owns 64 consecutive voxels of a K-row; parent = the first voxel of the voxel's run of equal values
//            inside those 64 (a ballot), so the runs are components before the first union;
//   merge:   unions with the previous 64-voxel piece of the row and with the rows (j-1), (i-1, j-1 .. j+1) — only where the
//            voxel in front of it in its row has not made the same connection already;
//   flatten: the first voxel of every run finds its root and hands it to the run; it adds the run's length to size[root];
//   pick:    every root offers (size << 32 | ~root) to its (batch element, label) slot: a 64-bit atomicMax;
//   write:   a listed voxel whose root is not its slot's winner becomes the background.
constexpr int kMaxComponentLabels = 1024;

__device__ __forceinline__ int load_parent(int* parent, int v) {
  // other blocks change parents in this launch: an agent-scope load (served by L2, never by this CU's L1)
  return __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int find_root(int* parent, int v) {
  int p = load_parent(parent, v);
  while (p != v) {
    v = p;
    p = load_parent(parent, v);
  }
  return v;
}

__device__ __forceinline__ void unite(int* parent, int a, int b) {
  for (;;) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + a, b);  // a was a root when it was read; if it still is, it now hangs under b
    if (old == a) return;
    a = old;  // somebody hung a elsewhere meanwhile: unite that place with b
  }
}

struct WaveItem {
  int64_t row;
  int k;
  bool active;
};

// 64-voxel pieces of K-rows, one per wave and step
__device__ __forceinline__ WaveItem wave_item(int64_t w, int segments, int nk) {
  WaveItem it;
  it.row = w / segments;
  it.k = static_cast<int>(w - it.row * segments) * 64 + static_cast<int>(threadIdx.x & 63);
  it.active = it.k < nk;
  return it;
}

// the lane that starts this lane's run, from the ballot of run starts (lane 0 always starts one)
__device__ __forceinline__ int run_start_lane(unsigned long long starts, int lane) {
  const unsigned long long upto = starts & (~0ull >> (63 - lane));
  return upto != 0ull ? 63 - __clzll(static_cast<long long>(upto)) : lane;
}

template <int DT>
__global__ __launch_bounds__(256) void components_init_kernel(const typename Lab<DT>::T* __restrict__ x, int64_t rows, int nk,
                                                              const double* __restrict__ labels, int n_labels, int* __restrict__ parent,
                                                              unsigned* __restrict__ size) {
  using T = typename Lab<DT>::T;
  __shared__ double lds_labels[kMaxComponentLabels];
  for (int j = threadIdx.x; j < n_labels; j += 256) lds_labels[j] = labels[j];
  __syncthreads();
  const int lane = threadIdx.x & 63, segments = (nk + 63) / 64;
  const int64_t items = rows * segments;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); w < items; w += static_cast<int64_t>(gridDim.x) * 4) {
    const WaveItem it = wave_item(w, segments, nk);
    const int64_t v = it.row * nk + it.k;
    const T here = it.active ? x[v] : T{};
    const bool start = it.active && (lane == 0 || x[v - 1] != here);
    const int first = run_start_lane(__ballot(start), lane);
    int listed = start ? (find_key(lds_labels, n_labels, Lab<DT>::to_double(here)) >= 0 ? 1 : 0) : 0;
    listed = __shfl(listed, first);
    if (it.active) {
      parent[v] = listed ? static_cast<int>(v) - (lane - first) : -1;
      size[v] = 0u;
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void components_merge_kernel(const typename Lab<DT>::T* __restrict__ x, int64_t rows, int ni, int nj, int nk,
                                                               int fully_connected, int* parent) {
  using T = typename Lab<DT>::T;
  const int lane = threadIdx.x & 63, segments = (nk + 63) / 64;
  const int64_t items = rows * segments;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); w < items; w += static_cast<int64_t>(gridDim.x) * 4) {
    const WaveItem it = wave_item(w, segments, nk);
    if (!it.active) continue;
    const int v = static_cast<int>(it.row * nk + it.k);
    if (parent[v] < 0) continue;  // (written by the launch before; the sign never changes)
    const int k = it.k, j = static_cast<int>(it.row % nj), i = static_cast<int>((it.row / nj) % ni);
    const T here = x[v];
    const bool joined = k > 0 && x[v - 1] == here;  // the voxel in front belongs to this voxel's run
    if (joined && lane == 0) unite(parent, v, v - 1);  // the run continues from the previous 64-voxel piece
    // rows in front of this one in C order: (i, j - 1), then (i - 1, j - 1 .. j + 1)
    for (int n = 0; n < 4; n++) {
      const int di = n == 0 ? 0 : -1, dj = n == 0 ? -1 : n - 2;
      if (!fully_connected && n != 0 && n != 2) continue;
      if (i + di < 0 || j + dj < 0 || j + dj >= nj) continue;
      const int at = v + (di * nj + dj) * nk;
      const bool left = k > 0 && x[at - 1] == here, mid = x[at] == here, right = k < nk - 1 && x[at + 1] == here;
      if (mid) {
        // with `joined && left` the voxel in front has united its own `mid`, and both runs carry the union over
        if (!(joined && left)) unite(parent, v, at);
      } else if (fully_connected) {
        if (left && !joined) unite(parent, v, at - 1);  // (joined: `left` is the `mid` of the voxel in front)
        if (right) unite(parent, v, at + 1);
      }
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void components_flatten_kernel(const typename Lab<DT>::T* __restrict__ x, int64_t rows, int nk, int* parent,
                                                                 unsigned* __restrict__ size) {
  using T = typename Lab<DT>::T;
  const int lane = threadIdx.x & 63, segments = (nk + 63) / 64;
  const int64_t items = rows * segments;
  for (int64_t w = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6); w < items; w += static_cast<int64_t>(gridDim.x) * 4) {
    const WaveItem it = wave_item(w, segments, nk);
    const int64_t v = it.row * nk + it.k;
    const T here = it.active ? x[v] : T{};
    const bool start = it.active && (lane == 0 || x[v - 1] != here);
    const unsigned long long starts = __ballot(start);
    const int first = run_start_lane(starts, lane);
    const bool listed = it.active && parent[v] >= 0;
    // (parents written in this launch are roots, read ones are ancestors: whichever a walk meets, it ends at the root)
    int root = -1;
    if (start && listed) root = find_root(parent, static_cast<int>(v));
    root = __shfl(root, first);
    if (!listed) continue;
    parent[v] = root;
    if (start) {
      const int valid = nk - (it.k - lane) < 64 ? nk - (it.k - lane) : 64;
      const unsigned long long behind = lane < 63 ? starts >> (lane + 1) : 0ull;
      const int next = behind != 0ull ? lane + 1 + __ffsll(static_cast<long long>(behind)) - 1 : valid;
      atomicAdd(size + root, static_cast<unsigned>(next - lane));
    }
  }
}

template <int DT>
__global__ __launch_bounds__(256) void components_pick_kernel(const typename Lab<DT>::T* __restrict__ x, int n, int per_element,
                                                              const double* __restrict__ labels, int n_labels, const int* __restrict__ parent,
                                                              const unsigned* __restrict__ size, unsigned long long* __restrict__ best) {
  for (int64_t at = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; at < n; at += static_cast<int64_t>(gridDim.x) * 256) {
    const int v = static_cast<int>(at);  // (the stride is counted in 64 bits: n may lie within one stride of 2^31)
    if (parent[v] != v) continue;
    const int label = find_key(labels, n_labels, Lab<DT>::to_double(x[v]));
    if (label < 0) continue;  // (cannot happen: a root is a listed voxel)
    const unsigned long long offer = (static_cast<unsigned long long>(size[v]) << 32) | static_cast<unsigned>(~static_cast<unsigned>(v));
    atomicMax(best + static_cast<int64_t>(v / per_element) * n_labels + label, offer);
  }
}

template <int DT>
__global__ __launch_bounds__(256) void components_write_kernel(const typename Lab<DT>::T* __restrict__ x, typename Lab<DT>::T* __restrict__ y, int n,
                                                               int per_element, const double* __restrict__ labels, int n_labels,
                                                               const int* __restrict__ parent, const unsigned long long* __restrict__ best,
                                                               double background) {
  using T = typename Lab<DT>::T;
  __shared__ double lds_labels[kMaxComponentLabels];
  for (int j = threadIdx.x; j < n_labels; j += 256) lds_labels[j] = labels[j];
  __syncthreads();
  const T fill = Lab<DT>::from_double(background);
  for (int64_t at = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; at < n; at += static_cast<int64_t>(gridDim.x) * 256) {
    const int v = static_cast<int>(at);
    T out = x[v];
    const int root = parent[v];
    if (root >= 0) {
      const int label = find_key(lds_labels, n_labels, Lab<DT>::to_double(out));
      const unsigned long long winner = best[static_cast<int64_t>(v / per_element) * n_labels + (label < 0 ? 0 : label)];
      if (static_cast<unsigned>(root) != ~static_cast<unsigned>(winner)) out = fill;
    }
    y[v] = out;
  }
}

int64_t components_best_offset(int64_t n) { return (8 * n + 15) / 16 * 16; }

template <int DT>
int launch_components(const void* x_, void* y_, int batch, const int32_t shape[3], const double* labels, int n_labels, double background,
                      int fully_connected, void* workspace, hipStream_t s) {
  using T = typename Lab<DT>::T;
  const T* x = static_cast<const T*>(x_);
  T* y = static_cast<T*>(y_);
  const int64_t per_element = static_cast<int64_t>(shape[0]) * shape[1] * shape[2], n = per_element * batch;
  const int64_t rows = static_cast<int64_t>(batch) * shape[0] * shape[1], items = rows * ((shape[2] + 63) / 64);
  int* parent = static_cast<int*>(workspace);
  unsigned* size = reinterpret_cast<unsigned*>(parent + n);
  unsigned long long* best = reinterpret_cast<unsigned long long*>(static_cast<char*>(workspace) + components_best_offset(n));
  if (hipMemsetAsync(best, 0, sizeof(unsigned long long) * batch * n_labels, s) != hipSuccess)
    return fail(TIO_ERR_LAUNCH, "tio_keep_largest_component: memset failed");
  const dim3 wave_grid(static_cast<unsigned>(items / 4 + 1 > 4096 ? 4096 : items / 4 + 1));
  const dim3 voxel_grid(static_cast<unsigned>(n / 256 + 1 > 8192 ? 8192 : n / 256 + 1));
  hipLaunchKernelGGL(components_init_kernel<DT>, wave_grid, dim3(256), 0, s, x, rows, shape[2], labels, n_labels, parent, size);
  if (const int rc = check_launch("tio_keep_largest_component (init)")) return rc;
  hipLaunchKernelGGL(components_merge_kernel<DT>, wave_grid, dim3(256), 0, s, x, rows, shape[0], shape[1], shape[2], fully_connected, parent);
  if (const int rc = check_launch("tio_keep_largest_component (merge)")) return rc;
  hipLaunchKernelGGL(components_flatten_kernel<DT>, wave_grid, dim3(256), 0, s, x, rows, shape[2], parent, size);
  if (const int rc = check_launch("tio_keep_largest_component (flatten)")) return rc;
  hipLaunchKernelGGL(components_pick_kernel<DT>, voxel_grid, dim3(256), 0, s, x, static_cast<int>(n), static_cast<int>(per_element), labels, n_labels,
                     parent, size, best);
  if (const int rc = check_launch("tio_keep_largest_component (pick)")) return rc;
  hipLaunchKernelGGL(components_write_kernel<DT>, voxel_grid, dim3(256), 0, s, x, y, static_cast<int>(n), static_cast<int>(per_element), labels,
                     n_labels, parent, best, background);
  return check_launch("tio_keep_largest_component (write)");
}

}  // namespace
}  // namespace tio

extern "C" int tio_label_remap(const void* x, void* y, int32_t dtype, int64_t n, const double* keys_dev, const double* values_dev, int32_t n_pairs,
                               int32_t mode, double constant, void* table_dev, void* stream) {
  using namespace tio;
  const int es = dtype_size(dtype);
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_label_remap: unknown dtype %d", dtype);
  if (n < 0 || n_pairs < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_remap: negative size");
  if (n_pairs > TIO_REMAP_MAX_PAIRS) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_remap: n_pairs %d beyond %d", n_pairs, TIO_REMAP_MAX_PAIRS);
  if (mode != TIO_REMAP_KEEP && mode != TIO_REMAP_CONSTANT) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_remap: unknown mode %d", mode);
  if (n == 0) return TIO_OK;
  if (x == nullptr || y == nullptr || (n_pairs > 0 && (keys_dev == nullptr || values_dev == nullptr)) || (dtype == TIO_I16 && table_dev == nullptr))
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_remap: null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(stream_blocks(n, es)), block(256);
  const int keep = mode == TIO_REMAP_KEEP;
  if (dtype == TIO_I16) {
    int16_t* table = static_cast<int16_t*>(table_dev);
    hipLaunchKernelGGL(remap_build_table_kernel, dim3(1), dim3(1024), 0, s, table, keys_dev, values_dev, n_pairs, keep, constant);
    if (const int rc = check_launch("tio_label_remap (table)")) return rc;
    hipLaunchKernelGGL(remap_table_kernel, grid, block, 0, s, static_cast<const int16_t*>(x), static_cast<int16_t*>(y), n, table);
    return check_launch("tio_label_remap");
  }
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    using T = typename Lab<DT>::T;
    auto kernel = n_pairs <= kRemapLdsPairs ? remap_search_kernel<DT, true> : remap_search_kernel<DT, false>;
    if constexpr (DT == TIO_U8 || DT == TIO_I8) kernel = remap_byte_kernel<DT>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, static_cast<const T*>(x), static_cast<T*>(y), n, keys_dev, values_dev, n_pairs, keep, constant);
  });
  return known ? check_launch("tio_label_remap") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_label_remap: unknown dtype %d", dtype);
}

extern "C" int tio_label_one_hot(const void* x, float* y, int32_t dtype, int32_t batch, int64_t n_spatial, int32_t num_classes, int32_t* status_dev,
                                 void* stream) {
  using namespace tio;
  const int es = dtype_size(dtype);
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_label_one_hot: unknown dtype %d", dtype);
  if (batch < 0 || n_spatial < 0 || num_classes < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_one_hot: negative size");
  if (status_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_one_hot: null status word");
  const bool empty = batch == 0 || n_spatial == 0;
  if (!empty && (x == nullptr || (num_classes > 0 && y == nullptr))) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_one_hot: null argument");
  if (empty) return TIO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status_dev, 0, sizeof(int32_t), s) != hipSuccess) return fail(TIO_ERR_LAUNCH, "tio_label_one_hot: memset failed");
  const int64_t groups = (n_spatial + 3) / 4 * batch;
  const dim3 grid(static_cast<unsigned>((groups + 255) / 256 > 4096 ? 4096 : (groups + 255) / 256)), block(256);
  const bool vec = n_spatial % 4 == 0 && reinterpret_cast<uintptr_t>(x) % (4 * es) == 0 && reinterpret_cast<uintptr_t>(y) % 16 == 0;
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const auto kernel = vec ? one_hot_kernel<DT, true> : one_hot_kernel<DT, false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, static_cast<const typename Lab<DT>::T*>(x), y, batch, n_spatial, num_classes, status_dev);
  });
  return known ? check_launch("tio_label_one_hot") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_label_one_hot: unknown dtype %d", dtype);
}

extern "C" int tio_label_contour(const void* x, float* y, int32_t dtype, int64_t n_batch_channels, const int32_t shape[3], void* stream) {
  using namespace tio;
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_label_contour: unknown dtype %d", dtype);
  if (shape == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_contour: null shape");
  if (n_batch_channels < 0 || shape[0] < 0 || shape[1] < 0 || shape[2] < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_contour: negative size");
  if (n_batch_channels == 0 || shape[0] == 0 || shape[1] == 0 || shape[2] == 0) return TIO_OK;
  if (x == nullptr || y == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_label_contour: null argument");
  const int tiles_j = (shape[1] + kContourTJ - 1) / kContourTJ, tiles_k = (shape[2] + kContourTK - 1) / kContourTK;
  const int64_t blocks = n_batch_channels * tiles_j * tiles_k;
  if (blocks >= (int64_t{1} << 31)) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "tio_label_contour: too many tiles");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(blocks)), block(kContourTJ * kContourTK);
  const bool known = dispatch_dtype(dtype, [&](auto dt) {
    hipLaunchKernelGGL(contour_kernel<decltype(dt)::value>, grid, block, 0, s, x, y, shape[0], shape[1], shape[2], tiles_j, tiles_k);
  });
  return known ? check_launch("tio_label_contour") : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_label_contour: unknown dtype %d", dtype);
}

extern "C" int64_t tio_keep_largest_workspace_bytes(int32_t batch, const int32_t shape[3], int32_t n_labels) {
  using namespace tio;
  if (shape == nullptr || batch < 0 || n_labels < 0 || shape[0] < 0 || shape[1] < 0 || shape[2] < 0) {
    set_error("tio_keep_largest_workspace_bytes: null or negative argument");
    return TIO_ERR_INVALID_ARGUMENT;
  }
  const int64_t n = static_cast<int64_t>(batch) * shape[0] * shape[1] * shape[2];
  return components_best_offset(n) + 8 * static_cast<int64_t>(batch) * n_labels + 16;
}

extern "C" int tio_keep_largest_component(const void* x, void* y, int32_t dtype, int32_t batch, const int32_t shape[3], const double* labels_dev,
                                          int32_t n_labels, double background, int32_t fully_connected, void* workspace_dev,
                                          int64_t workspace_bytes, void* stream) {
  using namespace tio;
  if (dtype != TIO_U8 && dtype != TIO_I8 && dtype != TIO_I16 && dtype != TIO_I32 && dtype != TIO_I64 && dtype != TIO_F32)
    return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_keep_largest_component: integer and float32 label maps only (dtype %d)", dtype);
  if (shape == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_keep_largest_component: null shape");
  if (batch < 0 || n_labels < 0 || shape[0] < 0 || shape[1] < 0 || shape[2] < 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_keep_largest_component: negative size");
  const int64_t n = static_cast<int64_t>(batch) * shape[0] * shape[1] * shape[2];
  if (n >= (int64_t{1} << 31)) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "tio_keep_largest_component: %lld voxels do not fit 32-bit indices", static_cast<long long>(n));
  if (n_labels > TIO_KEEP_LARGEST_MAX_LABELS)
    return fail(TIO_ERR_UNSUPPORTED_CONFIG, "tio_keep_largest_component: %d labels beyond %d per call", n_labels, TIO_KEEP_LARGEST_MAX_LABELS);
  if (n == 0) return TIO_OK;
  if (x == nullptr || y == nullptr || (n_labels > 0 && (labels_dev == nullptr || workspace_dev == nullptr)))
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_keep_largest_component: null argument");
  if (x == y) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_keep_largest_component: the output must not alias the input");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_labels == 0) {
    if (hipMemcpyAsync(y, x, n * dtype_size(dtype), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail(TIO_ERR_LAUNCH, "tio_keep_largest_component: copy failed");
    return TIO_OK;
  }
  if (reinterpret_cast<uintptr_t>(workspace_dev) % 16 != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_keep_largest_component: the workspace must be 16-byte aligned");
  if (workspace_bytes < tio_keep_largest_workspace_bytes(batch, shape, n_labels))
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_keep_largest_component: workspace of %lld bytes is too small", static_cast<long long>(workspace_bytes));
  switch (dtype) {
    case TIO_U8: return launch_components<TIO_U8>(x, y, batch, shape, labels_dev, n_labels, background, fully_connected, workspace_dev, s);
    case TIO_I8: return launch_components<TIO_I8>(x, y, batch, shape, labels_dev, n_labels, background, fully_connected, workspace_dev, s);
    case TIO_I16: return launch_components<TIO_I16>(x, y, batch, shape, labels_dev, n_labels, background, fully_connected, workspace_dev, s);
    case TIO_I32: return launch_components<TIO_I32>(x, y, batch, shape, labels_dev, n_labels, background, fully_connected, workspace_dev, s);
    case TIO_I64: return launch_components<TIO_I64>(x, y, batch, shape, labels_dev, n_labels, background, fully_connected, workspace_dev, s);
    default: return launch_components<TIO_F32>(x, y, batch, shape, labels_dev, n_labels, background, fully_connected, workspace_dev, s);
  }
}
