// kspace_artefacts.hip — Ghosting and Spike without a k-space round trip.
//
// Reference: transforms/intensity/ghosting.py (_add_ghosting :218-277, _add_ghosting_per_element :149-215) and
// transforms/intensity/spike.py (_add_spikes :124-162, _add_spikes_per_instance :165-223).  Both take fftn, fftshift, edit a
// few entries of the spectrum, shift back, ifftn and keep the real part.  The edits are so sparse that both are small REAL
// operators in image space (as Motion's compositing is, kspace.hip):
//
// Ghosting scales the k-space planes Z along ONE axis (length S) by 1 - strength.  The other two axes' transforms cancel,
// and with theta_f = 2 pi f / S every line along the axis becomes
//
//     out[i] = x[i] - (strength / S) * sum_{f in Z} ( cos(theta_f i) A_f + sin(theta_f i) B_f ),
//     A_f = sum_i' cos(theta_f i') x[i'],   B_f = sum_i' sin(theta_f i') x[i']
//
// — one reduction along the line and one update, a rank-2|Z| correction.
//
// Spike adds peak * intensity to a few k-space points (f_p0, f_p1, f_p2):
//
//     out[i, j, k] = x[i, j, k] + (peak * intensity / (I J K)) * sum_p cos 2 pi (f_p0 i / I + f_p1 j / J + f_p2 k / K)
//
// — one element-wise pass; only `peak = max |fftn(x)|` needs a spectrum (tio_complex_abs_max over the caller's rfftn).
//
// Every cosine and sine comes from a per-axis table E_S[r] = (cos, sin)(2 pi r / S), r = 0 .. S-1, evaluated in double on the
// host and rounded once to float32; the index f * i mod S is reduced in integers and stepped by addition, so no angle is ever
// formed in float32 and no transcendental runs on the device.  Spike's three-axis cosine is the real part of a product of
// three table entries.
#include <math.h>

#include <mutex>

#include "common.hpp"

namespace tio {
namespace {

constexpr int kThreads = 256;
constexpr int kFC = 8;                  // frequencies per chunk of the ghost kernel: 2 * kFC running sums per thread
constexpr int kMaxLines = 32;           // lines per tile, at most
constexpr int kLdsBudget = 156 * 1024;  // of the CU's 160 KiB, for one block
constexpr int kMaxAxis = 32768;         // f * i stays below 2^30

// ---------------------------------------------------------------------------------------------------------------------
// Ghosting.  The volume is (P, S, Q) around the axis: axis 0 -> (1, I, J K), axis 1 -> (I, J, K), axis 2 -> (I J, K, 1).  A
// block owns a tile of TL lines that are neighbours in memory — TL consecutive q of one p (Q > 1: every row s of the tile
// is a contiguous run of TL elements), or TL consecutive p (Q == 1: the whole tile is one contiguous run) — so no axis is
// ever transposed through HBM.  Thread (l, g) = (tid % TL, tid / TL) works on line l at s = g, g + G, ...  (G = 256 / TL):
//
//   sweep in    the tile -> LDS as float32 [s][TL + 1] (RESIDENT; the padding keeps both the row-wise sweep and the
//               line-wise loops conflict-free), in memory order
//   per chunk of kFC frequencies:
//     reduce    2 kFC running sums over the thread's s; lanes of one line folded by xor-shuffles, the four waves through LDS
//     update    corr[s] = sum_f cos * A_f + sin * B_f, added to the accumulator tile (only when there is more than one chunk)
//   sweep out   x - (strength / S) * corr, converted to the dtype, in memory order again (the last update leaves it in LDS)
//
// Beyond what LDS holds the input stays in memory (RESIDENT = false: the loops read it again, through L2) and only the
// accumulator tile is kept; the host then also narrows the tile (TL = 8, then 1) until that one fits.
struct GhostArgs {
  const void* x;
  void* y;
  const int32_t* params;  // [batch][4] = {axis, count, offset, strength bits}, then the frequencies
  const float2* table;    // E_S of this launch's axis
  const uint8_t* active;  // [batch] or null
  int64_t n_spatial;
  int32_t params_words, batch, channels, dtype, axis, max_count;
  int32_t P, S, Q;
  int32_t tl_shift, tiles_q;
};

__device__ __forceinline__ void copy_element(const void* x, void* y, int bytes, int64_t at) {
  switch (bytes) {
    case 1: static_cast<uint8_t*>(y)[at] = static_cast<const uint8_t*>(x)[at]; break;
    case 2: static_cast<uint16_t*>(y)[at] = static_cast<const uint16_t*>(x)[at]; break;
    case 4: static_cast<uint32_t*>(y)[at] = static_cast<const uint32_t*>(x)[at]; break;
    default: static_cast<uint64_t*>(y)[at] = static_cast<const uint64_t*>(x)[at]; break;
  }
}

template <bool RESIDENT>
__global__ __launch_bounds__(kThreads) void ghost_lines_kernel(GhostArgs a) {
  extern __shared__ __align__(16) float lds[];
  const int tid = threadIdx.x;
  const int bc = blockIdx.y, b = bc / a.channels;
  // ---- this element's record (block-uniform) ----
  const int32_t* head = a.params + 4 * static_cast<int64_t>(b);
  if (head[0] != a.axis) return;  // another launch's element
  int count = head[1];
  const int offset = head[2];
  const float strength = __int_as_float(head[3]);
  count = count < a.max_count ? count : a.max_count;
  const bool listed = count > 0 && offset >= 4 * a.batch && static_cast<int64_t>(offset) + count <= a.params_words;
  const bool plain = !listed || strength == 0.0f || (a.active != nullptr && a.active[b] == 0);

  // ---- the tile ----
  const int S = a.S, TL = 1 << a.tl_shift, pitch = TL + 1, G = kThreads >> a.tl_shift;
  const int l = tid & (TL - 1), g = tid >> a.tl_shift;
  int lines_here;
  int64_t base, lstride;
  if (a.Q == 1) {
    const int64_t p0 = static_cast<int64_t>(blockIdx.x) * TL;
    lines_here = static_cast<int>(a.P - p0 < TL ? a.P - p0 : TL);
    base = p0 * S;
    lstride = S;
  } else {
    const int p = blockIdx.x / a.tiles_q, q0 = (blockIdx.x - p * a.tiles_q) * TL;
    lines_here = a.Q - q0 < TL ? a.Q - q0 : TL;
    base = static_cast<int64_t>(p) * S * a.Q + q0;
    lstride = 1;
  }
  base += static_cast<int64_t>(bc) * a.n_spatial;
  const int64_t sstride = a.Q;
  // every element of the tile once, neighbours in memory on neighbouring lanes: fn(line, s, element index)
  auto sweep = [&](auto&& fn) {
    if (a.Q == 1) {
      for (int ll = 0; ll < lines_here; ll++)
        for (int s = tid; s < S; s += kThreads) fn(ll, s, base + static_cast<int64_t>(ll) * S + s);
    } else {
      const int n = S << a.tl_shift;
      for (int idx = tid; idx < n; idx += kThreads) {
        const int ll = idx & (TL - 1), s = idx >> a.tl_shift;
        if (ll < lines_here) fn(ll, s, base + static_cast<int64_t>(s) * sstride + ll);
      }
    }
  };
  if (plain) {  // an exact copy, whatever the dtype
    const int bytes = dtype_size(a.dtype);
    sweep([&](int, int, int64_t at) { copy_element(a.x, a.y, bytes, at); });
    return;
  }

  // ---- LDS: table | wave sums | line sums | input tile (RESIDENT) | accumulator tile (acc_tile) ----
  float2* tab = reinterpret_cast<float2*>(lds);
  float* red = lds + 2 * ((S + 1) & ~1);                // [2 kFC][4 waves][TL]
  float* coef = red + 2 * kFC * 4 * kMaxLines;           // [2 kFC][kMaxLines]
  float* xt = coef + 2 * kFC * kMaxLines;                // [S][pitch]
  float* acc = RESIDENT ? xt + S * pitch : xt;           // [S][pitch]
  float* final_tile = RESIDENT ? xt : acc;               // where the last update leaves the result
  for (int r = tid; r < S; r += kThreads) tab[r] = a.table[r];
  if constexpr (RESIDENT) sweep([&](int ll, int s, int64_t at) { xt[s * pitch + ll] = load_as_float(a.x, a.dtype, at); });
  __syncthreads();
  const bool line_ok = l < lines_here;
  auto value = [&](int s) -> float {
    if (!line_ok) return 0.0f;
    if constexpr (RESIDENT) return xt[s * pitch + l];
    else return load_as_float(a.x, a.dtype, base + static_cast<int64_t>(l) * lstride + static_cast<int64_t>(s) * sstride);
  };

  const float scale = strength / static_cast<float>(S);
  const int lane = tid & 63, wave = tid >> 6;
  const int n_chunks = (count + kFC - 1) / kFC;
  for (int c = 0; c < n_chunks; c++) {
    int start[kFC], step[kFC];
    float weight[kFC];
#pragma unroll
    for (int j = 0; j < kFC; j++) {
      const int at = c * kFC + j;
      const int f = at < count ? a.params[offset + at] : -1;
      const bool ok = f >= 0 && f < S;  // (anything else contributes nothing)
      weight[j] = ok ? 1.0f : 0.0f;
      start[j] = ok ? (f * g) % S : 0;  // f * s mod S at the thread's first s, then stepped by f * G mod S
      step[j] = ok ? (f * G) % S : 0;
    }
    // reduce
    float A[kFC], B[kFC];
    int r[kFC];
#pragma unroll
    for (int j = 0; j < kFC; j++) A[j] = 0.0f, B[j] = 0.0f, r[j] = start[j];
    for (int s = g; s < S; s += G) {
      const float v = value(s);
#pragma unroll
      for (int j = 0; j < kFC; j++) {
        const float2 e = tab[r[j]];
        A[j] = __builtin_fmaf(e.x, v, A[j]);
        B[j] = __builtin_fmaf(e.y, v, B[j]);
        r[j] += step[j];
        r[j] -= r[j] >= S ? S : 0;
      }
    }
    // lanes l, l + TL, l + 2 TL, ... of a wave hold the same line
#pragma unroll
    for (int j = 0; j < kFC; j++)
      for (int m = 32; m >= TL; m >>= 1) {
        A[j] += __shfl_xor(A[j], m);
        B[j] += __shfl_xor(B[j], m);
      }
    if (lane < TL) {
#pragma unroll
      for (int j = 0; j < kFC; j++) {
        red[((2 * j) * 4 + wave) * TL + lane] = A[j];
        red[((2 * j + 1) * 4 + wave) * TL + lane] = B[j];
      }
    }
    __syncthreads();
    for (int u = tid; u < (2 * kFC) << a.tl_shift; u += kThreads) {
      const int k = u >> a.tl_shift, ll = u & (TL - 1);
      const float* from = red + k * 4 * TL + ll;
      coef[k * kMaxLines + ll] = (from[0] + from[TL]) + (from[2 * TL] + from[3 * TL]);
    }
    __syncthreads();
    // update
    float cA[kFC], cB[kFC];
#pragma unroll
    for (int j = 0; j < kFC; j++) {
      cA[j] = weight[j] * coef[(2 * j) * kMaxLines + l];
      cB[j] = weight[j] * coef[(2 * j + 1) * kMaxLines + l];
      r[j] = start[j];
    }
    const bool first = c == 0, last = c == n_chunks - 1;
    for (int s = g; s < S; s += G) {
      float corr = 0.0f;
#pragma unroll
      for (int j = 0; j < kFC; j++) {
        const float2 e = tab[r[j]];
        corr = __builtin_fmaf(e.x, cA[j], corr);
        corr = __builtin_fmaf(e.y, cB[j], corr);
        r[j] += step[j];
        r[j] -= r[j] >= S ? S : 0;
      }
      if (!first) corr += acc[s * pitch + l];
      if (last) final_tile[s * pitch + l] = value(s) - scale * corr;
      else acc[s * pitch + l] = corr;
    }
    __syncthreads();  // the sums are read; the last chunk's results are in place
  }
  sweep([&](int ll, int s, int64_t at) { store_from_float(a.y, a.dtype, at, final_tile[s * pitch + ll]); });
}

// LDS bytes of one block
int64_t ghost_lds_bytes(int S, int tl, int tiles) {
  const int64_t fixed = 2 * ((S + 1) & ~1) + 2 * kFC * 4 * kMaxLines + 2 * kFC * kMaxLines;
  return 4 * (fixed + static_cast<int64_t>(tiles) * S * (tl + 1));
}

// ---------------------------------------------------------------------------------------------------------------------
// max |z| per row of interleaved complex64: every element read once (16-byte loads of two elements where the row's start
// allows, one element in front and one behind otherwise), the squares compared and ONE square root taken per block (the
// root is monotonic), then an atomic maximum on the bits of the non-negative result.
__global__ __launch_bounds__(kThreads) void complex_abs_max_kernel(const float2* z, int64_t n, uint32_t* out) {
  __shared__ float wave_max[kThreads / 64];
  const float2* p = z + static_cast<int64_t>(blockIdx.y) * n;
  const int64_t head = (reinterpret_cast<uintptr_t>(p) % 16 != 0 && n > 0) ? 1 : 0;
  const int64_t pairs = (n - head) / 2;
  const float4* p4 = reinterpret_cast<const float4*>(p + head);
  float m = 0.0f;
  for (int64_t at = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; at < pairs; at += static_cast<int64_t>(gridDim.x) * kThreads) {
    const float4 v = p4[at];
    m = fmaxf(m, v.x * v.x + v.y * v.y);
    m = fmaxf(m, v.z * v.z + v.w * v.w);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (head != 0) m = fmaxf(m, p[0].x * p[0].x + p[0].y * p[0].y);
    if (head + 2 * pairs < n) m = fmaxf(m, p[n - 1].x * p[n - 1].x + p[n - 1].y * p[n - 1].y);
  }
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(wave_max[0], wave_max[1]), fmaxf(wave_max[2], wave_max[3]));
    atomicMax(out + blockIdx.y, __float_as_uint(sqrtf(m)));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Spike.  One pass; a thread takes 16 bytes of the volume (V elements) where x and y share their phase inside a 16-byte
// line, single elements in front, behind, and everywhere when they do not.  For each spike the thread looks up
// E_I[f0 i mod I] * E_J[f1 j mod J] once and multiplies by E_K[f2 k mod K] per element; the three indices are reduced
// once per thread and spike and stepped by addition along the run.
struct SpikeArgs {
  const void* x;
  void* y;
  const int32_t* params;  // [batch][4] = {count, offset, intensity bits, 0}, then the (f0, f1, f2) triples
  const float2* table;    // E_I, E_J, E_K one after the other
  const float* peaks;     // [batch * channels]
  const uint8_t* active;  // [batch] or null
  int32_t params_words, batch, channels, max_count;
  int32_t I, J, K, n_spatial;
};

__device__ __forceinline__ float2 cmul(float2 u, float2 v) {
  return make_float2(__builtin_fmaf(u.x, v.x, -(u.y * v.y)), __builtin_fmaf(u.x, v.y, u.y * v.x));
}

// sum_p cos(...) for `n` (<= V) consecutive elements from linear index e0 of the volume
template <int V>
__device__ __forceinline__ void spike_sums(const SpikeArgs& a, const int32_t* triples, int count, int e0, int n, float (&sum)[V]) {
  const float2 *ti = a.table, *tj = ti + a.I, *tk = tj + a.J;
  const unsigned row = static_cast<unsigned>(e0) / static_cast<unsigned>(a.K);
  const int k0 = e0 - static_cast<int>(row) * a.K;
  const int i0 = static_cast<int>(row / static_cast<unsigned>(a.J)), j0 = static_cast<int>(row) - i0 * a.J;
#pragma unroll
  for (int v = 0; v < V; v++) sum[v] = 0.0f;
  for (int p = 0; p < count; p++) {
    const int f0 = triples[3 * p], f1 = triples[3 * p + 1], f2 = triples[3 * p + 2];
    if (f0 < 0 || f0 >= a.I || f1 < 0 || f1 >= a.J || f2 < 0 || f2 >= a.K) continue;  // (uniform; contributes nothing)
    int ri = (f0 * i0) % a.I, rj = (f1 * j0) % a.J, rk = (f2 * k0) % a.K, k = k0, j = j0;
    float2 w = cmul(ti[ri], tj[rj]);
#pragma unroll
    for (int v = 0; v < V; v++) {
      if (v < n) {
        const float2 e = tk[rk];
        sum[v] += __builtin_fmaf(w.x, e.x, -(w.y * e.y));
        rk += f2;
        rk -= rk >= a.K ? a.K : 0;
        if (++k == a.K) {  // the next row (indices stay inside their tables past the volume's end, where nothing uses them)
          k = 0, rk = 0;
          rj += f1;
          rj -= rj >= a.J ? a.J : 0;
          if (++j == a.J) {
            j = 0, rj = 0;
            ri += f0;
            ri -= ri >= a.I ? a.I : 0;
          }
          w = cmul(ti[ri], tj[rj]);
        }
      }
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void add_spikes_kernel(SpikeArgs a) {
  using T = typename Elem<DT>::type;
  constexpr int V = 16 / static_cast<int>(sizeof(T));
  union Pack {
    uint4 q;
    T e[V];
  };
  const int bc = blockIdx.y, b = bc / a.channels;
  const int32_t* head = a.params + 4 * static_cast<int64_t>(b);
  int count = head[0];
  const int offset = head[1];
  const float intensity = __int_as_float(head[2]);
  count = count < a.max_count ? count : a.max_count;
  const bool listed = count > 0 && offset >= 4 * a.batch && static_cast<int64_t>(offset) + 3 * static_cast<int64_t>(count) <= a.params_words;
  const bool plain = !listed || intensity == 0.0f || (a.active != nullptr && a.active[b] == 0);
  const int n = a.n_spatial;
  const T* x = static_cast<const T*>(a.x) + static_cast<int64_t>(bc) * n;
  T* y = static_cast<T*>(a.y) + static_cast<int64_t>(bc) * n;
  const int32_t* triples = a.params + offset;
  const float amplitude = plain ? 0.0f : a.peaks[bc] * intensity / (static_cast<float>(a.I) * static_cast<float>(a.J) * static_cast<float>(a.K));

  // [0, front) single, `groups` packs of V, the rest single
  const unsigned phase_x = static_cast<unsigned>(reinterpret_cast<uintptr_t>(x) % 16), phase_y = static_cast<unsigned>(reinterpret_cast<uintptr_t>(y) % 16);
  int front = n, groups = 0;
  if (phase_x == phase_y) {
    front = static_cast<int>((16 - phase_x) % 16) / static_cast<int>(sizeof(T));
    front = front < n ? front : n;
    groups = (n - front) / V;
  }
  const int behind = front + groups * V, singles = front + (n - behind);
  const int first = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  for (int at = first; at < groups; at += stride) {
    const int e0 = front + at * V;
    Pack in, out;
    in.q = *reinterpret_cast<const uint4*>(x + e0);
    if (plain) {
      out.q = in.q;
    } else {
      float sum[V];
      spike_sums<V>(a, triples, count, e0, V, sum);
#pragma unroll
      for (int v = 0; v < V; v++) Elem<DT>::store(out.e, v, Elem<DT>::load(in.e, v) + amplitude * sum[v]);
    }
    *reinterpret_cast<uint4*>(y + e0) = out.q;
  }
  for (int at = first; at < singles; at += stride) {
    const int e0 = at < front ? at : behind + (at - front);
    if (plain) {
      y[e0] = x[e0];
    } else {
      float sum[1];
      spike_sums<1>(a, triples, count, e0, 1, sum);
      Elem<DT>::store(y, e0, Elem<DT>::load(x, e0) + amplitude * sum[0]);
    }
  }
}

// the checks the two transforms share; 0 volumes or 0 voxels: *empty
int check_volume(const char* who, const void* x, const void* y, int32_t dtype, int32_t batch, int32_t channels, const int32_t* shape,
                 bool* empty) {
  *empty = true;
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", who, dtype);
  if (shape == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null shape", who);
  if (batch < 0 || channels < 0 || shape[0] < 0 || shape[1] < 0 || shape[2] < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", who);
  for (int d = 0; d < 3; d++)
    if (shape[d] > kMaxAxis) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: axis %d has %d voxels (at most %d)", who, d, shape[d], kMaxAxis);
  const int64_t n_spatial = static_cast<int64_t>(shape[0]) * shape[1] * shape[2];
  const int64_t volumes = static_cast<int64_t>(batch) * channels;
  if (n_spatial >= (int64_t{1} << 31)) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: 2^31 voxels or more per volume", who);
  if (volumes > 65535) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 65535 volumes", who);
  if (volumes == 0 || n_spatial == 0) return TIO_OK;
  if (x == nullptr || y == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null data", who);
  const int size = dtype_size(dtype);
  const int64_t bytes = volumes * n_spatial * size;
  const uintptr_t ax = reinterpret_cast<uintptr_t>(x), ay = reinterpret_cast<uintptr_t>(y);
  if (ax < ay + bytes && ay < ax + bytes) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: the destination overlaps the source", who);
  if (ax % size != 0 || ay % size != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: data not aligned to its element", who);
  *empty = false;
  return TIO_OK;
}

}  // namespace
}  // namespace tio

extern "C" int tio_kspace_ghost_lines(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels, const int32_t shape[3],
                                      int32_t axes_mask, const int32_t* params_dev, int32_t params_words, int32_t max_count,
                                      const float* tables_dev, const uint8_t* active_dev, void* stream) {
  using namespace tio;
  const char* who = "tio_kspace_ghost_lines";
  bool empty;
  if (const int status = check_volume(who, x, y, dtype, batch, channels, shape, &empty); status != TIO_OK) return status;
  if (axes_mask < 0 || axes_mask > 7) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: axes_mask %d (bits 0 to 2)", who, axes_mask);
  if (max_count < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative max_count", who);
  if (empty) return TIO_OK;
  if (axes_mask == 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: axes_mask names no axis", who);
  if (params_dev == nullptr || tables_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null parameters or tables", who);
  if (static_cast<int64_t>(params_words) < 4 * static_cast<int64_t>(batch))
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: %d parameter words for a batch of %d (4 each, then the frequencies)", who, params_words, batch);
  if (reinterpret_cast<uintptr_t>(tables_dev) % 8 != 0 || reinterpret_cast<uintptr_t>(params_dev) % 4 != 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: parameters or tables not aligned", who);

  static std::once_flag once;
  static hipError_t raised = hipSuccess;
  std::call_once(once, [] {
    raised = hipFuncSetAttribute(reinterpret_cast<const void*>(&ghost_lines_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget);
    if (raised == hipSuccess)
      raised = hipFuncSetAttribute(reinterpret_cast<const void*>(&ghost_lines_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget);
  });
  if (raised != hipSuccess) return fail(TIO_ERR_LAUNCH, "%s: the LDS limit could not be raised", who);

  GhostArgs a{};
  a.x = x; a.y = y; a.params = params_dev; a.active = active_dev;
  a.n_spatial = static_cast<int64_t>(shape[0]) * shape[1] * shape[2];
  a.params_words = params_words; a.batch = batch; a.channels = channels; a.dtype = dtype; a.max_count = max_count;
  const bool chunks = max_count > kFC;
  int table_at = 0;
  for (int axis = 0; axis < 3; table_at += shape[axis], axis++) {
    if ((axes_mask >> axis & 1) == 0) continue;
    const int S = shape[axis];
    a.axis = axis;
    a.table = reinterpret_cast<const float2*>(tables_dev) + table_at;
    a.S = S;
    a.P = axis == 0 ? 1 : axis == 1 ? shape[0] : shape[0] * shape[1];
    a.Q = axis == 0 ? shape[1] * shape[2] : axis == 1 ? shape[2] : 1;
    // the widest tile that fits: with the input resident, else with the accumulator alone, else narrower
    bool resident = true;
    int shift = 5;
    if (ghost_lds_bytes(S, 32, chunks ? 2 : 1) > kLdsBudget) {
      resident = false;
      while (shift > 0 && ghost_lds_bytes(S, 1 << shift, 1) > kLdsBudget) shift = shift == 5 ? 3 : 0;
      if (ghost_lds_bytes(S, 1 << shift, 1) > kLdsBudget)
        return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: an axis of %d voxels does not fit the accumulator tile", who, S);
    }
    const int tl = 1 << shift;
    a.tl_shift = shift;
    a.tiles_q = (a.Q + tl - 1) / tl;
    const int64_t tiles = a.Q == 1 ? (static_cast<int64_t>(a.P) + tl - 1) / tl : static_cast<int64_t>(a.P) * a.tiles_q;
    const size_t lds_bytes = static_cast<size_t>(ghost_lds_bytes(S, tl, resident ? (chunks ? 2 : 1) : 1));
    const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(batch * channels));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (resident) hipLaunchKernelGGL(ghost_lines_kernel<true>, grid, dim3(kThreads), lds_bytes, s, a);
    else hipLaunchKernelGGL(ghost_lines_kernel<false>, grid, dim3(kThreads), lds_bytes, s, a);
    if (const int status = check_launch(who); status != TIO_OK) return status;
  }
  return TIO_OK;
}

extern "C" int tio_complex_abs_max(const void* z, int64_t rows, int64_t n, float* out_dev, void* stream) {
  using namespace tio;
  const char* who = "tio_complex_abs_max";
  if (rows < 0 || n < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", who);
  if (rows > 65535) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 65535 rows", who);
  if (n > (int64_t{1} << 40) / (rows > 0 ? rows : 1)) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 elements", who);
  if (rows == 0) return TIO_OK;
  if (out_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null output", who);
  if (reinterpret_cast<uintptr_t>(out_dev) % 4 != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: output not aligned", who);
  if (n > 0 && z == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null input", who);
  if (reinterpret_cast<uintptr_t>(z) % 8 != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: input not aligned to a complex64 element", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(out_dev, 0, static_cast<size_t>(rows) * sizeof(float), s) != hipSuccess) return fail(TIO_ERR_LAUNCH, "%s: clearing the output failed", who);
  if (n == 0) return TIO_OK;
  const int64_t blocks = (n / 2 + kThreads * 8 - 1) / (kThreads * 8);  // eight 16-byte loads per thread
  const dim3 grid(static_cast<unsigned>(blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks), static_cast<unsigned>(rows));
  hipLaunchKernelGGL(complex_abs_max_kernel, grid, dim3(kThreads), 0, s, static_cast<const float2*>(z), n, reinterpret_cast<uint32_t*>(out_dev));
  return check_launch(who);
}

extern "C" int tio_kspace_add_spikes(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels, const int32_t shape[3],
                                     const int32_t* params_dev, int32_t params_words, int32_t max_count, const float* tables_dev,
                                     const float* peaks_dev, const uint8_t* active_dev, void* stream) {
  using namespace tio;
  const char* who = "tio_kspace_add_spikes";
  bool empty;
  if (const int status = check_volume(who, x, y, dtype, batch, channels, shape, &empty); status != TIO_OK) return status;
  if (max_count < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative max_count", who);
  if (empty) return TIO_OK;
  if (params_dev == nullptr || tables_dev == nullptr || peaks_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null parameters, tables or peaks", who);
  if (static_cast<int64_t>(params_words) < 4 * static_cast<int64_t>(batch))
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: %d parameter words for a batch of %d (4 each, then the triples)", who, params_words, batch);
  if (reinterpret_cast<uintptr_t>(tables_dev) % 8 != 0 || reinterpret_cast<uintptr_t>(params_dev) % 4 != 0 || reinterpret_cast<uintptr_t>(peaks_dev) % 4 != 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "%s: parameters, tables or peaks not aligned", who);
  SpikeArgs a{};
  a.x = x; a.y = y; a.params = params_dev; a.table = reinterpret_cast<const float2*>(tables_dev); a.peaks = peaks_dev; a.active = active_dev;
  a.params_words = params_words; a.batch = batch; a.channels = channels; a.max_count = max_count;
  a.I = shape[0]; a.J = shape[1]; a.K = shape[2];
  a.n_spatial = shape[0] * shape[1] * shape[2];
  const int64_t packs = (static_cast<int64_t>(a.n_spatial) * dtype_size(dtype) + 15) / 16 + 2;
  int64_t blocks = (packs + kThreads - 1) / kThreads;
  blocks = blocks > 2048 ? 2048 : blocks;
  const dim3 grid(static_cast<unsigned>(blocks), static_cast<unsigned>(batch * channels));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool known = dispatch_dtype(dtype, [&](auto dt) { hipLaunchKernelGGL(add_spikes_kernel<decltype(dt)::value>, grid, dim3(kThreads), 0, s, a); });
  return known ? check_launch(who) : fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: dtype %d", who, dtype);
}
