// interpolate_adjoint.hip — the transposes of three data movers of interpolate.hip, for gradients with respect to the image:
//   tio_interpolate3d_adjoint     Resize / shared Anisotropy     (tio_interpolate3d, TIO_LINEAR and TIO_NEAREST)
//   tio_axis_gather_lerp_adjoint  per-instance Anisotropy        (tio_axis_gather_lerp)
//   tio_pad3d_adjoint             reflect / replicate / circular (tio_pad3d)
// DESIGN.md 4.8 / 4.23.
//
// All three are GATHERS: one thread per element of the result (the input-shaped gradient gx), lanes along K, every element
// written exactly once - no atomics, no zero-fill pass, a fixed order of additions per element, so two runs are bit-identical
// and an unwritten element is a bug a guard-banded buffer can see.  Gradients are float32 in and out; flat offsets are int64.
//
// What makes a gather possible.
//   interpolate3d   the forward's map is separable and, per axis, monotone: the outputs that read input index p form ONE
//                   contiguous range [first_at_least(p - 1), first_at_least(p + 1)) (linear: those whose lower tap is p - 1 or
//                   p) or [first_at_least(p), first_at_least(p + 1)) (nearest).  The ends come from a closed-form guess corrected
//                   by putting its four neighbours to the forward's OWN float32 index expression (lerp_index / floor(o * scale)
//                   of common.hpp and interpolate.hip), so membership and weights are the forward's bit for bit.
//   axis_gather     the tables are arbitrary data; the caller inverts them into per-element CSR lists (ops.Engine).
//   pad3d           along an axis, index p is the source of itself and of border positions it can list in closed form.
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace tio {
namespace {

struct InterpAdjointArgs {
  const float* gy;  // (N, out)
  float* gx;        // (N, in)
  int64_t n_bc;
  int in[3], out[3];
  float scale[3];      // as tio_interpolate3d forms them
  float inv_scale[3];  // fl(1 / scale), 0 where scale is 0: first_at_least's guess
  int mode;
};

// the forward's source index of output o along one axis (linear: the LOWER tap)
template <bool LINEAR>
__device__ __forceinline__ int source_index(int o, int n_in, int n_out, float scale) {
  if (LINEAR) return lerp_index(o, n_in, n_out, scale).i0;
  return min(static_cast<int>(floorf(__fmul_rn(static_cast<float>(o), scale))), n_in - 1);
}

// min { o in [0, n_out] : source_index(o) >= target }, source_index being non-decreasing in o with values in [0, n_in - 1]
//
// No loop and no branch.  source_index(o) >= target means fl(o * scale) >= target: the answer o* lies in
// [ceil(q (1 - 2^-24)), ceil(q)] with q = target / scale <= n_out.  The guess ceil(fl(target * inv_scale)), inv_scale = fl(1 / scale)
// from the host, carries two roundings: it is within q 2^-23 of q.  With n_out <= kMaxAxis = 2^21 both slacks stay below 1/4, so
// o* is one of guess - 2 .. guess + 1 (tio_interpolate3d_adjoint refuses longer output axes).  Those four candidates are put to
// the forward's own expression; as it is monotone, o* is the first of them plus the number that fall short.
constexpr int kMaxAxis = 1 << 21;

template <bool LINEAR>
__device__ __forceinline__ int first_at_least(int target, int n_in, int n_out, float scale, float inv_scale) {
  const int guess = static_cast<int>(fminf(ceilf(__fmul_rn(static_cast<float>(target), inv_scale)), static_cast<float>(n_out)));
  int o = guess - 2;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int candidate = guess - 2 + c;  // below 0: short by definition (o* >= 0); from n_out on: never short (o* <= n_out)
    const bool below = candidate < 0 || (candidate < n_out && source_index<LINEAR>(candidate, n_in, n_out, scale) < target);
    o += below ? 1 : 0;
  }
  o = min(o, n_out);
  o = (target > n_in - 1 || !(scale > 0.0f)) ? n_out : o;  // scale 0: every output reads index 0
  return target <= 0 ? 0 : o;
}

// the first output that reads input p.  Linear: the outputs whose lower tap is p - 1 read p as their upper tap - except on an
// axis copied one to one, where both taps are the output's own index
template <bool LINEAR>
__device__ __forceinline__ int first_reader(int p, int n_in, int n_out, float scale, float inv_scale) {
  if (LINEAR && n_in == n_out) return p;
  return first_at_least<LINEAR>(LINEAR ? p - 1 : p, n_in, n_out, scale, inv_scale);
}

// the weight with which output o reads input p along one axis, as the forward's lerp2 applies it: the two taps of the last
// index (and of an axis copied one to one) coincide, and the forward adds both products
template <bool LINEAR>
__device__ __forceinline__ float tap_weight(int o, int p, int n_in, int n_out, float scale) {
  if (!LINEAR) return 1.0f;
  const Lerp1D l = lerp_index(o, n_in, n_out, scale);
  const float w0 = l.i0 == p ? l.l0 : 0.0f, w1 = l.i1 == p ? l.l1 : 0.0f;
  return __fadd_rn(w0, w1);
}

template <bool LINEAR>
__global__ __launch_bounds__(256) void interpolate_adjoint_kernel(const InterpAdjointArgs a) {
  const int64_t n_out = static_cast<int64_t>(a.out[0]) * a.out[1] * a.out[2];
  const int64_t n_in = static_cast<int64_t>(a.in[0]) * a.in[1] * a.in[2];
  const int64_t total = n_in * a.n_bc;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t bc = t / n_in;
    int64_t r = t - bc * n_in;
    const int pk = static_cast<int>(r % a.in[2]);
    r /= a.in[2];
    const int pj = static_cast<int>(r % a.in[1]);
    const int pi = static_cast<int>(r / a.in[1]);
    const int i_lo = first_reader<LINEAR>(pi, a.in[0], a.out[0], a.scale[0], a.inv_scale[0]);
    const int i_hi = first_at_least<LINEAR>(pi + 1, a.in[0], a.out[0], a.scale[0], a.inv_scale[0]);
    const int j_lo = first_reader<LINEAR>(pj, a.in[1], a.out[1], a.scale[1], a.inv_scale[1]);
    const int j_hi = first_at_least<LINEAR>(pj + 1, a.in[1], a.out[1], a.scale[1], a.inv_scale[1]);
    const int k_lo = first_reader<LINEAR>(pk, a.in[2], a.out[2], a.scale[2], a.inv_scale[2]);
    const int k_hi = first_at_least<LINEAR>(pk + 1, a.in[2], a.out[2], a.scale[2], a.inv_scale[2]);
    const float* g = a.gy + bc * n_out;
    float sum = 0.0f;
    for (int oi = i_lo; oi < i_hi; oi++) {
      const float wi = tap_weight<LINEAR>(oi, pi, a.in[0], a.out[0], a.scale[0]);
      for (int oj = j_lo; oj < j_hi; oj++) {
        const float wj = tap_weight<LINEAR>(oj, pj, a.in[1], a.out[1], a.scale[1]);
        const float* row = g + (static_cast<int64_t>(oi) * a.out[1] + oj) * a.out[2];
        for (int ok = k_lo; ok < k_hi; ok++) {
          // the forward's order: the K weight, times the J weight, times the I weight, each product rounded
          const float wk = tap_weight<LINEAR>(ok, pk, a.in[2], a.out[2], a.scale[2]);
          const float w = __fmul_rn(__fmul_rn(wk, wj), wi);
          sum = __fadd_rn(sum, __fmul_rn(row[ok], w));
        }
      }
    }
    a.gx[t] = sum;
  }
}

struct AxisAdjointArgs {
  const float* gy;
  float* gx;
  const int32_t* offsets;    // (B, length + 1): the entries [offsets[b, p], offsets[b, p + 1]) of element b have source p
  const int32_t* positions;  // (B, entries): output position along the axis
  const float* weights;      // (B, entries), or nullptr: every weight is 1 (nearest)
  const uint8_t* active;     // (B) 0 = the forward copied the element; nullptr = all active
  int batch, channels, entries;
  int shape[3];
  int axis;
};

__global__ __launch_bounds__(256) void axis_gather_lerp_adjoint_kernel(const AxisAdjointArgs a) {
  const int64_t n = static_cast<int64_t>(a.shape[0]) * a.shape[1] * a.shape[2];
  const int64_t total = n * a.batch * a.channels;
  const int length = a.shape[a.axis];
  const int64_t stride = a.axis == 0 ? static_cast<int64_t>(a.shape[1]) * a.shape[2] : (a.axis == 1 ? a.shape[2] : 1);
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t bc = t / n;
    const int b = static_cast<int>(bc / a.channels);
    if (a.active != nullptr && a.active[b] == 0) {
      a.gx[t] = a.gy[t];
      continue;
    }
    const int64_t r = t - bc * n;
    const int k = static_cast<int>(r % a.shape[2]);
    const int j = static_cast<int>((r / a.shape[2]) % a.shape[1]);
    const int i = static_cast<int>(r / (static_cast<int64_t>(a.shape[1]) * a.shape[2]));
    const int p = a.axis == 0 ? i : (a.axis == 1 ? j : k);
    const int64_t line = t - static_cast<int64_t>(p) * stride;
    const int32_t* offsets = a.offsets + static_cast<int64_t>(b) * (length + 1);
    // the lists are data: whatever they hold, no read leaves the element's entries or its line
    const int begin = min(max(offsets[p], 0), a.entries), end = min(max(offsets[p + 1], begin), a.entries);
    const int64_t list = static_cast<int64_t>(b) * a.entries;
    float sum = 0.0f;
    for (int e = begin; e < end; e++) {
      const int q = min(max(a.positions[list + e], 0), length - 1);
      const float w = a.weights != nullptr ? a.weights[list + e] : 1.0f;
      sum = __fadd_rn(sum, __fmul_rn(a.gy[line + q * stride], w));
    }
    a.gx[t] = sum;
  }
}

struct PadAdjointArgs {
  const float* gy;  // (B * C, out)
  float* gx;        // (B * C, in)
  int64_t n_bc;
  int in[3], out[3], before[3], after[3];
  int mode;
};

// The output positions (unshifted: 0 .. out - 1) along one axis that read input index p: p itself, a run on the leading border
// and a run on the trailing border (tio_pad3d's limits: reflect pads < n, circular pads <= n, so each side folds at most once).
struct PadRuns {
  int left_start, left_count, right_start, right_count;
};

__device__ __forceinline__ PadRuns pad_runs(int p, int n, int before, int after, int mode) {
  PadRuns r;
  r.left_start = 0; r.left_count = 0; r.right_start = 0; r.right_count = 0;
  if (mode == TIO_PAD_REPLICATE) {
    if (p == 0) r.left_count = before;  // positions 0 .. before - 1
    if (p == n - 1) { r.right_start = before + n; r.right_count = after; }
  } else if (mode == TIO_PAD_CIRCULAR) {
    if (p >= n - before) { r.left_start = before + p - n; r.left_count = 1; }  // shifted position p - n
    if (p < after) { r.right_start = before + p + n; r.right_count = 1; }      // shifted position p + n
  } else {  // reflect: shifted positions -p and 2 (n - 1) - p
    if (p >= 1 && p <= before) { r.left_start = before - p; r.left_count = 1; }
    if (p <= n - 2 && p >= n - 1 - after) { r.right_start = before + 2 * (n - 1) - p; r.right_count = 1; }
  }
  return r;
}

__global__ __launch_bounds__(256) void pad_adjoint_kernel(const PadAdjointArgs a) {
  const int64_t n_out = static_cast<int64_t>(a.out[0]) * a.out[1] * a.out[2];
  const int64_t n_in = static_cast<int64_t>(a.in[0]) * a.in[1] * a.in[2];
  const int64_t total = n_in * a.n_bc;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t bc = t / n_in;
    int64_t r = t - bc * n_in;
    const int pk = static_cast<int>(r % a.in[2]);
    r /= a.in[2];
    const int pj = static_cast<int>(r % a.in[1]);
    const int pi = static_cast<int>(r / a.in[1]);
    const PadRuns ri = pad_runs(pi, a.in[0], a.before[0], a.after[0], a.mode);
    const PadRuns rj = pad_runs(pj, a.in[1], a.before[1], a.after[1], a.mode);
    const PadRuns rk = pad_runs(pk, a.in[2], a.before[2], a.after[2], a.mode);
    const float* g = a.gy + bc * n_out;
    float sum = 0.0f;
    // per axis three runs in ascending position: the leading border's, the voxel itself, the trailing border's
#pragma unroll
    for (int si = 0; si < 3; si++) {
      const int i0 = si == 0 ? ri.left_start : (si == 1 ? a.before[0] + pi : ri.right_start);
      const int ic = si == 0 ? ri.left_count : (si == 1 ? 1 : ri.right_count);
      for (int qi = i0; qi < i0 + ic; qi++) {
#pragma unroll
        for (int sj = 0; sj < 3; sj++) {
          const int j0 = sj == 0 ? rj.left_start : (sj == 1 ? a.before[1] + pj : rj.right_start);
          const int jc = sj == 0 ? rj.left_count : (sj == 1 ? 1 : rj.right_count);
          for (int qj = j0; qj < j0 + jc; qj++) {
            const float* row = g + (static_cast<int64_t>(qi) * a.out[1] + qj) * a.out[2];
#pragma unroll
            for (int sk = 0; sk < 3; sk++) {
              const int k0 = sk == 0 ? rk.left_start : (sk == 1 ? a.before[2] + pk : rk.right_start);
              const int kc = sk == 0 ? rk.left_count : (sk == 1 ? 1 : rk.right_count);
              for (int qk = k0; qk < k0 + kc; qk++) sum = __fadd_rn(sum, row[qk]);
            }
          }
        }
      }
    }
    a.gx[t] = sum;
  }
}

// the streaming launcher of interpolate.hip: at most 256 * 32 blocks, the kernels stride over the rest
template <typename Kernel, typename Args>
int launch_stream(Kernel kernel, const Args& a, int64_t total, hipStream_t s, const char* what) {
  if (total == 0) return TIO_OK;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, a);
  return check_launch(what);
}

}  // namespace
}  // namespace tio

extern "C" int tio_interpolate3d_adjoint(const float* gy, float* gx, int64_t n_batch_channels, const int32_t in_shape[3],
                                         const int32_t out_shape[3], int32_t mode, void* stream) {
  using namespace tio;
  if (in_shape == nullptr || out_shape == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_interpolate3d_adjoint: null shape");
  if (mode != TIO_NEAREST && mode != TIO_LINEAR) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_interpolate3d_adjoint: mode %d", mode);
  if (n_batch_channels < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_interpolate3d_adjoint: negative batch");
  InterpAdjointArgs a{};
  a.gy = gy; a.gx = gx; a.n_bc = n_batch_channels; a.mode = mode;
  for (int d = 0; d < 3; d++) {
    if (in_shape[d] < 1 || out_shape[d] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_interpolate3d_adjoint: shapes must be >= 1");
    if (in_shape[d] > kMaxAxis || out_shape[d] > kMaxAxis)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_interpolate3d_adjoint: an axis longer than %d voxels (axis %d)", kMaxAxis, d);
    a.in[d] = in_shape[d];
    a.out[d] = out_shape[d];
    a.scale[d] = mode == TIO_NEAREST ? static_cast<float>(in_shape[d]) / static_cast<float>(out_shape[d])
                                     : lerp_scale(in_shape[d], out_shape[d]);
    a.inv_scale[d] = a.scale[d] > 0.0f ? 1.0f / a.scale[d] : 0.0f;
  }
  if (n_batch_channels == 0) return TIO_OK;
  if (gy == nullptr || gx == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_interpolate3d_adjoint: null data");
  if (gy == gx) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_interpolate3d_adjoint: gx must not alias gy");
  const int64_t total = static_cast<int64_t>(in_shape[0]) * in_shape[1] * in_shape[2] * n_batch_channels;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == TIO_LINEAR) return launch_stream(interpolate_adjoint_kernel<true>, a, total, s, "tio_interpolate3d_adjoint");
  return launch_stream(interpolate_adjoint_kernel<false>, a, total, s, "tio_interpolate3d_adjoint");
}

extern "C" int tio_axis_gather_lerp_adjoint(const float* gy, float* gx, int32_t batch, int32_t channels, const int32_t shape[3],
                                            int32_t axis, const int32_t* offsets_dev, const int32_t* positions_dev,
                                            const float* weights_dev, int32_t entries, const uint8_t* active_dev, void* stream) {
  using namespace tio;
  if (shape == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_axis_gather_lerp_adjoint: null shape");
  if (axis < 0 || axis > 2) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_axis_gather_lerp_adjoint: axis %d", axis);
  if (batch < 0 || channels < 1 || entries < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_axis_gather_lerp_adjoint: bad batch / channels / entries");
  AxisAdjointArgs a{};
  a.gy = gy; a.gx = gx; a.offsets = offsets_dev; a.positions = positions_dev; a.weights = weights_dev; a.active = active_dev;
  a.batch = batch; a.channels = channels; a.entries = entries; a.axis = axis;
  for (int d = 0; d < 3; d++) {
    if (shape[d] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_axis_gather_lerp_adjoint: shapes must be >= 1");
    a.shape[d] = shape[d];
  }
  if (batch == 0) return TIO_OK;
  if (gy == nullptr || gx == nullptr || offsets_dev == nullptr || (entries > 0 && positions_dev == nullptr))
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_axis_gather_lerp_adjoint: null argument");
  if (gy == gx) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_axis_gather_lerp_adjoint: gx must not alias gy");
  const int64_t total = static_cast<int64_t>(shape[0]) * shape[1] * shape[2] * batch * channels;
  return launch_stream(axis_gather_lerp_adjoint_kernel, a, total, static_cast<hipStream_t>(stream), "tio_axis_gather_lerp_adjoint");
}

extern "C" int tio_pad3d_adjoint(const float* gy, float* gx, int32_t batch, int32_t channels, const int32_t in_shape[3],
                                 const int32_t padding[6], int32_t mode, void* stream) {
  using namespace tio;
  if (in_shape == nullptr || padding == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_pad3d_adjoint: null argument");
  if (mode != TIO_PAD_REFLECT && mode != TIO_PAD_REPLICATE && mode != TIO_PAD_CIRCULAR)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_pad3d_adjoint: mode %d (reflect, replicate or circular; the transpose of constant padding is a crop)", mode);
  if (batch < 0 || channels < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_pad3d_adjoint: bad batch / channels");
  PadAdjointArgs a{};
  a.gy = gy; a.gx = gx; a.n_bc = static_cast<int64_t>(batch) * channels; a.mode = mode;
  for (int d = 0; d < 3; d++) {
    if (in_shape[d] < 1 || padding[2 * d] < 0 || padding[2 * d + 1] < 0)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_pad3d_adjoint: shapes must be >= 1 and paddings >= 0");
    // tio_pad3d's own limits: each side then folds onto the axis at most once
    if (mode == TIO_PAD_REFLECT && (padding[2 * d] >= in_shape[d] || padding[2 * d + 1] >= in_shape[d]))
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_pad3d_adjoint: reflect padding must be smaller than the axis (axis %d)", d);
    if (mode == TIO_PAD_CIRCULAR && (padding[2 * d] > in_shape[d] || padding[2 * d + 1] > in_shape[d]))
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_pad3d_adjoint: circular padding must not exceed the axis (axis %d)", d);
    a.in[d] = in_shape[d];
    a.before[d] = padding[2 * d];
    a.after[d] = padding[2 * d + 1];
    a.out[d] = in_shape[d] + padding[2 * d] + padding[2 * d + 1];
  }
  if (batch == 0) return TIO_OK;
  if (gy == nullptr || gx == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_pad3d_adjoint: null data");
  if (gy == gx) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_pad3d_adjoint: gx must not alias gy");
  const int64_t total = static_cast<int64_t>(in_shape[0]) * in_shape[1] * in_shape[2] * a.n_bc;
  return launch_stream(pad_adjoint_kernel, a, total, static_cast<hipStream_t>(stream), "tio_pad3d_adjoint");
}
