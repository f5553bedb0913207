// points.hip — tio_points_warp: carry points through a resampling, one thread per point, one launch per batch.
//
// A resampling computes out(o) = in(s(o)): s maps an OUTPUT voxel coordinate to the INPUT coordinate it samples.  A point
// attached to the image moves the other way, p -> s^-1(p).  s is the reference's sampling grid (spatial.py:1570-1577):
//   no field          s(o) = M o                                   o = Minv p, one matrix
//   affine_first      s(o) = M o + d(o) / spacing_in
//   otherwise         s(o) = M (o + d(o) / spacing_out)
// with d the trilinear interpolation of the (n_i, n_j, n_k, 3) control points at u_a = o_a (n_a - 1) / max(S_a - 1, 1)
// (align_corners=True, spatial.py:2171-2189), u clamped to [0, n_a - 1]: the field extends constantly outside the output
// grid, so a point outside the field of view stays defined (and the field part of the Jacobian is zero there).
//
// With a field, s(o) = p is solved by a damped Newton iteration from the affine-only answer: the analytic Jacobian of the
// trilinear cell, the step halved while the residual max|s(o) - p| does not decrease, until the residual is at most
// TIO_POINTS_TOLERANCE voxel or TIO_POINTS_MAX_ITERATIONS steps were taken.  A point that does not get there keeps its
// best iterate and reports status 1; one that does takes one more full step, kept when it lowers the residual.
// Everything is float64 (the library is built with -ffp-contract=off: every product
// and sum rounds on its own, as a numpy restatement does); the result is rounded to float32 once, at the store.
//
// Launch: 256-thread blocks, none of which spans two batch elements.  Element b owns ceil(n_b / 256) consecutive blocks; a
// block finds its element by walking the offsets (uniform across the block: scalar loads), so an element without points
// owns no block and costs nothing.  The element's parameter block goes to LDS once per block.
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace tio {
namespace {

constexpr int PW_THREADS = 256;
constexpr int PB = TIO_POINTS_BLOCK_DOUBLES;
// layout of one element's parameter block (doubles)
constexpr int PB_M = 0, PB_MINV = 12, PB_OUT_SHAPE = 24, PB_SPACING_IN = 27, PB_SPACING_OUT = 30, PB_AFFINE_FIRST = 33, PB_GRID = 34,
              PB_CP_OFFSET = 37;
constexpr int PW_MAX_HALVINGS = 30;

struct Field {
  const float* cp;  // this element's (n_i, n_j, n_k, 3) control points
  int n[3];
  double scale[3];  // (n_a - 1) / max(S_a - 1, 1)
};

__device__ __forceinline__ void apply34(const double* m, const double v[3], double out[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) out[r] = ((m[4 * r] * v[0] + m[4 * r + 1] * v[1]) + m[4 * r + 2] * v[2]) + m[4 * r + 3];
}

// d(o) (mm) and D[c][a] = d d_c / d o_a
__device__ __forceinline__ void displacement(const Field& f, const double o[3], double d[3], double D[3][3]) {
  int i0[3], i1[3];
  double t[3], slope[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double hi = static_cast<double>(f.n[a] - 1);
    const double raw = o[a] * f.scale[a];
    const bool inside = raw >= 0.0 && raw <= hi;  // (a NaN is "outside": the field part of its Jacobian is zero)
    const double u = fmin(fmax(raw, 0.0), hi);    // fmax / fmin drop a NaN: index 0
    int lo = static_cast<int>(floor(u));
    lo = max(0, min(lo, f.n[a] - 2));  // the last cell takes u == n - 1 with t == 1; n == 1: cell 0, t == 0
    i0[a] = lo;
    i1[a] = min(lo + 1, f.n[a] - 1);
    t[a] = u - static_cast<double>(lo);
    slope[a] = inside ? f.scale[a] : 0.0;
  }
  const int64_t sj = static_cast<int64_t>(f.n[2]) * 3, si = sj * f.n[1];
  double c[2][2][2][3];
#pragma unroll
  for (int x = 0; x < 2; x++)
#pragma unroll
    for (int y = 0; y < 2; y++)
#pragma unroll
      for (int z = 0; z < 2; z++) {
        const float* corner = f.cp + (x ? i1[0] : i0[0]) * si + (y ? i1[1] : i0[1]) * sj + static_cast<int64_t>(z ? i1[2] : i0[2]) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) c[x][y][z][k] = static_cast<double>(corner[k]);
      }
  const double w[3][2] = {{1.0 - t[0], t[0]}, {1.0 - t[1], t[1]}, {1.0 - t[2], t[2]}};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    // along K, then J, then I; the differences give the three partial derivatives of the cell
    double vk[2][2], dk[2][2];
#pragma unroll
    for (int x = 0; x < 2; x++)
#pragma unroll
      for (int y = 0; y < 2; y++) {
        vk[x][y] = c[x][y][0][k] * w[2][0] + c[x][y][1][k] * w[2][1];
        dk[x][y] = c[x][y][1][k] - c[x][y][0][k];
      }
    double vj[2], dj[2], dkj[2];
#pragma unroll
    for (int x = 0; x < 2; x++) {
      vj[x] = vk[x][0] * w[1][0] + vk[x][1] * w[1][1];
      dj[x] = vk[x][1] - vk[x][0];
      dkj[x] = dk[x][0] * w[1][0] + dk[x][1] * w[1][1];
    }
    d[k] = vj[0] * w[0][0] + vj[1] * w[0][1];
    D[k][0] = (vj[1] - vj[0]) * slope[0];
    D[k][1] = (dj[0] * w[0][0] + dj[1] * w[0][1]) * slope[1];
    D[k][2] = (dkj[0] * w[0][0] + dkj[1] * w[0][1]) * slope[2];
  }
}

// s(o) and its Jacobian J[r][a] = d s_r / d o_a
__device__ __forceinline__ void forward_map(const double* hdr, const Field& f, bool affine_first, const double o[3], double s[3],
                                            double J[3][3]) {
  const double* M = hdr + PB_M;
  double d[3], D[3][3];
  displacement(f, o, d, D);
  if (affine_first) {
    apply34(M, o, s);
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double mm = hdr[PB_SPACING_IN + r];
      s[r] = s[r] + d[r] / mm;
#pragma unroll
      for (int a = 0; a < 3; a++) J[r][a] = M[4 * r + a] + D[r][a] / mm;
    }
  } else {
    double q[3], Q[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double mm = hdr[PB_SPACING_OUT + r];
      q[r] = o[r] + d[r] / mm;
#pragma unroll
      for (int a = 0; a < 3; a++) Q[r][a] = (r == a ? 1.0 : 0.0) + D[r][a] / mm;
    }
    apply34(M, q, s);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int a = 0; a < 3; a++) J[r][a] = (M[4 * r] * Q[0][a] + M[4 * r + 1] * Q[1][a]) + M[4 * r + 2] * Q[2][a];
  }
}

__device__ __forceinline__ double residual(const double s[3], const double p[3], double r[3]) {
#pragma unroll
  for (int a = 0; a < 3; a++) r[a] = s[a] - p[a];
  return fmax(fmax(fabs(r[0]), fabs(r[1])), fabs(r[2]));
}

// J x = r by Cramer's rule; false when J is singular (or not finite)
__device__ __forceinline__ bool solve3(const double J[3][3], const double r[3], double x[3]) {
  const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
  const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
  const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
  const double det = (J[0][0] * c00 + J[0][1] * c01) + J[0][2] * c02;
  if (!(fabs(det) > 0.0) || !(fabs(det) < 1.0e300)) return false;
  const double c10 = J[0][2] * J[2][1] - J[0][1] * J[2][2];
  const double c11 = J[0][0] * J[2][2] - J[0][2] * J[2][0];
  const double c12 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
  const double c20 = J[0][1] * J[1][2] - J[0][2] * J[1][1];
  const double c21 = J[0][2] * J[1][0] - J[0][0] * J[1][2];
  const double c22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
  x[0] = ((c00 * r[0] + c10 * r[1]) + c20 * r[2]) / det;
  x[1] = ((c01 * r[0] + c11 * r[1]) + c21 * r[2]) / det;
  x[2] = ((c02 * r[0] + c12 * r[1]) + c22 * r[2]) / det;
  return true;
}

__global__ __launch_bounds__(PW_THREADS) void points_warp_kernel(const float* __restrict__ points, float* __restrict__ out,
                                                                  int8_t* __restrict__ status, int64_t n_total,
                                                                  const int32_t* __restrict__ offsets, int batch,
                                                                  const double* __restrict__ blocks, const float* __restrict__ cp,
                                                                  int64_t cp_floats) {
  __shared__ double hdr[PB];
  // which element owns this block (uniform: the walk runs on the scalar unit)
  int64_t block = blockIdx.x;
  int element = 0, first = 0, count = 0;
  for (; element < batch; element++) {
    first = offsets[element];
    count = offsets[element + 1] - first;
    const int64_t owned = (static_cast<int64_t>(count) + PW_THREADS - 1) / PW_THREADS;
    if (block < owned) break;
    block -= owned;
  }
  if (element >= batch) return;  // (uniform: the whole block leaves before the barrier)
  if (threadIdx.x < PB) hdr[threadIdx.x] = blocks[static_cast<int64_t>(element) * PB + threadIdx.x];
  __syncthreads();
  const int64_t local = block * PW_THREADS + threadIdx.x;
  const int64_t index = first + local;
  if (local >= count || index < 0 || index >= n_total) return;

  const double p[3] = {static_cast<double>(points[3 * index]), static_cast<double>(points[3 * index + 1]),
                       static_cast<double>(points[3 * index + 2])};
  double o[3];
  apply34(hdr + PB_MINV, p, o);
  int code = 0;

  if (hdr[PB_CP_OFFSET] >= 0.0) {
    Field f;
    // (the header is data: sizes are checked as doubles before they become integers, so that no product can overflow)
    bool usable = cp != nullptr && hdr[PB_CP_OFFSET] <= 9.0e15;
    const int64_t cp_offset = usable ? static_cast<int64_t>(hdr[PB_CP_OFFSET]) : 0;
    int64_t cells = 3;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const bool sized = hdr[PB_GRID + a] >= 1.0 && hdr[PB_GRID + a] <= 1048576.0;
      f.n[a] = sized ? static_cast<int>(hdr[PB_GRID + a]) : 1;
      usable = usable && sized;
      cells *= f.n[a];
      const double extent = hdr[PB_OUT_SHAPE + a] - 1.0;
      f.scale[a] = static_cast<double>(f.n[a] - 1) / (extent > 1.0 ? extent : 1.0);
    }
    usable = usable && cp_offset + cells <= cp_floats;
    if (!usable) {
      code = 2;  // a header that names control points outside the buffer: the affine-only answer, and nothing is read
    } else {
      f.cp = cp + cp_offset;
      const bool affine_first = hdr[PB_AFFINE_FIRST] != 0.0;
      double s[3], J[3][3], r[3];
      forward_map(hdr, f, affine_first, o, s, J);
      double err = residual(s, p, r);
      code = 1;
      for (int iteration = 0; iteration < TIO_POINTS_MAX_ITERATIONS; iteration++) {
        if (err <= TIO_POINTS_TOLERANCE) {
          code = 0;
          break;
        }
        double step[3];
        if (!solve3(J, r, step)) break;
        double lambda = 1.0;
        bool improved = false;
        for (int halving = 0; halving < PW_MAX_HALVINGS; halving++) {
          const double trial[3] = {o[0] - lambda * step[0], o[1] - lambda * step[1], o[2] - lambda * step[2]};
          double st[3], Jt[3][3], rt[3];
          forward_map(hdr, f, affine_first, trial, st, Jt);
          const double et = residual(st, p, rt);
          if (et < err) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
              o[a] = trial[a];
              r[a] = rt[a];
#pragma unroll
              for (int b = 0; b < 3; b++) J[a][b] = Jt[a][b];
            }
            err = et;
            improved = true;
            break;
          }
          lambda *= 0.5;
        }
        if (!improved) break;  // stalled (or the residual is NaN): the best iterate stays
      }
      if (code == 1 && err <= TIO_POINTS_TOLERANCE) code = 0;  // the last step got there
      // The stop decides the status.  One more full step from a converged iterate squares what is left of the residual
      // (1e-7 -> the float64 floor): kept when it lowers the residual, at the price of one more evaluation of s.
      double step[3];
      if (code == 0 && err > 0.0 && solve3(J, r, step)) {
        const double trial[3] = {o[0] - step[0], o[1] - step[1], o[2] - step[2]};
        double st[3], Jt[3][3], rt[3];
        forward_map(hdr, f, affine_first, trial, st, Jt);
        if (residual(st, p, rt) < err) {
#pragma unroll
          for (int a = 0; a < 3; a++) o[a] = trial[a];
        }
      }
    }
  }
  out[3 * index] = static_cast<float>(o[0]);
  out[3 * index + 1] = static_cast<float>(o[1]);
  out[3 * index + 2] = static_cast<float>(o[2]);
  if (status != nullptr) status[index] = static_cast<int8_t>(code);
}

}  // namespace
}  // namespace tio

extern "C" int tio_points_warp(const float* points, float* out, int8_t* status, int64_t n_total, const int32_t* offsets_host,
                               const int32_t* offsets_dev, int32_t batch, const double* blocks_dev, const float* control_points_dev,
                               int64_t control_floats, void* stream) {
  using namespace tio;
  if (batch < 0 || n_total < 0 || control_floats < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_points_warp: negative size");
  if (n_total > INT32_MAX) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_points_warp: more than 2^31 - 1 points (int32 offsets)");
  if (batch == 0 || n_total == 0) {
    if (batch > 0 && offsets_host != nullptr && (offsets_host[0] != 0 || offsets_host[batch] != 0))
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_points_warp: offsets do not span the %lld points", static_cast<long long>(n_total));
    return TIO_OK;
  }
  if (offsets_host == nullptr || offsets_dev == nullptr || blocks_dev == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_points_warp: null offsets or parameter blocks");
  if (points == nullptr || out == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_points_warp: null points");
  if (control_floats > 0 && control_points_dev == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_points_warp: null control points of %lld floats", static_cast<long long>(control_floats));
  if (offsets_host[0] != 0 || offsets_host[batch] != n_total)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_points_warp: offsets run from %d to %d, expected 0 to %lld", offsets_host[0], offsets_host[batch],
                static_cast<long long>(n_total));
  int64_t blocks = 0;
  for (int32_t b = 0; b < batch; b++) {
    const int64_t count = static_cast<int64_t>(offsets_host[b + 1]) - offsets_host[b];
    if (count < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_points_warp: offsets decrease at element %d", b);
    blocks += (count + PW_THREADS - 1) / PW_THREADS;
  }
  hipLaunchKernelGGL(points_warp_kernel, dim3(static_cast<unsigned>(blocks)), dim3(PW_THREADS), 0, static_cast<hipStream_t>(stream), points, out,
                     status, n_total, offsets_dev, batch, blocks_dev, control_points_dev, control_floats);
  return check_launch("tio_points_warp");
}
