// resample.hip — fused spatial resampling for gfx950 (tio_resample3d).
//
// One launch replaces the reference's grid construction + two grid_sample calls
// (SURVEY.md §2.2 K1–K7; reference spatial.py:1504-1648, 1695-1731, 2171-2189):
// every output voxel computes its source coordinate in registers — affine 3x4
// as the same forward-FMA chain MKL's sgemm produces, optional trilinear lookup
// of the elastic control points staged in LDS, the redundant normalise /
// un-normalise round trip of F.grid_sample — then gathers 8 taps (or 1 for
// nearest), accumulates the in-bounds weight mask in the same order as ATen and
// applies `mask > 0.5 ? value : fill`.  No (I,J,K,3) grid ever reaches HBM.
//
// HBM-bound by design (algorithmic traffic = read input once + write output
// once); no MFMA: this is a gather/stencil op.  What actually limits it is the
// per-voxel float32 instruction count needed to stay bit-identical with the
// reference, so the kernel is organised around (1) latency hiding — one block
// walks kTileI output slabs so the control points are staged once per 2048
// voxels and many independent gathers are in flight, (2) a wave-uniform
// "interior" path (all 8 taps of all 64 lanes in bounds: no predication, no
// mask arithmetic — the mask is exactly > 0.5 there), (3) IEEE-exact division
// by reciprocal + two FMA refinements instead of the 12-instruction expansion.
//
// Host side, at the end of this file: the dispatcher — check_geometry, sort_images, choose_float_road (which road a call takes and why; the table
// is in DESIGN.md 4.1) and one launcher per road, tied together by resample3d_impl.
#include <type_traits>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>
#include <algorithm>

#include "resample_args.hpp"
#include "resample_coords.hpp"

namespace tio {

constexpr int kTileI = 8;          // output slabs walked by one block
constexpr int kRowsPerBlock = 4;   // one wave per output row (jo)
constexpr int kLanes = 64;         // contiguous ko per wave → coalesced stores
constexpr int kMaxCpLds = 6144;    // floats of control points staged in LDS (24 KiB)
constexpr int kLdsFloatsPerCU = 40960;   // 160 KiB
constexpr int kPlannedMinBricks = 12288;  // below: one kernel with in-kernel boxes (the plan costs a launch)
constexpr int kTileMinCap = 6144;       // the per-voxel fallback parks 8 planes x 3 coordinates x 256 threads there
constexpr int kTileBlocksPerCU = 3;       // resident blocks the default LDS budget is sized for

// ---- sampling --------------------------------------------------------------------
// Interior path: every tap of every lane of the wave is in bounds, so there is no
// predication, no mask arithmetic (the in-bounds weight sum is 1 up to rounding,
// always > 0.5) and the 8 offsets are base + launch constants.
template <int DT>
__device__ __forceinline__ void sample_interior(const ImgArgs& g, int b, int64_t n_in, int64_t n_out, int64_t o_idx,
                                                const float (&w)[8], int base, int dJK, int dK, int offn) {
  for (int c = 0; c < g.channels; c++) {
    const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
    const typename Elem<DT>::type* p = static_cast<const typename Elem<DT>::type*>(g.in) + bc * n_in;
    float val;
    if (g.interp == TIO_LINEAR_ADJOINT) {  // backward of TIO_LINEAR: scatter g * w to the 8 taps (all in bounds here)
      if constexpr (DT == TIO_F32) {
        const float gv = static_cast<const float*>(g.out)[bc * n_out + o_idx];
        float* q = const_cast<float*>(static_cast<const float*>(g.in)) + bc * n_in + base;
        unsafeAtomicAdd(q, gv * w[0]); unsafeAtomicAdd(q + dJK, gv * w[1]);
        unsafeAtomicAdd(q + dK, gv * w[2]); unsafeAtomicAdd(q + dJK + dK, gv * w[3]);
        unsafeAtomicAdd(q + 1, gv * w[4]); unsafeAtomicAdd(q + dJK + 1, gv * w[5]);
        unsafeAtomicAdd(q + dK + 1, gv * w[6]); unsafeAtomicAdd(q + dJK + dK + 1, gv * w[7]);
      }
      continue;
    }
    if (g.interp == TIO_LINEAR) {
      const typename Elem<DT>::type* q = p + base;
      const float v0 = Elem<DT>::load(q, 0), v1 = Elem<DT>::load(q, dJK);
      const float v2 = Elem<DT>::load(q, dK), v3 = Elem<DT>::load(q, dJK + dK);
      const float v4 = Elem<DT>::load(q, 1), v5 = Elem<DT>::load(q, dJK + 1);
      const float v6 = Elem<DT>::load(q, dK + 1), v7 = Elem<DT>::load(q, dJK + dK + 1);
      val = __fadd_rn(0.0f, __fmul_rn(v0, w[0]));  // keep ATen's `0 + v*w` (sign of zero)
      val = __fadd_rn(val, __fmul_rn(v1, w[1]));
      val = __fadd_rn(val, __fmul_rn(v2, w[2]));
      val = __fadd_rn(val, __fmul_rn(v3, w[3]));
      val = __fadd_rn(val, __fmul_rn(v4, w[4]));
      val = __fadd_rn(val, __fmul_rn(v5, w[5]));
      val = __fadd_rn(val, __fmul_rn(v6, w[6]));
      val = __fadd_rn(val, __fmul_rn(v7, w[7]));
    } else {
      val = Elem<DT>::load(p, offn);
    }
    Elem<DT>::store(g.out, bc * n_out + o_idx, val);
  }
}

// Boundary path: per-tap bounds, zero padding, in-bounds weight mask and fill, in
// exactly ATen's accumulation order (tnw,tne,tsw,tse,bnw,bne,bsw,bse).
template <int DT>
__device__ __forceinline__ void sample_boundary(const ImgArgs& g, int b, int64_t n_in, int64_t n_out, int64_t o_idx,
                                                const float (&w)[8], const int (&off)[8], unsigned okbits, float mask,
                                                int offn, bool okn) {
  for (int c = 0; c < g.channels; c++) {
    const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
    const typename Elem<DT>::type* p = static_cast<const typename Elem<DT>::type*>(g.in) + bc * n_in;
    float val;
    if (g.interp == TIO_LINEAR_ADJOINT) {  // backward of TIO_LINEAR with per-tap bounds; no gradient where the fill was taken
      if constexpr (DT == TIO_F32) {
        if (g.fill == nullptr || mask > 0.5f) {
          const float gv = static_cast<const float*>(g.out)[bc * n_out + o_idx];
          float* q = const_cast<float*>(static_cast<const float*>(g.in)) + bc * n_in;
#pragma unroll
          for (int k = 0; k < 8; k++)
            if ((okbits >> k) & 1u) unsafeAtomicAdd(q + off[k], gv * w[k]);
        }
      }
      continue;
    }
    if (g.interp == TIO_LINEAR) {
      val = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const float v = Elem<DT>::load(p, off[k]);
        const float next = __fadd_rn(val, __fmul_rn(v, w[k]));
        val = ((okbits >> k) & 1u) ? next : val;
      }
    } else {
      const float v = Elem<DT>::load(p, offn);
      val = okn ? v : 0.0f;
    }
    if (g.fill != nullptr) val = (mask > 0.5f) ? val : g.fill[c];
    Elem<DT>::store(g.out, bc * n_out + o_idx, val);
  }
}

}  // namespace tio
#include "resample_label.hpp"
namespace tio {

// DTMODE selects which element types a kernel instantiation can sample, so that the
// common launches do not pay registers for the rare ones: 0 = float32 only,
// 1 = float32 + {int16, uint8, int32} (intensity + label maps), 2 = every tio_dtype.
#define TIO_DISPATCH_IMAGE(DTMODE, DTYPE, CALL)                 \
  if constexpr (DTMODE == 0) {                                  \
    CALL(TIO_F32);                                              \
  } else {                                                      \
    switch (DTYPE) { /* uniform → scalar branch */              \
      case TIO_F32: CALL(TIO_F32); break;                       \
      case TIO_I16: CALL(TIO_I16); break;                       \
      case TIO_U8: CALL(TIO_U8); break;                         \
      case TIO_I32: CALL(TIO_I32); break;                       \
      default:                                                  \
        if constexpr (DTMODE == 2) {                            \
          switch (DTYPE) {                                      \
            case TIO_I64: CALL(TIO_I64); break;                 \
            case TIO_F16: CALL(TIO_F16); break;                 \
            case TIO_BF16: CALL(TIO_BF16); break;               \
            case TIO_F64: CALL(TIO_F64); break;                 \
            default: CALL(TIO_I8); break;                       \
          }                                                     \
        }                                                       \
        break;                                                  \
    }                                                           \
  }

// LABEL_PV = true: the same coordinates, every image resampled in the "label"
// partial-volume mode (resample_label.hpp); launched separately so that the intensity
// kernels carry none of its registers.
// B-spline orders 2 / 3 (include/tio_hip.h: TIO_QUADRATIC): same operations, same order as oracle/tio_oracle.c
__device__ __forceinline__ int spline_reflect(int i, int n) {
  const int n2 = 2 * n;
  if (i < 0) i = -i - 1;
  i %= n2;
  return i >= n ? n2 - i - 1 : i;
}

__device__ __forceinline__ void spline_weights(float x, int order, int& low, float (&w)[4]) {
  if (order == 2) {
    const float c = floorf(__fadd_rn(x, 0.5f));
    const float t = __fsub_rn(x, c);
    low = static_cast<int>(c) - 1;
    const float m = __fsub_rn(0.5f, t), p = __fadd_rn(0.5f, t);
    w[0] = __fmul_rn(__fmul_rn(0.5f, m), m);
    w[1] = __fsub_rn(0.75f, __fmul_rn(t, t));
    w[2] = __fmul_rn(__fmul_rn(0.5f, p), p);
    w[3] = 0.0f;
  } else {
    const float f = floorf(x);
    const float t = __fsub_rn(x, f);
    const float u = __fsub_rn(1.0f, t);
    low = static_cast<int>(f) - 1;
    w[0] = __fdiv_rn(__fmul_rn(__fmul_rn(u, u), u), 6.0f);
    w[1] = __fdiv_rn(__fadd_rn(__fmul_rn(__fmul_rn(__fmul_rn(t, t), __fsub_rn(t, 2.0f)), 3.0f), 4.0f), 6.0f);
    w[2] = __fdiv_rn(__fadd_rn(__fmul_rn(__fmul_rn(__fmul_rn(u, u), __fsub_rn(u, 2.0f)), 3.0f), 4.0f), 6.0f);
    w[3] = __fdiv_rn(__fmul_rn(__fmul_rn(t, t), t), 6.0f);
  }
}

// Orders 4 - 7 (oracle/tio_oracle.c: spline_weights_high, operation for operation): the Cox - de Boor recursion of the
// uniform B-spline in float64, v_j = N_m(tau + j), every term positive; tap k at low + k weighs v_{order - k}.
template <int ORDER>
__device__ __forceinline__ void spline_weights_high(float x, int& low, float (&w)[ORDER + 1]) {
  constexpr bool odd = (ORDER & 1) != 0;
  const float base = odd ? floorf(x) : floorf(__fadd_rn(x, 0.5f));
  const double tau = odd ? __dsub_rn(static_cast<double>(x), static_cast<double>(base))
                         : __dadd_rn(__dsub_rn(static_cast<double>(x), static_cast<double>(base)), 0.5);
  low = static_cast<int>(base) - (odd ? (ORDER - 1) / 2 : ORDER / 2);
  double v[ORDER + 1];
  v[0] = 1.0;
#pragma unroll
  for (int j = 1; j <= ORDER; j++) v[j] = 0.0;
#pragma unroll
  for (int m = 2; m <= ORDER + 1; m++) {
    const double inv = __ddiv_rn(1.0, static_cast<double>(m - 1));
#pragma unroll
    for (int j = ORDER; j >= 0; j--) {
      if (j <= m - 1) {
        const double same = j <= m - 2 ? v[j] : 0.0, below = j >= 1 ? v[j - 1] : 0.0;
        v[j] = __dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(tau, static_cast<double>(j)), same),
                                   __dmul_rn(__dsub_rn(__dsub_rn(static_cast<double>(m), tau), static_cast<double>(j)), below)), inv);
      }
    }
  }
#pragma unroll
  for (int k = 0; k <= ORDER; k++) w[k] = static_cast<float>(v[ORDER - k]);
}

template <int ORDER>
__device__ __forceinline__ float spline_sample_high(const float* __restrict__ coef, int I, int J, int K, float vi, float vj, float vk) {
  const float tiny = 5e-2f;
  if (!((vi > -tiny) & (vi < __fadd_rn(static_cast<float>(I - 1), tiny)) & (vj > -tiny) & (vj < __fadd_rn(static_cast<float>(J - 1), tiny)) &
        (vk > -tiny) & (vk < __fadd_rn(static_cast<float>(K - 1), tiny))))
    return 0.0f;
  int li, lj, lk;
  float wi[ORDER + 1], wj[ORDER + 1], wk[ORDER + 1];
  spline_weights_high<ORDER>(vi, li, wi);
  spline_weights_high<ORDER>(vj, lj, wj);
  spline_weights_high<ORDER>(vk, lk, wk);
  int kc[ORDER + 1];
#pragma unroll
  for (int r = 0; r <= ORDER; r++) kc[r] = spline_reflect(lk + r, K);
  float val = 0.0f;
#pragma unroll 1
  for (int p = 0; p <= ORDER; p++) {
    const int64_t ia = spline_reflect(li + p, I);
#pragma unroll 1
    for (int q = 0; q <= ORDER; q++) {
      const int64_t jb = spline_reflect(lj + q, J);
      // (wi / wj indexed by loop counters that are not unrolled: selected from registers, no scratch)
      float wp = wi[0], wq = wj[0];
#pragma unroll
      for (int e = 1; e <= ORDER; e++) { wp = p == e ? wi[e] : wp; wq = q == e ? wj[e] : wq; }
      const float wab = __fmul_rn(wp, wq);
      const float* row = coef + (ia * J + jb) * K;
#pragma unroll
      for (int r = 0; r <= ORDER; r++) {
        const float wabc = __fmul_rn(wab, wk[r]);
        val = __fadd_rn(val, __fmul_rn(wabc, row[kc[r]]));
      }
    }
  }
  return val;
}

__device__ __forceinline__ float spline_sample(const float* __restrict__ coef, int I, int J, int K, float vi, float vj, float vk, int order) {
  if (order == 4) return spline_sample_high<4>(coef, I, J, K, vi, vj, vk);
  if (order == 5) return spline_sample_high<5>(coef, I, J, K, vi, vj, vk);
  if (order == 6) return spline_sample_high<6>(coef, I, J, K, vi, vj, vk);
  if (order == 7) return spline_sample_high<7>(coef, I, J, K, vi, vj, vk);
  const float tiny = 5e-2f;
  if (!((vi > -tiny) & (vi < __fadd_rn(static_cast<float>(I - 1), tiny)) & (vj > -tiny) & (vj < __fadd_rn(static_cast<float>(J - 1), tiny)) &
        (vk > -tiny) & (vk < __fadd_rn(static_cast<float>(K - 1), tiny))))
    return 0.0f;
  int li, lj, lk;
  float wi[4], wj[4], wk[4];
  spline_weights(vi, order, li, wi);
  spline_weights(vj, order, lj, wj);
  spline_weights(vk, order, lk, wk);
  float val = 0.0f;
  for (int p = 0; p <= order; p++) {
    const int64_t ia = spline_reflect(li + p, I);
    for (int q = 0; q <= order; q++) {
      const int64_t jb = spline_reflect(lj + q, J);
      const float wab = __fmul_rn(wi[p], wj[q]);
      for (int r = 0; r <= order; r++) {
        const int64_t kc = spline_reflect(lk + r, K);
        const float wabc = __fmul_rn(wab, wk[r]);
        val = __fadd_rn(val, __fmul_rn(wabc, coef[(ia * J + jb) * K + kc]));
      }
    }
  }
  return val;
}

// MODE: 0 = nearest / trilinear images, 1 = "label" partial-volume images, 2 = B-spline images (coefficients in, float32 out)
template <bool ELASTIC_POSSIBLE, int DTMODE, int MODE = 0>
__global__ __launch_bounds__(kRowsPerBlock* kLanes) void resample_kernel(const ResampleArgs a) {
  constexpr bool LABEL_PV = MODE == 1;
  extern __shared__ __attribute__((aligned(16))) float s_cp[];

  // tile decode: XCD-contiguous chunks of (b, it, jt, kt), kt fastest
  const unsigned tile = xcd_remap(blockIdx.x, gridDim.x);
  const int kt = tile % a.tiles_k;
  const unsigned t1 = tile / a.tiles_k;
  const int jt = t1 % a.tiles_j;
  const unsigned t2 = t1 / a.tiles_j;
  const int it = t2 % a.tiles_i;
  const int b = t2 / a.tiles_i;

  const int lane = threadIdx.x & (kLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int jo = jt * kRowsPerBlock + wave;
  const int ko = kt * kLanes + lane;
  const int i_begin = it * kTileI;
  const int i_end = min(i_begin + kTileI, a.Io);

  const bool pass = a.passthrough != nullptr && a.passthrough[b] != 0;
  bool elastic = false;
  bool cp_in_lds = false;
  const float* cp_global = nullptr;
  if constexpr (ELASTIC_POSSIBLE) {
    elastic = !(a.cp_skip != nullptr && a.cp_skip[b] != 0);
    if (elastic && !pass) {
      const int n_cp = a.ni * a.nj * a.nk * 3;
      cp_global = a.cp + (a.cp_batched ? static_cast<int64_t>(b) * n_cp : 0);
      if (n_cp <= kMaxCpLds) {
        for (int t = threadIdx.x; t < n_cp; t += blockDim.x) s_cp[t] = cp_global[t];
        __syncthreads();
        cp_in_lds = true;
      }
    }
  }
  if (jo >= a.Jo || ko >= a.Ko) return;

  const int64_t n_in = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t n_out = static_cast<int64_t>(a.Io) * a.Jo * a.Ko;
  const int64_t row = static_cast<int64_t>(jo) * a.Ko + ko;
  const int64_t slab = static_cast<int64_t>(a.Jo) * a.Ko;

  if (pass) {  // gated-out element: bit-exact copy (spatial.py:1101-1106)
    for (int io = i_begin; io < i_end; io++) {
      const int64_t o_idx = io * slab + row;
      for (int im = 0; im < a.n_images; im++) {
        const ImgArgs& g = a.img[im];
        const int es = dtype_size(g.dtype);
        for (int c = 0; c < g.channels; c++) {
          const int64_t off = (static_cast<int64_t>(b) * g.channels + c) * n_out + o_idx;
          if (g.interp == TIO_LINEAR_ADJOINT) {
            // backward of the bit-exact copy: the identity.  `in` is the gradient accumulator, `out` the incoming
            // gradient, which is only ever READ in this mode (every voxel is visited once: no atomic needed)
            float* acc = const_cast<float*>(static_cast<const float*>(g.in));
            acc[off] = __fadd_rn(acc[off], static_cast<const float*>(g.out)[off]);
            continue;
          }
          const char* s = static_cast<const char*>(g.in) + off * es;
          char* d = static_cast<char*>(g.out) + off * es;
          for (int e = 0; e < es; e++) d[e] = s[e];
        }
      }
    }
    return;
  }

  const float* m = a.mapping + (a.mapping_batched ? b * 12 : 0);
  const float m00 = m[0], m01 = m[1], m02 = m[2], m03 = m[3];
  const float m10 = m[4], m11 = m[5], m12 = m[6], m13 = m[7];
  const float m20 = m[8], m21 = m[9], m22 = m[10], m23 = m[11];
  const float cj = static_cast<float>(jo), ck = static_cast<float>(ko);

  // k- and j-dependent control-grid lerp terms are loop invariants
  Lerp1D lj{0, 0, 1.0f, 0.0f}, lk{0, 0, 1.0f, 0.0f};
  int s_i = 0, s_j = 0;
  if constexpr (ELASTIC_POSSIBLE) {
    if (elastic) {
      lj = lerp_index(jo, a.nj, a.Jo, a.scale_j);
      lk = lerp_index(ko, a.nk, a.Ko, a.scale_k);
      s_i = a.nj * a.nk * 3;
      s_j = a.nk * 3;
    }
  }
  const int dJK = a.J * a.K, dK = a.K;
  const float hx = a.size_m1[0], hy = a.size_m1[1], hz = a.size_m1[2];

  for (int io = i_begin; io < i_end; io++) {
    const float ci = static_cast<float>(io);
    float vi, vj, vk;
    bool done = false;
    if constexpr (ELASTIC_POSSIBLE) {
      if (elastic) {
        const Lerp1D li = lerp_index(io, a.ni, a.Io, a.scale_i);
        const Disp d = cp_in_lds ? cp_trilerp3(s_cp, s_i, s_j, li, lj, lk) : cp_trilerp3(cp_global, s_i, s_j, li, lj, lk);
        float di = d.i, dj = d.j, dk = d.k;
        if (!a.unit_spacing) {  // mm → voxels: true division by the spacing
          di = exact_div(di, a.sp[0], a.rsp[0]);
          dj = exact_div(dj, a.sp[1], a.rsp[1]);
          dk = exact_div(dk, a.sp[2], a.rsp[2]);
        }
        if (a.affine_first) {  // spatial.py:1570-1573
          vi = __fadd_rn(TIO_AFFINE_ROW(m00, m01, m02, m03, ci, cj, ck), di);
          vj = __fadd_rn(TIO_AFFINE_ROW(m10, m11, m12, m13, ci, cj, ck), dj);
          vk = __fadd_rn(TIO_AFFINE_ROW(m20, m21, m22, m23, ci, cj, ck), dk);
        } else {  // spatial.py:1574-1577
          const float ei = __fadd_rn(ci, di), ej = __fadd_rn(cj, dj), ek = __fadd_rn(ck, dk);
          vi = TIO_AFFINE_ROW(m00, m01, m02, m03, ei, ej, ek);
          vj = TIO_AFFINE_ROW(m10, m11, m12, m13, ei, ej, ek);
          vk = TIO_AFFINE_ROW(m20, m21, m22, m23, ei, ej, ek);
        }
        done = true;
      }
    }
    if (!done) {  // spatial.py:1542-1543
      vi = TIO_AFFINE_ROW(m00, m01, m02, m03, ci, cj, ck);
      vj = TIO_AFFINE_ROW(m10, m11, m12, m13, ci, cj, ck);
      vk = TIO_AFFINE_ROW(m20, m21, m22, m23, ci, cj, ck);
    }
    if constexpr (MODE == 2) {  // grid_pull takes the voxel coordinates as they are (spatial.py:1749-1760)
      const int64_t o_idx = io * slab + row;
      for (int im = 0; im < a.n_images; im++) {
        const ImgArgs& g = a.img[im];
        for (int c = 0; c < g.channels; c++) {
          const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
          static_cast<float*>(g.out)[bc * n_out + o_idx] =
              spline_sample(static_cast<const float*>(g.in) + bc * n_in, a.I, a.J, a.K, vi, vj, vk, TIO_BSPLINE_ORDER(g.interp));
        }
      }
      continue;
    }
    // torchio axis i ≡ grid x ≡ ATen W ; j ≡ y ≡ H ; k ≡ z ≡ D
    const float x = normalise_roundtrip(vi, a.den[0], a.rden[0], hx);
    const float y = normalise_roundtrip(vj, a.den[1], a.rden[1], hy);
    const float z = normalise_roundtrip(vk, a.den[2], a.rden[2], hz);

    // ATen grid_sampler_3d corner weights (computed even for nearest data when a fill
    // mask is needed: the mask is always trilinear, spatial.py:1722-1727)
    const float x0 = floorf(x), y0 = floorf(y), z0 = floorf(z);
    const float x1 = x0 + 1.0f, y1 = y0 + 1.0f, z1 = z0 + 1.0f;
    float w[8];
    bool interior = true;
    if (a.any_linear) {
      const float wx0 = x1 - x, wx1 = x - x0;
      const float wy0 = y1 - y, wy1 = y - y0;
      const float wz0 = z1 - z, wz1 = z - z0;
      w[0] = __fmul_rn(__fmul_rn(wx0, wy0), wz0);
      w[1] = __fmul_rn(__fmul_rn(wx1, wy0), wz0);
      w[2] = __fmul_rn(__fmul_rn(wx0, wy1), wz0);
      w[3] = __fmul_rn(__fmul_rn(wx1, wy1), wz0);
      w[4] = __fmul_rn(__fmul_rn(wx0, wy0), wz1);
      w[5] = __fmul_rn(__fmul_rn(wx1, wy0), wz1);
      w[6] = __fmul_rn(__fmul_rn(wx0, wy1), wz1);
      w[7] = __fmul_rn(__fmul_rn(wx1, wy1), wz1);
      // x0 ∈ [0, S-2] ⇔ x0 and x1 both in bounds (integral floats; NaN fails)
      interior = (x0 >= 0.0f) & (x0 <= hx - 1.0f) & (y0 >= 0.0f) & (y0 <= hy - 1.0f) & (z0 >= 0.0f) & (z0 <= hz - 1.0f);
    }
    const int64_t o_idx = io * slab + row;
    if constexpr (LABEL_PV) {
      for (int im = 0; im < a.n_images; im++) {
        const ImgArgs& g = a.img[im];
        LabelSite site;
        site.in = g.in; site.out = g.out; site.labels = g.labels; site.pad_label = g.pad_label;
        site.in_base = static_cast<int64_t>(b) * n_in; site.out_index = static_cast<int64_t>(b) * n_out + o_idx;
        site.dtype = g.dtype; site.n_labels = g.n_labels; site.J = a.J; site.K = a.K;
        site.hx = hx; site.hy = hy; site.hz = hz;
        label_pv_voxel(site, x, y, z);
      }
      continue;
    }
    // nearest: nearbyint = round half to even (v_rndne_f32)
    const float xn = rintf(x), yn = rintf(y), zn = rintf(z);
    bool okn = true;
    if (a.any_nearest) {
      okn = (xn >= 0.0f) & (xn <= hx) & (yn >= 0.0f) & (yn <= hy) & (zn >= 0.0f) & (zn <= hz);
      interior = interior & okn;
    }

    if (__builtin_amdgcn_ballot_w64(!interior) == 0) {  // wave-uniform: whole wave interior
      const int base = (static_cast<int>(x0) * a.J + static_cast<int>(y0)) * a.K + static_cast<int>(z0);
      const int offn = (static_cast<int>(xn) * a.J + static_cast<int>(yn)) * a.K + static_cast<int>(zn);
      for (int im = 0; im < a.n_images; im++) {
        const ImgArgs& g = a.img[im];
#define TIO_CALL(DT) sample_interior<DT>(g, b, n_in, n_out, o_idx, w, base, dJK, dK, offn)
        TIO_DISPATCH_IMAGE(DTMODE, g.dtype, TIO_CALL)
#undef TIO_CALL
      }
    } else {
      const bool bx0 = (x0 >= 0.0f) & (x0 <= hx), bx1 = (x1 >= 0.0f) & (x1 <= hx);
      const bool by0 = (y0 >= 0.0f) & (y0 <= hy), by1 = (y1 >= 0.0f) & (y1 <= hy);
      const bool bz0 = (z0 >= 0.0f) & (z0 <= hz), bz1 = (z1 >= 0.0f) & (z1 <= hz);
      // clamp before the int conversion so that far-away coordinates stay defined
      const int ix0 = static_cast<int>(fminf(fmaxf(x0, 0.0f), hx)), ix1 = static_cast<int>(fminf(fmaxf(x1, 0.0f), hx));
      const int iy0 = static_cast<int>(fminf(fmaxf(y0, 0.0f), hy)), iy1 = static_cast<int>(fminf(fmaxf(y1, 0.0f), hy));
      const int iz0 = static_cast<int>(fminf(fmaxf(z0, 0.0f), hz)), iz1 = static_cast<int>(fminf(fmaxf(z1, 0.0f), hz));
      int off[8];
      unsigned okbits = 0;
      float mask = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const bool ok = ((k & 1) ? bx1 : bx0) & ((k & 2) ? by1 : by0) & ((k & 4) ? bz1 : bz0);
        off[k] = (((k & 1) ? ix1 : ix0) * a.J + ((k & 2) ? iy1 : iy0)) * a.K + ((k & 4) ? iz1 : iz0);
        okbits |= ok ? (1u << k) : 0u;
        if (a.any_linear) {
          const float next = __fadd_rn(mask, w[k]);  // same order as ATen's accumulation
          mask = ok ? next : mask;
        }
      }
      const int offn = (static_cast<int>(fminf(fmaxf(xn, 0.0f), hx)) * a.J + static_cast<int>(fminf(fmaxf(yn, 0.0f), hy))) * a.K +
                       static_cast<int>(fminf(fmaxf(zn, 0.0f), hz));
      for (int im = 0; im < a.n_images; im++) {
        const ImgArgs& g = a.img[im];
#define TIO_CALL(DT) sample_boundary<DT>(g, b, n_in, n_out, o_idx, w, off, okbits, mask, offn, okn)
        TIO_DISPATCH_IMAGE(DTMODE, g.dtype, TIO_CALL)
#undef TIO_CALL
      }
    }
  }
}

}  // namespace tio

#include "resample_exact_chain.hpp"
#include "resample_tile.hpp"
#include "resample_line.hpp"
#include "resample_plan.hpp"
#include "resample_fast.hpp"
#include "resample_lean_exact.hpp"
#include "resample_nearest.hpp"

// Device scratch for the brick plan of a planned launch (resample_plan.hpp): one buffer per (device, stream), grown on
// demand and kept.  A planned launch is a PAIR of kernels on the caller's stream — plan_bricks_kernel writes the buffer,
// the sampling kernel reads it — so the buffer is LEASED: the lease holds the slot's mutex from the lookup until both
// kernels are enqueued.  Two host threads that share a stream (the reference's Queue workers on the default stream,
// data/queue.py:119-123; ctypes drops the GIL around these calls) therefore enqueue planA, sampleA, planB, sampleB and
// never planA, planB, sampleA; the stream then orders the pairs on the device.  Growing (hipStreamSynchronize + hipFree +
// hipMalloc) also happens under the lease, i.e. while no other call holds a pointer it has not launched with yet.
namespace {
struct PlanSlot {
  int device;
  hipStream_t stream;
  int* ptr = nullptr;
  size_t cap = 0;
  std::mutex busy;
};
struct PlanLease {
  std::unique_lock<std::mutex> hold;
  int* ptr = nullptr;
};
}  // namespace

static PlanLease plan_workspace(hipStream_t s, size_t bytes) {
  static std::mutex registry_mu;
  static std::vector<PlanSlot*> registry;  // slots are never destroyed: their addresses (and mutexes) stay valid
  PlanLease lease;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return lease;
  PlanSlot* slot = nullptr;
  {
    std::lock_guard<std::mutex> lock(registry_mu);
    for (PlanSlot* sl : registry)
      if (sl->device == device && sl->stream == s) slot = sl;
    if (slot == nullptr) {
      slot = new PlanSlot();
      slot->device = device; slot->stream = s;
      registry.push_back(slot);
    }
  }
  lease.hold = std::unique_lock<std::mutex>(slot->busy);
  if (slot->cap < bytes) {
    if (slot->ptr != nullptr) {
      (void)hipStreamSynchronize(s);  // the previous (smaller) plan of this stream may still be read
      (void)hipFree(slot->ptr);
      slot->ptr = nullptr; slot->cap = 0;
    }
    if (hipMalloc(&slot->ptr, bytes) != hipSuccess) { slot->ptr = nullptr; return lease; }
    // (the first tio::kPlanHeaderInts ints: the multi-pass bricks' list header — zero between launches, see resample_lean_exact_kernel)
    if (hipMemsetAsync(slot->ptr, 0, tio::kPlanHeaderInts * sizeof(int), s) != hipSuccess) { (void)hipFree(slot->ptr); slot->ptr = nullptr; return lease; }
    slot->cap = bytes;
  }
  lease.ptr = slot->ptr;
  return lease;
}

// The dispatcher of tio_resample3d.  resample3d_impl (at the end) reads top to bottom: check_geometry, sort_images, the side groups (launch_nearest, launch_label_pv,
// launch_bspline), choose_float_road, that road's launcher.  choose_float_road makes no HIP call and is the only place where a switch or a threshold decides the float
// group's road; tio_resample3d_plan_bytes / tio_resample3d_plan ask it the same question for one aligned float32 image.
namespace {
using namespace tio;

using RowsKernel = void (*)(ResampleArgs);               // resample_kernel
using BrickKernel = void (*)(ResampleArgs, const int*);  // resample_tile_kernel, resample_planned_kernel
using LeanKernel = void (*)(LeanArgs);                   // resample_planned_lean_kernel, resample_lean_exact_*_kernel

// multiply-high reciprocal of a divisor (0: the divisor is 1, nothing to divide)
unsigned magic_u32(unsigned n) { return n > 1 ? 0xFFFFFFFFu / n + 1u : 0u; }

// tiles of ti x tj x tk output voxels: their counts per axis, the reciprocals, and one block per tile of every batch element
template <typename Args>
int set_tiles(Args& a, int ti, int tj, int tk, unsigned* blocks) {
  a.tiles_k = (a.Ko + tk - 1) / tk; a.tiles_j = (a.Jo + tj - 1) / tj; a.tiles_i = (a.Io + ti - 1) / ti;
  a.magic_k = magic_u32(a.tiles_k); a.magic_j = magic_u32(a.tiles_j); a.magic_i = magic_u32(a.tiles_i);
  const int64_t n = static_cast<int64_t>(a.B) * a.tiles_i * a.tiles_j * a.tiles_k;
  if (n >= (1LL << 31)) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: grid too large");
  *blocks = static_cast<unsigned>(n);
  return TIO_OK;
}

// more than 48 KiB of dynamic LDS have to be asked for, kernel by kernel
template <typename Kernel>
int reserve_lds(Kernel kernel, size_t bytes) {
  if (bytes > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes)) != hipSuccess)
    return fail(TIO_ERR_LAUNCH, "tio_resample3d: cannot reserve %zu bytes of LDS", bytes);
  return TIO_OK;
}

int control_floats(const ResampleArgs& a) { return a.cp != nullptr ? a.ni * a.nj * a.nk * 3 : 0; }
bool control_points_fit_lds(const ResampleArgs& a) { return control_floats(a) > 0 && control_floats(a) <= kMaxCpLds; }

// Where a planned road's plan lives: a plan made ahead by tio_resample3d_plan (geom->plan_dev: no planning kernel on this stream) or the stream's leased workspace.  The
// lease is held as long as this object lives: the launcher keeps it until the last kernel that reads the plan is enqueued.
struct Plan {
  PlanLease lease;
  int* ptr = nullptr;  // behind the header
  bool made_ahead = false;
};
int acquire_plan(const tio_resample_geom* geom, size_t need, hipStream_t s, Plan* plan) {
  if (geom->plan_dev != nullptr && geom->plan_bytes >= static_cast<int64_t>(need) && (reinterpret_cast<uintptr_t>(geom->plan_dev) & 15) == 0) {
    plan->ptr = static_cast<int*>(const_cast<void*>(geom->plan_dev)) + kPlanHeaderInts;
    plan->made_ahead = true;
    return TIO_OK;
  }
  plan->lease = plan_workspace(s, need);
  if (plan->lease.ptr == nullptr) return fail(TIO_ERR_LAUNCH, "tio_resample3d: cannot allocate the brick plan");
  plan->ptr = plan->lease.ptr + kPlanHeaderInts;
  return TIO_OK;
}

// plan_bricks_kernel for the 16^3 bricks of `a` (set_tiles and apply_road have run): plan_group lanes per brick
void enqueue_planner(const ResampleArgs& a, int* plan, int n_items, hipStream_t s) {
  const int plan_lanes = plan_group(a.cp != nullptr);
  const int plan_threads = n_items * plan_lanes > a.B ? n_items * plan_lanes : a.B;
  const dim3 plan_grid((plan_threads + 255) / 256);
  with_bools([&](auto elastic) { hipLaunchKernelGGL((plan_bricks_kernel<elastic.value, 16, 16, 16>), plan_grid, dim3(256), 0, s, a, plan, n_items); }, a.cp != nullptr);
}

// the 16^3 bricks of a planned road and their plan: the planner is enqueued unless the plan was made ahead
int plan_bricks(const tio_resample_geom* geom, ResampleArgs& a, size_t plan_need, hipStream_t s, Plan* plan, int* n_items) {
  unsigned bricks = 0;
  if (const int st = set_tiles(a, 16, 16, 16, &bricks)) return st;
  *n_items = static_cast<int>(bricks);  // (choose_float_road: below 2^26)
  if (const int st = acquire_plan(geom, plan_need, s, plan)) return st;
  if (!plan->made_ahead) enqueue_planner(a, plan->ptr, *n_items, s);
  return TIO_OK;
}

// The folded minimum of the planned FAST / lean roads: kMinSlots keys per channel that asked for it (common.hpp: min_workspace, all ones between launches; its own array,
// kind 1: tio_channel_min may be enqueued between a launch's kernels), finished by min_finish_kernel behind the sampling kernels.  Taken while the plan lease is held.
// channels == 0: nothing folds, and the images' out_min are cleared (tio_resample3d then runs the plain reduction).
struct FoldedMin {
  uint32_t* keys = nullptr;
  MinOuts outs{};
  int channels = 0;
};
int take_folded_min(ResampleArgs& a, bool allowed, hipStream_t s, FoldedMin* m) {
  for (int i = 0; i < a.n_images; i++) m->channels += a.img[i].out_min != nullptr ? a.img[i].channels : 0;
  if (m->channels == 0 || m->channels > kMinChannels || !allowed) {
    m->channels = 0;
    for (int i = 0; i < a.n_images; i++) a.img[i].out_min = nullptr;
    return TIO_OK;
  }
  int cap = 0;
  m->keys = min_workspace(s, m->channels * kMinSlots, &cap, /*kind=*/1);
  if (m->keys == nullptr) return fail(TIO_ERR_LAUNCH, "tio_resample3d: cannot allocate the reduction workspace");
  int slot = 0;
  for (int i = 0; i < a.n_images; i++)
    if (a.img[i].out_min != nullptr) {
      a.img[i].min_keys = m->keys + slot * kMinSlots;
      for (int c = 0; c < a.img[i].channels; c++) m->outs.p[slot + c] = a.img[i].out_min + c;
      slot += a.img[i].channels;
    }
  return TIO_OK;
}

void finish_folded_min(const FoldedMin& m, hipStream_t s) {
  if (m.channels > 0)
    hipLaunchKernelGGL(min_finish_kernel, dim3(static_cast<unsigned>(m.channels)), dim3(kMinSlots), 0, s, m.keys, m.outs, m.channels);
}

// fills the part of ResampleArgs that every group of images shares; an empty batch leaves a.B == 0 (nothing to do)
int check_geometry(const tio_resample_geom* geom, ResampleArgs& a) {
  if (geom->batch < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: negative batch");
  if (geom->batch == 0) return TIO_OK;  // an empty batch has no data pointers to speak of
  if (geom->mapping_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: mapping_dev is null");
  for (int d = 0; d < 3; d++) {
    if (geom->in_shape[d] < 1 || geom->out_shape[d] < 1)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: shapes must be >= 1");
  }
  const int64_t n_in = static_cast<int64_t>(geom->in_shape[0]) * geom->in_shape[1] * geom->in_shape[2];
  const int64_t n_out = static_cast<int64_t>(geom->out_shape[0]) * geom->out_shape[1] * geom->out_shape[2];
  if (n_in >= (1LL << 31) || n_out >= (1LL << 31))
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: more than 2^31 voxels per channel");
  if (geom->passthrough_dev != nullptr && n_in != n_out)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: passthrough needs in_shape == out_shape");
  if (geom->control_points_dev != nullptr) {
    for (int d = 0; d < 3; d++)
      if (geom->cp_shape[d] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: bad cp_shape");
  }

  a.B = geom->batch;
  a.I = geom->in_shape[0]; a.J = geom->in_shape[1]; a.K = geom->in_shape[2];
  a.Io = geom->out_shape[0]; a.Jo = geom->out_shape[1]; a.Ko = geom->out_shape[2];
  a.affine_first = geom->affine_first;
  a.mapping = geom->mapping_dev;
  a.mapping_batched = geom->mapping_batched;
  a.cp = geom->control_points_dev;
  a.cp_batched = geom->cp_batched;
  a.ni = geom->cp_shape[0]; a.nj = geom->cp_shape[1]; a.nk = geom->cp_shape[2];
  a.cp_skip = geom->cp_skip_dev;
  a.passthrough = geom->passthrough_dev;
  const float* sp = geom->affine_first ? geom->in_spacing : geom->out_spacing;
  a.unit_spacing = 1;
  a.short_div = 1;
  for (int d = 0; d < 3; d++) {
    a.sp[d] = sp[d];
    a.rsp[d] = 1.0f / sp[d];
    if (sp[d] != 1.0f) a.unit_spacing = 0;
    const int size = geom->in_shape[d];
    const int norm = geom->norm_shape[d] > 0 ? geom->norm_shape[d] : size;  // the grid's normalisation (first image's shape)
    a.den[d] = static_cast<float>(norm - 1 > 1 ? norm - 1 : 1);
    a.rden[d] = 1.0f / a.den[d];
    a.size_m1[d] = static_cast<float>(size - 1);
    a.dh[d] = 0.5f * a.den[d];
    a.rdh[d] = 1.0f / a.dh[d];
    a.half_h[d] = 0.5f * a.size_m1[d];
    if (a.den[d] > 8192.0f) a.short_div = 0;
    if (geom->norm_shape[d] < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: negative norm_shape");
  }
  if (a.cp != nullptr) {
    if (geom->control_points_dev != nullptr && !(sp[0] > 0.0f && sp[1] > 0.0f && sp[2] > 0.0f))
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: spacing must be positive");
    a.scale_i = lerp_scale(a.ni, a.Io);
    a.scale_j = lerp_scale(a.nj, a.Jo);
    a.scale_k = lerp_scale(a.nk, a.Ko);
  }
  return TIO_OK;
}

}  // namespace
namespace tio {
int resample_check_geometry(const tio_resample_geom* geom, ResampleArgs& a) { return check_geometry(geom, a); }
}  // namespace tio
namespace {

NearestArgs make_nearest_args(const ResampleArgs& a) {
  NearestArgs nn{};
  nn.B = a.B; nn.I = a.I; nn.J = a.J; nn.K = a.K; nn.Io = a.Io; nn.Jo = a.Jo; nn.Ko = a.Ko; nn.affine_first = a.affine_first;
  nn.mapping = a.mapping; nn.cp = a.cp; nn.cp_skip = a.cp_skip; nn.passthrough = a.passthrough;
  nn.mapping_batched = a.mapping_batched; nn.cp_batched = a.cp_batched; nn.ni = a.ni; nn.nj = a.nj; nn.nk = a.nk;
  nn.unit_spacing = a.unit_spacing;
  nn.scale_i = a.scale_i; nn.scale_j = a.scale_j; nn.scale_k = a.scale_k;
  for (int d = 0; d < 3; d++) {
    nn.sp[d] = a.sp[d]; nn.rsp[d] = a.rsp[d]; nn.den[d] = a.den[d]; nn.rden[d] = a.rden[d]; nn.size_m1[d] = a.size_m1[d];
    nn.ratio[d] = a.half_h[d] / a.dh[d];
    nn.dh[d] = a.dh[d]; nn.rdh[d] = a.rdh[d]; nn.half_h[d] = a.half_h[d];
  }
  return nn;
}

// what choose_float_road needs to know of the float group `a` beyond a.any_linear / a.any_nearest
struct FloatGroup {
  int dtmode = 0;            // 0: float32 images only, 1: small integers as well, 2: any dtype
  bool any_adjoint = false;  // a TIO_LINEAR_ADJOINT image (scatters to global memory)
  bool rows16 = true;        // every input starts on a 16-byte boundary
};
// a: everything that shares the brick / gather launch; pv: TIO_LABEL_PV images and spl: B-spline images (each their own launch of the gather kernel, same coordinates);
// nn: nearest images (label maps) for their own kernel (resample_nearest.hpp: bit-identical to the exact chain in every precision mode; TIO_NEAREST_KERNEL=0: they stay in `a`)
int sort_images(int32_t n_images, const tio_resample_image* images, const EnvSwitches& env, ResampleArgs& a, ResampleArgs& pv, ResampleArgs& spl, NearestArgs& nn,
                FloatGroup& group) {
  const bool nn_enabled = env.nearest_kernel != 0 && static_cast<int64_t>(a.I) * a.J <= (1LL << 24) && a.K < (1 << 24);
  for (int i = 0; i < n_images; i++) {
    const tio_resample_image& s = images[i];
    if (s.in == nullptr || s.out == nullptr || s.channels < 1)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: image %d has null data or no channels", i);
    if (!is_known_dtype(s.dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_resample3d: image %d dtype %d", i, s.dtype);
    if (s.interp != TIO_NEAREST && s.interp != TIO_LINEAR && s.interp != TIO_LABEL_PV && s.interp != TIO_LINEAR_ADJOINT &&
        TIO_BSPLINE_ORDER(s.interp) == 0)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: image %d interp %d", i, s.interp);
    if (TIO_BSPLINE_ORDER(s.interp) != 0) {
      if (s.dtype != TIO_F32)
        return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_resample3d: image %d: B-spline images hold float32 coefficients (tio_bspline_prefilter)", i);
      spl.img[spl.n_images++] = ImgArgs{s.in, s.out, nullptr, s.channels, s.dtype, s.interp, nullptr, 0, 0.0, nullptr, nullptr};
      continue;
    }
    if (s.interp == TIO_LINEAR_ADJOINT) {
      if (s.dtype != TIO_F32) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_resample3d: image %d: the adjoint works on float32 gradients", i);
      group.any_adjoint = true;
    }
    if (s.interp == TIO_LABEL_PV) {
      if (s.channels != 1)
        return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: image %d: TIO_LABEL_PV needs channels == 1, got %d", i, s.channels);
      if (s.n_labels < 0 || (s.n_labels > 0 && s.labels_dev == nullptr))
        return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: image %d: bad label table", i);
      pv.img[pv.n_images++] = ImgArgs{s.in, s.out, nullptr, 1, s.dtype, s.interp, s.labels_dev, s.n_labels, s.pad_label, nullptr, nullptr};
      continue;
    }
    if (nn_enabled && s.interp == TIO_NEAREST && s.out_min_dev == nullptr) {  // (with or without a fill rule)
      nn.img[nn.n_images++] = NearestImg{s.in, s.out, s.channels, dtype_size(s.dtype), s.fill_dev, s.dtype};
      if (s.fill_dev != nullptr) nn.any_fill = 1;
      continue;
    }
    a.img[a.n_images++] = ImgArgs{s.in, s.out, s.fill_dev, s.channels, s.dtype, s.interp, nullptr, 0, 0.0, s.out_min_dev, nullptr};
    // the in-bounds weight mask needs the trilinear weights even for nearest data (spatial.py:1722-1727)
    if (s.interp == TIO_LINEAR || s.interp == TIO_LINEAR_ADJOINT || s.fill_dev != nullptr) a.any_linear = 1;
    if (s.interp == TIO_NEAREST) a.any_nearest = 1;
    const int need = s.dtype == TIO_F32 ? 0 : ((s.dtype == TIO_I16 || s.dtype == TIO_U8 || s.dtype == TIO_I32) ? 1 : 2);
    group.dtmode = need > group.dtmode ? need : group.dtmode;
    group.rows16 = group.rows16 && (reinterpret_cast<uintptr_t>(s.in) & 15) == 0;
  }
  return TIO_OK;
}

// ---- the road of the float group: which one is taken when, and the kernels behind each, is the table of DESIGN.md 4.1 ----
enum FloatRoadKind { kRoadGather, kRoadBrick, kRoadPlannedBrick, kRoadFastBrick, kRoadPlannedFast, kRoadPlannedLean, kRoadLeanExact };

struct FloatRoad {
  FloatRoadKind kind = kRoadGather;
  bool exact_lerp = false;  // lean exact: ATen's interpolation order (bit-identical to the brick kernel) instead of TIGHT's fused lerps
  int64_t bricks = 0;       // 16^3 bricks of the launch (planned roads: the plan's items)
  size_t lds = 0;           // dynamic LDS of the sampling kernel, bytes
  size_t plan_need = 0;     // bytes of the plan the road starts from (0: it does not)
  int cp_lds = 0, tile_cap = 0, fill_recheck = 0, plan_multi = 0;  // what apply_road copies into ResampleArgs
  int ablate = 0;  // TIO_TILE_ABLATE: the planned lean kernel's instrumented instantiation (the exact roads stay away from it)
  int interleave = 0, pair = 0;  // launch_lean: TIO_LEAN_INTERLEAVE, TIO_LEAN_PAIR (A/B)
};
FloatRoad choose_float_road(const tio_resample_geom& geom, const ResampleArgs& a, const FloatGroup& g, const EnvSwitches& env) {
  FloatRoad r;
  // LDS-staged bricks whenever a trilinear image is present (the 8-tap gather is what the staging removes); pure nearest launches keep the one-load gather kernel.
  // TIO_RESAMPLE_PATH=gather|tile overrides (A/B tests compare the two bit for bit).
  bool use_tile = a.any_linear != 0;
  if (env.resample_path == 1) use_tile = false;
  if (env.resample_path == 2) use_tile = true;
  if (g.any_adjoint) use_tile = false;  // the adjoint scatters to global memory: gather kernel
  if (static_cast<int64_t>(a.Jo) * a.Ko * 8 >= (1LL << 31)) use_tile = false;  // 32-bit byte offsets inside one output plane
  if (static_cast<int64_t>(a.I) * a.J * a.K >= (1LL << 30)) use_tile = false;  // 32-bit byte offsets inside one input channel (f32 brick DMA)
  if (!use_tile) return r;
  r.kind = kRoadBrick;
  r.ablate = env.tile_ablate;
  r.fill_recheck = env.fast_fill_recheck;
  r.cp_lds = control_points_fit_lds(a) ? ((control_floats(a) + 3) & ~3) : 0;
  // default brick budget: whatever lets kTileBlocksPerCU blocks share the CU's 160 KiB (minus 2 KiB: LDS is allocated in granules, an exact third does not fit three times)
  const int cap = kLdsFloatsPerCU / kTileBlocksPerCU - 512 - r.cp_lds - kTileRedInts;
  const int max_cap = kLdsFloatsPerCU - r.cp_lds - kTileRedInts;
  r.tile_cap = cap < kTileMinCap ? kTileMinCap : (cap > max_cap ? max_cap : cap);
  r.lds = static_cast<size_t>(r.cp_lds + kTileRedInts + r.tile_cap) * sizeof(float);
  r.bricks = static_cast<int64_t>(a.B) * ((a.Io + 15) / 16) * ((a.Jo + 15) / 16) * ((a.Ko + 15) / 16);
  const size_t plan_plain = static_cast<size_t>(a.B) * 16 + static_cast<size_t>(r.bricks) * kDescInts;  // (ints behind the header)
  // fast intensity path: float32 trilinear images only (nearest / label images need the exact coordinates)
  const bool fast = geom.precision == TIO_PRECISION_FAST && g.dtmode == 0 && !a.any_nearest && !env.resample_exact;
  // The lean planned kernel with the reference's own coordinates (resample_lean_exact.hpp).  TIO_PRECISION_TIGHT: fused interpolation on exact coordinates / taps / fill
  // decisions; TIO_PRECISION_EXACT: ATen's interpolation order too, bit-identical to the brick kernel (TIO_EXACT_LEAN=0 keeps large exact launches on the brick kernel, =2
  // sends small ones to the lean kernel as well: A/B and tests).  Float32 trilinear images only, divisors the short division is proven for, unit spacing whenever a
  // displacement is divided by it; everything else runs the exact brick kernel.
  const bool tight = geom.precision == TIO_PRECISION_TIGHT && !env.resample_exact;  // (TIO_RESAMPLE_EXACT: the A/B switch forces ATen's interpolation order too)
  const bool lean_exact = !fast && (tight || ((geom.precision == TIO_PRECISION_EXACT || geom.precision == TIO_PRECISION_TIGHT) && env.exact_lean != 0)) &&
                          g.dtmode == 0 && !a.any_nearest && r.ablate == 0 && a.short_div != 0 && (a.cp == nullptr || a.unit_spacing != 0);
  if (fast || lean_exact) {
    // Planned bricks (resample_plan.hpp): a planning kernel, then one block per brick that starts from its 64-byte descriptor. Needs 16-byte rows for the LDS-DMA and
    // control cells at least a brick wide (the box comes from <= 27 vertices); small launches keep the single-kernel road (the planning kernel and the gap before the
    // second launch cost ~10-15 us, more than the planned bricks save below ~12 k bricks).  TIO_FAST_KERNEL=planned forces them, =brick keeps FAST launches off them (A/B).
    const bool force_planned = lean_exact ? (env.fast_kernel == 2 || env.exact_lean == 2) : env.fast_kernel == 2;
    bool planned = (lean_exact || env.fast_kernel != 1) && (a.K & 3) == 0 && (r.bricks >= kPlannedMinBricks || force_planned) && r.bricks < (1LL << 26) && g.rows16;
    // the caller expects boxes beyond the staging tile (tio_hip.h: TIO_GEOM_LARGE_BOXES): a planned FAST brick whose box does not fit samples voxel by voxel, the brick
    // kernel splits it into passes over its planes — the hint sends FAST launches there; the lean exact road stages such bricks in passes itself (plan_multi) and stays
    if ((geom.flags & (TIO_GEOM_LARGE_BOXES | TIO_GEOM_MOSTLY_LARGE_BOXES)) != 0 && !force_planned && !lean_exact) planned = false;
    if (planned && a.cp != nullptr) {
      const int n_ctl[3] = {a.ni, a.nj, a.nk}, n_vox[3] = {a.Io, a.Jo, a.Ko};
      for (int d = 0; d < 3; d++)
        if (n_ctl[d] > 2 && (n_vox[d] - 1) < 16 * (n_ctl[d] - 1)) planned = false;
    }
    if (planned) {
      r.kind = lean_exact ? kRoadLeanExact : (env.planned_lean != 0 ? kRoadPlannedLean : kRoadPlannedFast);
      r.exact_lerp = !tight;
      // the largest tile three blocks of which fit a CU: LDS is handed out in granules of 1 280 bytes here (measured: 13 440 floats keep three blocks resident, 13 568 drop
      // to two — profiles/r04_tile_cap.log)
      const int cap_p = (kLdsFloatsPerCU / kTileBlocksPerCU) / 320 * 320;
      r.tile_cap = cap_p < kTileMinCap ? kTileMinCap : (cap_p > kLdsFloatsPerCU ? kLdsFloatsPerCU : cap_p);
      r.cp_lds = 0;
      r.lds = static_cast<size_t>(r.tile_cap) * sizeof(float);
      r.interleave = env.lean_interleave;
      r.pair = env.lean_pair;
      // the exact-coordinate kernel stages bricks whose box exceeds the tile in passes over their planes (pass boxes behind the descriptors) — on the hint of a caller who
      // holds the mappings: TIO_GEOM_LARGE_BOXES, plan_multi = 1, a second kernel BEHIND the first walks the planner's list of such bricks (~6 - 15 us that a launch
      // without such bricks should not pay: profiles/r06_resample.md); TIO_GEOM_MOSTLY_LARGE_BOXES, plan_multi = 2: every block of ONE launch runs the body with the pass
      // switches, nothing is listed.  Without the hint such bricks sample voxel by voxel.
      if (lean_exact && env.lean_multi != 0)
        r.plan_multi = (geom.flags & TIO_GEOM_MOSTLY_LARGE_BOXES) != 0 ? 2 : ((geom.flags & TIO_GEOM_LARGE_BOXES) != 0 ? 1 : 0);
      // [header: kPlanHeaderInts ints] [B x 16 floats] [bricks x descriptors] ( [bricks x 4 pass boxes] [the list of multi-pass bricks] )
      const size_t n = static_cast<size_t>(r.bricks);
      const size_t plan_multi_ints = static_cast<size_t>(a.B) * 16 + n * (kDescInts + kPassInts * kPassesPerBrick) + ((n + 3) & ~static_cast<size_t>(3));
      r.plan_need = (kPlanHeaderInts + (r.plan_multi ? plan_multi_ints : plan_plain)) * sizeof(int);
      return r;
    }
    // (a TIGHT / EXACT launch the lean kernel does not take — too small, unaligned — goes on to the exact brick kernel)
    if (fast) {
      r.kind = kRoadFastBrick;  // the brick kernel's FAST instantiation with its in-kernel boxes
      return r;
    }
  }
  // Large affine-only exact launches of 16^3 bricks are planned too (resample_tile.hpp: the planned box only decides what is staged); TIO_EXACT_PLAN=0 switches it off, =2
  // forces it for small launches (A/B, tests).  Measured (8 x 256^3): affine 0.497 -> 0.478 ms; elastic launches LOSE (0.588 -> 0.610: 27 vertices with their control-point
  // reads per brick cost the planner more than the brick kernel's own reduction), and so do small ones.
  if (r.ablate == 0 && a.cp == nullptr && env.exact_plan != 0 && (r.bricks >= kPlannedMinBricks || env.exact_plan == 2) && r.bricks < (1LL << 26)) {
    r.kind = kRoadPlannedBrick;
    // (every plan starts behind kPlanHeaderInts ints: the list header of the lean exact road, which shares the stream's leased workspace and must find it zero)
    r.plan_need = (kPlanHeaderInts + plan_plain) * sizeof(int);
  }
  return r;
}

void apply_road(ResampleArgs& a, const FloatRoad& r) {
  a.fill_recheck = r.fill_recheck; a.cp_lds = r.cp_lds; a.tile_cap = r.tile_cap;
  a.plan_multi = r.plan_multi;
  for (int i = 0; i < a.n_images && r.kind != kRoadGather; i++) a.any_fill |= a.img[i].fill != nullptr ? 1 : 0;
}

LeanArgs make_lean_args(const ResampleArgs& a, const FloatRoad& r, const int* plan, int n_items) {
  LeanArgs la{};
  la.plan = plan; la.cp = a.cp;
  la.I = a.I; la.J = a.J; la.K = a.K; la.Io = a.Io; la.Jo = a.Jo; la.Ko = a.Ko;
  la.B = a.B; la.n_items = n_items;
  la.bricks_per_element = static_cast<unsigned>(a.tiles_i) * a.tiles_j * a.tiles_k;
  la.bpe_magic = magic_u32(la.bricks_per_element);
  la.ni = a.ni; la.nj = a.nj; la.nk = a.nk; la.cp_batched = a.cp_batched;
  la.sci = a.scale_i; la.scj = a.scale_j; la.sck = a.scale_k;
  for (int e = 0; e < 3; e++) la.dsc[e] = a.rsp[e] * (a.affine_first ? a.half_h[e] / a.dh[e] : 1.0f);
  la.hx = a.size_m1[0]; la.hy = a.size_m1[1]; la.hz = a.size_m1[2];
  la.affine_first = a.affine_first; la.ablate = r.ablate;
  la.mapping = a.mapping; la.mapping_batched = a.mapping_batched; la.unit_spacing = a.unit_spacing; la.fill_recheck = a.fill_recheck;
  for (int e = 0; e < 3; e++) { la.sp[e] = a.sp[e]; la.rsp[e] = a.rsp[e]; la.den[e] = a.den[e]; la.rden[e] = a.rden[e]; }
  for (int e = 0; e < 3; e++) { la.dh[e] = a.dh[e]; la.rdh[e] = a.rdh[e]; la.half_h[e] = a.half_h[e]; }
  la.interleave = r.interleave;
  la.tile_floats = r.tile_cap;
  return la;
}

// The label channel that may ride along the float images' last exact-coordinate launch (resample_lean_exact_label_kernel) instead of taking its own kernel.  es != 0: its
// launch is pending — launch_lean takes it when its conditions hold (es = 0), otherwise resample3d_impl launches it before it returns, whatever road the images took.
struct LabelRide {
  int es = 0;  // element size of the pending label channel (0: none)
  unsigned blocks = 0, lds = 0;
};
int launch_nearest_exact(const NearestArgs& nn, int es, unsigned blocks, unsigned lds, hipStream_t s) {
  const bool known = dispatch_element_size(es, [&](auto size) {
    with_bools([&](auto elastic) { hipLaunchKernelGGL((resample_nearest_exact_kernel<elastic.value, size.value>), dim3(blocks), dim3(256), lds, s, nn); }, nn.cp != nullptr);
  });
  return known ? TIO_OK : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_resample3d: label elements of %d bytes", es);
}

// nearest images (label maps): one launch per element size present.  `short_div`: the float group's gate of the exact coordinates; `floats_alone`: float images follow and
// nothing else does (the label channel may ride with them)
int launch_nearest(NearestArgs& nn, bool short_div, bool floats_alone, const EnvSwitches& env, hipStream_t s, LabelRide* label) {
  const bool rows = nn.Ko >= 48;  // bricks of 16 x 4 x 64 (a wave = one output row) unless the volume is narrower than that
  unsigned blocks = 0;
  if (const int st = set_tiles(nn, 16, rows ? 4 : 16, rows ? 64 : 16, &blocks)) return st;
  nn.eps = env.has_nearest_eps ? env.nearest_eps : kNearestEps;  // (TIO_NEAREST_EPS: calibration runs only)
  // without a fill rule the reference's own coordinates plane by plane (resample_nearest_exact_kernel; its gate is the float exact-coordinate kernel's: the short division,
  // unit spacing under control points, rows of at least 48 voxels)
  const bool exact = env.nearest_exact != 0 && nn.any_fill == 0 && rows && short_div && (nn.cp == nullptr || nn.unit_spacing != 0);
  // resident blocks per CU through UNUSED dynamic LDS: without control points the kernel holds 61 registers (eight blocks per CU), and eight blocks' slanted input
  // footprints evict one another's cache lines — three blocks per CU measured 0.236 -> 0.210 ms (int16) and 0.344 -> 0.286 (int32) on 8 x 256^3 at the bench's ranges, uint8
  // 0.172 -> 0.177; with control points (95 registers, five blocks) the launch is arithmetic bound and loses from four blocks down (profiles/r06_labels.md)
  const unsigned exact_lds = nn.cp == nullptr ? 52000u : 0u;
  for (int es = 1; es <= 8; es *= 2) {
    bool present = false;
    for (int i = 0; i < nn.n_images; i++) present = present || nn.img[i].es == es;
    if (!present) continue;
    // ... and its tail's: 24-bit offsets and buffer loads (I J <= 2^24, every channel below 2^32 bytes)
    const int64_t n_in = static_cast<int64_t>(nn.I) * nn.J * nn.K, n_out = static_cast<int64_t>(nn.Io) * nn.Jo * nn.Ko;
    const bool narrow = static_cast<int64_t>(nn.I) * nn.J <= (1 << 24) && static_cast<int64_t>(nn.K) * es < (1 << 24) &&
                        n_in * es < (int64_t{1} << 32) - 16 && n_out * es < (int64_t{1} << 32) - 16;
    if (exact && narrow && env.lean_label != 0 && nn.n_images == 1 && nn.img[0].channels == 1 && es <= 4 && floats_alone) {
      label->es = es; label->blocks = blocks; label->lds = exact_lds;  // ONE plain label channel beside float images: it may ride
    } else if (exact && narrow) {
      if (const int st = launch_nearest_exact(nn, es, blocks, exact_lds, s)) return st;
    } else {
      const bool known = dispatch_element_size(es, [&](auto size) {
        with_bools([&](auto elastic, auto wave_rows) {
          hipLaunchKernelGGL((resample_nearest_kernel<elastic.value, size.value, wave_rows.value ? 4 : 16, wave_rows.value ? 64 : 16, 16>), dim3(blocks), dim3(256), 0, s, nn);
        }, nn.cp != nullptr, rows);
      });
      if (!known) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_resample3d: label elements of %d bytes", es);
    }
  }
  return TIO_OK;
}

// the per-voxel gather kernel: a block walks kTileI output slabs of kRowsPerBlock rows of kLanes voxels, control points in LDS if they fit
int launch_rows(RowsKernel kernel, ResampleArgs& a, hipStream_t s) {
  unsigned blocks = 0;
  if (const int st = set_tiles(a, kTileI, kRowsPerBlock, kLanes, &blocks)) return st;
  const size_t lds = control_points_fit_lds(a) ? static_cast<size_t>(control_floats(a)) * sizeof(float) : 0;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kRowsPerBlock * kLanes), lds, s, a);
  return TIO_OK;
}

int launch_label_pv(ResampleArgs& pv, hipStream_t s) {
  return launch_rows(with_bools([](auto elastic) -> RowsKernel { return resample_kernel<elastic.value, 2, 1>; }, pv.cp != nullptr), pv, s);
}
int launch_bspline(ResampleArgs& spl, hipStream_t s) {
  return launch_rows(with_bools([](auto elastic) -> RowsKernel { return resample_kernel<elastic.value, 0, 2>; }, spl.cp != nullptr), spl, s);
}

int launch_gather(ResampleArgs& a, int dtmode, hipStream_t s) {
  const RowsKernel kernel = with_bools([&](auto e) -> RowsKernel {
    return dtmode == 0 ? resample_kernel<e.value, 0> : (dtmode == 1 ? resample_kernel<e.value, 1> : resample_kernel<e.value, 2>);
  }, a.cp != nullptr);
  const int status = launch_rows(kernel, a, s);
  return status != TIO_OK ? status : check_launch("tio_resample3d");
}

// one block of 256 threads per 16 x 16 x 16 brick, from a plan or (nullptr) with in-kernel boxes
int launch_brick_kernel(BrickKernel kernel, ResampleArgs& a, size_t lds, const int* plan, hipStream_t s) {
  unsigned blocks = 0;
  if (const int st = set_tiles(a, 16, 16, 16, &blocks)) return st;
  if (const int st = reserve_lds(kernel, lds)) return st;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds, s, a, plan);
  return check_launch("tio_resample3d");
}

// the brick kernel (three blocks per CU) in the instantiation of the launch's element types
int launch_brick_dtmode(ResampleArgs& a, int dtmode, size_t lds, const int* plan, hipStream_t s) {
  const BrickKernel kernel = with_bools([&](auto elastic) -> BrickKernel {
    if (dtmode == 1) return resample_tile_kernel<elastic.value, 1, 16, 16, 16, 3>;
    if (dtmode != 0) return resample_tile_kernel<elastic.value, 2, 16, 16, 16, 3>;
    return resample_tile_kernel<elastic.value, 0, 16, 16, 16, 3>;
  }, a.cp != nullptr);
  return launch_brick_kernel(kernel, a, lds, plan, s);
}

// brick, planned brick and FAST brick: resample_tile_kernel
int launch_brick(const tio_resample_geom* geom, ResampleArgs& a, const FloatRoad& r, int dtmode, hipStream_t s) {
  if (r.kind == kRoadFastBrick) {
    const BrickKernel kernel = with_bools([](auto elastic) -> BrickKernel { return resample_tile_kernel<elastic.value, 0, 16, 16, 16, 3, true>; }, a.cp != nullptr);
    return launch_brick_kernel(kernel, a, r.lds, nullptr, s);
  }
  Plan plan;  // (a lease is held until the brick kernel is enqueued)
  if (r.kind == kRoadPlannedBrick) {
    int n_items = 0;
    if (const int st = plan_bricks(geom, a, r.plan_need, s, &plan, &n_items)) return st;
  }
  return launch_brick_dtmode(a, dtmode, r.lds, plan.ptr, s);
}

// planned FAST (TIO_PLANNED_LEAN=0): one launch of resample_planned_kernel for all images and channels
int launch_planned_fast(const tio_resample_geom* geom, ResampleArgs& a, const FloatRoad& r, bool may_fold, hipStream_t s, bool* folded) {
  Plan plan;
  int n_items = 0;
  if (const int st = plan_bricks(geom, a, r.plan_need, s, &plan, &n_items)) return st;
  FoldedMin fm;
  if (const int st = take_folded_min(a, may_fold, s, &fm)) return st;
  *folded = fm.channels > 0;
  const BrickKernel kernel = with_bools([](auto elastic) -> BrickKernel { return resample_planned_kernel<elastic.value, 16, 16, 16, 3>; }, a.cp != nullptr);
  if (const int st = reserve_lds(kernel, r.lds)) return st;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(n_items)), dim3(256), r.lds, s, a, static_cast<const int*>(plan.ptr));
  finish_folded_min(fm, s);
  return check_launch("tio_resample3d");
}

// la.in / out / fill / strides (SECOND: the pair kernels' second channel) for channel c of image g
template <bool SECOND>
void set_lean_channel(LeanArgs& la, const ImgArgs& g, int c) {
  const int64_t n_in = static_cast<int64_t>(la.I) * la.J * la.K, n_out = static_cast<int64_t>(la.Io) * la.Jo * la.Ko;
  const float *in = static_cast<const float*>(g.in) + c * n_in, *fill = g.fill != nullptr ? g.fill + c : nullptr;
  float* out = static_cast<float*>(g.out) + c * n_out;
  const int64_t in_stride = g.channels * n_in, out_stride = g.channels * n_out;
  if constexpr (SECOND) { la.in2 = in; la.out2 = out; la.fill2 = fill; la.in_stride2 = in_stride; la.out_stride2 = out_stride; }
  else { la.in = in; la.out = out; la.fill = fill; la.in_stride = in_stride; la.out_stride = out_stride; }
}

// Planned lean (FAST coordinates) and lean exact (the reference's): one plan, one launch per channel of every image.  Lean exact without multi-pass bricks and without a
// folded minimum samples two channels per launch (resample_lean_exact_pair_kernel: one descriptor round trip, one set of control planes, ONE coordinate chain for both —
// a subject's float32 images share their geometry; an odd channel out goes alone) and takes the call's pending label channel along with the last of them
// (resample_lean_exact_label_kernel).  TIO_LEAN_PAIR=0: one launch per channel, TIO_LEAN_LABEL=0: the label map's own kernel (A/B)
int launch_lean(const tio_resample_geom* geom, ResampleArgs& a, const FloatRoad& r, bool may_fold, const NearestArgs& nn, LabelRide* label, hipStream_t s, bool* folded) {
  Plan plan;  // (a lease is held until the last launch is enqueued)
  int n_items = 0, channels = 0;
  if (const int st = plan_bricks(geom, a, r.plan_need, s, &plan, &n_items)) return st;
  FoldedMin fm;
  if (const int st = take_folded_min(a, may_fold, s, &fm)) return st;
  *folded = fm.channels > 0;
  const bool elastic = a.cp != nullptr, lean_exact = r.kind == kRoadLeanExact, fold = fm.channels > 0;
  const dim3 grid(static_cast<unsigned>(n_items)), grid_multi(static_cast<unsigned>(std::min<int64_t>(n_items, 3 * 256))), block(256);
  LeanArgs la = make_lean_args(a, r, plan.ptr, n_items);
  for (int i = 0; i < a.n_images; i++) channels += a.img[i].channels;
  LeanKernel kernel;
  if (lean_exact && a.plan_multi == 2)  // most bricks need passes: ONE launch of the body that knows them
    kernel = with_bools([](auto e, auto x, auto f) -> LeanKernel { return resample_lean_exact_all_kernel<e.value, x.value, f.value>; }, elastic, r.exact_lerp, fold);
  else if (lean_exact)
    kernel = with_bools([](auto e, auto x, auto f) -> LeanKernel { return resample_lean_exact_kernel<e.value, x.value, 3, f.value>; }, elastic, r.exact_lerp, fold);
  else if (r.ablate != 0)  // TIO_TILE_ABLATE: the instrumented instantiation (experiments only)
    kernel = with_bools([](auto e) -> LeanKernel { return resample_planned_lean_kernel<e.value, 16, 16, 16, 3, true>; }, elastic);
  else  // (the folded minimum: the instantiation whose element-0 bricks track what they store)
    kernel = with_bools([](auto e, auto f) -> LeanKernel { return resample_planned_lean_kernel<e.value, 16, 16, 16, 3, false, f.value>; }, elastic, fold);
  if (const int st = reserve_lds(kernel, r.lds)) return st;
  // plan_multi == 1: behind every launch, the kernel whose blocks walk the planner's list of multi-pass bricks — three per CU, leaving at once when the list is empty
  LeanKernel kernel_multi = nullptr, kernel_pair = nullptr, kernel_label_pair = nullptr, kernel_label_one = nullptr;
  if (a.plan_multi == 1) {
    kernel_multi = with_bools([](auto e, auto x, auto f) -> LeanKernel { return resample_lean_exact_multi_kernel<e.value, x.value, f.value>; }, elastic, r.exact_lerp, fold);
    if (const int st = reserve_lds(kernel_multi, r.lds)) return st;
  }
  const bool plain = lean_exact && a.plan_multi == 0 && !fold;
  const bool pairs = plain && channels >= 2 && r.pair != 0, label_here = plain && label->es != 0 && a.passthrough == nn.passthrough;
  if (pairs || label_here) {
    kernel_pair = with_bools([](auto e, auto x) -> LeanKernel { return resample_lean_exact_pair_kernel<e.value, x.value>; }, elastic, r.exact_lerp);
    if (const int st = reserve_lds(kernel_pair, r.lds)) return st;
  }
  if (label_here) {
    kernel_label_pair = with_bools([](auto e, auto x) -> LeanKernel { return resample_lean_exact_label_kernel<e.value, x.value, true>; }, elastic, r.exact_lerp);
    kernel_label_one = with_bools([](auto e, auto x) -> LeanKernel { return resample_lean_exact_label_kernel<e.value, x.value, false>; }, elastic, r.exact_lerp);
    if (const int st = reserve_lds(kernel_label_pair, r.lds)) return st;
    if (const int st = reserve_lds(kernel_label_one, r.lds)) return st;
    la.lab_in = nn.img[0].in; la.lab_out = nn.img[0].out; la.lab_es = label->es;
  }
  int launches_left = channels;
  bool have_first = false;
  for (int i = 0; i < a.n_images; i++) {
    const ImgArgs& g = a.img[i];
    for (int c = 0; c < g.channels; c++) {
      --launches_left;
      if (pairs && !have_first && launches_left > 0) {  // the first of two (an odd channel out is launched alone, below)
        set_lean_channel<false>(la, g, c);
        have_first = true;
        continue;
      }
      la.last_use = !plan.made_ahead && launches_left == 0;  // (only the leased workspace is left zeroed, and only by the call's last launch)
      la.min_keys = (fold && g.min_keys != nullptr) ? g.min_keys + c * kMinSlots : nullptr;
      const bool with_label = label_here && launches_left == 0;
      if (have_first) set_lean_channel<true>(la, g, c);
      else set_lean_channel<false>(la, g, c);
      const LeanKernel launch = have_first ? (with_label ? kernel_label_pair : kernel_pair) : (with_label ? kernel_label_one : kernel);
      have_first = false;
      hipLaunchKernelGGL(launch, grid, block, r.lds, s, la);
      if (kernel_multi != nullptr) hipLaunchKernelGGL(kernel_multi, grid_multi, block, r.lds, s, la);
    }
  }
  finish_folded_min(fm, s);
  if (label_here) label->es = 0;  // (taken along)
  return check_launch("tio_resample3d");
}

// `folded` comes back true when the launch itself produced every requested out_min_dev (planned FAST / lean bricks)
int resample3d_impl(const tio_resample_geom* geom, int32_t n_images, const tio_resample_image* images, void* stream, bool* folded) {
  *folded = false;
  if (geom == nullptr || images == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: null argument");
  if (n_images < 1 || n_images > TIO_MAX_IMAGES)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d: n_images=%d not in [1, %d]", n_images, TIO_MAX_IMAGES);
  ResampleArgs a{};
  int status = check_geometry(geom, a);
  if (status != TIO_OK || a.B == 0) return status;
  ResampleArgs pv = a, spl = a;
  pv.any_linear = 1;
  NearestArgs nn = make_nearest_args(a);
  FloatGroup group;
  const EnvSwitches& env = env_switches();  // (parsed once per process / tio_reload_env(): no getenv on this road)
  if ((status = sort_images(n_images, images, env, a, pv, spl, nn, group)) != TIO_OK) return status;

  hipStream_t s = static_cast<hipStream_t>(stream);
  LabelRide label;
  if (nn.n_images > 0) {
    const bool floats_alone = a.n_images > 0 && pv.n_images == 0 && spl.n_images == 0 && !group.any_adjoint;
    if ((status = launch_nearest(nn, a.short_div != 0, floats_alone, env, s, &label)) != TIO_OK) return status;
    if (a.n_images == 0 && pv.n_images == 0 && spl.n_images == 0) return check_launch("tio_resample3d");
  }
  if (pv.n_images > 0) {
    if ((status = launch_label_pv(pv, s)) != TIO_OK) return status;
    if (a.n_images == 0 && spl.n_images == 0) return check_launch("tio_resample3d");
  }
  if (spl.n_images > 0) {
    if ((status = launch_bspline(spl, s)) != TIO_OK) return status;
    if (a.n_images == 0) return check_launch("tio_resample3d");
  }

  const FloatRoad road = choose_float_road(*geom, a, group, env);
  apply_road(a, road);
  switch (road.kind) {
    case kRoadGather: status = launch_gather(a, group.dtmode, s); break;
    case kRoadBrick: case kRoadPlannedBrick: case kRoadFastBrick: status = launch_brick(geom, a, road, group.dtmode, s); break;
    case kRoadPlannedFast: status = launch_planned_fast(geom, a, road, pv.n_images == 0, s, folded); break;
    case kRoadPlannedLean: case kRoadLeanExact: status = launch_lean(geom, a, road, pv.n_images == 0, nn, &label, s, folded); break;
  }
  // a label channel nobody took along: its own launch, behind the float images' kernels — also where their road failed
  // (the images' status is already decided: a failure of this launch is not reported)
  if (label.es != 0) launch_nearest_exact(nn, label.es, label.blocks, label.lds, s);
  return status;
}

// the plan entry points choose for one float32 trilinear image whose rows are 16-byte aligned (the planner never reads an image)
int choose_plan_road(const tio_resample_geom* geom, ResampleArgs* a, FloatRoad* road) {
  const int status = check_geometry(geom, *a);
  if (status != TIO_OK) return status;
  a->any_linear = 1;
  *road = choose_float_road(*geom, *a, FloatGroup{}, env_switches());
  return TIO_OK;
}

}  // namespace

extern "C" int64_t tio_resample3d_plan_bytes(const tio_resample_geom* geom) {
  if (geom == nullptr || geom->batch < 1) return 0;
  ResampleArgs a{};
  FloatRoad road;
  return choose_plan_road(geom, &a, &road) == TIO_OK ? static_cast<int64_t>(road.plan_need) : 0;
}

extern "C" int tio_resample3d_plan(const tio_resample_geom* geom, void* plan_dev, int64_t plan_bytes, void* stream) {
  if (geom == nullptr || geom->batch < 1) return tio::fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_plan: no geometry / empty batch");
  ResampleArgs a{};
  FloatRoad road;
  if (const int st = choose_plan_road(geom, &a, &road)) return st;
  if (road.plan_need == 0) return tio::fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_plan: this geometry's launch does not start from a plan");
  if (plan_dev == nullptr || plan_bytes < static_cast<int64_t>(road.plan_need) || (reinterpret_cast<uintptr_t>(plan_dev) & 15) != 0)
    return tio::fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_plan: the plan needs %zu bytes, 16-byte aligned", road.plan_need);
  apply_road(a, road);
  unsigned bricks = 0;
  if (const int st = set_tiles(a, 16, 16, 16, &bricks)) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // The header of the multi-pass bricks' list (length, cursor, done count) is zero between launches: the leased workspace is zeroed when it is allocated and the last
  // walker of a call's last launch leaves zeros (la.last_use); a caller's buffer is zeroed here and keeps its length after every call it is handed to (a plan made ahead
  // serves any number of calls).  Only the lean exact road lists such bricks: the planned brick road has plan_multi == 0, nothing reads its header.
  if (a.plan_multi && hipMemsetAsync(plan_dev, 0, kPlanHeaderInts * sizeof(int), s) != hipSuccess)
    return tio::fail(TIO_ERR_LAUNCH, "tio_resample3d_plan: cannot reset the brick plan");
  enqueue_planner(a, static_cast<int*>(plan_dev) + kPlanHeaderInts, static_cast<int>(bricks), s);
  return tio::check_launch("tio_resample3d_plan");
}

extern "C" int tio_resample3d(const tio_resample_geom* geom, int32_t n_images, const tio_resample_image* images, void* stream) {
  bool folded = false;
  const int status = resample3d_impl(geom, n_images, images, stream, &folded);
  if (status != TIO_OK || folded || geom == nullptr || images == nullptr || geom->batch < 1) return status;
  // out_min_dev of launches that did not fold it into their stores: the plain reduction over what was just written
  const int64_t n_out = static_cast<int64_t>(geom->out_shape[0]) * geom->out_shape[1] * geom->out_shape[2];
  for (int i = 0; i < n_images; i++) {
    const tio_resample_image& im = images[i];
    if (im.out_min_dev == nullptr || im.interp == TIO_LINEAR_ADJOINT) continue;
    const int st = tio_channel_min(im.out, im.dtype, im.channels, n_out, im.out_min_dev, stream);
    if (st != TIO_OK) return st;
  }
  return TIO_OK;
}
