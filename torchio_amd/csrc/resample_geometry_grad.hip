// resample_geometry_grad.hip — tio_resample3d_geometry_grad: the gradient of a trilinear resampling with respect to its GEOMETRY,
// the 3 x 4 mapping and the elastic control points (what autograd derives through the (B, I, J, K, 3) grid of the reference's
// grid_sample, spatial.py:1695-1731, without that grid or any per-voxel gradient field ever reaching HBM).  DESIGN.md 4.8 / 4.21.
//
// Definition.  Images x_n (B, C_n, I, J, K), incoming gradients g_n (B, C_n, Io, Jo, Ko) float32, the geometry of tio_resample_geom.
// For output voxel o = (i, j, k) of element b the sampling coordinate (x_0, x_1, x_2) is the forward launch's own float32 value:
// the TIO_PRECISION_EXACT chain of resample_kernel through the helpers of resample_coords.hpp, in every precision mode (as the
// adjoint).  cell = floor(coordinate); the eight taps t carry the weights wa0 = cell_a + 1 - x_a (lower) and wa1 = x_a - cell_a.
//   per-axis derivative   D_a(o) = sum_n sum_c g_n[b,c,o] * sum_{t in bounds} x_n[b,c,t] * s_a(t) * (the two other axes' weights of t),
//                         s_a = -1 on the lower tap, +1 on the upper; taps out of bounds are skipped
//                         (ATen's grid_sampler_3d_backward, padding_mode="zeros", align_corners=True)
//   gate                  image n has fill_dev != NULL and the in-bounds weight of o (summed in ATen's tap order, as the forward
//                         sums it) is <= 0.5: the forward wrote the fill, image n adds nothing at o (the mask carries no gradient)
//   round trip            d_a = D_a * (S_own[a] - 1) / max(S_norm[a] - 1, 1): the normalise / un-normalise pair; exactly 0 where S_own[a] == 1
//   mapping, affine_first == 1 or no elastic component (none in the call, or cp_skip[b]):
//                         dM[r][0..3] += d_r * (i, j, k, 1);            dDisp[e] = d_e / in_spacing[e]
//   mapping, affine_first == 0 with an elastic component, s = c + disp / out_spacing the source coordinate the forward forms:
//                         dM[r][0..3] += d_r * (s_0, s_1, s_2, 1);      dDisp[e] = (sum_r M[r][e] d_r) / out_spacing[e]
//   control points        dCP[node][e] += W(node; i, j, k) * dDisp[e] over the eight nodes of the voxel's control cell, W the product of
//                         the forward's three align-corners lerp weights (lerp_index)
//   flags                 passthrough[b]: element b adds nothing; cp_skip[b]: nothing to dCP, its mapping still receives its gradient
//   shared parameters     mapping_batched == 0: dM is (1, 3, 4), summed over the batch; cp_batched == 0 likewise
//   outputs               float32 in the shapes of mapping / control_points, fully overwritten (the caller need not zero them)
//
// The reduction (sized in DESIGN.md 4.21).  The block shape is the gather road's: one wave per output row, 64 lanes along ko, kTileI
// slabs per block.  Mapping: 12 float32 accumulators per lane over the lane's <= kTileI voxels, summed across the wave by shuffles and
// across the four waves through LDS in a fixed order: ONE float64 partial per block.  Control points: i / j nodes and weights are
// wave-uniform, so a row reduces per k node by shuffles (fixed order) and 12 lanes add (2 x 2 nodes) x 3 components into the
// block's float64 LDS box of the nodes its voxels can touch; only non-zero entries of that box are flushed.  Across blocks: float64
// atomics into the workspace (the mapping's spread over kSpread slots per matrix against same-address queueing), and a finishing
// kernel sums the slots in a fixed order and writes the float32 outputs.
// Reproducibility: every float32 operation has a fixed order; the float64 additions (LDS box, workspace) have not.  Their
// differences are ~2^-53 of the magnitudes summed, so two runs differ at most in the last float32 rounding of an output.
#include <stdint.h>

#include "resample_args.hpp"
#include "resample_coords.hpp"

namespace tio {
namespace {

constexpr int kTileI = 8;         // output slabs walked by one block (resample.hip: the gather road's shape)
constexpr int kRowsPerBlock = 4;  // one wave per output row (jo)
constexpr int kLanes = 64;        // contiguous ko per wave
constexpr int kSpread = 16;       // workspace slots per mapping: block partials of one matrix queue on 16 cache lines, not one
constexpr int kSlotDoubles = 16;  // 12 used: one 128-byte line per slot
constexpr int kBoxDoubles = 1536;  // the block's LDS box of control values (12 KiB); a block whose nodes exceed it adds to the workspace directly

struct GradArgs {
  ResampleArgs a;        // geometry and images as the forward launch sees them (img[n].out: the incoming gradient, read)
  float ratio[3];        // (S_own - 1) / max(S_norm - 1, 1)
  double* ws_mapping;    // [n_mappings][kSpread][kSlotDoubles], or null: no mapping gradient wanted
  double* ws_cp;         // [n_grids][ni * nj * nk * 3], or null: no control-point gradient wanted
};

__device__ __forceinline__ float wave_sum(float v) {  // fixed order: the same tree in every run
#pragma unroll
  for (int offset = 32; offset > 0; offset >>= 1) v = __fadd_rn(v, __shfl_xor(v, offset, kLanes));
  return v;
}

// sum over the channels of image g of grad * (the three one-sided tap differences): D_x, D_y, D_z of one image at one voxel
template <int DT>
__device__ __forceinline__ void image_derivative(const ImgArgs& g, int b, int64_t n_in, int64_t n_out, int64_t o_idx, const int (&off)[8],
                                                 unsigned okbits, const float (&wx)[2], const float (&wy)[2], const float (&wz)[2],
                                                 float (&D)[3]) {
  for (int c = 0; c < g.channels; c++) {
    const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
    const typename Elem<DT>::type* p = static_cast<const typename Elem<DT>::type*>(g.in) + bc * n_in;
    const float gv = static_cast<const float*>(g.out)[bc * n_out + o_idx];
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {  // (offsets are clamped into the volume: the load is always legal, the value is dropped)
      const float t = Elem<DT>::load(p, off[k]);
      v[k] = ((okbits >> k) & 1u) ? t : 0.0f;
    }
    // tap k: bit0 = x + 1, bit1 = y + 1, bit2 = z + 1 (ATen's order, as in the forward)
    const float dx = (wy[0] * wz[0]) * (v[1] - v[0]) + (wy[1] * wz[0]) * (v[3] - v[2]) + (wy[0] * wz[1]) * (v[5] - v[4]) + (wy[1] * wz[1]) * (v[7] - v[6]);
    const float dy = (wx[0] * wz[0]) * (v[2] - v[0]) + (wx[1] * wz[0]) * (v[3] - v[1]) + (wx[0] * wz[1]) * (v[6] - v[4]) + (wx[1] * wz[1]) * (v[7] - v[5]);
    const float dz = (wx[0] * wy[0]) * (v[4] - v[0]) + (wx[1] * wy[0]) * (v[5] - v[1]) + (wx[0] * wy[1]) * (v[6] - v[2]) + (wx[1] * wy[1]) * (v[7] - v[3]);
    D[0] += gv * dx;
    D[1] += gv * dy;
    D[2] += gv * dz;
  }
}

template <bool ELASTIC_POSSIBLE>
__global__ __launch_bounds__(kRowsPerBlock* kLanes) void geometry_grad_kernel(const GradArgs ga) {
  const ResampleArgs& a = ga.a;
  __shared__ double s_box[ELASTIC_POSSIBLE ? kBoxDoubles : 1];
  __shared__ float s_rows[kRowsPerBlock][12];

  // tile decode: as resample_kernel
  const unsigned tile = xcd_remap(blockIdx.x, gridDim.x);
  const int kt = tile % a.tiles_k;
  const unsigned t1 = tile / a.tiles_k;
  const int jt = t1 % a.tiles_j;
  const unsigned t2 = t1 / a.tiles_j;
  const int it = t2 % a.tiles_i;
  const int b = t2 / a.tiles_i;

  if (a.passthrough != nullptr && a.passthrough[b] != 0) return;  // block-uniform: a gated-out element adds nothing

  const int lane = threadIdx.x & (kLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kLanes);
  const int jo_raw = jt * kRowsPerBlock + wave;
  const int ko_raw = kt * kLanes + lane;
  const bool active = jo_raw < a.Jo && ko_raw < a.Ko;
  const int jo = min(jo_raw, a.Jo - 1), ko = min(ko_raw, a.Ko - 1);  // idle threads shadow a voxel of the volume and add zeros
  const int i_begin = it * kTileI;
  const int i_end = min(i_begin + kTileI, a.Io);

  bool elastic = false;
  const float* cp = nullptr;
  if constexpr (ELASTIC_POSSIBLE) {
    elastic = !(a.cp_skip != nullptr && a.cp_skip[b] != 0);
    cp = a.cp + (a.cp_batched ? static_cast<int64_t>(b) * a.ni * a.nj * a.nk * 3 : 0);
  }
  const bool want_cp = ELASTIC_POSSIBLE && elastic && ga.ws_cp != nullptr;

  const int64_t n_in = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t n_out = static_cast<int64_t>(a.Io) * a.Jo * a.Ko;
  const int64_t row = static_cast<int64_t>(jo) * a.Ko + ko;
  const int64_t slab = static_cast<int64_t>(a.Jo) * a.Ko;

  const float* m = a.mapping + (a.mapping_batched ? b * 12 : 0);
  const float m00 = m[0], m01 = m[1], m02 = m[2], m03 = m[3];
  const float m10 = m[4], m11 = m[5], m12 = m[6], m13 = m[7];
  const float m20 = m[8], m21 = m[9], m22 = m[10], m23 = m[11];
  const float cj = static_cast<float>(jo), ck = static_cast<float>(ko);

  Lerp1D lj{0, 0, 1.0f, 0.0f}, lk{0, 0, 1.0f, 0.0f};
  int s_i = 0, s_j = 0;
  // the block's box of control nodes: [bi0, bi0 + bni) x [bj0, ...) x [bk0, ...), every node a voxel of the block can touch
  int bi0 = 0, bj0 = 0, bk0 = 0, bni = 0, bnj = 0, bnk = 0, kk_lo = 0, kk_hi = -1;
  bool box_in_lds = false;
  if constexpr (ELASTIC_POSSIBLE) {
    if (elastic) {
      lj = lerp_index(jo, a.nj, a.Jo, a.scale_j);
      lk = lerp_index(ko, a.nk, a.Ko, a.scale_k);
      s_i = a.nj * a.nk * 3;
      s_j = a.nk * 3;
    }
    if (want_cp) {  // lerp_index is monotone in its voxel: the first and the last voxel of each axis bound the nodes
      const int j_last = min(jt * kRowsPerBlock + kRowsPerBlock, a.Jo) - 1, k_last = min(kt * kLanes + kLanes, a.Ko) - 1;
      bi0 = lerp_index(i_begin, a.ni, a.Io, a.scale_i).i0;
      bni = lerp_index(i_end - 1, a.ni, a.Io, a.scale_i).i1 - bi0 + 1;
      bj0 = lerp_index(jt * kRowsPerBlock, a.nj, a.Jo, a.scale_j).i0;
      bnj = lerp_index(j_last, a.nj, a.Jo, a.scale_j).i1 - bj0 + 1;
      bk0 = lerp_index(kt * kLanes, a.nk, a.Ko, a.scale_k).i0;
      bnk = lerp_index(k_last, a.nk, a.Ko, a.scale_k).i1 - bk0 + 1;
      box_in_lds = static_cast<int64_t>(bni) * bnj * bnk * 3 <= kBoxDoubles;
      if (box_in_lds) {
        for (int t = threadIdx.x; t < bni * bnj * bnk * 3; t += blockDim.x) s_box[t] = 0.0;
      }
      kk_lo = bk0;  // this wave's k nodes are the block's: every wave of the block covers the same ko range
      kk_hi = bk0 + bnk - 1;
    }
    __syncthreads();  // (uniform: `elastic` and the pass flag are per element, an element per block)
  }

  const float hx = a.size_m1[0], hy = a.size_m1[1], hz = a.size_m1[2];
  const float sp0 = a.sp[0], sp1 = a.sp[1], sp2 = a.sp[2];

  float acc[12];
#pragma unroll
  for (int t = 0; t < 12; t++) acc[t] = 0.0f;

  for (int io = i_begin; io < i_end; io++) {
    const float ci = static_cast<float>(io);
    float vi, vj, vk;
    float p0 = ci, p1 = cj, p2 = ck;  // what multiplies the matrix: the output voxel, or the displaced source coordinate
    Lerp1D li{0, 0, 1.0f, 0.0f};
    bool chained = false;  // affine_first == 0 with an elastic component: the displacement goes through the matrix
    bool displaced = false;
    if constexpr (ELASTIC_POSSIBLE) displaced = elastic;
    if (displaced) {
      li = lerp_index(io, a.ni, a.Io, a.scale_i);
      const Disp d = cp_trilerp3(cp, s_i, s_j, li, lj, lk);
      float di = d.i, dj = d.j, dk = d.k;
      if (!a.unit_spacing) {  // mm -> voxels: true division by the spacing
        di = exact_div(di, a.sp[0], a.rsp[0]);
        dj = exact_div(dj, a.sp[1], a.rsp[1]);
        dk = exact_div(dk, a.sp[2], a.rsp[2]);
      }
      if (a.affine_first) {
        vi = __fadd_rn(TIO_AFFINE_ROW(m00, m01, m02, m03, ci, cj, ck), di);
        vj = __fadd_rn(TIO_AFFINE_ROW(m10, m11, m12, m13, ci, cj, ck), dj);
        vk = __fadd_rn(TIO_AFFINE_ROW(m20, m21, m22, m23, ci, cj, ck), dk);
      } else {
        p0 = __fadd_rn(ci, di); p1 = __fadd_rn(cj, dj); p2 = __fadd_rn(ck, dk);
        vi = TIO_AFFINE_ROW(m00, m01, m02, m03, p0, p1, p2);
        vj = TIO_AFFINE_ROW(m10, m11, m12, m13, p0, p1, p2);
        vk = TIO_AFFINE_ROW(m20, m21, m22, m23, p0, p1, p2);
        chained = true;
      }
    } else {
      vi = TIO_AFFINE_ROW(m00, m01, m02, m03, ci, cj, ck);
      vj = TIO_AFFINE_ROW(m10, m11, m12, m13, ci, cj, ck);
      vk = TIO_AFFINE_ROW(m20, m21, m22, m23, ci, cj, ck);
    }
    const float x = normalise_roundtrip(vi, a.den[0], a.rden[0], hx);
    const float y = normalise_roundtrip(vj, a.den[1], a.rden[1], hy);
    const float z = normalise_roundtrip(vk, a.den[2], a.rden[2], hz);

    // cell, weights, bounds and the in-bounds weight: resample_kernel's boundary path, operation for operation
    const float x0 = floorf(x), y0 = floorf(y), z0 = floorf(z);
    const float x1 = x0 + 1.0f, y1 = y0 + 1.0f, z1 = z0 + 1.0f;
    const float wx[2] = {x1 - x, x - x0}, wy[2] = {y1 - y, y - y0}, wz[2] = {z1 - z, z - z0};
    float w[8];
    corner_weights(wx[0], wx[1], wy[0], wy[1], wz[0], wz[1], w);
    const bool bx0 = (x0 >= 0.0f) & (x0 <= hx), bx1 = (x1 >= 0.0f) & (x1 <= hx);
    const bool by0 = (y0 >= 0.0f) & (y0 <= hy), by1 = (y1 >= 0.0f) & (y1 <= hy);
    const bool bz0 = (z0 >= 0.0f) & (z0 <= hz), bz1 = (z1 >= 0.0f) & (z1 <= hz);
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
      const float next = __fadd_rn(mask, w[k]);  // ATen's accumulation order
      mask = ok ? next : mask;
    }

    float D[3] = {0.0f, 0.0f, 0.0f};
    if (active && okbits != 0u) {
      const int64_t o_idx = io * slab + row;
      for (int im = 0; im < a.n_images; im++) {
        const ImgArgs& g = a.img[im];
        if (g.fill != nullptr && !(mask > 0.5f)) continue;  // the forward wrote the fill here
        switch (g.dtype) {  // uniform: a scalar branch
          case TIO_F32: image_derivative<TIO_F32>(g, b, n_in, n_out, o_idx, off, okbits, wx, wy, wz, D); break;
          case TIO_F16: image_derivative<TIO_F16>(g, b, n_in, n_out, o_idx, off, okbits, wx, wy, wz, D); break;
          case TIO_BF16: image_derivative<TIO_BF16>(g, b, n_in, n_out, o_idx, off, okbits, wx, wy, wz, D); break;
          default: image_derivative<TIO_F64>(g, b, n_in, n_out, o_idx, off, okbits, wx, wy, wz, D); break;
        }
      }
    }
    const float d0 = D[0] * ga.ratio[0], d1 = D[1] * ga.ratio[1], d2 = D[2] * ga.ratio[2];

    acc[0] += d0 * p0; acc[1] += d0 * p1; acc[2] += d0 * p2; acc[3] += d0;
    acc[4] += d1 * p0; acc[5] += d1 * p1; acc[6] += d1 * p2; acc[7] += d1;
    acc[8] += d2 * p0; acc[9] += d2 * p1; acc[10] += d2 * p2; acc[11] += d2;

    if constexpr (ELASTIC_POSSIBLE) {
      if (want_cp) {
        float e0 = d0, e1 = d1, e2 = d2;
        if (chained) {  // M^T d
          e0 = m00 * d0 + m10 * d1 + m20 * d2;
          e1 = m01 * d0 + m11 * d1 + m21 * d2;
          e2 = m02 * d0 + m12 * d1 + m22 * d2;
        }
        if (!a.unit_spacing) { e0 = e0 / sp0; e1 = e1 / sp1; e2 = e2 / sp2; }
        // i / j nodes and weights are the wave's; per k node one shuffle sum, then 12 lanes add (2 x 2 nodes) x 3 components
        for (int kk = kk_lo; kk <= kk_hi; kk++) {
          const float ckk = (lk.i0 == kk ? lk.l0 : 0.0f) + (lk.i1 == kk ? lk.l1 : 0.0f);
          const float t0 = wave_sum(ckk * e0), t1s = wave_sum(ckk * e1), t2s = wave_sum(ckk * e2);
          if (lane < 12) {
            const int combo = lane / 3, e = lane - combo * 3;
            const float te = e == 0 ? t0 : (e == 1 ? t1s : t2s);
            const float wi = (combo & 1) ? li.l1 : li.l0, wj = (combo & 2) ? lj.l1 : lj.l0;
            const int ii = (combo & 1) ? li.i1 : li.i0, jj = (combo & 2) ? lj.i1 : lj.i0;
            const float value = (wi * wj) * te;
            if (value != 0.0f) {
              if (box_in_lds) {
                atomicAdd(&s_box[(((ii - bi0) * bnj + (jj - bj0)) * bnk + (kk - bk0)) * 3 + e], static_cast<double>(value));
              } else {
                const int64_t grid = a.cp_batched ? static_cast<int64_t>(b) * a.ni * a.nj * a.nk * 3 : 0;
                unsafeAtomicAdd(ga.ws_cp + grid + (static_cast<int64_t>(ii) * a.nj + jj) * a.nk * 3 + kk * 3 + e, static_cast<double>(value));
              }
            }
          }
        }
      }
    }
  }

  // mapping: wave sums by shuffles, the four rows through LDS in a fixed order, one float64 partial per block
  if (ga.ws_mapping != nullptr) {
#pragma unroll
    for (int t = 0; t < 12; t++) {
      const float total = wave_sum(acc[t]);
      if (lane == 0) s_rows[wave][t] = total;
    }
  }
  __syncthreads();
  if (ga.ws_mapping != nullptr && threadIdx.x < 12) {
    double total = 0.0;
    for (int r = 0; r < kRowsPerBlock; r++) total += static_cast<double>(s_rows[r][threadIdx.x]);
    if (total != 0.0) {
      double* slot = ga.ws_mapping + ((a.mapping_batched ? static_cast<int64_t>(b) : 0) * kSpread + (blockIdx.x % kSpread)) * kSlotDoubles;
      unsafeAtomicAdd(slot + threadIdx.x, total);
    }
  }
  if constexpr (ELASTIC_POSSIBLE) {
    if (want_cp && box_in_lds) {  // (the barrier above ordered the box's additions before these reads)
      const int64_t grid = a.cp_batched ? static_cast<int64_t>(b) * a.ni * a.nj * a.nk * 3 : 0;
      for (int t = threadIdx.x; t < bni * bnj * bnk * 3; t += blockDim.x) {
        const double value = s_box[t];
        if (value == 0.0) continue;
        const int e = t % 3, node = t / 3;
        const int kk = node % bnk, jj = (node / bnk) % bnj, ii = node / (bnk * bnj);
        unsafeAtomicAdd(ga.ws_cp + grid + ((static_cast<int64_t>(ii + bi0) * a.nj + (jj + bj0)) * a.nk + (kk + bk0)) * 3 + e, value);
      }
    }
  }
}

// workspace -> float32 outputs: the mapping's slots summed in a fixed order; one thread per output value
__global__ void geometry_grad_finish_kernel(const double* __restrict__ ws_mapping, const double* __restrict__ ws_cp, float* __restrict__ d_mapping,
                                            float* __restrict__ d_cp, int64_t n_mapping, int64_t n_cp) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t < n_mapping) {
    if (d_mapping != nullptr) {
      const double* slots = ws_mapping + (t / 12) * kSpread * kSlotDoubles + t % 12;
      double total = 0.0;
      for (int s = 0; s < kSpread; s++) total += slots[s * kSlotDoubles];
      d_mapping[t] = static_cast<float>(total);
    }
  } else if (t - n_mapping < n_cp) {
    if (d_cp != nullptr) d_cp[t - n_mapping] = static_cast<float>(ws_cp[t - n_mapping]);
  }
}

struct Layout {
  int64_t mapping_doubles = 0, cp_doubles = 0;
  int64_t bytes() const { return (mapping_doubles + cp_doubles) * static_cast<int64_t>(sizeof(double)); }
};

Layout workspace_layout(const tio_resample_geom* geom) {
  Layout l;
  const int64_t batch = geom->batch > 0 ? geom->batch : 0;
  l.mapping_doubles = (geom->mapping_batched ? batch : 1) * kSpread * kSlotDoubles;
  if (geom->control_points_dev != nullptr && geom->cp_shape[0] > 0 && geom->cp_shape[1] > 0 && geom->cp_shape[2] > 0)
    l.cp_doubles = (geom->cp_batched ? batch : 1) * static_cast<int64_t>(geom->cp_shape[0]) * geom->cp_shape[1] * geom->cp_shape[2] * 3;
  return l;
}

}  // namespace
}  // namespace tio

using namespace tio;

extern "C" int64_t tio_resample3d_geometry_grad_workspace_bytes(const tio_resample_geom* geom) {
  if (geom == nullptr) {
    fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad_workspace_bytes: null geometry");
    return 0;
  }
  return workspace_layout(geom).bytes();
}

extern "C" int tio_resample3d_geometry_grad(const tio_resample_geom* geom, int32_t n_images, const tio_resample_image* images, float* d_mapping,
                                            float* d_control_points, void* workspace, int64_t workspace_bytes, void* stream) {
  if (geom == nullptr || images == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad: null argument");
  if (n_images < 1 || n_images > TIO_MAX_IMAGES)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad: n_images must be in 1..%d", TIO_MAX_IMAGES);
  if (d_mapping == nullptr && d_control_points == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad: neither d_mapping nor d_control_points is wanted");
  if (d_control_points != nullptr && geom->control_points_dev == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad: d_control_points without control points in the geometry");
  GradArgs ga{};
  ResampleArgs& a = ga.a;
  if (const int st = resample_check_geometry(geom, a)) return st;
  for (int i = 0; i < n_images; i++) {
    const tio_resample_image& s = images[i];
    if (s.in == nullptr || s.out == nullptr || s.channels < 1)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad: image %d has null data or no channels", i);
    if (!is_known_dtype(s.dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_resample3d_geometry_grad: image %d dtype %d", i, s.dtype);
    if (!is_float_dtype(s.dtype))
      return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_resample3d_geometry_grad: image %d: only floating-point images carry a geometry gradient", i);
    if (s.interp != TIO_LINEAR)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad: image %d interp %d: only TIO_LINEAR images carry a geometry gradient", i, s.interp);
    a.img[a.n_images++] = ImgArgs{s.in, s.out, s.fill_dev, s.channels, s.dtype, s.interp, nullptr, 0, 0.0, nullptr, nullptr};
  }
  const Layout layout = workspace_layout(geom);
  if (workspace == nullptr || workspace_bytes < layout.bytes())
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad: the workspace holds %lld bytes, %lld are needed", static_cast<long long>(workspace_bytes),
                static_cast<long long>(layout.bytes()));
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad: the workspace must be 8-byte aligned");
  unsigned blocks = 0;
  if (a.B > 0) {
    a.tiles_k = (a.Ko + kLanes - 1) / kLanes; a.tiles_j = (a.Jo + kRowsPerBlock - 1) / kRowsPerBlock; a.tiles_i = (a.Io + kTileI - 1) / kTileI;
    const int64_t n = static_cast<int64_t>(a.B) * a.tiles_i * a.tiles_j * a.tiles_k;
    if (n >= (1LL << 31)) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_resample3d_geometry_grad: grid too large");
    blocks = static_cast<unsigned>(n);
  }
  for (int d = 0; d < 3; d++) ga.ratio[d] = a.B > 0 ? a.size_m1[d] / a.den[d] : 0.0f;

  hipStream_t s = static_cast<hipStream_t>(stream);
  ga.ws_mapping = d_mapping != nullptr ? static_cast<double*>(workspace) : nullptr;
  ga.ws_cp = d_control_points != nullptr ? static_cast<double*>(workspace) + layout.mapping_doubles : nullptr;
  if (hipMemsetAsync(workspace, 0, static_cast<size_t>(layout.bytes()), s) != hipSuccess)
    return fail(TIO_ERR_LAUNCH, "tio_resample3d_geometry_grad: cannot clear the workspace");
  if (blocks > 0) {
    with_bools([&](auto elastic) { hipLaunchKernelGGL((geometry_grad_kernel<elastic.value>), dim3(blocks), dim3(kRowsPerBlock * kLanes), 0, s, ga); },
               a.cp != nullptr);
  }
  const int64_t n_mapping = d_mapping != nullptr ? layout.mapping_doubles / (kSpread * kSlotDoubles) * 12 : 0;
  const int64_t n_cp = d_control_points != nullptr ? layout.cp_doubles : 0;
  const int64_t threads = n_mapping + n_cp;
  if (threads > 0)
    hipLaunchKernelGGL(geometry_grad_finish_kernel, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, s, ga.ws_mapping, ga.ws_cp, d_mapping,
                       d_control_points, n_mapping, n_cp);
  return check_launch("tio_resample3d_geometry_grad");
}
