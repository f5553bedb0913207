// stencil.hip — the separable stencil for gfx950 (Blur / antialias; blur.py:157-252):
//   tio_separable_conv3d          one pass per active axis: the generic, 16-byte ring and K kernels below and the plain
//                                 I / J and bias-on-load instantiations of conv_march_kernel (stencil_march.hpp)
//   tio_separable_conv3d_passes   what plan_conv would launch, without launching it
//   tio_separable_conv3d_adjoint  the backward pass
//   tio_blur_fused                BiasField on the loads of the I pass, Noise on the stores of the fused J + K pass
// plan_conv / launch_conv decide every launch, those of the fused J + K instantiations in stencil_fused.hip included.
// HBM-bound: one read + one write of the volume per pass.  No MFMA.
#include <algorithm>

#include "common.hpp"
#include "philox_normal.hpp"
#include "stencil_march.hpp"  // kBlock, ConvArgs, conv_march_kernel

namespace tio {

// =============================================================================
// Separable cross-correlation with replicate padding
// =============================================================================
// One pass = one axis.  Lanes always run along K (contiguous), so every global
// access is a coalesced row segment.  A block stages the line segment it needs
// (+ replicate-clamped halo) in LDS once and every thread then reads its
// 2r+1 taps from LDS in tap order — the accumulation order of the oracle — so
// each input element is fetched from HBM/L2 ~once per pass instead of 2r+1 times.
//   axis I / J : tile = kConvLine outputs along the axis x 64 lanes along K
//   axis K     : tile = 4 rows x 256 outputs along K (one wave per row)
constexpr int kConvLine = 32;   // outputs along the stencil axis per block (axes I, J)
constexpr int kConvKSpan = 256; // outputs along K per wave (axis K)
constexpr int kMaxRadius = 48;  // LDS budget: (32 + 96) * 64 * 4 B = 32 KiB

template <int SRC_DT, int DST_DT>
__global__ __launch_bounds__(kBlock) void conv_line_kernel(const ConvArgs a) {
  // axes I and J.  grid: x = K tiles (64), y = tiles along the axis, z = other axis * (B*C)
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int r = a.radius, ntaps = 2 * r + 1;
  float* s_taps = s_mem;                 // ntaps
  float* s_tile = s_mem + ((ntaps + 3) & ~3);  // (kConvLine + 2r) x 64
  const int n_other = a.axis == 0 ? a.J : a.I;  // size of the non-stencil, non-K axis
  const int other = blockIdx.z % n_other;
  const int bc = blockIdx.z / n_other;
  const int b = bc / a.channels;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave index in an SGPR
  const int k = blockIdx.x * 64 + lane;
  const int n = a.axis == 0 ? a.I : a.J;        // length of the stencil axis
  const int p0 = blockIdx.y * kConvLine;         // first output position along the axis
  const int64_t n_spatial = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t base = static_cast<int64_t>(bc) * n_spatial;
  const int64_t stride = a.axis == 0 ? static_cast<int64_t>(a.J) * a.K : a.K;
  const int64_t other_stride = a.axis == 0 ? a.K : static_cast<int64_t>(a.J) * a.K;
  const int64_t line = base + other * other_stride + k;  // element (axis pos 0, other, k)
  const bool active = k < a.K;

  if (a.skip != nullptr && a.skip[b] != 0) {
    // rows with no blur are restored bit-exactly (blur.py:249-251): emitted unchanged by the last pass
    if (a.last_pass && active) {
      const int es = dtype_size(a.orig_dtype);
      for (int q = wave; q < kConvLine && p0 + q < n; q += kBlock / 64) {
        const int64_t e = line + static_cast<int64_t>(p0 + q) * stride;
        const char* s = static_cast<const char*>(a.x_orig) + e * es;
        char* d = static_cast<char*>(a.dst) + e * es;
        for (int c = 0; c < es; c++) d[c] = s[c];
      }
    }
    return;
  }
  const float* t = a.taps + (a.taps_batched ? static_cast<int64_t>(b) * 3 * a.tap_stride : 0) +
                   static_cast<int64_t>(a.axis) * a.tap_stride;
  for (int i = threadIdx.x; i < ntaps; i += kBlock) s_taps[i] = t[i];
  const int rows = min(kConvLine, n - p0) + 2 * r;
  if (active) {
    for (int q = wave; q < rows; q += kBlock / 64) {
      const int pos = min(max(p0 + q - r, 0), n - 1);  // replicate padding == clamp
      s_tile[q * 64 + lane] = Elem<SRC_DT>::load(a.src, line + static_cast<int64_t>(pos) * stride);
    }
  }
  __syncthreads();
  if (!active) return;
  for (int q = wave; q < kConvLine && p0 + q < n; q += kBlock / 64) {
    float acc = 0.0f;
    const float* col = s_tile + q * 64 + lane;
    for (int tt = 0; tt < ntaps; tt++) acc = __fadd_rn(acc, __fmul_rn(s_taps[tt], col[tt * 64]));
    Elem<DST_DT>::store(a.dst, line + static_cast<int64_t>(p0 + q) * stride, acc);
  }
}

template <int SRC_DT, int DST_DT>
__global__ __launch_bounds__(kBlock) void conv_k_kernel(const ConvArgs a) {
  // axis K.  grid: x = K tiles (256), y = J tiles (4 rows, one per wave), z = I * (B*C)
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int r = a.radius, ntaps = 2 * r + 1;
  float* s_taps = s_mem;
  const int pitch = kConvKSpan + 2 * r;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave index in an SGPR
  float* s_row = s_mem + ((ntaps + 3) & ~3) + wave * pitch;
  const int i = blockIdx.z % a.I;
  const int bc = blockIdx.z / a.I;
  const int b = bc / a.channels;
  const int j = blockIdx.y * (kBlock / 64) + wave;
  const int k0 = blockIdx.x * kConvKSpan;
  const int64_t n_spatial = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t row = static_cast<int64_t>(bc) * n_spatial + (static_cast<int64_t>(i) * a.J + j) * a.K;
  const bool active = j < a.J;

  if (a.skip != nullptr && a.skip[b] != 0) {
    if (a.last_pass && active) {
      const int es = dtype_size(a.orig_dtype);
      for (int q = lane; q < kConvKSpan && k0 + q < a.K; q += 64) {
        const int64_t e = row + k0 + q;
        const char* s = static_cast<const char*>(a.x_orig) + e * es;
        char* d = static_cast<char*>(a.dst) + e * es;
        for (int c = 0; c < es; c++) d[c] = s[c];
      }
    }
    return;
  }
  const float* t = a.taps + (a.taps_batched ? static_cast<int64_t>(b) * 3 * a.tap_stride : 0) + 2 * a.tap_stride;
  for (int q = threadIdx.x; q < ntaps; q += kBlock) s_taps[q] = t[q];
  const int span = min(kConvKSpan, a.K - k0);
  if (active) {
    for (int q = lane; q < span + 2 * r; q += 64) {
      const int pos = min(max(k0 + q - r, 0), a.K - 1);
      s_row[q] = Elem<SRC_DT>::load(a.src, row + pos);
    }
  }
  __syncthreads();
  if (!active) return;
  for (int q = lane; q < span; q += 64) {
    float acc = 0.0f;
    for (int tt = 0; tt < ntaps; tt++) acc = __fadd_rn(acc, __fmul_rn(s_taps[tt], s_row[q + tt]));
    Elem<DST_DT>::store(a.dst, row + k0 + q, acc);
  }
}

// ---- float32 fast paths: 16-byte global accesses ------------------------------------
// Same arithmetic (tap order, separate multiply and add) as the generic kernels above;
// used when source and destination are float32, K % 4 == 0, pointers are 16-byte
// aligned and the radius is small enough for the LDS tile.
constexpr int kConvMaxRadiusV4 = 16;  // (32 + 2*16) rows x 1 KiB = 64 KiB of LDS

constexpr int kConvStep = 16;  // output rows per marching step (axes I, J)

template <bool FUSE_K, bool PRE_BIAS, int POST_NOISE>
__global__ __launch_bounds__(kBlock) void conv_line_v4_kernel(const ConvArgs a) {
  // axes I and J.  grid: x = K tiles (256 = 64 lanes x float4), y = segments along the axis, z = other axis * (B*C).
  // A block marches along the stencil axis with a ring of kConvStep + 2r + kConvStep rows in
  // LDS: every input row is fetched exactly once (no halo re-reads between steps) and the
  // 16-byte loads of step s+1 are in flight while step s is computed.
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int r = a.radius, ntaps = 2 * r + 1;
  const int ring = 2 * kConvStep + 2 * r;
  float* s_taps = s_mem;                                                   // ntaps
  float4* s_ring = reinterpret_cast<float4*>(s_mem + ((ntaps + 3) & ~3));  // ring x 64 float4
  // fused J+K: every wave owns one staged row (8 + 256 + 8 floats) behind the ring
  float* s_krow = reinterpret_cast<float*>(s_ring + ring * 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * 272;
  const int n_other = a.axis == 0 ? a.J : a.I;
  const int other = blockIdx.z % n_other;
  const int bc = blockIdx.z / n_other;
  const int b = bc / a.channels;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave index in an SGPR
  const int k = blockIdx.x * 256 + 4 * lane;
  const int n = a.axis == 0 ? a.I : a.J;
  const int seg = (n + gridDim.y - 1) / gridDim.y;                 // outputs per segment (multiple of kConvStep except the last)
  const int p_begin = blockIdx.y * seg, p_end = min(p_begin + seg, n);
  const int64_t n_spatial = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t stride = a.axis == 0 ? static_cast<int64_t>(a.J) * a.K : a.K;
  const int64_t other_stride = a.axis == 0 ? a.K : static_cast<int64_t>(a.J) * a.K;
  const int64_t line = static_cast<int64_t>(bc) * n_spatial + other * other_stride + k;
  const bool active = k < a.K;
  const float* src = static_cast<const float*>(a.src);
  float* dst = static_cast<float*>(a.dst);
  if (p_begin >= p_end) return;

  if (a.skip != nullptr && a.skip[b] != 0) {  // rows with no blur: emitted unchanged by the last pass
    if (a.last_pass && active) {
      const float* orig = static_cast<const float*>(a.x_orig);
      for (int p = p_begin + wave; p < p_end; p += kBlock / 64) {
        const int64_t e = line + static_cast<int64_t>(p) * stride;
        *reinterpret_cast<float4*>(dst + e) = *reinterpret_cast<const float4*>(orig + e);
      }
    }
    return;
  }
  const float* t = a.taps + (a.taps_batched ? static_cast<int64_t>(b) * 3 * a.tap_stride : 0) +
                   static_cast<int64_t>(a.axis) * a.tap_stride;
  typedef __attribute__((address_space(4))) const float* const_float_ptr;  // taps are read-only for the whole launch
  const_float_ptr tc = (const_float_ptr)(t);
  const_float_ptr tk = (const_float_ptr)(a.taps + (a.taps_batched ? static_cast<int64_t>(b) * 3 * a.tap_stride : 0) + 2 * a.tap_stride);
  (void)s_taps; (void)tk; (void)s_krow;
  float tkw[17];  // the K taps of the fused stage, once, at their window positions (see conv_march_kernel)
  (void)tkw;
  if constexpr (FUSE_K) {
    const int rk0 = a.radius_k;
#pragma unroll
    for (int jj = 0; jj < 17; jj++) {
      const int tt = jj - (8 - rk0);
      tkw[jj] = (tt >= 0 && tt <= 2 * rk0) ? tk[tt] : 0.0f;
    }
  }
  float noise_mu = a.noise_mean, noise_sd = a.noise_std;  // scalar loads, once (see conv_march_kernel)
  if constexpr (POST_NOISE != 0) {
    if (a.noise_batched) {
      noise_mu = ((const_float_ptr)a.noise_mean_b)[b];
      noise_sd = ((const_float_ptr)a.noise_std_b)[b];
    }
  }
  constexpr int RW = kConvStep / (kBlock / 64);  // rows per wave per step (4)
  // PRE_BIAS (I pass of tio_blur_fused): every row is multiplied by exp(trilinear(coarse)) on its
  // way into the ring — the arithmetic of bias_kernel (K- and J-lerps of a coarse plane are
  // invariants of the lane's four k positions, redone only when the row enters a new cell)
  Lerp1D b_lk[4];
  Lerp1D b_lj{0, 0, 1.0f, 0.0f};
  float b_p0[4] = {0.f, 0.f, 0.f, 0.f}, b_p1[4] = {0.f, 0.f, 0.f, 0.f};
  int b_cur0 = -1, b_cur1 = -1;
  const float* b_fg = nullptr;
  if constexpr (PRE_BIAS) {
    b_fg = a.bias_coarse + static_cast<int64_t>(bc) * (a.bias_ci * a.bias_cj * a.bias_ck);
    b_lj = lerp_index(other, a.bias_cj, a.J, a.bias_sj);
#pragma unroll
    for (int e = 0; e < 4; e++) b_lk[e] = lerp_index(min(k + e, a.K - 1), a.bias_ck, a.K, a.bias_sk);
  }
  auto bias_row = [&](float4 v, int pos) -> float4 {
    if constexpr (PRE_BIAS) {
      const Lerp1D li = lerp_index(pos, a.bias_ci, a.I, a.bias_si);
      const int s_i = a.bias_cj * a.bias_ck, s_j = a.bias_ck;
      auto plane = [&](int ii, float (&out)[4]) {
        const float* r0 = b_fg + ii * s_i + b_lj.i0 * s_j;
        const float* r1 = b_fg + ii * s_i + b_lj.i1 * s_j;
#pragma unroll
        for (int e = 0; e < 4; e++)
          out[e] = lerp2(lerp2(r0[b_lk[e].i0], b_lk[e].l0, r0[b_lk[e].i1], b_lk[e].l1), b_lj.l0,
                         lerp2(r1[b_lk[e].i0], b_lk[e].l0, r1[b_lk[e].i1], b_lk[e].l1), b_lj.l1);
      };
      if (li.i0 != b_cur0) {
        if (li.i0 == b_cur1) {
#pragma unroll
          for (int e = 0; e < 4; e++) b_p0[e] = b_p1[e];
        } else {
          plane(li.i0, b_p0);
        }
        b_cur0 = li.i0;
      }
      if (li.i1 != b_cur1) {
        if (li.i1 == b_cur0) {
#pragma unroll
          for (int e = 0; e < 4; e++) b_p1[e] = b_p0[e];
        } else {
          plane(li.i1, b_p1);
        }
        b_cur1 = li.i1;
      }
      v.x = __fmul_rn(v.x, expf(lerp2(b_p0[0], li.l0, b_p1[0], li.l1)));  // bias_field.py:341, :130
      v.y = __fmul_rn(v.y, expf(lerp2(b_p0[1], li.l0, b_p1[1], li.l1)));
      v.z = __fmul_rn(v.z, expf(lerp2(b_p0[2], li.l0, b_p1[2], li.l1)));
      v.w = __fmul_rn(v.w, expf(lerp2(b_p0[3], li.l0, b_p1[3], li.l1)));
    }
    return v;
  };
  // logical row index q counts from p_begin - r; ring slot = q mod ring (tracked incrementally)
  // prologue: rows q in [0, kConvStep + 2r) for the first step
  if (active) {
    for (int q = wave; q < kConvStep + 2 * r; q += kBlock / 64) {
      const int pos = min(max(p_begin - r + q, 0), n - 1);  // replicate padding == clamp
      s_ring[q * 64 + lane] = bias_row(*reinterpret_cast<const float4*>(src + line + static_cast<int64_t>(pos) * stride), pos);
    }
  }
  __syncthreads();
  int slot0 = 0;  // ring slot of logical row (step start - r)
  // rows of step s+1 (pre1) are written to the ring at the end of step s; rows of step s+2
  // (pre2) are requested at the start of step s — two steps of 16-byte loads in flight per lane
  typedef float v4f __attribute__((ext_vector_type(4)));  // native vector type: stays in registers (HIP's float4 struct arrays did not)
  v4f pre1[RW], pre2[RW];
#define TIO_FETCH_ROWS(DSTV, P_FIRST) /* rows P_FIRST + r + wave*RW + u, replicate-clamped */        \
  _Pragma("unroll") for (int u = 0; u < RW; u++) {                                                  \
    const int pos_ = min(max((P_FIRST) + r + wave * RW + u, 0), n - 1);                             \
    DSTV[u] = *reinterpret_cast<const v4f*>(src + line + static_cast<int64_t>(pos_) * stride);     \
  }
  if (active && p_begin + kConvStep < p_end) { TIO_FETCH_ROWS(pre1, p_begin + kConvStep) }
  for (int p0 = p_begin; p0 < p_end; p0 += kConvStep) {
    const bool more = p0 + kConvStep < p_end;
    if (active && p0 + 2 * kConvStep < p_end) { TIO_FETCH_ROWS(pre2, p0 + 2 * kConvStep) }
    if (active) {
#pragma unroll
      for (int u = 0; u < RW; u++) {
        const int o = wave * RW + u;  // output row inside the step
        if (p0 + o < p_end) {
          float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          int slot = slot0 + o;
          if (slot >= ring) slot -= ring;
          for (int tt = 0; tt < ntaps; tt++) {
            const float w = tc[tt];  // scalar load (constant address space), not an LDS read per lane
            const float4 v = s_ring[slot * 64 + lane];
            acc.x = __fadd_rn(acc.x, __fmul_rn(w, v.x));
            acc.y = __fadd_rn(acc.y, __fmul_rn(w, v.y));
            acc.z = __fadd_rn(acc.z, __fmul_rn(w, v.z));
            acc.w = __fadd_rn(acc.w, __fmul_rn(w, v.w));
            slot = slot + 1 == ring ? 0 : slot + 1;
          }
          if constexpr (FUSE_K) {
            // the row this wave just produced (its 256 K positions are spread over the 64 lanes)
            // goes through the register-window K filter of conv_k_v4_kernel before it is stored:
            // the float32 rounding between the J and the K pass is kept, only the HBM round trip goes
            const int rk = a.radius_k;
            const float edge_l = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc.x), 0));
            const float edge_r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc.w), a.K / 4 - 1));
            *reinterpret_cast<float4*>(s_krow + 8 + 4 * lane) = acc;
            // replicate padding over the WHOLE halo (8 positions a side), not only the radius: the fast taps run over a tier of
            // radii with zero-padded taps, and 0 * (whatever LDS held before) is NaN when that happens to be non-finite
            // (round 5: tests/test_gpu_ops_parity.py::test_fused_jk_stage_every_k_radius failed behind a test that left Inf there)
            (void)rk;
            for (int h = lane; h < 16; h += a.K / 4) {  // only the K/4 lanes that own data are active here
              if (h < 8) s_krow[h] = edge_l;                   // left
              else s_krow[8 + a.K + (h - 8)] = edge_r;         // right
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const float4* rv = reinterpret_cast<const float4*>(s_krow + 8) + lane;
            float w[20];
#pragma unroll
            for (int d = 0; d < 5; d++) {
              const float4 c = rv[d - 2];
              w[4 * d] = c.x; w[4 * d + 1] = c.y; w[4 * d + 2] = c.z; w[4 * d + 3] = c.w;
            }
            float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int jj = 0; jj < 17; jj++) {
              if (jj >= 8 - rk && jj <= 8 + rk) {
                const float tw = tkw[jj];
                out.x = __fadd_rn(out.x, __fmul_rn(tw, w[jj]));
                out.y = __fadd_rn(out.y, __fmul_rn(tw, w[jj + 1]));
                out.z = __fadd_rn(out.z, __fmul_rn(tw, w[jj + 2]));
                out.w = __fadd_rn(out.w, __fmul_rn(tw, w[jj + 3]));
              }
            }
            acc = out;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if constexpr (POST_NOISE != 0) {
              // the arithmetic of noise_kernel's 16-byte path: same Philox block (global element
              // index >> 2), same mean + std * z, same add
              const int64_t e0 = line + static_cast<int64_t>(p0 + o) * stride;  // element index of acc.x in the tensor
              float z[4];
              if constexpr (POST_NOISE == 2) {  // explicit draws (tio_add_noise with base1_dev): the reference's own stream
                const float4 zb = *reinterpret_cast<const float4*>(a.noise_base + e0);
                z[0] = zb.x; z[1] = zb.y; z[2] = zb.z; z[3] = zb.w;
              } else {
                philox_normal4(a.noise_seed, 0, static_cast<uint64_t>(e0 >> 2), z);
              }
              const float mu = noise_mu, sd = noise_sd;
              acc.x = __fadd_rn(acc.x, __fadd_rn(mu, __fmul_rn(sd, z[0])));
              acc.y = __fadd_rn(acc.y, __fadd_rn(mu, __fmul_rn(sd, z[1])));
              acc.z = __fadd_rn(acc.z, __fadd_rn(mu, __fmul_rn(sd, z[2])));
              acc.w = __fadd_rn(acc.w, __fadd_rn(mu, __fmul_rn(sd, z[3])));
            }
          }
          *reinterpret_cast<float4*>(dst + line + static_cast<int64_t>(p0 + o) * stride) = acc;
        }
      }
    }
    if (more) {
      // the new rows overwrite slots that were last read one step ago (ring = 2 steps + 2r)
      if (active) {
#pragma unroll
        for (int u = 0; u < RW; u++) {
          int slot = slot0 + kConvStep + 2 * r + wave * RW + u;
          if (slot >= ring) slot -= ring;
          if (slot >= ring) slot -= ring;
          if constexpr (PRE_BIAS) {
            const int pos = min(max(p0 + kConvStep + r + wave * RW + u, 0), n - 1);
            s_ring[slot * 64 + lane] = bias_row(make_float4(pre1[u].x, pre1[u].y, pre1[u].z, pre1[u].w), pos);
          } else {
            *reinterpret_cast<v4f*>(&s_ring[slot * 64 + lane]) = pre1[u];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < RW; u++) pre1[u] = pre2[u];
      slot0 += kConvStep;
      if (slot0 >= ring) slot0 -= ring;
      __syncthreads();
    }
  }
}

#undef TIO_FETCH_ROWS

// (ConvArgs and the register-window marching kernel, conv_march_kernel: stencil_march.hpp)

constexpr int kConvKRows = 16;  // rows per wave per block (axis K)

__global__ __launch_bounds__(kBlock) void conv_k_v4_kernel(const ConvArgs a) {
  // axis K.  grid: x = K tiles (256), y = J groups (4 waves x kConvKRows rows), z = I * (B*C).
  // Each wave walks kConvKRows rows: one 16-byte load per lane per row (the next row's load
  // is in flight while the current one is filtered), taps applied to lane-consecutive
  // positions (conflict-free LDS reads), results transposed through LDS so that the store
  // is one 16-byte access per lane as well.
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int r = a.radius, ntaps = 2 * r + 1;
  const int r4 = max((r + 3) & ~3, 8);           // aligned offset of the main part inside a staged row (>= 8: window path)
  const int pitch = kConvKSpan + 2 * r4;         // floats per wave row (multiple of 4)
  float* s_taps = s_mem;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave index in an SGPR
  float* s_row = s_mem + ((ntaps + 3) & ~3) + wave * (pitch + kConvKSpan);
  float* s_out = s_row + pitch;
  const int i = blockIdx.z % a.I;
  const int bc = blockIdx.z / a.I;
  const int b = bc / a.channels;
  const int j0 = (blockIdx.y * (kBlock / 64) + wave) * kConvKRows;
  const int k0 = blockIdx.x * kConvKSpan;
  const int64_t n_spatial = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t plane = static_cast<int64_t>(bc) * n_spatial + static_cast<int64_t>(i) * a.J * a.K;
  const float* src = static_cast<const float*>(a.src);
  float* dst = static_cast<float*>(a.dst);
  const int kk = k0 + 4 * lane;                  // this lane's 4 consecutive positions
  const bool lane_in = kk < a.K;                 // K % 4 == 0: all four or none
  const int j_end = min(j0 + kConvKRows, a.J);

  if (a.skip != nullptr && a.skip[b] != 0) {
    if (a.last_pass && lane_in) {
      const float* orig = static_cast<const float*>(a.x_orig);
      for (int j = j0; j < j_end; j++)
        *reinterpret_cast<float4*>(dst + plane + static_cast<int64_t>(j) * a.K + kk) =
            *reinterpret_cast<const float4*>(orig + plane + static_cast<int64_t>(j) * a.K + kk);
    }
    return;
  }
  const float* t = a.taps + (a.taps_batched ? static_cast<int64_t>(b) * 3 * a.tap_stride : 0) + 2 * a.tap_stride;
  typedef __attribute__((address_space(4))) const float* const_float_ptr;  // taps are read-only for the whole launch
  const_float_ptr tc = (const_float_ptr)(t);  // scalar loads; every wave works on its own LDS rows, no block barrier
  (void)s_taps;
  // the taps of the register-window path, once, at the window positions that use them (see conv_march_kernel)
  float tkw[17];
#pragma unroll
  for (int jj = 0; jj < 17; jj++) {
    const int tt = jj - (8 - r);
    tkw[jj] = (r <= 8 && tt >= 0 && tt <= 2 * r) ? tc[tt] : 0.0f;
  }
  const int span = min(kConvKSpan, a.K - k0);
  const float* in = s_row + r4 - r;
  // halo: lane q < 2r owns one replicate-clamped position outside the span (r on each side);
  // it is fetched together with the row, one row ahead, so no load sits on the critical path
  const int h_off = lane < r ? lane - r : span + (lane - r);
  const int h_pos = min(max(k0 + h_off, 0), a.K - 1);
  const bool h_in = lane < 2 * r;  // r <= kConvMaxRadiusV4 = 16: at most 32 halo lanes
  constexpr int G = 4;  // rows per group: the next group's loads are in flight while this one is filtered
  float4 cur[G], nxt[G];
  float hcur[G], hnxt[G];
#pragma unroll
  for (int u = 0; u < G; u++) {
    cur[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    hcur[u] = 0.0f;
    if (j0 + u < j_end) {
      const int64_t row = plane + static_cast<int64_t>(j0 + u) * a.K;
      if (lane_in) cur[u] = *reinterpret_cast<const float4*>(src + row + kk);
      if (h_in) hcur[u] = src[row + h_pos];
    }
  }
  for (int jg = j0; jg < j_end; jg += G) {
#pragma unroll
    for (int u = 0; u < G; u++) {
      nxt[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      hnxt[u] = 0.0f;
      if (jg + G + u < j_end) {
        const int64_t row = plane + static_cast<int64_t>(jg + G + u) * a.K;
        if (lane_in) nxt[u] = *reinterpret_cast<const float4*>(src + row + kk);
        if (h_in) hnxt[u] = src[row + h_pos];
      }
    }
#pragma unroll
    for (int u = 0; u < G; u++) {
      const int j = jg + u;
      if (j < j_end) {
        const int64_t row = plane + static_cast<int64_t>(j) * a.K;
        if (lane_in) *reinterpret_cast<float4*>(s_row + r4 + 4 * lane) = cur[u];
        if (h_in) s_row[r4 + h_off] = hcur[u];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // same wave: LDS operations complete in order
        __builtin_amdgcn_wave_barrier();
        if (r <= 8) {
          // register window: the lane's 4 outputs need positions 4l-8 .. 4l+11 = five aligned
          // 16-byte LDS reads (instead of one 4-byte read per tap and output); taps outside the
          // radius are skipped by a scalar branch, so the accumulation order is the oracle's
          const float4* rv = reinterpret_cast<const float4*>(s_row + r4) + lane;
          float w[20];
#pragma unroll
          for (int d = 0; d < 5; d++) {
            const float4 c = rv[d - 2];
            w[4 * d] = c.x; w[4 * d + 1] = c.y; w[4 * d + 2] = c.z; w[4 * d + 3] = c.w;
          }
          float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
          for (int jj = 0; jj < 17; jj++) {
            if (jj >= 8 - r && jj <= 8 + r) {
              const float tw = tkw[jj];
              acc.x = __fadd_rn(acc.x, __fmul_rn(tw, w[jj]));
              acc.y = __fadd_rn(acc.y, __fmul_rn(tw, w[jj + 1]));
              acc.z = __fadd_rn(acc.z, __fmul_rn(tw, w[jj + 2]));
              acc.w = __fadd_rn(acc.w, __fmul_rn(tw, w[jj + 3]));
            }
          }
          if (lane_in) *reinterpret_cast<float4*>(dst + row + kk) = acc;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          continue;
        }
        for (int q = lane; q < span; q += 64) {
          float acc = 0.0f;
          for (int tt = 0; tt < ntaps; tt++) acc = __fadd_rn(acc, __fmul_rn(tc[tt], in[q + tt]));
          s_out[q] = acc;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane_in) *reinterpret_cast<float4*>(dst + row + kk) = *reinterpret_cast<const float4*>(s_out + 4 * lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
#pragma unroll
    for (int u = 0; u < G; u++) {
      cur[u] = nxt[u];
      hcur[u] = hnxt[u];
    }
  }
}

struct ConvFuse {  // optional pointwise stages of tio_blur_fused
  const float* bias_coarse = nullptr;
  int bias_shape[3] = {0, 0, 0};
  int noise_on = 0, noise_batched = 0;
  float noise_mean = 0.0f, noise_std = 0.0f;
  const float* noise_mean_b = nullptr;
  const float* noise_std_b = nullptr;
  uint64_t noise_seed = 0;
  const float* noise_base = nullptr;
  int fma = 0;
  bool any() const { return bias_coarse != nullptr || noise_on != 0; }
};

// ---- the dispatcher's decisions (host only) --------------------------------------------------
// plan_conv decides everything launch_conv launches — the pass list and, per pass, the kernel family, the compile-time
// radius of the marching kernel, the stages that ride along, the grid and the dynamic LDS — from counts and alignment bits
// alone: it reads no pointer and enqueues nothing.  launch_conv and tio_separable_conv3d_passes both go through it, so what
// the latter reports is what the former launches (tests/test_stencil_passes.py pins the thresholds on the CPU).
constexpr unsigned kAlignedX = 1u, kAlignedY = 2u, kAlignedTmp0 = 4u, kAlignedTmp1 = 8u;  // bit set: that buffer is 16-byte aligned

static unsigned conv_alignment(const void* x, const void* y, const void* tmp0, const void* tmp1) {
  auto ok = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  return (ok(x) ? kAlignedX : 0u) | (ok(y) ? kAlignedY : 0u) | (ok(tmp0) ? kAlignedTmp0 : 0u) | (ok(tmp1) ? kAlignedTmp1 : 0u);
}

// Returns the number of passes (1 .. 3; 0 when no radius is active), TIO_ERR_UNSUPPORTED_CONFIG when stages ride along
// and the fused form does not exist for these arguments, TIO_ERR_INVALID_ARGUMENT when a pass does not fit one launch.
static int plan_conv(int dt, int32_t batch, int32_t channels, const int32_t shape[3], const int32_t radius[3], unsigned aligned,
                     bool has_skip, bool bias_on, int noise_on, bool fma, tio_conv_pass out[3]) {
  int active[3], n_active = 0;
  for (int ax = 0; ax < 3; ax++)
    if (radius[ax] > 0) active[n_active++] = ax;
  const bool io_aligned = (aligned & (kAlignedX | kAlignedY | kAlignedTmp0)) == (kAlignedX | kAlignedY | kAlignedTmp0);
  // J and K can share one pass when the whole K row sits in one 256-wide tile and both radii
  // are small: the J kernel filters every row it produces along K before storing it
  // (only the 16-byte kernels have the fused K stage: with a pointer that keeps a pass off them — the gate of the loop
  // below — the K pass must stay in the plan, or nothing filters along K)
  const bool fuse_jk = dt == TIO_F32 && radius[1] > 0 && radius[2] > 0 && radius[1] <= kConvMaxRadiusV4 && radius[2] <= 8 &&
                       shape[2] <= 256 && (shape[2] & 3) == 0 && !env_switches().conv_no_fuse && io_aligned;
  if (bias_on || noise_on != 0) {
    // the pointwise stages ride on the marching I pass (loads) and the fused J+K pass (stores)
    const bool ok = dt == TIO_F32 && n_active == 3 && fuse_jk && radius[0] <= kConvMaxRadiusV4 && !has_skip && io_aligned;
    if (!ok) return TIO_ERR_UNSUPPORTED_CONFIG;
  }
  const int bcs = batch * channels;
  int n_passes = 0;
  unsigned src_bit = kAlignedX;
  for (int s = 0; s < n_active; s++) {
    const int axis = active[s];
    if (axis == 2 && fuse_jk) break;  // done by the J pass
    const bool first = s == 0, last = s == n_active - 1 || (axis == 1 && fuse_jk);
    const unsigned dst_bit = last ? kAlignedY : ((s % 2 == 0) ? kAlignedTmp0 : kAlignedTmp1);
    tio_conv_pass& p = out[n_passes++];
    p = tio_conv_pass{};
    p.axis = axis; p.radius = radius[axis]; p.last = last ? 1 : 0;
    const int ntaps = 2 * radius[axis] + 1;
    unsigned gx, gy, gz;
    size_t lds;
    if (axis == 2) {
      p.family = TIO_CONV_K;
      gx = (shape[2] + kConvKSpan - 1) / kConvKSpan; gy = (shape[1] + 3) / 4; gz = static_cast<unsigned>(shape[0]) * bcs;
      lds = (((ntaps + 3) & ~3) + 4 * (kConvKSpan + 2 * radius[axis])) * sizeof(float);
    } else {
      const int n = shape[axis], other = axis == 0 ? shape[1] : shape[0];
      p.family = TIO_CONV_LINE;
      gx = (shape[2] + 63) / 64; gy = (n + kConvLine - 1) / kConvLine; gz = static_cast<unsigned>(other) * bcs;
      lds = (((ntaps + 3) & ~3) + (kConvLine + 2 * radius[axis]) * 64) * sizeof(float);
      p.segments = static_cast<int32_t>(gy); p.rows_per_segment = kConvLine;
    }
    // (the limit of the generic kernels' grid holds for every family: one rule, whatever the pointers' alignment)
    if (gz > 65535u || gy > 65535u) return TIO_ERR_INVALID_ARGUMENT;
    const bool f32_pass = (first ? dt == TIO_F32 : true) && (last ? dt == TIO_F32 : true);
    const bool pass_aligned = ((shape[2] & 3) == 0) && (aligned & (src_bit | dst_bit | kAlignedX)) == (src_bit | dst_bit | kAlignedX);
    if (f32_pass && pass_aligned && radius[axis] <= kConvMaxRadiusV4) {  // 16-byte access fast paths
      if (axis == 2) {
        const int r4 = std::max((radius[axis] + 3) & ~3, 8);
        p.family = TIO_CONV_K_V4;
        lds = (((ntaps + 3) & ~3) + 4 * (2 * kConvKSpan + 2 * r4)) * sizeof(float);
        gy = static_cast<unsigned>((shape[1] + 4 * kConvKRows - 1) / (4 * kConvKRows));
      } else {
        // one or two marching segments per line: enough blocks to fill the chip, halo re-read only at the cut
        const int n = shape[axis], other = axis == 0 ? shape[1] : shape[0];
        const int64_t lines = static_cast<int64_t>((shape[2] + 255) / 256) * other * bcs;
        int segs = lines >= 4096 ? 1 : (lines >= 2048 ? 2 : 4);
        int seg_len = ((n + segs - 1) / segs + kConvStep - 1) / kConvStep * kConvStep;
        segs = (n + seg_len - 1) / seg_len;
        gx = static_cast<unsigned>((shape[2] + 255) / 256);
        gy = static_cast<unsigned>(segs);
        const bool fused = axis == 1 && fuse_jk;
        p.radius_k = fused ? radius[2] : 0;
        p.pre_bias = (axis == 0 && bias_on) ? 1 : 0;
        p.post_noise = fused ? noise_on : 0;
        // (the bias variant needs > 240 VGPRs beyond radius 6: the LDS ring kernel is the better choice there)
        if (radius[axis] <= (p.pre_bias ? 6 : kMarchMaxRadius) && !env_switches().conv_ring) {
          // register-window marching: one strip per wave, enough segments for >= 8 waves per SIMD
          p.family = TIO_CONV_MARCH;
          p.radius_class = std::min(radius[axis], kMarchMaxRadius);
          p.fma = fma ? 1 : 0;
          const int64_t strips = lines;
          int want = static_cast<int>((8192 + strips - 1) / strips);
          want = std::max(1, std::min(want, std::max(1, n / 32)));
          const int len = (n + want - 1) / want;
          gy = static_cast<unsigned>((n + len - 1) / len);
          gz = static_cast<unsigned>((static_cast<int64_t>(other) * bcs + kBlock / 64 - 1) / (kBlock / 64));
          lds = fused ? 4 * 272 * sizeof(float) : 0;
        } else {
          p.family = TIO_CONV_RING;
          lds = (((ntaps + 3) & ~3) + (2 * kConvStep + 2 * radius[axis]) * 256 + (fused ? 4 * 272 : 0)) * sizeof(float);
        }
        // the kernels cut the line themselves, into gridDim.y segments of ceil(n / gridDim.y) rows
        p.segments = static_cast<int32_t>(gy);
        p.rows_per_segment = static_cast<int32_t>((n + gy - 1) / gy);
      }
    }
    p.grid[0] = static_cast<int32_t>(gx); p.grid[1] = static_cast<int32_t>(gy); p.grid[2] = static_cast<int32_t>(gz);
    p.k_tiles = static_cast<int32_t>(gx);
    p.lds_bytes = static_cast<int32_t>(lds);
    src_bit = dst_bit;
  }
  return n_passes;
}

template <int DT>
static int launch_conv(const void* x, void* y, float* tmp0, float* tmp1, int32_t batch, int32_t channels,
                       const int32_t shape[3], const float* taps, int taps_batched, int tap_stride,
                       const int32_t radius[3], const uint8_t* skip, hipStream_t stream, const ConvFuse& fuse = ConvFuse()) {
  tio_conv_pass passes[3];
  const int n_passes = plan_conv(DT, batch, channels, shape, radius, conv_alignment(x, y, tmp0, tmp1), skip != nullptr,
                                 fuse.bias_coarse != nullptr, fuse.noise_on, fuse.fma != 0, passes);
  if (n_passes == TIO_ERR_INVALID_ARGUMENT) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d: volume too large for one launch");
  if (n_passes < 0) return n_passes;
  const void* src = x;
  for (int s = 0; s < n_passes; s++) {
    const tio_conv_pass& p = passes[s];
    const int axis = p.axis;
    const bool first = s == 0, last = p.last != 0;
    void* dst = last ? y : static_cast<void*>((s % 2 == 0) ? tmp0 : tmp1);
    ConvArgs a{};
    a.src = src; a.dst = dst; a.x_orig = x; a.taps = taps; a.skip = skip;
    a.I = shape[0]; a.J = shape[1]; a.K = shape[2];
    a.channels = channels; a.axis = axis; a.radius = p.radius;
    a.taps_batched = taps_batched; a.tap_stride = tap_stride; a.orig_dtype = DT; a.last_pass = last ? 1 : 0;
    a.radius_k = p.radius_k;
    const dim3 grid(static_cast<unsigned>(p.grid[0]), static_cast<unsigned>(p.grid[1]), static_cast<unsigned>(p.grid[2]));
    const size_t lds = static_cast<size_t>(p.lds_bytes);
    const bool fused = p.radius_k > 0, pre_bias = p.pre_bias != 0, post_noise = p.post_noise != 0, noise_base = p.post_noise == 2;
    if (pre_bias) {
      a.bias_coarse = fuse.bias_coarse;
      a.bias_ci = fuse.bias_shape[0]; a.bias_cj = fuse.bias_shape[1]; a.bias_ck = fuse.bias_shape[2];
      a.bias_si = lerp_scale(a.bias_ci, shape[0]); a.bias_sj = lerp_scale(a.bias_cj, shape[1]); a.bias_sk = lerp_scale(a.bias_ck, shape[2]);
    }
    if (post_noise) {
      a.noise_on = fuse.noise_on; a.noise_base = fuse.noise_base; a.noise_batched = fuse.noise_batched; a.noise_mean = fuse.noise_mean; a.noise_std = fuse.noise_std;
      a.noise_mean_b = fuse.noise_mean_b; a.noise_std_b = fuse.noise_std_b; a.noise_seed = fuse.noise_seed;
    }
    switch (p.family) {
      case TIO_CONV_K_V4:
        hipLaunchKernelGGL(conv_k_v4_kernel, grid, dim3(kBlock), lds, stream, a);
        break;
      case TIO_CONV_MARCH: {
        a.bcs = batch * channels;
        a.fma = p.fma;
        // cache policy of this pass (common.hpp: launch_streams): a marching pass writes every float32 voxel of the batch once
        const bool streams = launch_streams(static_cast<int64_t>(a.bcs) * shape[0] * shape[1] * shape[2] * static_cast<int64_t>(sizeof(float)));
        if (fused) {  // the fused J + K instantiations are built in a translation unit of their own (stencil_fused.hip)
          launch_conv_march_fused(p.radius_class, p.post_noise, p.fma != 0, streams, grid, lds, stream, a);
          break;
        }
        with_march_radius(p.radius_class, [&](auto radius_tag) {
          with_bools([&](auto bias, auto fm) {
            constexpr int R = decltype(radius_tag)::value;
            if (streams) hipLaunchKernelGGL((conv_stream_march_kernel<R, false, decltype(bias)::value, 0, decltype(fm)::value>), grid, dim3(kBlock), lds, stream, a);
            else hipLaunchKernelGGL((conv_march_kernel<R, false, decltype(bias)::value, 0, decltype(fm)::value>), grid, dim3(kBlock), lds, stream, a);
          }, pre_bias, p.fma != 0);
        });
        break;
      }
      case TIO_CONV_RING: {
#define TIO_LINE_LAUNCH(FK, PB, PN)                                                                                   \
  {                                                                                                                   \
    auto kern = conv_line_v4_kernel<FK, PB, PN>;                                                                      \
    if (lds > 48 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                               static_cast<int>(lds)) != hipSuccess)                                  \
      return fail(TIO_ERR_LAUNCH, "tio_separable_conv3d: cannot reserve %zu bytes of LDS", lds);                       \
    hipLaunchKernelGGL(kern, grid, dim3(kBlock), lds, stream, a);                                                      \
  }
        if (fused && noise_base) TIO_LINE_LAUNCH(true, false, 2)
        else if (fused && post_noise) TIO_LINE_LAUNCH(true, false, 1)
        else if (fused) TIO_LINE_LAUNCH(true, false, 0)
        else if (pre_bias) TIO_LINE_LAUNCH(false, true, 0)
        else TIO_LINE_LAUNCH(false, false, 0)
#undef TIO_LINE_LAUNCH
        break;
      }
      default: {  // the generic kernels: any dtype, any alignment
#define TIO_CONV_LAUNCH(S, D)                                                                      \
  do {                                                                                             \
    if (axis == 2) hipLaunchKernelGGL((conv_k_kernel<S, D>), grid, dim3(kBlock), lds, stream, a);  \
    else hipLaunchKernelGGL((conv_line_kernel<S, D>), grid, dim3(kBlock), lds, stream, a);         \
  } while (0)
        if (first && last) TIO_CONV_LAUNCH(DT, DT);
        else if (first) TIO_CONV_LAUNCH(DT, TIO_F32);
        else if (last) TIO_CONV_LAUNCH(TIO_F32, DT);
        else TIO_CONV_LAUNCH(TIO_F32, TIO_F32);
#undef TIO_CONV_LAUNCH
        break;
      }
    }
    src = dst;
  }
  return check_launch("tio_separable_conv3d");
}

}  // namespace tio

using namespace tio;

extern "C" int tio_separable_conv3d(const void* x, void* y, void* tmp, int32_t dtype, int32_t batch,
                                    int32_t channels, const int32_t shape[3], const float* taps_dev,
                                    int32_t taps_batched, int32_t tap_stride, const int32_t radius[3],
                                    const uint8_t* skip_dev, void* stream) {
  if (batch == 0) return TIO_OK;  // an empty batch has no data pointers to speak of
  if (x == nullptr || y == nullptr || shape == nullptr || radius == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d: null argument");
  if (!is_float_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_separable_conv3d: dtype %d", dtype);
  if (batch < 0 || channels < 1 || shape[0] < 1 || shape[1] < 1 || shape[2] < 1)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d: bad shape");
  int n_active = 0;
  for (int a = 0; a < 3; a++) {
    if (radius[a] < 0 || 2 * radius[a] + 1 > tap_stride)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d: radius[%d]=%d does not fit tap_stride=%d", a,
                  radius[a], tap_stride);
    if (radius[a] > kMaxRadius) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d: radius[%d]=%d exceeds %d", a, radius[a], kMaxRadius);
    if (radius[a] > 0) n_active++;
  }
  if (n_active > 0 && taps_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d: null taps");
  const int64_t n = static_cast<int64_t>(shape[0]) * shape[1] * shape[2];
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (batch == 0) return TIO_OK;
  if (n_active == 0) {  // every sigma <= 0: identity (blur.py:144-145)
    if (hipMemcpyAsync(y, x, static_cast<size_t>(batch) * channels * n * dtype_size(dtype), hipMemcpyDeviceToDevice, s) !=
        hipSuccess)
      return fail(TIO_ERR_LAUNCH, "tio_separable_conv3d: copy failed");
    return TIO_OK;
  }
  if (n_active > 1 && tmp == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d: tmp is required when more than one axis is active");
  float* tmp0 = static_cast<float*>(tmp);
  float* tmp1 = tmp0 != nullptr ? tmp0 + static_cast<int64_t>(batch) * channels * n : nullptr;
  int status = TIO_OK;
  const bool known = dispatch_float_dtype(dtype, [&](auto dt) {
    status = launch_conv<decltype(dt)::value>(x, y, tmp0, tmp1, batch, channels, shape, taps_dev, taps_batched, tap_stride, radius, skip_dev, s);
  });
  return known ? status : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_separable_conv3d: dtype %d", dtype);
}

extern "C" int tio_separable_conv3d_passes(int32_t dtype, int32_t batch, int32_t channels, const int32_t shape[3],
                                           const int32_t radius[3], int32_t aligned16, int32_t has_skip, int32_t bias_on,
                                           int32_t noise_on, int32_t fast_math, tio_conv_pass out_passes[3]) {
  if (shape == nullptr || radius == nullptr || out_passes == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_passes: null argument");
  if (!is_float_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_separable_conv3d_passes: dtype %d", dtype);
  if (batch < 0 || channels < 1 || shape[0] < 1 || shape[1] < 1 || shape[2] < 1)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_passes: bad shape");
  for (int a = 0; a < 3; a++)
    if (radius[a] < 0 || radius[a] > kMaxRadius)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_passes: radius[%d]=%d is not in 0 .. %d", a, radius[a], kMaxRadius);
  if (noise_on < 0 || noise_on > 2) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_passes: noise_on must be 0, 1 or 2");
  if (batch == 0) return 0;
  const bool stages = bias_on != 0 || noise_on != 0 || fast_math != 0;  // the caller asks about tio_blur_fused
  if (stages && (dtype != TIO_F32 || aligned16 == 0)) return TIO_ERR_UNSUPPORTED_CONFIG;
  const unsigned aligned = aligned16 != 0 ? (kAlignedX | kAlignedY | kAlignedTmp0 | kAlignedTmp1) : 0u;
  const int n_passes = plan_conv(dtype, batch, channels, shape, radius, aligned, has_skip != 0, bias_on != 0, noise_on, fast_math != 0, out_passes);
  if (n_passes == TIO_ERR_INVALID_ARGUMENT) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_passes: volume too large for one launch");
  return n_passes;
}

// =============================================================================
// Backward of the replicate-padded separable correlation (ABI 16)
// =============================================================================
// y[p] = sum_t w[t] x[clamp(p + t - r)] along one axis.  Its transpose as a GATHER (one thread per element of gx, lanes along K):
// gx[m] = sum_p gy[p] W(p, m), W(p, m) = the taps t with clamp(p + t - r) == m — for every p within r of m the one tap
// t = m - p + r, and on the two border voxels also every tap that was clamped onto them: m == 0 collects t < r - p of
// p = 0 .. r - 1, m == n - 1 collects t > n - 1 - p + r of p = n - r .. n - 1.  Off the hot path (nobody trains through a
// Gaussian blur in the pipeline of BASELINE.json): plain global loads, float32 accumulation in ascending p.
struct ConvAdjointArgs {
  const float* gy;
  float* gx;
  const float* taps;  // (1|B, 3, tap_stride)
  const uint8_t* skip;
  int64_t n_spatial, n_total, stride;
  int channels, extent, r, axis, tap_stride, taps_batched, J, K;
};

__global__ __launch_bounds__(kBlock) void conv_axis_adjoint_kernel(const ConvAdjointArgs a) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= a.n_total) return;
  const int b = static_cast<int>(e / (a.n_spatial * a.channels));
  if (a.skip != nullptr && a.skip[b] != 0) {
    a.gx[e] = a.gy[e];
    return;
  }
  const int64_t v = e % a.n_spatial;
  const int k = static_cast<int>(v % a.K), j = static_cast<int>((v / a.K) % a.J), i = static_cast<int>(v / (static_cast<int64_t>(a.K) * a.J));
  const int m = a.axis == 0 ? i : (a.axis == 1 ? j : k);
  const int n = a.extent, r = a.r;
  const float* w = a.taps + (a.taps_batched ? static_cast<int64_t>(b) * 3 * a.tap_stride : 0) + static_cast<int64_t>(a.axis) * a.tap_stride;
  const float* line = a.gy + (e - static_cast<int64_t>(m) * a.stride);
  float acc = 0.0f;
  const int lo = max(0, m - r), hi = min(n - 1, m + r);
  for (int p = lo; p <= hi; p++) acc = __builtin_fmaf(w[m - p + r], line[static_cast<int64_t>(p) * a.stride], acc);
  if (m == 0) {  // taps clamped onto the first voxel
    for (int p = 0; p <= min(r - 1, n - 1); p++) {
      float clamped = 0.0f;
      for (int t = 0; t < r - p; t++) clamped += w[t];
      acc = __builtin_fmaf(clamped, line[static_cast<int64_t>(p) * a.stride], acc);
    }
  }
  if (m == n - 1) {  // ... onto the last
    for (int p = max(0, n - r); p <= n - 1; p++) {
      float clamped = 0.0f;
      for (int t = n - p + r; t <= 2 * r; t++) clamped += w[t];
      acc = __builtin_fmaf(clamped, line[static_cast<int64_t>(p) * a.stride], acc);
    }
  }
  a.gx[e] = acc;
}

extern "C" int tio_separable_conv3d_adjoint(const float* gy, float* gx, float* tmp, int32_t batch, int32_t channels,
                                            const int32_t shape[3], const float* taps_dev, int32_t taps_batched,
                                            int32_t tap_stride, const int32_t radius[3], const uint8_t* skip_dev, void* stream) {
  if (batch == 0) return TIO_OK;
  if (gy == nullptr || gx == nullptr || shape == nullptr || radius == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_adjoint: null argument");
  if (batch < 0 || channels < 1 || shape[0] < 1 || shape[1] < 1 || shape[2] < 1)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_adjoint: bad shape");
  int n_active = 0;
  for (int a = 0; a < 3; a++) {
    if (radius[a] < 0 || 2 * radius[a] + 1 > tap_stride)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_adjoint: radius[%d]=%d does not fit tap_stride=%d", a, radius[a], tap_stride);
    if (radius[a] > 0) n_active++;
  }
  if (n_active > 0 && taps_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_adjoint: null taps");
  if (n_active > 1 && tmp == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_adjoint: tmp is required when more than one axis is active");
  const int64_t n = static_cast<int64_t>(shape[0]) * shape[1] * shape[2];
  const int64_t total = static_cast<int64_t>(batch) * channels * n;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_active == 0) {
    if (hipMemcpyAsync(gx, gy, static_cast<size_t>(total) * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return fail(TIO_ERR_LAUNCH, "tio_separable_conv3d_adjoint: copy failed");
    return TIO_OK;
  }
  if ((total + kBlock - 1) / kBlock > 0x7FFFFFFF) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_separable_conv3d_adjoint: tensor too large");
  // the forward pass runs I, J, K: the transposes run K, J, I; the last one writes gx
  const float* src = gy;
  int pass = 0;
  for (int axis = 2; axis >= 0; axis--) {
    if (radius[axis] <= 0) continue;
    float* dst = ((n_active - 1 - pass) % 2 == 0) ? gx : tmp;
    ConvAdjointArgs a;
    a.gy = src; a.gx = dst; a.taps = taps_dev; a.skip = skip_dev;
    a.n_spatial = n; a.n_total = total;
    a.stride = axis == 0 ? static_cast<int64_t>(shape[1]) * shape[2] : (axis == 1 ? shape[2] : 1);
    a.channels = channels; a.extent = shape[axis]; a.r = radius[axis]; a.axis = axis; a.tap_stride = tap_stride;
    a.taps_batched = taps_batched; a.J = shape[1]; a.K = shape[2];
    hipLaunchKernelGGL(conv_axis_adjoint_kernel, dim3(static_cast<unsigned>((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
    src = dst;
    pass++;
  }
  return check_launch("tio_separable_conv3d_adjoint");
}

extern "C" int tio_blur_fused(const void* x, void* y, void* tmp, int32_t dtype, int32_t batch, int32_t channels,
                              const int32_t shape[3], const float* taps_dev, int32_t taps_batched, int32_t tap_stride,
                              const int32_t radius[3], const float* bias_coarse_dev, const int32_t bias_coarse_shape[3],
                              int32_t noise_on, float noise_mean, float noise_std, const float* noise_mean_dev,
                              const float* noise_std_dev, int32_t noise_batched, uint64_t philox_seed, const float* noise_base_dev,
                              int32_t fast_math, void* stream) {
  if (batch == 0) return TIO_OK;
  if (x == nullptr || y == nullptr || tmp == nullptr || shape == nullptr || radius == nullptr || taps_dev == nullptr)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_blur_fused: null argument");
  if (dtype != TIO_F32) return TIO_ERR_UNSUPPORTED_CONFIG;
  if (batch < 0 || channels < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_blur_fused: bad batch/channels");
  for (int d = 0; d < 3; d++) {
    if (shape[d] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_blur_fused: shapes must be >= 1");
    if (radius[d] < 0 || radius[d] > kMaxRadius || 2 * radius[d] + 1 > tap_stride)
      return fail(TIO_ERR_INVALID_ARGUMENT, "tio_blur_fused: bad radius");
  }
  if (bias_coarse_dev != nullptr) {
    if (bias_coarse_shape == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_blur_fused: null coarse shape");
    for (int d = 0; d < 3; d++)
      if (bias_coarse_shape[d] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_blur_fused: bad coarse shape");
  }
  if (noise_on && noise_batched && (noise_mean_dev == nullptr || noise_std_dev == nullptr))
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_blur_fused: batched noise needs mean_dev and std_dev");
  if (noise_on < 0 || noise_on > 2) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_blur_fused: noise_on must be 0, 1 or 2");
  if (noise_on == 2 && noise_base_dev == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_blur_fused: noise_on == 2 needs noise_base_dev");
  if (noise_on == 2 && (reinterpret_cast<uintptr_t>(noise_base_dev) & 15) != 0) return TIO_ERR_UNSUPPORTED_CONFIG;
  // (the header's contract, with or without a stage riding along: launch_conv itself asks only when one does)
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(tmp)) & 15) != 0) return TIO_ERR_UNSUPPORTED_CONFIG;
  if (batch == 0) return TIO_OK;
  const int64_t n = static_cast<int64_t>(shape[0]) * shape[1] * shape[2];
  ConvFuse fuse;
  fuse.bias_coarse = bias_coarse_dev;
  if (bias_coarse_dev != nullptr)
    for (int d = 0; d < 3; d++) fuse.bias_shape[d] = bias_coarse_shape[d];
  fuse.noise_on = noise_on; fuse.noise_batched = noise_batched; fuse.noise_mean = noise_mean; fuse.noise_std = noise_std;
  fuse.noise_mean_b = noise_mean_dev; fuse.noise_std_b = noise_std_dev; fuse.noise_seed = philox_seed;
  fuse.noise_base = noise_on == 2 ? noise_base_dev : nullptr;
  fuse.fma = fast_math != 0;
  float* tmp0 = static_cast<float*>(tmp);
  float* tmp1 = tmp0 + static_cast<int64_t>(batch) * channels * n;
  const int status = launch_conv<TIO_F32>(x, y, tmp0, tmp1, batch, channels, shape, taps_dev, taps_batched, tap_stride, radius, nullptr,
                                          static_cast<hipStream_t>(stream), fuse);
  return status;
}
