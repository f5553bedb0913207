// Nearest-neighbour images without a fill rule (label maps, masks): their own kernel, bit-identical to the exact
// coordinate chain at a fraction of its cost.
//
// Reference: `_sample_batch_grid_sample(..., mode="nearest")` -> F.grid_sample(padding_mode="zeros", align_corners=True)
// (transforms/spatial/spatial.py:1695-1731): the value of the input voxel at nearbyint(coordinate) per axis, zero
// outside.  The result depends on the coordinate only through three roundings, so the float32 op sequence of the
// reference's chain (affine_grid-style matmul, field upsampling, normalise / un-normalise: ~115 vector instructions per
// voxel with control points) matters only where a coordinate lies within rounding error of a half-integer.  The kernel
//   1. evaluates the FAST coordinate line of the column (resample_line.hpp: one fma per axis and plane),
//   2. takes the voxel as decided when on every axis |x - rint(x)| <= 1/2 - margin, margin = kNearestEps (row + S + |x|)
//      with row = sum |m_rc| S_out,c + |m_r3| (every partial sum of the reference's matmul is below it) — the rounding, and
//      the in-bounds test (it flips at -1/2 and S - 1/2: half-integers too), are then the same for any coordinate within
//      `margin` of x; the FAST and the exact coordinate differ by less than a tenth of it (bound and measurement:
//      DESIGN.md section 4.1b),
//   3. re-evaluates the few undecided voxels of the column with the exact chain (exact_voxel_coords, resample_exact_chain.hpp: the
//      operation sequence of resample_kernel, which tests/ pin against the oracle and the reference's golden vectors).
// One load per voxel straight from global memory (no LDS: a nearest image has no taps to share), element size 1 / 2 / 4 / 8
// bytes copied as bits, every image and channel of the launch that has that size.
#pragma once
#include "resample_coords.hpp"
#include "resample_exact_chain.hpp"
#include "resample_tile.hpp"
#include "resample_line.hpp"
#include "resample_plan.hpp"
#include "resample_lean_exact.hpp"

namespace tio {

constexpr float kNearestEps = 1e-6f;  // decision margin per unit of magnitude (~16 float32 ulps)

struct NearestImg {
  const void* in;
  void* out;
  int channels, es;   // es: bytes per element
  const float* fill;  // per-channel fill values (float32, `.to(dtype)` on store) or nullptr: no fill rule
  int dtype;          // only read to convert the fill value
};

// what the kernel needs of a launch (ResampleArgs carries 1 KiB of image descriptors for the other kernels)
struct NearestArgs {
  int B, I, J, K, Io, Jo, Ko, affine_first;
  const float* mapping;
  const float* cp;
  const uint8_t* cp_skip;
  const uint8_t* passthrough;
  int mapping_batched, cp_batched, ni, nj, nk, unit_spacing;
  float sp[3], rsp[3];
  float scale_i, scale_j, scale_k;
  float den[3], rden[3], size_m1[3];
  float ratio[3];  // (S - 1) / max(S_norm - 1, 1) per axis: the FAST line works in voxels of the image's own grid
  float dh[3], rdh[3], half_h[3];  // resample_nearest_exact_kernel: the folded normalise round trip (den / 2, its reciprocal, (S - 1) / 2)
  int tiles_k, tiles_j, tiles_i;
  unsigned magic_k, magic_j, magic_i;
  float eps;       // kNearestEps (TIO_NEAREST_EPS: calibration runs)
  int any_fill;    // an image of the launch has a fill rule: the in-bounds weight is decided as well
  int n_images;
  NearestImg img[TIO_MAX_IMAGES];
};

template <int ES> struct NearestCarrier { typedef uint32_t type; };  // what a loaded element travels in (a whole register)
template <> struct NearestCarrier<8> { typedef uint64_t type; };

// nearbyint per axis (round half to even: v_rndne_f32), zero padding: offset of the source voxel, or -1
__device__ __forceinline__ int nearest_offset(float x, float y, float z, float hx, float hy, float hz, int J, int K) {
  const float xn = rintf(x), yn = rintf(y), zn = rintf(z);
  const bool ok = (xn >= 0.0f) & (xn <= hx) & (yn >= 0.0f) & (yn <= hy) & (zn >= 0.0f) & (zn <= hz);  // NaN fails
  return ok ? (static_cast<int>(xn) * J + static_cast<int>(yn)) * K + static_cast<int>(zn) : -1;
}

// (a * b + c on 24-bit operands: one full-rate instruction; written out because the compiler turns __mul24(a, b) + c
// with a scalar b into the quarter-rate v_mad_u64_u32).  UNSIGNED 24-bit multiplicands: the offsets are only used for
// taps inside the volume (indices >= 0), and the inner product ix * J + iy runs up to I * J - 1 < 2^24 — the signed
// form (v_mad_i32_i24, multiplicands in [-2^23, 2^23)) sign-extended it from 2^23 on and sent the "decided" voxels
// of such a region to offset < 0, i.e. to 0 (tests/test_gpu_nearest_kernel.py::test_plane_larger_than_2_23).
__device__ __forceinline__ int mad24(int a, int b, int c) {
  int r;
  asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// a fill value as the bits of an element of `dtype` (what Elem<DT>::store writes: integers truncate towards zero)
template <int ES>
__device__ __forceinline__ typename NearestCarrier<ES>::type nearest_fill_bits(int dtype, float v) {
  if constexpr (ES == 8) {
    return dtype == TIO_F64 ? static_cast<uint64_t>(__double_as_longlong(static_cast<double>(v))) : static_cast<uint64_t>(static_cast<int64_t>(v));
  } else if constexpr (ES == 4) {
    return dtype == TIO_F32 ? __float_as_uint(v) : static_cast<uint32_t>(static_cast<int32_t>(static_cast<int64_t>(v)));
  } else if constexpr (ES == 2) {
    if (dtype == TIO_F16) { const _Float16 h = static_cast<_Float16>(v); uint16_t bits; __builtin_memcpy(&bits, &h, 2); return bits; }
    if (dtype == TIO_BF16) return float_to_bf16_bits(v);
    return static_cast<uint16_t>(static_cast<int16_t>(static_cast<int64_t>(v)));
  } else {
    return static_cast<uint8_t>(static_cast<int64_t>(v));
  }
}

// Images WITH a fill rule (round 4; a label map with `default_pad_label` != 0): the reference keeps the sampled value where the
// in-bounds weight of the TRILINEAR taps exceeds 1/2 and stores the fill value elsewhere (spatial.py:1719-1728: the mask is
// always trilinear).  Same scheme as for the index: the FAST line's weight decides unless it lies within a margin of 1/2
// (fast_fill_margin, resample_exact_chain.hpp), the exact chain re-decides the rest.  Bit `t` of `usefill` = plane t stores
// the fill value in every image that has one.  Until round 4 such an image stayed with the float images of its call and
// pinned all of them to the exact kernels (VERDICT r3 missing #5).
//
// One block per 16 x TJ x TK brick of the output (TJ * TK = 256), one column of 16 planes per thread: 16 x 4 x 64 — a wave
// is one output row of 64 voxels: its loads touch one or two cache lines and its stores are contiguous — or 16 x 16 x 16
// for volumes narrower than that.  The host only launches it for I * J <= 2^24 and K < 2^24 (unsigned 24-bit multiply-adds).
template <bool ELASTIC_POSSIBLE, int ES, int TJ, int TK, int TI>
__global__ __launch_bounds__(256) void resample_nearest_kernel(const NearestArgs a) {
  typedef typename RawBits<ES>::type bits_t;
  static_assert(TJ * TK == 256 && (TK & (TK - 1)) == 0 && (TI == 16 || TI == 32), "one thread per column of the brick");
  // (TI = 32 — the prologue spread over twice the voxels — was measured: 128 VGPRs, four waves per SIMD; int16 + elastic
  //  0.330 -> 0.313 ms, uint8 affine 0.246 -> 0.365 ms: the launch code instantiates 16 only)
  constexpr int G = 4;
  {  // the arguments everything below starts from, requested together (left alone the compiler fetches each one right
     // before its first use: a dozen dependent round trips through the scalar cache)
    const float* mp = a.mapping; const uint8_t* pp = a.passthrough; const float* cpp = a.cp;
    asm volatile("" ::"s"(a.tiles_k), "s"(a.tiles_j), "s"(a.tiles_i), "s"(a.magic_k), "s"(a.magic_j), "s"(a.magic_i), "s"(mp), "s"(pp), "s"(cpp),
                 "s"(a.mapping_batched), "s"(a.Io), "s"(a.Jo), "s"(a.Ko), "s"(a.I), "s"(a.J), "s"(a.K), "s"(a.eps), "s"(a.n_images));
  }
  const unsigned tile = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned t1 = fastdiv_exact(tile, a.magic_k, a.tiles_k);
  const int kt = tile - t1 * a.tiles_k;
  const unsigned t2 = fastdiv_exact(t1, a.magic_j, a.tiles_j);
  const int jt = t1 - t2 * a.tiles_j;
  const unsigned t3 = fastdiv_exact(t2, a.magic_i, a.tiles_i);
  const int it = t2 - t3 * a.tiles_i;
  const int b = t3;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int tk = tid & (TK - 1), tj = tid / TK;
  const int i_begin = it * TI, j_lo = jt * TJ, k_lo = kt * TK;
  const int i_count = min(TI, a.Io - i_begin), nv = min(TJ, a.Jo - j_lo), nw = min(TK, a.Ko - k_lo);
  const bool col_active = (tj < nv) & (tk < nw);
  const int jv = min(tj, nv - 1), kw = min(tk, nw - 1);  // idle threads shadow the last column (they never store)
  const int jo = j_lo + jv, ko = k_lo + kw;
  const int64_t n_in = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t n_out = static_cast<int64_t>(a.Io) * a.Jo * a.Ko;
  const int slab = a.Jo * a.Ko;
  const int64_t col = static_cast<int64_t>(i_begin) * slab + static_cast<int64_t>(jo) * a.Ko + ko;  // first voxel of the column

  if (a.passthrough != nullptr && a.passthrough[b] != 0) {  // gated-out element: bit-exact copy (spatial.py:1101-1106)
    if (col_active) {
      for (int im = 0; im < a.n_images; im++) {
        const NearestImg& g = a.img[im];
        if (g.es != ES) continue;
        for (int c = 0; c < g.channels; c++) {
          const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
          const bits_t* src = static_cast<const bits_t*>(g.in) + bc * n_out + col;
          bits_t* dst = static_cast<bits_t*>(g.out) + bc * n_out + col;
          for (int t = 0; t < i_count; t++) dst[static_cast<int64_t>(t) * slab] = src[static_cast<int64_t>(t) * slab];
        }
      }
    }
    return;
  }

  // the element's mapping: raw for the exact chain, rows scaled by the axis ratios for the FAST line
  float m[12];
  {
    const float* mp = a.mapping + (a.mapping_batched ? b * 12 : 0);
#pragma unroll
    for (int q = 0; q < 12; q++) m[q] = mp[q];
  }
  FastFrameG f;
#pragma unroll
  for (int q = 0; q < 12; q++) f.m[q] = m[q] * a.ratio[q >> 2];
  f.affine_first = a.affine_first != 0;
  f.ni = a.ni; f.nj = a.nj; f.nk = a.nk; f.sci = a.scale_i; f.scj = a.scale_j; f.sck = a.scale_k;
  f.elastic = false; f.cp = nullptr;
#pragma unroll
  for (int e = 0; e < 3; e++) f.dsc[e] = a.rsp[e] * (f.affine_first ? a.ratio[e] : 1.0f);
  if constexpr (ELASTIC_POSSIBLE) {
    f.elastic = !(a.cp_skip != nullptr && a.cp_skip[b] != 0);
    f.cp = f.elastic ? a.cp + (a.cp_batched ? static_cast<int64_t>(b) * (a.ni * a.nj * a.nk * 3) : 0) : nullptr;
  }
  pipe_brick_frame(f, j_lo, k_lo);
  float col3[3], lim0[3];
  const float fv = static_cast<float>(jv), fw = static_cast<float>(kw);
  const float eps = a.eps;
#pragma unroll
  for (int r = 0; r < 3; r++) {
    col3[r] = __builtin_fmaf(f.m[4 * r + 1], fv, f.m[4 * r + 2] * fw);
    // 1/2 - eps (row + S): |x - rint(x)| <= lim0 - eps |x| decides the axis (block uniform part)
    const float row = fabsf(m[4 * r]) * static_cast<float>(a.Io) + fabsf(m[4 * r + 1]) * static_cast<float>(a.Jo) +
                      fabsf(m[4 * r + 2]) * static_cast<float>(a.Ko) + fabsf(m[4 * r + 3]);
    // (the mapping works in voxels of the NORMALISING grid; on an image `ratio` times finer its roundings count `ratio` times)
    lim0[r] = 0.5f - eps * (row * fmaxf(1.0f, a.ratio[r]) + a.size_m1[r] + 1.0f);  // (NaN / Inf / huge mapping: NaN or negative — nothing is decided)
  }
  Lerp1D lj{0, 0, 1.0f, 0.0f}, lk{0, 0, 1.0f, 0.0f};
  if constexpr (ELASTIC_POSSIBLE) {
    if (f.elastic) {
      lj = lerp_index(jo, a.nj, a.Jo, a.scale_j);
      lk = lerp_index(ko, a.nk, a.Ko, a.scale_k);
    }
  }
  const float hx = a.size_m1[0], hy = a.size_m1[1], hz = a.size_m1[2];
  const unsigned uhx = static_cast<unsigned>(a.I - 1), uhy = static_cast<unsigned>(a.J - 1), uhz = static_cast<unsigned>(a.K - 1);
  const bool any_fill = a.any_fill != 0;  // (launch uniform)
  // (on an image `ratio` times finer than the normalising grid the chain's roundings count `ratio` times: as for lim0 above)
  const float fill_margin = any_fill ? fast_fill_margin(m, static_cast<float>(a.Io), static_cast<float>(a.Jo), static_cast<float>(a.Ko), hx + 1.0f,
                                                        hy + 1.0f, hz + 1.0f) * fmaxf(1.0f, fmaxf(a.ratio[0], fmaxf(a.ratio[1], a.ratio[2])))
                                     : -1.0f;
  unsigned usefill = 0u;

  const float cj = static_cast<float>(jo), ck = static_cast<float>(ko);
  ColumnPlanes planes;
  planes.cell = -2;
#pragma unroll
  for (int e = 0; e < 3; e++) { planes.P0[e] = 0.0f; planes.P1[e] = 0.0f; }
  float C3[3];
#pragma unroll
  for (int r = 0; r < 3; r++) C3[r] = static_cast<float>(static_cast<double>(f.m[4 * r]) * i_begin + f.c[r]);

  // ---- 1 + 2: the FAST line, four planes at a time; undecided planes are remembered -------------------------------------
  // A line holds inside one control cell, and sixteen planes lie in one cell or two (three with control grids denser than
  // a brick: the planes of the third are left to the exact chain).  Both lines are fetched up front; a group of four
  // planes takes the line of its cell, the one group a cell boundary falls into selects plane by plane.  (Leaving the
  // planes behind a boundary to the exact chain, as the first version did, cost a fifth of the kernel's instructions:
  // every lane of a wave shares the boundary, 38 % of the bricks have one, and the chain is ten times the FAST line.)
  int offs[TI];
  unsigned undecided = 0u;
  {
    const int u1 = i_begin + i_count;
    float Aa[3] = {0.0f, 0.0f, 0.0f}, Ba[3] = {0.0f, 0.0f, 0.0f}, Ab[3] = {0.0f, 0.0f, 0.0f}, Bb[3] = {0.0f, 0.0f, 0.0f};
    const int run_a1 = fast_column_line(f, lj, lk, planes, i_begin, u1, i_begin, C3, col3, lane, Aa, Ba);  // (wave uniform: the runs
    int run_b1 = run_a1;                                                                                  //  depend on the plane index only)
    if (run_a1 < u1) run_b1 = fast_column_line(f, lj, lk, planes, run_a1, u1, i_begin, C3, col3, lane, Ab, Bb);
    // margin of a run of planes [s0, s1] on a line: |x| along a line is largest at one of its ends
    auto line_margin = [&](const float (&A3)[3], const float (&B3)[3], float s0, float s1, float& lim, bool& lim_ok) {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const float xa = __builtin_fmaf(s0, B3[r], A3[r]), xb = __builtin_fmaf(s1, B3[r], A3[r]);
        const float l = __builtin_fmaf(-eps, fmaxf(fabsf(xa), fabsf(xb)), lim0[r]);
        lim_ok &= l >= 0.0f;  // NaN / Inf in the mapping or the line, coordinates far beyond float32's integers: false
        lim = fminf(lim, l);  // (fminf / fmaxf drop a NaN operand: that is what lim_ok is for)
      }
    };
    auto decide = [&](int t, float x, float y, float z, bool in_run, float lim, bool masked) {
      const float xn = rintf(x), yn = rintf(y), zn = rintf(z);
      // (fmaxf would drop a NaN term — but a NaN coordinate means a NaN line, and then lim is -1: undecided)
      bool decided = in_run & (fmaxf(fmaxf(fabsf(x - xn), fabsf(y - yn)), fabsf(z - zn)) <= lim);
      if (masked) {  // (wave uniform) a lane of this group may leave the volume and an image has a fill rule: the in-bounds weight
        FastTaps ts;
        const float x0 = floorf(x), y0 = floorf(y), z0 = floorf(z);
        ts.fx = x - x0; ts.fy = y - y0; ts.fz = z - z0;
        const float mk = fast_mask(ts, x0, y0, z0, hx, hy, hz);
        usefill |= (mk > 0.5f) ? 0u : (1u << t);          // (NaN: fill — and undecided through lim)
        decided &= !(fabsf(mk - 0.5f) <= fill_margin);    // within the margin of the threshold: the exact chain decides
      }
      const int ix = static_cast<int>(xn), iy = static_cast<int>(yn), iz = static_cast<int>(zn);
      const bool ok = (static_cast<unsigned>(ix) <= uhx) & (static_cast<unsigned>(iy) <= uhy) & (static_cast<unsigned>(iz) <= uhz);
      const int off = mad24(mad24(ix, a.J, iy), a.K, iz);
      offs[t] = (decided & ok) ? off : -1;
      undecided |= (decided | (t >= i_count)) ? 0u : (1u << t);
    };
    // does a lane of the wave leave the volume somewhere on planes [s0, s1] of the line (monotone per axis: its two ends tell)?
    auto leaves_volume = [&](const float (&A3)[3], const float (&B3)[3], float s0, float s1) -> bool {
      bool inside = true;
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const float xa = __builtin_fmaf(s0, B3[r], A3[r]), xb = __builtin_fmaf(s1, B3[r], A3[r]);
        const float h = r == 0 ? hx : (r == 1 ? hy : hz);
        inside &= (fminf(xa, xb) >= 0.0f) & (fmaxf(xa, xb) < h);  // (NaN: not inside)
      }
      return __builtin_amdgcn_ballot_w64(!inside) != 0ull;
    };
#pragma unroll
    for (int t0 = 0; t0 < TI; t0 += G) {
      if (t0 < i_count) {  // (block uniform)
        const int p0 = i_begin + t0;
        const bool straddles = (p0 < run_a1) & (p0 + G > run_a1) & (run_a1 < u1);  // (uniform)
        if (!straddles) {
          const bool second = p0 >= run_a1;  // (uniform: the line of this group's cell)
          float A3[3], B3[3];
#pragma unroll
          for (int r = 0; r < 3; r++) { A3[r] = second ? Ab[r] : Aa[r]; B3[r] = second ? Bb[r] : Ba[r]; }
          const int run0 = second ? run_a1 : i_begin, run_end = second ? run_b1 : run_a1;
          const float s0 = static_cast<float>(p0 - run0);
          float lim = 1.0f;
          bool lim_ok = true;
          line_margin(A3, B3, s0, s0 + static_cast<float>(G - 1), lim, lim_ok);
          if (!lim_ok) lim = -1.0f;  // nothing of this group is decided by the FAST line
          const bool masked = any_fill && leaves_volume(A3, B3, s0, s0 + static_cast<float>(G - 1));
#pragma unroll
          for (int q = 0; q < G; q++) {
            const float sq = s0 + static_cast<float>(q);
            decide(t0 + q, __builtin_fmaf(sq, B3[0], A3[0]), __builtin_fmaf(sq, B3[1], A3[1]), __builtin_fmaf(sq, B3[2], A3[2]),
                   p0 + q < run_end, lim, masked);  // (beyond the run: a third cell, or past the last plane of a ragged brick)
          }
        } else {
          const float sa = static_cast<float>(p0 - i_begin);
          float lim = 1.0f;
          bool lim_ok = true;
          line_margin(Aa, Ba, sa, static_cast<float>(run_a1 - 1 - i_begin), lim, lim_ok);
          line_margin(Ab, Bb, 0.0f, static_cast<float>(p0 + G - 1 - run_a1), lim, lim_ok);
          if (!lim_ok) lim = -1.0f;
#pragma unroll
          for (int q = 0; q < G; q++) {
            const bool second = p0 + q >= run_a1;  // (uniform)
            const float sq = static_cast<float>(second ? p0 + q - run_a1 : p0 + q - i_begin);
            decide(t0 + q, __builtin_fmaf(sq, second ? Bb[0] : Ba[0], second ? Ab[0] : Aa[0]),
                   __builtin_fmaf(sq, second ? Bb[1] : Ba[1], second ? Ab[1] : Aa[1]),
                   __builtin_fmaf(sq, second ? Bb[2] : Ba[2], second ? Ab[2] : Aa[2]), p0 + q < run_b1, lim, any_fill);
          }
        }
      } else {
#pragma unroll
        for (int q = 0; q < G; q++) offs[t0 + q] = -1;
      }
    }
  }
  if (!col_active) undecided = 0u;

  // ---- the decided voxels: every image and channel of this element size -------------------------------------------------
  // Sixteen unconditional loads (a voxel without a source reads element 0 and drops it; idle threads shadow a real
  // column), ONE wait, then the stores.  The wait is written out: the stores sit in per-lane conditionals, and after
  // such a join the compiler no longer knows what is outstanding — it would put s_waitcnt vmcnt(0) in front of every
  // store, which also waits for the PREVIOUS store to be acknowledged: sixteen memory round trips per column (measured:
  // 0.35 ms per 8 x 256^3 launch whatever else the kernel did).
  typedef typename NearestCarrier<ES>::type carrier_t;
  for (int im = 0; im < a.n_images; im++) {
    const NearestImg& g = a.img[im];
    if (g.es != ES) continue;
    for (int c = 0; c < g.channels; c++) {
      const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
      const bits_t* __restrict__ src = static_cast<const bits_t*>(g.in) + bc * n_in;
      bits_t* __restrict__ dst = static_cast<bits_t*>(g.out) + bc * n_out + col;
      carrier_t v[TI];
#pragma unroll
      for (int t = 0; t < TI; t++) v[t] = static_cast<carrier_t>(src[max(offs[t], 0)]);
#pragma unroll
      for (int t0 = 0; t0 < TI; t0 += 16)  // (one statement per sixteen registers: an asm takes at most thirty operands)
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(v[t0 + 0]), "+v"(v[t0 + 1]), "+v"(v[t0 + 2]), "+v"(v[t0 + 3]), "+v"(v[t0 + 4]), "+v"(v[t0 + 5]), "+v"(v[t0 + 6]),
                       "+v"(v[t0 + 7]), "+v"(v[t0 + 8]), "+v"(v[t0 + 9]), "+v"(v[t0 + 10]), "+v"(v[t0 + 11]), "+v"(v[t0 + 12]),
                       "+v"(v[t0 + 13]), "+v"(v[t0 + 14]), "+v"(v[t0 + 15]));
      // (the fill value of this channel as element bits; images without a fill rule ignore `usefill`)
      typedef __attribute__((address_space(4))) const float* const_float_ptr;
      const bool has_fill = g.fill != nullptr;
      const carrier_t fillb = has_fill ? nearest_fill_bits<ES>(g.dtype, ((const_float_ptr)g.fill)[c]) : static_cast<carrier_t>(0);
      const unsigned fillmask = has_fill ? usefill : 0u;
#pragma unroll
      for (int t = 0; t < TI; t++)
        if (col_active && t < i_count && !((undecided >> t) & 1u))
          dst[static_cast<int64_t>(t) * slab] =
              ((fillmask >> t) & 1u) ? static_cast<bits_t>(fillb) : (offs[t] >= 0 ? static_cast<bits_t>(v[t]) : static_cast<bits_t>(0));
    }
  }

  // ---- 3: the undecided ones through the exact chain ---------------------------------------------------------------------
  while (__builtin_amdgcn_ballot_w64(undecided != 0u) != 0ull) {
    if (undecided != 0u) {
      const int t = __builtin_ctz(undecided);
      undecided &= undecided - 1u;
      float x, y, z;
      exact_voxel_coords<ELASTIC_POSSIBLE>(a, m, f.elastic, f.cp, lj, lk, i_begin + t, cj, ck, x, y, z);
      const int off = nearest_offset(x, y, z, hx, hy, hz, a.J, a.K);
      const bool keep = !any_fill || exact_fill_mask(x, y, z, hx, hy, hz) > 0.5f;  // (spatial.py:1722-1727: the mask is trilinear)
      for (int im = 0; im < a.n_images; im++) {
        const NearestImg& g = a.img[im];
        if (g.es != ES) continue;
        for (int c = 0; c < g.channels; c++) {
          const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
          const bits_t* src = static_cast<const bits_t*>(g.in) + bc * n_in;
          bits_t* dst = static_cast<bits_t*>(g.out) + bc * n_out + col;
          const bits_t sampled = off >= 0 ? src[off] : static_cast<bits_t>(0);
          dst[static_cast<int64_t>(t) * slab] = (g.fill != nullptr && !keep) ? static_cast<bits_t>(nearest_fill_bits<ES>(g.dtype, g.fill[c])) : sampled;
        }
      }
    }
  }
}


// =====================================================================================================================
// Round 6: label maps WITHOUT a fill rule on the reference's own coordinates, plane by plane (VERDICT r5 next #4a).
// The kernel above spends most of its 76 vector instructions per voxel on the prologue of its FAST line and the decision
// whether the line may be trusted.  Since round 5 the exact chain itself is cheap where a column walks 16 planes
// (resample_lean_exact.hpp: lean_exact_planes, 27 instructions per voxel affine, 38 fused) — cheaper still here: a wave of a
// 16 x 4 x 64 brick is ONE output row, so the row-shared partial sums fma(j, m1, i m0) and the control grid's lerp along I are
// the same in all four 16-lane rows of the wave, every row makes them for its own use and the DPP row broadcast hands them
// round as in the float kernel.  Then three roundings, the bounds, one load per voxel (element bits), one store: the
// reference's `_sample_batch_grid_sample(..., mode="nearest")` (spatial.py:1695-1731) bit for bit BY CONSTRUCTION — no margin,
// no undecided voxels, no second chain.  Launched for images without a fill rule (the trilinear in-bounds weight of a
// fill rule is the kernel above's business), divisors the short division is proven for, unit spacing under control points
// (the float kernel's gate) and volumes at least 48 wide (a wave = one row).
// =====================================================================================================================
// a channel as a raw buffer (range check = the channel's bytes) and one element of it at a byte offset
template <int ES>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t nearest_channel_rsrc(const NearestImg& g, int64_t bc, int64_t n_in) {
  const char* src = static_cast<const char*>(g.in) + bc * n_in * ES;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(src), 0, static_cast<int>(static_cast<unsigned>(n_in) * ES), 0x00020000);
}
template <int ES>
__device__ __forceinline__ typename RawBits<ES>::type nearest_buffer_load(__amdgpu_buffer_rsrc_t rsrc, unsigned off) {
  if constexpr (ES == 1) return __builtin_amdgcn_raw_buffer_load_b8(rsrc, off, 0, 0);
  else if constexpr (ES == 2) return __builtin_amdgcn_raw_buffer_load_b16(rsrc, off, 0, 0);
  else if constexpr (ES == 4) return __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0);
  else {
    const auto w = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, 0);
    return static_cast<uint64_t>(w[0]) | (static_cast<uint64_t>(w[1]) << 32);
  }
}

template <bool ELASTIC_POSSIBLE, int ES>
__global__ __launch_bounds__(256, 3) void resample_nearest_exact_kernel(const NearestArgs a) {
  typedef typename RawBits<ES>::type bits_t;
  constexpr int TI = 16, TJ = 4, TK = 64;
  {
    const float* mp = a.mapping; const uint8_t* pp = a.passthrough; const float* cpp = a.cp;
    asm volatile("" ::"s"(a.tiles_k), "s"(a.tiles_j), "s"(a.tiles_i), "s"(a.magic_k), "s"(a.magic_j), "s"(a.magic_i), "s"(mp), "s"(pp), "s"(cpp),
                 "s"(a.mapping_batched), "s"(a.Io), "s"(a.Jo), "s"(a.Ko), "s"(a.I), "s"(a.J), "s"(a.K), "s"(a.n_images));
  }
  const unsigned tile = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned t1 = fastdiv_exact(tile, a.magic_k, a.tiles_k);
  const int kt = tile - t1 * a.tiles_k;
  const unsigned t2 = fastdiv_exact(t1, a.magic_j, a.tiles_j);
  const int jt = t1 - t2 * a.tiles_j;
  const unsigned t3 = fastdiv_exact(t2, a.magic_i, a.tiles_i);
  const int it = t2 - t3 * a.tiles_i;
  const int b = t3;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int tk = tid & (TK - 1), tj = tid / TK;
  const int i_begin = it * TI, j_lo = jt * TJ, k_lo = kt * TK;
  const int i_count = min(TI, a.Io - i_begin), nv = min(TJ, a.Jo - j_lo), nw = min(TK, a.Ko - k_lo);
  const bool col_active = (tj < nv) & (tk < nw);
  const int jv = min(tj, nv - 1), kw = min(tk, nw - 1);  // idle threads shadow the last column (they never store)
  const int jo = j_lo + jv, ko = k_lo + kw;
  const int64_t n_in = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t n_out = static_cast<int64_t>(a.Io) * a.Jo * a.Ko;
  const int slab = a.Jo * a.Ko;
  const int64_t col = static_cast<int64_t>(i_begin) * slab + static_cast<int64_t>(jo) * a.Ko + ko;  // first voxel of the column

  if (a.passthrough != nullptr && a.passthrough[b] != 0) {  // gated-out element: bit-exact copy (spatial.py:1101-1106)
    if (col_active) {
      for (int im = 0; im < a.n_images; im++) {
        const NearestImg& g = a.img[im];
        if (g.es != ES) continue;
        for (int c = 0; c < g.channels; c++) {
          const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
          const bits_t* src = static_cast<const bits_t*>(g.in) + bc * n_out + col;
          bits_t* dst = static_cast<bits_t*>(g.out) + bc * n_out + col;
          for (int t = 0; t < i_count; t++) dst[static_cast<int64_t>(t) * slab] = src[static_cast<int64_t>(t) * slab];
        }
      }
    }
    return;
  }

  float m[12];
  {
    typedef __attribute__((address_space(4))) const float* const_float_ptr;
    const_float_ptr mp = (const_float_ptr)(a.mapping) + (a.mapping_batched ? b * 12 : 0);
#pragma unroll
    for (int q = 0; q < 12; q++) m[q] = mp[q];
  }
  bool elastic = false;
  const float* cp = nullptr;
  if constexpr (ELASTIC_POSSIBLE) {
    elastic = !(a.cp_skip != nullptr && a.cp_skip[b] != 0);
    cp = elastic ? a.cp + (a.cp_batched ? static_cast<int64_t>(b) * (a.ni * a.nj * a.nk * 3) : 0) : nullptr;
  }
  const float cj = static_cast<float>(jo), ck = static_cast<float>(ko);
  const float hx = a.size_m1[0], hy = a.size_m1[1], hz = a.size_m1[2];
  const int i_last = i_begin + i_count - 1;
  Lerp1D lj{0, 0, 1.0f, 0.0f}, lk{0, 0, 1.0f, 0.0f}, li_lane{0, 0, 1.0f, 0.0f};
  int ia = 0, ib = 0;
  if constexpr (ELASTIC_POSSIBLE) {
    if (elastic) {
      lj = lerp_index(jo, a.nj, a.Jo, a.scale_j);
      lk = lerp_index(ko, a.nk, a.Ko, a.scale_k);
      li_lane = lerp_index(min(i_begin + (lane & (TI - 1)), i_last), a.ni, a.Io, a.scale_i);  // lane t of every row: plane t
      ia = __builtin_amdgcn_readlane(li_lane.i0, 0);
      ib = __builtin_amdgcn_readlane(li_lane.i1, TI - 1);
    }
  }
  if (elastic && ib - ia > 2) {
    // control grids denser than a brick (more than three control planes under it; rare): every voxel through the chain of ONE
    // voxel, loaded and stored as it comes (no register array: a run-time plane index would put it in scratch)
    if (col_active) {
      for (int t = 0; t < i_count; t++) {
        float x, y, z;
        exact_voxel_coords<ELASTIC_POSSIBLE>(a, m, elastic, cp, lj, lk, i_begin + t, cj, ck, x, y, z);
        const int off = nearest_offset(x, y, z, hx, hy, hz, a.J, a.K);
        for (int im = 0; im < a.n_images; im++) {
          const NearestImg& g = a.img[im];
          if (g.es != ES) continue;
          for (int c = 0; c < g.channels; c++) {
            const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
            const bits_t* src = static_cast<const bits_t*>(g.in) + bc * n_in;
            bits_t* dst = static_cast<bits_t*>(g.out) + bc * n_out + col;
            dst[static_cast<int64_t>(t) * slab] = off >= 0 ? src[off] : static_cast<bits_t>(0);
          }
        }
      }
    }
    return;
  }
  unsigned boffs[TI];  // BYTE offsets of the source voxels inside their channel, 0xFFFFFFFF = none (zero padding)
  // the launch's first channel of this element size (there is one: the host launches per element size present)
  int im0 = 0;
  while (im0 < a.n_images - 1 && a.img[im0].es != ES) im0++;
  const __amdgpu_buffer_rsrc_t rsrc0 = nearest_channel_rsrc<ES>(a.img[im0], static_cast<int64_t>(b) * a.img[im0].channels, n_in);
  bits_t v0[TI];
  {
    CtlPlanes P{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (ELASTIC_POSSIBLE) {
      if (elastic) {
        const int s_i = a.nj * a.nk * 3, s_j = a.nk * 3;
        float pa[3], pb[3], pc[3];
        cp_plane(cp, ia, s_i, s_j, lj, lk, pa);
        cp_plane(cp, min(ia + 1, a.ni - 1), s_i, s_j, lj, lk, pb);
        cp_plane(cp, min(ia + 2, a.ni - 1), s_i, s_j, lj, lk, pc);
        P.a_i = pa[0]; P.a_j = pa[1]; P.a_k = pa[2];
        P.b_i = pb[0]; P.b_j = pb[1]; P.b_k = pb[2];
        P.c_i = pc[0]; P.c_j = pc[1]; P.c_k = pc[2];
        asm volatile("" : "+v"(P.a_i), "+v"(P.a_j), "+v"(P.a_k), "+v"(P.b_i), "+v"(P.b_j), "+v"(P.b_k), "+v"(P.c_i), "+v"(P.c_j), "+v"(P.c_k));
      }
    }
    LeanArgs la;  // (only the round trip's constants are read: lean_exact_coord / _shared with UNIT spacing)
#pragma unroll
    for (int e = 0; e < 3; e++) { la.dh[e] = a.dh[e]; la.rdh[e] = a.rdh[e]; la.half_h[e] = a.half_h[e]; la.sp[e] = a.sp[e]; la.rsp[e] = a.rsp[e]; }
    // (the mapping and the round trip's constants in VECTOR registers: this kernel has registers to spare — 85 of 168 — and no
    // scalar ones: with the 21 of them in scalar registers the plane loop re-read spilled scalars through v_readlane, ~40 a plane)
#pragma unroll
    for (int q = 0; q < 12; q++) asm volatile("" : "+v"(m[q]));
#pragma unroll
    for (int e = 0; e < 3; e++) asm volatile("" : "+v"(la.dh[e]), "+v"(la.rdh[e]), "+v"(la.half_h[e]));
    BoxDmaStepper<4> no_dma;
    no_dma.left = 0;
    float X[TI], Y[TI], Z[TI];
    const bool ident = (m[0] == 1.0f) & (m[1] == 0.0f) & (m[2] == 0.0f) & (m[3] == 0.0f) & (m[4] == 0.0f) & (m[5] == 1.0f) &
                       (m[6] == 0.0f) & (m[7] == 0.0f) & (m[8] == 0.0f) & (m[9] == 0.0f) & (m[10] == 1.0f) & (m[11] == 0.0f);
    // Plane by plane, as soon as a plane's coordinates stand: its offset on the full-rate pipes (the first build of this kernel:
    // two quarter-rate v_mad_u64_u32, six float compares and an EXEC-masked branch per voxel) — the rounded coordinates as
    // integers: v_cvt_i32_f32 saturates, so "0 <= xn <= S - 1" on the float is ONE unsigned compare on the integer, NaN
    // (converted to 0) caught by two ordered compares; (ix J + iy) K + iz as two 24-bit multiply-adds (the launch gate:
    // I J <= 2^24, channels below 2^32 bytes) — and the LOAD of the launch's first channel: the memory system works while the
    // next plane is formed (all 16 coordinates first, then 16 loads: launch time = arithmetic + traffic, not their maximum).
    const unsigned Hx = static_cast<unsigned>(hx), Hy = static_cast<unsigned>(hy), Hz = static_cast<unsigned>(hz);
    const int Kes = a.K * ES, Jin = a.J;
    auto each = [&](int t) {
      const float x = X[t], y = Y[t], z = Z[t];
      const int ix = static_cast<int>(rintf(x)), iy = static_cast<int>(rintf(y)), iz = static_cast<int>(rintf(z));
      const bool ok = (static_cast<unsigned>(ix) <= Hx) & (static_cast<unsigned>(iy) <= Hy) & (static_cast<unsigned>(iz) <= Hz) &
                      !__builtin_isunordered(x, y) & (z == z);
      const int off = mad24(mad24(ix, Jin, iy), Kes, ES == 1 ? iz : iz * ES);
      boffs[t] = ok ? static_cast<unsigned>(off) : 0xFFFFFFFFu;
      v0[t] = nearest_buffer_load<ES>(rsrc0, boffs[t]);
    };
    bool done = false;
    if constexpr (ELASTIC_POSSIBLE) {
      if (elastic) {
        if (ident) lean_exact_planes<1, true, true, true, 4>(m, la, i_begin, i_last, cj, ck, li_lane, ia, P, no_dma, lane, X, Y, Z, each);
        else if (a.affine_first) lean_exact_planes<2, true, true, true, 4>(m, la, i_begin, i_last, cj, ck, li_lane, ia, P, no_dma, lane, X, Y, Z, each);
        else lean_exact_planes<3, true, true, true, 4>(m, la, i_begin, i_last, cj, ck, li_lane, ia, P, no_dma, lane, X, Y, Z, each);
        done = true;
      }
    }
    if (!done) lean_exact_planes<0, true, true, true, 4>(m, la, i_begin, i_last, cj, ck, li_lane, ia, P, no_dma, lane, X, Y, Z, each);
  }

  // (an offset beyond the channel — 0xFFFFFFFF: no source voxel — reads as zero: the zero padding is the descriptor's range
  // check, no select behind the load.)  The stores in the `scalar base + 32-bit vector offset` form on one running scalar
  // pointer (lean_exact_group_store); full bricks without predicates.  Further channels of this element size: sixteen loads, the stores.
  typedef __attribute__((address_space(1))) char* global_char_ptr;
  typedef __attribute__((address_space(1))) bits_t* global_bits_ptr;
  const bool full = (i_count == TI) & (nv == TJ) & (nw == TK);  // block uniform
  const unsigned urow = static_cast<unsigned>(jo * a.Ko + ko) * static_cast<unsigned>(ES);
  const int64_t slab_b = static_cast<int64_t>(slab) * ES;
  auto store_channel = [&](const NearestImg& g, int64_t bc, const bits_t (&v)[TI]) {
    global_char_ptr out_t = (global_char_ptr)(static_cast<char*>(g.out) + (bc * n_out + static_cast<int64_t>(i_begin) * slab) * ES);
    if (full) {
      unsigned row_off = urow;
      asm volatile("" : "+v"(row_off));  // (in the stores' own block: instruction selection must SEE the zero extension)
#pragma unroll
      for (int t = 0; t < TI; t++) {
        *(global_bits_ptr)(out_t + row_off) = v[t];
        out_t += slab_b;
        asm volatile("" : "+s"(out_t));
      }
    } else if (col_active) {
      unsigned row_off = urow;
      asm volatile("" : "+v"(row_off));
      for (int t = 0; t < i_count; t++) {
        bits_t w = v[0];
#pragma unroll
        for (int u = 1; u < TI; u++) w = (t == u) ? v[u] : w;  // (scalar selects: no dynamically indexed register array)
        *(global_bits_ptr)(out_t + row_off) = w;
        out_t += slab_b;
      }
    }
  };
  store_channel(a.img[im0], static_cast<int64_t>(b) * a.img[im0].channels, v0);
  for (int im = im0; im < a.n_images; im++) {
    const NearestImg& g = a.img[im];
    if (g.es != ES) continue;
    for (int c = (im == im0 ? 1 : 0); c < g.channels; c++) {
      const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
      const __amdgpu_buffer_rsrc_t rsrc = nearest_channel_rsrc<ES>(g, bc, n_in);
      bits_t v[TI];
#pragma unroll
      for (int t = 0; t < TI; t++) v[t] = nearest_buffer_load<ES>(rsrc, boffs[t]);
      store_channel(g, bc, v);
    }
  }
}

}  // namespace tio
