// stencil_march_kernel.inc - the text of the register-window marching kernel.  stencil_march.hpp includes it twice, with
//   TIO_MARCH_KERNEL  the kernel's name (conv_march_kernel / conv_stream_march_kernel)
//   TIO_MARCH_STREAM  false / true: the cache policy of its row loads and row stores
// defined, and says there why this is an included text and not a function template.
template <int R, bool FUSE_K, bool PRE_BIAS, int POST_NOISE, bool FMA>
__global__ __launch_bounds__(kBlock, (FUSE_K && !PRE_BIAS && R <= 6) ? 4 : 1) void TIO_MARCH_KERNEL(const ConvArgs a) {
  constexpr bool STREAM = TIO_MARCH_STREAM;
  constexpr int W = 2 * R + 1;
  typedef float v4f __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(4))) const float* const_float_ptr;
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* s_krow = s_mem + wave * 272;  // fused J+K: 8 + 256 + 8 floats per wave
  (void)s_krow;
  const int n_other = a.axis == 0 ? a.J : a.I;
  // block order (tiles_a): 1 = strips along grid.x (consecutive blocks work on adjacent strips of the
  // same segment: their rows are adjacent in memory), 0 = strips along grid.z
  const int strip_block = a.tiles_a ? blockIdx.x : blockIdx.z;
  const int k_tile = a.tiles_a ? blockIdx.z : blockIdx.x;
  const int strip = strip_block * (kBlock / 64) + wave;
  if (strip >= n_other * a.bcs) return;  // waves are independent: no barrier anywhere below
  const int other = strip % n_other;
  const int bc = strip / n_other;
  const int b = bc / a.channels;
  const int k = k_tile * 256 + 4 * lane;
  const int n = a.axis == 0 ? a.I : a.J;
  const int seg = (n + gridDim.y - 1) / gridDim.y;
  const int p_begin = blockIdx.y * seg, p_end = min(p_begin + seg, n);
  const int64_t n_spatial = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t stride = a.axis == 0 ? static_cast<int64_t>(a.J) * a.K : a.K;
  const int64_t other_stride = a.axis == 0 ? a.K : static_cast<int64_t>(a.J) * a.K;
  const int64_t line = static_cast<int64_t>(bc) * n_spatial + other * other_stride + k;
  const float* src = static_cast<const float*>(a.src);
  float* dst = static_cast<float*>(a.dst);
  if (p_begin >= p_end || k >= a.K) return;

  if (a.skip != nullptr && a.skip[b] != 0) {  // rows with no blur: emitted unchanged by the last pass
    if (a.last_pass) {
      const float* orig = static_cast<const float*>(a.x_orig);
      for (int p = p_begin; p < p_end; p++) {
        const int64_t e = line + static_cast<int64_t>(p) * stride;
        *reinterpret_cast<v4f*>(dst + e) = *reinterpret_cast<const v4f*>(orig + e);
      }
    }
    return;
  }
  const int64_t tap_base = a.taps_batched ? static_cast<int64_t>(b) * 3 * a.tap_stride : 0;
  const_float_ptr tc = (const_float_ptr)(a.taps + tap_base + static_cast<int64_t>(a.axis) * a.tap_stride);
  const_float_ptr tk = (const_float_ptr)(a.taps + tap_base + 2 * a.tap_stride);
  (void)tk;
  float tw[W];  // scalar registers
#pragma unroll
  for (int t = 0; t < W; t++) tw[t] = tc[t];
  // The K taps as well, ONCE, at the positions the register window uses them (tap t of radius rk sits at jj = 8 - rk + t;
  // zeros beyond the radius).  Until round 4 every tap was a scalar load INSIDE the marching loop — its address depends on the
  // run-time radius — followed by s_waitcnt lgkmcnt(0): thirteen serialised round trips through the scalar cache per row.
  float tkw[17];
  (void)tkw;
  if constexpr (FUSE_K) {
    const int rk0 = a.radius_k;
#pragma unroll
    for (int jj = 0; jj < 17; jj++) {
      const int t = jj - (8 - rk0);
      tkw[jj] = (t >= 0 && t <= 2 * rk0) ? tk[t] : 0.0f;
    }
  }
  // noise parameters of this strip's element, once, through the scalar cache: as plain global loads inside
  // the marching loop they sit behind a branch, and the compiler's wait at the join is vmcnt(0) - it
  // drained the two prefetched rows (and the previous store) on every row
  float noise_mu = a.noise_mean, noise_sd = a.noise_std;
  if constexpr (POST_NOISE != 0) {
    if (a.noise_batched) {
      noise_mu = ((const_float_ptr)a.noise_mean_b)[b];
      noise_sd = ((const_float_ptr)a.noise_std_b)[b];
    }
  }

  // PRE_BIAS: the arithmetic of bias_kernel, coarse planes cached while the row stays in a cell
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
  auto bias_row = [&](v4f v, int pos) -> v4f {
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
#define TIO_ROW_POS(P) min(max((P), 0), n - 1) /* replicate padding == clamp */
  auto row_load = [&](const float* p) -> v4f {
    if constexpr (STREAM) return __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    else return *reinterpret_cast<const v4f*>(p);
  };
#define TIO_ROW_LOAD(P) row_load(src + line + static_cast<int64_t>(TIO_ROW_POS(P)) * stride)
  v4f win[W];
#pragma unroll
  for (int t = 0; t < 2 * R; t++) win[t] = bias_row(TIO_ROW_LOAD(p_begin - R + t), TIO_ROW_POS(p_begin - R + t));
  win[2 * R] = win[0];
  // kMarchAhead rows of 16-byte loads in flight per lane (4 measured no faster than 2: the passes
  // are not latency bound)
  v4f nxt[kMarchAhead];
#pragma unroll
  for (int d = 0; d < kMarchAhead; d++) nxt[d] = TIO_ROW_LOAD(p_begin + R + d);
  for (int p0 = p_begin; p0 < p_end; p0 += W) {
#pragma unroll
    for (int u = 0; u < W; u++) {
      const int p = p0 + u;
      if (p >= p_end) return;  // wave uniform
      __builtin_amdgcn_sched_barrier(0);  // keep the rows apart: no hoisting of later rows' work into this one
      // the newest row (p + R) replaces the oldest one; the window of output p is slots u .. u + 2R (mod W)
      win[(2 * R + u) % W] = bias_row(nxt[0], TIO_ROW_POS(p + R));
#pragma unroll
      for (int d = 0; d + 1 < kMarchAhead; d++) nxt[d] = nxt[d + 1];
      // explicit draws of this output row: requested BEFORE the row that is loaded ahead (vector loads return in order: the
      // wait in front of the sum then leaves the newer row load in flight), used a whole window of taps later
      v4f zrow = {0.0f, 0.0f, 0.0f, 0.0f};
      if constexpr (POST_NOISE == 2) zrow = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(a.noise_base + line + static_cast<int64_t>(p) * stride));
      (void)zrow;
      nxt[kMarchAhead - 1] = TIO_ROW_LOAD(p + R + kMarchAhead);
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if constexpr (FMA) {
#pragma unroll
        for (int t = 0; t < W; t++) {
          const v4f v = win[(u + t) % W];
          acc.x = __builtin_fmaf(tw[t], v.x, acc.x);
          acc.y = __builtin_fmaf(tw[t], v.y, acc.y);
          acc.z = __builtin_fmaf(tw[t], v.z, acc.z);
          acc.w = __builtin_fmaf(tw[t], v.w, acc.w);
        }
      } else {
#pragma unroll
        for (int t = 0; t < W; t++) {
          const v4f v = win[(u + t) % W];
          acc.x = __fadd_rn(acc.x, __fmul_rn(tw[t], v.x));
          acc.y = __fadd_rn(acc.y, __fmul_rn(tw[t], v.y));
          acc.z = __fadd_rn(acc.z, __fmul_rn(tw[t], v.z));
          acc.w = __fadd_rn(acc.w, __fmul_rn(tw[t], v.w));
        }
      }
      if constexpr (FUSE_K) {
        // the register-window K filter of conv_k_v4_kernel on the row this wave just produced
        int rk = a.radius_k;
        // exact taps: the radius is re-read as an opaque scalar on every row, so the tier and tap conditions below are a
        // compare and a branch each; hoisted out of the marching loop they are eight 64-bit masks, 16 scalar registers
        // held across the whole loop, and with in-kernel noise the kernel spilled scalar registers at every radius >= 3
        if constexpr (!FMA) asm volatile("" : "+s"(rk));
        const float edge_l = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc.x), 0));
        const float edge_r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(acc.w), a.K / 4 - 1));
        *reinterpret_cast<float4*>(s_krow + 8 + 4 * lane) = acc;
        // replicate padding over the WHOLE halo (8 positions a side), not only the radius: the fast taps below run over a tier of
        // radii with zero-padded taps, and 0 * (whatever LDS held before) is NaN when that happens to be non-finite (round 5:
        // test_fused_jk_stage_every_k_radius failed for the radii inside a tier behind a test that had left Inf in LDS)
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
        if constexpr (FMA) {
          // fast taps: three branch-free tiers (radius <= 4 / <= 6 / <= 8) over the preloaded, zero-padded taps — a tap
          // beyond the radius is fma(0, w, out) = out for every finite w (the fast mode's contract is float rounding on finite
          // data; the exact mode below keeps the skipped taps skipped)
#define TIO_K_TIER(T)                                              \
  _Pragma("unroll") for (int jj = 8 - (T); jj <= 8 + (T); jj++) { \
    const float tv = tkw[jj];                                      \
    out.x = __builtin_fmaf(tv, w[jj], out.x);                      \
    out.y = __builtin_fmaf(tv, w[jj + 1], out.y);                  \
    out.z = __builtin_fmaf(tv, w[jj + 2], out.z);                  \
    out.w = __builtin_fmaf(tv, w[jj + 3], out.w);                  \
  }
          if (rk <= 4) { TIO_K_TIER(4) } else if (rk <= 6) { TIO_K_TIER(6) } else { TIO_K_TIER(8) }
#undef TIO_K_TIER
        } else {
          // exact taps: the taps taken and their order are the oracle's (a skipped tap stays skipped: 0 * w is not nothing for
          // a non-finite w).  Tiers of two radii — the inner taps of a tier unconditional, only its outermost pair (radii
          // 6 / 8) or the taps beyond |d| = 1 (radii <= 4) behind a scalar branch: 2 - 6 branches per row instead of 17.
#define TIO_K_TAP(JJ)                                       \
  {                                                         \
    const float tv = tkw[JJ];                               \
    out.x = __fadd_rn(out.x, __fmul_rn(tv, w[(JJ)]));       \
    out.y = __fadd_rn(out.y, __fmul_rn(tv, w[(JJ) + 1]));   \
    out.z = __fadd_rn(out.z, __fmul_rn(tv, w[(JJ) + 2]));   \
    out.w = __fadd_rn(out.w, __fmul_rn(tv, w[(JJ) + 3]));   \
  }
          if (rk <= 4) {
#pragma unroll
            for (int jj = 4; jj <= 12; jj++) {
              if (jj >= 7 && jj <= 9) TIO_K_TAP(jj)
              else if (jj >= 8 - rk && jj <= 8 + rk) TIO_K_TAP(jj)
            }
          } else if (rk <= 6) {
            if (rk == 6) TIO_K_TAP(2)
#pragma unroll
            for (int jj = 3; jj <= 13; jj++) TIO_K_TAP(jj)
            if (rk == 6) TIO_K_TAP(14)
          } else {
            if (rk == 8) TIO_K_TAP(0)
#pragma unroll
            for (int jj = 1; jj <= 15; jj++) TIO_K_TAP(jj)
            if (rk == 8) TIO_K_TAP(16)
          }
#undef TIO_K_TAP
        }
        acc = out;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if constexpr (POST_NOISE != 0) {  // the arithmetic of noise_kernel's 16-byte path
          const int64_t e0 = line + static_cast<int64_t>(p) * stride;
          float z[4];
          if constexpr (POST_NOISE == 2) {
            z[0] = zrow.x; z[1] = zrow.y; z[2] = zrow.z; z[3] = zrow.w;
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
      if constexpr (STREAM) {
        // (component by component, as the struct assignment below is lowered: the four become ONE global_store_dwordx4 ... nt in both
        // translation units.  Stored as one 4-vector, the instantiations built with the SLP vectoriser took other registers than their siblings.)
        float* row = dst + line + static_cast<int64_t>(p) * stride;
        __builtin_nontemporal_store(acc.x, row);
        __builtin_nontemporal_store(acc.y, row + 1);
        __builtin_nontemporal_store(acc.z, row + 2);
        __builtin_nontemporal_store(acc.w, row + 3);
      } else {
        *reinterpret_cast<float4*>(dst + line + static_cast<int64_t>(p) * stride) = acc;
      }
    }
  }
#undef TIO_ROW_LOAD
#undef TIO_ROW_POS
}

