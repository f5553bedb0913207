// resample_fast.hpp — the TIO_PRECISION_FAST path of tio_resample3d: launches of float32 trilinear images whose
// caller accepts the reference's own tolerance for intensities (1e-4 relative, BASELINE.json north_star) instead of
// the bit-exact reproduction of its float32 operation sequence.
//
// What it does differently from the exact brick kernel (resample_tile.hpp):
//   * coordinates as a LINE in the plane index per control cell, box-relative (x(t) = A + t B, the constant formed in
//     float64): 3 fma per voxel, no coordinate arrays, error ~2e-6 voxel on top of the reference's own rounding;
//   * the staged box from the <= 27 VERTICES of (planes x control cells) — the coordinate map is multilinear on each
//     such sub-box, so its extremes sit on vertices — instead of per-voxel min / max tracking and a block reduction;
//   * that planning is a kernel of its own, ONE THREAD PER BRICK (plan_bricks_kernel, resample_plan.hpp, microseconds): 16 dwords per
//     brick (box, float64-formed line constants, kind) and the scaled mapping per batch element.  The sampling
//     kernel (resample_planned_kernel, one block per 16^3 brick) starts with one s_load_dwordx16, issues its LDS-DMA
//     (scalar-addressed: one wave instruction per group of rows of one x-plane) and forms the per-column line while
//     the brick is on its way: no decode, no vertex evaluation, no reductions, no LDS besides the tile;
//   * seven fma lerps, the fill rule's in-bounds weight in its separable form and only in waves that really have a
//     column leaving the volume (a monotone line is interior when its two end planes are).
//
// Round-2 history (profiles/r02_resample_sq.md has every number): five other structures around the same arithmetic
// were built and measured — lean bricks with in-kernel planning, persistent streaming rings, pipelined persistent
// bricks, wide (8 / 16 wave) blocks — none beat the brick kernel's FAST instantiation (0.437 ms on the bench launch);
// the shader-clock traces showed why (a block's life is kernarg -> mapping -> vertices -> reductions -> barrier -> DMA
// -> barrier -> sampling, and with LDS capping a CU at three bricks the throughput is 3 / that latency).  Moving the
// planning out of the sampling kernel is what shortened it: 0.372 ms affine / 0.42 ms elastic (36 % / 32 % of 8 TB/s).
// Those kernels are gone from the tree; commit 45474dd has them all.
//
// This file holds only the kernels that TIO_PRECISION_FAST alone reaches.  The line coordinates they share with the exact
// lean and nearest kernels are in resample_line.hpp; the planner, the plan layout, the LDS-DMA helpers and LeanArgs, which
// every planned launch uses, are in resample_plan.hpp.
#pragma once
#include "resample_args.hpp"
#include "resample_exact_chain.hpp"
#include "resample_tile.hpp"
#include "resample_line.hpp"
#include "resample_plan.hpp"

namespace tio {

// =====================================================================================================================
// One block per planned brick, one column of TI planes per thread; images and channels of the launch one after the
// other through the same LDS tile (the geometry, hence the box and the lines, is shared).
// =====================================================================================================================
template <bool ELASTIC_POSSIBLE, int TI, int TJ, int TK, int OCC>
__global__ __launch_bounds__(TJ* TK, (TJ * TK) / 256 * OCC) void resample_planned_kernel(const ResampleArgs a, const int* __restrict__ plan) {
  constexpr int NT = TJ * TK, NW = NT / 64;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_tile = smem;
  typedef __attribute__((address_space(4))) const int* const_int_ptr;
  typedef __attribute__((address_space(4))) const float* const_float_ptr;

  const unsigned brick = xcd_remap(blockIdx.x, gridDim.x);
  const_int_ptr d = (const_int_ptr)(plan + a.B * 16) + static_cast<size_t>(brick) * kDescInts;
  const int kind_w = d[0];
  const int kind = kind_w & 0xFF;
  StreamBox bx;
  bx.kind = kind; bx.interior = kind_w >> 8;
  bx.bx0 = d[1]; bx.by0 = d[2]; bx.za = d[3]; bx.Lx = d[4]; bx.Ly = d[5]; bx.cpr = d[6];
  const float C3[3] = {__int_as_float(d[7]), __int_as_float(d[8]), __int_as_float(d[9])};
  const int b = d[10], i_begin = d[11], j_lo = d[12], k_lo = d[13];
  const bool elastic = ELASTIC_POSSIBLE && d[14] != 0;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tk = tid % TK, tj = tid / TK;
  const int i_count = min(TI, a.Io - i_begin), nv = min(TJ, a.Jo - j_lo), nw = min(TK, a.Ko - k_lo);
  const bool col_active = (tj < nv) & (tk < nw);
  const int jv = min(tj, nv - 1), kw = min(tk, nw - 1);
  const int64_t n_in = static_cast<int64_t>(a.I) * a.J * a.K;
  const int64_t n_out = static_cast<int64_t>(a.Io) * a.Jo * a.Ko;
  const int slab = a.Jo * a.Ko;
  const int64_t slab_b = static_cast<int64_t>(slab) * 4;
  const int col_off = (j_lo + jv) * a.Ko + (k_lo + kw);
  const unsigned urow = static_cast<unsigned>(col_off) * 4u;
  const int u0 = i_begin, u1 = i_begin + i_count;

  // The folded minimum (ImgArgs::out_min): the waves of the FIRST batch element fold the keys of what they store into one
  // of kMinSlots keys per channel (by brick, so that a few hundred — not sixteen thousand — atomics meet on an address;
  // returnless: nobody waits for them); min_finish_kernel, launched behind this kernel, folds the slots, decodes the
  // result into out_min[c] and restores the keys.  It replaces the three launches and the re-read of tio_channel_min
  // for the next transform's "minimum" fill.  (A first version decoded in the last wave to finish, through a ticket
  // counter and returning atomics: 0.40 -> 0.43 - 0.45 ms per launch, more than the reduction it saved.)
  auto publish_min = [&](const ImgArgs& g, int c, uint32_t kmin) {
    const uint32_t wmin = wave_min_u32(kmin);
    if (lane == 0 && wmin != 0xFFFFFFFFu)
      __hip_atomic_fetch_min(g.min_keys + c * kMinSlots + (brick & (kMinSlots - 1)), wmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };

  if (kind == kDescGated || kind == kDescOutside) {  // gated-out element: bit-exact copy; nothing of the volume in sight: fill (or 0)
    for (int im = 0; im < a.n_images; im++) {
      const ImgArgs& g = a.img[im];
      for (int c = 0; c < g.channels; c++) {
        const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
        char* out_chan = static_cast<char*>(g.out) + bc * n_out * 4;
        const float* in_chan = static_cast<const float*>(g.in) + bc * n_in;
        const float fillv = g.fill != nullptr ? ((const_float_ptr)g.fill)[c] : 0.0f;
        uint32_t kmin = 0xFFFFFFFFu;
        if (col_active) {
          for (int t = u0; t < u1; t++) {
            const float val = kind == kDescGated ? in_chan[static_cast<int64_t>(t) * slab + col_off] : fillv;
            *reinterpret_cast<float*>(out_chan + t * slab_b + urow) = val;
            kmin = min(kmin, float_to_key(val));
          }
        }
        if (g.out_min != nullptr && b == 0) publish_min(g, c, kmin);
      }
    }
    return;
  }

  // the scaled mapping of this batch element: scalar loads, no arithmetic
  FastFrameG f;
  {
    const_float_ptr fm = (const_float_ptr)(plan) + b * 16;
#pragma unroll
    for (int q = 0; q < 12; q++) f.m[q] = fm[q];
  }
  f.affine_first = a.affine_first != 0;
  f.ni = a.ni; f.nj = a.nj; f.nk = a.nk; f.sci = a.scale_i; f.scj = a.scale_j; f.sck = a.scale_k;
  f.elastic = elastic;
  f.cp = elastic ? a.cp + (a.cp_batched ? static_cast<int64_t>(b) * (a.ni * a.nj * a.nk * 3) : 0) : nullptr;
  f.j_lo = j_lo; f.k_lo = k_lo;
  {
    const float ratio[3] = {a.half_h[0] / a.dh[0], a.half_h[1] / a.dh[1], a.half_h[2] / a.dh[2]};
#pragma unroll
    for (int e = 0; e < 3; e++) { f.dsc[e] = a.rsp[e] * (f.affine_first ? ratio[e] : 1.0f); f.c[e] = 0.0; }
  }

  if (kind == kDescSlow) {  // box beyond the LDS budget / non-finite geometry: per-voxel evaluation, global gathers (rare)
    // (with the reference's exact coordinate chain: gather_voxel applies the fill rule to the coordinate it is handed)
    const float* mp = a.mapping + (a.mapping_batched ? b * 12 : 0);
    float mm[12];
#pragma unroll
    for (int q = 0; q < 12; q++) mm[q] = mp[q];
    Lerp1D lj_e{0, 0, 1.0f, 0.0f}, lk_e{0, 0, 1.0f, 0.0f};
    if (elastic) {
      lj_e = lerp_index(j_lo + jv, a.nj, a.Jo, a.scale_j);
      lk_e = lerp_index(k_lo + kw, a.nk, a.Ko, a.scale_k);
    }
    for (int im = 0; im < a.n_images; im++) {
      const ImgArgs& g = a.img[im];
      if (col_active) {
        for (int t = u0; t < u1; t++) {
          float x, y, z;
          exact_voxel_coords<ELASTIC_POSSIBLE>(a, mm, elastic, f.cp, lj_e, lk_e, t, static_cast<float>(j_lo + jv), static_cast<float>(k_lo + kw), x, y, z);
          gather_voxel<0>(g, a, b, n_in, n_out, t * slab + col_off, x, y, z, false);
        }
      }
      if (g.out_min != nullptr && b == 0) {  // (this thread reads back what it has just stored)
        for (int c = 0; c < g.channels; c++) {
          uint32_t kmin = 0xFFFFFFFFu;
          if (col_active) {
            const float* out_chan = static_cast<const float*>(g.out) + (static_cast<int64_t>(b) * g.channels + c) * n_out;
            for (int t = u0; t < u1; t++) kmin = min(kmin, float_to_key(out_chan[static_cast<int64_t>(t) * slab + col_off]));
          }
          publish_min(g, c, kmin);
        }
      }
    }
    return;
  }

  StageLanes sl;
  sl.cpr = -1; sl.rpi = 1; sl.row_l = 0; sl.gz_rel = 0; sl.goff = 0; sl.lane_ok = false;
  // per-column constants, formed while the first brick is on its way
  const float fv = static_cast<float>(jv), fw = static_cast<float>(kw);
  float col3[3];
  Lerp1D lj{0, 0, 1.0f, 0.0f}, lk{0, 0, 1.0f, 0.0f};
  ColumnPlanes planes;
  planes.cell = -2;
#pragma unroll
  for (int e = 0; e < 3; e++) { planes.P0[e] = 0.0f; planes.P1[e] = 0.0f; }
  FastAddr ta;
  ta.sYb = bx.cpr * 16; ta.sXb = bx.Ly * ta.sYb; ta.sXYb = ta.sXb + ta.sYb;
  ta.sYf = static_cast<float>(ta.sYb); ta.sXf = static_cast<float>(ta.sXb);
  ta.base_f = static_cast<float>(static_cast<unsigned>(reinterpret_cast<uintptr_t>((fast_lds_wptr)s_tile)));
  const float ox = static_cast<float>(bx.bx0), oy = static_cast<float>(bx.by0), oz = static_cast<float>(bx.za);
  const float hx = a.size_m1[0], hy = a.size_m1[1], hz = a.size_m1[2];

  bool first = true;
  for (int im = 0; im < a.n_images; im++) {
    const ImgArgs& g = a.img[im];
    for (int c = 0; c < g.channels; c++) {
      const int64_t bc = static_cast<int64_t>(b) * g.channels + c;
      char* out_chan = static_cast<char*>(g.out) + bc * n_out * 4;
      const float* in_chan = static_cast<const float*>(g.in) + bc * n_in;
      const bool has_fill = g.fill != nullptr;
      const float fillv = has_fill ? ((const_float_ptr)g.fill)[c] : 0.0f;
      if (!first) __syncthreads();  // the previous channel's taps are read
      stream_stage_packed<NW>(s_tile, in_chan, bx, a.I, a.J, a.K, wave, lane, sl);
      if (first) {
#pragma unroll
        for (int r = 0; r < 3; r++) col3[r] = __builtin_fmaf(f.m[4 * r + 1], fv, f.m[4 * r + 2] * fw);
        if constexpr (ELASTIC_POSSIBLE) {
          if (elastic) {
            lj = lerp_index(j_lo + jv, a.nj, a.Jo, a.scale_j);
            lk = lerp_index(k_lo + kw, a.nk, a.Ko, a.scale_k);
          }
        }
        first = false;
      }
      float A3[3], B3[3];
      int run0 = u0;
      int run1 = fast_column_line(f, lj, lk, planes, run0, u1, u0, C3, col3, lane, A3, B3);
      tile_dma_wait();
      __syncthreads();
      const bool track = g.out_min != nullptr && b == 0;  // block uniform
      uint32_t kmin = 0xFFFFFFFFu;
      unsigned unsure = 0u;  // planes of this column whose in-bounds weight came within the margin of 1/2
      const float margin = (a.fill_recheck != 0 && has_fill) ? ((const_float_ptr)(plan) + b * 16)[12] : -1.0f;
      if (col_active) {
        for (;;) {
          char* o_run = out_chan + static_cast<int64_t>(run0) * slab_b;
          if (track)
            fast_sample_line<4, true>(run1 - run0, A3, B3, ta, o_run, urow, slab_b, has_fill & !bx.interior, ox, oy, oz, hx, hy, hz, fillv, kmin, margin, run0 - u0, unsure);
          else
            fast_sample_line<4, false>(run1 - run0, A3, B3, ta, o_run, urow, slab_b, has_fill & !bx.interior, ox, oy, oz, hx, hy, hz, fillv, kmin, margin, run0 - u0, unsure);
          run0 = run1;
          if (run0 >= u1) break;
          run1 = fast_column_line(f, lj, lk, planes, run0, u1, u0, C3, col3, lane, A3, B3);
        }
      }
      if (has_fill & !bx.interior)  // (block uniform) re-decide the recorded voxels with the exact chain
        fast_fill_tail<ELASTIC_POSSIBLE>(unsure, a, a.mapping + (a.mapping_batched ? b * 12 : 0), elastic, f.cp, lj, lk, u0, static_cast<float>(j_lo + jv),
                                         static_cast<float>(k_lo + kw), in_chan, a.I, a.J, a.K, hx, hy, hz, fillv, out_chan, slab_b, urow, track ? &kmin : nullptr);
      if (track) publish_min(g, c, kmin);
    }
  }
}



// =====================================================================================================================
// Round 3: the LEAN planned kernel — ONE channel of one float32 trilinear image per launch; a FAST call with several images
// or channels is one plan and one lean launch per channel (resample_planned_kernel above, with its image / channel loops,
// remains for launches that fold the minimum of their output).
//
// Shader-clock stamps in the general kernel (profiles/r03_planned2_stamps.log) showed where a block's life goes:
// 900 ticks to its descriptor, **6 400 from the descriptor to the last DMA instruction issued**, 2 400 until the box has
// landed, 5 900 of sampling, 600 until the stores are acknowledged.  The 6 400 are not the DMA: halving the number of
// vector-memory instructions (packed DMA rows, 16-byte stores) changed nothing.  They are the PROLOGUE — ~550
// instructions and five dependent scalar-load round trips (grid size -> plan pointer -> descriptor -> mapping ->
// image table -> fill value) generated from a 900-byte argument struct with image and channel loops, 64 spilled scalar
// registers — executed by waves that are nearly alone on their SIMDs (~9 clocks per dependent instruction).  Same
// arithmetic here, organised for the shortest road to the first DMA instruction: a 150-byte argument block that arrives
// in the first scalar loads, the descriptor and the element's mapping requested TOGETHER (the element index comes from
// the brick index by a multiply-high, not from the descriptor), lane constants formed in the shadow of those loads,
// no loops over images or channels, the per-column constants after the DMA has been issued.
// (That argument block is LeanArgs, resample_plan.hpp: the lean exact kernels take it too.)
// =====================================================================================================================

// FAST trilinear sample straight from global memory (bricks whose box does not fit the tile, non-finite geometry): zero
// padding, the staged path's lerp nest and separable fill rule
__device__ __forceinline__ float lean_gather(const float* __restrict__ chan, int I, int J, int K, float x, float y, float z, bool has_fill,
                                             float fillv, float hx, float hy, float hz, float margin, int plane, unsigned& unsure) {
  if (!(fabsf(x) <= 1e30f) | !(fabsf(y) <= 1e30f) | !(fabsf(z) <= 1e30f)) return has_fill ? fillv : 0.0f;  // NaN / Inf: nothing in bounds
  const float x0 = floorf(x), y0 = floorf(y), z0 = floorf(z);
  FastTaps ts;
  ts.fx = x - x0; ts.fy = y - y0; ts.fz = z - z0;
  const float cx = fminf(fmaxf(x0, -2.0f), hx + 1.0f), cy = fminf(fmaxf(y0, -2.0f), hy + 1.0f), cz = fminf(fmaxf(z0, -2.0f), hz + 1.0f);
  const int ix = static_cast<int>(cx), iy = static_cast<int>(cy), iz = static_cast<int>(cz);
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const int px = ix + (t & 1), py = iy + ((t >> 1) & 1), pz = iz + (t >> 2);
    const bool ok = (static_cast<unsigned>(px) < static_cast<unsigned>(I)) & (static_cast<unsigned>(py) < static_cast<unsigned>(J)) &
                    (static_cast<unsigned>(pz) < static_cast<unsigned>(K)) & (cx == x0) & (cy == y0) & (cz == z0);
    ts.v[t] = ok ? chan[(static_cast<int64_t>(px) * J + py) * K + pz] : 0.0f;
  }
  float val = fast_finish(ts);
  if (has_fill) {
    const float mk = fast_mask(ts, x0, y0, z0, hx, hy, hz);
    val = (mk > 0.5f) ? val : fillv;
    unsure |= (fabsf(mk - 0.5f) <= margin) ? (1u << plane) : 0u;  // re-decided by the kernel's tail (exact chain)
  }
  return val;
}

// Brick shape TI x TJ x TK (planes x rows x lanes along K, TJ * TK = 256 threads); the planner is instantiated for the same
// shape.  Tried and dropped (profiles/r03_resample.md): eight waves per 16-plane brick (two threads per column) — no
// faster for affine launches, much slower for elastic ones; 8-plane bricks with five or six blocks per CU — no faster;
// 16 x 8 x 32 bricks (longer rows: fewer, fuller cache lines) — boxes outgrow the tile, slower; 16-byte stores through a
// quad transpose — a quarter of the store instructions, no faster (the transpose costs what the stores saved).  Later in
// round 3 (profiles/r03_resample.md section 5): wave priorities (s_setprio around the DMA issue or the sampling),
// nontemporal stores, a wave footprint of 8 x 8 columns (conflict-free LDS reads, 32-byte store segments), the box
// through registers (global_load_dwordx4 + ds_write_b128) instead of the LDS-DMA, 12- and 14-plane bricks with a fourth
// block per CU, 512-thread blocks on 16 x 16 x 32 and 8 x 16 x 32 bricks — none faster on the affine launch (the
// 16 x 16 x 32 bricks gain 6 % on an elastic-only launch and lose 2 x on rotated boxes that outgrow 80 KB).
// INSTR = true is the INSTRUMENTED instantiation (launched only when TIO_TILE_ABLATE is set: tests/native/resample_bench
// --ablate): a.ablate 1 no DMA, 2 no sampling, 64 shader-clock stamps written over the brick's first output row, 128
// every lane samples one LDS address.  The production instantiation (INSTR = false) carries none of it.
// FOLD_MIN = true is the instantiation launched when the caller asked for the folded minimum (LeanArgs::min_keys): the
// bricks of batch element 0 run the TRACK form of the sampling loop.  Its own instantiation because the second copy of the
// loop costs scalar registers (14 / 26 more spilled) that launches without the request should not pay for.
template <bool ELASTIC_POSSIBLE, int TI, int TJ, int TK, int WAVES_PER_SIMD, bool INSTR = false, bool FOLD_MIN = false>
__global__ __launch_bounds__(TJ* TK, WAVES_PER_SIMD) void resample_planned_lean_kernel(const LeanArgs a) {
  const int ablate = INSTR ? a.ablate : 0;
  constexpr int NW = TJ * TK / 64;
  static_assert((TJ * TK) % 64 == 0 && (TK & (TK - 1)) == 0, "one thread per column of the brick");
  constexpr int PLANES = TI;  // output planes per thread
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_tile = smem;
  typedef __attribute__((address_space(4))) const int* const_int_ptr;
  typedef __attribute__((address_space(4))) const float* const_float_ptr;

  // every argument the road to the first DMA needs, in scalar registers NOW: the loads go out back to back and share one
  // wait (left to itself the compiler fetches each kernel argument right before its first use: five round trips)
  {
    const int* plan_p = a.plan; const float* in_p = a.in;
    asm volatile("" ::"s"(a.n_items), "s"(a.bricks_per_element), "s"(a.bpe_magic), "s"(plan_p), "s"(in_p), "s"(a.B), "s"(a.I), "s"(a.J), "s"(a.K));
    if constexpr (INSTR) asm volatile("" ::"s"(a.ablate));
  }
  const unsigned long long t_entry = (ablate & 64) ? __builtin_amdgcn_s_memtime() : 0ull;
  const unsigned brick = xcd_remap(blockIdx.x, static_cast<unsigned>(a.n_items));
  const int b = static_cast<int>(fastdiv_exact(brick, a.bpe_magic, a.bricks_per_element));
  // the two scalar loads everything waits for, requested together
  const_int_ptr d = (const_int_ptr)(a.plan + a.B * 16) + static_cast<size_t>(brick) * kDescInts;
  const_float_ptr fm = (const_float_ptr)(a.plan) + b * 16;
  const int kind_w = d[0];
  StreamBox bx;
  bx.bx0 = d[1]; bx.by0 = d[2]; bx.za = d[3]; bx.Lx = d[4]; bx.Ly = d[5]; bx.cpr = d[6];
  const float C3[3] = {__int_as_float(d[7]), __int_as_float(d[8]), __int_as_float(d[9])};
  const int i_begin = d[11], j_lo = d[12], k_lo = d[13];
  const bool elastic = ELASTIC_POSSIBLE && d[14] != 0;
  FastFrameG f;
#pragma unroll
  for (int q = 0; q < 12; q++) f.m[q] = fm[q];

  // lane constants (no dependence on the loads above)
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tk = tid & (TK - 1), tj = tid / TK;
  constexpr int part = 0;
  const int slab = a.Jo * a.Ko;
  const int64_t slab_b = static_cast<int64_t>(slab) * 4;
  const float* in_chan = a.in + static_cast<int64_t>(b) * a.in_stride;
  char* out_chan = reinterpret_cast<char*>(a.out + static_cast<int64_t>(b) * a.out_stride);

  const int kind = kind_w & 0xFF;
  bx.kind = kind; bx.interior = kind_w >> 8;
  unsigned long long t_desc = 0ull, t_issued = 0ull;
  if (ablate & 64) { asm volatile("" ::"s"(kind)); t_desc = __builtin_amdgcn_s_memtime(); }
  if (kind == kDescStaged && !(ablate & 1)) {  // the road to the first DMA instruction ends here
    StageLanes sl;
    sl.cpr = -1; sl.rpi = 1; sl.row_l = 0; sl.gz_rel = 0; sl.goff = 0; sl.lane_ok = false;
    if (INSTR && (ablate & 2048))  // experiment: the box requested with the nontemporal hint
      stream_stage_packed<NW, 2>(s_tile, in_chan, bx, a.I, a.J, a.K, wave, lane, sl);
    else
      stream_stage_packed<NW>(s_tile, in_chan, bx, a.I, a.J, a.K, wave, lane, sl, INSTR ? ((ablate & 256) ? 3 : ((ablate & 512) ? 2 : 0)) : 0);
  }
  if (ablate & 64) t_issued = __builtin_amdgcn_s_memtime();

  const int i_count = min(TI, a.Io - i_begin), nv = min(TJ, a.Jo - j_lo), nw = min(TK, a.Ko - k_lo);
  const bool col_active = (tj < nv) & (tk < nw);
  const int jv = min(tj, nv - 1), kw = min(tk, nw - 1);
  const int col_off = (j_lo + jv) * a.Ko + (k_lo + kw);
  const unsigned urow = static_cast<unsigned>(col_off) * 4u;
  const int u_ref = i_begin;  // plane the descriptor's line constants refer to
  const int u0 = min(i_begin + part * PLANES, i_begin + i_count), u1 = min(u0 + PLANES, i_begin + i_count);
  const bool has_fill = a.fill != nullptr;
  const float fillv = has_fill ? ((const_float_ptr)a.fill)[0] : 0.0f;
  const float hx = a.hx, hy = a.hy, hz = a.hz;

  const bool track = FOLD_MIN && a.min_keys != nullptr && b == 0;  // block uniform
  uint32_t kmin = 0xFFFFFFFFu;
  auto publish_min = [&]() {  // (one returnless atomic per wave, spread over kMinSlots addresses by brick: resample_planned_kernel)
    const uint32_t wmin = wave_min_u32(kmin);
    if (lane == 0 && wmin != 0xFFFFFFFFu)
      __hip_atomic_fetch_min(a.min_keys + (brick & (kMinSlots - 1)), wmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  if (kind == kDescGated || kind == kDescOutside) {  // gated-out element: bit-exact copy; nothing of the volume in sight: fill (or 0)
    if (col_active) {
      for (int t = u0; t < u1; t++) {
        const float val = kind == kDescGated ? in_chan[static_cast<int64_t>(t) * slab + col_off] : fillv;
        *reinterpret_cast<float*>(out_chan + t * slab_b + urow) = val;
        kmin = min(kmin, float_to_key(val));
      }
    }
    if (track) publish_min();
    return;
  }

  f.affine_first = a.affine_first != 0;
  f.ni = a.ni; f.nj = a.nj; f.nk = a.nk; f.sci = a.sci; f.scj = a.scj; f.sck = a.sck;
  f.elastic = elastic;
  f.cp = elastic ? a.cp + (a.cp_batched ? static_cast<int64_t>(b) * (a.ni * a.nj * a.nk * 3) : 0) : nullptr;
  f.j_lo = j_lo; f.k_lo = k_lo;
#pragma unroll
  for (int e = 0; e < 3; e++) { f.dsc[e] = a.dsc[e]; f.c[e] = 0.0; }

  // The fill decision of voxels whose FAST in-bounds weight comes within `margin` of 1/2 (a few hundred per 256^3 volume, all
  // in bricks on the volume's surface) is made by the reference's exact chain, in a tail behind the sampling loops
  // (resample_exact_chain.hpp); the loops only raise the plane's bit in `unsure`.
  unsigned unsure = 0u;
  const float margin = (a.fill_recheck != 0 && has_fill) ? fm[12] : -1.0f;
  auto lean_tail = [&]() {
    if (__builtin_amdgcn_ballot_w64(unsure != 0u) == 0ull) return;
    ExactChainArgs ea;
    ea.ni = a.ni; ea.nj = a.nj; ea.nk = a.nk; ea.Io = a.Io; ea.unit_spacing = a.unit_spacing; ea.affine_first = a.affine_first;
    ea.scale_i = a.sci;
#pragma unroll
    for (int e = 0; e < 3; e++) { ea.sp[e] = a.sp[e]; ea.rsp[e] = a.rsp[e]; ea.den[e] = a.den[e]; ea.rden[e] = a.rden[e]; }
    ea.size_m1[0] = hx; ea.size_m1[1] = hy; ea.size_m1[2] = hz;
    Lerp1D lj_e{0, 0, 1.0f, 0.0f}, lk_e{0, 0, 1.0f, 0.0f};
    if (elastic) {
      lj_e = lerp_index(j_lo + jv, a.nj, a.Jo, a.scj);
      lk_e = lerp_index(k_lo + kw, a.nk, a.Ko, a.sck);
    }
    fast_fill_tail<ELASTIC_POSSIBLE>(unsure, ea, a.mapping + (a.mapping_batched ? b * 12 : 0), elastic, f.cp, lj_e, lk_e, u0, static_cast<float>(j_lo + jv),
                                     static_cast<float>(k_lo + kw), in_chan, a.I, a.J, a.K, hx, hy, hz, fillv, out_chan, slab_b, urow, track ? &kmin : nullptr);
  };

  if (kind == kDescSlow) {  // box beyond the LDS budget / non-finite geometry: per-voxel evaluation, global gathers (rare)
    pipe_brick_frame(f, j_lo, k_lo);
    if (col_active) {
      for (int t = u0; t < u1; t++) {
        float x, y, z;
        fast_coord(f, static_cast<float>(t), static_cast<float>(jv), static_cast<float>(kw), x, y, z);
        const float val = lean_gather(in_chan, a.I, a.J, a.K, x, y, z, has_fill, fillv, hx, hy, hz, margin, t - u0, unsure);
        *reinterpret_cast<float*>(out_chan + t * slab_b + urow) = val;
        if (!((unsure >> (t - u0)) & 1u)) kmin = min(kmin, float_to_key(val));  // (a re-decided voxel is counted by the tail)
      }
    }
    if (has_fill) lean_tail();
    if (track) publish_min();
    return;
  }

  // per-column constants, formed while the box is on its way
  const float fv = static_cast<float>(jv), fw = static_cast<float>(kw);
  float col3[3];
#pragma unroll
  for (int r = 0; r < 3; r++) col3[r] = __builtin_fmaf(f.m[4 * r + 1], fv, f.m[4 * r + 2] * fw);
  Lerp1D lj{0, 0, 1.0f, 0.0f}, lk{0, 0, 1.0f, 0.0f};
  if constexpr (ELASTIC_POSSIBLE) {
    if (elastic) {
      lj = lerp_index(j_lo + jv, a.nj, a.Jo, a.scj);
      lk = lerp_index(k_lo + kw, a.nk, a.Ko, a.sck);
    }
  }
  ColumnPlanes planes;
  planes.cell = -2;
#pragma unroll
  for (int e = 0; e < 3; e++) { planes.P0[e] = 0.0f; planes.P1[e] = 0.0f; }
  FastAddr ta;
  ta.sYb = bx.cpr * 16; ta.sXb = bx.Ly * ta.sYb; ta.sXYb = ta.sXb + ta.sYb;
  ta.sYf = static_cast<float>(ta.sYb); ta.sXf = static_cast<float>(ta.sXb);
  ta.base_f = static_cast<float>(static_cast<unsigned>(reinterpret_cast<uintptr_t>((fast_lds_wptr)s_tile)));
  const float ox = static_cast<float>(bx.bx0), oy = static_cast<float>(bx.by0), oz = static_cast<float>(bx.za);

  float A3[3], B3[3];
  int run0 = u0;
  int run1 = fast_column_line(f, lj, lk, planes, run0, u1, u_ref, C3, col3, lane, A3, B3);
  if (ablate & 128) {  // experiment: every lane samples the box origin (same instructions, one LDS address per wave)
#pragma unroll
    for (int r = 0; r < 3; r++) { A3[r] = 0.25f; B3[r] = 0.0f; }
  }
  unsigned long long t_ready = 0ull, t_own = 0ull, t_landed = 0ull;
  if (ablate & 64) t_ready = __builtin_amdgcn_s_memtime();
  tile_dma_wait();
  if (ablate & 64) t_own = __builtin_amdgcn_s_memtime();
  __syncthreads();
  if (ablate & 64) t_landed = __builtin_amdgcn_s_memtime();
  if (col_active && u0 < u1 && !(ablate & 2)) {
    const bool needs_mask = has_fill & !bx.interior;
    for (;;) {
      char* o_run = out_chan + static_cast<int64_t>(run0) * slab_b;
      if (track)
        fast_sample_line<4, true>(run1 - run0, A3, B3, ta, o_run, urow, slab_b, needs_mask, ox, oy, oz, hx, hy, hz, fillv, kmin, margin, run0 - u0, unsure);
      else
        fast_sample_line<4, false>(run1 - run0, A3, B3, ta, o_run, urow, slab_b, needs_mask, ox, oy, oz, hx, hy, hz, fillv, kmin, margin, run0 - u0, unsure);
      run0 = run1;
      if (run0 >= u1) break;
      run1 = fast_column_line(f, lj, lk, planes, run0, u1, u_ref, C3, col3, lane, A3, B3);
    }
  }
  if (has_fill & !bx.interior) lean_tail();  // (block uniform)
  if (track) publish_min();
  if (ablate & 64) {  // instrumentation: the block's shader-clock stamps over the first row of its own output
    const unsigned long long t_sampled = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    const unsigned long long t_drained = __builtin_amdgcn_s_memtime();
    if (tid == 0 && nw >= 12 && i_count >= 1) {
      unsigned* w = reinterpret_cast<unsigned*>(out_chan + static_cast<int64_t>(i_begin) * slab_b) + (j_lo * a.Ko + k_lo);
      w[0] = 0x53544D50u;
      w[1] = static_cast<unsigned>(t_entry); w[2] = static_cast<unsigned>(t_entry >> 32);
      w[3] = static_cast<unsigned>(t_desc - t_entry); w[4] = static_cast<unsigned>(t_issued - t_entry);
      w[5] = static_cast<unsigned>(t_ready - t_entry); w[6] = static_cast<unsigned>(t_own - t_entry);
      w[7] = static_cast<unsigned>(t_landed - t_entry); w[8] = static_cast<unsigned>(t_sampled - t_entry);
      w[9] = static_cast<unsigned>(t_drained - t_entry); w[10] = static_cast<unsigned>(kind);
      w[11] = static_cast<unsigned>(__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)));   // HW_ID
      w[12] = static_cast<unsigned>(__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)));  // XCC_ID
    }
  }
}

}  // namespace tio
