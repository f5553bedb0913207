// resample_plan.hpp — everything a brick plan is, for every planned launch of tio_resample3d, exact or FAST: the planning
// kernel (plan_bricks_kernel, one group of lanes per brick: the staged box from the brick's vertices), the plan's layout,
// the packed LDS-DMA that stages a planned box (StreamBox, StageLanes, stream_stage_packed), the decoder of the folded
// minimum (min_finish_kernel) and the argument block of the lean kernels (LeanArgs).  The kernels that consume a plan are
// in resample_tile.hpp, resample_fast.hpp, resample_lean_exact.hpp and resample_nearest.hpp.  Built on
// resample_tile.hpp (box_address_fits, kTileFar) and resample_line.hpp (the frame and its vertices).
#pragma once
#include "resample_args.hpp"
#include "resample_tile.hpp"
#include "resample_line.hpp"

namespace tio {

struct StreamBox {
  int kind, bx0, by0, za, Lx, Ly, cpr, interior;
};

// Lane constants of the LDS-DMA for one row length (cpr 16-byte chunks per row): a wave instruction
// covers rpi = 64 / cpr consecutive rows of one x-plane, lane l fetching chunk ch_l of row row_l.
struct StageLanes {
  int cpr;            // key (-1: nothing cached)
  int rpi;            // rows per wave instruction
  int row_l, gz_rel;  // this lane's row inside the group and 4 * its chunk index
  unsigned goff;      // byte offset of this lane's chunk from the group's first byte (needs K: per launch constant)
  bool lane_ok;       // row_l < rpi
};

__device__ __forceinline__ void stage_lanes(StageLanes& sl, int cpr, int K, int lane) {
  if (cpr == sl.cpr) return;
  const float rcp = __builtin_amdgcn_rcpf(static_cast<float>(cpr));
  sl.cpr = cpr;
  sl.row_l = static_cast<int>((static_cast<float>(lane) + 0.5f) * rcp);
  const int ch_l = lane - sl.row_l * cpr;
  sl.rpi = __builtin_amdgcn_readfirstlane(static_cast<int>(64.0f * rcp + 1e-3f));
  sl.lane_ok = sl.row_l < sl.rpi;
  sl.gz_rel = 4 * ch_l;
  sl.goff = static_cast<unsigned>(sl.row_l * K + 4 * ch_l) * 4u;
}

// This wave's share (instructions wave, wave + NW, ...) of the LDS-DMA of one box, PACKED (round 3): the rows of the
// box are one dense sequence in LDS (x-plane after x-plane, row pitch = 4 cpr floats), and a wave instruction simply
// covers the next rpi rows of that sequence, whatever x-plane they belong to.  One instruction sequence per x-plane
// would take ceil(Ly / rpi) instructions for each — for the bench geometry (Ly ~ 21, rpi = 10) three, the third
// carrying a single row — i.e. 63 instructions for a box of 44 KiB; packed, the same box takes 45.  A
// vector-memory instruction costs this kernel's CU about the same whatever it moves (profiles/r03_resample.md), so the
// count is what matters.  The price is a per-lane address (row -> x-plane and row inside it, advanced incrementally)
// instead of scalar pointer increments: a handful of vector instructions per DMA instruction.  Boxes that stick out
// of the volume check rows per lane and store zeros for the chunks outside.
template <int NW, int AUX = 0>
__device__ __forceinline__ int stream_stage_packed(float* __restrict__ tile, const float* __restrict__ src, const StreamBox& bx, int I, int J,
                                                    int K, int wave, int lane, StageLanes& sl, int skip_mod = 0) {
  // skip_mod (instrumented instantiation only, --ablate 256 / 512): every skip_mod-th DMA instruction of a wave is NOT issued
  // (the tile keeps stale data: timing experiment — how much of the launch is the number of line requests)
  typedef __attribute__((address_space(1))) const char* global_byte_ptr;
  stage_lanes(sl, bx.cpr, K, lane);
  const int rpi = sl.rpi;
  const int total_rows = bx.Lx * bx.Ly;
  // (uniform float divisions of small integers: exact after the half-step nudge)
  const int n_instr = __builtin_amdgcn_readfirstlane(static_cast<int>((static_cast<float>(total_rows + rpi - 1) + 0.5f) * __builtin_amdgcn_rcpf(static_cast<float>(rpi))));
  const int step = NW * rpi;  // rows between two instructions of this wave
  const float rcp_ly = __builtin_amdgcn_rcpf(static_cast<float>(bx.Ly));
  const int step_p = __builtin_amdgcn_readfirstlane(static_cast<int>((static_cast<float>(step) + 0.5f) * rcp_ly));
  const int step_r = step - step_p * bx.Ly;
  // this lane's first row of the sequence -> (x-plane, row)
  int row = wave * rpi + sl.row_l;
  int p = static_cast<int>((static_cast<float>(row) + 0.5f) * rcp_ly);
  int r = row - p * bx.Ly;
  const unsigned plane_b = static_cast<unsigned>(J) * static_cast<unsigned>(K) * 4u, row_b = static_cast<unsigned>(K) * 4u;
  // byte offset of this lane's chunk from the box origin (inside one channel: < 2^32, resample.hip checks n_in < 2^30)
  unsigned off = static_cast<unsigned>(p) * plane_b + static_cast<unsigned>(r) * row_b + static_cast<unsigned>(sl.gz_rel) * 4u;
  const unsigned step_b = static_cast<unsigned>(step_p) * plane_b + static_cast<unsigned>(step_r) * row_b;
  const unsigned wrap_b = plane_b - static_cast<unsigned>(bx.Ly) * row_b;  // one x-plane further, Ly rows back
  global_byte_ptr origin = (global_byte_ptr)(src) + ((static_cast<int64_t>(bx.bx0) * J + bx.by0) * K + bx.za) * 4;
  const int dgroup = rpi * bx.cpr * 4;  // LDS floats per instruction
  float* lp = tile + wave * dgroup;
  int issued = 0;
  const bool ch_ok = static_cast<unsigned>(bx.za + sl.gz_rel) < static_cast<unsigned>(K);
  int it = 0;
  for (int n = wave; n < n_instr; n += NW, it++) {
    const bool in_box = sl.lane_ok & (row < total_rows) & !(skip_mod > 0 && (it % skip_mod) == skip_mod - 1);
    if (bx.interior) {
      if (in_box) __builtin_amdgcn_global_load_lds(origin + off, (fast_lds_wptr)(lp), 16, 0, AUX);
      issued++;
    } else {
      const bool in_vol = in_box & ch_ok & (static_cast<unsigned>(bx.bx0 + p) < static_cast<unsigned>(I)) &
                          (static_cast<unsigned>(bx.by0 + r) < static_cast<unsigned>(J));
      if (__builtin_amdgcn_ballot_w64(in_vol) != 0ull) issued++;
      if (in_vol) __builtin_amdgcn_global_load_lds(origin + off, (fast_lds_wptr)(lp), 16, 0, AUX);
      else if (in_box) lds_zero_chunk(lp + 4 * lane);
    }
    row += step; p += step_p; r += step_r; off += step_b;
    if (r >= bx.Ly) { r -= bx.Ly; p += 1; off += wrap_b; }
    lp += NW * dgroup;
  }
  return issued;
}

struct PipePlan {
  int b, it, jt, kt;
  int i_begin, j_lo, k_lo, i_count, nv, nw;
  int fast;  // the brick's whole plane range in one pass: a staged box, or nothing of the volume in sight
  StreamBox bx;
};

template <int TI, int TJ, int TK>
__device__ __forceinline__ void pipe_decode(const ResampleArgs& a, unsigned tile, PipePlan& p) {
  const unsigned t1 = fastdiv_exact(tile, a.magic_k, a.tiles_k);
  p.kt = tile - t1 * a.tiles_k;
  const unsigned t2 = fastdiv_exact(t1, a.magic_j, a.tiles_j);
  p.jt = t1 - t2 * a.tiles_j;
  const unsigned t3 = fastdiv_exact(t2, a.magic_i, a.tiles_i);
  p.it = t2 - t3 * a.tiles_i;
  p.b = static_cast<int>(t3);
  p.i_begin = p.it * TI; p.j_lo = p.jt * TJ; p.k_lo = p.kt * TK;
  p.i_count = min(TI, a.Io - p.i_begin); p.nv = min(TJ, a.Jo - p.j_lo); p.nw = min(TK, a.Ko - p.k_lo);
  p.fast = 0;
}

__device__ __forceinline__ void pipe_brick_frame(FastFrameG& f, int j_lo, int k_lo) {
#pragma unroll
  for (int r = 0; r < 3; r++)
    f.c[r] = static_cast<double>(f.m[4 * r + 1]) * j_lo + static_cast<double>(f.m[4 * r + 2]) * k_lo + static_cast<double>(f.m[4 * r + 3]);
  f.j_lo = j_lo; f.k_lo = k_lo;
}

// vertex `vtx` of the brick framed in f (planes [u0, u0 + n)): its coordinate, clamped for the integer box
__device__ __forceinline__ void pipe_vertex(const ResampleArgs& a, const FastFrameG& f, int vtx, int u0, int n, int nv, int nw, int (&r)[6], bool& bad) {
  const int u_lo = u0, u_hi = u0 + n - 1;
  int du, dv, dw;
  if (f.elastic) { du = vtx % 3; dv = (vtx / 3) % 3; dw = vtx / 9; } else { du = vtx & 1; dv = (vtx >> 1) & 1; dw = vtx >> 2; }
  bool dense = false;
  float u = du == 0 ? static_cast<float>(u_lo) : static_cast<float>(u_hi);
  float v = dv == 0 ? 0.0f : static_cast<float>(nv - 1);
  float w = dw == 0 ? 0.0f : static_cast<float>(nw - 1);
  if (f.elastic) {
    if (du == 2) u = fast_breakpoint(f.sci, f.ni, u_lo, u_hi, dense);
    if (dv == 2) v = fast_breakpoint(f.scj, f.nj, f.j_lo, f.j_lo + nv - 1, dense) - static_cast<float>(f.j_lo);
    if (dw == 2) w = fast_breakpoint(f.sck, f.nk, f.k_lo, f.k_lo + nw - 1, dense) - static_cast<float>(f.k_lo);
  }
  float x, y, z;
  fast_coord(f, u, v, w, x, y, z);
  constexpr float kMargin = 1.0f / 64.0f;
  bad = !(fabsf(x) <= 1e30f) | !(fabsf(y) <= 1e30f) | !(fabsf(z) <= 1e30f) | dense;
  const float capx = a.size_m1[0] + 1.0f + kTileFar, capy = a.size_m1[1] + 1.0f + kTileFar, capz = a.size_m1[2] + 1.0f + kTileFar;
  r[0] = -static_cast<int>(fminf(fmaxf(floorf(x - kMargin), -kTileFar), capx));
  r[1] = static_cast<int>(fminf(fmaxf(floorf(x + kMargin), -kTileFar), capx));
  r[2] = -static_cast<int>(fminf(fmaxf(floorf(y - kMargin), -kTileFar), capy));
  r[3] = static_cast<int>(fminf(fmaxf(floorf(y + kMargin), -kTileFar), capy));
  r[4] = -static_cast<int>(fminf(fmaxf(floorf(z - kMargin), -kTileFar), capz));
  r[5] = static_cast<int>(fminf(fmaxf(floorf(z + kMargin), -kTileFar), capz));
}

// =====================================================================================================================
// The plan: 16 dwords per brick, 16 floats per batch element ahead of them
//   brick:  [0] kind | interior << 8   [1] bx0 [2] by0 [3] za [4] Lx [5] Ly [6] cpr   [7..9] C3 (float bits): the mapping
//           of (i_begin, j_lo, k_lo) relative to the box origin   [10] b [11] i_begin [12] j_lo [13] k_lo [14] elastic
//   batch:  [0..11] mapping rows scaled by the axis ratios (S_own - 1) / max(S_norm - 1, 1)   [12] margin of the fill decision
// Round 6 (a.plan_multi, the exact-coordinate lean kernel only): a brick whose box exceeds the tile is bounded again in HALVES,
// then QUARTERS, of its planes.  kind = kDescMulti, [1..6] = the box of pass 0, [15] = passes | state of pass q << (8 + 4 q), and the
// boxes of ALL passes follow the descriptors: kPassInts ints per pass, 4 passes per brick, at plan + B 16 + n_items 16 +
// brick 32:  [0] bx0 [1] by0 [2] za [3] Lx [4] Ly [5] cpr [6] state (kPassStaged / kPassOutside / kPassSlow) | interior << 8
// [7] planes.  A pass that still does not fit samples its planes voxel by voxel; the others stage their box one after the other.
// Behind the pass boxes: the LIST of these bricks, which the walker blocks of resample_lean_exact_kernel take bricks from; its
// header — [0] their number, [1] / [2] the walkers' cursor and done count — sits in FRONT of the plan (plan[-kPlanHeaderInts ...]:
// one place whatever the launch's size, zero between launches).
// =====================================================================================================================
enum : int { kPlanHeaderInts = 16, kDescMulti = 4, kPassInts = 8, kPassesPerBrick = 4, kPassStaged = 0, kPassOutside = 1, kPassSlow = 2 };

// the integer box of extremes `ext` (butterfly-reduced: identical in every lane of the group)
struct PlanBox {
  int xmin, ymin, za, Lx, Ly, cpr, interior, outside, fits;
};
__device__ __forceinline__ PlanBox plan_box(const ResampleArgs& a, const int (&ext)[7], bool weird) {
  PlanBox pb;
  const int xmin = -ext[0], xmax = ext[1], ymin = -ext[2], ymax = ext[3], zmin = -ext[4], zmax = ext[5];
  const bool wrd = weird | (ext[6] != 0);
  pb.interior = (xmin >= 0) & (xmax + 1 <= a.I - 1) & (ymin >= 0) & (ymax + 1 <= a.J - 1) & (zmin >= 0) & (zmax + 1 <= a.K - 1) & !wrd;
  pb.outside = ((xmax + 1 < 0) | (xmin > a.I - 1) | (ymax + 1 < 0) | (ymin > a.J - 1) | (zmax + 1 < 0) | (zmin > a.K - 1)) & !wrd;
  pb.za = zmin & ~3; pb.Lx = xmax + 2 - xmin; pb.Ly = ymax + 2 - ymin;
  const int Lz = ((zmax + 1 + 4) & ~3) - pb.za;
  pb.fits = !wrd && (Lz <= 256) && (pb.Lx <= 4096) && (pb.Ly <= 4096) && (static_cast<int64_t>(pb.Lx) * pb.Ly * Lz <= static_cast<int64_t>(a.tile_cap));
  pb.xmin = xmin; pb.ymin = ymin; pb.cpr = Lz >> 2;
  return pb;
}
// ... of a PASS of a multi-pass brick: the consumer (resample_lean_exact_kernel) takes the planner's word for these, so the
// conditions it re-checks for a one-pass box — the tap addresses formed from absolute indices stay exact in float32
// (box_address_fits, resample_tile.hpp) — are decided here
__device__ __forceinline__ PlanBox plan_pass_box(const ResampleArgs& a, const int (&ext)[7], bool weird) {
  PlanBox pb = plan_box(a, ext, weird);
  if (pb.fits && !box_address_fits(pb.xmin, pb.ymin, pb.za, pb.Lx, pb.Ly, pb.cpr)) pb.fits = 0;
  return pb;
}
// A group of lanes per brick, one vertex per lane: 32 lanes (27 busy) when the launch has control points — a vertex then
// reads 24 control values, and one thread walking its 27 vertices one after the other made the planner a chain of 27
// memory round trips (21.6 us per bench launch; side by side 16.4) — 8 lanes for affine-only launches (5.8 us either
// way).  The extremes meet through shuffles inside the group; its lane 0 writes the descriptor.
constexpr int plan_group(bool elastic_possible) { return elastic_possible ? 32 : 8; }

template <bool ELASTIC_POSSIBLE, int TI, int TJ, int TK>
__global__ __launch_bounds__(256) void plan_bricks_kernel(const ResampleArgs a, int* __restrict__ plan, int n_items) {
  constexpr int GROUP = plan_group(ELASTIC_POSSIBLE);
  const int gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const float ratio[3] = {a.half_h[0] / a.dh[0], a.half_h[1] / a.dh[1], a.half_h[2] / a.dh[2]};
  if (gtid < a.B) {
    const float* m = a.mapping + (a.mapping_batched ? gtid * 12 : 0);
    float* fr = reinterpret_cast<float*>(plan) + gtid * 16;
    for (int q = 0; q < 12; q++) fr[q] = m[q] * ratio[q >> 2];
    {  // [12]: the margin of the fill decision for this element (resample_exact_chain.hpp)
      float mm[12];
      for (int q = 0; q < 12; q++) mm[q] = m[q];
      fr[12] = fast_fill_margin(mm, static_cast<float>(a.Io), static_cast<float>(a.Jo), static_cast<float>(a.Ko), a.size_m1[0] + 1.0f,
                                a.size_m1[1] + 1.0f, a.size_m1[2] + 1.0f);
    }
    fr[13] = __int_as_float(a.tile_cap);  // (the tile the boxes were sized for: the consumer of a multi-pass brick compares it with its own)
    for (int q = 14; q < 16; q++) fr[q] = 0.0f;
  }
  const int t = gtid / GROUP, v = gtid % GROUP;
  if (t >= n_items) return;  // (whole groups leave together: the shuffles below stay inside a group)
  PipePlan p;
  pipe_decode<TI, TJ, TK>(a, static_cast<unsigned>(t), p);
  int* d = plan + a.B * 16 + t * kDescInts;
  if (a.passthrough != nullptr && a.passthrough[p.b] != 0) {
    for (int q = v; q < kDescInts; q += GROUP) d[q] = q == 0 ? kDescGated : (q == 10 ? p.b : (q == 11 ? p.i_begin : (q == 12 ? p.j_lo : (q == 13 ? p.k_lo : 0))));
    return;
  }
  FastFrameG f;
  f.affine_first = a.affine_first != 0;
  f.ni = a.ni; f.nj = a.nj; f.nk = a.nk; f.sci = a.scale_i; f.scj = a.scale_j; f.sck = a.scale_k;
  f.cp = nullptr; f.elastic = false;
  bool weird = false;
  {
    const float* m = a.mapping + (a.mapping_batched ? p.b * 12 : 0);
#pragma unroll
    for (int q = 0; q < 12; q++) {
      const float mv = m[q];
      weird |= (__float_as_uint(mv) & 0x7FFFFFFFu) > 0x7149F2CAu;  // |m| > 1e30, Inf or NaN
      f.m[q] = mv * ratio[q >> 2];
    }
  }
#pragma unroll
  for (int e = 0; e < 3; e++) f.dsc[e] = a.rsp[e] * (f.affine_first ? ratio[e] : 1.0f);
  if constexpr (ELASTIC_POSSIBLE) {
    f.elastic = !(a.cp_skip != nullptr && a.cp_skip[p.b] != 0);
    f.cp = f.elastic ? a.cp + (a.cp_batched ? static_cast<int64_t>(p.b) * (a.ni * a.nj * a.nk * 3) : 0) : nullptr;
  }
  pipe_brick_frame(f, p.j_lo, p.k_lo);
  int ext[7] = {-0x40000000, -0x40000000, -0x40000000, -0x40000000, -0x40000000, -0x40000000, 0};
  const int n_vert = f.elastic ? 27 : 8;
  if (v < n_vert) {
    int r[6]; bool bad;
    pipe_vertex(a, f, v, p.i_begin, p.i_count, p.nv, p.nw, r, bad);
#pragma unroll
    for (int q = 0; q < 6; q++) ext[q] = r[q];
    ext[6] = bad ? 1 : 0;
  }
#pragma unroll
  for (int s = GROUP / 2; s > 0; s >>= 1) {
#pragma unroll
    for (int q = 0; q < 7; q++) ext[q] = max(ext[q], __shfl_xor(ext[q], s));
  }
  // (the butterfly leaves the extremes in EVERY lane of the group: the decisions below are uniform across it)
  const PlanBox whole = plan_box(a, ext, weird);
  const bool wrd = weird | (ext[6] != 0);
  int kind = whole.outside ? kDescOutside : (whole.fits ? kDescStaged : kDescSlow);
  PlanBox first = whole;
  int d15 = 0;
  if (a.plan_multi != 0 && kind == kDescSlow && !wrd) {
    // the box exceeds the tile: halves of the planes, else quarters (pass boxes behind the descriptors)
    int* passes = plan + a.B * 16 + n_items * kDescInts + t * (kPassInts * kPassesPerBrick);
    for (int nsplit = 2; nsplit <= 4; nsplit *= 2) {
      const int span = TI / nsplit;
      bool all_ok = true;
      for (int q = 0; q < nsplit; q++) {
        const int u0 = p.i_begin + q * span, n = min(span, p.i_begin + p.i_count - u0);
        int e7[7] = {-0x40000000, -0x40000000, -0x40000000, -0x40000000, -0x40000000, -0x40000000, 0};
        if (v < n_vert && n > 0) {
          int r[6]; bool bad;
          pipe_vertex(a, f, v, u0, n, p.nv, p.nw, r, bad);
#pragma unroll
          for (int c = 0; c < 6; c++) e7[c] = r[c];
          e7[6] = bad ? 1 : 0;
        }
#pragma unroll
        for (int sft = GROUP / 2; sft > 0; sft >>= 1) {
#pragma unroll
          for (int c = 0; c < 7; c++) e7[c] = max(e7[c], __shfl_xor(e7[c], sft));
        }
        PlanBox pb = plan_pass_box(a, e7, weird);
        if (n <= 0) { pb.outside = 1; pb.fits = 0; pb.interior = 0; }  // (no plane of a partial brick in this part: nothing to do)
        all_ok &= (pb.fits | pb.outside) != 0;
        const int state = pb.outside ? kPassOutside : (pb.fits ? kPassStaged : kPassSlow);
        if (q == 0) { first = pb; d15 = nsplit; }
        d15 |= state << (8 + 4 * q);
        if (v == 0) {
          int* r8 = passes + q * kPassInts;
          r8[0] = pb.xmin; r8[1] = pb.ymin; r8[2] = pb.za; r8[3] = pb.Lx; r8[4] = pb.Ly; r8[5] = pb.cpr;
          r8[6] = state | (pb.interior << 8); r8[7] = max(n, 0);
        }
      }
      kind = kDescMulti;
      if (all_ok) break;
    }
  }
  if (v != 0) return;
  if (kind == kDescMulti && a.plan_multi == 1) {  // ... and listed for the walker blocks of resample_lean_exact_kernel: [0] the count (left at zero by the last launch that read this buffer), [4 ...] the bricks
    int* list = plan + a.B * 16 + n_items * (kDescInts + kPassInts * kPassesPerBrick);
    const int at = atomicAdd(plan - kPlanHeaderInts, 1);
    if (at < n_items) list[at] = t;
  }
  d[10] = p.b; d[11] = p.i_begin; d[12] = p.j_lo; d[13] = p.k_lo; d[15] = d15;
  d[0] = kind | (first.interior << 8);
  d[1] = first.xmin; d[2] = first.ymin; d[3] = first.za; d[4] = first.Lx; d[5] = first.Ly; d[6] = first.cpr;
  const double org[3] = {static_cast<double>(first.xmin), static_cast<double>(first.ymin), static_cast<double>(first.za)};
#pragma unroll
  for (int r = 0; r < 3; r++) d[7 + r] = __float_as_int(static_cast<float>(static_cast<double>(f.m[4 * r]) * p.i_begin + f.c[r] - org[r]));
  d[14] = f.elastic ? 1 : 0;
}

constexpr int kMinSlots = 64;  // keys per channel of the folded minimum

// one 64-lane block per channel: the slots' minimum, decoded; the slots go back to all ones
constexpr int kMinChannels = 16;  // channels of one launch that can fold their minimum (more: the plain reduction)
struct MinOuts { float* p[kMinChannels]; };

__global__ __launch_bounds__(kMinSlots) void min_finish_kernel(uint32_t* __restrict__ keys, const MinOuts outs, int n_channels) {
  const int c = blockIdx.x;
  if (c >= n_channels) return;
  uint32_t* slot = keys + c * kMinSlots + threadIdx.x;
  const uint32_t k = __hip_atomic_exchange(slot, 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t m = wave_min_u32(k);
  if (threadIdx.x == 0) *outs.p[c] = key_to_float(m);
}

struct LeanArgs {
  const float* in;    // channel c of a (B, C, I, J, K) image: base pointer of (0, c), batch elements in_stride apart
  float* out;         // the same channel of the (B, C, Io, Jo, Ko) output, batch elements out_stride apart
  int64_t in_stride, out_stride;
  const float* fill;  // one float, or nullptr (no fill rule)
  const int* plan;    // plan_bricks_kernel's output
  const float* cp;    // control points (ELASTIC_POSSIBLE) or nullptr
  int I, J, K, Io, Jo, Ko;
  int B, n_items;
  unsigned bricks_per_element, bpe_magic;
  int ni, nj, nk, cp_batched;
  float sci, scj, sck;
  float dsc[3];
  float hx, hy, hz;
  int affine_first, ablate;
  // what the exact chain of the fill recheck reads (resample_exact_chain.hpp; only voxels whose in-bounds weight is within
  // a margin of 1/2 get there): the unscaled mapping, the spacings, the normalisation divisors
  const float* mapping;
  int mapping_batched, unit_spacing, fill_recheck;
  float sp[3], rsp[3], den[3], rden[3];
  // resample_lean_exact.hpp: the folded normalise round trip (den / 2, its reciprocal, (S - 1) / 2) and the A/B switch of its
  // interleaved DMA issue
  float dh[3], rdh[3], half_h[3];
  int interleave;
  int tile_floats;  // floats of ONE staging tile of this launch (the planner's tile_cap)
  int last_use;     // resample_lean_exact_multi_kernel: this launch is the last one that reads the plan (the last walker zeroes the list's length)
  // the folded minimum (tio_resample_image.out_min_dev): kMinSlots keys of this channel, or nullptr.  Only the bricks of batch
  // element 0 track what they store (a block-uniform branch into the TRACK instantiation of the sampling loop).
  uint32_t* min_keys;
  // resample_lean_exact_pair_kernel (round 6): a SECOND channel of the same geometry — another image of the subject or another channel
  // of this one — sampled by the same block from the same coordinates (the box is staged again into the same tile)
  const float* in2;
  float* out2;
  int64_t in_stride2, out_stride2;
  const float* fill2;
  // resample_lean_exact_label_kernel (round 6): ONE nearest-neighbour label channel of the same geometry riding along — element bits of
  // lab_es bytes (1, 2 or 4), no fill rule (zero padding) — sampled from the same coordinates behind the float channels
  const void* lab_in;
  void* lab_out;
  int lab_es;
};

}  // namespace tio
