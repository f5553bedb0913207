// resample_line.hpp — the source coordinate of a column of output voxels as a LINE in the plane index, box-relative
// (x(t) = A + t B per control cell, the constant formed in float64), and the column helpers built on it: the frame of a
// brick, the displacement and coordinate of a point in it, the cell breakpoints, the eight-tap gather from a staged box with
// its separable fill rule, and the per-column line through a run of planes.  Used by the FAST kernels (resample_fast.hpp),
// by the planner (resample_plan.hpp: the vertices of a brick), by the lean exact kernel (resample_lean_exact.hpp) and by the
// exact nearest kernel (resample_nearest.hpp).
#pragma once
#include "resample_coords.hpp"
#include "resample_tile.hpp"

namespace tio {

typedef __attribute__((address_space(3))) const float* fast_lds_ptr;
typedef __attribute__((address_space(3))) float* fast_lds_wptr;

// continuous position along one control axis -> cell and weight (ATen's align_corners lerp,
// extended to non-integer positions; NaN positions land in cell 0 with weight 0)
__device__ __forceinline__ void fast_axis(float src, int n, int& i0, int& i1, float& l) {
  const float c = fminf(fmaxf(floorf(src), 0.0f), static_cast<float>(n > 1 ? n - 2 : 0));
  i0 = static_cast<int>(c);
  i1 = min(i0 + 1, n - 1);
  l = fminf(fmaxf(src - c, 0.0f), 1.0f);
}

template <typename CP>
struct FastFrameT {
  float m[12];            // voxel mapping (rows scaled by the normalisation ratio of the axis)
  double c[3];            // mapping applied to (0, j_lo, k_lo)
  int j_lo, k_lo;
  bool elastic, affine_first;
  CP cp;                  // control points of this batch element (LDS copy in the streaming kernel, global in the brick kernel)
  int ni, nj, nk;
  float sci, scj, sck;    // control-grid lerp scales
  float dsc[3];           // displacement scale: 1 / spacing (times the axis ratio when affine_first)
};

// displacement (already in voxels) at the volume position (i, j, k), any of them fractional
template <typename CP>
__device__ __forceinline__ void fast_displacement(const FastFrameT<CP>& f, float pi, float pj, float pk, float (&d)[3]) {
  int i0, i1, j0, j1, k0, k1;
  float li, lj, lk;
  fast_axis(f.sci * pi, f.ni, i0, i1, li);
  fast_axis(f.scj * pj, f.nj, j0, j1, lj);
  fast_axis(f.sck * pk, f.nk, k0, k1, lk);
  const int s_i = f.nj * f.nk * 3, s_j = f.nk * 3;
#pragma unroll
  for (int e = 0; e < 3; e++) {
    const CP p = f.cp + e;
    const float a00 = p[i0 * s_i + j0 * s_j + k0 * 3], a01 = p[i0 * s_i + j0 * s_j + k1 * 3];
    const float a10 = p[i0 * s_i + j1 * s_j + k0 * 3], a11 = p[i0 * s_i + j1 * s_j + k1 * 3];
    const float b00 = p[i1 * s_i + j0 * s_j + k0 * 3], b01 = p[i1 * s_i + j0 * s_j + k1 * 3];
    const float b10 = p[i1 * s_i + j1 * s_j + k0 * 3], b11 = p[i1 * s_i + j1 * s_j + k1 * 3];
    const float a0 = __builtin_fmaf(lk, a01 - a00, a00), a1 = __builtin_fmaf(lk, a11 - a10, a10);
    const float b0 = __builtin_fmaf(lk, b01 - b00, b00), b1 = __builtin_fmaf(lk, b11 - b10, b10);
    const float av = __builtin_fmaf(lj, a1 - a0, a0), bv = __builtin_fmaf(lj, b1 - b0, b0);
    d[e] = __builtin_fmaf(li, bv - av, av) * f.dsc[e];
  }
}

// sampling coordinate (volume frame) of output position (u, j_lo + v, k_lo + w), u / v / w possibly fractional
template <typename CP>
__device__ __forceinline__ void fast_coord(const FastFrameT<CP>& f, float u, float v, float w, float& x, float& y, float& z) {
  float d[3] = {0.0f, 0.0f, 0.0f};
  if (f.elastic) fast_displacement(f, u, static_cast<float>(f.j_lo) + v, static_cast<float>(f.k_lo) + w, d);
  float eu = u, ev = v, ew = w, ax = 0.0f, ay = 0.0f, az = 0.0f;
  if (f.affine_first) { ax = d[0]; ay = d[1]; az = d[2]; } else { eu += d[0]; ev += d[1]; ew += d[2]; }
  x = __builtin_fmaf(f.m[0], eu, __builtin_fmaf(f.m[1], ev, __builtin_fmaf(f.m[2], ew, static_cast<float>(f.c[0])))) + ax;
  y = __builtin_fmaf(f.m[4], eu, __builtin_fmaf(f.m[5], ev, __builtin_fmaf(f.m[6], ew, static_cast<float>(f.c[1])))) + ay;
  z = __builtin_fmaf(f.m[8], eu, __builtin_fmaf(f.m[9], ev, __builtin_fmaf(f.m[10], ew, static_cast<float>(f.c[2])))) + az;
}

// first interior control-cell boundary of the index range [lo, hi] along an axis (lo itself when
// there is none); `dense` is raised when a second one follows
__device__ __forceinline__ float fast_breakpoint(float sc, int n, int lo, int hi, bool& dense) {
  if (n <= 2 || !(sc > 0.0f)) return static_cast<float>(lo);
  const float cell_lo = fminf(fmaxf(floorf(sc * static_cast<float>(lo)), 0.0f), static_cast<float>(n - 2));
  const float cell_hi = fminf(fmaxf(floorf(sc * static_cast<float>(hi)), 0.0f), static_cast<float>(n - 2));
  if (cell_hi <= cell_lo) return static_cast<float>(lo);
  dense |= cell_hi > cell_lo + 1.0f;
  return fminf(fmaxf((cell_lo + 1.0f) / sc, static_cast<float>(lo)), static_cast<float>(hi));
}

struct FastTaps {
  float v[8];
  float fx, fy, fz;
};

struct FastAddr {
  float sXf, sYf, base_f;
  unsigned sXb, sYb, sXYb;
};

__device__ __forceinline__ void fast_issue(FastTaps& ts, float x, float y, float z, const FastAddr& ta) {
  const float x0 = floorf(x), y0 = floorf(y), z0 = floorf(z);
  ts.fx = x - x0; ts.fy = y - y0; ts.fz = z - z0;
  // LDS byte address in float32 (every term an integer far below 2^24: exact), one conversion
  const float af = __builtin_fmaf(x0, ta.sXf, __builtin_fmaf(y0, ta.sYf, __builtin_fmaf(z0, 4.0f, ta.base_f)));
  const unsigned addr = static_cast<unsigned>(static_cast<int>(af));
  fast_lds_ptr q00 = reinterpret_cast<fast_lds_ptr>(static_cast<uintptr_t>(addr));
  fast_lds_ptr q10 = reinterpret_cast<fast_lds_ptr>(static_cast<uintptr_t>(addr + ta.sXb));
  fast_lds_ptr q01 = reinterpret_cast<fast_lds_ptr>(static_cast<uintptr_t>(addr + ta.sYb));
  fast_lds_ptr q11 = reinterpret_cast<fast_lds_ptr>(static_cast<uintptr_t>(addr + ta.sXYb));
  ts.v[0] = q00[0]; ts.v[4] = q00[1];
  ts.v[1] = q10[0]; ts.v[5] = q10[1];
  ts.v[2] = q01[0]; ts.v[6] = q01[1];
  ts.v[3] = q11[0]; ts.v[7] = q11[1];
}

__device__ __forceinline__ float fast_finish(const FastTaps& ts) {
  const float a00 = __builtin_fmaf(ts.fz, ts.v[4] - ts.v[0], ts.v[0]);
  const float a10 = __builtin_fmaf(ts.fz, ts.v[5] - ts.v[1], ts.v[1]);
  const float a01 = __builtin_fmaf(ts.fz, ts.v[6] - ts.v[2], ts.v[2]);
  const float a11 = __builtin_fmaf(ts.fz, ts.v[7] - ts.v[3], ts.v[3]);
  const float b0 = __builtin_fmaf(ts.fy, a01 - a00, a00);
  const float b1 = __builtin_fmaf(ts.fy, a11 - a10, a10);
  return __builtin_fmaf(ts.fx, b1 - b0, b0);
}

// separable form of the in-bounds weight sum; (x0, y0, z0) = first-tap indices in the volume's frame
__device__ __forceinline__ float fast_mask(const FastTaps& ts, float x0, float y0, float z0, float hx, float hy, float hz) {
  const float mx = (((x0 >= 0.0f) & (x0 <= hx)) ? 1.0f - ts.fx : 0.0f) + (((x0 >= -1.0f) & (x0 <= hx - 1.0f)) ? ts.fx : 0.0f);
  const float my = (((y0 >= 0.0f) & (y0 <= hy)) ? 1.0f - ts.fy : 0.0f) + (((y0 >= -1.0f) & (y0 <= hy - 1.0f)) ? ts.fy : 0.0f);
  const float mz = (((z0 >= 0.0f) & (z0 <= hz)) ? 1.0f - ts.fz : 0.0f) + (((z0 >= -1.0f) & (z0 <= hz - 1.0f)) ? ts.fz : 0.0f);
  return mx * my * mz;
}

// n planes of this thread's column: coordinate(t) = (ax, ay, az) + t (bxs, bys, bzs), box-relative.
// G voxels have their LDS reads in flight before the first interpolation starts.  The output
// address is a block-uniform running pointer (one plane = slab_b bytes) + this thread's byte offset.
// TRACK: the ordered-integer key of the smallest value stored (the folded minimum of the launch's own output)
// MASKED: the fill rule.  The FAST in-bounds weight decides; a voxel whose weight is within `margin` of 1/2 additionally
// raises bit (plane_base + its index in the run) of `unsure`: the kernel's tail re-decides those with the reference's
// exact chain (resample_exact_chain.hpp).  margin < 0: nothing is ever recorded (A/B: TIO_FAST_FILL_RECHECK=0).
template <bool MASKED, int G, bool NOSTORE = false, bool TRACK = false>
__device__ __forceinline__ void fast_sample_run(int n, float ax, float ay, float az, float bxs, float bys, float bzs, const FastAddr& ta,
                                                char* out_generic, unsigned urow, int64_t slab_b, float ox, float oy, float oz, float hx,
                                                float hy, float hz, float fillv, uint32_t& kmin, float margin, int plane_base, unsigned& unsure) {
  // The running pointer passes through an empty asm (to pin it to scalar registers), which hides its address space
  // from the compiler: it MUST be typed global here, or the stores become flat_store_dword — flat operations count
  // on lgkmcnt as well, so every wait for the LDS taps would also wait for the previous voxels' stores to be
  // acknowledged by memory (measured: the whole sampling phase then runs at the store round-trip time).
  typedef __attribute__((address_space(1))) char* global_char_ptr;
  typedef __attribute__((address_space(1))) float* global_float_ptr;
  global_char_ptr out_t = (global_char_ptr)out_generic;
  const float bxg = static_cast<float>(G) * bxs, byg = static_cast<float>(G) * bys, bzg = static_cast<float>(G) * bzs;
  // full groups store unconditionally — one basic block, so the scheduler can interleave the G voxels' dependent
  // chains (a lone wave on its SIMD pays ~9 clocks per DEPENDENT instruction) — then one guarded tail group
#pragma unroll 1
  for (int tg = 0; tg < n; tg += G) {
    FastTaps ts[G];
    float x0s[G], y0s[G], z0s[G];
#pragma unroll
    for (int q = 0; q < G; q++) {
      const float qf = static_cast<float>(q);
      const float x = q == 0 ? ax : __builtin_fmaf(qf, bxs, ax);
      const float y = q == 0 ? ay : __builtin_fmaf(qf, bys, ay);
      const float z = q == 0 ? az : __builtin_fmaf(qf, bzs, az);
      fast_issue(ts[q], x, y, z, ta);
      if constexpr (MASKED) { x0s[q] = x - ts[q].fx; y0s[q] = y - ts[q].fy; z0s[q] = z - ts[q].fz; }
    }
    __builtin_amdgcn_sched_barrier(0);
    float vals[G];
    unsigned redo = 0u;  // voxels of this group the tail will store again (their first value never reaches the folded minimum)
#pragma unroll
    for (int q = 0; q < G; q++) {
      vals[q] = fast_finish(ts[q]);
      if constexpr (MASKED) {
        const float mk = fast_mask(ts[q], x0s[q] + ox, y0s[q] + oy, z0s[q] + oz, hx, hy, hz);
        vals[q] = (mk > 0.5f) ? vals[q] : fillv;
        // (a NaN weight compares false: the FAST answer — fill — stands; planes beyond the run are never raised)
        const bool again = (fabsf(mk - 0.5f) <= margin) & (tg + q < n);
        unsure |= again ? (1u << (plane_base + tg + q)) : 0u;
        if constexpr (TRACK) redo |= again ? (1u << q) : 0u;
      }
    }
    // (the row offset re-enters the block as a 32-bit register: instruction selection works block by block, and only a zero
    // extension it can SEE lets the store take the `scalar base + 32-bit vector offset` form — one 64-bit vector add per store less)
    unsigned row_off = urow;
    asm volatile("" : "+v"(row_off));
    if (tg + G <= n) {
#pragma unroll
      for (int q = 0; q < G; q++) {
        if (!NOSTORE || vals[q] == 1.2345e37f) *(global_float_ptr)(out_t + row_off) = vals[q];
        if constexpr (TRACK) kmin = ((redo >> q) & 1u) ? kmin : min(kmin, float_to_key(vals[q]));
        out_t += slab_b;
        asm volatile("" : "+s"(out_t));  // one running pointer (2 scalar adds per plane), not G precomputed ones
      }
    } else {
#pragma unroll
      for (int q = 0; q < G; q++) {
        if (tg + q < n) {
          unsigned tail_off = row_off;  // (its own block)
          asm volatile("" : "+v"(tail_off));
          if (!NOSTORE || vals[q] == 1.2345e37f) *(global_float_ptr)(out_t + tail_off) = vals[q];
          if constexpr (TRACK) kmin = ((redo >> q) & 1u) ? kmin : min(kmin, float_to_key(vals[q]));
        }
        out_t += slab_b;
        asm volatile("" : "+s"(out_t));
      }
    }
    ax += bxg; ay += byg; az += bzg;
    __builtin_amdgcn_sched_barrier(0);
  }
}


// ---- the coordinate line of one column through a run of planes inside ONE control cell ---------------------
// x(run0 + t) = A + t B, box-relative: C3 = mapping of (u_ref, j_lo, k_lo) relative to the box origin (float64 ->
// float32, block uniform), col3 = the column's own (v, w) offset through the mapping, the elastic part as a linear
// function of the plane index inside the cell.  Returns the end of the run (the next cell boundary or `limit`).
struct ColumnPlanes {
  int cell;        // control cell whose end planes are cached (-2: none)
  float P0[3], P1[3];
};

template <typename CP>
__device__ __forceinline__ int fast_column_line(const FastFrameT<CP>& f, const Lerp1D& lj, const Lerp1D& lk, ColumnPlanes& cache, int run0,
                                                int limit, int u_ref, const float (&C3)[3], const float (&col3)[3], int lane,
                                                float (&A3)[3], float (&B3)[3]) {
  int run1 = limit;
  const float du = static_cast<float>(run0 - u_ref);
  if (f.elastic) {
    const int cmax = f.ni > 1 ? f.ni - 2 : 0;
    const int cell_l = min(max(static_cast<int>(floorf(f.sci * static_cast<float>(run0 + lane))), 0), cmax);
    const int cell = __builtin_amdgcn_readlane(cell_l, 0);
    const unsigned long long later = __builtin_amdgcn_ballot_w64((lane < run1 - run0) & (cell_l > cell));
    if (later != 0ull) run1 = run0 + __builtin_ctzll(later);
    if (cell != cache.cell) {  // (j, k)-lerped control planes at the two ends of the cell
      const int s_i = f.nj * f.nk * 3, s_j = f.nk * 3;
      const int c1 = min(cell + 1, f.ni - 1);
#pragma unroll
      for (int e = 0; e < 3; e++) {
        const CP q = f.cp + e;
        const float a00 = q[cell * s_i + lj.i0 * s_j + lk.i0 * 3], a01 = q[cell * s_i + lj.i0 * s_j + lk.i1 * 3];
        const float a10 = q[cell * s_i + lj.i1 * s_j + lk.i0 * 3], a11 = q[cell * s_i + lj.i1 * s_j + lk.i1 * 3];
        const float b00 = q[c1 * s_i + lj.i0 * s_j + lk.i0 * 3], b01 = q[c1 * s_i + lj.i0 * s_j + lk.i1 * 3];
        const float b10 = q[c1 * s_i + lj.i1 * s_j + lk.i0 * 3], b11 = q[c1 * s_i + lj.i1 * s_j + lk.i1 * 3];
        const float a0 = __builtin_fmaf(lk.l1, a01 - a00, a00), a1 = __builtin_fmaf(lk.l1, a11 - a10, a10);
        const float b0 = __builtin_fmaf(lk.l1, b01 - b00, b00), b1 = __builtin_fmaf(lk.l1, b11 - b10, b10);
        cache.P0[e] = __builtin_fmaf(lj.l1, a1 - a0, a0);
        cache.P1[e] = __builtin_fmaf(lj.l1, b1 - b0, b0);
      }
      cache.cell = cell;
    }
    // d(run0 + t) = P0 + (sci (run0 + t) - cell) (P1 - P0)
    const float l_ref = fminf(fmaxf(__builtin_fmaf(f.sci, static_cast<float>(run0), -static_cast<float>(cell)), 0.0f), 1.0f);
    float D0[3], D1[3];
#pragma unroll
    for (int e = 0; e < 3; e++) {
      const float dP = cache.P1[e] - cache.P0[e];
      D0[e] = __builtin_fmaf(l_ref, dP, cache.P0[e]) * f.dsc[e];
      D1[e] = f.sci * dP * f.dsc[e];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) {
      if (f.affine_first) {
        A3[r] = __builtin_fmaf(f.m[4 * r], du, C3[r] + col3[r]) + D0[r];
        B3[r] = f.m[4 * r] + D1[r];
      } else {
        A3[r] = __builtin_fmaf(f.m[4 * r], du + D0[0], __builtin_fmaf(f.m[4 * r + 1], D0[1], __builtin_fmaf(f.m[4 * r + 2], D0[2], C3[r] + col3[r])));
        B3[r] = __builtin_fmaf(f.m[4 * r], 1.0f + D1[0], __builtin_fmaf(f.m[4 * r + 1], D1[1], f.m[4 * r + 2] * D1[2]));
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 3; r++) { A3[r] = __builtin_fmaf(f.m[4 * r], du, C3[r] + col3[r]); B3[r] = f.m[4 * r]; }
  }
  return run1;
}

// Sample one run with the cheapest loop that is correct for it: the fill rule only matters where a tap can leave
// the volume.  Each coordinate of the line is monotone, so a column whose two END planes keep all first taps in
// [0, S - 2] is interior for the whole run; the wave takes the masked loop only if one of its columns is not.
template <int GMAX, bool TRACK = false>
__device__ __forceinline__ void fast_sample_line(int len, const float (&A3)[3], const float (&B3)[3], const FastAddr& ta, char* o, unsigned urow,
                                                 int64_t slab_b, bool needs_mask, float ox, float oy, float oz, float hx, float hy, float hz,
                                                 float fillv, uint32_t& kmin, float margin, int plane_base, unsigned& unsure) {
  bool masked = false;
  if (needs_mask) {
    const float el = static_cast<float>(len - 1);
    const float xa = A3[0] + ox, xb = __builtin_fmaf(el, B3[0], A3[0]) + ox;
    const float ya = A3[1] + oy, yb = __builtin_fmaf(el, B3[1], A3[1]) + oy;
    const float za = A3[2] + oz, zb = __builtin_fmaf(el, B3[2], A3[2]) + oz;
    const bool inside = (fminf(xa, xb) >= 0.0f) & (fmaxf(xa, xb) < hx) & (fminf(ya, yb) >= 0.0f) & (fmaxf(ya, yb) < hy) &
                        (fminf(za, zb) >= 0.0f) & (fmaxf(za, zb) < hz);
    masked = __builtin_amdgcn_ballot_w64(!inside) != 0ull;
  }
  if (!masked) {
    if (GMAX == 8 && len > 4)
      fast_sample_run<false, 8, false, TRACK>(len, A3[0], A3[1], A3[2], B3[0], B3[1], B3[2], ta, o, urow, slab_b, 0.f, 0.f, 0.f, hx, hy, hz, fillv, kmin, margin, plane_base, unsure);
    else
      fast_sample_run<false, 4, false, TRACK>(len, A3[0], A3[1], A3[2], B3[0], B3[1], B3[2], ta, o, urow, slab_b, 0.f, 0.f, 0.f, hx, hy, hz, fillv, kmin, margin, plane_base, unsure);
  } else {  // rare (waves on the volume's surface): four voxels in flight keep the register budget of the common loop
    fast_sample_run<true, 4, false, TRACK>(len, A3[0], A3[1], A3[2], B3[0], B3[1], B3[2], ta, o, urow, slab_b, ox, oy, oz, hx, hy, hz, fillv, kmin, margin, plane_base, unsure);
  }
}

typedef FastFrameT<const float*> FastFrameG;

}  // namespace tio
