// resample_args.hpp — the argument blocks of the resampling kernels (resample.hip fills them; every resample_*.hpp reads them).
#pragma once
#include "common.hpp"

namespace tio {
struct ImgArgs {
  const void* in;
  void* out;
  const float* fill;  // nullptr → no mask step
  int channels;
  int dtype;
  int interp;
  // TIO_LABEL_PV only: sorted label table (may be null), its length, the pad label
  const double* labels;
  int n_labels;
  double pad_label;
  // the folded minimum (planned FAST launches): per-channel result, and this image's first key in the workspace
  float* out_min;
  uint32_t* min_keys;
};

struct ResampleArgs {
  int B;
  int I, J, K;
  int Io, Jo, Ko;
  int affine_first;
  const float* mapping;
  int mapping_batched;
  const float* cp;
  int cp_batched;
  int ni, nj, nk;
  const uint8_t* cp_skip;
  const uint8_t* passthrough;
  float sp[3], rsp[3];              // mm → voxel spacing and its float32 reciprocal
  int unit_spacing;                 // all three spacings == 1.0f: d / 1 is the identity
  float scale_i, scale_j, scale_k;  // ATen lerp scales of the control grid
  float den[3], rden[3];            // max(S-1,1) per input axis and reciprocal
  float size_m1[3];                 // S-1 per input axis
  float dh[3], rdh[3], half_h[3];   // den/2, its reciprocal, (S-1)/2: the folded normalise round trip
  int short_div;                    // every den <= 8192: one division refinement is exact
  int any_linear, any_nearest;      // which coordinate products are needed at all
  int n_images;
  ImgArgs img[TIO_MAX_IMAGES];
  int tiles_k, tiles_j, tiles_i;
  unsigned magic_k, magic_j, magic_i;  // multiply-high reciprocals of the tile counts (tile kernel)
  int cp_lds;    // floats of LDS reserved for the control points (0 = read them from global)
  int tile_cap;  // floats of LDS available for one staged input brick (tile kernel)
  int any_fill;      // an image of the launch has a fill rule
  int plan_multi;    // plan_bricks_kernel: bricks whose box exceeds the tile get pass boxes over halves / quarters of their planes (the exact-coordinate lean kernel reads them)
  int fill_recheck;  // FAST kernels: voxels whose in-bounds weight is within a margin of 1/2 take the exact chain's decision (A/B: TIO_FAST_FILL_RECHECK=0)
};

// resample.hip: the checks of a tio_resample_geom and the part of ResampleArgs every launch of that geometry shares (an empty batch leaves
// a.B == 0); for the entry points in other files that take the same geometry (resample_geometry_grad.hip)
int resample_check_geometry(const tio_resample_geom* geom, ResampleArgs& a);
}  // namespace tio
