/*
 * tio_hip.h — C ABI of the MI355X (gfx950) 3-D augmentation engine.
 *
 * This is the drop-in boundary.  The reference (TorchIO 2.0.0a2)
 * has no FFI of its own: its transforms call torch.nn.functional directly.  Each
 * entry point below replaces one of the reference's private functional seams;
 * the file:line next to it is the reference code whose arithmetic it reproduces.
 *
 * Conventions
 *   - every pointer named *_dev (and x / y / in / out) is DEVICE memory unless
 *     the comment says HOST; nothing here allocates or frees the caller's tensors, and nothing synchronises in the
 *     steady state (two entry points keep a small scratch array per (device, stream) for themselves — the brick plan
 *     of large tio_resample3d launches, the keys of tio_channel_min — allocated on first use and grown on demand,
 *     which synchronises that one time; do not capture their first call into a graph);
 *   - tensors are dense row-major (B, C, I, J, K) — K fastest — exactly the
 *     layout of ImagesBatch.data (reference src/torchio/data/batch.py:21-50);
 *   - alignment of the element type suffices for every pointer unless an entry point asks for more (plan_dev,
 *     tio_blur_fused, noise_base_dev, tio_unique_labels: 16 bytes) — the 16-byte roads look at the pointers they are
 *     given and leave the work to their element-wise twins, same values, when a dense view starts off such a boundary;
 *   - inputs are borrowed, outputs must not alias inputs;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - every function returns TIO_OK (0) or a negative tio_status; the failing
 *     call's message is available through tio_last_error() (thread-local);
 *   - re-entrant: no global mutable state besides the thread-local error text and those mutex-guarded scratch tables
 *     (the reference calls transforms from Queue worker threads, src/torchio/data/queue.py:119-123); calls that share
 *     a stream are ordered by it, calls on different streams use different scratch.
 *
 * The CPU restatement in oracle/ exports the same functions with the prefix
 * tio_oracle_ and HOST pointers (stream ignored); it is test infrastructure.
 */
#ifndef TIO_HIP_H
#define TIO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIO_ABI_VERSION 18
#define TIO_MAX_IMAGES 8 /* images resampled per launch with shared coordinates */

typedef enum tio_status {
  TIO_OK = 0,
  TIO_ERR_INVALID_ARGUMENT = -1,
  TIO_ERR_UNSUPPORTED_DTYPE = -2,
  TIO_ERR_LAUNCH = -3,
  TIO_ERR_NO_DEVICE = -4,
  TIO_ERR_UNSUPPORTED_CONFIG = -5 /* valid arguments, but this fused form is not available for them: nothing was launched */
} tio_status;

/* Element types of image tensors (torch dtype ↔ code is fixed here). */
typedef enum tio_dtype {
  TIO_F32 = 0,
  TIO_F64 = 1,
  TIO_F16 = 2,
  TIO_BF16 = 3,
  TIO_U8 = 4,
  TIO_I8 = 5,
  TIO_I16 = 6,
  TIO_I32 = 7,
  TIO_I64 = 8
} tio_dtype;

typedef enum tio_precision {
  TIO_PRECISION_EXACT = 0,
  TIO_PRECISION_FAST = 1,
  TIO_PRECISION_TIGHT = 2 /* ABI 13: the reference's coordinates, taps and fill decisions bit for bit; fused interpolation */
} tio_precision;

typedef enum tio_interp {
  TIO_NEAREST = 0, /* grid_sample(mode="nearest"): nearbyint, half-to-even      */
  TIO_LINEAR = 1,  /* grid_sample(mode="bilinear"): 8-tap trilinear, zero pad   */
  /* label_interpolation="label" with one_hot_label_interpolation="linear", C == 1,
   * no antialias (_resample_label_partial_volume, spatial.py:1275-1389), fused:
   * the one-hot (B, L, I, J, K) tensor is never built.  Per output voxel the value of
   * one-hot channel l is the sum, in ATen's tap order, of the trilinear weights of
   * the in-bounds taps that carry label l; the winner is torch.argmax's (first
   * maximum = smallest label); the voxel is in bounds when the float32 sum over the
   * channels (torch.sum's cascade over the sorted label table) exceeds 0.5, else it
   * receives the pad label.                                                       */
  TIO_LABEL_PV = 2,
  /* The ADJOINT of TIO_LINEAR — the backward pass of the trilinear resampling with respect to the image
   * (what autograd derives from grid_sample in the reference, whose transforms are differentiable:
   * tests/test_noise.py:75-80, docs/concepts/transforms.md:289-299).  For such an image the roles of the two
   * buffers are swapped: `out` is READ, (B, C, Io, Jo, Ko) float32 = dL/d(output); `in` is ACCUMULATED INTO
   * (despite the const), (B, C, I, J, K) float32, zero-initialised by the caller: every output voxel adds
   * g * w_t to its in-bounds taps (hardware float atomics: the order of the additions is not defined).  A
   * non-NULL fill_dev means the forward pass used a fill value: voxels whose in-bounds weight is <= 0.5 took the
   * fill and carry no gradient.  Same geometry struct, same coordinate arithmetic as the forward launch.     */
  TIO_LINEAR_ADJOINT = 3,
  /* B-spline interpolation of order 2 / 3 — the reference's orders >= 2 go to torch-interpol (spatial.py:1734-1761:
   * interpol.grid_pull(data.float(), grid, interpolation=order, bound="dct2", extrapolate=False, prefilter=True)).
   * Here `in` holds the B-spline COEFFICIENTS of the image (float32, tio_bspline_prefilter), `out` is float32 (the
   * caller casts back like `.to(data.dtype)`), and each output voxel is the (order + 1)^3-tap sum of the basis weights at
   * its voxel coordinate — the coordinate the reference hands to grid_pull, i.e. BEFORE grid_sample's normalise /
   * un-normalise round trip — with half-sample-symmetric ("dct2") index reflection, and zero wherever a coordinate lies
   * outside (-0.05, S - 1 + 0.05) (grid_pull's extrapolate=False mask); fill_dev is ignored, as the reference ignores
   * its fill value on this road.  torch-interpol is not vendored by the reference (pyproject.toml:46) and absent from
   * the build image: the arithmetic follows its published algorithm, pinned against scipy.ndimage (mode="reflect",
   * the same extension) instead of against the package itself — "parity unpinned" in DESIGN.md.                      */
  TIO_QUADRATIC = 4,
  TIO_CUBIC = 5,
  /* Orders 4 - 7 ("fourth" ... "seventh", ABI 10): the same road — prefilter (2 / 2 / 3 / 3 poles), then the (order + 1)^3
   * taps.  The basis weights of these orders come from the Cox - de Boor recursion of the uniform B-spline, evaluated in
   * float64 and rounded to float32 (every term positive: no cancellation; the truncated-power form loses four digits at
   * order 7), identically in the oracle and on the device.  Orders 4 and 5 are pinned against scipy.ndimage like 2 and 3;
   * scipy stops at 5, so 6 and 7 are held to what defines them: the interpolation property, partition of unity, exact
   * reproduction of polynomials up to the order, and a float64 numpy reference built from scipy.interpolate.BSpline
   * (tests/test_bspline.py).  Parity with the reference (torch-interpol) stays unpinned, as for orders 2 and 3.          */
  TIO_BSPLINE4 = 6,
  TIO_BSPLINE5 = 7,
  TIO_BSPLINE6 = 8,
  TIO_BSPLINE7 = 9
} tio_interp;
/* B-spline order of an interpolation code (0 for the others) */
#define TIO_BSPLINE_ORDER(interp) ((interp) == TIO_QUADRATIC ? 2 : (interp) == TIO_CUBIC ? 3 : ((interp) >= TIO_BSPLINE4 && (interp) <= TIO_BSPLINE7) ? (interp) - 2 : 0)

/* ------------------------------------------------------------------------ */
/* Fused spatial resampling                                                  */
/* ------------------------------------------------------------------------ */

/*
 * Geometry shared by every image of one resampling launch.  Replaces the
 * materialised (I,J,K,3) sampling grid of the reference:
 *   _build_sampling_grid            spatial.py:1504-1579
 *   _output_voxel_coordinates       spatial.py:1604-1613
 *   _apply_voxel_mapping            spatial.py:1616-1624   ([c,1] @ M^T, float32)
 *   _upsample_displacement_field    spatial.py:2171-2189   (trilinear, align_corners)
 *   _voxel_coordinates_to_grid      spatial.py:1627-1648   (g = 2 v / max(S-1,1) - 1)
 *   ATen grid_sampler un-normalise  ((g + 1) / 2) * (S - 1)
 *   per-instance variant            spatial.py:1881-1918   (B matrices / fields, no
 *                                                           (B,I,J,K,3) stack)
 *   grid_sample under autograd      spatial.py:1695-1731   (the grid's gradient, chained to the mapping and
 *                                                           the control points: tio_resample3d_geometry_grad)
 */
typedef struct tio_resample_geom {
  int32_t batch;        /* B                                                     */
  int32_t in_shape[3];  /* input  (I, J, K)                                      */
  int32_t out_shape[3]; /* output (I, J, K)                                      */
  int32_t affine_first; /* 1: v = M c + d / in_spacing ; 0: v = M (c + d / out_spacing) */
  /* Output-voxel → input-voxel mapping, float32 rows [m00 m01 m02 m03 | m10 ...]
   * (the first three rows of spatial.py:1582-1601's matrix, already cast to f32).
   * mapping_batched = 0: one 3x4 shared by the batch; 1: B matrices.            */
  const float* mapping_dev;
  int32_t mapping_batched;
  /* Elastic control points in mm, (n, ni, nj, nk, 3) float32, n = B if
   * cp_batched else 1; NULL = no elastic component.                            */
  const float* control_points_dev;
  int32_t cp_batched;
  int32_t cp_shape[3];
  /* Optional per-element flags (B bytes each, NULL = all zero):
   *   cp_skip[b]     != 0 → element b has no elastic component
   *                         (control_points None, spatial.py:1542-1543);
   *   passthrough[b] != 0 → element b is copied bit-exactly (gated-out rows,
   *                         spatial.py:1078-1107); needs in_shape == out_shape. */
  const uint8_t* cp_skip_dev;
  const uint8_t* passthrough_dev;
  float in_spacing[3];  /* AffineMatrix.spacing of the input grid, as float32    */
  float out_spacing[3]; /* ... of the output grid                                */
  /* Shape whose (S - 1) normalises the voxel coordinates before grid_sample un-normalises
   * them with the image's own (S - 1).  The reference builds ONE grid from the first selected
   * image and samples every image with it (spatial.py:1136-1191, 1704), so an image of another
   * shape (Resample("t1") on a multi-resolution subject) sees g = 2 v / (S_first - 1) - 1 but
   * x = ((g + 1) / 2) (S_own - 1).  All zeros = in_shape (the usual case: every image shares it). */
  int32_t norm_shape[3];
  /* tio_precision.  TIO_PRECISION_EXACT (0, the default): the reference's float32 operation
   * sequence, bit for bit.  TIO_PRECISION_FAST: the float32 trilinear images of the call may skip
   * the normalise / un-normalise round trip of the coordinates and interpolate with nested fma
   * lerps — same interpolant, different rounding: within ~1e-5 absolute of the exact result on
   * unit-range data (the north_star bar for intensities is 1e-4 relative).  Nearest-neighbour
   * images WITHOUT a fill rule (label maps) are bit-identical to the reference in either mode
   * and do not hold the float images back (their own kernel: the index of a voxel only
   * depends on its coordinate's rounding, and coordinates within rounding error of a
   * half-integer are re-evaluated with the exact chain); any other image in the call — a
   * nearest image with a fill rule, TIO_LABEL_PV, another dtype — keeps the whole call exact.
   * TIO_PRECISION_TIGHT (ABI 13): every sampling coordinate is the reference's float32 value bit for bit (MKL's FMA
   * order, ATen's lerp nesting, the normalise / un-normalise round trip), hence the same eight taps, the same weights
   * and the same `mask > 0.5` decisions; only the interpolation of the float32 trilinear images is fused (three nested
   * fma lerps instead of ATen's eight weighted taps): the result differs from the reference by the rounding of seven
   * fused multiply-adds (~1e-7 of the taps) and meets |d| <= 1e-4 max(|ref|, 1e-3 range) PER VOXEL on white noise, which
   * TIO_PRECISION_FAST cannot (one ulp of a coordinate is already more).  Launches the lean exact-coordinate kernel does
   * not take (small launches, other dtypes, non-unit spacing with control points) run the exact kernels. */
  int32_t precision;
  /* Optional (NULL / 0 = the call plans for itself): a brick plan made AHEAD of the call by tio_resample3d_plan from a
   * geometry with exactly these fields (ABI 11).  Large launches of 16^3 bricks start from a plan — one descriptor per
   * brick, written by a small kernel that reads only the geometry above (mapping, control points, flags), never the
   * images — and that kernel plus the gap behind it sit on the critical path of the call (~8 - 23 us + ~5 us on the
   * bench launch).  A caller that knows the geometry before the data is ready (a Compose that has drawn every child's
   * parameters) can have the plan made on another stream while earlier work runs.  The plan must stay untouched until
   * the call's kernels have finished; a call that takes another road than the one the plan was made for ignores it.
   * A plan is valid for any number of tio_resample3d calls, one after the other on streams ordered behind each other,
   * whose tio_resample_geom equals the one it was planned with (but for plan_dev / plan_bytes) — `flags` and `precision`
   * included: the library checks only its size, and a plan made under another hint or precision can have the same size
   * and drop bricks.
   * (torchio_amd: Engine.resample_plan tags the plan with that signature, Engine.resample3d hands over only a match.) */
  const void* plan_dev;
  int64_t plan_bytes;
  /* TIO_GEOM_* bits (ABI 14; 0 = none).  Hints of a caller who holds the mappings on the host, about SPEED only: every road
   * computes the same values in the exact modes and stays within its mode's tolerance otherwise.
   * TIO_GEOM_LARGE_BOXES: the input boxes of SOME 16^3 output bricks are expected to exceed the staging tile of the planned
   * roads (an element rotated beyond ~12 degrees about all three axes, a strong zoom).  Without the hint such a brick samples
   * voxel by voxel from global memory (3.5 x the time; fine for the odd brick).  With it (ABI 15) the exact-coordinate lean
   * kernels — TIO_PRECISION_EXACT / TIGHT, large float32 launches — have the planner bound such bricks again in halves /
   * quarters of their planes and list them; a second kernel behind the first walks the list and stages each brick in two or
   * four passes (~6 - 15 us per launch when the list is short: why it is a hint).  FAST launches take the brick kernels with
   * in-kernel boxes, which split such a brick likewise (resample_tile.hpp).
   * TIO_GEOM_MOSTLY_LARGE_BOXES (ABI 15): MOST bricks are expected to — the pass logic then runs in every block of ONE launch
   * (no list, no second kernel; its one-pass bricks cost 2 - 7 % more than without the hint). */
  int32_t flags;
} tio_resample_geom;

#define TIO_GEOM_LARGE_BOXES 1
#define TIO_GEOM_MOSTLY_LARGE_BOXES 2

/* One image tensor resampled with the shared geometry
 * (_resample_image_batch, spatial.py:1194-1272; _sample_batch_grid_sample,
 * spatial.py:1695-1731). */
typedef struct tio_resample_image {
  const void* in;       /* (B, C, I, J, K)                                       */
  void* out;            /* (B, C, Io, Jo, Ko), same dtype                        */
  int32_t channels;     /* C                                                     */
  int32_t dtype;        /* tio_dtype; computed in float32, cast back like
                           `.float()` / `.to(data.dtype)` (spatial.py:1708,1731) */
  int32_t interp;       /* tio_interp                                            */
  /* Per-channel fill (C floats, device).  NULL = reference's "fill is scalar 0"
   * branch (no mask step, spatial.py:2075-2076).  Non-NULL = trilinear in-bounds
   * weight mask, out = mask > 0.5 ? sampled : fill[c]  (spatial.py:1719-1728).  */
  const float* fill_dev;
  /* TIO_LABEL_PV only (ignored otherwise; requires channels == 1).
   *   labels_dev / n_labels: torch.unique(data) of the WHOLE batch tensor as
   *     ascending float64 (spatial.py:1360).  Only the POSITION of a label in this
   *     table matters, and only through the rounding order of the reference's
   *     channel sum (ATen's cascade_sum dumps its accumulator every 16 channels);
   *     NULL / 0 = plain sequential sum in ascending label order, which is what the
   *     cascade does for fewer than 16 distinct labels.
   *   pad_label: default_pad_label, cast to the image dtype like
   *     torch.full_like(resampled, default_pad_label)  (spatial.py:1380-1384).  */
  const double* labels_dev;
  int32_t n_labels;
  double pad_label;
  /* Optional (NULL = not wanted): C floats on the device that receive the per-channel minimum of the FIRST batch
   * element of `out` — what the NEXT transform's default_pad_value="minimum" will ask for (spatial.py:2054-2060,
   * 2094-2095: `tensor[0, c].min()` of the data it is handed).  Large TIO_PRECISION_FAST launches fold it into their
   * stores (no extra pass over the volume); every other launch runs tio_channel_min on `out` before returning.
   * NaN propagates like torch.min.  Ignored for TIO_LINEAR_ADJOINT. */
  float* out_min_dev;
} tio_resample_image;

/* Bytes of the brick plan tio_resample3d would make for this geometry when every image of the call is a float32
 * trilinear image (0: such a call takes a road without a plan — small launches, K not a multiple of 4, ...);
 * geom->plan_dev / plan_bytes are ignored.  Host-only: nothing is enqueued. */
int64_t tio_resample3d_plan_bytes(const tio_resample_geom* geom);
/* Enqueue the planning kernel for this geometry on `stream`: plan_dev (>= tio_resample3d_plan_bytes(geom) bytes,
 * 16-byte aligned) is then handed to tio_resample3d in geom->plan_dev, on any stream ordered behind this one. */
int tio_resample3d_plan(const tio_resample_geom* geom, void* plan_dev, int64_t plan_bytes, void* stream);

/* Resample n_images image tensors through ONE coordinate computation. */
int tio_resample3d(const tio_resample_geom* geom, int32_t n_images,
                   const tio_resample_image* images, void* stream);

/*
 * The gradient of a trilinear resampling with respect to its GEOMETRY: the mapping and the control points (additive to ABI 18,
 * HIP only).  Replaces what autograd derives through the materialised (B, I, J, K, 3) grid of the reference:
 *   _sample_batch_grid_sample       spatial.py:1695-1731   (F.grid_sample under autograd: grid_sampler_3d_backward's grad_grid,
 *                                                           chained back through the grid's construction)
 * One fused launch forms dL/d(coordinate) per output voxel from the incoming gradients and the eight taps and reduces it straight
 * into 12 numbers per mapping and ni * nj * nk * 3 per control grid; no per-voxel gradient field reaches memory.
 *   images[n].in    x_n (B, C_n, I, J, K), one of the four float dtypes (others: TIO_ERR_UNSUPPORTED_DTYPE)
 *   images[n].out   g_n (B, C_n, Io, Jo, Ko) float32 = dL/d(output of the forward), READ
 *   images[n].interp  TIO_LINEAR (anything else: TIO_ERR_INVALID_ARGUMENT); fill_dev as in the forward; the label fields and
 *                   out_min_dev are ignored
 * With the forward's own float32 sampling coordinate of output voxel o = (i, j, k) of element b (the TIO_PRECISION_EXACT chain,
 * whatever geom->precision says, as for TIO_LINEAR_ADJOINT), cell = floor(coordinate):
 *   D_a(o) = sum_n sum_c g_n[b,c,o] * sum_{taps t in bounds} x_n[b,c,t] * s_a(t) * (product of the two other axes' weights of t),
 *            s_a = -1 on the lower tap and +1 on the upper (ATen's grid_sampler_3d_backward, padding_mode="zeros",
 *            align_corners=True); where fill_dev of image n is non-NULL and the in-bounds weight is <= 0.5 the forward wrote
 *            the fill and image n adds nothing at o;
 *   d_a    = D_a * (S_own[a] - 1) / max(S_norm[a] - 1, 1)   (the normalise / un-normalise round trip; exactly 0 where S_own[a] == 1);
 *   affine_first == 1, or no elastic component:   dM[r][0..3] += d_r * (i, j, k, 1),        dDisp[e] = d_e / in_spacing[e];
 *   affine_first == 0 with an elastic component, s = c + disp / out_spacing:
 *                                                 dM[r][0..3] += d_r * (s_0, s_1, s_2, 1),  dDisp[e] = (sum_r M[r][e] d_r) / out_spacing[e];
 *   dCP[node][e] += W(node; i, j, k) * dDisp[e] over the eight nodes of the voxel's control cell, W the align-corners lerp weights
 *            of the forward.
 * An element with passthrough[b] adds nothing; one with cp_skip[b] adds nothing to dCP, its mapping still receives a gradient.
 * d_mapping: float32 (B | 1, 3, 4) as mapping_batched says, d_control_points: float32 in the shape of the control points; shared
 * parameters receive the sum over the batch.  Both are fully overwritten.  Either may be NULL (not wanted; d_control_points must
 * be NULL when the geometry has no control points), not both.  workspace: tio_resample3d_geometry_grad_workspace_bytes(geom) bytes,
 * 8-byte aligned, on the device; its contents on entry do not matter.  Sums across blocks are float64 hardware atomics: two runs
 * differ at most in the last float32 rounding of an output.  plan_dev, precision and flags of the geometry are ignored.
 */
int64_t tio_resample3d_geometry_grad_workspace_bytes(const tio_resample_geom* geom);
int tio_resample3d_geometry_grad(const tio_resample_geom* geom, int32_t n_images, const tio_resample_image* images, float* d_mapping,
                                 float* d_control_points, void* workspace, int64_t workspace_bytes, void* stream);

/* Per-channel minimum of the FIRST batch element, kept on the device (the
 * reference's default_pad_value="minimum": spatial.py:2054-2060,2094-2095 —
 * there a host .item() per channel; here out_dev[c] feeds fill_dev directly).
 * x is (B, C, n_spatial); out_dev receives C floats. */
int tio_channel_min(const void* x, int32_t dtype, int32_t channels,
                    int64_t n_spatial, float* out_dev, void* stream);

/* ------------------------------------------------------------------------ */
/* Intensity path                                                            */
/* ------------------------------------------------------------------------ */

/*
 * Separable 3-axis cross-correlation with replicate padding — the stencil under
 * Blur (blur.py:157-252: F.pad(mode="replicate") + F.conv3d per axis, order
 * I, J, K) and the antialias filter (spatial.py:1980-2031).
 *   taps_dev: (n, 3, tap_stride) float32, n = B if taps_batched else 1; for
 *             axis a the 2*radius[a]+1 centred taps start at offset 0 (already
 *             normalised / zero-extended / delta for sigma = 0 exactly as
 *             blur.py:179-183 and blur.py:292-328 build them);
 *   radius:   HOST int32[3]; radius[a] = 0 skips axis a (sigma <= 0, blur.py:177);
 *   skip_dev: optional B bytes; non-zero rows are copied bit-exactly
 *             (blur.py:249-251).
 *   tmp:      scratch with the size of y (may be NULL when at most one axis is
 *             active).
 * Computes in float32 (blur.py:173 `.float()`), stores dtype (blur.py:204).
 */
int tio_separable_conv3d(const void* x, void* y, void* tmp, int32_t dtype,
                         int32_t batch, int32_t channels, const int32_t shape[3],
                         const float* taps_dev, int32_t taps_batched,
                         int32_t tap_stride, const int32_t radius[3],
                         const uint8_t* skip_dev, void* stream);

/*
 * What tio_separable_conv3d / tio_blur_fused would launch for these arguments (ABI 18).  Host-only: nothing is
 * enqueued and no pointer is read — the launcher and this function share one decision function, so the answer is
 * the launch.  One tio_conv_pass per kernel launch, in launch order.
 *   aligned16: non-zero = x, y and tmp are 16-byte aligned; 0 = x is not (no 16-byte kernel runs);
 *   has_skip:  a skip_dev would be passed;
 *   bias_on / noise_on (0, 1, 2) / fast_math: the stages of tio_blur_fused; any of them non-zero asks about
 *              tio_blur_fused (TIO_ERR_UNSUPPORTED_CONFIG where that entry point returns it).
 * Returns the number of passes (0 .. 3; 0 = every radius is 0, or an empty batch) or a negative tio_status:
 * TIO_ERR_INVALID_ARGUMENT where the launch would be refused before anything runs — a pass whose lines, counted as
 * (the other non-K axis, or I for the K pass) x batch x channels, exceed 65 535.
 * Honours TIO_CONV_RING and TIO_CONV_NO_FUSE as the launcher does.
 */
typedef enum tio_conv_family {
  TIO_CONV_LINE = 0,  /* generic I / J kernel: any dtype, any alignment; 32-row tiles */
  TIO_CONV_K = 1,     /* generic K kernel */
  TIO_CONV_K_V4 = 2,  /* 16-byte K kernel */
  TIO_CONV_MARCH = 3, /* register-window marching kernel (I / J, radius <= 8) */
  TIO_CONV_RING = 4   /* LDS-ring marching kernel (I / J, radius <= 16) */
} tio_conv_family;

typedef struct tio_conv_pass {
  int32_t axis;             /* 0 = I, 1 = J, 2 = K */
  int32_t family;           /* tio_conv_family */
  int32_t radius;           /* run-time radius along `axis` */
  int32_t radius_class;     /* TIO_CONV_MARCH: the compile-time radius of the instantiation; otherwise 0 */
  int32_t radius_k;         /* > 0: the K taps of this radius are applied to every row the pass stores (fused J + K) */
  int32_t pre_bias;         /* the bias field multiplies the rows this pass loads */
  int32_t post_noise;       /* 0 = none, 1 = Philox draws, 2 = explicit draws added to the rows this pass stores */
  int32_t fma;              /* taps accumulate with fused multiply-adds */
  int32_t grid[3];
  int32_t segments;         /* I / J passes: pieces a line is cut into along the axis (0 for K passes) */
  int32_t rows_per_segment; /* I / J passes: output rows of every piece but the last, which holds the rest */
  int32_t k_tiles;          /* blocks along K */
  int32_t lds_bytes;        /* dynamic LDS of the launch */
  int32_t last;             /* the pass stores into y (in the dtype of the call) */
} tio_conv_pass;

int tio_separable_conv3d_passes(int32_t dtype, int32_t batch, int32_t channels, const int32_t shape[3],
                                const int32_t radius[3], int32_t aligned16, int32_t has_skip,
                                int32_t bias_on, int32_t noise_on, int32_t fast_math,
                                tio_conv_pass out_passes[3]);

/*
 * Backward of tio_separable_conv3d with respect to x (ABI 16): gx = A_I^T A_J^T A_K^T gy, where A_a is the
 * replicate-padded correlation along axis a — the transpose of a CLAMPED stencil folds the taps that were
 * clamped onto a border voxel back onto it.  What autograd computes through the reference's
 * F.pad(mode="replicate") + grouped conv3d per axis (blur.py:157-252), one gather kernel per active axis.
 *   gy, gx: (B, C, I, J, K) float32 (the reference computes the blur, hence its backward, in float32:
 *           blur.py:173); taps_dev / taps_batched / tap_stride / radius / skip_dev as in the forward call;
 *           rows with skip_dev[b] != 0 pass their gradient through (the forward copied them);
 *   tmp:    scratch with the size of gx (may be NULL when at most one axis is active).
 */
int tio_separable_conv3d_adjoint(const float* gy, float* gx, float* tmp, int32_t batch,
                                 int32_t channels, const int32_t shape[3], const float* taps_dev,
                                 int32_t taps_batched, int32_t tap_stride, const int32_t radius[3],
                                 const uint8_t* skip_dev, void* stream);

/*
 * Blur with its neighbours folded in: y = Noise(Blur(BiasField(x))) in the separable passes
 * of tio_separable_conv3d — the bias field multiplies every row on its way into the first
 * (I) pass, the noise is added to every row the last (fused J+K) pass stores, so the two
 * elementwise transforms cost no extra trip through HBM.  Values are bit-identical to
 * tio_bias_field_apply -> tio_separable_conv3d -> tio_add_noise (same float32 operations in
 * the same order; tests compare the two).  Replaces, for a Compose that holds them back to
 * back, bias_field.py:99-132 + blur.py:76-252 + noise.py:98-123.
 *   bias_coarse_dev == NULL: no bias stage;  noise_on == 0: no noise stage (fast-mode
 *   Philox draws only, as tio_add_noise with base1_dev == NULL, not rician);
 *   tmp: scratch of 2 x size(y) floats.
 * Returns TIO_ERR_UNSUPPORTED_CONFIG (and launches nothing) unless: float32, 16-byte
 * aligned, all three radii in 1..16 (K: 1..8), K <= 256 and K % 4 == 0 — the caller then
 * runs the three entry points one after the other.
 */
int tio_blur_fused(const void* x, void* y, void* tmp, int32_t dtype, int32_t batch,
                   int32_t channels, const int32_t shape[3], const float* taps_dev,
                   int32_t taps_batched, int32_t tap_stride, const int32_t radius[3],
                   const float* bias_coarse_dev, const int32_t bias_coarse_shape[3],
                   int32_t noise_on, float noise_mean, float noise_std,
                   const float* noise_mean_dev, const float* noise_std_dev,
                   int32_t noise_batched, uint64_t philox_seed, const float* noise_base_dev,
                   int32_t fast_math, void* stream);
/* noise_on (ABI 12): 0 = no noise stage; 1 = in-kernel Philox draws (philox_seed), as tio_add_noise with base1_dev == NULL;
 * 2 = explicit draws: noise_base_dev holds one float32 normal draw per element, laid out like x (16-byte aligned) — as
 * tio_add_noise with base1_dev.  This is how the REFERENCE's noise stream (noise.py:108-116: one seeded CPU generator,
 * reproduced on the device by tio_mt19937_randn_device) rides on the stencil's stores: the draws are made ahead on another
 * stream, the sum x + (mean + std z) costs no pass of its own.  Same float32 operations as tio_add_noise. */
/* fast_math (ABI 8): 0 = every tap is `acc = acc + w * v` with two roundings, the reference's accumulation (bit-identical
 * to tio_separable_conv3d); 1 = fused multiply-adds in the register-window passes (radii <= 8): one rounding per tap,
 * results within float rounding of the exact ones (~1e-7 relative; the contract for intensities is 1e-4), and a J+K pass
 * that is bound by vector instructions ~25 % shorter.  The counterpart of tio_resample_geom.precision for the stencil. */

/*
 * BiasField: y = x * exp(trilinear_upsample(coarse))   (or x / ... when divide)
 *   bias_field.py:296-341 (_generate_bias_field), :201-255 (_apply_bias_per_element),
 *   :130 / :196 (multiply / divide).  coarse_dev is (B, C, si, sj, sk) float32 —
 *   the seeded CPU-generator draw of bias_field.py:321-330 stays on the host
 *   side of this boundary.  skip_dev: optional B bytes, rows copied bit-exactly
 *   (std == 0 rows, bias_field.py:247-253).
 */
int tio_bias_field_apply(const void* x, void* y, int32_t dtype, int32_t batch,
                         int32_t channels, const int32_t shape[3],
                         const float* coarse_dev, const int32_t coarse_shape[3],
                         int32_t divide, const uint8_t* skip_dev, void* stream);

/*
 * Noise: y = x + (mean + std * z)            (noise.py:98-123, :166-178)
 *        rician: y = sqrt((x + n1)^2 + n2^2), n_i = mean + std * z_i
 *   mean_dev / std_dev: per-element (B floats) when params_batched, else the
 *   scalars mean / std are used.
 *   base1_dev / base2_dev: standard-normal draws shaped like x.  Parity mode: the
 *   caller fills them from the reference's seeded CPU generator (noise.py:177).
 *   Fast mode (base1_dev == NULL): drawn in-kernel from Philox4x32-10 keyed by
 *   (philox_seed, element index) + Box-Muller; base2 uses stream id 1.
 *   keep_dev: optional B bytes; rows with keep == 0 are copied bit-exactly
 *   (noise.py:126-146).
 */
int tio_add_noise(const void* x, void* y, int32_t dtype, int32_t batch,
                  int64_t n_per_element, float mean, float std,
                  const float* mean_dev, const float* std_dev,
                  int32_t params_batched, int32_t rician, const float* base1_dev,
                  const float* base2_dev, uint64_t philox_seed,
                  const uint8_t* keep_dev, void* stream);

/* Fill out_dev[0..n) with the same standard normals the fast noise mode draws
 * (stream_id 0 → base1, 1 → base2). */
int tio_philox_normal(float* out_dev, int64_t n, uint64_t philox_seed,
                      int32_t stream_id, void* stream);

/*
 * Gamma: y = sign(x) * |x| ^ gamma            (gamma.py:80-91, :133-142)
 *   gamma_dev: per-element exponents (B floats) when params_batched, else the
 *   scalar gamma (= exp(log_gamma), gamma.py:103-120).
 */
int tio_gamma_pow(const void* x, void* y, int32_t dtype, int32_t batch,
                  int64_t n_per_element, float gamma, const float* gamma_dev,
                  int32_t params_batched, void* stream);

/*
 * The gradients of the four intensity operations above with respect to their PARAMETERS (additive to ABI 18, HIP only): what
 * autograd derives through the reference's compositions of torch operations (bias_field.py:237-244, blur.py:157-252,
 * x + (mean + std z), sign(x) |x|^gamma) at the cost of a full-size field and a full-size gradient of it per parameter.  Each is
 * one reduction of the volume into a handful of numbers: one read of x and of the incoming gradient, no per-voxel intermediate.
 * Common to the four:
 *   gy         float32, shaped like the forward's output: dL/d(output); x has `element_type`, a tio_dtype code: one of the four
 *              float types (any other code: TIO_ERR_UNSUPPORTED_DTYPE);
 *   terms      formed in float32 from the forward's own float32 values (y before its store rounds it, the same lerp weights, the
 *              same expf / powf; float64 data: the forward's float64 expressions for gamma and noise, narrowed once for bias and
 *              taps), summed in float64 from the lane up, float64 hardware atomics across blocks, ONE rounding to float32:
 *              two runs differ at most in the last float32 rounding of an output;
 *   workspace  *_workspace_bytes(...) bytes on the device, 8-byte aligned; its contents on entry do not matter;
 *   outputs    float32, fully overwritten; flagged rows (skip_dev set, keep_dev == 0) add exactly zero; parameters shared across
 *              the batch receive the sum over the batch;
 *   errors     bad arguments return TIO_ERR_INVALID_ARGUMENT with nothing launched.
 *
 * tio_bias_field_grad: arguments as tio_bias_field_apply.  d_coarse (B, C, si, sj, sk):
 *   d_coarse[b,c,n] = s * sum_v gy[b,c,v] * y[b,c,v] * W(n; v),  s = +1 (multiply) / -1 (divide), W the product of the three
 *   align-corners lerp weights of the forward.
 * tio_gamma_grad: arguments as tio_gamma_pow (and: a non-NULL gamma_dev without params_batched holds the one shared exponent, so a
 *   device scalar needs no host round trip; likewise mean_dev / std_dev below).  d_gamma (B floats when params_batched, else 1):
 *   d_gamma[b] = sum_{v: x != 0} gy * y * log|x|   (x == 0 adds nothing: ATen's rule for pow with respect to the exponent).
 * tio_noise_grad: arguments as tio_add_noise.  d_mean, d_std (B floats when params_batched, else 1); either may be NULL, not both.
 *   additive: d_mean[b] = sum gy, d_std[b] = sum gy * z (x may be NULL);
 *   rician, a = x + n1, n_i = mean + std z_i:  d_mean = sum gy (a + n2) / y,  d_std = sum gy (a z1 + n2 z2) / y;  y == 0 adds nothing;
 *   base1_dev == NULL: z is regenerated in the kernel, bit for bit the draws of tio_philox_normal (stream ids 0 and 1).
 * tio_separable_conv3d_taps_grad: arguments as tio_separable_conv3d_adjoint, plus x with its element type.  d_taps in the layout of
 *   taps_dev ((B | 1, 3, tap_stride); zero beyond 2 * radius[a] + 1 and on axes with radius 0).  With y = A_K A_J A_I x:
 *   dW_I[t] = sum_v (A_J^T A_K^T gy)[v] x[clamp(v + (t - r) e_I)],  dW_J[t] = sum_v (A_K^T gy)[v] (A_I x)[clamp(v + (t - r) e_J)],
 *   dW_K[t] = sum_v gy[v] (A_J A_I x)[clamp(v + (t - r) e_K)];  the intermediates are single-axis launches of
 *   tio_separable_conv3d / tio_separable_conv3d_adjoint into `scratch` (2 x the volume, in floats).  Radii up to 16.
 */
int64_t tio_bias_field_grad_workspace_bytes(int32_t batch, int32_t channels, const int32_t coarse_shape[3]);
int tio_bias_field_grad(const void* x, const float* gy, int32_t element_type, int32_t batch, int32_t channels, const int32_t shape[3],
                        const float* coarse_dev, const int32_t coarse_shape[3], int32_t divide, const uint8_t* skip_dev,
                        float* d_coarse, void* workspace, int64_t workspace_bytes, void* stream);
int64_t tio_gamma_grad_workspace_bytes(int32_t batch, int32_t params_batched);
int tio_gamma_grad(const void* x, const float* gy, int32_t element_type, int32_t batch, int64_t n_per_element, float gamma,
                   const float* gamma_dev, int32_t params_batched, float* d_gamma, void* workspace, int64_t workspace_bytes,
                   void* stream);
int64_t tio_noise_grad_workspace_bytes(int32_t batch, int32_t params_batched);
int tio_noise_grad(const void* x, const float* gy, int32_t element_type, int32_t batch, int64_t n_per_element, float mean, float std,
                   const float* mean_dev, const float* std_dev, int32_t params_batched, int32_t rician, const float* base1_dev,
                   const float* base2_dev, uint64_t philox_seed, const uint8_t* keep_dev, float* d_mean, float* d_std,
                   void* workspace, int64_t workspace_bytes, void* stream);
int64_t tio_separable_conv3d_taps_grad_workspace_bytes(int32_t batch, int32_t taps_batched);
int tio_separable_conv3d_taps_grad(const void* x, int32_t element_type, const float* gy, float* scratch, int32_t batch, int32_t channels,
                                   const int32_t shape[3], const float* taps_dev, int32_t taps_batched, int32_t tap_stride,
                                   const int32_t radius[3], const uint8_t* skip_dev, float* d_taps, void* workspace,
                                   int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------ */
/* F.interpolate users: Resize, Anisotropy                */
/* ------------------------------------------------------------------------ */

/*
 * B-spline coefficients of a (B * C) stack of volumes for tio_resample3d's TIO_QUADRATIC / TIO_CUBIC images: the
 * recursive prefilter of order `order` (2: pole sqrt(8) - 3, 3: pole sqrt(3) - 2; 4 and 5: two poles, 6 and 7: three — the roots
 * inside the unit circle of the order's B-spline polynomial) along I, J, K, one pole after the other, with the
 * half-sample-symmetric ("dct2") boundary — what grid_pull(prefilter=True, bound="dct2") applies before sampling
 * (spatial.py:1753-1760).  x has `dtype`, y is float32 of the same shape.
 */
int tio_bspline_prefilter(const void* x, float* y, int32_t dtype, int64_t n_batch_channels, const int32_t shape[3],
                          int32_t order, void* stream);

/*
 * F.interpolate(x.float(), size=out_shape, mode=...).to(x.dtype) on a dense
 * (N, I, J, K) stack of volumes (N = B * C):
 *   mode TIO_NEAREST: the legacy "nearest" — src = min(floor(dst * float(in) / float(out)), in - 1)
 *                     (resize.py:70-76, anisotropy.py:380-384), an element move for every dtype;
 *   mode TIO_LINEAR:  "trilinear" with align_corners=True (resize.py:70-76,
 *                     anisotropy.py:386-391): ATen's source index / lambda per axis and the
 *                     K-, J-, I-nested fma(t0, w0, t1 * w1), computed in float32.
 */
int tio_interpolate3d(const void* x, void* y, int32_t dtype, int64_t n_batch_channels,
                      const int32_t in_shape[3], const int32_t out_shape[3], int32_t mode, void* stream);

/*
 * Anisotropy with per-element parameters (_simulate_anisotropy_fixed_axis,
 * anisotropy.py:180-208): along `axis`, y[b, c, .., p, ..] = x[.., lower[b, p], ..] (upper_dev
 * NULL: nearest) or x[.., lower[b, p], ..] * (1 - w[b, p]) + x[.., upper[b, p], ..] * w[b, p] with
 * every product and the sum rounded separately like the reference's three tensor ops.  The
 * (B, length) index / weight tables are the reference's own integer arithmetic, done on the
 * host.  active_dev (B bytes or NULL): 0 = the element is copied unchanged (factor <= 1).
 */
int tio_axis_gather_lerp(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels,
                         const int32_t shape[3], int32_t axis, const int32_t* lower_dev,
                         const int32_t* upper_dev, const float* weight_dev, const uint8_t* active_dev,
                         void* stream);

/*
 * Flip (transforms/spatial/flip.py:182-236): y = torch.flip(x, axes) as one element move.
 * axes_mask: bit a = flip spatial axis a for every element; flags_dev (B x 3 bytes, or NULL)
 * overrides it per element (_flip_per_element: a flip + torch.where per axis in the reference).
 */
int tio_flip3d(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels,
               const int32_t shape[3], int32_t axes_mask, const uint8_t* flags_dev, void* stream);

/*
 * Reorient (transforms/spatial/reorient.py:63-91 _apply_reorientation: up to three torch.flip
 * passes, then permute(...).contiguous()) and Transpose (transforms/spatial/transpose.py:44:
 * permute(0, 1, 4, 3, 2).contiguous()) as one element move.  Additive to ABI 18, HIP only.
 *   y is (B, C, in_shape[perm[0]], in_shape[perm[1]], in_shape[perm[2]]);
 *   y[b, c, o0, o1, o2] = x[b, c, i0, i1, i2] with i[perm[d]] = o_d, or in_shape[perm[d]] - 1 - o_d
 *   when bit perm[d] of flip_mask is set: nibabel's apply_orientation order (flip the input axes,
 *   then transpose by perm = argsort(ornt[:, 0])).
 * Every dtype (dispatch on the element size).  perm[2] == 2 keeps rows along K (a grid-stride
 * move); any other perm goes through a 64 x 64 LDS tile so that reads and writes are both
 * coalesced.  x and y must not overlap.
 */
int tio_permute3d(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels,
                  const int32_t in_shape[3], const int32_t perm[3], int32_t flip_mask, void* stream);

typedef enum tio_pad_mode {
  TIO_PAD_CONSTANT = 0,  /* F.pad(mode="constant", value=fill); also the statistic modes (per-element constants) */
  TIO_PAD_REFLECT = 1,   /* F.pad(mode="reflect"): mirror without repeating the edge                              */
  TIO_PAD_REPLICATE = 2, /* F.pad(mode="replicate"): clamp                                                        */
  TIO_PAD_CIRCULAR = 3   /* F.pad(mode="circular"): wrap                                                          */
} tio_pad_mode;

/*
 * pad_tensor (transforms/spatial/_padding.py:62-104; Pad, pad.py:88-108; GridSampler's border
 * padding, data/sampler.py:127-147): y = F.pad(x, (k0, k1, j0, j1, i0, i1), mode, value) as one
 * element move.  padding = (i0, i1, j0, j1, k0, k1).  The 'mean' / 'median' / 'minimum' modes of
 * the reference are constant padding with one value per batch element: fill_per_element_dev
 * (B values of the image dtype) overrides `fill` then.
 */
int tio_pad3d(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels,
              const int32_t in_shape[3], const int32_t padding[6], int32_t mode, double fill,
              const void* fill_per_element_dev, void* stream);

/*
 * The transposes of three of the data movers above (additive to ABI 18, HIP only): what autograd derives for the image
 * through the reference's F.interpolate / gather / F.pad calls.  Gradients are float32 in and out.  Each is a GATHER:
 * one thread per element of gx, every element of gx written exactly once (no atomics, the caller need not zero it), the
 * additions of an element in a fixed order - two calls give the same bits.  gx must not alias gy.
 *
 * tio_interpolate3d_adjoint: gy (N, out_shape) -> gx (N, in_shape), the transpose of tio_interpolate3d for TIO_LINEAR
 *   (trilinear, align_corners=True: resize.py:70-76, anisotropy.py:386-391) and TIO_NEAREST (the legacy "nearest":
 *   resize.py:70-76, anisotropy.py:380-384).  Per axis the outputs that read an input index form one contiguous range; its
 *   ends and the weights come from the forward's own float32 index expressions, the product of the three weights is
 *   rounded in the forward's order (K, J, I).  An input no output reads (down-sampling) receives 0.  No axis longer than
 *   2^21 voxels on either side (the closed-form range ends are proven up to there): TIO_ERR_INVALID_ARGUMENT beyond.
 *
 * tio_axis_gather_lerp_adjoint: the transpose of tio_axis_gather_lerp (_simulate_anisotropy_fixed_axis,
 *   anisotropy.py:180-208).  The caller inverts the (B, length) tables into per-element lists:
 *     offsets_dev    int32 (B, length + 1): entries [offsets[b, p], offsets[b, p + 1]) of element b read source index p
 *     positions_dev  int32 (B, entries): the output position along the axis of each entry
 *     weights_dev    float32 (B, entries): its weight (1 - w for a `lower` entry, w for an `upper` one, each as the
 *                    forward forms it), or NULL: every weight is 1 (nearest)
 *   gx[b, c, .., p, ..] = sum over p's entries of gy[.., position, ..] * weight, in list order.  Offsets and positions
 *   are clamped to the element's list and line.  active_dev (B bytes or NULL): 0 = gx is a copy of gy for that element.
 *
 * tio_pad3d_adjoint: gy (B, C, in_shape + padding) -> gx (B, C, in_shape), the transpose of tio_pad3d
 *   (_padding.py:62-104) for TIO_PAD_REFLECT / TIO_PAD_REPLICATE / TIO_PAD_CIRCULAR under tio_pad3d's own limits: along
 *   an axis an index receives its own position plus at most one border position per side (reflect, circular) or the whole
 *   border run (replicate, first and last index); the three axes' position sets multiply.  TIO_PAD_CONSTANT: refused
 *   (its transpose is a crop).
 */
int tio_interpolate3d_adjoint(const float* gy, float* gx, int64_t n_batch_channels, const int32_t in_shape[3],
                              const int32_t out_shape[3], int32_t mode, void* stream);
int tio_axis_gather_lerp_adjoint(const float* gy, float* gx, int32_t batch, int32_t channels, const int32_t shape[3],
                                 int32_t axis, const int32_t* offsets_dev, const int32_t* positions_dev,
                                 const float* weights_dev, int32_t entries, const uint8_t* active_dev, void* stream);
int tio_pad3d_adjoint(const float* gy, float* gx, int32_t batch, int32_t channels, const int32_t in_shape[3],
                      const int32_t padding[6], int32_t mode, void* stream);

/* ------------------------------------------------------------------------ */
/* Feeding side: dense-inference patch aggregation        */
/* ------------------------------------------------------------------------ */

typedef enum tio_overlap_mode {
  TIO_OVERLAP_CROP = 0,    /* out[dst] = patch[src]          (aggregator.py:166-204) */
  TIO_OVERLAP_AVERAGE = 1, /* out += patch; weights += 1     (aggregator.py:206-214) */
  TIO_OVERLAP_HANN = 2     /* out += patch * w; weights += w (aggregator.py:216-232) */
} tio_overlap_mode;

#define TIO_MAX_PATCHES 32 /* placements per call */

/* Where one patch lands: voxels [src_ini, src_ini + extent) of the patch go to
 * [dst_ini, dst_ini + extent) of the volume (PatchLocation.to_slices(), or the trimmed
 * centre that 'crop' keeps).  HOST memory, copied into the launch. */
typedef struct tio_patch_placement {
  int32_t dst_ini[3];
  int32_t src_ini[3];
  int32_t extent[3];
} tio_patch_placement;

/*
 * PatchAggregator.add_batch without the D2H copy (aggregator.py:94-99 forces
 * tensor.cpu() and accumulates with one Python slice assignment per patch).
 *   out        (C, I, J, K) device accumulator, same dtype as the patches
 *   weight_sum (C, I, J, K) device, same dtype; NULL for TIO_OVERLAP_CROP
 *   patches    (n_patches, C, pi, pj, pk) device
 *   window_*   HANN only: the three 1-D windows torch.hann_window(size + 2,
 *              periodic=False)[1:-1] as float32 (device); the 3-D weight of a voxel
 *              is (wi * wj) * wk in float32, the rounding of _build_hann_3d
 *              (aggregator.py:237-245).
 * Every volume voxel applies the patches that cover it IN PATCH ORDER, so overlaps
 * accumulate in the reference's order (float addition does not commute) and 'crop'
 * keeps the last writer.  Arithmetic: float64 for TIO_F64, otherwise float32 rounded to
 * the storage dtype after every patch - what the in-place `+=` on a half tensor does.
 * CROP copies elements and takes every dtype; AVERAGE / HANN need a floating dtype.
 */
int tio_patch_accumulate(void* out, void* weight_sum, int32_t dtype, int32_t channels,
                         const int32_t vol_shape[3], const void* patches, int32_t n_patches,
                         const int32_t patch_shape[3], const tio_patch_placement* placements_host,
                         int32_t mode, const float* window_i_dev, const float* window_j_dev,
                         const float* window_k_dev, void* stream);

/*
 * torch.unique(data) of an 8- or 16-bit integer label map: the sorted value set that sizes the
 * one-hot encoding of the partial-volume label mode (spatial.py:1360; it becomes labels_dev /
 * n_labels of a TIO_LABEL_PV image).  A presence bitmap instead of torch.unique's sort.
 *   x             device, n elements of dtype TIO_U8 / TIO_I8 / TIO_I16, 16-byte aligned
 *   table_dev     device, room for 65536 doubles (256 for the 8-bit types): the values, ascending
 *   count_dev     device, one int32: how many
 *   workspace_dev device, 8 KiB scratch (the bitmap; cleared by the call)
 * Other dtypes: TIO_ERR_UNSUPPORTED_DTYPE, nothing launched (callers keep torch.unique).
 */
int tio_unique_labels(const void* x, int32_t dtype, int64_t n, double* table_dev, int32_t* count_dev,
                      void* workspace_dev, void* stream);

/* ------------------------------------------------------------------------ */
/* Label-map transforms (ABI 17)                                             */
/* ------------------------------------------------------------------------ */

typedef enum tio_remap_mode {
  TIO_REMAP_KEEP = 0,    /* a value that is no key stays                      (remap_labels.py:54, remove_labels.py:57) */
  TIO_REMAP_CONSTANT = 1 /* a value that is no key becomes `constant`         (sequential_labels.py:58: zeros_like)     */
} tio_remap_mode;
#define TIO_REMAP_MAX_PAIRS 65536

/*
 * RemapLabels / RemoveLabels / SequentialLabels and its inverse (remap_labels.py:54-57, remove_labels.py:57-60,
 * sequential_labels.py:58-61, :100-104: one full-volume `data == old` plus a masked write PER PAIR) as one pass for any
 * number of pairs: y[v] = values[j] where double(x[v]) == keys[j], else x[v] (KEEP) or `constant` (CONSTANT), both cast
 * to the dtype.  Every comparison is against the ORIGINAL value, so {1: 2, 2: 1} swaps, as in the reference.
 *   x, y        n elements of any tio_dtype; y == x (in place) is allowed
 *   keys_dev    device, n_pairs <= TIO_REMAP_MAX_PAIRS doubles, strictly ASCENDING (unique)
 *   values_dev  device, n_pairs doubles
 *   table_dev   device scratch of 65536 int16 (128 KiB), TIO_I16 only (NULL otherwise): the dense table a one-block launch
 *               fills in front of the streaming one.  8-bit data: a 256-entry table in LDS; every other dtype: a binary
 *               search in the keys (from LDS up to 2048 pairs).
 */
int tio_label_remap(const void* x, void* y, int32_t dtype, int64_t n, const double* keys_dev,
                    const double* values_dev, int32_t n_pairs, int32_t mode, double constant,
                    void* table_dev, void* stream);

/*
 * OneHot (one_hot.py:64-68: .long(), F.one_hot, permute, .float()): x is (B, 1, n_spatial) of any tio_dtype, y is
 * (B, num_classes, n_spatial) float32 with y[b, c, v] = (x[b, 0, v] == c).  The input is read once.
 *   status_dev  device, one int32, cleared by the call: non-zero afterwards when some value was negative, >= num_classes
 *               or no integer (F.one_hot raises there; such a voxel is 0 in every class here and the caller raises).
 */
int tio_label_one_hot(const void* x, float* y, int32_t dtype, int32_t batch, int64_t n_spatial,
                      int32_t num_classes, int32_t* status_dev, void* stream);

/*
 * Contour (contour.py:66-70: F.pad(value=-1), -max_pool3d(-padded, 3), `eroded != data.float()`): for every one of the
 * n_batch_channels volumes, y = (min over the 3 x 3 x 3 neighbourhood of float32(x), -1 outside the volume) != float32(x)
 * as float32 0 / 1.  What the code computes, not its docstring: the 26-neighbourhood, a voxel is marked where a neighbour
 * is SMALLER, and every voxel on a face of the volume is marked unless its value is <= -1.
 */
int tio_label_contour(const void* x, float* y, int32_t dtype, int64_t n_batch_channels,
                      const int32_t shape[3], void* stream);

#define TIO_KEEP_LARGEST_MAX_LABELS 1024 /* labels per call (the caller splits a longer list) */

/*
 * KeepLargestComponent (keep_largest.py:108-125: per label and batch element a mask copied to the HOST, SimpleITK's
 * ConnectedComponent + RelabelComponent, a masked write).  x, y: (B, 1, I, J, K) of TIO_U8 / I8 / I16 / I32 / I64 / F32
 * (others: TIO_ERR_UNSUPPORTED_DTYPE), y must not alias x.  y = x, except that a voxel whose value is listed and whose
 * connected component — of voxels of that same value, inside its batch element, 26-connected when fully_connected else
 * 6-connected — is not the largest such component of that value in that element becomes `background`.  All listed labels
 * are handled in one pass.  Of equally large components the one whose first voxel comes first in C order is kept.
 *   labels_dev     device, n_labels <= TIO_KEEP_LARGEST_MAX_LABELS doubles, strictly ascending
 *                  (more: TIO_ERR_UNSUPPORTED_CONFIG)
 *   workspace_dev  device, 16-byte aligned, workspace_bytes >= the size the helper below returns for these arguments
 * B * I * J * K >= 2^31: TIO_ERR_UNSUPPORTED_CONFIG (voxel indices are int32).
 */
int64_t tio_keep_largest_workspace_bytes(int32_t batch, const int32_t shape[3], int32_t n_labels);
int tio_keep_largest_component(const void* x, void* y, int32_t dtype, int32_t batch, const int32_t shape[3],
                               const double* labels_dev, int32_t n_labels, double background,
                               int32_t fully_connected, void* workspace_dev, int64_t workspace_bytes,
                               void* stream);

/*
 * LabelsToImage (labels_to_image.py:182-218 _generate_per_element, :263-290 _generate_from_labels: PER LABEL a full-volume
 * randn_like, a multiply, an add, a `==` mask, a cast, another multiply and an accumulate) as one pass: the masks
 * `label == v` are disjoint, so every voxel gets one Gaussian draw with the mean and the deviation of its own label.
 * Additive to ABI 18; no CPU restatement.
 *   labels       (batch, channels, n_spatial) of any tio_dtype; only channel 0 of each element is read (`label_data[:, 0:1]`)
 *   out          (batch, 1, n_spatial) float32, must not overlap `labels` (nor `base_dev`)
 *   keys_dev     device, n_keys <= TIO_REMAP_MAX_PAIRS doubles, strictly ASCENDING (as tio_label_remap)
 *   mean_dev, std_dev   device, n_keys floats each, or batch * n_keys (element-major) when params_batched
 * A voxel whose value is no key (the reference takes its keys from element 0 alone; a non-integer value of a floating map)
 * is written as +0.0f; so is one whose key has mean and deviation both zero (the reference's `continue`).
 *
 * Fused mode (base_dev == NULL): out[b, v] = fadd(mean[k], fmul(std[k], z)), two separately rounded float32 operations, z
 * the standard normal tio_philox_normal(out, batch * n_spatial, philox_seed, 0) puts at flat index b * n_spatial + v.
 * One-label mode (base_dev != NULL: batch * n_spatial standard normals of the caller): only key index base_key is
 * looked at.  Where the label equals keys[base_key] the call writes fadd(fadd(fmul(base, std), mean), +0.0f) — the
 * reference's `randn * std + mean`, `* mask`, `result +=` onto zeros — and every other voxel keeps what `out` holds: the
 * caller clears `out` once and calls once per label, in the reference's loop order, with the reference's own draws.
 * 8-bit labels: a 256-entry table in LDS; other dtypes: a binary search in the keys, from LDS up to 2048 of them.
 * batch > 65535: TIO_ERR_UNSUPPORTED_CONFIG.  batch == 0 or n_spatial == 0: TIO_OK, nothing done.
 */
int tio_labels_to_image(const void* labels, int32_t dtype, int32_t batch, int32_t channels, int64_t n_spatial,
                        const double* keys_dev, int32_t n_keys, const float* mean_dev, const float* std_dev,
                        int32_t params_batched, float* out, uint64_t philox_seed, const float* base_dev,
                        int32_t base_key, void* stream);

/* ------------------------------------------------------------------------ */
/* Intensity preprocessing with on-device statistics (ABI 17, additive)      */
/* ------------------------------------------------------------------------ */
/*
 * Normalize / Standardize / Clamp / Mask (transforms/intensity/normalize.py, standardize.py, clamp.py, mask.py).  Every
 * entry point reads every tio_dtype and converts an element to float32 first, as the reference's `.float()` does
 * (float64 and int64 are rounded to float32).
 *
 * The two statistics read ONE batch element — `img_batch.data[0]`, (channels, n_spatial) — and an optional mask:
 *   mask           device or NULL (every element counts), (mask_channels, n_spatial) of any tio_dtype (bool: TIO_U8);
 *                  inside = nonzero (`.bool()`); mask_channels is 1 (broadcast over the channels) or `channels`
 *   record_dev     device, 8-byte aligned, written by the call (layouts below)
 *   workspace_dev  device, 16-byte aligned, at least tio_intensity_stats_workspace_bytes() bytes; it may hold anything
 *                  (the kernels zero what they use) and may be reused by the next call on the same stream
 */
int64_t tio_intensity_stats_workspace_bytes(void);

/*
 * Standardize.make_params (standardize.py:63-76: a boolean gather, `.mean()`, `.std()`, two read-backs): the count, the
 * mean and the unbiased standard deviation (n - 1) of the inside elements.  Accumulated in float64 (shifted sums per
 * thread, Chan's pairwise merge above them), rounded ONCE to float32.  Per-block partials go to fixed slots and are merged
 * in a fixed order, no float atomics: two calls on the same input return the same bits.
 *   record_dev  { int64 count; float32 mean; float32 std; }  — count 0: mean and std NaN; count 1: std NaN (torch.std)
 */
int tio_intensity_moments(const void* x, int32_t dtype, int32_t channels, int64_t n_spatial, const void* mask,
                          int32_t mask_dtype, int32_t mask_channels, void* record_dev, void* workspace_dev,
                          int64_t workspace_bytes, void* stream);

/*
 * compute_quantile (transforms/_statistics.py:36-41: torch.kthvalue once or twice per quantile, each a selection pass
 * with a read-back) for up to two fractions in one call.  With n the number of inside elements and
 * lower = floor(q * (n - 1)) — float64, on the device, the reference's two operations — the record of fraction k holds
 * the (lower + 1)-th and the (lower + 2)-th smallest inside value (the same value when lower == n - 1) and n; the host
 * finishes with the reference's own `lower_value.lerp(upper_value, index - lower)`.  Exact: a radix select over an
 * order-preserving 32-bit key (NaN sorts last, as torch.kthvalue sorts it; of -0 and +0 either may be returned) in three
 * data passes of 11 / 11 / 10 bits, a one-block scan after each; no host round trip in between.
 *   fractions    HOST, n_fractions (1 or 2) doubles in [0, 1]
 *   record_dev   n_fractions x { float32 lower_value; float32 upper_value; int64 n; }  — n == 0: the values are NaN
 */
int tio_intensity_quantiles(const void* x, int32_t dtype, int32_t channels, int64_t n_spatial, const void* mask,
                            int32_t mask_dtype, int32_t mask_channels, const double* fractions,
                            int32_t n_fractions, void* record_dev, void* workspace_dev, int64_t workspace_bytes,
                            void* stream);

typedef enum tio_map_mode {
  TIO_MAP_RESCALE_CLIP = 0, /* (min(max(x, in_min), in_max) - in_min) / in_range * out_range + out_min  (normalize.py:182-183) */
  TIO_MAP_RESCALE = 1,      /* (x - out_min) / out_range * in_range + in_min: the inverse               (normalize.py:287, :297) */
  TIO_MAP_SUB_DIV = 2,      /* (x - in_min) / in_range                                                  (standardize.py:97)     */
  TIO_MAP_MUL_ADD = 3       /* x * in_range + in_min                                                    (standardize.py:138)    */
} tio_map_mode;

/*
 * The elementwise half of Normalize, Standardize and their inverses in one pass: x is (batch, n_per_element) of any
 * tio_dtype, y the same shape in float32.  Every operation is a separately rounded float32 operation — IEEE division, no
 * multiply-add contraction — which is what ATen's CPU kernels compute for `(data - a) / b * c + d` with Python scalars.
 * The clip propagates NaN like torch.clamp.
 *   out_min_dev, out_range_dev  device, `batch` floats each, or both NULL (then the scalars out_min / out_range): the
 *                  per-instance output range of _out_min_and_range (normalize.py:320-327); RESCALE modes only.  With
 *                  them, RESCALE leaves an element whose out_range is 0 as it is (normalize.py:293-298).
 */
int tio_intensity_map(const void* x, float* y, int32_t dtype, int32_t batch, int64_t n_per_element, int32_t mode,
                      float in_min, float in_max, float in_range, float out_min, float out_range,
                      const float* out_min_dev, const float* out_range_dev, void* stream);

/*
 * Clamp (clamp.py:56: `data.clamp(min=, max=)` with Python floats; either bound optional, not both absent): NaN
 * propagates.  y has torch's promoted dtype: the float dtypes stay (the bounds are cast to the dtype; float64 compares in
 * float64), every integer dtype becomes float32.
 */
int tio_intensity_clamp(const void* x, void* y, int32_t dtype, int64_t n, int32_t has_min, double out_min,
                        int32_t has_max, double out_max, void* stream);

/*
 * Mask (mask.py:69-70: `torch.where(mask.expand_as(data), data, outside_value)`): y[i] = x[i] where
 * mask[i % mask_n] is nonzero, else outside_value; mask_n divides n (the mask of the first batch element, broadcast over
 * the batch and, with one mask channel, over the channels).  y has the promoted dtype of tio_intensity_clamp.
 */
int tio_intensity_mask(const void* x, void* y, int32_t dtype, int64_t n, const void* mask, int32_t mask_dtype,
                       int64_t mask_n, double outside_value, void* stream);

/* ------------------------------------------------------------------------ */
/* Swap and HistogramStandardization (ABI 17, additive)                      */
/* ------------------------------------------------------------------------ */
/*
 * Swap (transforms/intensity/swap.py:195-219 _apply_swaps, :222-258 _apply_swaps_per_instance: per swap two patch clones
 * and two assignments, on the per-instance path through advanced-indexing gathers over index tensors).  x and y are
 * (batch, channels, shape) of elements of `element_bytes` (1, 2, 4 or 8; no dtype is interpreted), aligned to the element
 * only; y must not overlap x.  The swaps of a list apply one after the other to every channel; within a swap both patches
 * are read, then A is written, then B — where the two overlap, B's write stays.  One stream-ordered copy and ONE launch
 * whatever the number of swaps: the result is a gather from x (csrc/swap.hip has the rule and the single-writer argument).
 *   patch        1 <= patch[a] <= shape[a]
 *   origins_dev  device int32 [lists][s_max][2][3]: (A, B) origins; the caller keeps them inside [0, shape - patch]
 *                (a box outside the volume is not written, and nothing outside the volume is read)
 *   counts_dev   device int32 [lists]: the swaps of each list (at most s_max)
 *   lists        1 (one list for the whole batch) or `batch`
 *   s_max        0: a plain copy; origins_dev and counts_dev may then be NULL.  There is no upper limit.
 */
int tio_swap_patches(const void* x, void* y, int32_t element_bytes, int32_t batch, int32_t channels, const int32_t shape[3],
                     const int32_t patch[3], const int32_t* origins_dev, const int32_t* counts_dev, int32_t lists,
                     int32_t s_max, void* stream);

/*
 * `np.percentile(values, 100 * q)` for up to 32 fractions and EVERY batch element in one call, without the host
 * (histogram_standardization.py:280 copies each element to the host for it, :105-106 likewise in the training).  x is
 * (batch, channels, n_spatial); an element's values are its inside elements as float32, all channels together.  The mask
 * is that of the statistics above — (mask_channels, n_spatial), shared by the batch elements.  A radix select over the key of
 * tio_intensity_quantiles in four data passes of 11 / 7 / 7 / 7 bits — pass 1 one histogram per element for all ranks, the
 * later passes one 128-bin histogram in LDS per group of ranks that share a prefix — with a one-block scan per element after
 * each; finished on the device by numpy's rule: virtual = (100 q) / 100 * (n - 1), lower = floor(virtual), g = virtual - lower, d = upper_value -
 * lower_value rounded to float32 (numpy subtracts in the array's dtype), then in float64 lower_value + d * g for g < 0.5,
 * else upper_value - d * (1 - g).  A NaN among an element's values makes all its results NaN; so does n == 0.
 *   fractions      HOST, n_fractions (1 .. 32) doubles in [0, 1]
 *   values_dev     device float64 [batch][n_fractions], written
 *   counts_dev     device int64 [batch], written: the inside elements of each batch element
 *   workspace_dev  device, 16-byte aligned, tio_intensity_multi_quantiles_workspace_bytes(batch, n_fractions) bytes (0 for
 *                  arguments the call refuses); it may hold anything
 */
int64_t tio_intensity_multi_quantiles_workspace_bytes(int32_t batch, int32_t n_fractions);
int tio_intensity_multi_quantiles(const void* x, int32_t dtype, int32_t batch, int32_t channels, int64_t n_spatial,
                                  const void* mask, int32_t mask_dtype, int32_t mask_channels, const double* fractions,
                                  int32_t n_fractions, double* values_dev, int64_t* counts_dev, void* workspace_dev,
                                  int64_t workspace_bytes, void* stream);

/*
 * _apply_histogram_standardization (histogram_standardization.py:276-303) for every batch element, given its percentiles
 * on the device: a one-block kernel builds each element's table, one pass applies it.  Every step is a separately rounded
 * float32 operation in the reference's order: the percentiles rounded to float32, `diff` of both, |diff_input| < 1e-5 ->
 * inf, slopes by IEEE division, intercept = landmark - slope * input_landmark, bin = the number of inner edges < x
 * (torch.bucketize, right=False), y = slope[bin] * x + intercept[bin] (a product, then a sum).  x of any tio_dtype is
 * converted to float32 first; y has x's dtype (the reference assigns the float32 result into the image's tensor): integer
 * dtypes by a C cast, truncating toward zero — a result outside the dtype's range is undefined, as it is in the reference.
 *   percentiles_dev  device float64 [batch][n_landmarks] (tio_intensity_multi_quantiles' values_dev)
 *   landmarks_dev    device float32 [n_landmarks], 2 <= n_landmarks <= 32
 *   table_dev        device float32 [batch][3][32], workspace
 */
int tio_histogram_standardize(const void* x, void* y, int32_t dtype, int32_t batch, int64_t n_per_element,
                              const double* percentiles_dev, const float* landmarks_dev, int32_t n_landmarks,
                              float* table_dev, void* stream);

/* ------------------------------------------------------------------------ */
/* Ghosting and Spike (ABI 17, additive): csrc/kspace_artefacts.hip          */
/* ------------------------------------------------------------------------ */
/*
 * Both entries below that take `tables_dev` read the SAME table: device float32 [I + J + K][2], for each spatial axis in
 * turn (cos, sin)(2 pi r / S), r = 0 .. S-1, S the axis' length — evaluated in double and rounded once to float32 by the
 * caller, 8-byte aligned.  Arithmetic is float32; x of any tio_dtype is converted on load, y has x's dtype (the reference's
 * `.float()` / `.to(dtype)`: integers truncate toward zero) and must not overlap x.  Data is aligned to its element only.
 * Every axis has at most 32768 voxels, a volume fewer than 2^31, batch * channels at most 65535 (more:
 * TIO_ERR_UNSUPPORTED_CONFIG).  `active_dev`: device uint8 [batch] or NULL (all active).  An inactive element, one with
 * an empty list, or one with zero strength / intensity comes out as an exact copy of its input, bit for bit.
 */

/*
 * Ghosting (transforms/intensity/ghosting.py:218-277 _add_ghosting, :149-215 _add_ghosting_per_element: fftn, fftshift, a
 * mask along one axis, ifftshift, ifftn, real part).  For every line along the element's axis (length S)
 *     out[i] = x[i] - (strength / S) * sum_{f in Z} ( cos(2 pi f i / S) A_f + sin(2 pi f i / S) B_f ),
 *     A_f = sum_i' cos(2 pi f i' / S) x[i'],   B_f = sum_i' sin(2 pi f i' / S) x[i']
 * with Z the UNSHIFTED frequencies of the scaled planes (shifted index u -> (u - S/2) mod S, S/2 rounded down); a
 * frequency listed twice counts twice.  One launch per axis in `axes_mask`; no transposed copy for any axis.
 *   axes_mask     bit a set: some element's axis is a.  An element whose axis has no bit is NOT WRITTEN.
 *   params_dev    device int32 [params_words]: per batch element {axis, count, offset, strength as float32 bits}, then
 *                 the frequencies; `offset` is the word index of the element's first frequency.  A list that leaves
 *                 [4 * batch, params_words) makes its element a copy; a frequency outside [0, S) contributes nothing.
 *   max_count     no element uses more than this many frequencies (longer lists are cut); decides the LDS layout
 * An axis longer than LDS holds an accumulator line for (about 9600 voxels): TIO_ERR_UNSUPPORTED_CONFIG.
 */
int tio_kspace_ghost_lines(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels, const int32_t shape[3],
                           int32_t axes_mask, const int32_t* params_dev, int32_t params_words, int32_t max_count,
                           const float* tables_dev, const uint8_t* active_dev, void* stream);

/*
 * `spectrum.abs().amax(dim=(-3, -2, -1))` (transforms/intensity/spike.py:152, :201) of a spectrum the caller computed: z is
 * (rows, n) interleaved complex64 on the device, 8-byte aligned; out_dev receives `rows` float32 maxima of |z| (0 for
 * n == 0).  The call clears and writes out_dev itself, the caller prepares nothing; every element is read once.
 * |z| = sqrt(re^2 + im^2) in float32, within 2 ulp of hypot.  CONTRACT: finite input with |re|, |im| < 1.8e19 (the squares
 * must not overflow; a NaN is ignored, not propagated).  rows <= 65535.
 */
int tio_complex_abs_max(const void* z, int64_t rows, int64_t n, float* out_dev, void* stream);

/*
 * Spike (transforms/intensity/spike.py:124-162 _add_spikes, :165-223 _add_spikes_per_instance: fftn, fftshift, peak * intensity
 * added at a few points, ifftshift, ifftn, real part):
 *     out[i, j, k] = x[i, j, k] + (peak * intensity / (I J K)) * sum_p cos 2 pi (f_p0 i / I + f_p1 j / J + f_p2 k / K)
 * with (f_p0, f_p1, f_p2) the UNSHIFTED frequencies of point p; a point listed twice counts twice.  One pass, 16-byte
 * accesses where x and y share their phase inside 16 bytes, single elements otherwise.
 *   params_dev    device int32 [params_words]: per batch element {count, offset, intensity as float32 bits, 0}, then the
 *                 triples; `offset` is the word index of the element's first triple.  Checked like the ghost lists.
 *   peaks_dev     device float32 [batch * channels] (tio_complex_abs_max); read on the device only
 */
int tio_kspace_add_spikes(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels, const int32_t shape[3],
                          const int32_t* params_dev, int32_t params_words, int32_t max_count, const float* tables_dev,
                          const float* peaks_dev, const uint8_t* active_dev, void* stream);

/* ------------------------------------------------------------------------ */
/* Motion: k-space compositing                                               */
/* ------------------------------------------------------------------------ */
#define TIO_MAX_SEGMENTS 32

/*
 * _apply_motion_segments (transforms/intensity/motion.py:334-372).  The reference takes
 * spectrum = fftn(x_0), overwrites the planes [bounds[s], bounds[s+1]) along the FIRST
 * spatial axis with the same planes of fftn(x_s) for every motion segment s >= 1 (x_s: the
 * rigidly moved image, tio_resample3d with the matrix of _apply_rigid_transform,
 * motion.py:393-425) and returns ifftn(spectrum).real.  Only the first axis is masked, so
 * the transforms along J and K cancel and the composite is the real linear map
 *
 *     out[b, c, i, j, k] = sum_s sum_i' W[s][i'][i] * x_s[b, c, i', j, k]
 *     W[s][i'][i] = (1 / I) * sum_{f = bounds[s]}^{bounds[s+1] - 1} cos(2 pi f (i - i') / I)
 *
 * which tio_kspace_segment_mix evaluates as one float32 GEMM per (b, c) on the matrix cores
 * (v_mfma_f32_32x32x2_f32: exact float32 products and sums, no FFT, no complex volumes).
 *   segments    host array of n_segments DEVICE pointers, each a float32 (B, C, I, J, K)
 *               tensor: segments[0] = data.float(), segments[s] = moved image s
 *   bounds      host, n_segments + 1 plane indices, bounds[0] = 0, bounds[n_segments] = I
 *               (_segment_bounds, motion.py:375-390)
 *   mix_dev     device, float32 (n_segments, I, I): the table W above; fill a host buffer
 *               with tio_kspace_mix_table (float64 arithmetic) and upload it once per shape
 *   out         device (B, C, I, J, K) of `dtype` (`.to(data.dtype)`); must not alias a segment
 *   active_dev  device, B bytes or NULL: elements with 0 are skipped, their `out` rows are NOT
 *               written (the caller restores them from the input, torch.where in the reference)
 * Parity: float rounding only (the reference's complex64 FFTs and this GEMM are two float32
 * evaluations of the same sums): <= 1e-5 of the image's magnitude in the tests.
 */
int tio_kspace_segment_mix(const void* const* segments, int32_t n_segments, const int32_t* bounds,
                           const float* mix_dev, void* out, int32_t dtype, int32_t batch,
                           int32_t channels, const int32_t shape[3], const uint8_t* active_dev,
                           void* stream);
/* Host helper: fills table_host (n_segments * length * length floats) with W. */
int tio_kspace_mix_table(int32_t length, int32_t n_segments, const int32_t* bounds, float* table_host);

/* ------------------------------------------------------------------------ */
/* Host helper: torch's CPU `randn` stream on all host cores (ABI 8)         */
/* ------------------------------------------------------------------------ */
/*
 * Replaces: `torch.randn(data.shape, generator=cpu_gen)` of the reference's Noise (transforms/intensity/noise.py:108-116,
 * 166-178: ONE CPU generator seeded with params["seed"], shared by the images of the batch in dict order, one or — Rician —
 * two draws per image).  torch draws on a single thread: 0.35 s for the bench batch.  Here the mt19937 state chain runs on
 * one thread with integer vectors and every other step (tempering, the 24-bit uniform, the Box-Muller step of
 * normal_fill_16_AVX2 with avx_mathfun's log / sincos) on `n_threads - 1` more, in place in `out`.  BIT-IDENTICAL to
 * torch 2.10's CPU kernel for float32 and n >= 16 (pinned against torch.randn: tests/test_host_rng.py); n < 16 returns
 * TIO_ERR_UNSUPPORTED_CONFIG (torch takes another path there: the caller keeps using torch.randn).  Host pointers only, no
 * device work, no stream.  The state persists across calls, like the generator it stands for: a second call continues
 * the stream where the first one stopped (including the 16 extra draws torch spends when n is not a multiple of 16).
 */
#define TIO_HOST_MT_STATE_BYTES 2688
typedef struct tio_host_mt_state { uint64_t opaque[TIO_HOST_MT_STATE_BYTES / 8]; } tio_host_mt_state;
/* `torch.Generator().manual_seed(seed)` (at::mt19937 keeps the low 32 bits) */
int tio_host_mt19937_seed(tio_host_mt_state* state, uint64_t seed);
/* `torch.randn(n, generator=...)` into out (host memory, ideally pinned); n_threads <= 1: everything on the calling thread */
int tio_host_mt19937_randn(tio_host_mt_state* state, float* out, int64_t n, int32_t n_threads);

/*
 * The same stream with the draws produced ON THE DEVICE (ABI 9): the host keeps the one part that is a chain — the
 * mt19937 state twists — and hands the device a PLAN: a snapshot of the state every 128 blocks (2.5 KB per 79 872 draws:
 * 4 MB for 8 x 256^3) plus the rest of the current block and torch's 16 tail draws.  tio_mt19937_randn_device replays the
 * twists from the snapshots (one workgroup per snapshot, the state in LDS) and applies tempering, the 24-bit uniform and
 * normal_fill_16_AVX2's Box-Muller step with avx_mathfun's log / sincos — the float32 operation sequence of the host
 * restatement, every multiply-add fused where torch's build fuses it: BIT-IDENTICAL to torch.randn(n, generator=cpu_gen)
 * (tests/test_gpu_device_rng.py).  No 4-bytes-per-draw upload, no worker threads: 6.5 ms of one host core per 134 M draws.
 *
 *   words = tio_host_mt19937_plan_words(n);                 capacity (uint32 words) a plan of n draws can need
 *   tio_host_mt19937_plan(state, n, plan_host, words, &used, n_threads);   advances `state` exactly like tio_host_mt19937_randn(state, ., n, .)
 *   copy plan_host[0 : used] to plan_dev (the caller's copy, on `stream`)
 *   tio_mt19937_randn_device(plan_host, plan_dev, out_dev, stream);
 *
 * tio_host_mt19937_plan returns TIO_ERR_UNSUPPORTED_CONFIG — and leaves the state untouched — when n < 16 or when the
 * stream stands inside a group of 16 (a previous draw count that was not a multiple of 16 AND did not end a block: torch's
 * groups then straddle state blocks); the caller falls back to tio_host_mt19937_randn.
 * n_threads > 1 cuts long chains into segments: mt19937 is linear over GF(2), so a thread can JUMP to the start of its
 * segment (g(f) applied to the state, g = x^J mod the characteristic polynomial — computed and verified at first use,
 * csrc/host_rng_jump.cpp) and chain from there: 134 M draws are planned in ~1.2 ms on 8 threads (0.55 - 0.65 on 32) instead of 5.5 - 7 ms on one.
 * The snapshot at the start of a jumped segment may differ from the chained one in the 31 low bits of its first word —
 * bits that are not part of the generator's state (the recurrence never reads them).
 */
int64_t tio_host_mt19937_plan_words(int64_t n);
int tio_host_mt19937_plan(tio_host_mt_state* state, int64_t n, uint32_t* plan_host, int64_t capacity_words, int64_t* used_words,
                          int32_t n_threads);
/* The same plan started AHEAD of its launch (ABI 10): _begin hands the call to a native thread and returns a handle (0: bad
 * arguments) at once, _end waits for it and returns what tio_host_mt19937_plan would have (status, *used_words).  The state
 * and the plan buffer belong to the job until _end has returned; one job per state at a time.  For a caller that knows the
 * seed before it is ready to launch (Compose drawing its children's parameters ahead, torchio_amd/transforms/compose.py):
 * the 0.6 - 0.9 ms of the state chain then overlap the caller's enqueue work instead of sitting on its critical path. */
int64_t tio_host_mt19937_plan_begin(tio_host_mt_state* state, int64_t n, uint32_t* plan_host, int64_t capacity_words, int32_t n_threads);
int tio_host_mt19937_plan_end(int64_t handle, int64_t* used_words);
int tio_mt19937_randn_device(const uint32_t* plan_host, const uint32_t* plan_dev, float* out_dev, void* stream);
/* The plan whose snapshots the DEVICE makes (ABI 15).  With several ranks per host the state chain is what the
 * reference-identical noise mode waits for (eight ranks: 4.8 - 5.7 ms per step and rank on the 15 threads each gets, against
 * 1.8 ms of GPU time).  Every snapshot is an independent polynomial evaluation over GF(2) — a jump is the correlation of the
 * polynomial's bits with the generator's own word sequence — so:
 *   tio_host_mt19937_plan_prefix(state, n, plan_host, capacity, &prefix_words, &used_words, &total_blocks)
 *       writes only the PREFIX of the plan — header, the rest of the current block, snapshot 0 (the state the chain starts
 *       from): prefix_words (= 1 280) words to upload of the used_words the plan has on the device — and advances `state` like
 *       tio_host_mt19937_plan does, lazily: the twists are owed and settled (one host-side jump) if the state is read again.
 *       TIO_ERR_UNSUPPORTED_CONFIG (state untouched) where tio_host_mt19937_plan returns it, and when n is not a multiple of 16
 *       (torch's tail rule needs the final state at once) — the caller then makes the whole plan on the host.
 *   tio_host_mt19937_segment_polynomials(segment_blocks, count, out)
 *       the jump polynomials t * segment_blocks twists ahead, t = 1 .. count, 624 words each (bit k of word k / 32 = the
 *       coefficient of x^k) — cached per segment length; upload once per device and length.
 *   tio_mt19937_device_snapshots(plan_dev, total_blocks, segment_blocks, polys_dev, stream)
 *       one workgroup per segment of segment_blocks (a multiple of 128) twists: jumps to its first state, chains through the
 *       segment, writes the snapshots into plan_dev.  The draw kernels above then read plan_dev as if the host had made it. */
int tio_host_mt19937_plan_prefix(tio_host_mt_state* state, int64_t n, uint32_t* plan_host, int64_t capacity_words, int64_t* prefix_words,
                                 int64_t* used_words, int64_t* total_blocks);
int tio_host_mt19937_segment_polynomials(int64_t segment_blocks, int32_t count, uint32_t* out);
int tio_mt19937_device_snapshots(uint32_t* plan_dev, int64_t total_blocks, int64_t segment_blocks, const uint32_t* polys_dev, void* stream);
/* Noise.apply_transform for a float32 image in one kernel: out = x + (mean + std z) with z the plan's draws (the three
 * float32 roundings of noise.py:178, :119, as tio_add_noise) — the draws never exist in memory.  x / out: the image's
 * B * n_per_element values (the plan's n); mean_dev / std_dev: (B,) per-element parameters or NULL (then the scalars).
 * out may be x itself only when n is a multiple of 16 (otherwise TIO_ERR_UNSUPPORTED_CONFIG: torch's tail rule draws the
 * last 16 values a second time, from x). */
int tio_mt19937_add_noise_device(const uint32_t* plan_host, const uint32_t* plan_dev, const float* x_dev, float* out_dev,
                                 int64_t n_per_element, float mean, float std, const float* mean_dev, const float* std_dev,
                                 void* stream);

/* ------------------------------------------------------------------------ */
/* PCA over the channel axis (additive to ABI 18, HIP only)                  */
/* ------------------------------------------------------------------------ */
/*
 * PCA (transforms/intensity/pca.py:83-140 _pca_single).  The reference's first step is `tensor.float()` (pca.py:102), so
 * these entry points take float32 data and nothing else: the caller casts where the reference does.  x is a dense
 * (batch, channels, voxels) tensor at any 4-byte boundary, 1 <= channels <= TIO_PCA_MAX_CHANNELS, voxels >= 1.
 * batch == 0: TIO_OK, nothing done.
 */
#define TIO_PCA_MAX_CHANNELS 1024

/*
 * The centring and the covariance that torch.pca_lowrank derives its basis from (pca.py:105-109: `flat.mean(dim=0)`,
 * `flat - mean`, and the matrix products inside pca_lowrank), exact instead of sketched, in ONE read of x:
 *   mean[b, c]       = sum_v x[b, c, v] / voxels                                   (batch, channels) float64
 *   scatter[b, i, j] = sum_v (x[b, i, v] - mean[b, i]) (x[b, j, v] - mean[b, j])   (batch, channels, channels) float64,
 *                      symmetric bit for bit, both triangles written
 * Accumulated in float64 on the matrix cores around the pivot x[b, c, 0] and corrected for the pivot at the end, so a mean
 * far above the deviation costs nothing.  Per-chunk partials go to fixed slots of the workspace and are added in ascending
 * order, no float atomics: two calls on the same input return the same bits.
 *   workspace_dev  device, 8-byte aligned, at least tio_channel_scatter_workspace_bytes(batch, channels, voxels) bytes;
 *                  it may hold anything and may be reused by the next call on the same stream
 * batch > 65535: TIO_ERR_UNSUPPORTED_CONFIG.
 */
int64_t tio_channel_scatter_workspace_bytes(int32_t batch, int32_t channels, int64_t voxels); /* -1: bad sizes */
/* HOST only, nothing is enqueued: how tio_channel_scatter splits that call.  out = { chunks of voxels, voxels per chunk
 * (a multiple of 16), tile pairs (16 x 16 channels) per block, blocks of the accumulating launch }. */
int tio_channel_scatter_plan(int32_t batch, int32_t channels, int64_t voxels, int32_t out[4]);
int tio_channel_scatter(const float* x, int32_t batch, int32_t channels, int64_t voxels, double* mean, double* scatter,
                        void* workspace_dev, int64_t workspace_bytes, void* stream);

/*
 * The rest of _pca_single in one pass (pca.py:106 `flat - mean`, :111 `centered @ v`, :119 `/ std`, :123 `/ first_std`,
 * :127 `(projected - lo) / (hi - lo)`, :130 `.clamp(0, 1)`), the scalings folded into the weights by the caller:
 *   y[b, k, v] = sum_c weights[b, k, c] (x[b, c, v] - center[b, c]) + offset[b, k],   clamped to [0, 1] when clip != 0
 * center_dev (batch, channels), weights_dev (batch, components, channels), offset_dev (batch, components): float32 on the
 * device; y (batch, components, voxels) float32, 1 <= components <= channels.  The difference is rounded to float32 before
 * the product, as in the reference, one fma per term in ascending channel order.  A NaN stays NaN through the clamp
 * (torch.clamp).  Components are taken 8 at a time; x is read once per 8.  batch > 65535: TIO_ERR_UNSUPPORTED_CONFIG.
 */
int tio_channel_project(const float* x, int32_t batch, int32_t channels, int64_t voxels, const float* center_dev,
                        const float* weights_dev, const float* offset_dev, int32_t components, int32_t clip, float* y,
                        void* stream);

/* ------------------------------------------------------------------------ */
/* Points through a resampling (additive to ABI 18, HIP only)                */
/* ------------------------------------------------------------------------ */
/*
 * A resampling computes out(o) = in(s(o)); a point attached to the image moves by s^-1.  One launch warps the points of a
 * whole batch, one thread per point, 256-thread blocks none of which spans two elements (csrc/points.hip).
 *   points / out        (n_total, 3) float32 on the device at any 4-byte boundary: input voxel coordinates (IJK) in, output
 *                       voxel coordinates out; out may be points itself
 *   status              (n_total,) int8 on the device or NULL: 0 converged (always, without a field), 1 not converged within
 *                       TIO_POINTS_MAX_ITERATIONS steps (the best iterate is stored), 2 the element's block names control
 *                       points outside the buffer (the affine-only answer is stored, the buffer is not read)
 *   offsets_host / _dev the same batch + 1 int32 values on the host (validated: from 0 to n_total, never decreasing; sizes the
 *                       grid) and on the device: element b owns the points offsets[b] .. offsets[b + 1] - 1; an element
 *                       without points owns no block
 *   blocks_dev          (batch, TIO_POINTS_BLOCK_DOUBLES) float64 on the device, 8-byte aligned; per element
 *                         [0:12]  M, the 3x4 output-voxel -> input-voxel matrix inv(A_in) inv(T) A_out, row-major
 *                         [12:24] its inverse, computed by the caller in float64
 *                         [24:27] output shape   [27:30] input spacing   [30:33] output spacing   (mm)
 *                         [33]    affine_first (0 / 1)
 *                         [34:37] control grid (n_i, n_j, n_k)
 *                         [37]    offset of this element's (n_i, n_j, n_k, 3) control points in control_points_dev, in floats;
 *                                 -1: no field                          [38:40] reserved
 *   control_points_dev  float32 on the device, control_floats of them (NULL / 0 when no element has a field)
 * Without a field  o = Minv (p, 1).  With one, s(o) = p is solved for
 *   affine_first:  s(o) = M o + d(o) / spacing_in          otherwise:  s(o) = M (o + d(o) / spacing_out)
 * (spatial.py:1570-1577), d the trilinear interpolation of the control points at o_a (n_a - 1) / max(S_a - 1, 1), the index
 * clamped to [0, n_a - 1] (align_corners=True, spatial.py:2171-2189; constant outside the output grid), by Newton's
 * iteration from the affine-only answer with the cell's analytic Jacobian, the step halved while max|s(o) - p| does not
 * decrease, until that residual is <= TIO_POINTS_TOLERANCE voxel.  That stop decides the status; a converged point then
 * takes one more full step, kept when it lowers the residual.  All arithmetic is float64; the stored float32 is its one
 * rounding.  Nothing is read back and nothing synchronises.  n_total > 2^31 - 1: TIO_ERR_INVALID_ARGUMENT.
 */
#define TIO_POINTS_BLOCK_DOUBLES 40
#define TIO_POINTS_MAX_ITERATIONS 50
#define TIO_POINTS_TOLERANCE 1.0e-7
int tio_points_warp(const float* points, float* out, int8_t* status, int64_t n_total, const int32_t* offsets_host,
                    const int32_t* offsets_dev, int32_t batch, const double* blocks_dev, const float* control_points_dev,
                    int64_t control_floats, void* stream);

/* ------------------------------------------------------------------------ */
/* Patch feeding: weighted centres and patch batches (additive to ABI 18, HIP only) */
/* ------------------------------------------------------------------------ */
/*
 * WeightedSampler / LabelSampler of the reference (data/sampler.py:252-274, 320-360) draw a patch CENTRE from a probability
 * map whose border is masked (a patch centred there would stick out: half <= pos < shape - half on every axis, half =
 * patch / 2 > 0), one torch.multinomial over the whole volume per patch.  Here the law is a two-level inverse CDF.
 *
 * The weight source is channel 0 of an image, (I, J, K) dense, of any tio_dtype (element_type):
 *   label_mode 0   the voxel converted to float32 (`.float()`, sampler.py:281);
 *   label_mode 1   a label looked up in the HOST table of n_labels <= TIO_CENTRE_MAX_LABELS (label_values[q],
 *                  label_weights[q]) pairs, later pairs overriding earlier ones (the loop of assignments at sampler.py:324-327),
 *                  0 for a label the table does not hold; n_labels == 0: weight = label > 0 (sampler.py:329).
 * A SEGMENT is TIO_CENTRE_SEGMENT consecutive flat voxels (the last one may be shorter).
 *
 * tio_centre_law_sums: prefix_dev receives ceil(I J K / TIO_CENTRE_SEGMENT) float64 values, the inclusive prefix sums of the
 * segments' masked weights; record_dev the total and whether any unmasked weight is negative, infinite or NaN.  The masked
 * map is never stored.  Three stream-ordered steps: the record is cleared; one launch adds every segment in a fixed order
 * within the block that owns it; one single-block launch adds the segment totals in ascending order.  No floating-point
 * atomic: the values do not depend on the launch geometry.
 *
 * tio_centre_draw: n_draws independent draws with replacement from the law the same source arguments describe, prefix_dev /
 * record_dev as left by tio_centre_law_sums.  Uniforms: uniforms_dev[n] (float64 in [0, 1)) or, when that is NULL, this
 * library's stream: philox4x32_10 (csrc/philox_normal.hpp), counter {n lo, n hi, 2, 0}, key {seed lo, seed hi},
 * u = ((c[0] >> 5) * 2^26 + (c[1] >> 6)) * 2^-53 (stream ids 0 and 1 of that counter word belong to the noise).
 * uniforms_out_dev (or NULL) receives the values used.  Per draw: t = u * total; the first segment whose prefix exceeds t
 * (binary search); its weights recomputed as the sums computed them; the first voxel of positive weight at which the running
 * float64 sum, added in flat order, exceeds t - prefix_before; if rounding leaves none, the segment's last voxel of positive
 * weight.  centres_dev[n]: the flat index (-1 when the law holds no positive weight); corners_dev[n][3]:
 * min(max(centre - patch / 2, 0), shape - patch).  A voxel of zero weight is never chosen.
 */
#define TIO_CENTRE_SEGMENT 2048
#define TIO_CENTRE_MAX_LABELS 64
typedef struct tio_centre_record {
  double total;     /* float64 sum of the masked weights */
  int32_t invalid;  /* 1: an unmasked weight is negative, infinite or NaN */
  int32_t reserved; /* 0 */
} tio_centre_record;
int tio_centre_law_sums(const void* weights, int32_t element_type, int32_t label_mode, const double* label_values,
                        const float* label_weights, int32_t n_labels, const int32_t shape[3], const int32_t patch[3],
                        double* prefix_dev, tio_centre_record* record_dev, void* stream);
int tio_centre_draw(const void* weights, int32_t element_type, int32_t label_mode, const double* label_values,
                    const float* label_weights, int32_t n_labels, const int32_t shape[3], const int32_t patch[3],
                    const double* prefix_dev, const tio_centre_record* record_dev, int64_t n_draws, uint64_t seed,
                    const double* uniforms_dev, double* uniforms_out_dev, int64_t* centres_dev, int32_t* corners_dev, void* stream);

/*
 * All patches of one image in one launch (the slicing of sampler.py:54-67, N times, and the torch.stack of the collation):
 * x (channels, I, J, K) -> y (n_patches, channels, pi, pj, pk), elements of 1, 2, 4 or 8 bytes moved as bits.  corners_dev is
 * int32 [n_patches][3] ON THE DEVICE (after tio_centre_draw nothing goes through the host); each corner is clamped to
 * [0, shape - patch] inside the kernel, so no read leaves x whatever the array holds.  y is written in aligned 16-byte
 * stores (single elements up to its first and after its last 16-byte boundary of each patch volume), x is read with the
 * widest loads the address of each 16-byte group allows.  patch > shape on any axis: TIO_ERR_INVALID_ARGUMENT, nothing
 * launched.
 */
int tio_patch_gather(const void* x, void* y, int32_t element_bytes, int32_t channels, const int32_t shape[3], const int32_t patch[3],
                     const int32_t* corners_dev, int32_t n_patches, void* stream);

/*
 * NIfTI-1 payloads decoded on the device (additive to ABI 18, HIP only): what a host reader does after reading the bytes
 * - reinterpret, byte swap, Fortran-to-C reorder, promotion or scaling, conversion - as ONE launch over the raw bytes.
 *   raw_dev  batch * channels dense volumes of I * J * K disk elements each, back to back, exactly as they lie in the
 *            file (I fastest, the channel slowest); the first starts on a 16-byte boundary
 *   y        (batch, channels, I, J, K) contiguous, of out_type:  y[b, c, i, j, k] = raw[b * channels + c][(k * J + j) * I + i]
 *   values   unscaled: the disk value in its natural type - the disk type itself, except u16 -> int32, u32 -> int64 and
 *            u64 -> int64 (two's-complement wrap);  scaled: double(x) * slope, rounded, + inter, rounded (no fma): float64
 *   out_type the natural type (TIO_F64 when scaled), or TIO_F32 / TIO_F64 reached by ONE round-to-nearest-even
 *            conversion from the exact unscaled value or from the float64 scaled value; anything else:
 *            TIO_ERR_UNSUPPORTED_DTYPE
 * disk_type is a NIfTI-1 datatype code: 2 u8, 4 i16, 8 i32, 16 f32, 64 f64, 256 i8, 512 u16, 768 u32, 1024 i64, 1280 u64.
 * I > 1 and K > 1 go through a 64 x 64 LDS tile (rows read along i, columns written along k); I == 1 or K == 1 (2-D
 * images) move element by element.  Bad arguments: TIO_ERR_INVALID_ARGUMENT, nothing launched.  raw_dev and y must not
 * overlap.
 */
typedef struct tio_nifti_layout {
  int32_t disk_type;  /* NIfTI datatype code */
  int32_t swap_bytes; /* payload is big-endian */
  int32_t shape[3];   /* I, J, K: on disk I is the fastest axis, in y K is */
  int32_t channels;
  int32_t scaled;     /* apply slope / inter (float64 arithmetic, two roundings) */
  double slope, inter;
} tio_nifti_layout;
int tio_nifti_decode(const void* raw_dev, void* y, int32_t out_type, int32_t batch, const tio_nifti_layout* layout, void* stream);

/* ------------------------------------------------------------------------ */
/* Introspection                                                             */
/* ------------------------------------------------------------------------ */
int tio_abi_version(void);
const char* tio_last_error(void);
/* Number of visible HIP devices (0 when none; never throws). */
int tio_device_count(void);
/* The library parses its TIO_* environment switches (A/B experiments, see torchio_amd/csrc/common.hpp: EnvSwitches)
 * ONCE, at the first call that needs one; no entry point calls getenv() afterwards.  A process that changes such a
 * variable later (tests, tests/native/resample_bench) calls this to have them parsed again.  ABI 10. */
void tio_reload_env(void);
/* The cache policy a launch that writes `bytes_written` bytes takes (host only, nothing is launched): 1 = "stream" — its
 * once-touched rows bypass the caches' retention (nontemporal loads and stores: the marching stencil passes of
 * tio_separable_conv3d / tio_blur_fused), 0 = the default policy.  A launch streams when it writes more than the Infinity Cache holds
 * (256 MiB), or more than TIO_STREAM_BYTES when that is set (0: every launch streams).  Results do not depend on it. */
int tio_launch_streams(int64_t bytes_written);

#ifdef __cplusplus
}
#endif
#endif /* TIO_HIP_H */
