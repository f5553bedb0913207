// permute.hip — tio_permute3d: an axis permutation of a (B, C, I, J, K) volume with flips folded into the addressing.
// Replaces Reorient's up to three torch.flip passes plus permute(...).contiguous() (transforms/spatial/reorient.py:63-91
// _apply_reorientation) and Transpose's permute(0, 1, 4, 3, 2).contiguous() (transforms/spatial/transpose.py:44):
// one launch that reads and writes every byte once.
//
//   y[b, c, o0, o1, o2] = x[b, c, i0, i1, i2],  i[perm[d]] = o_d, or in_shape[perm[d]] - 1 - o_d when bit perm[d] of the
//   flip mask is set (nibabel's apply_orientation: flip the input axes, then transpose).
//
// Two routes, chosen on the host from perm alone:
//   perm[2] == 2  rows along K stay rows: one thread per output element, lanes along K on both sides (like flip_kernel).
//   perm[2] != 2  the fast output axis is a slow input axis.  A 64 x 64 tile over input axis 2 ("k", fast on the read
//                 side) and input axis perm[2] ("m", fast on the write side) goes through LDS: rows are read along k and
//                 columns are written along m, so both sides are coalesced.  The third spatial axis ("r") and B*C are the
//                 slow dimension, folded with the tile coordinates into one linear tile index that the blocks stride over
//                 (no gridDim.y/z limit).  The row pitch is 65 elements: a column read of 4-byte elements then touches
//                 bank (lane * 65 + row) % 32 = (lane + row) % 32, distinct inside each 32-lane half; 8-byte elements
//                 take the dword pairs 2 * (lane + row) % 64, distinct as well.  1- and 2-byte elements are staged as
//                 dwords (one element per lane and access).
// Flips only change which output row / column a tile maps to and the direction inside it.  Edge tiles are predicated per
// lane on the INPUT coordinates, which map one-to-one onto output coordinates.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.hpp"

namespace tio {
namespace {

constexpr int PERMUTE_TILE = 64;
constexpr int PERMUTE_PITCH = PERMUTE_TILE + 1;

struct PermuteRowArgs {
  const void* x;
  void* y;
  int64_t n_bc;
  int in[3], out[3];
  int perm0, perm1;  // input axes of output axes 0 and 1 (output axis 2 is input axis 2)
  int mask;
};

template <int ES>
__global__ __launch_bounds__(256) void permute_rows_kernel(const PermuteRowArgs a) {
  using RAW = typename RawBits<ES>::type;
  const int64_t n = static_cast<int64_t>(a.out[0]) * a.out[1] * a.out[2];
  const int64_t total = n * a.n_bc;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t bc = t / n;
    const int64_t r = t - bc * n;
    int k = static_cast<int>(r % a.out[2]);
    int o1 = static_cast<int>((r / a.out[2]) % a.out[1]);
    int o0 = static_cast<int>(r / (static_cast<int64_t>(a.out[1]) * a.out[2]));
    if (a.mask & (1 << a.perm0)) o0 = a.out[0] - 1 - o0;
    if (a.mask & (1 << a.perm1)) o1 = a.out[1] - 1 - o1;
    if (a.mask & 4) k = a.out[2] - 1 - k;
    const int i = a.perm0 == 0 ? o0 : o1;
    const int j = a.perm0 == 0 ? o1 : o0;
    static_cast<RAW*>(a.y)[t] = static_cast<const RAW*>(a.x)[bc * n + (static_cast<int64_t>(i) * a.in[1] + j) * a.in[2] + k];
  }
}

struct PermuteTileArgs {
  const void* x;
  void* y;
  int64_t n;             // elements of one (b, c) volume
  int64_t n_tiles;       // tiles_k * tiles_m * R * B * C
  int K, M, R;           // extents of input axis 2, of input axis perm[2] and of the remaining input axis
  int tiles_k, tiles_m;
  int64_t in_stride_m, in_stride_r;    // input element strides of m and r (k has stride 1)
  int64_t out_stride_k, out_stride_r;  // output element strides of the axes k and r land on (m lands on stride 1)
  int flip_k, flip_m, flip_r;
};

template <int ES>
__global__ __launch_bounds__(256) void permute_tile_kernel(const PermuteTileArgs a) {
  using RAW = typename RawBits<ES>::type;
  using CELL = typename std::conditional<ES == 8, uint64_t, uint32_t>::type;
  __shared__ CELL tile[PERMUTE_TILE][PERMUTE_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    int64_t q = t;
    const int k0 = static_cast<int>(q % a.tiles_k) * PERMUTE_TILE;
    q /= a.tiles_k;
    const int m0 = static_cast<int>(q % a.tiles_m) * PERMUTE_TILE;
    q /= a.tiles_m;
    const int r = static_cast<int>(q % a.R);
    const int64_t bc = q / a.R;
    const int rows_m = min(PERMUTE_TILE, a.M - m0), rows_k = min(PERMUTE_TILE, a.K - k0);
    // rows along k: lane = k inside the tile, the waves share the rows m
    if (lane < rows_k) {
      const RAW* src = static_cast<const RAW*>(a.x) + bc * a.n + r * a.in_stride_r + m0 * a.in_stride_m + (k0 + lane);
#pragma unroll 4
      for (int row = wave; row < rows_m; row += 4) tile[row][lane] = src[row * a.in_stride_m];
    }
    __syncthreads();
    // columns along m: lane = m inside the tile, the waves share the output rows k
    if (lane < rows_m) {
      const int ro = a.flip_r ? a.R - 1 - r : r;
      const int mo = a.flip_m ? a.M - 1 - (m0 + lane) : m0 + lane;
      RAW* dst = static_cast<RAW*>(a.y) + bc * a.n + ro * a.out_stride_r + mo;
#pragma unroll 4
      for (int row = wave; row < rows_k; row += 4) {
        const int ko = a.flip_k ? a.K - 1 - (k0 + row) : k0 + row;
        dst[ko * a.out_stride_k] = static_cast<RAW>(tile[lane][row]);
      }
    }
    __syncthreads();  // the next tile of this block overwrites the cells
  }
}

template <typename Kernel, typename Args>
int launch_permute(Kernel kernel, const Args& a, int64_t blocks, hipStream_t s) {
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, a);
  return check_launch("tio_permute3d");
}

}  // namespace
}  // namespace tio

extern "C" int tio_permute3d(const void* x, void* y, int32_t dtype, int32_t batch, int32_t channels, const int32_t in_shape[3],
                             const int32_t perm[3], int32_t flip_mask, void* stream) {
  using namespace tio;
  if (in_shape == nullptr || perm == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_permute3d: null shape or perm");
  const int es = dtype_size(dtype);
  if (!is_known_dtype(dtype)) return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_permute3d: dtype %d", dtype);
  if (batch < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_permute3d: negative batch");
  if (channels < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_permute3d: channels must be >= 1");
  int seen = 0;
  for (int d = 0; d < 3; d++) {
    if (in_shape[d] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_permute3d: shapes must be >= 1");
    if (perm[d] >= 0 && perm[d] <= 2) seen |= 1 << perm[d];
  }
  if (seen != 7)
    return fail(TIO_ERR_INVALID_ARGUMENT, "tio_permute3d: perm (%d, %d, %d) is not a permutation of (0, 1, 2)", perm[0], perm[1], perm[2]);
  if (flip_mask < 0 || flip_mask > 7) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_permute3d: flip mask %d outside 0..7", flip_mask);
  if (batch == 0) return TIO_OK;
  if (x == nullptr || y == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_permute3d: null data");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n_bc = static_cast<int64_t>(batch) * channels;
  const int64_t n = static_cast<int64_t>(in_shape[0]) * in_shape[1] * in_shape[2];
  const int out[3] = {in_shape[perm[0]], in_shape[perm[1]], in_shape[perm[2]]};

  if (perm[2] == 2) {  // rows stay rows
    PermuteRowArgs a{};
    a.x = x; a.y = y; a.n_bc = n_bc; a.perm0 = perm[0]; a.perm1 = perm[1]; a.mask = flip_mask;
    for (int d = 0; d < 3; d++) { a.in[d] = in_shape[d]; a.out[d] = out[d]; }
    int64_t blocks = (n * n_bc + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    int status = TIO_OK;
    const bool known = dispatch_element_size(es, [&](auto size) { status = launch_permute(permute_rows_kernel<decltype(size)::value>, a, blocks, s); });
    return known ? status : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_permute3d: dtype %d", dtype);
  }

  // the tile: input axis 2 (k) x input axis perm[2] (m); r is the input axis that is left
  const int axis_m = perm[2], axis_r = 1 - axis_m;
  const int d_k = perm[0] == 2 ? 0 : 1, d_r = 1 - d_k;  // the output axes k and r land on
  const int64_t in_stride[3] = {static_cast<int64_t>(in_shape[1]) * in_shape[2], in_shape[2], 1};
  const int64_t out_stride[3] = {static_cast<int64_t>(out[1]) * out[2], out[2], 1};
  PermuteTileArgs a{};
  a.x = x; a.y = y; a.n = n;
  a.K = in_shape[2]; a.M = in_shape[axis_m]; a.R = in_shape[axis_r];
  a.tiles_k = (a.K + PERMUTE_TILE - 1) / PERMUTE_TILE;
  a.tiles_m = (a.M + PERMUTE_TILE - 1) / PERMUTE_TILE;
  a.n_tiles = static_cast<int64_t>(a.tiles_k) * a.tiles_m * a.R * n_bc;
  a.in_stride_m = in_stride[axis_m]; a.in_stride_r = in_stride[axis_r];
  a.out_stride_k = out_stride[d_k]; a.out_stride_r = out_stride[d_r];
  a.flip_k = (flip_mask >> 2) & 1; a.flip_m = (flip_mask >> axis_m) & 1; a.flip_r = (flip_mask >> axis_r) & 1;
  int64_t blocks = a.n_tiles;
  if (blocks > (1 << 20)) blocks = 1 << 20;  // the blocks stride over the rest
  int status = TIO_OK;
  const bool known = dispatch_element_size(es, [&](auto size) { status = launch_permute(permute_tile_kernel<decltype(size)::value>, a, blocks, s); });
  return known ? status : fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_permute3d: dtype %d", dtype);
}
