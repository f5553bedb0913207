// nifti_codec.hip — tio_nifti_decode: the payload of NIfTI-1 files, as it lies on disk, to (B, C, I, J, K) tensors in ONE launch.
// On disk I is the fastest axis and the channel the slowest; in y K is the fastest.  So the move is a full axis reversal per
// (b, c) volume,
//
//   y[b, c, i, j, k] = convert(raw[b * C + c][(k * J + j) * I + i]),
//
// and convert() is everything a host reader does after the reorder: byte swap of a big-endian payload, the promotion of the
// unsigned types torch does not have (u16 -> i32, u32 / u64 -> i64), or the scaling `double(x) * slope + inter` with two
// roundings (this file is built with -ffp-contract=off like every other), and at most ONE further rounding to float32.
//
// Two routes, chosen on the host from the shape alone:
//   I > 1 and K > 1  the fast axes differ: the 64 x 64 LDS tile of permute.hip over i (fast on the read side) and k (fast on
//                    the write side).  Rows are read along i and columns are written along k, so both sides are coalesced; j
//                    and B * C are folded with the tile coordinates into one linear tile index that the blocks stride over.
//                    The cells hold the RAW disk element (a dword, or a dword pair for the 8-byte types; 1- and 2-byte
//                    types are staged one element per dword), the row pitch is 65 cells: a column read of dwords touches
//                    bank (lane * 65 + row) % 32 = (lane + row) % 32, distinct inside each 32-lane group, and dword pairs
//                    2 * (lane + row) % 64, distinct as well.  The conversion runs in registers between the LDS read and
//                    the store, so the tile is as small as the disk type allows and one tile serves every output type.
//   I == 1 or K == 1 (2-D images, single rows): one thread per output element, lanes along the output's fast axis.
// Edge tiles are predicated per lane; a lane never reads a cell that was not written for the same tile.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.hpp"

namespace tio {
namespace {

constexpr int NIFTI_TILE = 64;
constexpr int NIFTI_PITCH = NIFTI_TILE + 1;

// NIfTI-1 datatype codes (nifti1.h: DT_UINT8 ... DT_UINT64)
enum : int { NII_U8 = 2, NII_I16 = 4, NII_I32 = 8, NII_F32 = 16, NII_F64 = 64, NII_I8 = 256, NII_U16 = 512, NII_U32 = 768, NII_I64 = 1024, NII_U64 = 1280 };

template <int DISK> struct Disk;
#define TIO_NIFTI_DISK(CODE, T, NATURAL)                 \
  template <> struct Disk<CODE> {                        \
    using type = T;                                      \
    static constexpr int natural = NATURAL;              \
  };
TIO_NIFTI_DISK(NII_U8, uint8_t, TIO_U8)
TIO_NIFTI_DISK(NII_I8, int8_t, TIO_I8)
TIO_NIFTI_DISK(NII_I16, int16_t, TIO_I16)
TIO_NIFTI_DISK(NII_U16, uint16_t, TIO_I32)
TIO_NIFTI_DISK(NII_I32, int32_t, TIO_I32)
TIO_NIFTI_DISK(NII_U32, uint32_t, TIO_I64)
TIO_NIFTI_DISK(NII_I64, int64_t, TIO_I64)
TIO_NIFTI_DISK(NII_U64, uint64_t, TIO_I64)
TIO_NIFTI_DISK(NII_F32, float, TIO_F32)
TIO_NIFTI_DISK(NII_F64, double, TIO_F64)
#undef TIO_NIFTI_DISK

int natural_type(int disk) {
  switch (disk) {
    case NII_U8: return TIO_U8;
    case NII_I8: return TIO_I8;
    case NII_I16: return TIO_I16;
    case NII_U16: case NII_I32: return TIO_I32;
    case NII_U32: case NII_I64: case NII_U64: return TIO_I64;
    case NII_F32: return TIO_F32;
    case NII_F64: return TIO_F64;
    default: return -1;
  }
}

template <int OUT> struct OutType;
template <> struct OutType<TIO_U8> { using type = uint8_t; };
template <> struct OutType<TIO_I8> { using type = int8_t; };
template <> struct OutType<TIO_I16> { using type = int16_t; };
template <> struct OutType<TIO_I32> { using type = int32_t; };
template <> struct OutType<TIO_I64> { using type = int64_t; };
template <> struct OutType<TIO_F32> { using type = float; };
template <> struct OutType<TIO_F64> { using type = double; };

template <int ES> __device__ __forceinline__ typename RawBits<ES>::type swap_bytes(typename RawBits<ES>::type v);
template <> __device__ __forceinline__ uint8_t swap_bytes<1>(uint8_t v) { return v; }
template <> __device__ __forceinline__ uint16_t swap_bytes<2>(uint16_t v) { return static_cast<uint16_t>((v << 8) | (v >> 8)); }
template <> __device__ __forceinline__ uint32_t swap_bytes<4>(uint32_t v) { return __builtin_bswap32(v); }
template <> __device__ __forceinline__ uint64_t swap_bytes<8>(uint64_t v) { return __builtin_bswap64(v); }

// raw bits of one disk element -> one output element.  Integer -> float conversions are single roundings to nearest even
// (v_cvt_* for up to 32 bits, the compiler's exact sticky-bit sequence for 64-bit integers); the unscaled natural type only
// moves bits (two's-complement wrap for u64 -> i64, NaN payloads untouched).
template <int DISK, int OUT, bool SCALED>
__device__ __forceinline__ typename OutType<OUT>::type convert(typename RawBits<sizeof(typename Disk<DISK>::type)>::type bits, bool swap,
                                                               double slope, double inter) {
  using T = typename Disk<DISK>::type;
  using O = typename OutType<OUT>::type;
  constexpr int ES = sizeof(T);
  if (swap) bits = swap_bytes<ES>(bits);
  T value;
  __builtin_memcpy(&value, &bits, ES);
  if constexpr (SCALED) {
    const double scaled = __dadd_rn(__dmul_rn(static_cast<double>(value), slope), inter);  // two roundings, never an fma
    return static_cast<O>(scaled);
  } else if constexpr (OUT == Disk<DISK>::natural && !std::is_floating_point<T>::value) {
    return static_cast<O>(value);  // same width, or a widening that keeps the value (u16 -> i32, u32 -> i64); u64 -> i64 wraps
  } else if constexpr (OUT == Disk<DISK>::natural) {
    O moved;
    __builtin_memcpy(&moved, &bits, ES);
    return moved;
  } else {
    return static_cast<O>(value);
  }
}

struct NiftiArgs {
  const void* raw;
  void* y;
  int64_t n;        // elements of one (b, c) volume
  int64_t n_bc;     // batch * channels
  int64_t n_tiles;  // tiles_i * tiles_k * J * n_bc
  int I, J, K;
  int tiles_i, tiles_k;
  int swap;
  double slope, inter;
};

template <int DISK, int OUT, bool SCALED>
__global__ __launch_bounds__(256) void nifti_rows_kernel(const NiftiArgs a) {
  using T = typename Disk<DISK>::type;
  using RAW = typename RawBits<sizeof(T)>::type;
  using O = typename OutType<OUT>::type;
  const int64_t total = a.n * a.n_bc;
  const bool swap = a.swap != 0;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < total;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t bc = t / a.n;
    const int64_t r = t - bc * a.n;
    const int k = static_cast<int>(r % a.K);
    const int j = static_cast<int>((r / a.K) % a.J);
    const int i = static_cast<int>(r / (static_cast<int64_t>(a.J) * a.K));
    const RAW bits = static_cast<const RAW*>(a.raw)[bc * a.n + (static_cast<int64_t>(k) * a.J + j) * a.I + i];
    static_cast<O*>(a.y)[t] = convert<DISK, OUT, SCALED>(bits, swap, a.slope, a.inter);
  }
}

template <int DISK, int OUT, bool SCALED>
__global__ __launch_bounds__(256) void nifti_tile_kernel(const NiftiArgs a) {
  using T = typename Disk<DISK>::type;
  constexpr int ES = sizeof(T);
  using RAW = typename RawBits<ES>::type;
  using CELL = typename std::conditional<ES == 8, uint64_t, uint32_t>::type;
  using O = typename OutType<OUT>::type;
  __shared__ CELL tile[NIFTI_TILE][NIFTI_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool swap = a.swap != 0;
  const int64_t plane_in = static_cast<int64_t>(a.J) * a.I;   // disk stride of k
  const int64_t plane_out = static_cast<int64_t>(a.J) * a.K;  // output stride of i
  for (int64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
    int64_t q = t;
    const int i0 = static_cast<int>(q % a.tiles_i) * NIFTI_TILE;
    q /= a.tiles_i;
    const int k0 = static_cast<int>(q % a.tiles_k) * NIFTI_TILE;
    q /= a.tiles_k;
    const int j = static_cast<int>(q % a.J);
    const int64_t bc = q / a.J;
    const int rows_k = min(NIFTI_TILE, a.K - k0), rows_i = min(NIFTI_TILE, a.I - i0);
    // rows along i: lane = i inside the tile, the waves share the rows k
    if (lane < rows_i) {
      const RAW* src = static_cast<const RAW*>(a.raw) + bc * a.n + k0 * plane_in + static_cast<int64_t>(j) * a.I + (i0 + lane);
#pragma unroll 4
      for (int row = wave; row < rows_k; row += 4) tile[row][lane] = src[row * plane_in];
    }
    __syncthreads();
    // columns along k: lane = k inside the tile, the waves share the output rows i
    if (lane < rows_k) {
      O* dst = static_cast<O*>(a.y) + bc * a.n + i0 * plane_out + static_cast<int64_t>(j) * a.K + (k0 + lane);
#pragma unroll 4
      for (int row = wave; row < rows_i; row += 4)
        dst[row * plane_out] = convert<DISK, OUT, SCALED>(static_cast<RAW>(tile[lane][row]), swap, a.slope, a.inter);
    }
    __syncthreads();  // the next tile of this block overwrites the cells
  }
}

template <int DISK, int OUT, bool SCALED>
int launch_decode(const NiftiArgs& a, bool tiled, hipStream_t s) {
  if (tiled) {
    int64_t blocks = a.n_tiles;
    if (blocks > (1 << 20)) blocks = 1 << 20;  // the blocks stride over the rest
    hipLaunchKernelGGL((nifti_tile_kernel<DISK, OUT, SCALED>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, a);
  } else {
    int64_t blocks = (a.n * a.n_bc + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL((nifti_rows_kernel<DISK, OUT, SCALED>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, a);
  }
  return check_launch("tio_nifti_decode");
}

// the output types one disk type has: its natural type, float32 and float64 when unscaled; float64 and float32 when scaled
template <int DISK>
int decode_disk(const NiftiArgs& a, int out_type, bool scaled, bool tiled, hipStream_t s) {
  constexpr int NATURAL = Disk<DISK>::natural;
  if (scaled) {
    if (out_type == TIO_F64) return launch_decode<DISK, TIO_F64, true>(a, tiled, s);
    if (out_type == TIO_F32) return launch_decode<DISK, TIO_F32, true>(a, tiled, s);
  } else {
    if (out_type == NATURAL) return launch_decode<DISK, NATURAL, false>(a, tiled, s);
    if (out_type == TIO_F32) return launch_decode<DISK, TIO_F32, false>(a, tiled, s);
    if (out_type == TIO_F64) return launch_decode<DISK, TIO_F64, false>(a, tiled, s);
  }
  return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_nifti_decode: out_type %d for disk type %d%s (its natural type, float32 or float64)", out_type, DISK,
              scaled ? ", scaled" : "");
}

}  // namespace
}  // namespace tio

extern "C" int tio_nifti_decode(const void* raw_dev, void* y, int32_t out_type, int32_t batch, const tio_nifti_layout* layout, void* stream) {
  using namespace tio;
  if (layout == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_nifti_decode: null layout");
  const int natural = natural_type(layout->disk_type);
  if (natural < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_nifti_decode: disk_type %d is not a supported NIfTI-1 datatype", layout->disk_type);
  if (batch < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_nifti_decode: negative batch");
  if (layout->channels < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_nifti_decode: channels must be >= 1");
  for (int d = 0; d < 3; d++)
    if (layout->shape[d] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_nifti_decode: shapes must be >= 1");
  const bool scaled = layout->scaled != 0;
  const bool allowed = out_type == TIO_F32 || out_type == TIO_F64 || (!scaled && out_type == natural);
  if (!allowed)
    return fail(TIO_ERR_UNSUPPORTED_DTYPE, "tio_nifti_decode: out_type %d for disk type %d%s (its natural type, float32 or float64)", out_type,
                layout->disk_type, scaled ? ", scaled" : "");
  if (batch == 0) return TIO_OK;
  if (raw_dev == nullptr || y == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_nifti_decode: null data");
  if ((reinterpret_cast<uintptr_t>(raw_dev) & 15) != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "tio_nifti_decode: raw_dev must be 16-byte aligned");
  NiftiArgs a{};
  a.raw = raw_dev; a.y = y;
  a.I = layout->shape[0]; a.J = layout->shape[1]; a.K = layout->shape[2];
  a.n = static_cast<int64_t>(a.I) * a.J * a.K;
  a.n_bc = static_cast<int64_t>(batch) * layout->channels;
  a.tiles_i = (a.I + NIFTI_TILE - 1) / NIFTI_TILE;
  a.tiles_k = (a.K + NIFTI_TILE - 1) / NIFTI_TILE;
  a.n_tiles = static_cast<int64_t>(a.tiles_i) * a.tiles_k * a.J * a.n_bc;
  a.swap = layout->swap_bytes != 0;
  a.slope = layout->slope; a.inter = layout->inter;
  const bool tiled = a.I > 1 && a.K > 1;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (layout->disk_type) {
    case NII_U8: return decode_disk<NII_U8>(a, out_type, scaled, tiled, s);
    case NII_I8: return decode_disk<NII_I8>(a, out_type, scaled, tiled, s);
    case NII_I16: return decode_disk<NII_I16>(a, out_type, scaled, tiled, s);
    case NII_U16: return decode_disk<NII_U16>(a, out_type, scaled, tiled, s);
    case NII_I32: return decode_disk<NII_I32>(a, out_type, scaled, tiled, s);
    case NII_U32: return decode_disk<NII_U32>(a, out_type, scaled, tiled, s);
    case NII_I64: return decode_disk<NII_I64>(a, out_type, scaled, tiled, s);
    case NII_U64: return decode_disk<NII_U64>(a, out_type, scaled, tiled, s);
    case NII_F32: return decode_disk<NII_F32>(a, out_type, scaled, tiled, s);
    default: return decode_disk<NII_F64>(a, out_type, scaled, tiled, s);
  }
}
