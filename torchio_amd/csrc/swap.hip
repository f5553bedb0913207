// swap.hip — Swap (reference transforms/intensity/swap.py: _apply_swaps :195-219, _apply_swaps_per_instance :222-258).
//
// The reference replays S swaps one after the other, four small copies each.  Every swap moves whole voxels, so the result
// is a gather from the INPUT: for an output voxel t walk the swaps from the last to the first — where the position lies in
// B_r it came from A_r (B is written last, so it wins where the two overlap), else where it lies in A_r it came from B_r —
// and out[t] = in[position].
//
// One stream-ordered copy x -> y, then ONE launch whose threads are the voxels of the 2 S boxes (times channels, times
// batch).  The thread for voxel t of box X of swap s leaves when a later swap's A or B contains t, or when X is A and B_s
// contains t: of all (swap, box) pairs that contain t exactly one stays — the last one in the order A_0 B_0 A_1 B_1 ... —
// so every voxel has at most one writer, nothing is atomic, and the launch reads x only, never y.
// A block works on one box: its own origins are read through indices that depend on the block alone (scalar loads).
#include "common.hpp"

namespace tio {
namespace {

struct SwapGeom {
  int32_t shape[3], patch[3];
  int32_t channels, lists, s_max;
  int64_t tasks;           // batch * channels * s_max * 2 * blocks_per_box
  int32_t blocks_per_box;
};

__device__ __forceinline__ bool inside(int i, int j, int k, const int32_t* o, const int32_t* p) {
  return i >= o[0] && i < o[0] + p[0] && j >= o[1] && j < o[1] + p[1] && k >= o[2] && k < o[2] + p[2];
}

// two boxes of the patch's size share a voxel
__device__ __forceinline__ bool boxes_meet(const int32_t* o, const int32_t* other, const int32_t* p) {
  return abs(o[0] - other[0]) < p[0] && abs(o[1] - other[1]) < p[1] && abs(o[2] - other[2]) < p[2];
}

// Whether two BOXES meet is the same for every voxel of a block, and most boxes meet no other box.  So the swaps are first
// looked at 256 at a time, one per thread: which later swaps have a box that meets this block's box (only those can contain
// one of its voxels), and which is the last earlier swap with a box that meets the PARTNER box — swap s moves every voxel of
// the box to its partner's place, and the positions of the block stay together inside that box until such a swap moves some
// of them and not others; from there on each voxel is traced on its own.
template <typename T>
__global__ __launch_bounds__(256) void swap_gather_kernel(const T* __restrict__ x, T* __restrict__ y, const int32_t* __restrict__ origins,
                                                          const int32_t* __restrict__ counts, SwapGeom g) {
  __shared__ unsigned long long later_mask[4], earlier_mask[4];  // per wave of the block: bit = lane = swap of the chunk
  const int64_t n_spatial = static_cast<int64_t>(g.shape[0]) * g.shape[1] * g.shape[2];
  const int patch_voxels = g.patch[0] * g.patch[1] * g.patch[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t task = blockIdx.x; task < g.tasks; task += gridDim.x) {  // (everything up to `v` is uniform in the block)
    const int chunk = static_cast<int>(task % g.blocks_per_box);
    int64_t rest = task / g.blocks_per_box;
    const int which = static_cast<int>(rest % 2);  // 0: box A, 1: box B
    rest /= 2;
    const int s = static_cast<int>(rest % g.s_max);
    const int64_t bc = rest / g.s_max;
    const int list = g.lists == 1 ? 0 : static_cast<int>(bc / g.channels);
    int count = counts[list];
    count = count < g.s_max ? count : g.s_max;
    if (s >= count) continue;
    const int32_t* boxes = origins + static_cast<int64_t>(list) * g.s_max * 6;  // [s][A, B][3]
    const int32_t* own = boxes + (2 * s + which) * 3;
    const int32_t* partner = boxes + (2 * s + 1 - which) * 3;
    // an origin outside the volume (the caller checks them): nothing is written for that box
    if (own[0] < 0 || own[1] < 0 || own[2] < 0 || own[0] > g.shape[0] - g.patch[0] || own[1] > g.shape[1] - g.patch[1] ||
        own[2] > g.shape[2] - g.patch[2])
      continue;
    const int v = chunk * 256 + static_cast<int>(threadIdx.x);
    const bool active = v < patch_voxels;  // (the others only help with the swaps)
    int i = own[0] + v / (g.patch[1] * g.patch[2]);
    int j = own[1] + v / g.patch[2] % g.patch[1];
    int k = own[2] + v % g.patch[2];
    bool later = which == 0 && inside(i, j, k, partner, g.patch);  // B_s is written after A_s
    int diverge = -1;                                              // the last swap before s that meets the partner box
    for (int base = (count - 1) / 256 * 256; base >= 0; base -= 256) {
      const int r = base + static_cast<int>(threadIdx.x);
      bool meets_own = false, meets_partner = false;
      if (r < count && r != s) {
        const int32_t *a = boxes + 2 * r * 3, *b = a + 3;
        if (r > s) meets_own = boxes_meet(own, a, g.patch) || boxes_meet(own, b, g.patch);
        else meets_partner = boxes_meet(partner, a, g.patch) || boxes_meet(partner, b, g.patch);
      }
      const unsigned long long mine_later = __ballot(meets_own), mine_earlier = __ballot(meets_partner);
      if (lane == 0) later_mask[wave] = mine_later, earlier_mask[wave] = mine_earlier;
      __syncthreads();
      for (int w = 3; w >= 0; w--) {
        unsigned long long bits = later_mask[w];
        while (bits != 0ull && !later) {
          const int bit = 63 - __clzll(static_cast<long long>(bits));
          bits &= ~(1ull << bit);
          const int32_t *a = boxes + 2 * (base + w * 64 + bit) * 3, *b = a + 3;
          later = inside(i, j, k, a, g.patch) || inside(i, j, k, b, g.patch);
        }
        if (diverge < 0 && earlier_mask[w] != 0ull) diverge = base + w * 64 + 63 - __clzll(static_cast<long long>(earlier_mask[w]));
      }
      __syncthreads();  // (the masks are read)
    }
    if (later || !active) continue;  // a later box's thread writes this voxel
    const int64_t to = (static_cast<int64_t>(i) * g.shape[1] + j) * g.shape[2] + k;
    i += partner[0] - own[0], j += partner[1] - own[1], k += partner[2] - own[2];
    for (int r = diverge; r >= 0; r--) {
      const int32_t *a = boxes + 2 * r * 3, *b = a + 3;
      if (inside(i, j, k, b, g.patch)) {
        i += a[0] - b[0], j += a[1] - b[1], k += a[2] - b[2];
      } else if (inside(i, j, k, a, g.patch)) {
        i += b[0] - a[0], j += b[1] - a[1], k += b[2] - a[2];
      }
    }
    if (i < 0 || j < 0 || k < 0 || i >= g.shape[0] || j >= g.shape[1] || k >= g.shape[2]) continue;  // (an earlier box out of range)
    const int64_t from = (static_cast<int64_t>(i) * g.shape[1] + j) * g.shape[2] + k;
    y[bc * n_spatial + to] = x[bc * n_spatial + from];
  }
}

}  // namespace
}  // namespace tio

extern "C" int tio_swap_patches(const void* x, void* y, int32_t element_bytes, int32_t batch, int32_t channels, const int32_t shape[3],
                                const int32_t patch[3], const int32_t* origins_dev, const int32_t* counts_dev, int32_t lists, int32_t s_max,
                                void* stream) {
  using namespace tio;
  const char* who = "tio_swap_patches";
  if (element_bytes != 1 && element_bytes != 2 && element_bytes != 4 && element_bytes != 8)
    return fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: elements of %d bytes (1, 2, 4 or 8)", who, element_bytes);
  if (shape == nullptr || patch == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null shape or patch", who);
  if (batch < 0 || channels < 0 || shape[0] < 0 || shape[1] < 0 || shape[2] < 0 || s_max < 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: negative size", who);
  for (int a = 0; a < 3; a++) {
    if (patch[a] < 1) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: patch size %d along axis %d (at least 1)", who, patch[a], a);
    if (patch[a] > shape[a])
      return fail(TIO_ERR_INVALID_ARGUMENT, "%s: patch (%d, %d, %d) cannot be larger than the volume (%d, %d, %d)", who, patch[0], patch[1],
                  patch[2], shape[0], shape[1], shape[2]);
  }
  if (lists != 1 && lists != batch) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: %d location lists for a batch of %d (1 or as many)", who, lists, batch);
  const int64_t limit = int64_t{1} << 40;  // (what the other entries take; every index below is int64)
  const int64_t plane = static_cast<int64_t>(shape[0]) * shape[1];
  if (plane > limit || (shape[2] > 0 && plane > limit / shape[2])) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 voxels", who);
  const int64_t n_spatial = plane * shape[2];
  const int64_t volumes = static_cast<int64_t>(batch) * channels;
  if (volumes > 0 && n_spatial > limit / volumes) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: more than 2^40 elements", who);
  const int64_t n = volumes * n_spatial;
  if (n == 0) return TIO_OK;
  if (x == nullptr || y == nullptr) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null data", who);
  const int64_t bytes = n * element_bytes;
  const uintptr_t ax = reinterpret_cast<uintptr_t>(x), ay = reinterpret_cast<uintptr_t>(y);
  if (ax < ay + bytes && ay < ax + bytes) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: the destination overlaps the source", who);
  if (ax % element_bytes != 0 || ay % element_bytes != 0) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: data not aligned to its element", who);
  if (s_max > 0 && (origins_dev == nullptr || counts_dev == nullptr)) return fail(TIO_ERR_INVALID_ARGUMENT, "%s: null origins or counts", who);
  const int64_t patch_voxels = static_cast<int64_t>(patch[0]) * patch[1] * patch[2];
  if (patch_voxels >= (int64_t{1} << 31) - 256) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: a patch of 2^31 voxels or more", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(y, x, static_cast<size_t>(bytes), hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(TIO_ERR_LAUNCH, "%s: copy failed", who);
  if (s_max == 0) return TIO_OK;
  SwapGeom g;
  for (int a = 0; a < 3; a++) g.shape[a] = shape[a], g.patch[a] = patch[a];
  g.channels = channels;
  g.lists = lists;
  g.s_max = s_max;
  g.blocks_per_box = static_cast<int32_t>((patch_voxels + 255) / 256);
  if (volumes > (int64_t{1} << 62) / (2 * static_cast<int64_t>(s_max)) / g.blocks_per_box) return fail(TIO_ERR_UNSUPPORTED_CONFIG, "%s: too many box voxels", who);
  g.tasks = volumes * s_max * 2 * g.blocks_per_box;
  const dim3 grid(static_cast<unsigned>(g.tasks < (1 << 20) ? g.tasks : (1 << 20))), block(256);
  const bool known = dispatch_element_size(element_bytes, [&](auto size) {
    using T = typename RawBits<decltype(size)::value>::type;
    hipLaunchKernelGGL(swap_gather_kernel<T>, grid, block, 0, s, static_cast<const T*>(x), static_cast<T*>(y), origins_dev, counts_dev, g);
  });
  return known ? check_launch(who) : fail(TIO_ERR_UNSUPPORTED_DTYPE, "%s: elements of %d bytes (1, 2, 4 or 8)", who, element_bytes);
}
