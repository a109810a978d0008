// The token statistics over a subset of each image's tokens (include/isic_hip_moments_ragged.h): flags on the dense grid
// (isic_token_moments_masked_f32) and offsets into a compacted store (isic_token_moments_ragged_f32), one launch each.
//
// A block of 256 threads takes one image (graph) and one slab of 64 channels, brings the n kept tokens into LDS as [n][64]
// floats and then runs csrc/token_moments.inc -- the source text of the dense kernel at W = 64, the only width it takes up
// to 256 tokens -- with the token count n.  A row therefore has the bits isic_token_moments_f32 gives for B = 1, T = n on a
// contiguous copy of the kept tokens; T and max_nodes only size the dynamic LDS.
//
//   * Masked staging.  T <= 256: thread t looks at keep[b][t].  A ballot per wave, the popcount of the lanes below for the
//     position inside the wave, the four wave totals through LDS for the wave's base: n and the ASCENDING list of kept
//     token ids (a stable compaction -- the sums follow compacted positions, not token ids).  The staging loop then reads row
//     list[i] into tile row i.  The kernel has NO static LDS of its own: at T = 196 the dense kernel's 49 KiB tile and 3.5 KiB
//     of partials fill a third of a CU's 160 KiB exactly, and one KiB more would leave two blocks per CU where the dense
//     kernel has three (measured: 1.8 x its time with every flag set).  So the four wave totals lie in the first 16 bytes of
//     the tile, which is filled only after they are read, and the list, one byte per id, lies in the tile's LAST row: with
//     n < T that row is never staged, and with n == T the list is the identity and is not used at all.
//   * Ragged staging.  The two offsets of the graph are read and compared with `total` and `max_nodes` before anything is
//     indexed with them; a bad graph adds 1 to bad[0] (an integer atomic), zeroes its count and leaves.
//   * n == 0: every thread of the block knows it after the one barrier of the compaction (masked) or from the offsets
//     (ragged), so the whole block writes its quiet NaNs and leaves together, before any further barrier.
#include "common.h"
#include "../../include/isic_hip_moments_ragged.h"

#include <limits.h>

namespace {

constexpr int BLOCK = 256;
#define MOMENTS_BLOCK 256               // token_moments.inc
constexpr int W = 64;                   // the dense kernel's slab width for T <= 256
constexpr int MAX_TILE_BYTES = ISIC_MOMENTS_RAGGED_MAX_NODES * W * (int)sizeof(float);
static_assert(MAX_TILE_BYTES == 65536 && ISIC_MOMENTS_RAGGED_MAX_NODES == BLOCK, "one thread per token, the dense kernel's tile");

struct SubsetArgs {
  const float* X;
  const uint8_t* keep;                  // masked
  const int64_t* offsets;               // ragged
  float* out;
  int32_t* counts;
  uint32_t* bad;
  int64_t ldx, ldo, total;
  int T, D, slabs, vec, max_nodes;
  float eps;
  int unbiased;
};

#include "token_moments.inc"

// the n == 0 row: six quiet NaNs per channel of the slab
__device__ __forceinline__ void write_nan_row(float* orow, int D, int d0) {
  const int c = threadIdx.x;
  if (c < W && d0 + c < D) {
    const float qnan = __uint_as_float(0x7FC00000u);
#pragma unroll
    for (int s = 0; s < 6; ++s) orow[(int64_t)s * D + d0 + c] = qnan;
  }
}

__global__ __launch_bounds__(BLOCK) void token_moments_masked_kernel(SubsetArgs a) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [T][W]; rows 0..n-1 are used
  const int tid = threadIdx.x, lane = tid % ISIC_WAVE, wave = tid / ISIC_WAVE;
  const int T = a.T;
  // no static LDS of its own (see the head of the file): the wave totals lie in the first 16 bytes of the tile, the list in
  // its last row.  The two overlap at T == 1 only, where the list is never written (n < T means n == 0).
  int* wave_total = reinterpret_cast<int*>(tile);
  uint8_t* list = reinterpret_cast<uint8_t*>(tile + (T - 1) * W);          // [256] token ids, each < T <= 256
  const int64_t b = blockIdx.x / a.slabs;
  const int slab = (int)(blockIdx.x % a.slabs), d0 = slab * W;

  // ---- n and the ascending list of kept token ids
  const bool kept = tid < T && a.keep[b * T + tid] != 0;
  const unsigned long long votes = __ballot(kept);
  if (lane == 0) wave_total[wave] = __popcll(votes);
  __syncthreads();
  int base = 0, n = 0;
#pragma unroll
  for (int w = 0; w < BLOCK / ISIC_WAVE; ++w) {
    const int c = wave_total[w];
    if (w < wave) base += c;
    n += c;
  }
  if (kept && n < T) list[base + __popcll(votes & ((1ull << lane) - 1ull))] = (uint8_t)tid;   // base + position < n < T
  if (slab == 0 && tid == 0 && a.counts) a.counts[b] = n;
  float* orow = a.out + b * a.ldo;
  if (n == 0) {                                // the same n in every thread: the block leaves together
    write_nan_row(orow, a.D, d0);
    return;
  }
  __syncthreads();                             // the list is written, the wave totals are read: the tile may be filled
  const float* xs = a.X + b * T * a.ldx + d0;
  if (n == T)                                  // every token kept: the list is the identity (and row T - 1 is staged)
    stage_rows<W>(xs, a.ldx, n, a.D, d0, a.vec, tile, [](int t) { return t; });
  else
    stage_rows<W>(xs, a.ldx, n, a.D, d0, a.vec, tile, [&](int i) { return (int)list[i]; });
  __syncthreads();
  moments_of_tile<W>(tile, n, a.D, d0, a.eps, a.unbiased, orow);
}

__global__ __launch_bounds__(BLOCK) void token_moments_ragged_kernel(SubsetArgs a) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [max_nodes][W]; rows 0..n-1 are used
  const int64_t g = blockIdx.x / a.slabs;
  const int slab = (int)(blockIdx.x % a.slabs), d0 = slab * W;
  const int64_t lo = a.offsets[g], hi = a.offsets[g + 1];
  // compared with the sizes passed by value before anything is indexed (the subtraction cannot overflow: 0 <= lo <= hi)
  if (lo < 0 || hi < lo || hi > a.total || hi - lo > (int64_t)a.max_nodes) {
    if (slab == 0 && threadIdx.x == 0) {
      atomicAdd(a.bad, 1u);
      if (a.counts) a.counts[g] = 0;
    }
    return;                                    // the same offsets in every thread: the block leaves together
  }
  const int n = (int)(hi - lo);
  if (slab == 0 && threadIdx.x == 0 && a.counts) a.counts[g] = n;
  float* orow = a.out + g * a.ldo;
  if (n == 0) {
    write_nan_row(orow, a.D, d0);
    return;
  }
  stage_rows<W>(a.X + lo * a.ldx + d0, a.ldx, n, a.D, d0, a.vec, tile, [](int t) { return t; });
  __syncthreads();
  moments_of_tile<W>(tile, n, a.D, d0, a.eps, a.unbiased, orow);
}

template <auto Kernel>
int launch_subset(const SubsetArgs& a, int64_t blocks, int rows, hipStream_t st) {
  const size_t lds = (size_t)rows * W * sizeof(float);
  return isic_launch_lds<Kernel, MAX_TILE_BYTES>(dim3((unsigned)blocks), dim3(BLOCK), lds, st, a);
}

bool aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace

extern "C" {

int isic_token_moments_masked_f32(const float* X, const uint8_t* keep, int64_t B, int T, int D, int64_t ldx, float eps,
                                  int unbiased, float* out, int64_t ldo, int32_t* counts, void* stream) {
  ISIC_CHECK_ARG(B >= 0 && T >= 1 && D >= 1 && ldx >= D && ldo >= (int64_t)6 * D);
  ISIC_CHECK_ARG(eps >= 0.f);                  // false for a NaN as well
  ISIC_CHECK_ARG(unbiased == 0 || unbiased == 1);
  ISIC_CHECK_ARG((X && out && keep) || B == 0);
  ISIC_CHECK_ARG(aligned_to(counts, 4));
  if (T > ISIC_MOMENTS_RAGGED_MAX_NODES) return ISIC_ERR_UNSUPPORTED;
  const int slabs = ceil_div(D, W);
  if (B > (int64_t)INT_MAX / slabs) return ISIC_ERR_UNSUPPORTED;
  if (B == 0) return ISIC_OK;
  SubsetArgs a = {};
  a.X = X; a.keep = keep; a.out = out; a.counts = counts; a.ldx = ldx; a.ldo = ldo; a.T = T; a.D = D; a.slabs = slabs;
  a.vec = (ldx % 4 == 0 && aligned_to(X, 16)) ? 1 : 0;
  a.eps = eps; a.unbiased = unbiased;
  return launch_subset<token_moments_masked_kernel>(a, B * slabs, T, as_stream(stream));
}

int isic_token_moments_ragged_f32(const float* X, const int64_t* node_offsets, int64_t G, int max_nodes, int64_t total,
                                  int D, int64_t ldx, float eps, int unbiased, float* out, int64_t ldo, int32_t* counts,
                                  uint32_t* bad, void* stream) {
  ISIC_CHECK_ARG(G >= 0 && max_nodes >= 0 && total >= 0 && D >= 1 && ldx >= D && ldo >= (int64_t)6 * D);
  ISIC_CHECK_ARG(eps >= 0.f);                  // false for a NaN as well
  ISIC_CHECK_ARG(unbiased == 0 || unbiased == 1);
  ISIC_CHECK_ARG(((X || total == 0) && out && node_offsets && bad) || G == 0);
  ISIC_CHECK_ARG(aligned_to(node_offsets, 8) && aligned_to(counts, 4) && aligned_to(bad, 4));
  if (max_nodes > ISIC_MOMENTS_RAGGED_MAX_NODES) return ISIC_ERR_UNSUPPORTED;
  const int slabs = ceil_div(D, W);
  if (G > (int64_t)INT_MAX / slabs) return ISIC_ERR_UNSUPPORTED;
  if (G == 0) return ISIC_OK;
  SubsetArgs a = {};
  a.X = X; a.offsets = node_offsets; a.out = out; a.counts = counts; a.bad = bad; a.ldx = ldx; a.ldo = ldo; a.total = total;
  a.D = D; a.slabs = slabs; a.max_nodes = max_nodes;
  a.vec = (ldx % 4 == 0 && aligned_to(X, 16)) ? 1 : 0;
  a.eps = eps; a.unbiased = unbiased;
  return launch_subset<token_moments_ragged_kernel>(a, G * slabs, max_nodes, as_stream(stream));
}

}  // extern "C"
