// Per-image statistics of a token grid over its token axis (include/isic_hip_moments.h): mean, max, std, median, skewness
// and excess kurtosis of X[b, 0:T, d] for every (b, d), in one launch.  Replaces the eight or so torch passes (one of them a
// full sort per column) of the reference's concat_patch_moments (utils.py:16-31).
//
//   * Tile.  Block (b, slab) stages X[b, 0:T, slab] into LDS as [T][W] floats, W = 64 / 32 / 16 by T so that the tile is
//     at most 64 KiB.  Thread (g, c) = (tid / W, tid % W) owns channel c of the slab and the tokens g, g + G, ... with
//     G = 256 / W.  A wave reads 64 consecutive floats of the tile per instruction (one row at W = 64, two at 32, four at
//     16): no bank conflict.  Channels past D are staged as zeros and never written out.
//   * Moments and median.  What happens once the slab is staged -- the two walks, the partial sums meeting in ascending
//     thread order, the radix-select median and the epilogue -- is csrc/token_moments.inc, the source text the masked and
//     ragged entries (token_moments_ragged.hip) run as well, here with the runtime token count T.
#include "common.h"
#include "../../include/isic_hip_moments.h"

#include <limits.h>

namespace {

constexpr int BLOCK = 256;
#define MOMENTS_BLOCK 256               // token_moments.inc
constexpr int MAX_TILE_BYTES = 65536;

struct MomentsArgs {
  const float* X;
  float* out;
  int64_t ldx, ldo;
  int T, D, slabs, vec;
  float eps;
  int unbiased;
};

#include "token_moments.inc"

template <int W>
__global__ __launch_bounds__(BLOCK) void token_moments_kernel(MomentsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [T][W]
  const int T = a.T;
  const int64_t b = blockIdx.x / a.slabs;
  const int d0 = (int)(blockIdx.x % a.slabs) * W;
  // ---- stage the slab: X is read here and nowhere else
  stage_rows<W>(a.X + b * T * a.ldx + d0, a.ldx, T, a.D, d0, a.vec, tile, [](int t) { return t; });
  __syncthreads();
  moments_of_tile<W>(tile, T, a.D, d0, a.eps, a.unbiased, a.out + b * a.ldo);
}

int slab_width(int T) { return T <= 256 ? 64 : (T <= 512 ? 32 : 16); }

template <int W>
int launch_moments(const MomentsArgs& a, int64_t blocks, hipStream_t st) {
  const size_t lds = (size_t)a.T * W * sizeof(float);
  return isic_launch_lds<token_moments_kernel<W>, MAX_TILE_BYTES>(dim3((unsigned)blocks), dim3(BLOCK), lds, st, a);
}

}  // namespace

extern "C" {

int isic_token_moments_f32(const float* X, int64_t B, int T, int D, int64_t ldx, float eps, int unbiased, float* out,
                           int64_t ldo, void* stream) {
  ISIC_CHECK_ARG(B >= 0 && T >= 1 && D >= 1 && ldx >= D && ldo >= (int64_t)6 * D);
  ISIC_CHECK_ARG(eps >= 0.f);                  // false for a NaN as well
  ISIC_CHECK_ARG((unbiased == 0 || unbiased == 1) && !(unbiased && T < 2));
  ISIC_CHECK_ARG((X && out) || B == 0);
  if (T > ISIC_MOMENTS_MAX_T) return ISIC_ERR_UNSUPPORTED;
  const int W = slab_width(T);
  const int slabs = ceil_div(D, W);
  if (B > (int64_t)INT_MAX / slabs) return ISIC_ERR_UNSUPPORTED;
  if (B == 0) return ISIC_OK;
  MomentsArgs a;
  a.X = X; a.out = out; a.ldx = ldx; a.ldo = ldo; a.T = T; a.D = D; a.slabs = slabs;
  a.vec = (ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0) ? 1 : 0;
  a.eps = eps; a.unbiased = unbiased;
  const int64_t blocks = B * slabs;
  hipStream_t st = as_stream(stream);
  switch (W) {
    case 64: return launch_moments<64>(a, blocks, st);
    case 32: return launch_moments<32>(a, blocks, st);
    default: return launch_moments<16>(a, blocks, st);
  }
}

}  // extern "C"
