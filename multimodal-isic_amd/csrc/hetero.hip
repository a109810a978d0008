// Edge-wise heterophily measures of a patch graph (gfx950): per directed edge (src -> dst)
//   H_kl        = sum_c p[src,c] * log((p[src,c] + eps) / (p[dst,c] + eps))        (04_measure_heterophily.py:164)
//   H_dirichlet = 0.5 * || x[src] - x[dst] ||^2                                     (:165)
//   H_spatial   = Euclidean distance of the two patches on the grid_w-wide lattice  (:124-125,166)
//   same_class  = dominant_class[src] == dominant_class[dst]                        (:130)
// HBM-bound row gather: one wave per edge, both embedding rows read with 16-byte loads (D floats each), squared
// difference reduced across the 64 lanes; the class-probability rows (C <= 64) ride on the first lanes.
// Self loops are NOT dropped here (the reference strips them, :117-118): the host filters on src != dst so that
// the surviving values keep the reference's edge order.  The gather itself is edge_gather.inc, shared with the kernel for
// graphs of unequal size (hetero_ragged.hip).
#include "common.h"
#include "edge_gather.inc"

namespace {

__global__ __launch_bounds__(256) void edge_hetero_kernel(const float* __restrict__ x, const float* __restrict__ probs,
                                                          const int* __restrict__ dominant, const int64_t* __restrict__ src,
                                                          const int64_t* __restrict__ dst, int64_t E, int D, int C, int grid_w,
                                                          int nodes_per_graph, float eps, float* __restrict__ h_kl,
                                                          float* __restrict__ h_dir, float* __restrict__ h_spatial,
                                                          float* __restrict__ same_class) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  for (int64_t e = wave0; e < E; e += nwaves) {
    const int64_t s = src[e], d = dst[e];
    float acc, kl;
    edge_row_sums(x + (size_t)s * D, x + (size_t)d * D, probs + (size_t)s * C, probs + (size_t)d * C, D, C, eps, lane, acc, kl);
    if (lane == 0) {
      h_dir[e] = 0.5f * acc;
      h_kl[e] = kl;
      // lattice coordinates of the node inside ITS graph (04:124-125 uses % 14 and // 14 of the local index)
      h_spatial[e] = lattice_distance((int)(s % nodes_per_graph), (int)(d % nodes_per_graph), grid_w);
      same_class[e] = dominant[s] == dominant[d] ? 1.f : 0.f;
    }
  }
}

}  // namespace

extern "C" {

int isic_edge_heterophily_f32(const float* x, const float* probs, const int32_t* dominant_class, const int64_t* src,
                              const int64_t* dst, int64_t num_edges, int D, int C, int grid_w, int nodes_per_graph,
                              float eps, float* h_kl, float* h_dirichlet, float* h_spatial, float* same_class,
                              void* stream) {
  ISIC_CHECK_ARG(num_edges >= 0 && D > 0 && C > 0 && grid_w > 0 && nodes_per_graph > 0);
  if (num_edges == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && probs && dominant_class && src && dst && h_kl && h_dirichlet && h_spatial && same_class);
  int64_t blocks = (num_edges + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(edge_hetero_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, probs, dominant_class,
                     src, dst, num_edges, D, C, grid_w, nodes_per_graph, eps, h_kl, h_dirichlet, h_spatial, same_class);
  return isic_launch_status();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------
// Lesion-mask -> patch flags (save_latent.py:73-87): flags[b, i, j] = 1 iff the P x P pixel block (i, j) of mask b
// holds any value > 0.  One wave per patch; lanes stride the block's pixels; a ballot reduces.
namespace {

__global__ __launch_bounds__(256) void mask_patch_flags_kernel(const float* __restrict__ mask, unsigned char* __restrict__ flags,
                                                               int64_t B, int H, int W, int P) {
  const int lane = threadIdx.x & 63;
  const int gh = H / P, gw = W / P;
  const int64_t total = B * gh * gw;
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < total; w += (int64_t)gridDim.x * 4) {
    const int64_t b = w / (gh * gw);
    const int r = (int)(w - b * (gh * gw));
    const int pi = r / gw, pj = r - pi * gw;
    const float* base = mask + (b * H + (int64_t)pi * P) * W + (int64_t)pj * P;
    bool any = false;
    for (int t = lane; t < P * P; t += 64) any |= base[(int64_t)(t / P) * W + (t % P)] > 0.f;
    const unsigned long long bal = __ballot(any);
    if (lane == 0) flags[w] = bal != 0ull ? 1 : 0;
  }
}

}  // namespace

extern "C" int isic_mask_patch_flags_f32(const float* mask, uint8_t* flags, int64_t B, int H, int W, int patch, void* stream) {
  ISIC_CHECK_ARG(B >= 0 && H > 0 && W > 0 && patch > 0 && H % patch == 0 && W % patch == 0);
  if (B == 0) return ISIC_OK;
  ISIC_CHECK_ARG(mask && flags);
  int64_t blocks = (B * (H / patch) * (W / patch) + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(mask_patch_flags_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), mask, flags, B, H, W,
                     patch);
  return isic_launch_status();
}
