// The heterophily stage on patch graphs of unequal size (include/isic_hip_hetero_ragged.h; gfx950): the edge-wise row gather
// with LOCAL node ids and a lattice position per node, the per-graph class bookkeeping of 04_measure_heterophily.py:115-149
// with integer counters in LDS, and the order-preserving removal of the self-loop edges from the per-edge values.  lambda_2
// of the same graphs is isic_laplacian_lambda2_ragged_f64 in spectral.hip.
//
// Every value read from device memory that becomes an index (graph offsets, edge endpoints, classes, graph ids, prefix sums)
// is compared with the sizes passed by value first; what does not fit gives NaN / `bad` or is dropped, never dereferenced.
// No floating-point atomics: integer counts, one thread's fp64 finish, stable scans.
#include "common.h"
#include "edge_gather.inc"
#include "../../include/isic_hip_hetero_ragged.h"

namespace {

#include "ragged_scan.inc"                                  // RG_BLOCK, rg_block_scan

constexpr int HR_MAX_CLASSES = 64;

// the last g in [0, G) with offsets[g] <= i: zero-length segments before it share its offset and are stepped over
__device__ __forceinline__ int hr_graph_of(const int64_t* __restrict__ offsets, int G, int64_t i) {
  int lo = 0, hi = G;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// one wave per edge (as edge_hetero_kernel); every test below is wave-uniform
__global__ __launch_bounds__(256) void edge_hetero_ragged_kernel(
    const float* __restrict__ x, const float* __restrict__ probs, const int* __restrict__ dominant,
    const int* __restrict__ patch_pos, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
    const int64_t* __restrict__ edge_offsets, const int64_t* __restrict__ node_offsets, const int* __restrict__ edge_graph, int G,
    int64_t T, int64_t E, int D, int C, int grid_w, float eps, float* __restrict__ h_kl, float* __restrict__ h_dir,
    float* __restrict__ h_spatial, float* __restrict__ same_class) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  for (int64_t e = wave0; e < E; e += nwaves) {
    const int g = edge_graph ? edge_graph[e] : hr_graph_of(edge_offsets, G, e);
    bool ok = g >= 0 && g < G;
    int64_t n0 = 0, s = 0, d = 0;
    if (ok) {
      n0 = node_offsets[g];
      const int64_t n1 = node_offsets[g + 1];
      ok = edge_offsets[g] <= e && e < edge_offsets[g + 1] && n0 >= 0 && n1 >= n0 && n1 <= T;
      if (ok) {
        s = src[e];
        d = dst[e];
        ok = (uint64_t)s < (uint64_t)(n1 - n0) && (uint64_t)d < (uint64_t)(n1 - n0);
      }
    }
    if (!ok) {                                             // no row is read
      if (lane == 0) h_kl[e] = h_dir[e] = h_spatial[e] = same_class[e] = __builtin_nanf("");
      continue;
    }
    const int64_t rs = n0 + s, rd = n0 + d;
    float acc, kl;
    edge_row_sums(x + (size_t)rs * D, x + (size_t)rd * D, probs + (size_t)rs * C, probs + (size_t)rd * C, D, C, eps, lane, acc,
                  kl);
    if (lane == 0) {
      h_dir[e] = 0.5f * acc;
      h_kl[e] = kl;
      h_spatial[e] = lattice_distance(patch_pos ? patch_pos[rs] : (int)s, patch_pos ? patch_pos[rd] : (int)d, grid_w);
      same_class[e] = dominant[rs] == dominant[rd] ? 1.f : 0.f;
    }
  }
}

// one workgroup per graph: class histogram of the nodes, then the edges with src != dst counted, compared and binned
__global__ __launch_bounds__(RG_BLOCK) void graph_homophily_ragged_kernel(
    const int* __restrict__ dominant, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
    const int64_t* __restrict__ edge_offsets, const int64_t* __restrict__ node_offsets, int64_t T, int64_t E, int C,
    int64_t* __restrict__ num_edges, double* __restrict__ h_adj, double* __restrict__ expected, double* __restrict__ compat,
    uint32_t* __restrict__ bad) {
  __shared__ unsigned hist[HR_MAX_CLASSES];
  __shared__ unsigned pair[HR_MAX_CLASSES * HR_MAX_CLASSES];
  __shared__ unsigned cnt[3];                              // [0] edges with src != dst  [1] of those, same class  [2] bad input
  const int g = blockIdx.x, tid = threadIdx.x;
  double* cm = compat + (size_t)g * C * C;
  const int64_t n0 = node_offsets[g], n1 = node_offsets[g + 1], e0 = edge_offsets[g], e1 = edge_offsets[g + 1];
  const int64_t n = n1 - n0;
  int wrong = !(n0 >= 0 && n1 >= n0 && n1 <= T && e0 >= 0 && e1 >= e0 && e1 <= E);      // block-uniform
  if (!wrong) {
    for (int i = tid; i < C; i += RG_BLOCK) hist[i] = 0;
    for (int i = tid; i < C * C; i += RG_BLOCK) pair[i] = 0;
    if (tid < 3) cnt[tid] = 0;
    __syncthreads();
    int bd = 0;
    for (int64_t i = tid; i < n; i += RG_BLOCK) {
      const int c = dominant[n0 + i];
      if ((unsigned)c < (unsigned)C) atomicAdd(&hist[c], 1u);
      else bd = 1;
    }
    // every class of the graph is checked before one of them indexes the pair counts
    wrong = __syncthreads_or(bd);
  }
  if (!wrong) {
    unsigned ne = 0, same = 0;
    int bd = 0;
    for (int64_t e = e0 + tid; e < e1; e += RG_BLOCK) {
      const int64_t s = src[e], d = dst[e];
      if ((uint64_t)s >= (uint64_t)n || (uint64_t)d >= (uint64_t)n) {
        bd = 1;
        continue;
      }
      if (s == d) continue;                                // 04:115-116
      const int cs = dominant[n0 + s], cd = dominant[n0 + d];
      ++ne;
      same += cs == cd ? 1u : 0u;
      atomicAdd(&pair[cs * C + cd], 1u);
    }
    if (ne) atomicAdd(&cnt[0], ne);
    if (same) atomicAdd(&cnt[1], same);
    wrong = __syncthreads_or(bd);
  }
  if (wrong) {
    const double nan = __builtin_nan("");
    for (int i = tid; i < C * C; i += RG_BLOCK) cm[i] = nan;
    if (tid == 0) {
      num_edges[g] = 0;
      h_adj[g] = expected[g] = nan;
      bad[g] = 1u;
    }
    return;
  }
  if (tid == 0) {                                          // 04:128-139 in fp64
    const double edge_h = cnt[0] ? (double)cnt[1] / (double)cnt[0] : 0.0;
    const double nn = (double)(n > 1 ? n : 1);
    double ex = 0.0;
    for (int k = 0; k < C; ++k) {
      const double pk = (double)hist[k] / nn;
      ex += pk * pk;
    }
    num_edges[g] = (int64_t)cnt[0];
    expected[g] = ex;
    h_adj[g] = ex < 1.0 ? (edge_h - ex) / (1.0 - ex) : 1.0;
    bad[g] = 0u;
  }
  for (int r = tid; r < C; r += RG_BLOCK) {                 // 04:141-149: rows over their sums
    unsigned rsum = 0;
    for (int c = 0; c < C; ++c) rsum += pair[r * C + c];
    for (int c = 0; c < C; ++c) cm[r * C + c] = rsum ? (double)pair[r * C + c] / (double)rsum : 0.0;
  }
}

// one workgroup per graph: the edges with src != dst chunk by chunk at base + block scan (stable), M value rows each
__global__ __launch_bounds__(RG_BLOCK) void edge_values_compact_ragged_kernel(
    const float* __restrict__ values, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
    const int64_t* __restrict__ edge_offsets, const int64_t* __restrict__ kept_offsets, int M, int64_t E,
    float* __restrict__ out) {
  __shared__ int wsum[RG_WAVES];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t e0 = edge_offsets[g], e1 = edge_offsets[g + 1];
  if (!(e0 >= 0 && e1 >= e0 && e1 <= E)) return;            // block-uniform
  const int64_t k0 = kept_offsets[g], k1 = kept_offsets[g + 1];
  const int64_t lo = k0 > 0 ? k0 : 0, hi = k1 < E ? k1 : E;  // the graph's own output segment, inside the arrays
  int64_t base = k0;
  for (int64_t c0 = e0; c0 < e1; c0 += RG_BLOCK) {          // block-uniform trip count
    const int64_t e = c0 + tid;
    const bool flag = e < e1 && src[e] != dst[e];
    int total;
    const int64_t p = base + rg_block_scan(flag, wsum, total);
    if (flag && p >= lo && p < hi)
      for (int m = 0; m < M; ++m) out[(size_t)m * E + p] = values[(size_t)m * E + e];
    base += total;
  }
}

}  // namespace

extern "C" {

int isic_edge_heterophily_ragged_f32(const float* x, const float* probs, const int32_t* dominant_class,
                                     const int32_t* patch_pos, const int64_t* src, const int64_t* dst,
                                     const int64_t* edge_offsets, const int64_t* node_offsets, const int32_t* edge_graph, int G,
                                     int64_t T, int64_t E, int D, int C, int grid_w, float eps, float* h_kl,
                                     float* h_dirichlet, float* h_spatial, float* same_class, void* stream) {
  ISIC_CHECK_ARG(G >= 0 && T >= 0 && E >= 0 && D > 0 && C > 0 && grid_w > 0);
  if (G == 0) return ISIC_OK;
  ISIC_CHECK_ARG(edge_offsets && node_offsets);
  ISIC_CHECK_ARG(E == 0 || (src && dst && h_kl && h_dirichlet && h_spatial && same_class));
  ISIC_CHECK_ARG(T == 0 || (x && probs && dominant_class));
  if (T >= 0x80000000LL || E >= 0x80000000LL) return ISIC_ERR_UNSUPPORTED;
  if (E == 0) return ISIC_OK;
  int64_t blocks = (E + 3) / 4;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(edge_hetero_ragged_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, probs,
                     dominant_class, patch_pos, src, dst, edge_offsets, node_offsets, edge_graph, G, T, E, D, C, grid_w, eps, h_kl,
                     h_dirichlet, h_spatial, same_class);
  return isic_launch_status();
}

int isic_graph_homophily_ragged(const int32_t* dominant_class, const int64_t* src, const int64_t* dst,
                                const int64_t* edge_offsets, const int64_t* node_offsets, int G, int64_t T, int64_t E, int C,
                                int64_t* num_edges, double* h_adj, double* expected, double* compat, uint32_t* bad,
                                void* stream) {
  ISIC_CHECK_ARG(G >= 0 && T >= 0 && E >= 0 && C > 0);
  if (G == 0) return ISIC_OK;
  ISIC_CHECK_ARG(edge_offsets && node_offsets && num_edges && h_adj && expected && compat && bad);
  ISIC_CHECK_ARG(E == 0 || (src && dst));
  ISIC_CHECK_ARG(T == 0 || dominant_class);
  if (C > HR_MAX_CLASSES || T >= 0x80000000LL || E >= 0x80000000LL) return ISIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(graph_homophily_ragged_kernel, dim3((unsigned)G), dim3(RG_BLOCK), 0, as_stream(stream), dominant_class,
                     src, dst, edge_offsets, node_offsets, T, E, C, num_edges, h_adj, expected, compat, bad);
  return isic_launch_status();
}

int isic_edge_values_compact_ragged_f32(const float* values, const int64_t* src, const int64_t* dst,
                                        const int64_t* edge_offsets, const int64_t* kept_offsets, int G, int M, int64_t E,
                                        float* out, void* stream) {
  ISIC_CHECK_ARG(G >= 0 && M >= 0 && E >= 0);
  if (G == 0) return ISIC_OK;
  ISIC_CHECK_ARG(edge_offsets && kept_offsets);
  ISIC_CHECK_ARG(E == 0 || (src && dst));
  ISIC_CHECK_ARG((int64_t)M * E == 0 || (values && out));
  if (E >= 0x80000000LL) return ISIC_ERR_UNSUPPORTED;
  if ((int64_t)M * E == 0) return ISIC_OK;
  hipLaunchKernelGGL(edge_values_compact_ragged_kernel, dim3((unsigned)G), dim3(RG_BLOCK), 0, as_stream(stream), values, src,
                     dst, edge_offsets, kept_offsets, M, E, out);
  return isic_launch_status();
}

}  // extern "C"
