// The random patch graphs of 03_build_graphs.py:57-78 on the device, bit for bit (include/isic_hip_randgraph.h states the
// definition): one workgroup of 256 lanes per graph, every r value of the list from one pass over the random stream.
// The stream, the draws, Fisher-Yates and the bitmap enumeration are csrc/rand_graph.inc (which describes them), shared with
// the build for graphs of unequal size (csrc/rand_graph_ragged.hip); here the group is the whole workgroup.
// Bounds: a target is p + (p >= i) <= n - 1 and never i, so a graph has at most min(2 n r, n (n - 1)) = cap edges; the
// write loop is fenced by cap all the same.
#include "rand_graph.inc"
#include "../../include/isic_hip_randgraph.h"

namespace {

using namespace randgraph;

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / ISIC_WAVE;
constexpr int MAX_N = ISIC_RANDGRAPH_MAX_NODES;
constexpr int MAX_LIST = ISIC_RANDGRAPH_MAX_R_VALUES;
static_assert(MAX_N <= BLOCK && MAX_N <= 256, "one node per lane, node ids and draws in a byte");

// bitmap words + draw bytes + permutation bytes at n = MAX_N, r = n - 1
constexpr size_t MAX_DYN_LDS = graph_lds_bytes(MAX_N, MAX_N - 2);
static_assert(MAX_DYN_LDS + 2 * MT_N * 4 + 64 <= 160 * 1024, "LDS of a gfx950 workgroup");

struct RandGraphArgs {
  const int64_t* seeds;
  int64_t* edges;
  int32_t* counts;
  int G, n, n_r;
  int swaps;                     // S
  int regens;                    // state regenerations that hold a used word
  unsigned z_bytes;              // round4(n S)
  // in ASCENDING order of the clamped r (ties in the caller's order):
  int r[MAX_LIST];               // clamped
  int slot[MAX_LIST];            // index in the caller's list (row of counts)
  int cap[MAX_LIST];
  int64_t base[MAX_LIST];        // first element of the r value's block in edges
};

__global__ __launch_bounds__(BLOCK) void rand_graph_kernel(RandGraphArgs a) {
  __shared__ unsigned st[2][MT_N];
  __shared__ int wave_total[WAVES];
  extern __shared__ unsigned dyn[];
  const int tid = threadIdx.x, g = blockIdx.x;
  const int n = a.n;
  const int RW = (n + 31) >> 5;
  unsigned* bm = dyn;                                                   // [RW][n]
  unsigned char* zs = reinterpret_cast<unsigned char*>(dyn + RW * n);   // [S][n]
  unsigned char* p = zs + a.z_bytes;                                    // [m][n]

  generate<BLOCK>(st, bm, zs, p, tid, (unsigned)((unsigned long long)a.seeds[g] & 0xFFFFFFFFull), n, a.swaps, a.regens);

  int r_prev = 0;
  for (int j = 0; j < a.n_r; ++j) {
    const int r = a.r[j], cap = a.cap[j];
    add_targets(bm, p, tid, n, r_prev, r);
    r_prev = r > r_prev ? r : r_prev;
    __syncthreads();
    int pos, total;
    place_rows<BLOCK>(bm, tid, n, wave_total, pos, total);
    int64_t* src = a.edges + a.base[j] + (int64_t)g * 2 * cap;
    write_rows(bm, tid, n, pos, cap, src, src + cap, 0);
    if (tid == 0) a.counts[(size_t)a.slot[j] * a.G + g] = total < cap ? total : cap;
    __syncthreads();                                                    // wave_total and the bitmap are reused
  }
}

__global__ void rand_graph_zero_counts_kernel(int32_t* counts, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) counts[i] = 0;
}

}  // namespace

extern "C" {

int isic_random_graph_i64(const int64_t* seeds, int G, int n_nodes, const int* r_values, int n_r, int64_t* edges,
                          int32_t* counts, void* stream) {
  ISIC_CHECK_ARG(r_values && G >= 0 && n_nodes >= 0 && ((seeds && edges && counts) || G == 0));
  ISIC_CHECK_ARG(!(reinterpret_cast<uintptr_t>(seeds) & 7) && !(reinterpret_cast<uintptr_t>(edges) & 7) &&
                 !(reinterpret_cast<uintptr_t>(counts) & 3));
  if (n_nodes > MAX_N || n_r > MAX_LIST || n_r < 1) return ISIC_ERR_UNSUPPORTED;
  if (G == 0) return ISIC_OK;
  hipStream_t st = as_stream(stream);
  if (n_nodes < 2) {
    const int64_t count = (int64_t)n_r * G;
    hipLaunchKernelGGL(rand_graph_zero_counts_kernel, dim3((unsigned)ceil_div64(count, BLOCK)), dim3(BLOCK), 0, st, counts, count);
    return isic_launch_status();
  }
  const int n = n_nodes, m = n - 1;
  RandGraphArgs a;
  a.seeds = seeds; a.edges = edges; a.counts = counts; a.G = G; a.n = n; a.n_r = n_r;
  int clamped[MAX_LIST], order[MAX_LIST];
  int64_t base[MAX_LIST], at = 0;
  int r_max = 1;
  for (int j = 0; j < n_r; ++j) {
    const int r = r_values[j] < 1 ? 1 : (r_values[j] > m ? m : r_values[j]);                 // 03:60
    clamped[j] = r;
    r_max = r > r_max ? r : r_max;
    const int64_t cap = 2 * (int64_t)n * r < (int64_t)n * m ? 2 * (int64_t)n * r : (int64_t)n * m;
    base[j] = at;
    at += 2 * (int64_t)G * cap;
    int k = j;                                                                                 // stable insertion
    while (k > 0 && clamped[order[k - 1]] > r) { order[k] = order[k - 1]; --k; }
    order[k] = j;
  }
  for (int k = 0; k < n_r; ++k) {
    const int j = order[k], r = clamped[j];
    a.r[k] = r; a.slot[k] = j; a.base[k] = base[j];
    a.cap[k] = 2 * n * r < n * m ? 2 * n * r : n * m;
  }
  for (int k = n_r; k < MAX_LIST; ++k) { a.r[k] = 0; a.slot[k] = 0; a.cap[k] = 0; a.base[k] = 0; }
  a.swaps = r_max < m - 1 ? r_max : m - 1;
  a.regens = graph_regens(n, a.swaps);
  a.z_bytes = (unsigned)round4((size_t)n * a.swaps);
  const size_t lds = graph_lds_bytes(n, a.swaps);
  return isic_launch_lds<rand_graph_kernel, (int)MAX_DYN_LDS>(dim3((unsigned)G), dim3(BLOCK), lds, st, a);
}

}  // extern "C"
