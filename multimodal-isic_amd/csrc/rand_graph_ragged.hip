// The reference's random patch graphs for a batch of graphs of UNEQUAL size (include/isic_hip_randgraph_ragged.h): count, then
// write, each graph with its own node count, clamp and seed.  The stream, the draws, Fisher-Yates and the bitmap enumeration
// are csrc/rand_graph.inc, the text isic_random_graph_i64 runs.
//
// Lanes and LDS follow the graph.  Two size classes, one launch each (the second only when max_nodes > PACK_NODES):
//   * n <= 64: a WAVE per graph, four graphs to a 256-lane workgroup, each wave with its own MT state (5 KB), bitmap, draw
//     bytes and permutation columns (sized by min(max_nodes, 64)).  The waves share nothing and never meet at a
//     __syncthreads(): a wave whose graph is empty, bad or of the other class simply returns, and seeding chains and
//     regenerations of different length run side by side.
//   * 64 < n <= max_nodes: a 256-lane workgroup per graph.  The whole workgroup takes the same graph, so every
//     __syncthreads() is reached by all of it or (a graph of the other class, a bad graph) by none.
// Both calls regenerate the graph; _count stops at the row counts.  Nothing read from device memory is used as an index
// before it is compared with a size passed by value: a graph's offsets against node_offsets[G] and max_nodes, a segment
// against `total` and the graph's own edge count (so a write position is < the segment's length).
#include "rand_graph.inc"
#include "../../include/isic_hip_randgraph_ragged.h"

namespace {

using namespace randgraph;

constexpr int BLOCK = 256;
constexpr int MAX_N = ISIC_RANDGRAPH_RAGGED_MAX_NODES;
constexpr int MAX_LIST = ISIC_RANDGRAPH_RAGGED_MAX_R_VALUES;
constexpr int PACK_N = ISIC_RANDGRAPH_RAGGED_PACK_NODES;
static_assert(PACK_N == ISIC_WAVE && MAX_N <= BLOCK && MAX_N <= 256, "one node per lane, node ids and draws in a byte");
static_assert(graph_lds_bytes(MAX_N, MAX_N - 2) + 2 * MT_N * 4 + 64 <= 160 * 1024, "LDS of a gfx950 workgroup");
static_assert((BLOCK / PACK_N) * (graph_lds_bytes(PACK_N, PACK_N - 2) + 2 * MT_N * 4) <= 64 * 1024, "the packed class needs no opt-in");

struct RaggedArgs {
  const int64_t* seeds;
  const int64_t* node_off;       // [G+1]
  int64_t* counts;               // _count: [n_r][G]
  const int64_t* edge_off;       // _write: [n_r][G+1]
  int64_t* src;
  int64_t* dst;
  unsigned* bad;
  int64_t total;
  int G, max_nodes, n_r, global_ids;
  int n_above, n_upto;           // this launch's class: n_above < n <= n_upto
  int first;                     // the class that also answers for bad graphs
  unsigned group_words;          // dynamic LDS words of one group
  // in ASCENDING order (ties in the caller's order), each at least 1; the kernel clamps by the graph's own n - 1:
  int r[MAX_LIST];
  int slot[MAX_LIST];            // index in the caller's list
};

// Does the segment [s0, s1) of pair (j, g) lie in [0, total] with exactly `count` slots?
__device__ __forceinline__ bool segment_fits(const RaggedArgs& a, int j, int64_t g, int64_t count, int64_t& s0) {
  const int64_t* row = a.edge_off + (size_t)a.slot[j] * ((size_t)a.G + 1);
  s0 = row[g];
  const int64_t s1 = row[g + 1];
  return s0 >= 0 && s1 >= s0 && s1 <= a.total && s1 - s0 == count;
}

template <int LANES, bool WRITE>
__global__ __launch_bounds__(BLOCK) void rand_graph_ragged_kernel(RaggedArgs a) {
  constexpr int GROUPS = BLOCK / LANES;
  __shared__ unsigned st[GROUPS][2][MT_N];
  __shared__ int wave_total[BLOCK / ISIC_WAVE];
  extern __shared__ unsigned dyn[];
  const int grp = threadIdx.x / LANES, lane = threadIdx.x % LANES;
  const int64_t g = (int64_t)blockIdx.x * GROUPS + grp;
  if (g >= a.G) return;                                                 // (uniform over the group, as every return below)
  const int64_t lo = a.node_off[g], hi = a.node_off[g + 1], T = a.node_off[a.G];
  if (lo < 0 || hi < lo || hi > T || hi - lo > a.max_nodes) {           // a bad graph: count 0, nothing written
    if (a.first) {
      if (!WRITE && lane < a.n_r) a.counts[(size_t)lane * a.G + g] = 0;
      if (lane == 0) atomicAdd(a.bad, 1u);
    }
    return;
  }
  const int n = (int)(hi - lo);
  if (n <= a.n_above || n > a.n_upto) return;
  if (n < 2) {                                                          // no edges (n_above < 0: the packed class)
    if (lane < a.n_r) {
      int64_t s0;
      if (!WRITE) a.counts[(size_t)lane * a.G + g] = 0;
      else if (!segment_fits(a, lane, g, 0, s0)) atomicAdd(a.bad, 1u);
    }
    return;
  }
  const int m = n - 1;
  const int r_top = a.r[a.n_r - 1] < m ? a.r[a.n_r - 1] : m;
  const int S = r_top < m - 1 ? r_top : m - 1;
  const int RW = (n + 31) >> 5;
  unsigned* bm = dyn + (size_t)grp * a.group_words;                     // [RW][n]
  unsigned char* zs = reinterpret_cast<unsigned char*>(bm + RW * n);    // [S][n]
  unsigned char* p = zs + round4((size_t)n * S);                        // [m][n]

  generate<LANES>(st[grp], bm, zs, p, lane, (unsigned)((unsigned long long)a.seeds[g] & 0xFFFFFFFFull), n, S, graph_regens(n, S));

  const int64_t add = a.global_ids ? lo : 0;
  int r_prev = 0;
  for (int j = 0; j < a.n_r; ++j) {
    const int r = a.r[j] < m ? a.r[j] : m;                              // 03:61, by the graph's own node count
    add_targets(bm, p, lane, n, r_prev, r);
    r_prev = r > r_prev ? r : r_prev;
    group_sync<LANES>();
    int pos, total;
    place_rows<LANES>(bm, lane, n, wave_total, pos, total);
    if (!WRITE) {
      if (lane == 0) a.counts[(size_t)a.slot[j] * a.G + g] = total;
    } else {
      int64_t s0;
      if (segment_fits(a, j, g, total, s0)) write_rows(bm, lane, n, pos, total, a.src + s0, a.dst + s0, add);
      else if (lane == 0) atomicAdd(a.bad, 1u);
    }
    group_sync<LANES>();                                                // wave_total and the bitmap are reused
  }
}

template <bool WRITE>
int launch(RaggedArgs a, hipStream_t st) {
  const int r_top = a.r[a.n_r - 1];
  auto class_words = [&](int nmax) -> unsigned {
    if (nmax < 2) return 0u;
    const int m = nmax - 1, rt = r_top < m ? r_top : m;
    return (unsigned)(graph_lds_bytes(nmax, rt < m - 1 ? rt : m - 1) / 4);
  };
  // graphs of up to PACK_N nodes (and the bad ones): a wave each
  constexpr int GROUPS = BLOCK / PACK_N;
  a.n_above = -1;
  a.n_upto = PACK_N;
  a.first = 1;
  a.group_words = class_words(a.max_nodes < PACK_N ? a.max_nodes : PACK_N);
  hipLaunchKernelGGL((rand_graph_ragged_kernel<PACK_N, WRITE>), dim3((unsigned)ceil_div64(a.G, GROUPS)), dim3(BLOCK),
                     (size_t)GROUPS * a.group_words * 4, st, a);
  if (isic_launch_status() != ISIC_OK) return ISIC_ERR_LAUNCH;
  if (a.max_nodes <= PACK_N) return ISIC_OK;
  // larger graphs: a workgroup each
  a.n_above = PACK_N;
  a.n_upto = a.max_nodes;
  a.first = 0;
  a.group_words = class_words(a.max_nodes);
  return isic_launch_lds<rand_graph_ragged_kernel<BLOCK, WRITE>, (int)graph_lds_bytes(MAX_N, MAX_N - 2)>(
      dim3((unsigned)a.G), dim3(BLOCK), (size_t)a.group_words * 4, st, a);
}

// the r list in ascending order, each value at least 1 and at most MAX_N (a larger one clamps to n - 1 anyway)
void sort_r(const int* r_values, int n_r, RaggedArgs& a) {
  for (int j = 0; j < n_r; ++j) {
    const int r = r_values[j] < 1 ? 1 : (r_values[j] > MAX_N ? MAX_N : r_values[j]);
    int k = j;                                                          // stable insertion
    while (k > 0 && a.r[k - 1] > r) { a.r[k] = a.r[k - 1]; a.slot[k] = a.slot[k - 1]; --k; }
    a.r[k] = r;
    a.slot[k] = j;
  }
  for (int k = n_r; k < MAX_LIST; ++k) { a.r[k] = 0; a.slot[k] = 0; }
}

inline bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

}  // namespace

extern "C" {

int isic_random_graph_ragged_count(const int64_t* seeds, const int64_t* node_offsets, int G, int max_nodes,
                                   const int* r_values, int n_r, int64_t* counts, uint32_t* bad, void* stream) {
  ISIC_CHECK_ARG(r_values && G >= 0 && max_nodes >= 0 && ((seeds && node_offsets && counts && bad) || G == 0));
  ISIC_CHECK_ARG(!misaligned(seeds, 7) && !misaligned(node_offsets, 7) && !misaligned(counts, 7) && !misaligned(bad, 3));
  if (max_nodes > MAX_N || n_r > MAX_LIST || n_r < 1) return ISIC_ERR_UNSUPPORTED;
  if (G == 0) return ISIC_OK;
  RaggedArgs a = {};
  a.seeds = seeds; a.node_off = node_offsets; a.counts = counts; a.bad = bad;
  a.G = G; a.max_nodes = max_nodes; a.n_r = n_r;
  sort_r(r_values, n_r, a);
  return launch<false>(a, as_stream(stream));
}

int isic_random_graph_ragged_write(const int64_t* seeds, const int64_t* node_offsets, int G, int max_nodes,
                                   const int* r_values, int n_r, const int64_t* edge_off, int64_t total, int global_ids,
                                   int64_t* src, int64_t* dst, uint32_t* bad, void* stream) {
  ISIC_CHECK_ARG(r_values && G >= 0 && max_nodes >= 0 && total >= 0);
  ISIC_CHECK_ARG((seeds && node_offsets && edge_off && bad && ((src && dst) || total == 0)) || G == 0);
  ISIC_CHECK_ARG(!misaligned(seeds, 7) && !misaligned(node_offsets, 7) && !misaligned(edge_off, 7) && !misaligned(src, 7) &&
                 !misaligned(dst, 7) && !misaligned(bad, 3));
  if (max_nodes > MAX_N || n_r > MAX_LIST || n_r < 1) return ISIC_ERR_UNSUPPORTED;
  if (G == 0) return ISIC_OK;
  RaggedArgs a = {};
  a.seeds = seeds; a.node_off = node_offsets; a.edge_off = edge_off; a.src = src; a.dst = dst; a.bad = bad;
  a.total = total; a.G = G; a.max_nodes = max_nodes; a.n_r = n_r; a.global_ids = global_ids ? 1 : 0;
  sort_r(r_values, n_r, a);
  return launch<true>(a, as_stream(stream));
}

}  // extern "C"
