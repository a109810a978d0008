// The random patch graphs of 03_build_graphs.py:57-78 on the device, bit for bit (include/isic_hip_randgraph.h states the
// definition): one workgroup of 256 lanes per graph, every r value of the list from one pass over the random stream.
//
//   * Stream.  MT19937 in LDS, double-buffered: a regeneration reads the old 624 words from one buffer and writes the new
//     ones into the other, so a lane never overwrites a word another lane still has to read.  Word k mixes old[k], old[k+1]
//     and word (k + 397) % 624, which is OLD for k < 227 and NEW (word k - 227) after; a lane-parallel phase is valid only
//     among words whose new source is already written, hence three phases with a barrier after each: 0..226, 227..453
//     (new 0..226), 454..622 (new 227..395), and in the last phase one more lane forms word 623 from old[623], new[0] and
//     new[396].  One lane seeds (init_genrand is a chain).
//   * Draws.  Node i owns words [i W, (i + 1) W), W = n - 2, and uses the first S = min(max r, n - 2) of them.  After a
//     regeneration lane l looks at words l, l + 256, l + 512 of the block; (node, step) of each of its three slots advances
//     by 624 words per block without a division.  A used word is tempered and reduced at once: z = word % (m - t) < 256 is
//     kept as ONE BYTE, zs[t][node].  The next regeneration's first phase writes the buffer nobody reads any more, so the
//     draws need no barrier of their own.
//   * Fisher-Yates, one node per lane, on byte columns p[.][node] in LDS (n (n - 1) bytes: 65 KB at n = 256): S swaps.
//   * For the r values in ascending order: the target columns [r_prev, r) are OR-ed into the symmetric adjacency bitmap
//     (LDS, word w of row i at bm[w n + i]), then lane i counts row i, a block-wide prefix sum places the row, and the
//     lane writes its (src, dst) pairs in ascending bit order.  The bitmap only grows, which is the prefix property.
// Bounds: a target is p + (p >= i) <= n - 1 and never i, so a graph has at most min(2 n r, n (n - 1)) = cap edges; the
// write loop is fenced by cap all the same.
#include "common.h"
#include "../../include/isic_hip_randgraph.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / ISIC_WAVE;
constexpr int MT_N = 624, MT_M = 397, MT_D = MT_N - MT_M;      // 227
constexpr int MAX_N = ISIC_RANDGRAPH_MAX_NODES;
constexpr int MAX_LIST = ISIC_RANDGRAPH_MAX_R_VALUES;
constexpr int SLOTS = (MT_N + BLOCK - 1) / BLOCK;              // words of a block one lane looks at
static_assert(MT_D <= BLOCK && MT_N - 1 - 2 * MT_D + 1 <= BLOCK, "one word per lane and phase");
static_assert(MAX_N <= BLOCK && MAX_N <= 256, "one node per lane, node ids and draws in a byte");

constexpr size_t round4(size_t b) { return (b + 3) & ~(size_t)3; }
// bitmap words + draw bytes + permutation bytes at n = MAX_N, r = n - 1
constexpr size_t MAX_DYN_LDS = (size_t)MAX_N * ((MAX_N + 31) / 32) * 4 + round4((size_t)MAX_N * (MAX_N - 2)) +
                               round4((size_t)MAX_N * (MAX_N - 1));
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

__device__ __forceinline__ unsigned mt_mix(unsigned cur, unsigned nxt, unsigned src) {
  const unsigned y = (cur & 0x80000000u) | (nxt & 0x7FFFFFFFu);
  return src ^ (y >> 1) ^ ((y & 1u) ? 0x9908B0DFu : 0u);
}
__device__ __forceinline__ unsigned mt_temper(unsigned y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9D2C5680u;
  y ^= (y << 15) & 0xEFC60000u;
  y ^= y >> 18;
  return y;
}

__global__ __launch_bounds__(BLOCK) void rand_graph_kernel(RandGraphArgs a) {
  __shared__ unsigned st[2][MT_N];
  __shared__ int wave_total[WAVES];
  extern __shared__ unsigned dyn[];
  const int tid = threadIdx.x, g = blockIdx.x;
  const int n = a.n, m = n - 1, W = m - 1, S = a.swaps;
  const int RW = (n + 31) >> 5;
  unsigned* bm = dyn;                                                   // [RW][n]
  unsigned char* zs = reinterpret_cast<unsigned char*>(dyn + RW * n);   // [S][n]
  unsigned char* p = zs + a.z_bytes;                                    // [m][n]

  if (tid == 0) {
    unsigned s = (unsigned)((unsigned long long)a.seeds[g] & 0xFFFFFFFFull);
    st[0][0] = s;
    for (int j = 1; j < MT_N; ++j) {
      s = 1812433253u * (s ^ (s >> 30)) + (unsigned)j;
      st[0][j] = s;
    }
  }
  for (int e = tid; e < RW * n; e += BLOCK) bm[e] = 0u;
  if (tid < n)
    for (int t = 0; t < m; ++t) p[t * n + tid] = (unsigned char)t;

  // (node, step) of the words this lane looks at in the current block, and the advance per block
  int node[SLOTS] = {}, step[SLOTS] = {};
  int adv_node = 0, adv_step = 0;
  if (W > 0) {
    adv_node = MT_N / W;
    adv_step = MT_N - adv_node * W;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int k = tid + s * BLOCK;
      node[s] = k / W;
      step[s] = k - node[s] * W;
    }
  }
  __syncthreads();

  int cur = 0;
  for (int b = 0; b < a.regens; ++b) {
    const unsigned* o = st[cur];
    unsigned* nw = st[cur ^ 1];
    if (tid < MT_D) nw[tid] = mt_mix(o[tid], o[tid + 1], o[tid + MT_M]);
    __syncthreads();
    if (tid < MT_D) {
      const int k = MT_D + tid;
      nw[k] = mt_mix(o[k], o[k + 1], nw[k - MT_D]);
    }
    __syncthreads();
    if (tid < MT_N - 1 - 2 * MT_D) {                                    // 454..622
      const int k = 2 * MT_D + tid;
      nw[k] = mt_mix(o[k], o[k + 1], nw[k - MT_D]);
    } else if (tid == MT_N - 1 - 2 * MT_D) {
      nw[MT_N - 1] = mt_mix(o[MT_N - 1], nw[0], nw[MT_M - 1]);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int k = tid + s * BLOCK;
      if (k < MT_N && node[s] < n && step[s] < S)
        zs[step[s] * n + node[s]] = (unsigned char)(mt_temper(nw[k]) % (unsigned)(m - step[s]));
      node[s] += adv_node;
      step[s] += adv_step;
      if (step[s] >= W) { step[s] -= W; node[s] += 1; }
    }
    cur ^= 1;
  }
  __syncthreads();

  if (tid < n)
    for (int t = 0; t < S; ++t) {
      const int u = t + zs[t * n + tid];                                // < m
      const unsigned char x = p[t * n + tid], y = p[u * n + tid];
      p[t * n + tid] = y;
      p[u * n + tid] = x;
    }
  // (a lane reads only its own column of p below: no barrier)

  int r_prev = 0;
  for (int j = 0; j < a.n_r; ++j) {
    const int r = a.r[j], cap = a.cap[j];
    if (tid < n)
      for (int t = r_prev; t < r; ++t) {
        int c = p[t * n + tid];
        c += (c >= tid) ? 1 : 0;
        atomicOr(&bm[(c >> 5) * n + tid], 1u << (c & 31));
        atomicOr(&bm[(tid >> 5) * n + c], 1u << (tid & 31));
      }
    r_prev = r > r_prev ? r : r_prev;
    __syncthreads();
    int cnt = 0;
    if (tid < n)
      for (int w = 0; w < RW; ++w) cnt += __popc(bm[w * n + tid]);
    int incl = cnt;                                                     // inclusive scan inside the wave
    const int lane = tid & (ISIC_WAVE - 1), wv = tid / ISIC_WAVE;
#pragma unroll
    for (int o = 1; o < ISIC_WAVE; o <<= 1) {
      const int v = __shfl_up(incl, o, ISIC_WAVE);
      if (lane >= o) incl += v;
    }
    if (lane == ISIC_WAVE - 1) wave_total[wv] = incl;
    __syncthreads();
    int pos = incl - cnt, total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      const int v = wave_total[w];
      pos += w < wv ? v : 0;
      total += v;
    }
    int64_t* src = a.edges + a.base[j] + (int64_t)g * 2 * cap;
    int64_t* dst = src + cap;
    if (tid < n)
      for (int w = 0; w < RW; ++w) {
        unsigned bits = bm[w * n + tid];
        while (bits && pos < cap) {
          const int c = (w << 5) + __ffs(bits) - 1;
          bits &= bits - 1u;
          src[pos] = tid;
          dst[pos] = c;
          ++pos;
        }
      }
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
  // words up to the last used one: node n - 1, step S - 1
  const int64_t used = a.swaps > 0 ? (int64_t)(n - 1) * (m - 1) + a.swaps : 0;
  a.regens = (int)ceil_div64(used, MT_N);
  a.z_bytes = (unsigned)round4((size_t)n * a.swaps);
  const size_t lds = (size_t)n * ((n + 31) / 32) * 4 + a.z_bytes + round4((size_t)n * m);
  static IsicPerDeviceOnce once;              // hipFuncSetAttribute is per device
  if (isic_once_per_device(once, [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(rand_graph_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)MAX_DYN_LDS);
      }) != hipSuccess)
    return ISIC_ERR_LAUNCH;
  hipLaunchKernelGGL(rand_graph_kernel, dim3((unsigned)G), dim3(BLOCK), lds, st, a);
  return isic_launch_status();
}

}  // extern "C"
