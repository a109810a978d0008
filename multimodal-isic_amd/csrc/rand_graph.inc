// The device text of the reference's random patch graph (include/isic_hip_randgraph.h states the definition), shared by
// csrc/rand_graph.hip (one 256-lane workgroup per graph of ONE node count) and csrc/rand_graph_ragged.hip (a node count per
// graph; a wave or a workgroup per graph): bit-equality of the two builds is a property of this text, not of two copies.
//
// A GROUP of LANES lanes builds one graph, one node per lane (n <= LANES).  LANES == 64: the group is a wave and is
// synchronised inside the wave only -- the LDS operations of one wave execute in issue order, so a fence that keeps the
// compiler from moving them is all a hand-over between lanes needs, and no __syncthreads() is ever reached; the waves of a
// workgroup may then take graphs of different size, or none.  Any other LANES: the group is the WHOLE workgroup and every
// group_sync is a __syncthreads(), so every lane of the workgroup must make the same calls with the same trip counts.
//
//   * Stream.  MT19937 in LDS, double-buffered: a regeneration reads the old 624 words from one buffer and writes the new
//     ones into the other, so a lane never overwrites a word another lane still has to read.  Word k mixes old[k], old[k+1]
//     and word (k + 397) % 624, which is OLD for k < 227 and NEW (word k - 227) after; a lane-parallel phase is valid only
//     among words whose new source is already written, hence three phases with a group_sync after each: 0..226, 227..453
//     (new 0..226), 454..622 (new 227..395), and in the last phase one lane also forms word 623 from old[623], new[0] and
//     new[396].  One lane seeds (init_genrand is a chain).
//   * Draws.  Node i owns words [i W, (i + 1) W), W = n - 2, and uses the first S = min(max r, n - 2) of them.  After a
//     regeneration lane l looks at words l, l + LANES, ... of the block; (node, step) of each of its slots advances by 624
//     words per block without a division.  A used word is tempered and reduced at once: z = word % (m - t) < 256 is kept
//     as ONE BYTE, zs[t][node].  The next regeneration's first phase writes the buffer nobody reads any more, so the draws
//     need no group_sync of their own.
//   * Fisher-Yates, one node per lane, on byte columns p[.][node] in LDS (n (n - 1) bytes): S swaps.
//   * For the r values in ascending order: the target columns [r_prev, r) are OR-ed into the symmetric adjacency bitmap
//     (LDS, word w of row i at bm[w n + i]), then lane i counts row i, a prefix sum over the group places the row, and the
//     lane writes its (src, dst) pairs in ascending bit order.  The bitmap only grows, which is the prefix property.
#ifndef ISIC_RAND_GRAPH_INC
#define ISIC_RAND_GRAPH_INC

#include "common.h"

namespace randgraph {

constexpr int MT_N = 624, MT_M = 397, MT_D = MT_N - MT_M;      // 227
constexpr size_t round4(size_t b) { return (b + 3) & ~(size_t)3; }

// bitmap words + draw bytes + permutation bytes of one graph of n >= 2 nodes and S swaps
__host__ __device__ constexpr size_t graph_lds_bytes(int n, int S) {
  return (size_t)n * ((n + 31) / 32) * 4 + round4((size_t)n * S) + round4((size_t)n * (n - 1));
}
// state regenerations that hold a used word: the words up to node n - 1, step S - 1
__host__ __device__ constexpr int graph_regens(int n, int S) {
  return S > 0 ? ((n - 1) * (n - 2) + S + MT_N - 1) / MT_N : 0;
}

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

template <int LANES>
__device__ __forceinline__ void group_sync() {
  if constexpr (LANES == ISIC_WAVE) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// Seeds, draws and shuffles: on return lane i < n holds in p[0..S-1][i] the first S entries of node i's permutation (the
// rest of its column is the identity the swaps left behind), bm is zero, and a lane may read ITS OWN column of p without a
// further group_sync; the bitmap of other lanes' rows needs one (the r loop has it after add_targets).
// st: [2][MT_N] words, bm: [ceil(n / 32)][n] words, zs: [S][n] bytes, p: [n - 1][n] bytes, all this group's own.
template <int LANES>
__device__ __forceinline__ void generate(unsigned (*st)[MT_N], unsigned* bm, unsigned char* zs, unsigned char* p, int lane,
                                         unsigned seed32, int n, int S, int regens) {
  constexpr int SLOTS = (MT_N + LANES - 1) / LANES;               // words of a block one lane looks at
  const int m = n - 1, W = m - 1;
  const int RW = (n + 31) >> 5;

  if (lane == 0) {
    unsigned s = seed32;
    st[0][0] = s;
    for (int j = 1; j < MT_N; ++j) {
      s = 1812433253u * (s ^ (s >> 30)) + (unsigned)j;
      st[0][j] = s;
    }
  }
  for (int e = lane; e < RW * n; e += LANES) bm[e] = 0u;
  if (lane < n)
    for (int t = 0; t < m; ++t) p[t * n + lane] = (unsigned char)t;

  // (node, step) of the words this lane looks at in the current block, and the advance per block
  int node[SLOTS] = {}, step[SLOTS] = {};
  int adv_node = 0, adv_step = 0;
  if (W > 0) {
    adv_node = MT_N / W;
    adv_step = MT_N - adv_node * W;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int k = lane + s * LANES;
      node[s] = k / W;
      step[s] = k - node[s] * W;
    }
  }
  group_sync<LANES>();

  int cur = 0;
  for (int b = 0; b < regens; ++b) {
    const unsigned* o = st[cur];
    unsigned* nw = st[cur ^ 1];
    for (int k = lane; k < MT_D; k += LANES) nw[k] = mt_mix(o[k], o[k + 1], o[k + MT_M]);
    group_sync<LANES>();
    for (int k = MT_D + lane; k < 2 * MT_D; k += LANES) nw[k] = mt_mix(o[k], o[k + 1], nw[k - MT_D]);
    group_sync<LANES>();
    for (int k = 2 * MT_D + lane; k < MT_N - 1; k += LANES) nw[k] = mt_mix(o[k], o[k + 1], nw[k - MT_D]);      // 454..622
    if (lane == LANES - 1) nw[MT_N - 1] = mt_mix(o[MT_N - 1], nw[0], nw[MT_M - 1]);
    group_sync<LANES>();
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int k = lane + s * LANES;
      if (k < MT_N && node[s] < n && step[s] < S)
        zs[step[s] * n + node[s]] = (unsigned char)(mt_temper(nw[k]) % (unsigned)(m - step[s]));
      node[s] += adv_node;
      step[s] += adv_step;
      if (step[s] >= W) { step[s] -= W; node[s] += 1; }
    }
    cur ^= 1;
  }
  group_sync<LANES>();

  if (lane < n)
    for (int t = 0; t < S; ++t) {
      const int u = t + zs[t * n + lane];                               // < m
      const unsigned char x = p[t * n + lane], y = p[u * n + lane];
      p[t * n + lane] = y;
      p[u * n + lane] = x;
    }
}

// The target columns [r_from, r_to) of every node into the symmetric bitmap.  A group_sync must follow before rows are read.
__device__ __forceinline__ void add_targets(unsigned* bm, const unsigned char* p, int lane, int n, int r_from, int r_to) {
  if (lane < n)
    for (int t = r_from; t < r_to; ++t) {
      int c = p[t * n + lane];
      c += (c >= lane) ? 1 : 0;
      atomicOr(&bm[(c >> 5) * n + lane], 1u << (c & 31));
      atomicOr(&bm[(lane >> 5) * n + c], 1u << (lane & 31));
    }
}

// Lane i's row: its number of set bits (0 for lane >= n), its first position `pos` in the graph's ascending edge list and
// the graph's `total`.  LANES == 64: shuffles only, wave_total is not used.  Otherwise wave_total [LANES / 64] ints of LDS
// and one __syncthreads() inside; a group_sync must follow before wave_total is used again.
template <int LANES>
__device__ __forceinline__ void place_rows(const unsigned* bm, int lane, int n, int* wave_total, int& pos, int& total) {
  const int RW = (n + 31) >> 5;
  int cnt = 0;
  if (lane < n)
    for (int w = 0; w < RW; ++w) cnt += __popc(bm[w * n + lane]);
  int incl = cnt;                                                       // inclusive scan inside the wave
  const int wl = lane & (ISIC_WAVE - 1), wv = lane / ISIC_WAVE;
#pragma unroll
  for (int o = 1; o < ISIC_WAVE; o <<= 1) {
    const int v = __shfl_up(incl, o, ISIC_WAVE);
    if (wl >= o) incl += v;
  }
  pos = incl - cnt;
  if constexpr (LANES == ISIC_WAVE) {
    total = __shfl(incl, ISIC_WAVE - 1, ISIC_WAVE);
  } else {
    if (wl == ISIC_WAVE - 1) wave_total[wv] = incl;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int w = 0; w < LANES / ISIC_WAVE; ++w) {
      const int v = wave_total[w];
      pos += w < wv ? v : 0;
      total += v;
    }
  }
}

// Lane i writes row i's pairs (i + add, c + add) from position pos on, in ascending bit order, never at or past `limit`.
__device__ __forceinline__ void write_rows(const unsigned* bm, int lane, int n, int pos, int limit, int64_t* src, int64_t* dst,
                                           int64_t add) {
  const int RW = (n + 31) >> 5;
  if (lane < n)
    for (int w = 0; w < RW; ++w) {
      unsigned bits = bm[w * n + lane];
      while (bits && pos < limit) {
        const int c = (w << 5) + __ffs(bits) - 1;
        bits &= bits - 1u;
        src[pos] = lane + add;
        dst[pos] = c + add;
        ++pos;
      }
    }
}

}  // namespace randgraph
#endif  // ISIC_RAND_GRAPH_INC
