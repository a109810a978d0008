// The exact 2-hop neighbourhood of every graph of a batch, built on the device (include/isic_hip_h2.h):
//   isic_two_hop_count   deg1[i], deg2[i] = entries of row i of A1 (the symmetrised 1-hop graph) and A2 (distance exactly 2)
//   isic_two_hop_write   col / val / perm of both operators behind the caller's exclusive scans of those degrees
// Both are the same build: a block of 256 threads takes one graph (n <= 256 nodes), thread i owns node i.
//
//   * Validation before anything is indexed: the node-range and CSR checks of graph_resident.inc (the write also: every row
//     pointer of both operators against [0, nnz1] / [0, nnz2]), joined by __syncthreads_or.  A bad graph adds 1 to bad[0] (an
//     integer atomic) and writes nothing.
//   * A1 as bit rows in LDS, 8 words a row at a stride of ROW = 9 words (thread i reads words i * 9 + k: 32 lanes on 32 banks;
//     at a stride of 8 they would meet on four).  Thread i walks CSR row i and sets (i,j) and (j,i) with atomicOr on LDS -- an
//     integer OR, so the matrix does not depend on the order of the entries or of the threads; self loops are skipped,
//     duplicates set a set bit.
//   * A2: thread i keeps row i of A1 in eight registers, ORs the rows of its neighbours (one LDS row per set bit) and masks
//     out A1 and the diagonal.  Row i of A2 goes to LDS as well: the write needs the rows of OTHER nodes for perm.
//   * The write walks the set bits of a row in ascending order: the k-th set bit j of row i is slot rowptr[i] + k, col = lo + j,
//     val = r[i] * r[j] with r = 1.0f / sqrtf((float)deg) (hipcc rounds the division and the square root correctly unless
//     told otherwise; nothing here can contract to an FMA), perm = rowptr[j] + the number of set bits of row j below i.
//     A slot outside [rowptr[i], rowptr[i+1]) is not stored.
#include "common.h"
#include "graph_resident.inc"

#include "../../include/isic_hip_h2.h"

#include <limits.h>

namespace {

constexpr int BLOCK = GR_BLOCK;
constexpr int WORDS = ISIC_H2_MAX_NODES / 32;      // 8 words of 32 bits a row
constexpr int ROW = WORDS + 1;                     // LDS stride of a bit row
static_assert(ISIC_H2_MAX_NODES == BLOCK && WORDS == 8, "a thread per node, eight words per bit row");

struct TwoHopArgs {
  GrCsr csr;                  // the input graph: structure only, val is NULL
  const int64_t* offsets;
  const int32_t* rowptr1;     // write only
  const int32_t* rowptr2;
  int32_t* deg1;              // count only
  int32_t* deg2;
  int32_t* col1;              // write only
  float* val1;
  int32_t* perm1;
  int32_t* col2;
  float* val2;
  int32_t* perm2;
  uint32_t* bad;
  int64_t nnz1, nnz2, N;
  int max_nodes;
};

// the set bits of w below position b
__device__ __forceinline__ int below(uint32_t w, int b) { return __popc(w & ((1u << b) - 1u)); }

// One operator of one row: bits[] is row i, rows[] the operator's bit rows in LDS, rs[] its 1 / sqrt(deg), rp[] its row pointers.
__device__ __forceinline__ void write_row(const uint32_t (&bits)[WORDS], const uint32_t* rows, const float* rs, const int32_t* rp,
                                          int i, int64_t lo, int32_t* col, float* val, int32_t* perm) {
  const int64_t b = rp[i], e = rp[i + 1];
  const float ri = rs[i];
  const int iw = i >> 5, ib = i & 31;
  int64_t slot = b;
#pragma unroll
  for (int w = 0; w < WORDS; ++w) {
    uint32_t m = bits[w];
    while (m) {
      const int j = w * 32 + __ffs(m) - 1;
      m &= m - 1;
      if (slot >= b && slot < e) {                 // the row's own segment, itself inside [0, nnz] (validated)
        const uint32_t* rj = rows + j * ROW;
        int rank = below(rj[iw], ib);
        for (int k = 0; k < iw; ++k) rank += __popc(rj[k]);
        col[slot] = (int32_t)(lo + j);
        val[slot] = ri * rs[j];
        perm[slot] = rp[j] + rank;
      }
      ++slot;
    }
  }
}

template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void two_hop_kernel(TwoHopArgs a) {
  __shared__ uint32_t adj1[ISIC_H2_MAX_NODES * ROW];
  __shared__ uint32_t adj2[WRITE ? ISIC_H2_MAX_NODES * ROW : 1];
  __shared__ float rs1[WRITE ? ISIC_H2_MAX_NODES : 1], rs2[WRITE ? ISIC_H2_MAX_NODES : 1];
  __shared__ int32_t rp1[WRITE ? ISIC_H2_MAX_NODES + 1 : 1], rp2[WRITE ? ISIC_H2_MAX_NODES + 1 : 1];
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x;

  // ---- the graph's node range, then its CSR range, row pointers and column ids (graph_resident.inc)
  const GrRange nr = gr_range(a.offsets, g, a.N, a.max_nodes);
  const int64_t lo = nr.lo;
  const int n = nr.n;
  int flag = nr.flag;
  if (n > 0) {
    flag = gr_csr_flag(a.csr, lo, n);
    if (WRITE) {                                   // the operators' row pointers of this graph's rows: values inside [0, nnzp]
      for (int r = tid; r <= n; r += BLOCK) {
        const int64_t v1 = a.rowptr1[lo + r], v2 = a.rowptr2[lo + r];
        if (v1 < 0 || v1 > a.nnz1 || v2 < 0 || v2 > a.nnz2) flag = 1;
      }
    }
  }
  flag = __syncthreads_or(flag);
  if (flag || n == 0) {                            // the same verdict in every thread: the block leaves together
    if (flag && tid == 0) atomicAdd(a.bad, 1u);
    return;
  }

  // ---- A1 as bit rows (n <= max_nodes <= 256 = BLOCK: thread i is node i)
  for (int w = tid; w < n * ROW; w += BLOCK) adj1[w] = 0u;
  __syncthreads();
  if (tid < n) {
    const int pb = a.csr.rowptr[lo + tid], pe = a.csr.rowptr[lo + tid + 1];
    for (int p = pb; p < pe; ++p) {
      const int j = (int)((int64_t)a.csr.col[p] - lo);                // 0 .. n - 1 (validated)
      if (j != tid) {
        atomicOr(&adj1[tid * ROW + (j >> 5)], 1u << (j & 31));
        atomicOr(&adj1[j * ROW + (tid >> 5)], 1u << (tid & 31));
      }
    }
  }
  __syncthreads();

  // ---- A2: the OR of the neighbours' rows, without A1 and the diagonal
  uint32_t b1[WORDS], b2[WORDS];
  int d1 = 0, d2 = 0;
#pragma unroll
  for (int k = 0; k < WORDS; ++k) { b1[k] = 0u; b2[k] = 0u; }
  if (tid < n) {
#pragma unroll
    for (int k = 0; k < WORDS; ++k) b1[k] = adj1[tid * ROW + k];
#pragma unroll
    for (int w = 0; w < WORDS; ++w) {
      uint32_t m = b1[w];
      while (m) {
        const uint32_t* rj = adj1 + (w * 32 + __ffs(m) - 1) * ROW;
        m &= m - 1;
#pragma unroll
        for (int k = 0; k < WORDS; ++k) b2[k] |= rj[k];
      }
    }
#pragma unroll
    for (int k = 0; k < WORDS; ++k) {
      b2[k] &= ~b1[k];
      if (k == (tid >> 5)) b2[k] &= ~(1u << (tid & 31));
      d1 += __popc(b1[k]);
      d2 += __popc(b2[k]);
    }
  }
  if (!WRITE) {
    if (tid < n) {
      a.deg1[lo + tid] = d1;
      a.deg2[lo + tid] = d2;
    }
    return;
  }

  // ---- the write: rows of A2, 1 / sqrt(deg) and the operators' row pointers to LDS, then every thread its two rows
  if (tid < n) {
#pragma unroll
    for (int k = 0; k < WORDS; ++k) adj2[tid * ROW + k] = b2[k];
    rs1[tid] = d1 > 0 ? 1.0f / sqrtf((float)d1) : 0.f;
    rs2[tid] = d2 > 0 ? 1.0f / sqrtf((float)d2) : 0.f;
  }
  for (int r = tid; r <= n; r += BLOCK) {
    rp1[r] = a.rowptr1[lo + r];
    rp2[r] = a.rowptr2[lo + r];
  }
  __syncthreads();
  if (tid < n) {
    write_row(b1, adj1, rs1, rp1, tid, lo, a.col1, a.val1, a.perm1);
    write_row(b2, adj2, rs2, rp2, tid, lo, a.col2, a.val2, a.perm2);
  }
}

// the argument checks the two entries share; 1 = go on, else the code to return
int check_common(const GrCsr& s, const int64_t* node_offsets, int64_t G, int max_nodes, int64_t N, const uint32_t* bad) {
  ISIC_CHECK_ARG(G >= 0 && N >= 0 && s.nnz >= 0 && max_nodes >= 0);
  ISIC_CHECK_ARG((gr_csr_args_ok(s, false) && node_offsets && bad) || G == 0);
  // (the alignment of the CSR arrays once more: here it is asked of an empty batch too)
  ISIC_CHECK_ARG(gr_aligned_to(node_offsets, 8) && gr_aligned_to(s.rowptr, 4) && gr_aligned_to(s.col, 4) && gr_aligned_to(bad, 4));
  if (max_nodes > ISIC_H2_MAX_NODES) return ISIC_ERR_UNSUPPORTED;
  if (G > (int64_t)INT_MAX || N > (int64_t)INT_MAX || s.nnz > (int64_t)INT_MAX) return ISIC_ERR_UNSUPPORTED;
  return 1;
}

}  // namespace

extern "C" {

int isic_two_hop_count(const int32_t* rowptr, const int32_t* col, int64_t nnz, const int64_t* node_offsets, int64_t G,
                       int max_nodes, int64_t N, int32_t* deg1, int32_t* deg2, uint32_t* bad, void* stream) {
  const GrCsr csr = {rowptr, col, nullptr, nnz};
  const int rc = check_common(csr, node_offsets, G, max_nodes, N, bad);
  if (rc != 1) return rc;
  ISIC_CHECK_ARG(((deg1 && deg2) || N == 0 || G == 0) && gr_aligned_to(deg1, 4) && gr_aligned_to(deg2, 4));
  if (G == 0) return ISIC_OK;
  TwoHopArgs a = {};
  a.csr = csr; a.offsets = node_offsets; a.deg1 = deg1; a.deg2 = deg2; a.bad = bad; a.N = N; a.max_nodes = max_nodes;
  hipLaunchKernelGGL(two_hop_kernel<false>, dim3((unsigned)G), dim3(BLOCK), 0, as_stream(stream), a);
  return isic_launch_status();
}

int isic_two_hop_write(const int32_t* rowptr, const int32_t* col, int64_t nnz, const int64_t* node_offsets, int64_t G,
                       int max_nodes, int64_t N, const int32_t* rowptr1, const int32_t* rowptr2, int64_t nnz1, int64_t nnz2,
                       int32_t* col1, float* val1, int32_t* perm1, int32_t* col2, float* val2, int32_t* perm2, uint32_t* bad,
                       void* stream) {
  const GrCsr csr = {rowptr, col, nullptr, nnz};
  const int rc = check_common(csr, node_offsets, G, max_nodes, N, bad);
  if (rc != 1) return rc;
  ISIC_CHECK_ARG(nnz1 >= 0 && nnz2 >= 0);
  ISIC_CHECK_ARG((rowptr1 && rowptr2 && ((col1 && val1 && perm1) || nnz1 == 0) && ((col2 && val2 && perm2) || nnz2 == 0)) || G == 0);
  ISIC_CHECK_ARG(gr_aligned_to(rowptr1, 4) && gr_aligned_to(rowptr2, 4) && gr_aligned_to(col1, 4) && gr_aligned_to(val1, 4) &&
                 gr_aligned_to(perm1, 4) && gr_aligned_to(col2, 4) && gr_aligned_to(val2, 4) && gr_aligned_to(perm2, 4));
  if (nnz1 > (int64_t)INT_MAX || nnz2 > (int64_t)INT_MAX) return ISIC_ERR_UNSUPPORTED;
  if (G == 0) return ISIC_OK;
  TwoHopArgs a = {};
  a.csr = csr; a.offsets = node_offsets; a.rowptr1 = rowptr1; a.rowptr2 = rowptr2; a.col1 = col1;
  a.val1 = val1; a.perm1 = perm1; a.col2 = col2; a.val2 = val2; a.perm2 = perm2; a.bad = bad; a.nnz1 = nnz1; a.nnz2 = nnz2;
  a.N = N; a.max_nodes = max_nodes;
  hipLaunchKernelGGL(two_hop_kernel<true>, dim3((unsigned)G), dim3(BLOCK), 0, as_stream(stream), a);
  return isic_launch_status();
}

}  // extern "C"
