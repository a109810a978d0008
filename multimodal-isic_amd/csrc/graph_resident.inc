// What the graph-resident kernels share (gpr_prop.hip, h2_prop.hip, two_hop.hip): a block of 256 threads owns one graph of at
// most 256 nodes, validates everything it read from device memory before it indexes with it, and gathers CSR rows out of a
// slab of 32 feature columns in LDS.  Needs common.h.
//
// The validation is what the headers promise ("no argument VALUE makes a kernel read or write outside the arrays"), written
// once: gr_range compares the graph's two offsets with N and max_nodes; gr_csr_flag compares the two ends of its CSR
// range with nnz, every row pointer of its rows with that range and every column id of the range with the graph's own node
// range.  Both answer 1 for a bad graph; the kernel joins the threads' answers with __syncthreads_or, so the block leaves
// together.  What a kernel does about a bad graph (who adds to bad[0], what else is zeroed) stays with the kernel.
#pragma once
#include "../../include/isic_hip_gpr.h"
#include "../../include/isic_hip_h2.h"

constexpr int GR_BLOCK = 256;                              // threads per block = the most nodes of a graph
constexpr int GR_W = ISIC_GPR_SLAB;                        // feature columns per slab
constexpr int GR_ROWS_PER_PASS = GR_BLOCK / GR_W;          // 8 rows of the slab per pass of the block
constexpr int GR_MAX_LDS_BYTES = 2 * ISIC_GPR_MAX_NODES * GR_W * (int)sizeof(float);
static_assert(GR_W == 32 && GR_ROWS_PER_PASS == 8 && GR_MAX_LDS_BYTES == 65536, "a half wave per row of the slab");
static_assert(ISIC_GPR_SLAB == ISIC_H2_SLAB && ISIC_GPR_MAX_NODES == ISIC_H2_MAX_NODES && ISIC_GPR_MAX_NODES == GR_BLOCK,
              "one geometry for every graph-resident kernel");

struct GrCsr {
  const int32_t* rowptr;
  const int32_t* col;
  const float* val;        // NULL where only the structure is read (two_hop.hip)
  int64_t nnz;
};

// ---------------------------------------------------------------- device
// Graph g's node range [lo, lo + n) out of offsets[g], offsets[g + 1], compared with the sizes passed by value before anything
// is indexed with it.  flag = 1 (and n = 0) if the offsets decrease, leave [0, N] or span more than max_nodes.
struct GrRange {
  int64_t lo;
  int n, flag;
};
__device__ __forceinline__ GrRange gr_range(const int64_t* offsets, int64_t g, int64_t N, int max_nodes) {
  const int64_t lo = offsets[g], hi = offsets[g + 1];
  const bool range_ok = lo >= 0 && hi >= lo && hi <= N && hi - lo <= (int64_t)max_nodes;
  return {lo, range_ok ? (int)(hi - lo) : 0, range_ok ? 0 : 1};
}

// This thread's share of the CSR check of rows [lo, lo + n), n > 0 (0 <= lo < lo + n <= N: rowptr[lo .. lo + n] exists): 1 if
// the rows do not fit the arrays or hold a column id outside the graph.
__device__ __forceinline__ int gr_csr_flag(const GrCsr& s, int64_t lo, int n) {
  const int64_t pb = s.rowptr[lo], pe = s.rowptr[lo + n];
  if (pb < 0 || pe < pb || pe > s.nnz) return 1;
  int flag = 0;
  for (int r = threadIdx.x; r < n; r += GR_BLOCK) {
    const int64_t b = s.rowptr[lo + r], e = s.rowptr[lo + r + 1];
    if (b < pb || e < b || e > pe) flag = 1;
  }
  for (int64_t p = pb + threadIdx.x; p < pe; p += GR_BLOCK) {
    const int64_t cl = (int64_t)s.col[p] - lo;
    if (cl < 0 || cl >= n) flag = 1;
  }
  return flag;
}

// sum_p val[p] * src[col[p] - lo][c] over the slots of a validated row, in slot order: one fmaf chain.  src is a [n][GR_W] slab
// in LDS, ilo = (unsigned)lo: every column id is an int32 inside [lo, lo + n), so col - lo is 0 .. n - 1.
__device__ __forceinline__ float gr_row_sum(const GrCsr& s, int64_t row, unsigned ilo, const float* src, int c) {
  const int pb = s.rowptr[row], pe = s.rowptr[row + 1];
  float acc = 0.f;
#pragma unroll 4
  for (int p = pb; p < pe; ++p) acc = fmaf(s.val[p], src[(int)((unsigned)s.col[p] - ilo) * GR_W + c], acc);
  return acc;
}

// ---------------------------------------------------------------- host
static inline bool gr_aligned_to(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// rowptr present, col (and val, where the entry reads values) present unless nnz == 0, all 4-byte aligned
static inline bool gr_csr_args_ok(const GrCsr& s, bool need_val) {
  return s.rowptr && ((s.col && (s.val || !need_val)) || s.nnz == 0) && gr_aligned_to(s.rowptr, 4) && gr_aligned_to(s.col, 4) &&
         gr_aligned_to(s.val, 4);
}

// One block of GR_BLOCK threads per graph, at most 64 KB of dynamic LDS.
template <auto Kernel, class Args>
static inline int gr_launch(int64_t blocks, size_t lds_bytes, hipStream_t st, const Args& a) {
  return isic_launch_lds<Kernel, GR_MAX_LDS_BYTES>(dim3((unsigned)blocks), dim3(GR_BLOCK), lds_bytes, st, a);
}
