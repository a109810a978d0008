// The two-operator propagation of H2GCN, graph-resident (include/isic_hip_h2.h):
//   forward   Z[:, 0:F] = A1^ H,  Z[:, F:2F] = A2^ H                       isic_h2_prop_f32
//   backward  dH = (A1^ dZ[:, 0:F]) + (A2^ dZ[:, F:2F])                     isic_h2_prop_bwd_f32
// on the SAME two CSRs: both operators are symmetric (csrc/two_hop.hip writes them).
//
// The layout is gpr_prop.hip's: a block of 256 threads takes one graph (n <= 256 nodes) and one slab of W = 32 feature columns;
// thread t owns column c = t % 32 of rows r = t / 32 + 8 j.  The slab of H goes once into LDS as [n][32] floats (the backward
// stages the two slabs of dZ, [2][n][32]), one barrier, then every thread gathers its rows out of LDS in slot order: the 32
// lanes of a half wave read the 32 consecutive floats of one row -- one bank each under the (a / 4) % 32 rule of ds_read_b32
// -- and the two halves of a wave never conflict.  The CSR entries of a row are the same address in all 32 lanes of a half
// wave: one request.  Nothing is carried across rows, so there is no register array and no template on the row count: the
// 2-hop rows hold tens to hundreds of entries and the row loop is the whole kernel.
//
//   * Validation before anything is indexed: the node-range check and, for BOTH operators, the CSR check of
//     graph_resident.inc, joined by __syncthreads_or.  A bad graph adds 1 to bad[0] (an integer atomic, slab 0 only) and
//     writes nothing.
//   * The backward completes the sum over A1's row, then the sum over A2's row, then adds the two: three roundings more than
//     the longer dot product, in a fixed order.  No float atomics anywhere.
#include "common.h"
#include "graph_resident.inc"

#include "../../include/isic_hip_h2.h"

#include <limits.h>

namespace {

constexpr int BLOCK = GR_BLOCK, W = GR_W, ROWS_PER_PASS = GR_ROWS_PER_PASS;

struct H2Args {
  GrCsr op1, op2;
  const int64_t* offsets;
  const float* X;          // forward: H (row stride ldx = ldh); backward: dZ (ldx = ldz)
  float* out;              // forward: Z (ldo = ldz); backward: dH (ldo = ldh)
  uint32_t* bad;
  int64_t N, ldx, ldo;
  int max_nodes, F, slabs;
};

template <bool BWD>
__global__ __launch_bounds__(BLOCK) void h2_prop_kernel(H2Args a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];    // forward [n][W]; backward [2][n][W]
  const int tid = threadIdx.x, F = a.F;
  const int64_t g = blockIdx.x / a.slabs;
  const int slab = (int)(blockIdx.x % a.slabs), f0 = slab * W;

  // ---- the graph's node range, then both CSR ranges, their row pointers and column ids (graph_resident.inc)
  const GrRange nr = gr_range(a.offsets, g, a.N, a.max_nodes);
  const int64_t lo = nr.lo;
  const int n = nr.n;
  int flag = nr.flag;
  if (n > 0) flag = gr_csr_flag(a.op1, lo, n) | gr_csr_flag(a.op2, lo, n);
  flag = __syncthreads_or(flag);
  if (flag || n == 0) {                         // the same verdict in every thread: the block leaves together
    if (flag && slab == 0 && tid == 0) atomicAdd(a.bad, 1u);
    return;
  }

  // ---- stage the slab(s)
  const int c = tid % W, r0 = tid / W;
  const bool col_ok = f0 + c < F;
  float* buf1 = lds;
  float* buf2 = BWD ? lds + n * W : lds;
  for (int r = r0; r < n; r += ROWS_PER_PASS) {
    const int64_t at = (lo + r) * a.ldx + f0 + c;
    buf1[r * W + c] = col_ok ? a.X[at] : 0.f;
    if (BWD) buf2[r * W + c] = col_ok ? a.X[at + F] : 0.f;
  }
  __syncthreads();

  // ---- gather: every column id is an int32 inside [lo, hi), so col - lo is 0 .. n - 1
  const unsigned ilo = (unsigned)lo;
  for (int r = r0; r < n; r += ROWS_PER_PASS) {
    const float s1 = gr_row_sum(a.op1, lo + r, ilo, buf1, c);
    const float s2 = gr_row_sum(a.op2, lo + r, ilo, buf2, c);
    if (col_ok) {
      const int64_t at = (lo + r) * a.ldo + f0 + c;
      if (BWD) {
        a.out[at] = s1 + s2;
      } else {
        a.out[at] = s1;
        a.out[at + F] = s2;
      }
    }
  }
}

template <bool BWD>
int launch(const H2Args& a, int64_t blocks, hipStream_t st) {
  return gr_launch<h2_prop_kernel<BWD>>(blocks, (size_t)(BWD ? 2 : 1) * a.max_nodes * W * sizeof(float), st, a);
}

// the argument checks and the launch the two entries share (ldh, ldz as the header names them)
int run(bool bwd, const GrCsr& op1, const GrCsr& op2, const int64_t* node_offsets, int64_t G, int max_nodes, int64_t N,
        const float* X, float* out, int64_t ldh, int64_t ldz, int F, uint32_t* bad, void* stream) {
  ISIC_CHECK_ARG(G >= 0 && N >= 0 && op1.nnz >= 0 && op2.nnz >= 0 && max_nodes >= 0 && F >= 1);
  ISIC_CHECK_ARG(ldh >= (int64_t)F && ldz >= 2 * (int64_t)F);
  ISIC_CHECK_ARG((gr_csr_args_ok(op1, true) && gr_csr_args_ok(op2, true) && node_offsets && bad && ((X && out) || N == 0)) ||
                 G == 0);
  ISIC_CHECK_ARG(gr_aligned_to(node_offsets, 8) && gr_aligned_to(X, 4) && gr_aligned_to(out, 4) && gr_aligned_to(bad, 4));
  if (max_nodes > ISIC_H2_MAX_NODES) return ISIC_ERR_UNSUPPORTED;
  if (N > (int64_t)INT_MAX || op1.nnz > (int64_t)INT_MAX || op2.nnz > (int64_t)INT_MAX) return ISIC_ERR_UNSUPPORTED;
  if (G > (int64_t)INT_MAX / ceil_div(F, W)) return ISIC_ERR_UNSUPPORTED;
  if (G == 0) return ISIC_OK;
  H2Args a = {};
  a.op1 = op1; a.op2 = op2; a.offsets = node_offsets; a.X = X; a.out = out; a.bad = bad; a.N = N;
  a.ldx = bwd ? ldz : ldh; a.ldo = bwd ? ldh : ldz; a.max_nodes = max_nodes; a.F = F; a.slabs = ceil_div(F, W);
  const int64_t blocks = G * a.slabs;
  return bwd ? launch<true>(a, blocks, as_stream(stream)) : launch<false>(a, blocks, as_stream(stream));
}

}  // namespace

extern "C" {

int isic_h2_prop_f32(const int32_t* rowptr1, const int32_t* col1, const float* val1, int64_t nnz1, const int32_t* rowptr2,
                     const int32_t* col2, const float* val2, int64_t nnz2, const int64_t* node_offsets, int64_t G,
                     int max_nodes, int64_t N, const float* H, int64_t ldh, int F, float* Z, int64_t ldz, uint32_t* bad,
                     void* stream) {
  return run(false, GrCsr{rowptr1, col1, val1, nnz1}, GrCsr{rowptr2, col2, val2, nnz2}, node_offsets, G, max_nodes, N, H, Z, ldh,
             ldz, F, bad, stream);
}

int isic_h2_prop_bwd_f32(const int32_t* rowptr1, const int32_t* col1, const float* val1, int64_t nnz1, const int32_t* rowptr2,
                         const int32_t* col2, const float* val2, int64_t nnz2, const int64_t* node_offsets, int64_t G,
                         int max_nodes, int64_t N, const float* dZ, int64_t ldz, int F, float* dH, int64_t ldh, uint32_t* bad,
                         void* stream) {
  return run(true, GrCsr{rowptr1, col1, val1, nnz1}, GrCsr{rowptr2, col2, val2, nnz2}, node_offsets, G, max_nodes, N, dZ, dH, ldh,
             ldz, F, bad, stream);
}

}  // extern "C"
