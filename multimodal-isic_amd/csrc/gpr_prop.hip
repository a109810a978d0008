// The K-hop polynomial graph filter of GPR-GNN / APPNP, graph-resident (include/isic_hip_gpr.h):
//   forward   Z  = sum_k gamma[k] A^^k H (+ bias)                      isic_gpr_prop_f32
//   backward  dH = sum_k gamma[k] (A^^T)^k dZ,  dgamma[k] = <(A^^T)^k dZ, H>      isic_gpr_prop_bwd_f32
// Both are ONE kernel: the backward is the forward's hop loop on the transposed CSR with dZ for H, plus a dot
// product per hop against the element of H the thread holds in a register.
//
// A block of 256 threads takes one graph (n <= 256 nodes) and one slab of W = 32 feature columns.  Thread t owns column
// c = t % 32 of rows r = t / 32 + 8 j, j < RPT = ceil(max_nodes / 8) rounded up to 8, 16, 25 or 32 (a template parameter, so
// that z[] and h[] are registers: 60 / 80 / 129 / 157 VGPRs, no spill).  The forward runs the same instantiation with
// partial, Hd NULL (a forward-only instantiation took 256 registers and spilled at RPT = 25 with this hipcc).
// The slab of H goes once into LDS buffer 0 as [n][32] floats; hop k reads buffer (k - 1) % 2 and writes buffer k % 2,
// ONE barrier per hop (the barrier in front of hop k + 1 orders hop k's reads of a buffer before hop k + 1's writes to
// it); the last hop writes no buffer.  LDS banking: the 32 lanes of a half wave read
// (and write) the 32 consecutive floats of one row -- one bank each under the (a / 4) % 32 rule of ds_read_b32 / ds_write_b32
// -- and the two halves of a wave never conflict.  The CSR entries of a row are read from memory by every hop (the same
// address in all 32 lanes of a half wave: one request, an L1 hit after the validation pass below has read them once).
//
//   * Validation before anything is indexed: the node-range and CSR checks of graph_resident.inc, joined by __syncthreads_or.
//     A bad graph adds 1 to bad[0] (an integer atomic, slab 0 only), zeroes its dgamma partials and writes nothing else.
//   * dgamma.  After hop k a thread has s = sum_j P_k[r_j][c] h[j]; a wave's s meet in the xor tree of wave_sum, the four wave
//     sums of hop k are parked in LDS and added in wave order by thread k at the end: partial[block][k].  The blocks' partials
//     meet in order A of slab_sum.inc (isic_slab_reduce_launch, 16 lanes per element).  No float atomics anywhere.
#include "slab_sum.inc"
#include "graph_resident.inc"

#include "../../include/isic_hip_gpr.h"

#include <limits.h>

namespace {

constexpr int BLOCK = GR_BLOCK, W = GR_W, ROWS_PER_PASS = GR_ROWS_PER_PASS;
static_assert(ISIC_GPR_MAX_K + 1 <= BLOCK, "thread k adds the wave sums of hop k");

struct GprArgs {
  GrCsr csr;
  const int64_t* offsets;
  const float* X;          // forward: H; backward: dZ
  const float* Hd;         // backward: H when dgamma is wanted, else NULL
  const float* gamma;
  const float* bias;       // forward only (NULL in the backward)
  float* out;              // forward: Z; backward: dH or NULL
  float* partial;          // backward: [blocks][K + 1] when dgamma is wanted, else NULL
  uint32_t* bad;
  int64_t N;
  int max_nodes, K, F, slabs;
};

template <int RPT>
__global__ __launch_bounds__(BLOCK) void gpr_prop_kernel(GprArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];    // [2][n][W]
  __shared__ float wave_part[(ISIC_GPR_MAX_K + 1) * (BLOCK / ISIC_WAVE)];
  const int tid = threadIdx.x, K = a.K, F = a.F;
  const int64_t g = blockIdx.x / a.slabs;
  const int slab = (int)(blockIdx.x % a.slabs), f0 = slab * W;
  const bool want_dg = a.partial != nullptr;      // backward with dgamma; the forward has neither partial nor Hd
  float* prow = want_dg ? a.partial + (int64_t)blockIdx.x * (K + 1) : nullptr;

  // ---- the graph's node range, then its CSR range, row pointers and column ids (graph_resident.inc)
  const GrRange nr = gr_range(a.offsets, g, a.N, a.max_nodes);
  const int64_t lo = nr.lo;
  const int n = nr.n;
  int flag = nr.flag;
  if (n > 0) flag = gr_csr_flag(a.csr, lo, n);
  flag = __syncthreads_or(flag);
  if (flag || n == 0) {                         // the same verdict in every thread: the block leaves together
    if (flag && slab == 0 && tid == 0) atomicAdd(a.bad, 1u);
    if (want_dg && tid <= K) prow[tid] = 0.f;
    return;
  }

  // ---- stage the slab: buffer 0, the k = 0 term, the row bounds and (backward) the matching elements of H
  const int c = tid % W, r0 = tid / W;
  const bool col_ok = f0 + c < F;
  float* buf0 = lds;
  float* buf1 = lds + n * W;
  float z[RPT], h[RPT];
  const float g0 = a.gamma[0];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int r = r0 + ROWS_PER_PASS * j;
    z[j] = 0.f; h[j] = 0.f;
    if (r < n) {
      const int64_t at = (lo + r) * F + f0 + c;
      const float v = col_ok ? a.X[at] : 0.f;
      buf0[r * W + c] = v;
      z[j] = g0 * v;
      if (want_dg) {
        h[j] = col_ok ? a.Hd[at] : 0.f;
        s = fmaf(v, h[j], s);
      }
    }
  }
  if (want_dg) {
    s = wave_sum(s);
    if (tid % ISIC_WAVE == 0) wave_part[tid / ISIC_WAVE] = s;
  }

  // ---- the hops
  const unsigned ilo = (unsigned)lo;
  for (int k = 1; k <= K; ++k) {
    __syncthreads();
    const float* src = (k & 1) ? buf0 : buf1;
    float* dst = (k & 1) ? buf1 : buf0;
    const float gk = a.gamma[k];
    const bool last = k == K;
    s = 0.f;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      const int r = r0 + ROWS_PER_PASS * j;
      if (r < n) {
        // the row bounds are read again by every hop (an L1 hit): kept across the hops they cost two registers a row, and
        // with them the kernel took 238 registers at RPT = 16 and spilled at 25
        const float acc = gr_row_sum(a.csr, lo + r, ilo, src, c);
        if (!last) dst[r * W + c] = acc;
        z[j] = fmaf(gk, acc, z[j]);
        if (want_dg) s = fmaf(acc, h[j], s);
      }
    }
    if (want_dg) {
      s = wave_sum(s);
      if (tid % ISIC_WAVE == 0) wave_part[k * (BLOCK / ISIC_WAVE) + tid / ISIC_WAVE] = s;
    }
  }

  // ---- store once
  if (a.out && col_ok) {
    const float bv = a.bias ? a.bias[f0 + c] : 0.f;
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      const int r = r0 + ROWS_PER_PASS * j;
      if (r < n) a.out[(lo + r) * F + f0 + c] = a.bias ? z[j] + bv : z[j];
    }
  }
  if (want_dg) {
    __syncthreads();
    if (tid <= K) {
      const float* wp = wave_part + tid * (BLOCK / ISIC_WAVE);
      prow[tid] = ((wp[0] + wp[1]) + wp[2]) + wp[3];
    }
  }
}

template <int RPT>
int launch_rpt(const GprArgs& a, int64_t blocks, hipStream_t st) {
  return gr_launch<gpr_prop_kernel<RPT>>(blocks, (size_t)2 * a.max_nodes * W * sizeof(float), st, a);
}

int launch(const GprArgs& a, int64_t blocks, hipStream_t st) {
  const int rpt = ceil_div(a.max_nodes, ROWS_PER_PASS);
  if (rpt <= 8) return launch_rpt<8>(a, blocks, st);
  if (rpt <= 16) return launch_rpt<16>(a, blocks, st);
  if (rpt <= 25) return launch_rpt<25>(a, blocks, st);      // up to 200 nodes: the reference's 196
  return launch_rpt<32>(a, blocks, st);
}

// the argument checks the two entries share; 1 = go on, else the code to return
int check_common(const GrCsr& s, const int64_t* node_offsets, int64_t G, int max_nodes, int64_t N, const float* X,
                 const float* gamma, int K, int F, const uint32_t* bad) {
  ISIC_CHECK_ARG(G >= 0 && N >= 0 && s.nnz >= 0 && max_nodes >= 0 && F >= 1 && K >= 0 && K <= ISIC_GPR_MAX_K);
  ISIC_CHECK_ARG((gr_csr_args_ok(s, true) && node_offsets && gamma && bad && (X || N == 0)) || G == 0);
  // (the alignment of the CSR arrays once more: here it is asked of an empty batch too)
  ISIC_CHECK_ARG(gr_aligned_to(node_offsets, 8) && gr_aligned_to(s.rowptr, 4) && gr_aligned_to(s.col, 4) &&
                 gr_aligned_to(s.val, 4) && gr_aligned_to(X, 4) && gr_aligned_to(gamma, 4) && gr_aligned_to(bad, 4));
  if (max_nodes > ISIC_GPR_MAX_NODES) return ISIC_ERR_UNSUPPORTED;
  if (G > (int64_t)INT_MAX / ceil_div(F, W)) return ISIC_ERR_UNSUPPORTED;
  return 1;
}

}  // namespace

extern "C" {

int isic_gpr_prop_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t nnz, const int64_t* node_offsets,
                      int64_t G, int max_nodes, int64_t N, const float* H, const float* gamma, int K, int F,
                      const float* bias, float* Z, uint32_t* bad, void* stream) {
  const GrCsr csr = {rowptr, col, val, nnz};
  const int rc = check_common(csr, node_offsets, G, max_nodes, N, H, gamma, K, F, bad);
  if (rc != 1) return rc;
  ISIC_CHECK_ARG((Z || G == 0) && gr_aligned_to(Z, 4) && gr_aligned_to(bias, 4));
  if (G == 0) return ISIC_OK;
  GprArgs a = {};
  a.csr = csr; a.offsets = node_offsets; a.X = H; a.gamma = gamma; a.bias = bias; a.out = Z;
  a.bad = bad; a.N = N; a.max_nodes = max_nodes; a.K = K; a.F = F; a.slabs = ceil_div(F, W);
  return launch(a, G * a.slabs, as_stream(stream));
}

size_t isic_gpr_prop_bwd_workspace_bytes(int64_t G, int K, int F) {
  if (G <= 0 || K < 0 || K > ISIC_GPR_MAX_K || F < 1) return 0;
  return (size_t)G * (size_t)ceil_div(F, W) * (size_t)(K + 1) * sizeof(float);
}

int isic_gpr_prop_bwd_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* val_t, int64_t nnz,
                          const int64_t* node_offsets, int64_t G, int max_nodes, int64_t N, const float* dZ, const float* H,
                          const float* gamma, int K, int F, float* dH, float* dgamma, float beta_gamma, void* workspace,
                          size_t workspace_bytes, uint32_t* bad, void* stream) {
  const GrCsr csr = {rowptr_t, col_t, val_t, nnz};
  const int rc = check_common(csr, node_offsets, G, max_nodes, N, dZ, gamma, K, F, bad);
  if (rc != 1) return rc;
  ISIC_CHECK_ARG(beta_gamma == 0.f || beta_gamma == 1.f);
  ISIC_CHECK_ARG(gr_aligned_to(dH, 4) && gr_aligned_to(dgamma, 4) && gr_aligned_to(H, 4));
  ISIC_CHECK_ARG(!dgamma || H || N == 0 || G == 0);
  hipStream_t st = as_stream(stream);
  if (G == 0) {
    if (dgamma && beta_gamma == 0.f && hipMemsetAsync(dgamma, 0, (size_t)(K + 1) * sizeof(float), st) != hipSuccess)
      return ISIC_ERR_LAUNCH;
    return ISIC_OK;
  }
  if (dgamma && (!workspace || !gr_aligned_to(workspace, 4) || workspace_bytes < isic_gpr_prop_bwd_workspace_bytes(G, K, F)))
    return ISIC_ERR_WORKSPACE;
  if (!dH && !dgamma) return ISIC_OK;
  GprArgs a = {};
  a.csr = csr; a.offsets = node_offsets; a.X = dZ; a.Hd = dgamma ? H : nullptr;
  a.gamma = gamma; a.out = dH; a.partial = dgamma ? reinterpret_cast<float*>(workspace) : nullptr; a.bad = bad;
  a.N = N; a.max_nodes = max_nodes; a.K = K; a.F = F; a.slabs = ceil_div(F, W);
  const int64_t blocks = G * a.slabs;
  const int lrc = launch(a, blocks, st);
  if (lrc != ISIC_OK || !dgamma) return lrc;
  isic_slab_reduce_launch(ISIC_SLAB_XOR16, a.partial, (int)blocks, K + 1, dgamma, beta_gamma, st);
  return isic_launch_status();
}

}  // extern "C"
