/* libisic_hip.so -- the K-hop polynomial graph filter of GPR-GNN (Chien et al. 2021) and APPNP on a batch of small graphs,
 * graph-resident: Z = sum_{k=0..K} gamma[k] A^^k H (+ bias) in ONE launch, and its backward in one launch plus a fixed-order
 * reduction.  Opt-in: isic_spmm_csr_f32 and its bits are untouched.  isic_hip/graph.py (gpr_prop) calls them.  Included by
 * isic_hip.h.
 *
 * Conventions as in isic_hip_ragged.h and isic_hip_moments_ragged.h: return 0 or a negative ISIC_ERR_* code, every argument is
 * checked before any device work, no allocation, no synchronisation, no read-back, `stream` last.  A value read from device
 * memory (a node offset, a row pointer, a column id) is compared with the sizes passed by value, or with the graph's own node
 * range, before it is used as an index: no argument VALUE makes a kernel read or write outside the arrays as their sizes are
 * stated here.
 *
 * The operator is a destination-major CSR over all N nodes of the batch (what isic_gcn_csr_build writes): rowptr int32 [N+1],
 * col int32 [nnz] GLOBAL node ids, val fp32 [nnz], nnz = the number of entries of col and val.  node_offsets is device int64
 * [G+1]: graph g owns nodes -- and CSR rows -- [node_offsets[g], node_offsets[g+1]), and every column id of its rows must lie
 * in that same range (a batch of graphs is block-diagonal).  max_nodes is the caller's bound on a graph's node count; a result
 * does not depend on it (it sizes the dynamic LDS and the registers a thread keeps).
 *
 * One workgroup of 256 threads takes one graph and one slab of ISIC_GPR_SLAB = 32 feature columns: the slab of H is staged
 * once into LDS as [n][32] floats, the K hops gather out of LDS between two such buffers with one barrier per hop, a thread
 * keeps its <= ceil(max_nodes / 8) elements of Z in registers across the hops and stores them once.  No power A^^k H is ever
 * written to memory.  gamma is read from DEVICE memory, so a captured step sees an optimiser's update.
 *
 * bad is device uint32 [1], zeroed by the caller; the kernels only add to it.  A graph is BAD if its offsets decrease, leave
 * [0, N] or span more than max_nodes, if a row pointer of its rows decreases or leaves [0, nnz], or if one of its rows holds
 * a column id outside the graph's own node range.  A bad graph writes nothing to Z (dH), contributes 0 to dgamma, adds 1 to
 * bad[0] and does not disturb its neighbours.  A graph of 0 nodes is legal and writes nothing.
 *
 * No floating-point atomics: two identical calls give identical bits.  The backward parks one partial <P_k, H> per
 * workgroup and k in the workspace, [G * ceil(F / 32)][K + 1], and adds them in the fixed order of csrc/slab_sum.inc
 * (order A, 16 lanes per element).
 *
 * ISIC_ERR_BAD_ARG: G, N, nnz or max_nodes negative, F < 1, K outside 0 .. ISIC_GPR_MAX_K; with G > 0 a NULL rowptr,
 * node_offsets, gamma, bad or output, a NULL H / dZ unless N == 0, a NULL col / val unless nnz == 0; node_offsets not 8-byte
 * aligned, another pointer not 4-byte aligned.  ISIC_ERR_UNSUPPORTED: max_nodes > ISIC_GPR_MAX_NODES, or G ceil(F / 32)
 * workgroups beyond 2^31 - 1; nothing is written.  ISIC_ERR_WORKSPACE: dgamma wanted and the workspace NULL, not 4-byte
 * aligned or smaller than isic_gpr_prop_bwd_workspace_bytes.  G == 0 returns 0 without a launch (the backward then writes
 * dgamma = beta_gamma * dgamma). */
#ifndef ISIC_HIP_GPR_H
#define ISIC_HIP_GPR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISIC_GPR_MAX_NODES 256
#define ISIC_GPR_MAX_K 16
#define ISIC_GPR_SLAB 32

/* Z[N, F] = sum_k gamma[k] A^^k H (+ bias[F], may be NULL) on the rows of every good graph; rows no graph owns are not
 * touched. */
int isic_gpr_prop_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t nnz,
                      const int64_t* node_offsets, int64_t G, int max_nodes, int64_t N, const float* H,
                      const float* gamma, int K, int F, const float* bias, float* Z, uint32_t* bad, void* stream);

/* The backward on the TRANSPOSED CSR (rowptr_t, col_t, val_t; a k-NN graph is directed): with P_k = (A^^T)^k dZ,
 *   dH[N, F] = sum_k gamma[k] P_k                         (may be NULL: not formed)
 *   dgamma[k] = beta_gamma * dgamma[k] + <P_k, H>         (may be NULL: no partial is formed and H is not read;
 *                                                          beta_gamma is 0 -- dgamma is never read -- or 1)
 * from one pass over the hops: the thread that owns an element of P_k holds the matching element of H in a register. */
size_t isic_gpr_prop_bwd_workspace_bytes(int64_t G, int K, int F);
int isic_gpr_prop_bwd_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* val_t, int64_t nnz,
                          const int64_t* node_offsets, int64_t G, int max_nodes, int64_t N, const float* dZ,
                          const float* H, const float* gamma, int K, int F, float* dH, float* dgamma,
                          float beta_gamma, void* workspace, size_t workspace_bytes, uint32_t* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_GPR_H */
