/* libisic_hip.so -- H2GCN (Zhu et al. 2020) on a batch of small graphs: the exact 2-hop neighbourhood built on the device
 * out of bit rows in LDS, and the two-operator propagation Z = [A1^ H | A2^ H], graph-resident, with its backward.  Opt-in:
 * isic_spmm_csr_f32, isic_gpr_prop_f32 and their bits are untouched.  isic_hip/graph.py (two_hop, h2_prop) calls them.
 * Included by isic_hip.h.
 *
 * Conventions as in isic_hip_gpr.h: return 0 or a negative ISIC_ERR_* code, every argument is checked before any device work,
 * no allocation, no synchronisation, no read-back, no floating-point atomics, `stream` last.  A value read from device memory
 * (a node offset, a row pointer, a column id) is compared with the sizes passed by value, or with the graph's own node range,
 * before it is used as an index: no argument VALUE makes a kernel read or write outside the arrays as their sizes are stated
 * here.
 *
 * The graph input of the two builders is a destination-major CSR over all N nodes of the batch with GLOBAL ids (what
 * isic_gcn_csr_build writes in any mode): rowptr int32 [N+1], col int32 [nnz]; only the structure is read, there is no val.
 * node_offsets is device int64 [G+1]: graph g owns nodes -- and CSR rows -- [node_offsets[g], node_offsets[g+1]), and every
 * column id of its rows must lie in that same range.  max_nodes is the caller's bound on a graph's node count.  The edge list
 * may be directed and hold duplicates and self loops.  Per graph with n nodes (tests/h2gcn_ref.py):
 *     A1[i,j] = 1  iff  i != j and the CSR holds (i,j) or (j,i)
 *     A2[i,j] = 1  iff  i != j, A1[i,j] = 0 and some m has A1[i,m] = A1[m,j] = 1
 *     dp[i]   = entries of row i of Ap,  r = 1.0f / sqrtf((float)dp[i])  (0 for an empty row),  val(i,j) = r[i] * r[j]
 * each step one correctly rounded fp32 operation.  Both operators are symmetric.
 *
 * One workgroup of 256 threads takes one graph.  The CSR entries set (i,j) and (j,i) in a 256 x 256-bit matrix in LDS with
 * integer LDS atomics (the result does not depend on their order), the thread of node i ORs the bit rows of its neighbours
 * and masks out A1 and the diagonal.
 *
 * bad is device uint32 [1], zeroed by the caller; the kernels only add to it.  A graph is BAD if its offsets decrease, leave
 * [0, N] or span more than max_nodes, if a row pointer of its rows decreases or leaves [0, nnz], if one of its rows holds a
 * column id outside the graph's own node range, or (write, prop) if a row pointer of an operator leaves [0, nnz1] resp.
 * [0, nnz2] (prop: or decreases, or holds a column id outside the graph).  A bad graph writes nothing, adds 1 to bad[0] and
 * does not disturb its neighbours.  Graphs of 0 and 1 node are legal.
 *
 * ISIC_ERR_BAD_ARG: G, N, an nnz or max_nodes negative, F < 1, ldh < F, ldz < 2 F; with G > 0 a NULL rowptr, node_offsets,
 * bad or output, a NULL col (val) unless its nnz == 0, a NULL H / dZ / degree array unless N == 0; node_offsets not 8-byte
 * aligned, another pointer not 4-byte aligned.  ISIC_ERR_UNSUPPORTED: max_nodes > ISIC_H2_MAX_NODES, N or an nnz beyond
 * 2^31 - 1, or more workgroups than 2^31 - 1; nothing is written.  G == 0 returns 0 without a launch. */
#ifndef ISIC_HIP_H2_H
#define ISIC_HIP_H2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISIC_H2_MAX_NODES 256
#define ISIC_H2_SLAB 32

/* deg1[N], deg2[N] (int32): the entries of every row of A1 and A2, on the rows of every good graph; rows no graph owns are
 * not touched. */
int isic_two_hop_count(const int32_t* rowptr, const int32_t* col, int64_t nnz, const int64_t* node_offsets, int64_t G,
                       int max_nodes, int64_t N, int32_t* deg1, int32_t* deg2, uint32_t* bad, void* stream);

/* rowptr1, rowptr2 int32 [N+1]: the exclusive prefix sums of deg1 / deg2 with the totals nnz1 / nnz2 appended (the caller's
 * scan; the totals also by value).  Rebuilds the bit rows and writes, for both operators, col (GLOBAL ids, ascending inside a
 * row), val and perm int32 [nnzp]: perm[slot of (i,j)] = the slot of (j,i) = rowptrp[j] + popcount(bits of row j below i).  An
 * operator with its perm is a complete symmetric CSR: its transpose is itself.  A store whose slot leaves its row's own
 * segment [rowptrp[i], rowptrp[i+1]) is dropped (row pointers that do not belong to the counts). */
int isic_two_hop_write(const int32_t* rowptr, const int32_t* col, int64_t nnz, const int64_t* node_offsets, int64_t G,
                       int max_nodes, int64_t N, const int32_t* rowptr1, const int32_t* rowptr2, int64_t nnz1, int64_t nnz2,
                       int32_t* col1, float* val1, int32_t* perm1, int32_t* col2, float* val2, int32_t* perm2, uint32_t* bad,
                       void* stream);

/* Z[:, 0:F] = A1^ H, Z[:, F:2F] = A2^ H on the rows of every good graph, H with row stride ldh >= F and Z with row stride
 * ldz >= 2 F (floats): either may be a slice of a wider buffer, and nothing beyond the 2 F columns is touched.  One workgroup
 * of 256 threads per graph and slab of ISIC_H2_SLAB columns: the slab of H is staged once in LDS as [n][32] floats and both
 * operators gather out of it, every sum in slot order. */
int isic_h2_prop_f32(const int32_t* rowptr1, const int32_t* col1, const float* val1, int64_t nnz1, const int32_t* rowptr2,
                     const int32_t* col2, const float* val2, int64_t nnz2, const int64_t* node_offsets, int64_t G,
                     int max_nodes, int64_t N, const float* H, int64_t ldh, int F, float* Z, int64_t ldz, uint32_t* bad,
                     void* stream);

/* dH[:, 0:F] = (A1^ dZ[:, 0:F]) + (A2^ dZ[:, F:2F]) on the same CSRs (the operators are symmetric): both slabs of dZ are
 * staged, each sum is completed in slot order, then the two are added. */
int isic_h2_prop_bwd_f32(const int32_t* rowptr1, const int32_t* col1, const float* val1, int64_t nnz1, const int32_t* rowptr2,
                         const int32_t* col2, const float* val2, int64_t nnz2, const int64_t* node_offsets, int64_t G,
                         int max_nodes, int64_t N, const float* dZ, int64_t ldz, int F, float* dH, int64_t ldh, uint32_t* bad,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_H2_H */
