/* libisic_hip.so -- patch graphs of unequal size: the subgraph induced by a node subset (the lesion patches of an image),
 * for a whole record set in two launches, and the one-launch assembly of a step's batched CSR out of a store whose graphs
 * differ in node and entry count (isic_csr_batch_assemble is the equal-size case).  Opt-in: the reference only knows
 * 196-node graphs.  Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h: return 0 or a negative ISIC_ERR_* code, every argument is checked before any device work,
 * no allocation, no synchronisation, `stream` last.  Every offset is 64-bit.  A value read from device memory (an offset, an
 * endpoint, a selection index) is compared with the array sizes passed by value before it is used as an index: no argument
 * VALUE makes a kernel read or write outside the arrays as their sizes are stated here.
 */
#ifndef ISIC_HIP_RAGGED_H
#define ISIC_HIP_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Induced subgraphs of G graphs.  node_offsets, edge_offsets int64 [G+1] (graph g owns nodes [node_offsets[g],
 * node_offsets[g+1]) of the T flags and edges [edge_offsets[g], edge_offsets[g+1]) of the E edges); src, dst int64 [E] hold
 * LOCAL node ids; keep uint8 [T], non-zero = kept.  Per graph (tests/ragged_graph_ref.py):
 *     k    = keep[g] if keep[g].any() else all ones        (a graph without a single kept node keeps every node)
 *     new  = cumsum(k) - 1                                 (compact local ids, order preserved)
 *     m    = k[src] & k[dst]                               (both endpoints kept)
 *     out  = (new[src[m]], new[dst[m]])                    (edge order preserved)
 *     rows = nonzero(k)                                    (old local id of every kept node)
 *
 * _count: one workgroup per graph.  Writes new_id int32 [T] (the compact id, -1 for a dropped node), kept_nodes[g] and
 * kept_edges[g] (int64) and bad[g] (uint32): the number of edges of g with an endpoint outside [0, n_g), which are never used
 * as an index and never kept; a graph whose own offsets are decreasing or leave [0, T] / [0, E] writes nothing but
 * bad[g] = 0xFFFFFFFF and zero counts.  G == 0 returns 0 and touches nothing.  ISIC_ERR_BAD_ARG: G, T or E negative, a NULL
 * pointer with G > 0 (src / dst may be NULL when E == 0, keep / new_id when T == 0).  ISIC_ERR_UNSUPPORTED: T or E >= 2^31. */
int isic_induced_subgraph_count(const int64_t* node_offsets, const int64_t* edge_offsets, const int64_t* src,
                                const int64_t* dst, const uint8_t* keep, int G, int64_t T, int64_t E, int32_t* new_id,
                                int64_t* kept_nodes, int64_t* kept_edges, uint32_t* bad, void* stream);

/* _write: the stable compaction, one workgroup per graph, from the new_id of _count and the EXCLUSIVE prefix sums of its two
 * count arrays with the totals appended: node_out_offsets, edge_out_offsets int64 [G+1], [G] == T_out resp. E_out.  Edges go
 * through in chunks of 256 with a block scan and a running base, so a graph's output order is its input order.  Writes
 * src_out, dst_out int64 [E_out] (compact LOCAL ids), edge_weight_out float [E_out] when edge_weight (float [E]) is given
 * (both or neither), and rows_out int64 [T_out] (old LOCAL id of every kept node).  A store whose position leaves the
 * graph's own output segment or [0, T_out) / [0, E_out) is dropped (offsets that do not belong to the counts).  Same
 * argument rules as _count; T_out and E_out follow those of T and E (negative -> BAD_ARG, >= 2^31 -> UNSUPPORTED), and the
 * outputs may be NULL where their size is 0. */
int isic_induced_subgraph_write(const int64_t* node_offsets, const int64_t* edge_offsets, const int64_t* src,
                                const int64_t* dst, const float* edge_weight, const int32_t* new_id, int G, int64_t T,
                                int64_t E, const int64_t* node_out_offsets, const int64_t* edge_out_offsets, int64_t T_out,
                                int64_t E_out, int64_t* src_out, int64_t* dst_out, float* edge_weight_out,
                                int64_t* rows_out, void* stream);

/* One launch assembles a step's batched CSR (and its transpose) out of ONE CSR built over a whole record set of G graphs of
 * unequal size (train.GraphStore): rowptr, rowptr_t int32 [N+1], col, col_t, perm_t int32 and val, val_t float [NNZ] with
 * GLOBAL ids, store_node_off int64 [G+1] (graph g owns rows [store_node_off[g], store_node_off[g+1])) and store_nnz_off int64
 * [G+1], store_nnz_off[g] = rowptr[store_node_off[g]] = rowptr_t[store_node_off[g]] (g owns those slots of both orientations).
 * sel int64 [B] picks the graphs (repeats allowed); node_base, nnz_base int64 [B+1] are the batch's exclusive prefix sums of
 * the picked graphs' node and entry counts with the totals appended (the host keeps the per-graph sizes).  For output slot i,
 * b = the last position with nnz_base[b] <= i (binary search; zero-length segments are stepped over), g = sel[b]:
 *     col_out[i]    = col[s] - store_node_off[g] + node_base[b],      s = store_nnz_off[g] + (i - nnz_base[b])   (col_t alike)
 *     perm_t_out[i] = perm_t[s] - store_nnz_off[g] + nnz_base[b],     val_out[i] = val[s]                         (val_t alike)
 * and for output row r of position b: rowptr_out[r] = rowptr[q] - store_nnz_off[g] + nnz_base[b] with q = store_node_off[g] +
 * (r - node_base[b]) (rowptr_t alike), row_index_out[r] = q (optional: NULL skips it) -- the node's row in the concatenated
 * feature store; rowptr_out[total_nodes] = rowptr_t_out[total_nodes] = total_nnz.  total_nodes = node_base[B] and total_nnz =
 * nnz_base[B] are passed by value (they size the launch and the outputs: [total_nodes + 1], [total_nnz]); a position whose
 * sel is outside [0, G) or whose segment is longer than the picked graph writes nothing for the excess.
 * B == 0 returns 0 and touches nothing.  ISIC_ERR_BAD_ARG: B, G, total_nodes or total_nnz negative, G == 0 with B > 0, a NULL
 * pointer other than row_index_out (col .. perm_t and their outputs may be NULL when total_nnz == 0).
 * ISIC_ERR_UNSUPPORTED: total_nodes or total_nnz >= 2^31 - 1. */
int isic_csr_batch_assemble_ragged(const int64_t* sel, const int64_t* node_base, const int64_t* nnz_base, int B, int G,
                                   int64_t total_nodes, int64_t total_nnz, const int64_t* store_node_off,
                                   const int64_t* store_nnz_off, const int32_t* rowptr, const int32_t* rowptr_t,
                                   const int32_t* col, const int32_t* col_t, const float* val, const float* val_t,
                                   const int32_t* perm_t, int32_t* rowptr_out, int32_t* rowptr_t_out, int32_t* col_out,
                                   int32_t* col_t_out, float* val_out, float* val_t_out, int32_t* perm_t_out,
                                   int32_t* row_index_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_RAGGED_H */
