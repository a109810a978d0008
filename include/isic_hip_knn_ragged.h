/* libisic_hip.so -- k-NN graphs among patch sets of unequal size (the lesion patches of every image of a frame): a Gram
 * kernel whose work follows each graph's own node count, and the edge lists of up to 16 k values with the reference's
 * per-image clamp (03_build_graphs.py:42-45) in one launch.  Opt-in: isic_knn_graph and the 196-node path are untouched.
 * Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h and isic_hip_ragged.h: return 0 or a negative ISIC_ERR_* code, every argument is checked
 * before any device work, no allocation, no synchronisation, `stream` last.  Every offset is 64-bit.  A value read from
 * device memory (an offset, a neighbour id, an edge position) is compared with the sizes passed by value before it is used
 * as an index: no argument VALUE makes a kernel read or write outside the arrays as their sizes are stated here.
 */
#ifndef ISIC_HIP_KNN_RAGGED_H
#define ISIC_HIP_KNN_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The Gram path of isic_knn_graph for graphs of 0 .. 208 nodes, sized by the graph: x float [total_nodes, D], offsets int64
 * [G+1] on the device (graph g owns rows [offsets[g], offsets[g+1])).  Per graph d = (|xi|^2 + |xj|^2) - 2 xi.xj in fp32,
 * clamp >= 0, diagonal = +inf, the k smallest of every row ascending, ties to the lower index; LOCAL ids to nn_idx int64
 * [total_nodes, k], -1 (and +inf in nn_dist float [total_nodes, k], optional) where a row has fewer than k candidates.
 * A graph of N nodes stages ceil(N/16)*16 rows and multiplies ceil(N/16)^2 tiles; every dot product takes the k-slices in
 * the MFMA order of isic_knn_graph's Gram kernel, and the norms (the Gram diagonal), the distance and the selection are the
 * same code as that kernel's (csrc/knn_tile.inc), so both outputs equal isic_knn_graph's bit for bit.
 * A graph is taken by the smallest workgroup that holds it (<= 64 nodes: 4 waves, <= 128: 8, <= 208: 13; one launch per
 * class up to max_nodes, which must be >= the largest graph).
 * Graphs of 0 or 1 node are legal (a single node gets a row of -1).  A graph whose offsets decrease, leave
 * [0, total_nodes] or span more than max_nodes writes nothing and reads no row of x.
 * G == 0 or total_nodes == 0 returns 0 and touches nothing.  ISIC_ERR_BAD_ARG: G, total_nodes or max_nodes negative, D or k
 * < 1, a NULL x / offsets / nn_idx.  ISIC_ERR_UNSUPPORTED: D % 32 != 0, D < 32, k > 16, max_nodes > 208, G > 2^22 (one
 * workgroup per graph).  The size classes are separate launches: after a non-zero return the outputs are unspecified (a
 * class may have been written before another failed to launch). */
int isic_knn_graph_ragged(const float* x, const int64_t* offsets, int G, int D, int k, int max_nodes,
                          int64_t total_nodes, int64_t* nn_idx, float* nn_dist /* may be NULL */, void* stream);

/* The edge lists of K k values out of ONE neighbour table nn_idx int64 [total_nodes, kmax] (LOCAL ids, ascending by
 * distance), one launch.  k_values: K ints in HOST memory (read by the entry itself, 1 <= K <= 16, each >= 1).  List q
 * holds for every graph g of n_g nodes n_g * kk edges, kk = 0 if n_g < 2 else max(1, min(k_values[q], n_g - 1))
 * (03_build_graphs.py:42-45), source-major with the neighbours ascending (:52-53): edge (i, j) goes to position
 * edge_base[q][g] + i * kk + j of src_out / dst_out int64 [total_edges] as (i, nn_idx[offsets[g] + i][j]), both plus
 * offsets[g] when global_ids != 0.  edge_base int64 [K, G+1] on the device: absolute positions in the flat outputs; the
 * sizes are analytic, so the host forms them from the node counts it holds (isic_hip.graph.knn_edge_offsets).
 * The kernel recomputes kk.  A pair (q, g) whose segment [edge_base[q][g], edge_base[q][g+1]) is not exactly n_g * kk long
 * or leaves [0, total_edges], whose kk exceeds kmax, or whose graph offsets decrease or leave [0, total_nodes], writes
 * nothing and adds 1 to bad[0]; a neighbour id outside [0, n_g) is never used as more than data: -1 is stored for it and
 * bad[0] grows by 1.  bad uint32 [1], zeroed by the caller.
 * G == 0 or total_edges == 0 returns 0 and touches nothing.  ISIC_ERR_BAD_ARG: a negative size, kmax < 1, K outside
 * [1, 16], a k value < 1, a NULL pointer (nn_idx may be NULL when total_nodes == 0).  ISIC_ERR_UNSUPPORTED: total_nodes >=
 * 2^31, kmax > 65536 or G > 2^22.  After a non-zero return the outputs are unspecified. */
int isic_knn_edges_ragged(const int64_t* nn_idx, int kmax, const int64_t* offsets, int G, int64_t total_nodes,
                          const int32_t* k_values, int K, const int64_t* edge_base /* [K, G+1] */, int64_t total_edges,
                          int global_ids, int64_t* src_out, int64_t* dst_out, uint32_t* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_KNN_RAGGED_H */
