/* libisic_hip.so -- the heterophily stage (04_measure_heterophily.py:107-181) on patch graphs of unequal size: the subgraphs
 * that lesion flags induce (isic_hip_ragged.h) or any record set whose graphs differ in node count.  Opt-in: the reference
 * only measures 196-node graphs on the 14-wide lattice (isic_edge_heterophily_f32, isic_laplacian_lambda2_f64).  Included by
 * isic_hip.h.
 *
 * Graphs are described as graph.induced_subgraphs returns them: src, dst int64 [E] hold LOCAL node ids; edge_offsets,
 * node_offsets int64 [G+1]; graph g owns edges [edge_offsets[g], edge_offsets[g+1]) and nodes [node_offsets[g],
 * node_offsets[g+1]) of x [T, D], probs [T, C] and dominant_class [T]; n_g = node_offsets[g+1] - node_offsets[g].
 *
 * Conventions as in isic_hip_ragged.h: return 0 or a negative ISIC_ERR_* code; ISIC_ERR_BAD_ARG (a negative size, a NULL
 * pointer where the sizes need one) is answered before ISIC_ERR_UNSUPPORTED, both before any device work; G == 0 returns 0 and
 * touches nothing; no allocation, no free, no synchronisation; `stream` last.  A value read from device memory (an offset, an
 * endpoint, a class, a graph id) is compared with the sizes passed by value before it is used as an index.  No entry uses a
 * floating-point atomic: every output is bit-identical from run to run.
 */
#ifndef ISIC_HIP_HETERO_RAGGED_H
#define ISIC_HIP_HETERO_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per directed edge e (self loops included, as isic_edge_heterophily_f32): h_kl, h_dirichlet, h_spatial, same_class float [E],
 * with the arithmetic of isic_edge_heterophily_f32 (one wave per edge, the same row gather).  The edge's graph g is
 * edge_graph[e] (int32 [E]) when given, else the last g with edge_offsets[g] <= e (binary search; empty graphs are stepped
 * over); its rows are node_offsets[g] + src[e] and node_offsets[g] + dst[e].  The lattice position of node i of graph g is
 * patch_pos[node_offsets[g] + i] (int32 [T]: the `rows` of an induced subgraph), or i when patch_pos is NULL:
 *     h_spatial = hypot(p_s % grid_w - p_d % grid_w, p_s / grid_w - p_d / grid_w).
 * An edge whose graph id is outside [0, G), that lies outside its graph's edge segment, whose graph's node segment leaves
 * [0, T] or whose endpoint is outside [0, n_g) gets NaN in all four outputs and reads no row.
 * ISIC_ERR_BAD_ARG: G, T, E negative, D, C, grid_w < 1, a NULL pointer with G > 0 (patch_pos and edge_graph are optional; src,
 * dst and the outputs may be NULL when E == 0, x, probs, dominant_class when T == 0).  ISIC_ERR_UNSUPPORTED: T or E >= 2^31. */
int isic_edge_heterophily_ragged_f32(const float* x, const float* probs, const int32_t* dominant_class,
                                     const int32_t* patch_pos, const int64_t* src, const int64_t* dst,
                                     const int64_t* edge_offsets, const int64_t* node_offsets, const int32_t* edge_graph, int G,
                                     int64_t T, int64_t E, int D, int C, int grid_w, float eps, float* h_kl,
                                     float* h_dirichlet, float* h_spatial, float* same_class, void* stream);

/* The class bookkeeping of 04:115-149 per graph, one workgroup per graph, integer counters in LDS, one thread finishes in
 * fp64:
 *     num_edges[g] = #{e : src != dst}                                                   (int64 [G], 04:115-116)
 *     edge_h       = #{src != dst, class[src] == class[dst]} / num_edges, 0 without edges (04:128-131)
 *     expected[g]  = sum_k (count_k / max(1, n_g))^2, count = class histogram of the graph's nodes   (double [G])
 *     h_adj[g]     = (edge_h - expected) / (1 - expected) if expected < 1 else 1          (double [G])
 *     compat[g]    = C x C counts of (class[src], class[dst]) over src != dst, every row divided by its sum, a zero row
 *                    stays zero                                                           (double [G, C, C])
 * n_g == 0: num_edges 0, h_adj 0, a zero matrix.  bad[g] (uint32 [G]) is 0 for a good graph; a dominant_class outside [0, C),
 * an edge endpoint outside [0, n_g) or offsets that decrease or leave [0, T] / [0, E] set bad[g] = 1, num_edges[g] = 0 and NaN
 * in h_adj, expected and compat of that graph; such a value is never used as an index.
 * ISIC_ERR_BAD_ARG: G, T, E negative, C < 1, a NULL pointer with G > 0 (src / dst may be NULL when E == 0, dominant_class when
 * T == 0).  ISIC_ERR_UNSUPPORTED: C > 64, T or E >= 2^31. */
int isic_graph_homophily_ragged(const int32_t* dominant_class, const int64_t* src, const int64_t* dst,
                                const int64_t* edge_offsets, const int64_t* node_offsets, int G, int64_t T, int64_t E, int C,
                                int64_t* num_edges, double* h_adj, double* expected, double* compat, uint32_t* bad,
                                void* stream);

/* Order-preserving removal of the self-loop edges (04:115-116) from M rows of per-edge values: values, out float [M, E].
 * kept_offsets int64 [G+1] is the exclusive prefix sum of isic_graph_homophily_ragged's num_edges with the total appended (a
 * device cumsum: nothing is read back).  One workgroup per graph, edges in chunks of 256 with a block scan and a running base
 * (as isic_induced_subgraph_write), so the kept values of graph g lie at out[m, kept_offsets[g] : kept_offsets[g+1]] in their
 * input order and isic_segment_stats_f32 runs on contiguous segments; the rest of out is left as it was.  A store whose
 * position leaves the graph's own output segment or [0, E) is dropped; a graph whose edge offsets decrease or leave [0, E]
 * writes nothing.  ISIC_ERR_BAD_ARG: G, M, E negative, a NULL pointer with G > 0 (values, src, dst, out may be NULL when
 * M * E == 0).  ISIC_ERR_UNSUPPORTED: E >= 2^31. */
int isic_edge_values_compact_ragged_f32(const float* values, const int64_t* src, const int64_t* dst,
                                        const int64_t* edge_offsets, const int64_t* kept_offsets, int G, int M, int64_t E,
                                        float* out, void* stream);

/* lambda_2 of I - D^-1/2 max(A, A^T) D^-1/2 per graph (isic_laplacian_lambda2_f64: the same device code, duplicated edges
 * summed, self loops skipped) with n_g nodes and LOCAL ids: lambda2 double [G].  max_nodes is a host-known bound on n_g that
 * sizes the workgroup's LDS.  n_g <= 1 gives 0.0; a graph with n_g > max_nodes, an endpoint outside [0, n_g) or offsets that
 * decrease or leave [0, E] gets NaN.  ISIC_ERR_BAD_ARG: G, E, max_nodes negative, a NULL pointer with G > 0 (src / dst may be
 * NULL when E == 0).  ISIC_ERR_UNSUPPORTED: max_nodes > ISIC_SPECTRAL_MAX_NODES, E >= 2^31. */
int isic_laplacian_lambda2_ragged_f64(const int64_t* src, const int64_t* dst, const int64_t* edge_offsets,
                                      const int64_t* node_offsets, int G, int64_t E, int max_nodes, double* lambda2,
                                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_HETERO_RAGGED_H */
