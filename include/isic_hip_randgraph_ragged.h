/* libisic_hip.so -- the random patch graphs of the reference (03_build_graphs.py:57-78, `_random_edge_index`) for a batch of
 * graphs of UNEQUAL size -- the lesion patches of every image of a frame -- bit for bit what the reference's host code gives
 * for each graph's own node count: count, then write.  Opt-in: isic_random_graph_i64 and its bits are untouched.
 * isic_hip/graph.py (random_graphs_ragged) calls it.  Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h and isic_hip_ragged.h: return 0 or a negative ISIC_ERR_* code, every argument is checked
 * before any device work, no allocation, no synchronisation, no read-back, `stream` last.  Every offset is 64-bit.  A value
 * read from device memory (a node offset, an edge offset) is compared with the sizes passed by value before it is used as
 * an index: no argument VALUE makes a kernel read or write outside the arrays as their sizes are stated here.
 *
 * The definition is the one include/isic_hip_randgraph.h states, PER GRAPH: graph g has n_g = node_offsets[g+1] -
 * node_offsets[g] nodes and the seed seeds[g] (the low 32 bits are used).  n_g < 2: no edges.  Otherwise every r is clamped
 * to [1, n_g - 1] by the graph's OWN node count (03:61), MT19937 is seeded, node i consumes n_g - 2 words, Fisher-Yates on
 * word % (m - t) with m = n_g - 1, targets c += (c >= i), edges symmetrised, deduplicated, ascending by (src, dst).  All r
 * values of a graph share its seed, so the targets for r are a prefix of those for r' > r.
 *
 * seeds         device int64 [G].
 * node_offsets  device int64 [G+1]: graph g owns nodes [node_offsets[g], node_offsets[g+1]); node_offsets[G] is the total.
 * max_nodes     the caller's bound on n_g (<= ISIC_RANDGRAPH_RAGGED_MAX_NODES); it sizes LDS and the launches.
 * r_values      HOST int [n_r], 1 <= n_r <= ISIC_RANDGRAPH_RAGGED_MAX_R_VALUES: read before the call returns.  Any order,
 *               repeats allowed; a value below 1 counts as 1.
 * bad           device uint32 [1], zeroed by the caller; the kernels only add to it.
 *
 * A graph is BAD if its offsets decrease, leave [0, node_offsets[G]] or span more than max_nodes: it gets count 0 for
 * every r, writes nothing, adds 1 to bad[0] (in either call) and does not disturb its neighbours.
 *
 * Lanes and LDS follow the graph: graphs of up to ISIC_RANDGRAPH_RAGGED_PACK_NODES (64) nodes take ONE WAVE each, four to
 * a workgroup, every wave with its own double-buffered MT19937 state, draw bytes, permutation columns and adjacency
 * bitmap in LDS (sized by min(max_nodes, 64)), synchronised inside the wave only; larger graphs take a 256-lane workgroup
 * each in a second launch, which is only made when max_nodes > 64.  The generator, the draw window, Fisher-Yates and the
 * bitmap enumeration are the source text isic_random_graph_i64 runs (csrc/rand_graph.inc).  Integer work only: two calls
 * give identical bits.
 *
 * ISIC_ERR_BAD_ARG: r_values NULL, G or max_nodes negative, with G > 0 a NULL seeds / node_offsets / counts / bad (write:
 * edge_off; src / dst unless total == 0), total negative, an int64 array not 8-byte aligned or bad not 4-byte aligned.
 * ISIC_ERR_UNSUPPORTED: max_nodes > ISIC_RANDGRAPH_RAGGED_MAX_NODES, n_r outside [1, ISIC_RANDGRAPH_RAGGED_MAX_R_VALUES].
 * G == 0: ISIC_OK, nothing is launched. */
#ifndef ISIC_HIP_RANDGRAPH_RAGGED_H
#define ISIC_HIP_RANDGRAPH_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISIC_RANDGRAPH_RAGGED_MAX_NODES 256
#define ISIC_RANDGRAPH_RAGGED_MAX_R_VALUES 16
#define ISIC_RANDGRAPH_RAGGED_PACK_NODES 64

/* counts int64 [n_r][G]: counts[j][g] = the number of edges of graph g for the caller's j-th r value (0 for n_g < 2 and
 * for a bad graph).  Every entry is written. */
int isic_random_graph_ragged_count(const int64_t* seeds, const int64_t* node_offsets, int G, int max_nodes,
                                   const int* r_values, int n_r, int64_t* counts, uint32_t* bad, void* stream);

/* edge_off int64 [n_r][G+1] on the device: graph g's edges for r value j go to slots [edge_off[j][g], edge_off[j][g+1])
 * of ONE flat pair of arrays src, dst int64 [total] (absolute positions; normally the exclusive prefix sums of _count's
 * counts over (j, g) in row-major order, each row closed by the next row's start).  Ids are LOCAL, or plus node_offsets[g]
 * when global_ids != 0.  A pair (j, g) whose segment leaves [0, total] or is not exactly as long as the graph's edge count
 * writes nothing and adds 1 to bad[0]; entries outside the segments are left untouched. */
int isic_random_graph_ragged_write(const int64_t* seeds, const int64_t* node_offsets, int G, int max_nodes,
                                   const int* r_values, int n_r, const int64_t* edge_off, int64_t total, int global_ids,
                                   int64_t* src, int64_t* dst, uint32_t* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_RANDGRAPH_RAGGED_H */
