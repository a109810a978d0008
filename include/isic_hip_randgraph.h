/* libisic_hip.so -- the random patch graphs of the reference (03_build_graphs.py:57-78, `_random_edge_index`; r in
 * {1..8, 12, 16} per image, 03:107-112) built on the device, BIT FOR BIT what the reference's host code gives: a batch of
 * G graphs and a list of r values in one launch.  isic_hip/graph.py (random_graphs) and build_graphs.py
 * (random_edge_index_batched) call it.  Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h: row-major device tensors, return 0 or a negative ISIC_ERR_* code, arguments are
 * checked before any device work, no allocation, no synchronisation, no read-back, `stream` last.
 *
 * The definition (the reference draws from a seeded CPU torch.Generator: `torch.randperm(n - 1, generator=g)[:r]` once
 * per node, which is MT19937 plus Fisher-Yates on 32-bit draws).  For one graph of n >= 2 nodes, seed s, r clamped to
 * [1, n - 1] (03:60), m = n - 1:
 *   1. Generator: standard MT19937 after init_genrand(s & 0xffffffff) -- only the low 32 bits of the seed matter.  Its
 *      outputs are the tempered 32-bit words in order; the first output follows the first regeneration of the state.
 *   2. Node i = 0..n-1 in turn consumes exactly m - 1 words, words [i (m - 1), (i + 1) (m - 1)).  With p = [0..m-1], for
 *      t = 0..m-2: z = word % (m - t) (on the 32-bit word), swap p[t] and p[t + z].  Position t is final after step t, so
 *      only the first min(r, m - 1) swaps are carried out; all m - 1 words are consumed all the same.
 *   3. The targets of node i are c = p[0..r-1] with c += (c >= i): the node itself is skipped.
 *   4. The edges are (i, c) and (c, i), deduplicated, ascending by (src, dst) -- what torch.unique(dim=1) yields, i.e.
 *      the set bits of the symmetric n x n adjacency bitmap in row-major order.
 * All r values of a graph share its seed (03:107-112,136), so the targets for r are a prefix of those for r' > r: one
 * permutation prefix of length max r serves the whole list.
 *
 * seeds     device int64 [G]: one seed per graph (any int64; the low 32 bits are used).
 * r_values  HOST int [n_r]: read before the call returns.  Any order, repeats allowed; each is clamped to [1, n_nodes - 1].
 * edges     device int64: for r value j (in the caller's order) a block [G][2][cap_j] of LOCAL node ids, row 0 the
 *           sources and row 1 the destinations, with cap_j = min(2 n r_j, n (n - 1)) for the clamped r_j; block j starts
 *           at element sum over j' < j of 2 G cap_j'.  Entries at or beyond counts[j][g] are LEFT UNTOUCHED.
 * counts    device int32 [n_r][G]: the number of edges of graph g for r value j (<= cap_j).
 *
 * One workgroup per graph: the MT state is regenerated block by block in LDS (three lane-parallel dependency phases per
 * 624 words), the draws that fall into a node's used window are kept as one byte each, the Fisher-Yates prefixes run one
 * node per lane on byte arrays in LDS, and for the r values in ascending order the new target columns are added to an
 * adjacency bitmap in LDS whose rows are then enumerated (popcount, prefix sum, write).  Integer work only: two calls
 * give identical bits.
 *
 * n_nodes < 2: ISIC_OK, every count 0, edges untouched.  n_nodes > ISIC_RANDGRAPH_MAX_NODES, n_r > ISIC_RANDGRAPH_MAX_R_VALUES
 * or n_r < 1: ISIC_ERR_UNSUPPORTED.  r_values NULL, G < 0, n_nodes < 0, seeds / edges / counts NULL with G > 0, seeds or
 * edges not 8-byte aligned, counts not 4-byte aligned: ISIC_ERR_BAD_ARG.  G == 0: ISIC_OK, nothing is launched.  Every
 * r in [1, n - 1] is supported for every n <= ISIC_RANDGRAPH_MAX_NODES. */
#ifndef ISIC_HIP_RANDGRAPH_H
#define ISIC_HIP_RANDGRAPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISIC_RANDGRAPH_MAX_NODES 256
#define ISIC_RANDGRAPH_MAX_R_VALUES 16
int isic_random_graph_i64(const int64_t* seeds, int G, int n_nodes, const int* r_values, int n_r, int64_t* edges,
                          int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_RANDGRAPH_H */
