// The fast path of isic_knn_graph (graph.hip) for graphs of up to 208 nodes, defined in knn_gram.hip: the whole Gram matrix
// of a graph in one workgroup, the top-k selected out of the accumulators.
#pragma once
#include "common.h"

// every graph has 1 .. 208 nodes, D % 32 == 0, k <= 16 (the domain of knn_tile.inc)
bool isic_knn_gram_supported(int D, int k, int max_nodes);
// nn_dist may be NULL; the arguments are those of isic_knn_graph, checked by it
int isic_knn_gram_launch(const float* x, const int64_t* offsets, int G, int D, int k, int64_t* nn_idx, float* nn_dist,
                         hipStream_t stream);
