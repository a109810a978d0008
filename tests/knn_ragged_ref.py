"""Torch-CPU restatement of the k-NN edge lists over graphs of unequal size (include/isic_hip_knn_ragged.h): the reference
builds them image by image on a frame that holds only the lesion patches (`03_build_graphs.py:37-54`), so the definition is
``oracle.graphs.knn_edge_index`` run per graph -- its own clamp k_g = max(1, min(k, n_g - 1)), no edge below 2 nodes -- and
the results concatenated with edge offsets."""
import numpy as np
import torch

from oracle import graphs


def knn_edges_ragged(x, offsets, k, global_ids=False):
    """x [T, D] (CPU), offsets [G+1] -> (edge_index int64 [2, E] with LOCAL ids (``global_ids``: plus the graph's first row),
    edge_offsets int64 [G+1]): graph g's list at columns edge_offsets[g]:edge_offsets[g+1], source-major."""
    offsets = np.asarray(offsets, dtype=np.int64)
    parts, counts = [], []
    for lo, hi in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
        e = graphs.knn_edge_index(x[lo:hi].float(), int(k))
        parts.append(e + (lo if global_ids else 0))
        counts.append(int(e.shape[1]))
    ei = torch.cat(parts, dim=1) if parts else torch.empty((2, 0), dtype=torch.long)
    return ei, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def keep_rows(keep):
    """Old local ids of the kept nodes; a graph without a kept node keeps every node (tests/ragged_graph_ref.py)."""
    keep = np.asarray(keep).reshape(-1) != 0
    return np.flatnonzero(keep if keep.any() else np.ones_like(keep))


def lesion_knn_record(x, keep, k):
    """One record of ``GraphStore(lesion_only=True, lesion_knn=k)``: (x[rows], edge_index among the kept rows, rows)."""
    rows = keep_rows(keep)
    xs = torch.as_tensor(np.asarray(x, dtype=np.float32))[torch.from_numpy(rows)]
    return xs, graphs.knn_edge_index(xs, int(k)), rows
