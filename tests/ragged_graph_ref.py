"""Numpy restatement of the induced subgraphs of include/isic_hip_ragged.h: the definition the kernels are held to, bit for bit
(integers and copied floats), and itself checked against a per-edge loop in tests/test_ragged_graph_cpu.py."""
import numpy as np


def induced_subgraph(src, dst, keep, edge_weight=None):
    """One graph with LOCAL ids -> (src', dst', rows[, edge_weight'])."""
    src, dst, k = np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(keep) != 0
    k = k if k.any() else np.ones_like(k)               # an image without a lesion mask keeps every patch
    new = np.cumsum(k) - 1                              # compact local ids, order preserved
    m = k[src] & k[dst]                                 # both endpoints kept
    out = (new[src[m]], new[dst[m]], np.nonzero(k)[0])  # edge_index order preserved; old local id of every kept node
    return out + (np.asarray(edge_weight)[m],) if edge_weight is not None else out


def induced_subgraphs(src, dst, edge_offsets, node_offsets, keep, edge_weight=None):
    """A record set -> (edge_index' [2, E'], edge_offsets', node_offsets', rows[, edge_weight']), as graph.induced_subgraphs."""
    parts = [induced_subgraph(src[e0:e1], dst[e0:e1], keep[n0:n1], None if edge_weight is None else edge_weight[e0:e1])
             for e0, e1, n0, n1 in zip(edge_offsets[:-1], edge_offsets[1:], node_offsets[:-1], node_offsets[1:])]
    cat = lambda j, dt: np.concatenate([p[j] for p in parts]).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
    off = lambda j: np.concatenate([[0], np.cumsum([len(p[j]) for p in parts])]).astype(np.int64)        # noqa: E731
    out = (np.stack([cat(0, np.int64), cat(1, np.int64)]), off(0), off(2), cat(2, np.int64))
    return out + (cat(3, np.float32),) if edge_weight is not None else out
