"""Numpy definition of the heterophily measures on patch graphs of unequal size (include/isic_hip_hetero_ragged.h): per graph
``oracle.heterophily.edge_heterophily`` on the graph's own nodes and LOCAL edges -- for a lesion-only graph the induced
subgraph of tests/ragged_graph_ref.py --, with H_spatial recomputed from every node's lattice position ``patch_pos``
(04_measure_heterophily.py:120-121,165 uses the node id; on an induced graph the node id is no longer the patch).  Checked
against a per-edge loop and against the reference's own output in tests/test_hetero_ragged_cpu.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ragged_graph_ref as R  # noqa: E402
from oracle import heterophily as OH  # noqa: E402

MEASURES = ["H_kl", "H_dirichlet", "H_spatial", "H_adj", "lambda_2"]


def graph_measures(x, probs, dominant, edge_index, patch_pos=None):
    """One graph: x[n,D], probs[n,C], dominant[n], edge_index[2,E] local ids, patch_pos[n] (None: the node id) -> the
    reference's per-image dict (04:162-169) plus ``num_nodes``, ``num_edges`` and ``expected``."""
    ei = np.asarray(edge_index, np.int64).reshape(2, -1)
    dom = np.asarray(dominant, np.int32)
    n, c = len(dom), np.asarray(probs).shape[1]
    out = OH.edge_heterophily(np.asarray(x, np.float32).reshape(n, -1), np.asarray(probs, np.float32).reshape(n, c), dom, ei)
    pos = np.arange(n, dtype=np.int64) if patch_pos is None else np.asarray(patch_pos, np.int64)
    m = ei[0] != ei[1]                                                       # 04:115-116
    ps, pd = pos[ei[0][m]], pos[ei[1][m]]
    out["H_spatial"] = np.sqrt((ps % OH.GRID_W - pd % OH.GRID_W) ** 2 + (ps // OH.GRID_W - pd // OH.GRID_W) ** 2)
    out["num_nodes"], out["num_edges"] = n, int(m.sum())
    out["expected"] = float(np.sum((np.bincount(dom, minlength=c) / max(1, n)) ** 2))
    return out


def ragged_measures(x, probs, dominant, edge_index, edge_offsets, node_offsets, patch_pos=None):
    """A record set described as graph.induced_subgraphs returns it -> one ``graph_measures`` dict per graph."""
    ei = np.asarray(edge_index, np.int64)
    return [graph_measures(x[n0:n1], probs[n0:n1], dominant[n0:n1], ei[:, e0:e1], None if patch_pos is None else patch_pos[n0:n1])
            for e0, e1, n0, n1 in zip(edge_offsets[:-1], edge_offsets[1:], node_offsets[:-1], node_offsets[1:])]


def lesion_only_measures(x, probs, dominant, edge_index, keep):
    """One image x[N,D], ... with lesion flags keep[N]: the measures of the induced subgraph, the kept patches at their place
    on the lattice (an image without a set flag keeps every node)."""
    s2, d2, rows = R.induced_subgraph(edge_index[0], edge_index[1], keep)
    return graph_measures(np.asarray(x)[rows], np.asarray(probs)[rows], np.asarray(dominant)[rows], np.stack([s2, d2]), rows)


def summarize(em):
    """`_summarize_image` (04:172-181) of a ``graph_measures`` dict, with ``num_nodes``."""
    out = {"num_edges": em["num_edges"], "num_nodes": em["num_nodes"]}
    with np.errstate(all="ignore"):
        for m in MEASURES:
            v = np.asarray(em[m], np.float64).reshape(-1)
            out[f"{m}_mean"] = float(np.mean(v)) if v.size else float("nan")
            out[f"{m}_std"] = float(np.std(v)) if v.size else float("nan")
            out[f"{m}_median"] = float(np.median(v)) if v.size else float("nan")
    out["H_compat_matrix"] = em["H_compat_matrix"]
    return out
