"""The random patch graphs over graphs of unequal size (include/isic_hip_randgraph_ragged.h) restated as a per-graph loop over
``rand_graph_ref`` -- MT19937 and Fisher-Yates written out, any n: each graph with its OWN node count, its own clamp of r to
[1, n - 1] (`03_build_graphs.py:61`), its own seed; the flat layout and the offsets of ``isic_hip.graph.random_graphs_ragged``.
Also the record ``train.GraphStore(lesion_only=True, lesion_random=r)`` holds for one input record."""
import os

import numpy as np

import rand_graph_ref as RR

# tests/golden/random_ragged.npz (tests/gen_random_ragged_golden.py): the reference's own _random_edge_index at these cases
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "random_ragged.npz")
GOLDEN_NODES = (2, 3, 5, 27, 33, 65)
GOLDEN_R = (1, 4, 16)
GOLDEN_SEEDS = (42, 10042)
GOLDEN_CASES = [(n, r, s) for n in GOLDEN_NODES for r in GOLDEN_R for s in GOLDEN_SEEDS]


def golden_key(n, r, seed):
    return f"n{n}.r{r}.s{seed}"


def random_graphs_ragged(seeds, sizes, r_values, global_ids=False):
    """-> {r: (edge_index int64 [2, E_r], edge_offsets int64 [G+1])}: graph g's edges for r are
    ``RR.random_edge_index(sizes[g], r, seeds[g])`` (none below 2 nodes), LOCAL ids or plus the graph's first row."""
    sizes = [int(n) for n in sizes]
    assert len(seeds) == len(sizes)
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = {}
    for r in dict.fromkeys(int(v) for v in r_values):
        parts, eo = [], [0]
        for g, (n, s) in enumerate(zip(sizes, seeds)):
            e = RR.graph(n, r, s) if n >= 2 else np.zeros((2, 0), dtype=np.int64)
            parts.append(e + (first[g] if global_ids else 0))
            eo.append(eo[-1] + e.shape[1])
        ei = np.concatenate(parts, axis=1) if parts else np.zeros((2, 0), dtype=np.int64)
        out[r] = (ei.astype(np.int64), np.asarray(eo, dtype=np.int64))
    return out


def random_edge_caps(sizes, r_values):
    """brute force, one (r, graph) at a time: min(2 n r_c, n (n - 1)), r_c = max(1, min(r, n - 1)); 0 below 2 nodes"""
    return np.asarray([[0 if n < 2 else min(2 * n * max(1, min(int(r), n - 1)), n * (n - 1)) for n in sizes] for r in r_values],
                      dtype=np.int64).reshape(len(list(r_values)), len(list(sizes)))


def lesion_random_record(x, keep, r, seed):
    """-> (x', rows, edge_index): the kept rows of ``x`` (all rows when no flag is set), their old local ids, and the random
    graph among them, ``_random_edge_index(len(rows), r, seed)``."""
    keep = np.asarray(keep).reshape(-1) != 0
    if not keep.any():
        keep = np.ones_like(keep)
    rows = np.flatnonzero(keep).astype(np.int64)
    n = int(rows.size)
    ei = RR.graph(n, r, seed) if n >= 2 else np.zeros((2, 0), dtype=np.int64)
    return np.asarray(x)[rows], rows, np.asarray(ei, dtype=np.int64)
