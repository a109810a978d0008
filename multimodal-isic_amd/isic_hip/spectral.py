"""Device launches of the heterophily stage's spectral and summary kernels (``csrc/spectral.hip``):

* ``laplacian_lambda2`` -- lambda_2 of the symmetrised normalised Laplacian per graph (``isic_laplacian_lambda2_f64``,
  04_measure_heterophily.py:149-159), one workgroup per graph, fp64; ``laplacian_lambda2_ragged`` is the same device code
  for graphs of unequal size with local ids (``isic_laplacian_lambda2_ragged_f64``);
* ``segment_stats`` -- mean / population std / median of contiguous segments (``isic_segment_stats_f32``,
  04_measure_heterophily.py:172-181), fp64 results.

Both take and return device tensors and never synchronise with the host."""
from __future__ import annotations

import torch

from .lib import IsicHipError, call

MAX_NODES = 196                   # ISIC_SPECTRAL_MAX_NODES (include/isic_hip.h)
MAX_SEGMENT = 16384               # ISIC_SEGMENT_MAX_LEN


def _dev(*ts):
    for t in ts:
        if not t.is_cuda:
            raise IsicHipError("the heterophily kernels run on the MI355X only (no CPU fallback)")


def laplacian_lambda2(src, dst, edge_offsets, n_graphs, nodes):
    """src/dst[E] int64 global node ids (g*nodes + local), edge_offsets[G+1] int64 -> lambda_2 [G] fp64.  Self loops are
    skipped by the kernel; a graph with an id outside it gets NaN.  nodes > MAX_NODES raises (code UNSUPPORTED)."""
    _dev(src, dst, edge_offsets)
    if edge_offsets.numel() != int(n_graphs) + 1:
        raise IsicHipError(f"edge_offsets has {edge_offsets.numel()} entries, expected {int(n_graphs) + 1}")
    out = torch.empty(int(n_graphs), device=edge_offsets.device, dtype=torch.float64)
    call("isic_laplacian_lambda2_f64", src.contiguous().to(torch.int64), dst.contiguous().to(torch.int64),
         edge_offsets.contiguous().to(torch.int64), int(n_graphs), int(nodes), out)
    return out


def laplacian_lambda2_ragged(src, dst, edge_offsets, node_offsets, max_nodes):
    """Graphs of unequal size (``isic_laplacian_lambda2_ragged_f64``): src/dst[E] int64 LOCAL node ids, edge_offsets and
    node_offsets [G+1] int64 -> lambda_2 [G] fp64.  ``max_nodes`` is a host-known bound on the node counts; a graph above it,
    with an id outside it or with offsets outside the arrays gets NaN, a graph of at most one node 0.0.
    max_nodes > MAX_NODES raises (code UNSUPPORTED)."""
    _dev(src, dst, edge_offsets, node_offsets)
    G = int(node_offsets.numel()) - 1
    if G < 0 or edge_offsets.numel() != G + 1:
        raise IsicHipError("edge_offsets and node_offsets must both have G + 1 entries")
    if src.numel() != dst.numel():
        raise IsicHipError("src and dst differ in length")
    out = torch.empty(G, device=edge_offsets.device, dtype=torch.float64)
    call("isic_laplacian_lambda2_ragged_f64", src.contiguous().to(torch.int64), dst.contiguous().to(torch.int64),
         edge_offsets.contiguous().to(torch.int64), node_offsets.contiguous().to(torch.int64), G, int(src.numel()),
         int(max_nodes), out)
    return out


def segment_stats(values, edge_offsets, max_segment):
    """values[M, E] fp32, edge_offsets[G+1] int64 (segments of the E columns), max_segment a host-known bound on the
    segment lengths -> (mean, std, median), each [M, G] fp64; an empty segment gives NaN."""
    _dev(values, edge_offsets)
    v = values.contiguous().float()
    if v.dim() != 2:
        raise IsicHipError("segment_stats takes values[M, E]")
    M, E = int(v.shape[0]), int(v.shape[1])
    G = int(edge_offsets.numel()) - 1
    outs = [torch.empty((M, G), device=v.device, dtype=torch.float64) for _ in range(3)]
    call("isic_segment_stats_f32", v, edge_offsets.contiguous().to(torch.int64), E, M, G, int(max_segment), *outs)
    return tuple(outs)
