"""Heterophily measures of the patch graphs on the MI355X -- the numeric core of the reference's
``04_measure_heterophily.py`` (`compute_edge_heterophily`, `:107-169`; `_summarize_image`, `:172-181`).

Per image and graph variant the reference computes, on CPU numpy: per-edge KL divergence of the teacher's patch
class distributions, per-edge Dirichlet energy of the patch embeddings, per-edge lattice distance, the adjusted
homophily of the teacher's dominant classes, the class compatibility matrix and the algebraic connectivity
lambda_2 of the symmetrised graph.  Here the edge-wise row gathers run in one HIP launch per batch of images
(``isic_edge_heterophily_f32``); the class bookkeeping is integer index plumbing in torch on the device; lambda_2 is
one HIP launch per batch (``isic_laplacian_lambda2_f64``: a workgroup per graph, fp64 Householder + Sturm
multisection in LDS), with a dense ``torch.linalg.eigvalsh`` only for graphs above 196 nodes, which the kernel does
not take.  ``heterophily_summary_device`` gives the per-image summaries of `:172-181` as device tensors
(``isic_segment_stats_f32``).  The reference's plotting / aggregation code (`:229-589`) is out of scope.

Graphs of unequal size -- the subgraphs that lesion flags induce (``heterophily_summary_lesion_only``,
``compute_edge_heterophily_batch(keep=...)``) or any ragged record set (``heterophily_summary_ragged``) -- go through the
entries of ``include/isic_hip_hetero_ragged.h``: local node ids, a lattice position per node, the class bookkeeping and the
self-loop compaction inside HIP kernels, up to 196 nodes per graph.  The equal-size path above is unchanged.
"""
from __future__ import annotations

import re

import numpy as np
import torch

from isic_hip import spectral
from isic_hip.lib import IsicHipError, call

EPS = 1e-8                                                        # 04:11
MEASURES = ["H_kl", "H_dirichlet", "H_spatial", "H_adj", "lambda_2"]
GRAPH_VARIANT_RE = re.compile(r"^(?P<kind>grid4|grid8|knn|random)(?P<param>\d+)?$")
GRID_W = 14                                                       # 04:124-125 (% 14, // 14)


def edge_index_from_variant(row, graph_variant):
    """`_edge_index_from_variant` (04:87-104)."""
    m = GRAPH_VARIANT_RE.match(graph_variant)
    if not m:
        raise ValueError(f"Unsupported graph variant: {graph_variant}")
    kind, param = m.group("kind"), m.group("param")
    get = (lambda k: row[k]) if isinstance(row, dict) else (lambda k: getattr(row, k))
    if kind == "grid4":
        return np.asarray(get("grid4_edge_index"))
    if kind == "grid8":
        return np.asarray(get("grid8_edge_index"))
    if kind == "knn":
        return np.asarray(get("knn_edge_indices")[int(param)])
    return np.asarray(get("random_edge_indices")[int(param)])


def edge_measures(x, probs, dominant, edge_index, nodes_per_graph, grid_w=GRID_W, eps=EPS):
    """Device tensors of a batch of graphs -> (H_kl, H_dirichlet, H_spatial, same_class) per edge [E] (fp32), for
    ALL edges of ``edge_index[2, E]`` (global node ids; the caller drops self loops)."""
    for t in (x, probs, dominant, edge_index):
        if not t.is_cuda:
            raise IsicHipError("measure_heterophily runs on the MI355X only (no CPU fallback)")
    x = x.contiguous().float()
    probs = probs.contiguous().float()
    dom = dominant.contiguous().to(torch.int32)
    ei = edge_index.contiguous().to(torch.int64)
    E = int(ei.shape[1])
    out = torch.empty((4, E), device=x.device, dtype=torch.float32)
    call("isic_edge_heterophily_f32", x, probs, dom, ei[0], ei[1], E, int(x.shape[1]), int(probs.shape[1]), int(grid_w),
         int(nodes_per_graph), float(eps), out[0], out[1], out[2], out[3])
    return out[0], out[1], out[2], out[3]


def _lambda2_eigvalsh(src, dst, n_graphs, nodes, weight=None):
    """Dense fp64 Laplacians + ``torch.linalg.eigvalsh``: the path for graphs above ``spectral.MAX_NODES`` nodes.
    ``weight`` (default 1 per edge) lets a caller pass self loops with weight 0 instead of filtering them."""
    dev = src.device
    A = torch.zeros((n_graphs * nodes, nodes), device=dev, dtype=torch.float64)
    # duplicated edges count with their multiplicity: scipy's COO -> CSR conversion sums them (04:151-152)
    w = torch.ones(src.numel(), device=dev, dtype=torch.float64) if weight is None else weight.to(torch.float64)
    A.index_put_((src, dst % nodes), w, accumulate=True)
    A = A.view(n_graphs, nodes, nodes)
    A = torch.maximum(A, A.transpose(1, 2))
    deg = A.sum(dim=2)
    dis = torch.where(deg > 0, deg.clamp_min(1e-300).rsqrt(), torch.zeros_like(deg))
    L = torch.eye(nodes, device=dev, dtype=torch.float64).unsqueeze(0) - dis.unsqueeze(2) * A * dis.unsqueeze(1)
    ev = torch.linalg.eigvalsh(L)
    return ev[:, 1] if nodes > 1 else torch.zeros(n_graphs, device=dev, dtype=torch.float64)


def lambda2_batch(src, dst, n_graphs, nodes):
    """Second-smallest eigenvalue of I - D^-1/2 max(A, A^T) D^-1/2 per graph (04:150-159) [n_graphs] fp64; src/dst are
    global ids of the self-loop-free edges.  HIP kernel up to ``spectral.MAX_NODES`` nodes, eigvalsh above."""
    if nodes > spectral.MAX_NODES:
        return _lambda2_eigvalsh(src, dst, n_graphs, nodes)
    # the kernel takes each graph's edges as one segment: order them by graph (stable, so any order is accepted); an id
    # outside [0, n_graphs * nodes) lands in the first / last graph, which the kernel then reports as NaN
    gid, order = torch.sort(torch.div(src, nodes, rounding_mode="floor").clamp(0, max(0, n_graphs - 1)), stable=True)
    offsets = torch.searchsorted(gid, torch.arange(n_graphs + 1, device=src.device, dtype=gid.dtype))
    return spectral.laplacian_lambda2(src[order], dst[order], offsets, n_graphs, nodes)


def _device_measures(x, p, dom, ei, counts, n_img, N):
    """The device part shared by ``compute_edge_heterophily_batch`` and ``heterophily_summary_device``.
    x[n_img*N, D], p[n_img*N, C] fp32, dom[n_img*N] int32, ei[2, E] global ids in image order, ``counts`` the host-known
    edge count of every image.  Self loops (04:117-118) are masked, not removed, so nothing here waits for the device:
    returns the per-edge measures [3, E] (H_kl, H_dirichlet, H_spatial) of ALL edges, the keep mask, the
    image of every edge, and per image num_edges, H_adj, the compatibility matrix and lambda_2."""
    dev = x.device
    C = int(p.shape[1])
    E = int(ei.shape[1])
    gid = torch.repeat_interleave(torch.arange(n_img, device=dev), torch.as_tensor(counts, device=dev), output_size=E)
    kl, dirich, spatial, same = edge_measures(x, p, dom, ei, N)
    src, dst = ei[0], ei[1]
    keep = src != dst                                                  # 04:117-118
    kf = keep.to(torch.float64)
    n_edges = torch.zeros(n_img, device=dev, dtype=torch.int64).index_add_(0, gid, keep.to(torch.int64))
    edge_h = torch.zeros(n_img, device=dev, dtype=torch.float64).index_add_(0, gid, same.double() * kf) / n_edges.clamp_min(1)
    pk = torch.zeros((n_img, C), device=dev, dtype=torch.float64)
    pk.index_put_((torch.arange(n_img * N, device=dev) // N, dom.long()), torch.ones(n_img * N, device=dev, dtype=torch.float64),
                  accumulate=True)
    pk /= max(1, N)
    expected = (pk * pk).sum(dim=1)
    # an image without edges has edge_h = 0 (04:131: the mean of an empty edge set is taken as 0.0)
    h_adj = torch.where(expected < 1.0, (edge_h - expected) / (1.0 - expected).clamp_min(1e-300), torch.ones_like(expected))
    compat = torch.zeros((n_img, C, C), device=dev, dtype=torch.float64)
    compat.index_put_((gid, dom[src].long(), dom[dst].long()), kf, accumulate=True)
    rs = compat.sum(dim=2, keepdim=True)
    compat = torch.where(rs != 0, compat / rs.clamp_min(1e-300), torch.zeros_like(compat))
    if N <= spectral.MAX_NODES:
        offsets = torch.as_tensor([0] + list(np.cumsum(counts)), device=dev, dtype=torch.int64)
        lam2 = spectral.laplacian_lambda2(src, dst, offsets, n_img, N)      # skips the self loops itself
    else:
        lam2 = _lambda2_eigvalsh(src, dst, n_img, N, weight=kf)
    return {"values": torch.stack([kl, dirich, spatial]), "keep": keep, "gid": gid, "num_edges": n_edges,
            "H_adj": h_adj, "expected": expected, "H_compat_matrix": compat, "lambda_2": lam2}


def _ragged_measures(x, probs, dominant, edge_index, edge_offsets, node_offsets, patch_pos, max_nodes, grid_w=GRID_W, eps=EPS):
    """The device part of the ragged path (include/isic_hip_hetero_ragged.h), four launches and a cumsum, nothing read back:
    x[T,D], probs[T,C] fp32, dominant[T], edge_index[2,E] LOCAL ids, edge_offsets / node_offsets [G+1], patch_pos[T] or None.
    Returns ``values`` [3,E] fp32 -- H_kl, H_dirichlet, H_spatial of the edges with src != dst, graph g's at columns
    ``kept_offsets[g]:kept_offsets[g+1]`` in their input order --, ``kept_offsets`` [G+1], and per graph ``num_edges``,
    ``H_adj``, ``expected``, ``H_compat_matrix``, ``lambda_2`` and ``bad`` (non-zero: invalid input, NaN results)."""
    for t in (x, probs, dominant, edge_index, edge_offsets, node_offsets) + (() if patch_pos is None else (patch_pos,)):
        if not t.is_cuda:
            raise IsicHipError("the ragged heterophily path takes device tensors (no CPU fallback)")
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must be [2, E]")
    dev = x.device
    x = x.contiguous().float()
    probs = probs.contiguous().float()
    dom = dominant.contiguous().to(torch.int32)
    ei = edge_index.contiguous().to(torch.int64)
    eoff, noff = edge_offsets.contiguous().to(torch.int64), node_offsets.contiguous().to(torch.int64)
    pos = None if patch_pos is None else patch_pos.contiguous().to(torch.int32)
    T, D, C, E, G = int(x.shape[0]), int(x.shape[1]), int(probs.shape[1]), int(ei.shape[1]), int(noff.numel()) - 1
    if G < 0 or eoff.numel() != G + 1:
        raise ValueError("edge_offsets and node_offsets must both have G + 1 entries")
    if probs.shape[0] != T or dom.numel() != T or (pos is not None and pos.numel() != T):
        raise ValueError("x, probs, dominant and patch_pos must have one row per node")
    # first: the launch that refuses graphs above spectral.MAX_NODES
    lam2 = spectral.laplacian_lambda2_ragged(ei[0], ei[1], eoff, noff, max_nodes)
    per_edge = torch.empty((4, E), device=dev, dtype=torch.float32)
    call("isic_edge_heterophily_ragged_f32", x, probs, dom, pos, ei[0], ei[1], eoff, noff, None, G, T, E, D, C, int(grid_w),
         float(eps), per_edge[0], per_edge[1], per_edge[2], per_edge[3])
    kept_offsets = torch.zeros(G + 1, device=dev, dtype=torch.int64)
    h_adj = torch.empty(G, device=dev, dtype=torch.float64)
    expected = torch.empty(G, device=dev, dtype=torch.float64)
    compat = torch.empty((G, C, C), device=dev, dtype=torch.float64)
    bad = torch.zeros(G, device=dev, dtype=torch.int32)                      # (uint32 on the device side)
    num_edges = torch.empty(G, device=dev, dtype=torch.int64)
    call("isic_graph_homophily_ragged", dom, ei[0], ei[1], eoff, noff, G, T, E, C, num_edges, h_adj, expected, compat, bad)
    torch.cumsum(num_edges, 0, out=kept_offsets[1:])
    values = torch.zeros((3, E), device=dev, dtype=torch.float32)
    call("isic_edge_values_compact_ragged_f32", per_edge, ei[0], ei[1], eoff, kept_offsets, G, 3, E, values)
    return {"values": values, "kept_offsets": kept_offsets, "num_edges": num_edges, "H_adj": h_adj, "expected": expected,
            "H_compat_matrix": compat, "lambda_2": lam2, "bad": bad}


def heterophily_summary_ragged(x, probs, dominant, edge_index, edge_offsets, node_offsets, patch_pos=None, max_nodes=None):
    """``heterophily_summary_device`` for graphs of unequal size, described as ``graph.induced_subgraphs`` returns them:
    ``x[T,D]``, ``probs[T,C]``, ``dominant[T]``, ``edge_index[2,E]`` with LOCAL node ids, ``edge_offsets`` and
    ``node_offsets`` ``[G+1]`` int64 -- device tensors.  ``patch_pos[T]`` is every node's position on the 14-wide lattice
    (the ``rows`` of an induced subgraph; None: the local id).  ``max_nodes`` is a host-known bound on the node counts; left
    out, it is read back from ``node_offsets`` (the only copy to the host).  Graphs above ``spectral.MAX_NODES`` nodes raise
    ``IsicHipError`` with code -2.  Returns the dict of ``heterophily_summary_device`` plus ``num_nodes`` [G] int64; a graph
    with an endpoint or class out of range or offsets outside the arrays gets NaN and ``num_edges`` 0."""
    noff = node_offsets.to(torch.int64)
    num_nodes = noff[1:] - noff[:-1]
    if max_nodes is None:
        max_nodes = int(num_nodes.max()) if num_nodes.numel() else 0
    rm = _ragged_measures(x, probs, dominant, edge_index, edge_offsets, node_offsets, patch_pos, int(max_nodes))
    E = int(rm["values"].shape[1])
    # a segment above the kernel's limit gets NaN from the kernel itself, so E is bound enough
    mean, std, median = spectral.segment_stats(rm["values"], rm["kept_offsets"], min(E, spectral.MAX_SEGMENT))
    out = {"num_edges": rm["num_edges"], "num_nodes": num_nodes}
    for i, m in enumerate(MEASURES[:3]):
        out[f"{m}_mean"], out[f"{m}_std"], out[f"{m}_median"] = mean[i], std[i], median[i]
    for m in ("H_adj", "lambda_2"):                                   # one value per image: std 0, median = mean
        v = rm[m]
        out[f"{m}_mean"], out[f"{m}_std"], out[f"{m}_median"] = v, torch.zeros_like(v), v.clone()
    out["H_compat_matrix"] = rm["H_compat_matrix"]
    return out


def _concat_local_edges(edge_index, G, dev):
    """``[G,2,E]`` or a list of ``[2,E_i]`` (local ids, device tensors) -> (edge_index [2, sum E_i], edge_offsets [G+1])."""
    if isinstance(edge_index, torch.Tensor):
        if not edge_index.is_cuda or edge_index.dim() != 3 or edge_index.shape[0] != G:
            raise IsicHipError("edge_index: a device tensor [G, 2, E] or one device tensor [2, E_i] per image")
        E = int(edge_index.shape[2])
        return (edge_index.to(torch.int64).permute(1, 0, 2).reshape(2, G * E),
                torch.arange(G + 1, device=dev, dtype=torch.int64) * E)
    if len(edge_index) != G or not all(e.is_cuda for e in edge_index):
        raise IsicHipError("edge_index: one device tensor [2, E_i] per image")
    counts = [int(e.shape[1]) for e in edge_index]
    ei = torch.cat([e.to(torch.int64) for e in edge_index], dim=1) if G else torch.zeros((2, 0), device=dev, dtype=torch.int64)
    return ei, torch.as_tensor([0] + list(np.cumsum(counts)), dtype=torch.int64).to(dev)


def _induce(x, probs, dominant, ei, eoff, noff, keep):
    """Flat node tensors ``[T, .]`` of a record set and its lesion flags ``keep[T]`` -> the arguments of the ragged path for
    the induced graphs: ``graph.induced_subgraphs``, then ONE gather of the three node tensors by ``rows``."""
    from isic_hip.graph import induced_subgraphs
    ei2, eoff2, noff2, rows = induced_subgraphs(ei, eoff, noff, keep)
    G = int(noff.numel()) - 1
    gid = torch.repeat_interleave(torch.arange(G, device=rows.device), noff2[1:] - noff2[:-1], output_size=int(rows.numel()))
    idx = noff[gid] + rows
    return x[idx], probs[idx], dominant[idx], ei2, eoff2, noff2, rows


def heterophily_summary_lesion_only(x, probs, dominant, edge_index, keep):
    """``heterophily_summary_device`` of the subgraphs that the lesion flags induce: ``x[G,N,D]``, ``probs[G,N,C]``,
    ``dominant[G,N]``, ``edge_index`` ``[G,2,E]`` or a list of ``[2,E_i]`` (local ids), ``keep[G,N]`` (non-zero = lesion
    patch; an image without a set flag keeps every node, as ``graph.induced_subgraphs`` defines) -- device tensors.  The
    kept patches keep their place on the lattice (H_spatial); everything else is measured on the induced graph.  Returns
    ``heterophily_summary_ragged``'s dict (``num_nodes``: the kept patches of every image)."""
    for t in (x, probs, dominant, keep):
        if not t.is_cuda:
            raise IsicHipError("heterophily_summary_lesion_only takes device tensors (no CPU fallback)")
    G, N, D = (int(s) for s in x.shape)
    if tuple(keep.shape) != (G, N):
        raise ValueError("keep must be [G, N]")
    if N > spectral.MAX_NODES:
        raise IsicHipError(f"the ragged heterophily path takes graphs of at most {spectral.MAX_NODES} nodes", code=-2)
    dev = x.device
    ei, eoff = _concat_local_edges(edge_index, G, dev)
    noff = torch.arange(G + 1, device=dev, dtype=torch.int64) * N
    xs, ps, ds, ei2, eoff2, noff2, rows = _induce(x.reshape(G * N, D), probs.reshape(G * N, -1), dominant.reshape(G * N), ei,
                                                  eoff, noff, keep.reshape(G * N))
    return heterophily_summary_ragged(xs, ps, ds, ei2, eoff2, noff2, patch_pos=rows, max_nodes=N)


def heterophily_summary_lesion_knn(x, probs, dominant, keep, k):
    """``heterophily_summary_lesion_only`` on the k-NN graph built AMONG the lesion patches of every image instead of the
    subgraph they induce in a k-NN graph over all patches (which loses every edge to a background patch): ``x[G,N,D]``,
    ``probs[G,N,C]``, ``dominant[G,N]`` device tensors, ``keep[G,N]`` (non-zero = lesion patch, host or device; an image
    without a set flag keeps every node).  The kept rows are gathered once, their neighbours come from one top-k launch
    and the edge list from one more (``isic_hip.graph.knn_indices_ragged`` / ``knn_edges_ragged``: every image with the
    reference's own clamp max(1, min(k, n - 1)), `03_build_graphs.py:42-45`, no edge below 2 kept patches); the kept
    patches keep their place on the lattice.  Returns ``heterophily_summary_ragged``'s dict: ``num_edges`` is n * k_clamped
    per image.  The flags are read on the host (the sizes of the launches follow from them)."""
    from isic_hip.graph import knn_edges_ragged, knn_indices_ragged
    xs, ps, ds, rows, offs, N = _gather_kept_patches(x, probs, dominant, keep, "heterophily_summary_lesion_knn")
    k = int(k)
    nn = knn_indices_ragged(xs, offs, max(1, min(k, offs.max_bag - 1)))
    ei, eoff = knn_edges_ragged(nn, offs, [k])[k]
    return heterophily_summary_ragged(xs, ps, ds, ei.contiguous(), torch.as_tensor(eoff).to(x.device), offs.device,
                                      patch_pos=rows, max_nodes=N)


def heterophily_summary_lesion_random(x, probs, dominant, keep, r, seeds):
    """The twin of ``heterophily_summary_lesion_knn`` for a ``random<r>`` variant: the reference's random graph built AMONG
    the lesion patches of every image, ``_random_edge_index(kept patches, r, seeds[g])`` bit for bit
    (`03_build_graphs.py:57-78`: r clamped by the image's own number of kept patches, no edge below 2 of them), instead of
    the subgraph they induce in the random graph over all patches (which keeps a neighbour with probability
    (kept - 1) / (all - 1) only).  ``seeds``: one Python int per image (`03:136`).  The kept rows are gathered once and
    the edge lists come from ``isic_hip.graph.random_graphs_ragged``; the kept patches keep their place on the lattice.
    Returns ``heterophily_summary_ragged``'s dict.  The flags are read on the host."""
    from isic_hip.graph import random_graphs_ragged
    xs, ps, ds, rows, offs, N = _gather_kept_patches(x, probs, dominant, keep, "heterophily_summary_lesion_random")
    if len(seeds) != offs.num_bags:
        raise ValueError("seeds: one per image")
    r = int(r)
    ei, eoff = random_graphs_ragged([int(s) for s in seeds], offs, [r])[r]
    return heterophily_summary_ragged(xs, ps, ds, ei.contiguous(), torch.as_tensor(eoff).to(x.device), offs.device,
                                      patch_pos=rows, max_nodes=N)


def _gather_kept_patches(x, probs, dominant, keep, who):
    """``x[G,N,D]``, ``probs[G,N,C]``, ``dominant[G,N]`` restricted to the rows ``keep[G,N]`` flags (an image without a set
    flag keeps every node) -> (x', probs', dominant', lattice position of every kept row, their BagOffsets, N)."""
    from isic_hip.bags import BagOffsets
    for t in (x, probs, dominant):
        if not t.is_cuda:
            raise IsicHipError(f"{who} takes device tensors (no CPU fallback)")
    G, N, D = (int(s) for s in x.shape)
    kh = np.asarray(keep.cpu() if isinstance(keep, torch.Tensor) else keep).reshape(-1) != 0
    if kh.size != G * N:
        raise ValueError("keep must be [G, N]")
    if N > spectral.MAX_NODES:
        raise IsicHipError(f"the ragged heterophily path takes graphs of at most {spectral.MAX_NODES} nodes", code=-2)
    kh = kh.reshape(G, N).copy()
    kh[~kh.any(axis=1)] = True
    dev = x.device
    flat = np.flatnonzero(kh.reshape(-1)).astype(np.int64)
    idx = torch.as_tensor(flat).to(dev)
    rows = torch.as_tensor(flat % max(N, 1)).to(dev)
    offs = BagOffsets.from_lengths(kh.sum(axis=1), dev)
    xs = x.reshape(G * N, D)[idx].float().contiguous()
    return xs, probs.reshape(G * N, -1)[idx], dominant.reshape(G * N)[idx], rows, offs, N


def _edge_heterophily_batch_ragged(embeddings, patch_probs, dominant_class, edge_indices, keep, dev):
    """``compute_edge_heterophily_batch`` through the ragged path: images of any node count, optionally induced by ``keep``."""
    n_img = len(embeddings)
    embs = [np.asarray(e, dtype=np.float32) for e in embeddings]
    ns = [int(e.shape[0]) for e in embs]
    if ns and max(ns) > spectral.MAX_NODES:
        raise IsicHipError(f"the ragged heterophily path takes graphs of at most {spectral.MAX_NODES} nodes", code=-2)
    cat = lambda arrs, dt: torch.as_tensor(np.concatenate([np.asarray(a, dtype=dt) for a in arrs])).to(dev)   # noqa: E731
    x, p, dom = cat(embs, np.float32), cat(patch_probs, np.float32), cat(dominant_class, np.int32)
    eis = [np.asarray(e, dtype=np.int64).reshape(2, -1) for e in edge_indices]
    ei = torch.as_tensor(np.concatenate(eis, axis=1)).to(dev)
    eoff = torch.as_tensor(np.concatenate([[0], np.cumsum([e.shape[1] for e in eis])]).astype(np.int64)).to(dev)
    noff = torch.as_tensor(np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)).to(dev)
    pos = None
    if keep is not None:
        if len(keep) != n_img or any(len(k) != n for k, n in zip(keep, ns)):
            raise ValueError("keep: one flag per node of every image")
        x, p, dom, ei, eoff, noff, pos = _induce(x, p, dom, ei, eoff, noff, cat(keep, np.bool_))
    rm = _ragged_measures(x, p, dom, ei, eoff, noff, pos, max(ns) if ns else 0)
    vals, bounds = rm["values"].cpu().numpy(), rm["kept_offsets"].cpu().numpy()
    h_adj, compat, lam = rm["H_adj"].cpu().numpy(), rm["H_compat_matrix"].cpu().numpy(), rm["lambda_2"].cpu().numpy()
    return [{"H_kl": vals[0, a:b], "H_dirichlet": vals[1, a:b], "H_spatial": vals[2, a:b], "H_adj": float(h_adj[i]),
             "lambda_2": np.array([float(lam[i])]), "H_compat_matrix": compat[i]}
            for i, (a, b) in enumerate(zip(bounds[:-1].tolist(), bounds[1:].tolist()))]


def compute_edge_heterophily_batch(embeddings, patch_probs, dominant_class, edge_indices, device="cuda:0", keep=None):
    """A batch of images: lists of ``patch_embeddings[N,D]``, ``patch_probs[N,C]``, ``dominant_class[N]`` and per-image
    ``edge_index[2,E_i]`` (local ids).  Returns one dict per image with the reference's keys (`04:163-170`).  With ``keep``
    (one flag array [N_i] per image: the lesion patches) the measures are those of the induced subgraphs, the surviving
    edges in the reference's order; that and images of unequal node count go through the ragged path (at most 196 nodes
    per image)."""
    dev = torch.device(device)
    n_img = len(embeddings)
    if keep is not None or len({int(np.asarray(e).shape[0]) for e in embeddings}) > 1:
        return _edge_heterophily_batch_ragged(embeddings, patch_probs, dominant_class, edge_indices, keep, dev)
    N = int(np.asarray(embeddings[0]).shape[0])
    C = int(np.asarray(patch_probs[0]).shape[1])
    x = torch.as_tensor(np.stack([np.asarray(e, dtype=np.float32) for e in embeddings])).to(dev).view(n_img * N, -1)
    p = torch.as_tensor(np.stack([np.asarray(q, dtype=np.float32) for q in patch_probs])).to(dev).view(n_img * N, C)
    dom = torch.as_tensor(np.stack([np.asarray(d, dtype=np.int32) for d in dominant_class])).to(dev).view(-1)
    eis = [torch.as_tensor(np.asarray(e, dtype=np.int64)) for e in edge_indices]
    counts = [int(e.shape[1]) for e in eis]
    ei = torch.cat([e + i * N for i, e in enumerate(eis)], dim=1).to(dev)
    dm = _device_measures(x, p, dom, ei, counts, n_img, N)
    vals = dm["values"][:, dm["keep"]].cpu().numpy()
    kl_c, di_c, sp_c = vals[0], vals[1], vals[2]
    bounds = np.concatenate([[0], np.cumsum(dm["num_edges"].cpu().numpy())])
    h_adj_c, compat_c, lam_c = dm["H_adj"].cpu().numpy(), dm["H_compat_matrix"].cpu().numpy(), dm["lambda_2"].cpu().numpy()
    expected = dm["expected"]
    out = []
    for i in range(n_img):
        a, b = int(bounds[i]), int(bounds[i + 1])
        out.append({"H_kl": kl_c[a:b], "H_dirichlet": di_c[a:b], "H_spatial": sp_c[a:b],
                    "H_adj": float(h_adj_c[i]), "lambda_2": np.array([float(lam_c[i])]),
                    "H_compat_matrix": compat_c[i]})
        if b == a:                                                    # 04:131: mean of an empty edge set -> 0.0
            e0 = float(expected[i])
            out[-1]["H_adj"] = (0.0 - e0) / (1.0 - e0) if e0 < 1.0 else 1.0
    return out


def heterophily_summary_device(x, probs, dominant, edge_index):
    """The per-image summaries of `_summarize_image` (04:172-181) for a batch of images, on the device and without a
    copy to the host.  ``x[G,N,D]``, ``probs[G,N,C]``, ``dominant[G,N]`` as ``pipeline.DeviceTeacherOutputs`` holds them;
    ``edge_index`` ``[G,2,E]`` or a list of ``[2,E_i]`` (local ids).  Returns a dict of device tensors: ``num_edges``
    [G] int64, ``{H_kl,H_dirichlet,H_spatial,H_adj,lambda_2}_{mean,std,median}`` [G] fp64 (std = population std, an
    image without edges gets NaN for the per-edge measures, as numpy does) and ``H_compat_matrix`` [G,C,C] fp64."""
    for t in (x, probs, dominant):
        if not t.is_cuda:
            raise IsicHipError("heterophily_summary_device takes device tensors (no CPU fallback)")
    G, N, D = (int(s) for s in x.shape)
    C = int(probs.shape[2])
    dev = x.device
    if isinstance(edge_index, torch.Tensor):
        if not edge_index.is_cuda:
            raise IsicHipError("heterophily_summary_device takes device tensors (no CPU fallback)")
        E = int(edge_index.shape[2])
        counts = [E] * G
        off = (torch.arange(G, device=dev, dtype=torch.int64) * N).view(G, 1, 1)
        ei = (edge_index.to(torch.int64) + off).permute(1, 0, 2).reshape(2, G * E)
    else:
        if len(edge_index) != G or not all(e.is_cuda for e in edge_index):
            raise IsicHipError("edge_index: one device tensor [2, E_i] per image")
        counts = [int(e.shape[1]) for e in edge_index]
        ei = torch.cat([e.to(torch.int64) + i * N for i, e in enumerate(edge_index)], dim=1)
    dm = _device_measures(x.reshape(G * N, D).contiguous().float(), probs.reshape(G * N, C).contiguous().float(),
                          dominant.reshape(G * N).contiguous().to(torch.int32), ei, counts, G, N)
    # order-preserving compaction of the kept edges without a host round trip: edge e goes to column
    # (number of kept edges up to e) - 1; self loops go to a spare last column that no segment covers
    keep = dm["keep"]
    Et = int(ei.shape[1])
    dest = torch.where(keep, torch.cumsum(keep.to(torch.int64), 0) - 1, torch.full_like(dm["gid"], Et))
    vals = torch.zeros((3, Et + 1), device=dev, dtype=torch.float32).index_copy_(1, dest, dm["values"])
    offsets = torch.cat([torch.zeros(1, device=dev, dtype=torch.int64), torch.cumsum(dm["num_edges"], 0)])
    mean, std, median = spectral.segment_stats(vals, offsets, max(counts) if counts else 0)
    out = {"num_edges": dm["num_edges"]}
    for i, m in enumerate(MEASURES[:3]):
        out[f"{m}_mean"], out[f"{m}_std"], out[f"{m}_median"] = mean[i], std[i], median[i]
    for m in ("H_adj", "lambda_2"):                                   # one value per image: std 0, median = mean
        v = dm[m].to(torch.float64)
        out[f"{m}_mean"], out[f"{m}_std"], out[f"{m}_median"] = v, torch.zeros_like(v), v.clone()
    out["H_compat_matrix"] = dm["H_compat_matrix"]
    return out


SUMMARY_STATS = ["num_edges"] + [f"{m}_{s}" for m in MEASURES for s in ("mean", "std", "median")]


def summary_records(summary, metas):
    """A ``heterophily_summary_device`` result -> one dict per image in ``summarize_image``'s layout (the meta keys,
    ``num_edges``, the statistics, ``H_compat_matrix``), from a single copy to the host.  A result of the ragged path
    (``heterophily_summary_ragged`` / ``_lesion_only``) gives the same records with ``num_nodes`` after ``num_edges``."""
    compat = summary["H_compat_matrix"]
    G, C = int(compat.shape[0]), int(compat.shape[-1])
    cols = [summary[k].to(torch.float64) for k in SUMMARY_STATS] + \
        ([summary["num_nodes"].to(torch.float64)] if "num_nodes" in summary else [])
    host = torch.cat([torch.stack(cols, dim=1), compat.reshape(G, C * C)], dim=1).cpu().numpy()
    rows = []
    for i, meta in enumerate(metas):
        out = dict(meta)
        out["num_edges"] = int(host[i, 0])
        if "num_nodes" in summary:
            out["num_nodes"] = int(host[i, len(SUMMARY_STATS)])
        for j, k in enumerate(SUMMARY_STATS[1:], start=1):
            out[k] = float(host[i, j])
        out["H_compat_matrix"] = host[i, len(cols):].reshape(C, C)
        rows.append(out)
    return rows


def compute_edge_heterophily(row, graph_variant=None, device="cuda:0"):
    """Drop-in for the reference function (04:107): one image (a row with ``patch_embeddings``, ``patch_probs``,
    ``dominant_class`` and either ``edge_index`` or the 03 graph columns)."""
    get = (lambda k: row[k]) if isinstance(row, dict) else (lambda k: getattr(row, k))
    ei = np.asarray(get("edge_index")) if graph_variant is None else edge_index_from_variant(row, graph_variant)
    return compute_edge_heterophily_batch([get("patch_embeddings")], [get("patch_probs")], [get("dominant_class")], [ei],
                                          device=device)[0]


def summarize_image(em, meta):
    """`_summarize_image` (04:172-181)."""
    out = dict(meta)
    out["num_edges"] = len(em["H_kl"])
    for m in MEASURES:
        vals = em[m]
        out[f"{m}_mean"] = float(np.mean(vals))
        out[f"{m}_std"] = float(np.std(vals))
        out[f"{m}_median"] = float(np.median(vals))
    out["H_compat_matrix"] = em["H_compat_matrix"]
    return out
