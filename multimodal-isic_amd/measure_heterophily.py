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


def compute_edge_heterophily_batch(embeddings, patch_probs, dominant_class, edge_indices, device="cuda:0"):
    """A batch of images of equal node count: lists of ``patch_embeddings[N,D]``, ``patch_probs[N,C]``,
    ``dominant_class[N]`` and per-image ``edge_index[2,E_i]`` (local ids).  Returns one dict per image with the
    reference's keys (`04:163-170`)."""
    dev = torch.device(device)
    n_img = len(embeddings)
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
    ``num_edges``, the statistics, ``H_compat_matrix``), from a single copy to the host."""
    compat = summary["H_compat_matrix"]
    G, C = int(compat.shape[0]), int(compat.shape[-1])
    host = torch.cat([torch.stack([summary[k].to(torch.float64) for k in SUMMARY_STATS], dim=1), compat.reshape(G, C * C)],
                     dim=1).cpu().numpy()
    rows = []
    for i, meta in enumerate(metas):
        out = dict(meta)
        out["num_edges"] = int(host[i, 0])
        for j, k in enumerate(SUMMARY_STATS[1:], start=1):
            out[k] = float(host[i, j])
        out["H_compat_matrix"] = host[i, len(SUMMARY_STATS):].reshape(C, C)
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
