"""Patch-graph structures and message-passing ops over libisic_hip (k-NN build,
destination-major CSR with GCN normalisation, CSR SpMM with autograd)."""
from __future__ import annotations

import torch

from .bags import BagOffsets
from .lib import ERR_UNSUPPORTED, IsicHipError, call
from .ops import _acc_target, _chk, _f32c, _grad_colsum, _grad_gemm, colsum


def _knn_launch(entry, x, offsets: BagOffsets, k, return_dist):
    """Checks, output allocation and the launch that ``isic_knn_graph`` and ``isic_knn_graph_ragged`` share; the former also
    takes a workspace of one float per node.  ``entry``: a name, or the rule that picks one once D is known."""
    _chk(x)
    x = _f32c(x)
    T, D = x.shape
    if T != offsets.total:
        raise ValueError(f"x has {T} rows but offsets cover {offsets.total}")
    if callable(entry):
        entry = entry(D)
    idx = torch.empty((T, k), device=x.device, dtype=torch.int64)
    dist = torch.empty((T, k), device=x.device, dtype=torch.float32) if return_dist else None
    ws = (torch.empty((T,), device=x.device, dtype=torch.float32),) if entry == "isic_knn_graph" else ()
    call(entry, x, offsets.device, offsets.num_bags, D, int(k), offsets.max_bag, T, idx, dist, *ws)
    return (idx, dist) if return_dist else idx


def knn_indices(x, offsets: BagOffsets, k, return_dist=False):
    """k nearest neighbours of every node inside its own graph -> LOCAL ids [T, k] (int64),
    ascending by distance (`03_build_graphs.py:46-50`)."""
    return _knn_launch("isic_knn_graph", x, offsets, k, return_dist)


KNN_RAGGED_MAX_NODES = 208
KNN_RAGGED_MAX_K = 16
KNN_RAGGED_MAX_GRAPHS = 1 << 22                 # one workgroup per graph
KNN_EDGES_MAX_K_VALUES = 16
# Whether knn_indices_ragged goes through isic_knn_graph_ragged where that entry supports the batch, and up to which mean
# number of 16 x 16 tiles per graph (ceil(n / 16)^2; 169 for the reference's 196 nodes): decided by the measurement of
# tools/knn_ragged_bench.py (profiles/knn_ragged_bench.txt, DESIGN.md "k-NN graphs among the lesion patches") -- the sized
# kernel wins on lesion-size batches (17 tiles) and up to 128 nodes (64 tiles) and is 2 % behind at 196 nodes (169).
KNN_RAGGED_USE_SIZED_KERNEL = True
KNN_RAGGED_MAX_MEAN_TILES = 64.0


def knn_ragged_supported(D, k, max_nodes):
    """What ``isic_knn_graph_ragged`` takes (include/isic_hip_knn_ragged.h)."""
    return D % 32 == 0 and D >= 32 and 1 <= k <= KNN_RAGGED_MAX_K and max_nodes <= KNN_RAGGED_MAX_NODES


def knn_indices_ragged(x, offsets: BagOffsets, k, return_dist=False):
    """``knn_indices`` for graphs of unequal size (the lesion patches of every image): LOCAL ids [T, k], -1 (distance +inf)
    where a graph has fewer than k other nodes; graphs of 0 or 1 node are legal.  Through ``isic_knn_graph_ragged`` -- the
    Gram kernel sized by each graph, bit-equal to ``knn_indices`` -- where that entry supports the batch (D % 32 == 0,
    k <= 16, up to 2^22 graphs of up to 208 nodes) and the graphs are small enough for it to be the faster one (on average at most
    ``KNN_RAGGED_MAX_MEAN_TILES`` tiles of 16 x 16 nodes), else through ``knn_indices``."""
    def entry(D):
        import numpy as np
        n = np.diff(offsets.host)
        tiles = float((((n + 15) // 16) ** 2).mean()) if n.size else 0.0
        sized = (KNN_RAGGED_USE_SIZED_KERNEL and tiles <= KNN_RAGGED_MAX_MEAN_TILES and offsets.num_bags <= KNN_RAGGED_MAX_GRAPHS
                 and knn_ragged_supported(D, int(k), offsets.max_bag))
        return "isic_knn_graph_ragged" if sized else "isic_knn_graph"

    return _knn_launch(entry, x, offsets, k, return_dist)


def knn_edge_counts(sizes, k_values):
    """-> int64 [K, G]: edges of graph g in the k-NN list of k_values[q], n_g * kk with the reference's per-image clamp
    kk = 0 if n_g < 2 else max(1, min(k, n_g - 1)) (`03_build_graphs.py:42-45`).  Host only."""
    import numpy as np
    n = np.asarray(sizes, dtype=np.int64).reshape(-1)
    ks = np.asarray([int(k) for k in k_values], dtype=np.int64).reshape(-1, 1)
    kk = np.where(n[None, :] < 2, 0, np.maximum(1, np.minimum(ks, n[None, :] - 1)))
    return n[None, :] * kk


def knn_edge_offsets(sizes, k_values):
    """-> {k: int64 [G+1]} the edge offsets of every k-NN list over graphs of ``sizes`` nodes (exclusive prefix sums of
    ``knn_edge_counts`` with the total appended).  Host only (numpy): the sizes are analytic, nothing is counted on the device."""
    import numpy as np
    cnt = knn_edge_counts(sizes, k_values)
    return {int(k): np.concatenate([[0], np.cumsum(cnt[q])]).astype(np.int64) for q, k in enumerate(k_values)}


def knn_edges_ragged(nn, offsets: BagOffsets, k_values, global_ids=False, check=True):
    """The k-NN edge lists of every k of ``k_values`` (1..16 distinct values) out of ONE neighbour table ``nn`` [T, kmax]
    (``knn_indices_ragged``), each graph with its own clamp kk = max(1, min(k, n_g - 1)) and no edge at all for a graph of
    fewer than 2 nodes (`03_build_graphs.py:42-53`): one launch (``isic_knn_edges_ragged``).
    -> ``{k: (edge_index [2, E_k], edge_offsets [G+1])}``: int64 views of ONE flat device buffer, source-major with the
    neighbours ascending by distance, LOCAL ids (``global_ids``: plus the graph's first row); ``edge_offsets`` is a host
    numpy array (``knn_edge_offsets``: the sizes are analytic, nothing is counted on the device).
    A k whose clamp exceeds ``nn``'s width in some graph is an ``IsicHipError`` (BAD_ARG) raised before the launch; with
    ``check`` the kernel's count of neighbour ids outside their graph (stored as -1) is read back (4 bytes) and a non-zero
    count is a ``ValueError``."""
    import ctypes

    import numpy as np
    ks = list(dict.fromkeys(int(k) for k in k_values))
    if not ks or len(ks) > KNN_EDGES_MAX_K_VALUES or min(ks) < 1:
        raise IsicHipError(f"knn_edges_ragged takes 1..{KNN_EDGES_MAX_K_VALUES} distinct k values >= 1, got {ks}", code=-1)
    if nn.dim() != 2 or nn.dtype != torch.int64 or not nn.is_cuda:
        raise IsicHipError("knn_edges_ragged needs a device int64 [T, kmax] neighbour table (no CPU fallback)")
    nn = nn.contiguous()
    T, kmax = int(nn.shape[0]), int(nn.shape[1])
    if T != offsets.total:
        raise ValueError(f"nn has {T} rows but offsets cover {offsets.total}")
    G = offsets.num_bags
    sizes = np.diff(offsets.host)
    cnt = knn_edge_counts(sizes, ks)                                        # [K, G]
    if G and int((cnt // np.maximum(sizes, 1)[None, :]).max()) > kmax:
        raise IsicHipError(f"isic_knn_edges_ragged failed: ISIC_ERR_BAD_ARG (a graph's clamped k exceeds the {kmax} "
                           f"neighbours per node of nn)", code=-1)
    base = np.zeros((len(ks), G + 1), dtype=np.int64)                       # absolute positions in the one flat output
    np.cumsum(cnt, axis=1, out=base[:, 1:])
    starts = np.concatenate([[0], np.cumsum(base[:, -1])])
    base += starts[:-1, None]
    total = int(starts[-1])
    flat = torch.empty((2, total), device=nn.device, dtype=torch.int64)
    bad = torch.zeros(1, device=nn.device, dtype=torch.int32)               # (uint32 on the device side)
    if total and G:
        kv = (ctypes.c_int32 * len(ks))(*ks)
        call("isic_knn_edges_ragged", nn, kmax, offsets.device, G, T, ctypes.addressof(kv), len(ks),
             torch.from_numpy(base).to(nn.device), total, 1 if global_ids else 0, flat[0], flat[1], bad)
        if check:
            n_bad = int(bad.item()) & 0xFFFFFFFF
            if n_bad:
                raise ValueError(f"knn_edges_ragged: {n_bad} neighbour id(s) outside their graph (stored as -1) or "
                                 "segments that do not fit their graph")
    return {k: (flat[:, int(starts[q]):int(starts[q + 1])], base[q] - starts[q]) for q, k in enumerate(ks)}


RANDOM_GRAPH_MAX_NODES = 256
RANDOM_GRAPH_MAX_R_VALUES = 16


def random_graph_launch(seeds, n_nodes, r_values, edges, counts):
    """The bare ``isic_random_graph_i64`` launch on buffers that exist: ``seeds`` int64 [G] on the device, ``edges`` int64
    (``random_graph_layout`` gives its size), ``counts`` int32 [len(r_values), G].  Nothing is read back."""
    import ctypes
    rs = (ctypes.c_int * len(r_values))(*[int(r) for r in r_values])
    call("isic_random_graph_i64", seeds, int(seeds.numel()), int(n_nodes), ctypes.addressof(rs), len(r_values), edges, counts)


def random_graph_layout(G, n_nodes, r_values):
    """-> ([(first element, cap_j)] per r value in the given order, total elements) of the ``edges`` buffer
    (include/isic_hip_randgraph.h): block j is [G][2][cap_j], cap_j = min(2 n r_j, n (n - 1)) for r_j clamped to [1, n - 1]."""
    n, blocks, at = int(n_nodes), [], 0
    for r in r_values:
        rc = max(1, min(int(r), n - 1))
        cap = min(2 * n * rc, n * (n - 1)) if n >= 2 else 0
        blocks.append((at, cap))
        at += 2 * int(G) * cap
    return blocks, at


def random_graphs(seeds, n_nodes, r_values, device=None):
    """The random graphs of `03_build_graphs.py:57-78` for G seeds and a list of r values, built on the device bit for bit
    as ``build_graphs._random_edge_index(n_nodes, r, seed)`` builds them on the host: ONE launch and ONE read-back (the
    edge counts).  ``seeds``: Python ints (only the low 32 bits matter, as for torch's CPU generator).  Returns
    ``{r: edges}``: a ``[G, 2, E]`` int64 tensor when every graph of that r has the same number of edges, else a list of
    ``[2, E_g]`` tensors -- views of the launch's buffer either way, LOCAL node ids, ascending by (src, dst)."""
    rs = list(dict.fromkeys(int(r) for r in r_values))
    n, G = int(n_nodes), len(seeds)
    if not rs or len(rs) > RANDOM_GRAPH_MAX_R_VALUES:
        raise IsicHipError(f"random_graphs takes 1..{RANDOM_GRAPH_MAX_R_VALUES} distinct r values, got {len(rs)}", code=-2)
    if n > RANDOM_GRAPH_MAX_NODES:
        raise IsicHipError(f"random_graphs supports up to {RANDOM_GRAPH_MAX_NODES} nodes, got {n}", code=-2)
    if not torch.cuda.is_available():
        raise IsicHipError("random_graphs needs the MI355X (the host build is build_graphs._random_edge_index)")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    blocks, total = random_graph_layout(G, n, rs)
    edges = torch.empty((total,), device=dev, dtype=torch.int64)
    if G == 0 or n < 2:
        return {r: edges.new_empty((G, 2, 0)) for r in rs}
    sd = torch.tensor([int(s) & 0xFFFFFFFF for s in seeds], dtype=torch.int64).to(dev)
    counts = torch.empty((len(rs), G), device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        random_graph_launch(sd, n, rs, edges, counts)
    cnt = counts.cpu().numpy()                                             # the one read-back
    out = {}
    for j, (r, (at, cap)) in enumerate(zip(rs, blocks)):
        block = edges[at:at + 2 * G * cap].view(G, 2, cap)
        es = cnt[j]
        if (es == es[0]).all():
            out[r] = block[:, :, :int(es[0])]
        else:
            out[r] = [block[g, :, :int(es[g])] for g in range(G)]
    return out


RANDOM_RAGGED_MAX_NODES = 256
RANDOM_RAGGED_MAX_R_VALUES = 16
# The packing of isic_random_graph_ragged_count / _write (include/isic_hip_randgraph_ragged.h): graphs of up to this many
# nodes take a wave each, four to a workgroup, with wave-level synchronisation only; larger graphs take a 256-lane
# workgroup each, in a second launch that is made only when the batch's largest graph exceeds it.  Measured by
# tools/rand_graph_ragged_bench.py (profiles/rand_graph_ragged_bench.txt, DESIGN.md "Random graphs among the lesion patches").
RANDOM_RAGGED_PACK_NODES = 64
RANDOM_RAGGED_GRAPHS_PER_WORKGROUP = 4


def random_edge_caps(sizes, r_values):
    """-> int64 [n_r, G]: the analytic upper bound on the edges of a random graph of ``sizes[g]`` nodes for ``r_values[j]``,
    min(2 n r_c, n (n - 1)) with the reference's per-graph clamp r_c = max(1, min(r, n - 1)) (`03_build_graphs.py:61`) and 0
    below 2 nodes.  Host only (numpy): for planning buffers; the exact counts need the draws (``random_graphs_ragged``)."""
    import numpy as np
    n = np.asarray(sizes, dtype=np.int64).reshape(1, -1)
    r = np.asarray([int(v) for v in r_values], dtype=np.int64).reshape(-1, 1)
    rc = np.maximum(1, np.minimum(r, n - 1))
    return np.where(n < 2, 0, np.minimum(2 * n * rc, n * (n - 1))).astype(np.int64)


def random_ragged_count_launch(seeds_dev, offsets: BagOffsets, r_values):
    """The bare ``isic_random_graph_ragged_count`` launch and the prefix sums the write needs, all on the device, nothing
    read back: -> (head int64 [n_r G + 1]: the counts [n_r, G] row-major and, in the low half of the last element, the
    kernels' uint32 count of bad graphs; bad: that count as a view; edge_off int64 [n_r, G + 1]: absolute positions in the
    one flat output, row j closing with row j + 1's start)."""
    import ctypes
    G, n_r = offsets.num_bags, len(r_values)
    dev = seeds_dev.device
    rv = (ctypes.c_int * n_r)(*[max(-1, min(int(r), 1 << 30)) for r in r_values])
    head = torch.zeros(n_r * G + 1, device=dev, dtype=torch.int64)
    counts, bad = head[:-1].view(n_r, G), head[-1:].view(torch.int32)
    call("isic_random_graph_ragged_count", seeds_dev, offsets.device, G, offsets.max_bag, ctypes.addressof(rv), n_r, counts, bad)
    ends = torch.cumsum(counts.reshape(-1), 0).view(n_r, G)
    edge_off = torch.empty((n_r, G + 1), device=dev, dtype=torch.int64)
    edge_off[:, 1:] = ends
    edge_off[0, 0] = 0
    edge_off[1:, 0] = ends[:-1, -1]
    return head, bad, edge_off


def random_ragged_write_launch(seeds_dev, offsets: BagOffsets, r_values, edge_off, flat, bad, global_ids=False):
    """The bare ``isic_random_graph_ragged_write`` launch into ``flat`` int64 [2, total]; nothing is read back."""
    import ctypes
    n_r, total = len(r_values), int(flat.shape[1])
    rv = (ctypes.c_int * n_r)(*[max(-1, min(int(r), 1 << 30)) for r in r_values])
    call("isic_random_graph_ragged_write", seeds_dev, offsets.device, offsets.num_bags, offsets.max_bag, ctypes.addressof(rv), n_r,
         edge_off, total, 1 if global_ids else 0, flat[0] if total else None, flat[1] if total else None, bad)


def random_graphs_ragged(seeds, offsets: BagOffsets, r_values, global_ids=False):
    """``random_graphs`` for graphs of unequal size (the lesion patches of every image): graph g has ``offsets``' g-th node
    count n_g and the seed ``seeds[g]`` (Python ints; the low 32 bits matter), and is, bit for bit,
    ``build_graphs._random_edge_index(n_g, r, seeds[g])`` -- r clamped to [1, n_g - 1] by the graph's OWN node count, no
    edge below 2 nodes.  -> ``{r: (edge_index [2, E_r], edge_offsets [G+1])}``: int64 views of ONE flat device buffer,
    ascending by (src, dst) inside each graph, LOCAL ids (``global_ids``: plus the graph's first row); ``edge_offsets`` is a
    host numpy array.  Two launches (``isic_random_graph_ragged_count`` / ``_write``) and ONE read-back, of the counts and
    the kernels' count of bad graphs; a non-zero one is a ``ValueError``.  Duplicate r values are collapsed."""
    import numpy as np
    rs = list(dict.fromkeys(int(r) for r in r_values))
    G = offsets.num_bags
    if not rs or len(rs) > RANDOM_RAGGED_MAX_R_VALUES:
        raise IsicHipError(f"random_graphs_ragged takes 1..{RANDOM_RAGGED_MAX_R_VALUES} distinct r values, got {len(rs)}", code=-2)
    if len(seeds) != G:
        raise ValueError(f"{len(seeds)} seeds for {G} graphs")
    if offsets.max_bag > RANDOM_RAGGED_MAX_NODES:
        raise IsicHipError(f"random_graphs_ragged supports up to {RANDOM_RAGGED_MAX_NODES} nodes per graph, got {offsets.max_bag}",
                           code=-2)
    if not offsets.device.is_cuda:
        raise IsicHipError("random_graphs_ragged needs the MI355X (the host build is build_graphs._random_edge_index)")
    dev = offsets.device.device
    if G == 0:
        flat = torch.empty((2, 0), device=dev, dtype=torch.int64)
        return {r: (flat, np.zeros(1, dtype=np.int64)) for r in rs}
    sd = torch.tensor([int(s) & 0xFFFFFFFF for s in seeds], dtype=torch.int64).to(dev)
    with torch.cuda.device(dev):
        head, bad, edge_off = random_ragged_count_launch(sd, offsets, rs)
        host = head.cpu().numpy()                                           # the one read-back
        n_bad = int(host[-1]) & 0xFFFFFFFF
        if n_bad:
            raise ValueError(f"random_graphs_ragged: {n_bad} graph(s) whose node offsets decrease, leave the node range or "
                             f"span more than {offsets.max_bag} nodes")
        cnt = host[:-1].reshape(len(rs), G)
        flat = torch.empty((2, int(cnt.sum())), device=dev, dtype=torch.int64)
        random_ragged_write_launch(sd, offsets, rs, edge_off, flat, bad, global_ids)
    ends = np.concatenate([[0], np.cumsum(cnt.sum(axis=1))])
    return {r: (flat[:, int(ends[j]):int(ends[j + 1])], np.concatenate([[0], np.cumsum(cnt[j])]).astype(np.int64))
            for j, r in enumerate(rs)}


def _dev_i64(v, device):
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=torch.int64).contiguous()
    import numpy as np
    return torch.as_tensor(np.asarray(v, dtype=np.int64)).to(device)


def induced_subgraphs(edge_index, edge_offsets, node_offsets, keep, edge_weight=None):
    """The subgraph induced by the kept nodes of every graph of a record set, in two launches and ONE read-back
    (include/isic_hip_ragged.h; tests/ragged_graph_ref.py restates it in numpy).  ``edge_index`` int64 [2, E] on the device
    with LOCAL node ids, graph g owning edges ``edge_offsets[g]:edge_offsets[g+1]`` and nodes ``node_offsets[g]:
    node_offsets[g+1]`` of ``keep`` ([T], non-zero = kept; a graph without a kept node keeps every node).  Returns
    ``(edge_index', edge_offsets', node_offsets', rows)`` -- device int64 tensors, compact LOCAL ids, edge order and node
    order preserved, ``rows`` [T'] the old LOCAL id of every kept node -- and the compacted ``edge_weight'`` as a fifth
    element when ``edge_weight`` is given.  An edge endpoint outside its graph is a ``ValueError`` raised before anything
    is written."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise ValueError("edge_index must be [2, E]")
    if not edge_index.is_cuda:
        raise IsicHipError("induced_subgraphs needs device tensors (no CPU fallback)")
    dev = edge_index.device
    ei = edge_index.to(torch.int64).contiguous()
    eoff, noff = _dev_i64(edge_offsets, dev), _dev_i64(node_offsets, dev)
    kp = keep if isinstance(keep, torch.Tensor) else torch.as_tensor(keep)
    kp = (kp != 0).to(device=dev, dtype=torch.uint8).contiguous()
    G, T, E = int(noff.numel()) - 1, int(kp.numel()), int(ei.shape[1])
    if G < 0 or eoff.numel() != G + 1:
        raise ValueError("edge_offsets and node_offsets must both have G + 1 entries")
    ew = _f32c(edge_weight) if edge_weight is not None else None
    if ew is not None and ew.numel() != E:
        raise ValueError("edge_weight must have one entry per edge")
    new_id = torch.empty(T, device=dev, dtype=torch.int32)
    counts = torch.zeros((2, G + 1), device=dev, dtype=torch.int64)        # row 0: kept nodes, row 1: kept edges; [G] stays 0
    bad = torch.zeros(G, device=dev, dtype=torch.int32)                     # (uint32 on the device side)
    call("isic_induced_subgraph_count", noff, eoff, ei[0], ei[1], kp, G, T, E, new_id, counts[0], counts[1], bad)
    # exclusive prefix sums with the totals appended: [0, c0, c0 + c1, ...]
    offs = torch.cumsum(counts, dim=1).roll(1, dims=1)
    offs[:, 0] = 0
    head = torch.cat([offs[:, -1], (bad != 0).sum().view(1)]).cpu().tolist()          # the one read-back: T', E', bad graphs
    t_out, e_out, n_bad = int(head[0]), int(head[1]), int(head[2])
    if n_bad:
        raise ValueError(f"induced_subgraphs: {n_bad} graph(s) have an edge endpoint outside [0, n) or offsets outside the arrays")
    ei_out = torch.empty((2, e_out), device=dev, dtype=torch.int64)
    rows = torch.empty(t_out, device=dev, dtype=torch.int64)
    ew_out = torch.empty(e_out, device=dev, dtype=torch.float32) if ew is not None else None
    call("isic_induced_subgraph_write", noff, eoff, ei[0], ei[1], ew, new_id, G, T, E, offs[0], offs[1], t_out, e_out,
         ei_out[0], ei_out[1], ew_out, rows)
    out = (ei_out, offs[1].clone(), offs[0].clone(), rows)
    return out + (ew_out,) if ew is not None else out


class GraphBatch:
    """Destination-major CSR (+ its transpose) of a batch of graphs with GCN symmetric
    normalisation and self loops (PyG ``gcn_norm`` semantics, `05_train_gnns.py:82`)."""

    MODES = {"gcn": 0, "sum": 1, "mean": 2}

    def __init__(self, edge_index, n_nodes, edge_weight=None, mode="gcn"):
        """mode 'gcn': self loops + symmetric normalisation (GCNConv / GCN2Conv); 'sum': plain neighbour
        sum (GINConv); 'mean': neighbour mean (SAGEConv).  'sum'/'mean' keep the edges as given."""
        if edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise ValueError("edge_index must be [2, E]")
        if not edge_index.is_cuda:
            raise IsicHipError("GraphBatch needs device tensors (no CPU fallback)")
        ei = edge_index.to(torch.int64).contiguous()
        E, n = int(ei.shape[1]), int(n_nodes)
        dev = ei.device
        ew = _f32c(edge_weight) if edge_weight is not None else None
        self.n_nodes, self.num_edges = n, E
        self.rowptr = torch.empty(n + 1, device=dev, dtype=torch.int32)
        self.col = torch.empty(E + n, device=dev, dtype=torch.int32)
        self.val = torch.empty(E + n, device=dev, dtype=torch.float32)
        self.rowptr_t = torch.empty(n + 1, device=dev, dtype=torch.int32)
        self.col_t = torch.empty(E + n, device=dev, dtype=torch.int32)
        self.val_t = torch.empty(E + n, device=dev, dtype=torch.float32)
        self.perm_t = torch.empty(E + n, device=dev, dtype=torch.int32)   # transposed slot -> CSR slot of the same edge
        nbytes = int(call("isic_gcn_csr_workspace_bytes", n, E))
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        self.mode = mode
        call("isic_gcn_csr_build", ei[0], ei[1], ew, E, n, self.MODES[mode], self.rowptr, self.col, self.val,
             self.rowptr_t, self.col_t, self.val_t, self.perm_t, ws, nbytes)


# The mode name of a ``GraphBatch`` whose CSR is symmetric with values of its own (an operator of ``two_hop``): no build
# produces it (``GraphBatch(..., mode="sym")`` is an error), only ``from_parts`` takes it; its ``_t`` arrays alias the forward
# ones and ``perm_t`` maps the slot of (i, j) to the slot of (j, i).
SYM_MODE = "sym"


def _graph_from_parts(n_nodes, num_edges, mode, parts):
    """A ``GraphBatch`` over CSR arrays that already exist on the device (no build launch): used by
    ``train.GraphStore`` to assemble a step's batch out of per-graph pieces built once.  ``mode``: a build mode, or
    ``"sym"`` for a symmetric operator that no build produces (``two_hop``)."""
    if mode not in GraphBatch.MODES and mode != SYM_MODE:
        raise ValueError(f"unknown graph mode '{mode}'")
    g = GraphBatch.__new__(GraphBatch)
    g.n_nodes, g.num_edges, g.mode = int(n_nodes), int(num_edges), mode
    for k in ("rowptr", "col", "val", "rowptr_t", "col_t", "val_t", "perm_t"):
        t = parts[k]
        want = torch.float32 if k.startswith("val") else torch.int32
        if not t.is_cuda or t.dtype != want:
            raise IsicHipError(f"GraphBatch.from_parts: {k} must be a device {want} tensor")
        setattr(g, k, t.contiguous())
    if g.rowptr.numel() != g.n_nodes + 1 or g.rowptr_t.numel() != g.n_nodes + 1:
        raise ValueError("rowptr must have n_nodes + 1 entries")
    return g


GraphBatch.from_parts = staticmethod(_graph_from_parts)


def _spmm_launch(graph, transposed, x, bias, out, alpha, addend, addend_scale):
    """One aggregation launch (forward CSR or its transpose)."""
    rp, c, v = (graph.rowptr_t, graph.col_t, graph.val_t) if transposed else (graph.rowptr, graph.col, graph.val)
    n, F = x.shape
    call("isic_spmm_csr_f32", rp, c, v, x, bias, out, n, F, alpha, addend, addend_scale)


class SpmmFn(torch.autograd.Function):
    """out = alpha * A^ x (+ bias) (+ addend_scale * addend); backward through the transposed CSR."""

    @staticmethod
    def forward(ctx, x, graph, bias, alpha, addend, addend_scale):
        _chk(x, bias, addend)
        x2 = _f32c(x)
        n, F = x2.shape
        if n != graph.n_nodes:
            raise ValueError(f"x has {n} rows, graph has {graph.n_nodes} nodes")
        out = torch.empty_like(x2)
        _spmm_launch(graph, False, x2, _f32c(bias) if bias is not None else None, out, float(alpha),
                     _f32c(addend) if addend is not None else None, float(addend_scale))
        ctx.graph, ctx.alpha, ctx.addend_scale = graph, float(alpha), float(addend_scale)
        ctx.has_bias, ctx.has_addend = bias is not None, addend is not None
        ctx.bias_param = bias                   # the Parameter itself: fused_grad_accumulation adds into its .grad
        return out

    @staticmethod
    def backward(ctx, dy):
        g = ctx.graph
        dy = _f32c(dy)
        dx = db = da = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(dy)
            _spmm_launch(g, True, dy, None, dx, ctx.alpha, None, 0.0)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _grad_colsum(ctx.bias_param, dy)
        if ctx.has_addend and ctx.needs_input_grad[4]:
            da = dy * ctx.addend_scale
        return dx, None, db, None, da, None


def spmm(x, graph, bias=None, alpha=1.0, addend=None, addend_scale=0.0):
    return SpmmFn.apply(x, graph, bias, alpha, addend, addend_scale)


GPR_MAX_NODES = 256
GPR_MAX_K = 16
GPR_SLAB = 32
# Which path ``gpr_prop`` takes inside the resident kernel's domain when the caller does not say: decided by the measurement of
# tools/gpr_bench.py (profiles/gpr_bench.txt, DESIGN.md "GPR-GNN and APPNP: the graph-resident K-hop kernel") under the
# project's rule -- the resident kernel is the default only if its advantage over the composed path on the WHOLE train step
# exceeds three times the wider run-to-run range.  Measured at 668 graphs x 196 nodes, F = 128, three layers, K = 10: the
# GraphMIL[gprgnn] step takes 8.04 ms resident against 10.87 ms composed (appnp: 7.69 against 8.46), ranges below 0.02 ms.
GPR_RESIDENT_DEFAULT = True
_LAST_PATH = {}                                 # entry name -> 'resident' | 'composed'
# What follows "NAME: n graph(s) whose node offsets decrease, leave the node range or span more than 256 nodes, " when a
# graph-resident kernel has counted graphs it refused (256 = GPR_MAX_NODES = H2_MAX_NODES: csrc/graph_resident.inc)
_REFUSED = {
    "gpr_prop": "or that hold a column id outside their own node range; their rows were not written",
    "h2_prop": "or whose operators hold a column id outside the graph's own node range; their rows were not written",
    "two_hop": "whose row pointers decrease or leave the entry range, or that hold a column id outside their own node range",
}


def _raise_if_refused(name, bad, also=None):
    """Reads the counter of refused graphs of a graph-resident kernel back -- ONE copy and synchronisation, together with the
    int64 values ``also`` -- and raises on a non-zero count; returns the values of ``also``."""
    *rest, n_bad = (bad if also is None else torch.cat([also, bad.to(torch.int64)])).cpu().tolist()
    n_bad &= 0xFFFFFFFF                                                     # (uint32 on the device side)
    if n_bad:
        raise ValueError(f"{name}: {n_bad} graph(s) whose node offsets decrease, leave the node range or span more than "
                         f"{GPR_MAX_NODES} nodes, {_REFUSED[name]}")
    return rest


def _resident_or_composed(name, resident, offsets, composed, apply, device, bad, check):
    """The dispatch ``gpr_prop`` and ``h2_prop`` share: ``composed()`` unless ``resident`` (the caller's choice or the entry's
    ``*_RESIDENT_DEFAULT``) and ``offsets`` are there, and wherever ``apply(bad)`` answers ISIC_ERR_UNSUPPORTED.  Records the
    path taken; a counter made here is read back if ``check``."""
    _LAST_PATH[name] = "composed"
    if not resident or offsets is None:
        return composed()
    own = bad is None
    if own:
        bad = torch.zeros(1, device=device, dtype=torch.int32)              # (uint32 on the device side)
    try:
        z = apply(bad)
    except IsicHipError as e:
        if e.code != ERR_UNSUPPORTED:
            raise
        return composed()
    _LAST_PATH[name] = "resident"
    if own and check:
        _raise_if_refused(name, bad)
    return z


def gpr_last_path():
    """'resident' or 'composed': the path the last ``gpr_prop`` call took (for tests and the benchmark)."""
    return _LAST_PATH.get("gpr_prop")


def gpr_gamma(K, alpha, dtype=torch.float32):
    """The PPR coefficients of GPR-GNN / APPNP: gamma[k] = alpha (1 - alpha)^k for k < K, gamma[K] = (1 - alpha)^K."""
    K, alpha = int(K), float(alpha)
    g = [alpha * (1.0 - alpha) ** k for k in range(K)] + [(1.0 - alpha) ** K]
    return torch.tensor(g, dtype=dtype)


def gpr_prop_composed(h, gamma, graph, bias=None):
    """Z = sum_k gamma[k] A^^k h (+ bias) as K calls of ``spmm`` plus torch axpys under ordinary autograd: the fallback
    outside the resident kernel's domain and the A/B baseline of tools/gpr_bench.py."""
    K = int(gamma.numel()) - 1
    p = h
    z = gamma[0] * p
    for k in range(1, K + 1):
        p = spmm(p, graph)
        z = z + gamma[k] * p
    return z + bias if bias is not None else z


class GprPropFn(torch.autograd.Function):
    """Z = sum_k gamma[k] A^^k h (+ bias) in one launch (``isic_gpr_prop_f32``); backward on the transposed CSR in one
    launch plus the fixed-order reduction of the d gamma partials (``isic_gpr_prop_bwd_f32``)."""

    @staticmethod
    def forward(ctx, h, gamma, graph, offsets, bias, bad):
        _chk(h, gamma, bias)
        h2, gm = _f32c(h), _f32c(gamma)
        n, F = h2.shape
        if n != graph.n_nodes or n != offsets.total:
            raise ValueError(f"h has {n} rows, graph has {graph.n_nodes} nodes, offsets cover {offsets.total}")
        K = int(gm.numel()) - 1
        z = torch.empty_like(h2)
        call("isic_gpr_prop_f32", graph.rowptr, graph.col, graph.val, int(graph.col.numel()), offsets.device, offsets.num_bags,
             offsets.max_bag, n, h2, gm, K, F, _f32c(bias) if bias is not None else None, z, bad)
        ctx.graph, ctx.offsets, ctx.K, ctx.bad = graph, offsets, K, bad
        ctx.params = (gamma, bias)              # the Parameters themselves: fused_grad_accumulation adds into their .grad
        ctx.save_for_backward(h2, gm)
        return z

    @staticmethod
    def backward(ctx, dz):
        from .ops import _workspace
        h2, gm = ctx.saved_tensors
        gamma, bias = ctx.params
        g, offs, K = ctx.graph, ctx.offsets, ctx.K
        dz = _f32c(dz)
        n, F = dz.shape
        dh = torch.empty_like(dz) if ctx.needs_input_grad[0] else None
        dg_out, tg, ws, nbytes = None, None, None, 0
        if ctx.needs_input_grad[1]:             # appnp: gamma is a buffer, no partials are formed
            tg = _acc_target(gamma)
            dg_out = tg if tg is not None else torch.empty((K + 1,), device=dz.device, dtype=torch.float32)
            nbytes = int(call("isic_gpr_prop_bwd_workspace_bytes", offs.num_bags, K, F))
            ws = _workspace(nbytes, dz.device)
        if dh is not None or dg_out is not None:
            call("isic_gpr_prop_bwd_f32", g.rowptr_t, g.col_t, g.val_t, int(g.col_t.numel()), offs.device, offs.num_bags,
                 offs.max_bag, n, dz, h2, gm, K, F, dh, dg_out, 1.0 if tg is not None else 0.0, ws, nbytes, ctx.bad)
        db = _grad_colsum(bias, dz) if bias is not None and ctx.needs_input_grad[4] else None
        dgamma = None if (dg_out is None or tg is not None) else dg_out.reshape(gamma.shape)
        return dh, dgamma, None, None, db, None


def gpr_prop(h, gamma, graph, offsets=None, bias=None, resident=None, check=True, bad=None):
    """The K-hop polynomial filter of GPR-GNN / APPNP on a 'gcn'-mode ``GraphBatch``: Z = sum_{k=0..K} gamma[k] A^^k h
    (+ bias), K = len(gamma) - 1, with gradients for ``h``, ``gamma`` (skipped when it does not require one) and ``bias``.

    ``resident`` picks the path: True = the graph-resident kernel (``isic_gpr_prop_f32``: every hop of a graph's column slab
    out of LDS, one launch), False = ``gpr_prop_composed``, None = ``GPR_RESIDENT_DEFAULT``.  The resident kernel needs
    ``offsets`` (``BagOffsets``: graph g owns rows offsets[g]:offsets[g+1], and every edge stays inside its graph) with at
    most 256 nodes per graph; wherever the entry answers ISIC_ERR_UNSUPPORTED, and without offsets, the composed path runs.

    The kernel counts graphs it refused -- offsets that do not fit, or a column id outside the graph's own node range; such a
    graph's rows of Z are NOT written: with ``check`` the counter is read back (4 bytes, a synchronisation) and a non-zero
    count is a ``ValueError``.  ``bad`` (device int32 [1]): the caller's own counter, added to and not read here."""
    if graph.mode != "gcn":
        raise ValueError(f"gpr_prop needs a 'gcn'-mode GraphBatch, got '{graph.mode}'")
    if gamma.dim() != 1 or not 1 <= gamma.numel() <= GPR_MAX_K + 1:
        raise IsicHipError(f"gpr_prop takes gamma [K + 1] with 0 <= K <= {GPR_MAX_K}, got {tuple(gamma.shape)}", code=-1)
    return _resident_or_composed("gpr_prop", GPR_RESIDENT_DEFAULT if resident is None else resident, offsets,
                                 lambda: gpr_prop_composed(h, gamma, graph, bias),
                                 lambda b: GprPropFn.apply(h, gamma, graph, offsets, bias, b), h.device, bad, check)


def gpr_check(bad):
    """Reads a ``gpr_prop`` counter back (a synchronisation) and raises on a non-zero count."""
    _raise_if_refused("gpr_prop", bad)


H2_MAX_NODES = 256
H2_SLAB = 32
# Which path ``h2_prop`` takes inside the resident kernel's domain when the caller does not say: decided by the measurement of
# tools/h2_bench.py (profiles/h2_bench.txt, DESIGN.md "H2GCN: the device 2-hop build and the two-operator propagation") under
# the project's rule -- the resident kernel is the default only if its advantage over the composed path on the WHOLE train step
# exceeds three times the wider run-to-run range.  Measured at 668 graphs x 196 nodes, F = 128, two layers: the GraphMIL[h2gcn]
# step takes 8.06 ms resident against 7.40 ms composed on grid8, 13.25 against 9.26 on knn8 and 13.44 against 9.53 on random8
# (ranges below 0.13 ms): the resident kernel loses on every variant, also at 117 - 129 entries per 2-hop row, and is opt-in.
H2_RESIDENT_DEFAULT = False


def h2_last_path():
    """'resident' or 'composed': the path the last ``h2_prop`` call took (for tests and the benchmark)."""
    return _LAST_PATH.get("h2_prop")


class TwoHopGraph:
    """The two symmetric operators of H2GCN over a batch of graphs (``two_hop``): ``a1`` = A1^, the symmetrised 1-hop graph
    without self loops, ``a2`` = A2^, the nodes at distance exactly 2, each D^-1/2 A D^-1/2 by its own row counts -- two
    ``GraphBatch``es of mode ``"sym"`` with GLOBAL ids, columns ascending inside a row.  ``mode`` is ``"h2"``: what
    ``GraphMIL(gnn_type="h2gcn")`` asks of a prebuilt graph."""

    mode = "h2"

    def __init__(self, a1, a2):
        if a1.n_nodes != a2.n_nodes:
            raise ValueError("the two operators must cover the same nodes")
        self.a1, self.a2, self.n_nodes = a1, a2, a1.n_nodes


def _sym_graph(n, rowptr, col, val, perm):
    return GraphBatch.from_parts(n, int(col.numel()), SYM_MODE, {"rowptr": rowptr, "col": col, "val": val, "rowptr_t": rowptr,
                                                                "col_t": col, "val_t": val, "perm_t": perm})


def two_hop_count_launch(graph, offsets, deg, bad):
    """The bare ``isic_two_hop_count`` launch: ``deg`` int32 [2, N] (zeroed by the caller), ``bad`` int32 [1]."""
    call("isic_two_hop_count", graph.rowptr, graph.col, int(graph.col.numel()), offsets.device, offsets.num_bags, offsets.max_bag,
         graph.n_nodes, deg[0], deg[1], bad)


def two_hop_write_launch(graph, offsets, rp, nnz1, nnz2, out1, out2, bad):
    """The bare ``isic_two_hop_write`` launch: ``rp`` int32 [2, N + 1], ``outp`` = (col, val, perm) of nnzp entries each."""
    call("isic_two_hop_write", graph.rowptr, graph.col, int(graph.col.numel()), offsets.device, offsets.num_bags, offsets.max_bag,
         graph.n_nodes, rp[0], rp[1], int(nnz1), int(nnz2), out1[0], out1[1], out1[2], out2[0], out2[1], out2[2], bad)


def two_hop(graph, offsets) -> TwoHopGraph:
    """The 1-hop and the exact 2-hop operator of every graph of a batch (include/isic_hip_h2.h; tests/h2gcn_ref.py restates
    them): ``graph`` is any ``GraphBatch`` -- only its structure is read: direction, duplicates, self loops and values do not
    matter -- and ``offsets`` (``BagOffsets``) says which rows each graph owns, at most 256 per graph.  Two launches
    (``isic_two_hop_count`` / ``_write``), a scan between them and ONE read-back: the two entry totals and the kernels' count of
    refused graphs, which is a ``ValueError`` when it is not zero."""
    n = graph.n_nodes
    if n != offsets.total:
        raise ValueError(f"graph has {n} nodes, offsets cover {offsets.total}")
    if offsets.max_bag > H2_MAX_NODES:
        raise IsicHipError(f"two_hop supports up to {H2_MAX_NODES} nodes per graph, got {offsets.max_bag}", code=ERR_UNSUPPORTED)
    dev = graph.rowptr.device
    i32 = torch.int32
    deg = torch.zeros((2, n), device=dev, dtype=i32)
    bad = torch.zeros(1, device=dev, dtype=i32)                             # (uint32 on the device side)
    two_hop_count_launch(graph, offsets, deg, bad)
    rp = torch.zeros((2, n + 1), device=dev, dtype=torch.int64)
    rp[:, 1:] = torch.cumsum(deg, dim=1, dtype=torch.int64)
    nnz1, nnz2 = _raise_if_refused("two_hop", bad, also=rp[:, -1])          # the one read-back
    if max(nnz1, nnz2) >= 2 ** 31 - 1:
        raise IsicHipError("two_hop: more than 2^31 - 2 entries in one operator", code=ERR_UNSUPPORTED)
    rp = rp.to(i32)
    outs = [(torch.empty(z, device=dev, dtype=i32), torch.empty(z, device=dev, dtype=torch.float32),
             torch.empty(z, device=dev, dtype=i32)) for z in (nnz1, nnz2)]
    two_hop_write_launch(graph, offsets, rp, nnz1, nnz2, outs[0], outs[1], bad)
    return TwoHopGraph(_sym_graph(n, rp[0], *outs[0]), _sym_graph(n, rp[1], *outs[1]))


def h2_prop_composed(h, g2):
    """[A1^ h | A2^ h] as two calls of ``spmm`` plus ``torch.cat`` under ordinary autograd: the fallback outside the resident
    kernel's domain and the A/B baseline of tools/h2_bench.py."""
    return torch.cat([spmm(h, g2.a1), spmm(h, g2.a2)], dim=1)


def _h2_launch(name, g2, offsets, x, ldx, F, out, ldo, bad):
    a1, a2 = g2.a1, g2.a2
    call(name, a1.rowptr, a1.col, a1.val, int(a1.col.numel()), a2.rowptr, a2.col, a2.val, int(a2.col.numel()), offsets.device,
         offsets.num_bags, offsets.max_bag, g2.n_nodes, x, int(ldx), int(F), out, int(ldo), bad)


class H2PropFn(torch.autograd.Function):
    """Z = [A1^ h | A2^ h] in one launch (``isic_h2_prop_f32``); the backward dh = A1^ dz[:, :F] + A2^ dz[:, F:] in one launch
    on the same CSRs (``isic_h2_prop_bwd_f32``): the operators are symmetric."""

    @staticmethod
    def forward(ctx, h, g2, offsets, bad):
        _chk(h)
        h2 = _f32c(h)
        n, F = h2.shape
        if n != g2.n_nodes or n != offsets.total:
            raise ValueError(f"h has {n} rows, graph has {g2.n_nodes} nodes, offsets cover {offsets.total}")
        z = torch.empty((n, 2 * F), device=h2.device, dtype=torch.float32)
        _h2_launch("isic_h2_prop_f32", g2, offsets, h2, F, F, z, 2 * F, bad)
        ctx.g2, ctx.offsets, ctx.bad = g2, offsets, bad
        return z

    @staticmethod
    def backward(ctx, dz):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        dz = _f32c(dz)
        n, F = dz.shape[0], dz.shape[1] // 2
        dh = torch.empty((n, F), device=dz.device, dtype=torch.float32)
        _h2_launch("isic_h2_prop_bwd_f32", ctx.g2, ctx.offsets, dz, 2 * F, F, dh, F, ctx.bad)
        return dh, None, None, None


def h2_prop(h, g2, offsets=None, resident=None, bad=None):
    """The layer of H2GCN on a ``TwoHopGraph``: Z [N, 2 F] = [A1^ h | A2^ h], with the gradient for ``h``.

    ``resident`` picks the path: True = the graph-resident kernel (``isic_h2_prop_f32``: a graph's column slab staged once in
    LDS, both operators gathered out of it, one launch), False = ``h2_prop_composed``, None = ``H2_RESIDENT_DEFAULT``.  The
    resident kernel needs ``offsets`` (``BagOffsets``: graph g owns rows offsets[g]:offsets[g+1]) with at most 256 nodes per
    graph; wherever the entry answers ISIC_ERR_UNSUPPORTED, and without offsets, the composed path runs.

    The kernel counts graphs it refused (their rows of Z are NOT written): without ``bad`` the counter is read back (4 bytes, a
    synchronisation) and a non-zero count is a ``ValueError``.  ``bad`` (device int32 [1]): the caller's own counter, added to
    and not read here (``h2_check``)."""
    if getattr(g2, "mode", None) != "h2":
        raise ValueError("h2_prop needs a TwoHopGraph (isic_hip.graph.two_hop)")
    return _resident_or_composed("h2_prop", H2_RESIDENT_DEFAULT if resident is None else resident, offsets,
                                 lambda: h2_prop_composed(h, g2), lambda b: H2PropFn.apply(h, g2, offsets, b), h.device, bad,
                                 True)


def h2_check(bad):
    """Reads an ``h2_prop`` counter back (a synchronisation) and raises on a non-zero count."""
    _raise_if_refused("h2_prop", bad)


class GcnBlockFn(torch.autograd.Function):
    """One residual GCN layer of GraphMIL as ONE autograd node (`05_train_gnns.py:184-199`):

        y = dropout(relu(LayerNorm(A^ (h W^T) + b))) + h

    The kernels are those of ``ops.linear`` -> ``spmm`` -> ``ops.layer_norm``; what the single node buys is the backward: the
    two gradient paths into ``h`` (the residual's dy and the convolution's (A^T d) W) meet in the epilogue of the data-gradient
    GEMM (``gemm(..., addend=dy)``) instead of in an elementwise pass autograd would launch over both [T, F] tensors."""

    @staticmethod
    def forward(ctx, h, weight, bias, gamma, beta, graph, eps, drop, residual):
        from .ops import NO_DROP, gemm
        _chk(h, weight, bias, gamma, beta)
        h2, w = _f32c(h), _f32c(weight)
        n, F = h2.shape[0], w.shape[0]
        if n != graph.n_nodes:
            raise ValueError(f"x has {n} rows, graph has {graph.n_nodes} nodes")
        if residual and w.shape[1] != F:
            raise ValueError("a residual GCN block keeps the feature width")
        drop = drop or NO_DROP
        lin = gemm(h2, w, trans_b=True)
        agg = torch.empty_like(lin)
        _spmm_launch(graph, False, lin, _f32c(bias) if bias is not None else None, agg, 1.0, None, 0.0)
        g_, b_ = _f32c(gamma), _f32c(beta)
        y = torch.empty_like(agg)
        mean = torch.empty((n,), device=h2.device, dtype=torch.float32)
        rstd = torch.empty((n,), device=h2.device, dtype=torch.float32)
        call("isic_layernorm_fwd_clk", agg, g_, b_, h2 if residual else None, y, mean, rstd, n, F, float(eps), 1, drop.threshold,
             drop.scale, drop.seed, drop.stream, drop.clock)
        ctx.graph, ctx.drop, ctx.residual = graph, drop, bool(residual)
        ctx.params = (weight, bias, gamma, beta)
        ctx.save_for_backward(h2, w, agg, g_, b_, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        from .ops import _workspace, gemm
        h2, w, agg, g_, b_, mean, rstd = ctx.saved_tensors
        weight, bias, gamma, beta = ctx.params
        drop = ctx.drop
        n, F = agg.shape
        dy2 = _f32c(dy)
        # LayerNorm (+ReLU +dropout) backward; dgamma / dbeta accumulate
        d_agg = torch.empty_like(agg)
        tg, tb = _acc_target(gamma), _acc_target(beta)
        fused_ln = tg is not None and tb is not None
        dg = tg if fused_ln else torch.zeros((F,), device=agg.device, dtype=torch.float32)
        db_ln = tb if fused_ln else torch.zeros((F,), device=agg.device, dtype=torch.float32)
        ws = _workspace(call("isic_layernorm_bwd_workspace_bytes", F), agg.device)
        # GCNConv's bias gradient = column sums of d_agg: taken by the LayerNorm backward itself for the vector widths
        dbias, want_db = None, bias is not None and ctx.needs_input_grad[2]
        if want_db and F in (64, 128, 256):
            t = _acc_target(bias)
            if t is None:
                t = dbias = torch.zeros((F,), device=agg.device, dtype=torch.float32)
            call("isic_layernorm_bwd_dxsum_ws", dy2, agg, g_, b_, mean, rstd, d_agg, dg, db_ln, t, n, F, 1, drop.threshold,
                 drop.scale, drop.seed, drop.stream, drop.clock, ws, ws.numel() if ws is not None else 0)
            want_db = False
        else:
            call("isic_layernorm_bwd_ws", dy2, agg, g_, b_, mean, rstd, d_agg, dg, db_ln, n, F, 1, drop.threshold, drop.scale,
                 drop.seed, drop.stream, drop.clock, ws, ws.numel() if ws is not None else 0)
        if want_db:
            dbias = _grad_colsum(bias, d_agg)
        d_lin = torch.empty_like(d_agg)
        _spmm_launch(ctx.graph, True, d_agg, None, d_lin, 1.0, None, 0.0)
        dW = _grad_gemm(weight, d_lin, h2) if ctx.needs_input_grad[1] else None
        dh = None
        if ctx.needs_input_grad[0]:
            dh = gemm(d_lin, w, addend=dy2 if ctx.residual else None)      # (A^T d) W + dy: both paths in one epilogue
        return dh, dW, dbias, (None if fused_ln else dg), (None if fused_ln else db_ln), None, None, None, None


def gcn_block(h, weight, bias, gamma, beta, graph, eps=1e-5, drop=None, residual=True):
    return GcnBlockFn.apply(h, weight, bias, gamma, beta, graph, eps, drop, residual)


class L2NormalizeFn(torch.autograd.Function):
    """Row-wise x / max(||x||_2, eps): ``F.normalize`` of SAGEConv(normalize=True)."""

    @staticmethod
    def forward(ctx, x, eps):
        _chk(x)
        x2 = _f32c(x)
        y = torch.empty_like(x2)
        n = torch.empty(x2.shape[0], device=x2.device, dtype=torch.float32)
        call("isic_l2normalize_fwd", x2, y, n, x2.shape[0], x2.shape[1], float(eps))
        ctx.save_for_backward(y, n)
        ctx.eps = float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, n = ctx.saved_tensors
        dx = torch.empty_like(y)
        call("isic_l2normalize_bwd", _f32c(dy), y, n, dx, y.shape[0], y.shape[1], ctx.eps)
        return dx, None


def l2_normalize(x, eps=1e-12):
    return L2NormalizeFn.apply(x, eps)


class GatFn(torch.autograd.Function):
    """PyG GATConv message passing on a 'gcn'-mode GraphBatch (self loops re-added): per-destination
    edge softmax of leaky_relu(<x', att_src>[src] + <x', att_dst>[dst]) and the weighted neighbour sum.
    ``concat=False``: the mean over heads, out [N,F] and bias [F], formed inside the kernels (``isic_gat_fwd_mean``)."""

    @staticmethod
    def forward(ctx, xp, att_src, att_dst, bias, graph, heads, slope, drop, concat=True):
        from .ops import NO_DROP
        _chk(xp, att_src, att_dst, bias)
        xp = _f32c(xp)
        N, HF = xp.shape
        F_ = HF // heads
        a_s, a_d = _f32c(att_src).reshape(heads, F_), _f32c(att_dst).reshape(heads, F_)
        drop = drop or NO_DROP
        dev = xp.device
        al = torch.empty((N, heads), device=dev, dtype=torch.float32)
        ar = torch.empty((N, heads), device=dev, dtype=torch.float32)
        call("isic_gat_scores", xp, a_s, a_d, al, ar, N, heads, F_)
        nnz = graph.col.numel()
        alpha = torch.empty((nnz, heads), device=dev, dtype=torch.float32)
        out = torch.empty_like(xp) if concat else torch.empty((N, F_), device=dev, dtype=torch.float32)
        call("isic_gat_fwd" if concat else "isic_gat_fwd_mean", xp, al, ar, graph.rowptr, graph.col, _f32c(bias) if bias is not None else None, out, alpha, N,
             heads, F_, float(slope), drop.threshold, drop.scale, drop.seed, drop.stream)
        ctx.graph, ctx.cfg = graph, (N, heads, F_, float(slope), drop, bias is not None, att_src.shape, concat)
        ctx.save_for_backward(xp, a_s, a_d, al, ar, alpha)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .ops import gemm
        xp, a_s, a_d, al, ar, alpha = ctx.saved_tensors
        N, H, F_, slope, drop, has_bias, att_shape, concat = ctx.cfg
        g = ctx.graph
        dout = _f32c(dout)
        dev = xp.device
        de = torch.empty_like(alpha)
        dar = torch.empty((N, H), device=dev, dtype=torch.float32)
        dal = torch.empty((N, H), device=dev, dtype=torch.float32)
        dxp = torch.empty_like(xp)
        call("isic_gat_bwd" if concat else "isic_gat_bwd_mean", dout, xp, alpha, al, ar, a_s, a_d, g.rowptr, g.col, g.rowptr_t, g.col_t, g.perm_t, de, dar,
             dal, dxp, N, H, F_, slope, drop.threshold, drop.scale, drop.seed, drop.stream)
        # d att_src[h,:] = dal[:,h]^T x'[:,h,:]   (strided views: one small GEMM per head)
        d_as = torch.empty((H, F_), device=dev, dtype=torch.float32)
        d_ad = torch.empty((H, F_), device=dev, dtype=torch.float32)
        for h in range(H):
            xh = xp[:, h * F_:(h + 1) * F_]
            gemm(dal[:, h:h + 1], xh, trans_a=True, out=d_as[h:h + 1])
            gemm(dar[:, h:h + 1], xh, trans_a=True, out=d_ad[h:h + 1])
        db = colsum(dout) if has_bias else None
        return dxp, d_as.reshape(att_shape), d_ad.reshape(att_shape), db, None, None, None, None, None


def gat_conv(xp, att_src, att_dst, bias, graph, heads, negative_slope=0.2, drop=None, concat=True):
    """x'[N, H*F] -> [N, H*F], or with ``concat=False`` the mean over heads [N, F] (``bias`` [F])."""
    return GatFn.apply(xp, att_src, att_dst, bias, graph, heads, negative_slope, drop, bool(concat))


class EdgeAttnFn(torch.autograd.Function):
    """Edge-softmax attention aggregation of ``isic_edge_attn_fwd/bwd``.
    mode 0 (GATv2Conv): ks = x_l (also the values), qd = x_r, att[H,F]; 'gcn'-mode GraphBatch (self loops re-added).
    mode 1 (TransformerConv): ks = key, qd = query, v = value, scale = 1/sqrt(F); 'sum'-mode GraphBatch.
    ``concat=False``: the mean over heads, out [N,F] and bias [F], formed inside the kernels (``isic_edge_attn_fwd_mean``)."""

    @staticmethod
    def forward(ctx, mode, ks, qd, v, att, bias, graph, heads, slope, scale, drop, concat=True):
        from .ops import NO_DROP
        _chk(ks, qd, v, att, bias)
        ks, qd = _f32c(ks), _f32c(qd)
        v = ks if mode == 0 else _f32c(v)
        N, HF = ks.shape
        F_ = HF // heads
        a = _f32c(att).reshape(heads, F_) if att is not None else None
        drop = drop or NO_DROP
        alpha = torch.empty((graph.col.numel(), heads), device=ks.device, dtype=torch.float32)
        out = torch.empty_like(ks) if concat else torch.empty((N, F_), device=ks.device, dtype=torch.float32)
        call("isic_edge_attn_fwd" if concat else "isic_edge_attn_fwd_mean", int(mode), ks, qd, v, a, graph.rowptr, graph.col, _f32c(bias) if bias is not None else None,
             out, alpha, N, heads, F_, float(slope), float(scale), drop.threshold, drop.scale, drop.seed, drop.stream)
        ctx.graph, ctx.cfg = graph, (int(mode), N, heads, F_, float(slope), float(scale), drop, bias is not None,
                                     att.shape if att is not None else None, concat)
        ctx.save_for_backward(ks, qd, v, a, alpha)
        return out

    @staticmethod
    def backward(ctx, dout):
        ks, qd, v, a, alpha = ctx.saved_tensors
        mode, N, H, F_, slope, scale, drop, has_bias, att_shape, concat = ctx.cfg
        g = ctx.graph
        dout = _f32c(dout)
        dev = ks.device
        de = torch.empty_like(alpha)
        dqd, dks = torch.empty_like(qd), torch.empty_like(ks)
        dv = torch.empty_like(v) if mode == 1 else None
        datt = torch.zeros((H, F_), device=dev, dtype=torch.float32) if mode == 0 else None
        call("isic_edge_attn_bwd" if concat else "isic_edge_attn_bwd_mean", mode, dout, ks, qd, v, a, alpha, g.rowptr, g.col, g.rowptr_t, g.col_t, g.perm_t, de, dqd,
             dks, dv, datt, N, H, F_, slope, scale, drop.threshold, drop.scale, drop.seed, drop.stream)
        db = colsum(dout) if has_bias else None
        return (None, dks, dqd, dv, datt.reshape(att_shape) if datt is not None else None, db, None, None, None, None, None,
                None)


def gatv2_conv(xl, xr, att, bias, graph, heads, negative_slope=0.2, drop=None, concat=True):
    """x_l, x_r [N, H*F] -> [N, H*F], or with ``concat=False`` the mean over heads [N, F] (``bias`` [F])."""
    return EdgeAttnFn.apply(0, xl, xr, None, att, bias, graph, heads, negative_slope, 1.0, drop, bool(concat))


def transformer_attention(q, k, v, graph, heads, drop=None, concat=True):
    """q, k, v [N, H*F] -> the attention aggregate [N, H*F], or with ``concat=False`` its mean over heads [N, F]."""
    F_ = q.shape[1] // heads
    return EdgeAttnFn.apply(1, k, q, v, None, None, graph, heads, 0.0, 1.0 / (F_ ** 0.5), drop, bool(concat))


class FaFn(torch.autograd.Function):
    """FAConv propagation on a 'gcn'-mode GraphBatch: out = sum tanh(<x,att_l>[src] + <x,att_r>[dst]) * w * x[src] +
    eps * x0 (``isic_fa_fwd/bwd``; the two scalar scores per node come from ``isic_gat_scores`` with one head)."""

    @staticmethod
    def forward(ctx, x, x0, att_l, att_r, graph, eps, drop):
        from .ops import NO_DROP
        _chk(x, x0, att_l, att_r)
        x, x0 = _f32c(x), _f32c(x0)
        N, F_ = x.shape
        al_w, ar_w = _f32c(att_l).reshape(1, F_), _f32c(att_r).reshape(1, F_)
        drop = drop or NO_DROP
        dev = x.device
        al = torch.empty((N, 1), device=dev, dtype=torch.float32)
        ar = torch.empty((N, 1), device=dev, dtype=torch.float32)
        call("isic_gat_scores", x, al_w, ar_w, al, ar, N, 1, F_)
        coef = torch.empty(graph.col.numel(), device=dev, dtype=torch.float32)
        out = torch.empty_like(x)
        call("isic_fa_fwd", x, x0, al, ar, graph.rowptr, graph.col, graph.val, out, coef, N, F_, float(eps), drop.threshold,
             drop.scale, drop.seed, drop.stream)
        ctx.graph, ctx.cfg = graph, (N, F_, float(eps), drop, att_l.shape, att_r.shape)
        ctx.save_for_backward(x, al_w, ar_w, coef)
        return out

    @staticmethod
    def backward(ctx, dout):
        from .ops import gemm
        x, al_w, ar_w, coef = ctx.saved_tensors
        N, F_, eps, drop, shp_l, shp_r = ctx.cfg
        g = ctx.graph
        dout = _f32c(dout)
        dev = x.device
        de = torch.empty_like(coef)
        dar = torch.empty((N, 1), device=dev, dtype=torch.float32)
        dal = torch.empty((N, 1), device=dev, dtype=torch.float32)
        dx = torch.empty_like(x)
        call("isic_fa_bwd", dout, x, coef, al_w, ar_w, g.rowptr, g.col, g.val, g.rowptr_t, g.col_t, g.val_t, g.perm_t, de, dar,
             dal, dx, N, F_, drop.threshold, drop.scale, drop.seed, drop.stream)
        d_l = torch.empty((1, F_), device=dev, dtype=torch.float32)
        d_r = torch.empty((1, F_), device=dev, dtype=torch.float32)
        gemm(dal, x, trans_a=True, out=d_l)              # d att_l = dal^T x
        gemm(dar, x, trans_a=True, out=d_r)
        return dx, dout * eps, d_l.reshape(shp_l), d_r.reshape(shp_r), None, None, None


def fa_conv(x, x0, att_l, att_r, graph, eps=0.1, drop=None):
    return FaFn.apply(x, x0, att_l, att_r, graph, eps, drop)
