"""GPR-GNN / APPNP restated in pure torch, fp64 by default (test infrastructure for include/isic_hip_gpr.h,
csrc/gpr_prop.hip, ``isic_hip.graph.gpr_prop`` and ``GraphMIL(gnn_type='gprgnn' | 'appnp')``).

    A^      PyG ``gcn_norm``: self loops dropped and one loop per node added (an existing loop keeps its weight), deg[i] the
            sum of the weights INTO i, A^[dst, src] += deg[src]^-1/2 w deg[dst]^-1/2 -- built dense by a per-edge loop
    layer   h = x lin.weight^T;  out = sum_{k=0..K} gamma[k] A^^k h + bias
    gamma   gamma[k] = alpha (1 - alpha)^k for k < K, gamma[K] = (1 - alpha)^K (PPR)
    APPNP   x_0 = h;  x_{k+1} = (1 - alpha) A^ x_k + alpha x_0;  out = x_K  -- the layer with the PPR gamma

The parts of GraphMIL that do not change (LayerNorm, ReLU, residual, the attention pool, the light classifier, the loss)
follow oracle/gnn.py ``graphmil_forward`` line for line in the working dtype; its ``DEFAULT_CFG`` and ``graph_loss`` are
used as they are.  Gradients come from autograd.  The error bounds of tests/test_gpr_gpu.py are computed here too."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import gnn

U32 = 2.0 ** -24                  # unit round-off of fp32


def dense_adj(edge_index, n, edge_weight=None, dtype=torch.float64, drop_edge=None):
    """A^ [n, n] (row = destination) by a per-edge loop.  ``drop_edge``: an edge id left out AFTER the normalisation -- the
    deliberately wrong hop of the bound's self-check."""
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    w = [1.0] * len(src) if edge_weight is None else [float(v) for v in edge_weight.tolist()]
    loop_w = [1.0] * n
    edges = []
    for e, (s, d) in enumerate(zip(src, dst)):
        if s == d:
            loop_w[s] = w[e]
        else:
            edges.append((e, s, d, w[e]))
    edges += [(-1, i, i, loop_w[i]) for i in range(n)]
    deg = torch.zeros(n, dtype=dtype)
    for _, s, d, we in edges:
        deg[d] += torch.tensor(we, dtype=dtype)
    dis = deg.pow(-0.5)
    dis[torch.isinf(dis)] = 0.0
    A = torch.zeros((n, n), dtype=dtype)
    for e, s, d, we in edges:
        if drop_edge is not None and e == drop_edge:
            continue
        A[d, s] += (dis[s] * torch.tensor(we, dtype=dtype)) * dis[d]
    return A


def max_row_entries(edge_index, n):
    """-> (longest CSR row, longest transposed CSR row) of the graph after ``gcn_norm``: entries per destination / per
    source, duplicates counted, the self loop included."""
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    cin, cout = [1] * n, [1] * n
    for s, d in zip(src, dst):
        if s != d:
            cin[d] += 1
            cout[s] += 1
    return (max(cin), max(cout)) if n else (0, 0)


def ppr_gamma(K, alpha, dtype=torch.float64):
    K, alpha = int(K), float(alpha)
    return torch.tensor([alpha * (1.0 - alpha) ** k for k in range(K)] + [(1.0 - alpha) ** K], dtype=dtype)


def gpr_propagate(h, A, gamma, bias=None):
    """sum_k gamma[k] A^k h (+ bias)."""
    p = h
    z = gamma[0] * p
    for k in range(1, gamma.numel()):
        p = A @ p
        z = z + gamma[k] * p
    return z + bias if bias is not None else z


def gpr_layer(x, A, lin_weight, bias, gamma):
    return gpr_propagate(F.linear(x, lin_weight), A, gamma, bias)


def appnp_recurrence(h, A, K, alpha):
    x = h
    for _ in range(int(K)):
        x = (1.0 - alpha) * (A @ x) + alpha * h
    return x


def propagate_bound(h, A, gamma, d, bias=None, extra=0):
    """The elementwise bound on |Z^ - Z| of an fp32 evaluation in ANY summation order with or without FMA contraction:
    sum_k c(k (d + 1) + K + 3 + extra) |gamma[k]| (|A|^k |h|) + u |bias|, c(m) = m u / (1 - m u), d the longest CSR row.
    (Row k of the sum: k nested dot products of at most d terms, each d - 1 adds and d multiplies folded or not, the
    multiply by gamma[k] and the K adds of the outer sum, plus the roundings of the fp32 inputs' products.)  -> fp64, and the
    per-k terms |gamma[k]| |A|^k |h| for the dgamma bound."""
    K = gamma.numel() - 1
    absA, p = A.abs().double(), h.abs().double()
    total = torch.zeros_like(p)
    powers = []
    for k in range(K + 1):
        if k:
            p = absA @ p
        m = (k * (d + 1) + K + 3 + extra) * U32
        powers.append(p)
        total = total + (m / (1.0 - m)) * float(abs(gamma[k])) * p
    if bias is not None:
        total = total + U32 * bias.abs().double()
    return total, powers


def dgamma_ref_and_bound(dz, A, h, K, d_t, dot_len=None):
    """One graph's part of dgamma[k] = <(A^T)^k dz, h> and of its bound c(k (d_t + 1) + K + 3 + N F) <|A^T|^k |dz|, |h|>;
    ``dot_len`` = N F of the whole batch (the parts of all graphs are added, in some order, into one dot product)."""
    At, absAt = A.t(), A.abs().t().double()
    p, q = dz, dz.abs().double()
    ref, bound = [], []
    for k in range(K + 1):
        if k:
            p, q = At @ p, absAt @ q
        m = (k * (d_t + 1) + K + 3 + (dz.numel() if dot_len is None else dot_len)) * U32
        ref.append((p * h).sum())
        bound.append((m / (1.0 - m)) * (q * h.abs().double()).sum())
    return torch.stack(ref), torch.stack(bound)


def graphmil_shapes(input_dim, cfg):
    """Parameter / buffer names and shapes of ``GraphMIL(gnn_type='gprgnn' | 'appnp')`` in state_dict order."""
    c = dict(dict(gnn.DEFAULT_CFG, gpr_k=10, gpr_alpha=0.1), **cfg)
    F_ = c["gnn_hidden"]
    s = OrderedDict()
    has_proj = c["use_residual"] and input_dim != F_
    if has_proj:
        s["input_proj.weight"] = (F_, input_dim)
        s["input_proj.bias"] = (F_,)
    in_dim = F_ if has_proj else input_dim
    for i in range(c["gnn_layers"]):
        s[f"gnn_layers.{i}.bias"] = (F_,)
        s[f"gnn_layers.{i}.gamma"] = (c["gpr_k"] + 1,)
        s[f"gnn_layers.{i}.lin.weight"] = (F_, in_dim)
        in_dim = F_
    for i in range(c["gnn_layers"]):
        s[f"layer_norms.{i}.weight"] = (F_,)
        s[f"layer_norms.{i}.bias"] = (F_,)
    for h in range(c["att_heads"]):
        s[f"attention_layers.{h}.0.weight"] = (c["att_dim"], F_)
        s[f"attention_layers.{h}.0.bias"] = (c["att_dim"],)
        s[f"attention_layers.{h}.2.weight"] = (1, c["att_dim"])
        s[f"attention_layers.{h}.2.bias"] = (1,)
    s["classifier.0.weight"] = (c["classifier_dim"], F_)
    s["classifier.0.bias"] = (c["classifier_dim"],)
    s["classifier.3.weight"] = (c["num_classes"], c["classifier_dim"])
    s["classifier.3.bias"] = (c["num_classes"],)
    return s


def graphmil_forward(p, cfg, x, edge_index, edge_weight=None):
    """One graph, eval mode (no dropout), in the dtype of ``x`` / ``p``: the layer above inside the unchanged GraphMIL
    (oracle/gnn.py ``graphmil_forward``: LayerNorm, ReLU, residual where the shapes agree, the attention heads, the light
    classifier).  -> dict(probs, att, hs)."""
    c = dict(gnn.DEFAULT_CFG, **cfg)
    A = dense_adj(edge_index, x.shape[0], edge_weight, dtype=x.dtype)
    h = F.linear(x, p["input_proj.weight"], p["input_proj.bias"]) if "input_proj.weight" in p else x
    hs = []
    for i in range(c["gnn_layers"]):
        h_prev = h
        pre = f"gnn_layers.{i}"
        h = gpr_layer(h, A, p[f"{pre}.lin.weight"], p[f"{pre}.bias"], p[f"{pre}.gamma"])
        if c["use_layer_norm"]:
            h = F.layer_norm(h, (h.shape[1],), p[f"layer_norms.{i}.weight"], p[f"layer_norms.{i}.bias"])
        h = F.relu(h)
        if c["use_residual"] and h_prev.shape == h.shape:
            h = h + h_prev
        hs.append(h)
    atts, pooled = [], []
    for hd in range(c["att_heads"]):
        tt = torch.tanh(F.linear(h, p[f"attention_layers.{hd}.0.weight"], p[f"attention_layers.{hd}.0.bias"]))
        a = torch.softmax(F.linear(tt, p[f"attention_layers.{hd}.2.weight"], p[f"attention_layers.{hd}.2.bias"]), dim=0)
        atts.append(a)
        pooled.append(torch.sum(a * h, dim=0))
    z = torch.stack(pooled, dim=0).mean(dim=0)
    u = F.linear(z, p["classifier.0.weight"], p["classifier.0.bias"])
    if "classifier.8.weight" in p:           # GraphMIL's default head (05:140-153): Linear LN ReLU Linear LN ReLU Linear
        u = F.relu(F.layer_norm(u, u.shape, p["classifier.1.weight"], p["classifier.1.bias"]))
        u = F.linear(u, p["classifier.4.weight"], p["classifier.4.bias"])
        u = F.relu(F.layer_norm(u, u.shape, p["classifier.5.weight"], p["classifier.5.bias"]))
        logits = F.linear(u, p["classifier.8.weight"], p["classifier.8.bias"])
    else:                                    # classifier_light, as oracle/gnn.py restates it
        logits = F.linear(F.relu(u), p["classifier.3.weight"], p["classifier.3.bias"])
    return {"probs": torch.softmax(logits, dim=0), "att": torch.cat(atts, dim=1), "hs": hs}


def graphmil_batch_loss_and_grads(p, cfg, xs, edge_indices, ys, dtype=torch.float64):
    """A batch as the per-graph forwards; the loss is the mean of ``gnn.graph_loss`` over the graphs (the batched model's
    ``labels`` path).  -> (loss, probs [G, C], att [sum n, heads], grads incl. 'x': the list of d x_g)."""
    q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    xx = [x.detach().to(dtype).clone().requires_grad_(True) for x in xs]
    outs = [graphmil_forward(q, cfg, x, ei) for x, ei in zip(xx, edge_indices)]
    loss = torch.stack([gnn.graph_loss(o["probs"], int(y)) for o, y in zip(outs, ys)]).mean()
    loss.backward()
    grads = {k: (v.grad.detach() if v.grad is not None else None) for k, v in q.items()}
    grads["x"] = [x.grad.detach() for x in xx]
    return (loss.detach(), torch.stack([o["probs"].detach() for o in outs]),
            torch.cat([o["att"].detach() for o in outs], dim=0), grads)


# ---------------------------------------------------------------------------------------------- the kernel test's batch
KERNEL_SIZES = (63, 1, 196, 0, 2, 256, 64, 65)        # mixed order, the empty graph in the middle
KERNEL_F = (4, 36, 64, 68, 128)                       # below one slab, a 4-column tail, two slabs, a tail again, four slabs
KERNEL_K = (0, 1, 2, 10, 16)


def knn_like_edges(n, k, gen):
    """A directed k-NN-like list over n nodes: node i receives an edge from min(k, n - 1) distinct other nodes, drawn with a
    preference for low ids (hubs: the transposed rows are long).  -> int64 [2, E], LOCAL ids, destination-major."""
    src, dst = [], []
    for i in range(n):
        want, got = min(k, n - 1), []
        while len(got) < want:
            for j in (torch.rand(4 * k, generator=gen) ** 2 * n).long().tolist():
                if j != i and j not in got and len(got) < want:
                    got.append(j)
        src += got
        dst += [i] * len(got)
    return torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)


def kernel_batch(seed=0, sizes=KERNEL_SIZES, k=8):
    """-> (sizes, offsets, per-graph LOCAL edge lists, per-graph edge weights or None): the graph of 196 nodes has a node
    (5) without an in-edge beyond its self loop, the graph of 65 nodes repeats ten of its edges, the graph of 64 nodes
    carries edge weights in [0.5, 1.5) (every other edge of the batch then weighs 1)."""
    gen = torch.Generator().manual_seed(seed)
    eis, ews = [], []
    for n in sizes:
        ei = knn_like_edges(n, k, gen)
        if n == 196:
            ei = ei[:, ei[1] != 5]
        if n == 65:
            ei = torch.cat([ei, ei[:, 7:17]], dim=1)
        eis.append(ei)
        ews.append(torch.rand(ei.shape[1], generator=gen) + 0.5 if n == 64 else None)
    offsets = [0]
    for n in sizes:
        offsets.append(offsets[-1] + n)
    return list(sizes), offsets, eis, ews


def batch_edges(offsets, eis, ews):
    """The batch's global edge list and weight vector (1 where a graph has none; None if no graph has any)."""
    ei = torch.cat([e + o for e, o in zip(eis, offsets[:-1])], dim=1)
    if all(w is None for w in ews):
        return ei, None
    return ei, torch.cat([w if w is not None else torch.ones(e.shape[1]) for e, w in zip(eis, ews)])


def mixed_sign_gamma(K, seed=1):
    """Coefficients as a GPR-GNN trained on a heterophilous graph has them: alternating signs, slowly decaying."""
    gen = torch.Generator().manual_seed(seed)
    g = (0.3 + torch.rand(K + 1, generator=gen)) * torch.tensor([(-1.0) ** k * 0.9 ** k for k in range(K + 1)])
    return g.float()
