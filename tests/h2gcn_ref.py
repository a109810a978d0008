"""H2GCN (Zhu et al., NeurIPS 2020) restated in pure torch / numpy, fp64 by default, with a dense adjacency (test
infrastructure for include/isic_hip_h2.h, csrc/two_hop.hip, csrc/h2_prop.hip, ``isic_hip.graph.two_hop`` / ``h2_prop`` and
``GraphMIL(gnn_type='h2gcn')``).

Per graph with n nodes and ANY edge list (directed, duplicates and self loops allowed, weights ignored):

    A1[i,j] = 1  iff  i != j and the list holds i->j or j->i
    A2[i,j] = 1  iff  i != j, A1[i,j] = 0 and some m has A1[i,m] = A1[m,j] = 1          (distance exactly 2)
    Ap^     = Dp^-1/2 Ap Dp^-1/2,  dp[i] = the number of entries of row i; a row without entries is a zero row
    fp32    r = 1.0f / sqrtf((float)d),  val(i,j) = r[i] * r[j]: one correctly rounded operation each

    r_0 = x_in (the projected input);  s_i = [A1^ r_{i-1} | A2^ r_{i-1}];  r_i = relu(LayerNorm(s_i));  h = [r_0 | ... | r_L]

The parts of GraphMIL that do not change (the attention pool, the light classifier, the loss) follow oracle/gnn.py
``graphmil_forward`` as tests/gpr_ref.py restates them.  Gradients come from autograd."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import gnn

U32 = 2.0 ** -24                  # unit round-off of fp32


# ---------------------------------------------------------------------------------------------- the two adjacencies
def two_hop_dense(edge_index, n):
    """-> (A1, A2) as bool numpy [n, n] by the definition above: a per-edge loop and a per-triple test, no matrix product."""
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    A1 = np.zeros((n, n), dtype=bool)
    for s, d in zip(ei[0].tolist(), ei[1].tolist()):
        if s != d:
            A1[s, d] = A1[d, s] = True
    A2 = np.zeros((n, n), dtype=bool)
    for i in range(n):
        nb = np.flatnonzero(A1[i])
        if nb.size:
            A2[i] = A1[nb].any(axis=0)
    A2 &= ~A1
    A2[np.arange(n), np.arange(n)] = False
    return A1, A2


def normalise(A, dtype=torch.float64):
    """D^-1/2 A D^-1/2 with d = the row counts, a zero row for an empty one -> torch [n, n]."""
    a = torch.as_tensor(np.asarray(A), dtype=dtype)
    d = a.sum(dim=1)
    r = torch.where(d > 0, d.clamp_min(1).rsqrt(), torch.zeros_like(d))
    return r[:, None] * a * r[None, :]


def csr_of(A):
    """The canonical CSR of a 0/1 matrix as the device writes it, in numpy: deg int32 [n], rowptr int64 [n+1], col int64
    (LOCAL, ascending inside a row), val float32 = r[i] * r[j] with r = float32(1) / sqrt(float32(deg)) (numpy rounds each of
    the three operations correctly), perm = the slot of (j,i) for the slot of (i,j)."""
    A = np.asarray(A, dtype=bool)
    n = A.shape[0]
    deg = A.sum(axis=1).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(deg, dtype=np.int64)])
    rows, cols = np.nonzero(A)                                  # row-major: ascending columns inside a row
    d32 = deg.astype(np.float32)
    with np.errstate(divide="ignore"):
        r = np.where(deg > 0, np.float32(1.0) / np.sqrt(d32, dtype=np.float32), np.float32(0.0)).astype(np.float32)
    val = (r[rows] * r[cols]).astype(np.float32)
    below = np.cumsum(A, axis=1) - A                            # below[j, i] = set bits of row j below column i
    perm = rowptr[cols] + below[cols, rows] if n else np.zeros(0, dtype=np.int64)
    return deg, rowptr, cols.astype(np.int64), val, perm.astype(np.int64)


def h2_layer(r, A1n, A2n):
    return torch.cat([A1n @ r, A2n @ r], dim=1)


def dot_bound(absA, absX, m):
    """c(m) |A| |X|, c(m) = m u / (1 - m u): the bound on an fp32 dot product of at most m - 2 terms in ANY summation order,
    with or without FMA contraction (tests/gpr_ref.py ``propagate_bound`` with K = 1 and gamma = (0, 1))."""
    mu = m * U32
    return (mu / (1.0 - mu)) * (absA.abs().double() @ absX.abs().double())


# ---------------------------------------------------------------------------------------------- the model
def graphmil_shapes(input_dim, cfg):
    """Parameter names and shapes of ``GraphMIL(gnn_type='h2gcn', classifier_light=True)`` in state_dict order: the layers own
    nothing, LayerNorm i is 2^(i+1) hidden wide, the pool and the classifier (2^(L+1) - 1) hidden."""
    c = dict(gnn.DEFAULT_CFG, **cfg)
    H, L = c["gnn_hidden"], c["gnn_layers"]
    s = OrderedDict()
    if input_dim != H:                             # h2gcn projects like fagcn / gcnii, with or without use_residual
        s["input_proj.weight"] = (H, input_dim)
        s["input_proj.bias"] = (H,)
    if c["use_layer_norm"]:
        for i in range(L):
            s[f"layer_norms.{i}.weight"] = (2 ** (i + 1) * H,)
            s[f"layer_norms.{i}.bias"] = (2 ** (i + 1) * H,)
    Fd = (2 ** (L + 1) - 1) * H
    for h in range(c["att_heads"]):
        s[f"attention_layers.{h}.0.weight"] = (c["att_dim"], Fd)
        s[f"attention_layers.{h}.0.bias"] = (c["att_dim"],)
        s[f"attention_layers.{h}.2.weight"] = (1, c["att_dim"])
        s[f"attention_layers.{h}.2.bias"] = (1,)
    s["classifier.0.weight"] = (c["classifier_dim"], Fd)
    s["classifier.0.bias"] = (c["classifier_dim"],)
    s["classifier.3.weight"] = (c["num_classes"], c["classifier_dim"])
    s["classifier.3.bias"] = (c["num_classes"],)
    return s


def graphmil_forward(p, cfg, x, edge_index):
    """One graph, eval mode (no dropout), in the dtype of ``x`` / ``p``.  -> dict(probs, att, h)."""
    c = dict(gnn.DEFAULT_CFG, **cfg)
    A1, A2 = two_hop_dense(edge_index, x.shape[0])
    A1n, A2n = normalise(A1, x.dtype), normalise(A2, x.dtype)
    r = F.linear(x, p["input_proj.weight"], p["input_proj.bias"]) if "input_proj.weight" in p else x
    reps = [r]
    for i in range(c["gnn_layers"]):
        r = h2_layer(r, A1n, A2n)
        if c["use_layer_norm"]:
            r = F.layer_norm(r, (r.shape[1],), p[f"layer_norms.{i}.weight"], p[f"layer_norms.{i}.bias"])
        r = F.relu(r)                              # the residual never applies: the width doubles
        reps.append(r)
    h = torch.cat(reps, dim=1)
    atts, pooled = [], []
    for hd in range(c["att_heads"]):
        tt = torch.tanh(F.linear(h, p[f"attention_layers.{hd}.0.weight"], p[f"attention_layers.{hd}.0.bias"]))
        a = torch.softmax(F.linear(tt, p[f"attention_layers.{hd}.2.weight"], p[f"attention_layers.{hd}.2.bias"]), dim=0)
        atts.append(a)
        pooled.append(torch.sum(a * h, dim=0))
    z = torch.stack(pooled, dim=0).mean(dim=0)
    u = F.linear(z, p["classifier.0.weight"], p["classifier.0.bias"])
    logits = F.linear(F.relu(u), p["classifier.3.weight"], p["classifier.3.bias"])          # classifier_light
    return {"probs": torch.softmax(logits, dim=0), "att": torch.cat(atts, dim=1), "h": h}


def graphmil_batch_loss_and_grads(p, cfg, xs, edge_indices, ys, dtype=torch.float64):
    """A batch as the per-graph forwards; the loss is the mean of ``gnn.graph_loss`` over the graphs.
    -> (loss, probs [G, C], att [sum n, heads], grads incl. 'x': the list of d x_g)."""
    q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
    xx = [x.detach().to(dtype).clone().requires_grad_(True) for x in xs]
    outs = [graphmil_forward(q, cfg, x, ei) for x, ei in zip(xx, edge_indices)]
    loss = torch.stack([gnn.graph_loss(o["probs"], int(y)) for o, y in zip(outs, ys)]).mean()
    loss.backward()
    grads = {k: (v.grad.detach() if v.grad is not None else None) for k, v in q.items()}
    grads["x"] = [x.grad.detach() for x in xx]
    return (loss.detach(), torch.stack([o["probs"].detach() for o in outs]),
            torch.cat([o["att"].detach() for o in outs], dim=0), grads)


# ---------------------------------------------------------------------------------------------- graphs
def path_edges(n):
    """0 - 1 - ... - n-1, each edge once and in one direction only."""
    return np.stack([np.arange(n - 1), np.arange(1, n)]).astype(np.int64).reshape(2, -1)


def star_edges(n):
    """every leaf -> the hub 0."""
    return np.stack([np.arange(1, n), np.zeros(n - 1, dtype=np.int64)]).astype(np.int64).reshape(2, -1)


def complete_edges(n):
    s, d = np.nonzero(~np.eye(n, dtype=bool))
    return np.stack([s, d]).astype(np.int64)


def knn_like_edges(n, k, rng):
    """A directed list: node i receives an edge from min(k, n - 1) distinct other nodes (low ids preferred, so there are hubs),
    then some edges twice and some self loops."""
    src, dst = [], []
    for i in range(n):
        want = min(k, n - 1)
        cand = np.unique(np.concatenate([(rng.random(4 * k) ** 2 * n).astype(np.int64), rng.permutation(n)[:want + 1]]))
        cand = cand[cand != i]
        got = rng.permutation(cand)[:want]
        src += got.tolist()
        dst += [i] * got.size
    ei = np.asarray([src, dst], dtype=np.int64).reshape(2, -1)
    if n >= 4:
        loops = rng.integers(0, n, size=3)
        ei = np.concatenate([ei, ei[:, 5:12], np.stack([loops, loops])], axis=1)
    return ei


# (size, kind): every size of the issue's list -- the word boundaries of the bit rows among them -- in mixed order, the empty
# graph in the middle; the star of 256 nodes has leaf rows of 254 two-hop entries each, the densest case there is
KERNEL_GRAPHS = ((63, "knn"), (1, "none"), (196, "knn"), (0, "none"), (2, "path"), (256, "star"), (64, "knn"), (65, "complete"),
                 (3, "path"), (255, "knn"), (64, "none"), (255, "path"))
KERNEL_F = (1, 31, 32, 33, 128, 130)


def make_edges(n, kind, rng, k=8):
    if kind == "knn":
        return knn_like_edges(n, k, rng)
    if kind == "path":
        return path_edges(n)
    if kind == "star":
        return star_edges(n)
    if kind == "complete":
        return complete_edges(n)
    return np.zeros((2, 0), dtype=np.int64)


def kernel_batch(seed=0, graphs=KERNEL_GRAPHS):
    """-> (sizes, offsets, per-graph LOCAL edge lists as int64 numpy [2, E])."""
    rng = np.random.default_rng(seed)
    sizes = [n for n, _ in graphs]
    eis = [make_edges(n, kind, rng) for n, kind in graphs]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return sizes, offsets, eis


def batch_edges(offsets, eis):
    """The batch's global edge list, torch int64 [2, E]."""
    return torch.as_tensor(np.concatenate([e + int(o) for e, o in zip(eis, offsets[:-1])], axis=1))


def batch_csr(offsets, eis):
    """The numpy restatement of both operators over the whole batch with GLOBAL ids: per operator a dict of deg, rowptr, col,
    val, perm, and the per-graph dense 0/1 matrices."""
    out = [dict(deg=[], rowptr=[np.zeros(1, dtype=np.int64)], col=[], val=[], perm=[], dense=[]) for _ in range(2)]
    for lo, hi, ei in zip(offsets[:-1], offsets[1:], eis):
        for o, A in zip(out, two_hop_dense(ei, int(hi - lo))):
            deg, rowptr, col, val, perm = csr_of(A)
            base = sum(int(c.size) for c in o["col"])             # the entries of the graphs before this one
            o["deg"].append(deg)
            o["rowptr"].append(rowptr[1:] + base)
            o["col"].append(col + lo)
            o["val"].append(val)
            o["perm"].append(perm + base)
            o["dense"].append(A)
    return [{k: (v if k == "dense" else np.concatenate(v)) for k, v in o.items()} for o in out]
