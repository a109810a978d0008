"""Gated attention pooling (Ilse et al. 2018) restated on torch-CPU in fp64: the DEFINITION the gated kernels and models are
held to.  The reference project has no gate branch, so there is no reference output to compare with:
this restatement of the arithmetic is the definition.  With the gate off every function here is the reference's own
arithmetic (oracle/mil.py, oracle/gnn.py), which tests/test_gated_pool_cpu.py checks.

    tv = tanh(h V^T + b_V)   sg = sigmoid(h U^T + b_U)   t = tv * sg   s = t w^T + b   att = softmax over each bag of s

Gradients come from autograd on these functions; the entry-level backward (``gate_bwd``) is written out as the formulas of
include/isic_hip_gated.h and checked against autograd in tests/test_gated_pool_cpu.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
EPS32 = 2.0 ** -24                                   # unit roundoff of fp32


def f64(p):
    return {k: v.detach().to(F64) for k, v in p.items()}


# ------------------------------------------------------------------ the two entries (include/isic_hip_gated.h)
def gate_fwd(p, heads, A):
    """p [T, 2 nA] (tanh-branch columns | gate columns) -> tv, sg, t   (fp64)."""
    nA = heads * A
    p = p.to(F64)
    tv, sg = torch.tanh(p[:, :nA]), torch.sigmoid(p[:, nA:])
    return tv, sg, tv * sg


def gate_bwd(d_s, w3, a, heads, A):
    """d_s [T, heads], w3 [heads, A], a [T, 2 nA] = tv | sg -> dict(d_p, d_bias, d_w3, d_b3) and, under ``abs_*``, the column
    sums of the summands' magnitudes (the sum|x| of the fp32 summation bound T * eps * sum|x|)."""
    nA = heads * A
    d_s, w3, a = d_s.to(F64), w3.to(F64).reshape(heads, A), a.to(F64)
    tv, sg = a[:, :nA], a[:, nA:]
    dse = d_s.repeat_interleave(A, dim=1)                                # d_s[n, k] at column k A + j
    d_t = dse * w3.reshape(1, nA)
    d_v = d_t * sg * (1.0 - tv * tv)
    d_g = d_t * tv * sg * (1.0 - sg)
    xw = dse * (tv * sg)
    return {"d_p": torch.cat([d_v, d_g], dim=1), "d_bias": torch.cat([d_v.sum(0), d_g.sum(0)]),
            "d_w3": xw.sum(0).reshape(heads, A), "d_b3": d_s.sum(0),
            "abs_d_bias": torch.cat([d_v.abs().sum(0), d_g.abs().sum(0)]), "abs_d_w3": xw.abs().sum(0).reshape(heads, A),
            "abs_d_b3": d_s.abs().sum(0)}


def entry_inputs(T, heads, A, seed=0, planted=True):
    """Seeded normals (fp32) for one entry-level case; ``planted``: a few values of p at 0, +-20, +-90 and +-inf."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + 31 * heads + A)
    nA = heads * A
    p = 2.0 * torch.randn(T, 2 * nA, generator=g)
    if planted:
        vals = [0.0, 20.0, -20.0, 90.0, -90.0, float("inf"), float("-inf")]
        flat = p.view(-1)
        for half in (0, 1):                                              # both branches see every planted value
            for i, v in enumerate(vals):
                n, j = (3 * i) % T, (5 * i + 1) % nA
                flat[n * 2 * nA + half * nA + j] = v
    d_s = torch.randn(T, heads, generator=g)
    w3 = torch.randn(heads, A, generator=g)
    return p, d_s, w3


# ------------------------------------------------------------------ the pooling heads
def scores(h, W, b, w, c, U=None, d=None):
    t = torch.tanh(F.linear(h, W, b))
    if U is not None:
        t = t * torch.sigmoid(F.linear(h, U, d))
    return F.linear(t, w, c)                                             # [N, 1]


def _gate_of(p, prefix):
    if f"{prefix}.0.weight" in p:
        return p[f"{prefix}.0.weight"], p[f"{prefix}.0.bias"]
    return None, None


def _hidden(p, x):
    return F.relu(F.linear(x, p["feature_extractor.0.weight"], p["feature_extractor.0.bias"]))     # dropout off (eval / p = 0)


def _bag_att(p, h):
    """Softmax over one bag; an empty bag has no rows and no attention."""
    U, d = _gate_of(p, "attention_gate")
    s = scores(h, p["attention.0.weight"], p["attention.0.bias"], p["attention.2.weight"], p["attention.2.bias"], U, d)
    return torch.softmax(s, dim=0)


def teacher_forward(p, x, offsets):
    """AttentionMIL_teacher on ragged bags: the five outputs of the batched model.  The gate is on iff ``p`` holds
    ``attention_gate.0.*``.  An empty bag pools nothing: bag_logits = 0, bag_probs = softmax(0) (as the ungated head)."""
    h = _hidden(p, x)
    P = F.linear(h, p["patch_classifier.weight"], p["patch_classifier.bias"])
    BL, att = [], []
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        a = _bag_att(p, h[lo:hi])
        att.append(a.reshape(-1))
        BL.append(torch.sum(a * P[lo:hi], dim=0))
    BL = torch.stack(BL)
    return {"bag_logits": BL, "bag_probs": torch.softmax(BL, dim=1), "attention": torch.cat(att), "patch_logits": P,
            "patch_probs": torch.softmax(P, dim=1)}


def attention_mil_forward(p, x, offsets):
    """AttentionMIL (feature-space pooling) on ragged bags -> probs [B, C], a [T, 1]."""
    h = _hidden(p, x)
    zs, att = [], []
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        a = _bag_att(p, h[lo:hi])
        att.append(a)
        zs.append(torch.sum(a * h[lo:hi], dim=0))
    logits = F.linear(torch.stack(zs), p["classifier.weight"], p["classifier.bias"])
    return torch.softmax(logits, dim=1), torch.cat(att)


def graphmil_mlp_forward(p, x, offsets, att_heads, layers=1):
    """GraphMIL(gnn_type='mlp', use_residual, use_layer_norm, classifier_light) in eval mode on a batch of graphs ->
    probs [G, C], att [N, heads].  The gates are on iff ``p`` holds ``attention_gates.*``."""
    h = F.linear(x, p["input_proj.weight"], p["input_proj.bias"]) if "input_proj.weight" in p else x
    for i in range(layers):
        hp = h
        h = F.linear(h, p[f"gnn_layers.{i}.0.weight"], p[f"gnn_layers.{i}.0.bias"])
        h = F.relu(F.layer_norm(h, (h.shape[1],), p[f"layer_norms.{i}.weight"], p[f"layer_norms.{i}.bias"]))
        if hp.shape == h.shape:
            h = h + hp
    zs, atts = [], []
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        hb, aa, pooled = h[lo:hi], [], []
        for k in range(att_heads):
            U, d = _gate_of(p, f"attention_gates.{k}")
            a = torch.softmax(scores(hb, p[f"attention_layers.{k}.0.weight"], p[f"attention_layers.{k}.0.bias"],
                                     p[f"attention_layers.{k}.2.weight"], p[f"attention_layers.{k}.2.bias"], U, d), dim=0)
            aa.append(a)
            pooled.append(torch.sum(a * hb, dim=0))
        atts.append(torch.cat(aa, dim=1))
        zs.append(torch.stack(pooled).mean(dim=0))
    u = F.relu(F.linear(torch.stack(zs), p["classifier.0.weight"], p["classifier.0.bias"]))
    logits = F.linear(u, p["classifier.3.weight"], p["classifier.3.bias"])
    return torch.softmax(logits, dim=1), torch.cat(atts)


def graph_loss(probs, y):
    """Mean over the graphs of the train loop's loss, CE(log(probs + 1e-9), y)."""
    return F.cross_entropy(torch.log(probs + 1e-9), y.long())


def loss_and_grads(forward, loss_of, p, x):
    """fp64 autograd: ``forward(q, xx)`` -> outputs, ``loss_of(outputs)`` -> scalar.  -> loss, outputs, gradients (+ 'x')."""
    q = {k: v.detach().to(F64).clone().requires_grad_(True) for k, v in p.items()}
    xx = x.detach().to(F64).clone().requires_grad_(True)
    out = forward(q, xx)
    loss = loss_of(out)
    loss.backward()
    g = {k: (v.grad.detach() if v.grad is not None else torch.zeros_like(v)) for k, v in q.items()}
    g["x"] = xx.grad.detach()
    return loss.detach(), out, g


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
