"""fp64 reference, derived bounds, wrong variants and case list for the head-averaged attention entries
(isic_gat_fwd_mean / isic_gat_bwd_mean / isic_edge_attn_fwd_mean / isic_edge_attn_bwd_mean: PyG ``concat=False``), and the
model-level restatement of GraphMIL with ``gnn_concat=False``.  Plain torch on the CPU; shared by
tests/test_attn_mean_cpu.py and tests/test_attn_mean_gpu.py.

Kernel level.  Nothing is written anew: the reference is the concat reference of tests/f32_kernel_ref.py evaluated on
the same inputs with a zero bias and the mean-path gradient dmean[n,F] broadcast over the heads, UNSCALED.  Every
gradient of the layer is linear in dout, so the concat gradients for that dout, divided by H, are the gradients of
    out[i,f] = (1/H) sum_h o[i,h,f] + bias_f[f].
Bounds (u = 2^-24), derived from the concat bounds b = att_bounds(inp, ref), nothing fitted:
  alpha      b.alpha                      (the softmax is untouched)
  out        b.out.mean(1) + (H + 2) u (|ref.out|.mean(1) + |bias_f|)
             (the error of every head's aggregate, then an H-term sum in any order, one scaling and one bias add)
  gradients  b[k] / H + 2 u |ref[k] / H|  (one more rounding for the 1/H factor, wherever it is applied)

Model level.  ``graphmil_mean_forward`` takes the layer arithmetic from oracle.gnn.gat_conv / gatv2_conv with a zero
[H*F] bias, then the mean over heads and the [F] bias; TransformerConv's aggregate and its [N,F] gate are written out;
the rest of GraphMIL.forward is as in oracle.gnn.graphmil_forward.  PARITY UNPINNED as every PyG layer here
(torch_geometric is absent)."""
import math
import os
import sys

import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import f32_kernel_ref as R  # noqa: E402
from oracle import gnn as G  # noqa: E402
from oracle import mil as _mil  # noqa: E402

F32, F64 = torch.float32, torch.float64
U = R.U

# ====================================================================================================== kernel level
# F below, at and above a wave (1, 16 | 64 | 65, 130); rows that keep the head sum in registers (F <= 256) and the one
# that adds into its own output row (257); gatv2's datt in registers (H ceil(F/64) <= 16) and through atomics (6 x 3,
# 4 x 5); the 1100-node graph has rows on both sides of the 512 edges kept in LDS.
MEAN_GAT_HF = ((1, 1), (3, 16), (4, 64), (2, 65), (8, 130))
MEAN_EA_HF = MEAN_GAT_HF + ((4, 257), (6, 168))
MEAN_BUGS = ("sum_not_mean", "bias_times_heads", "bwd_no_head_scale")
INHERITED_BUGS = ("philox_shift", "softmax_outgoing")
GRAD_KEYS = {"gat": ("de", "dal", "dar", "dxp"), "gatv2": ("de", "dqd", "dks", "datt"), "dot": ("de", "dqd", "dks", "dv")}


def _mean_cases():
    cases = []
    for layer, shapes in (("gat", MEAN_GAT_HF), ("gatv2", MEAN_EA_HF), ("dot", MEAN_EA_HF)):
        for H, F in shapes:
            for p in (0.0, R.ATT_P):
                cases.append(dict(layer=layer, n=R.ATT_N, H=H, F=F, p=p))
        for n in (1, 5):
            cases.append(dict(layer=layer, n=n, H=3, F=16, p=R.ATT_P))
    for c in cases:
        c["id"] = "{layer}-n{n}-H{H}-F{F}-p{p}".format(**c)
    return cases


MEAN_CASES = _mean_cases()
SMALL_MULTI_HEAD = [c for c in MEAN_CASES if c["H"] > 1 and (c["n"] < R.ATT_N or c["F"] <= 16)]


def mean_inputs(case):
    """att_inputs(case) with a zero concat bias and dout = dmean[n,F] broadcast over the heads; dmean and bias_f [F]
    come from the same seeded generator family"""
    inp = R.att_inputs(case)
    g = R._gen(case["n"], case["H"], case["F"], len(case["layer"]), int(case["p"] * 10), 41)
    inp.dmean = torch.randn(case["n"], case["F"], generator=g)
    inp.bias_f = torch.randn(case["F"], generator=g)
    inp.bias = torch.zeros(case["H"] * case["F"])
    inp.dout = inp.dmean.unsqueeze(1).expand(case["n"], case["H"], case["F"]).contiguous()
    return inp


def mean_eval(inp, dtype, bug=None):
    """float64: the reference; float32: a correct fp32 evaluation; bug=: one of the wrong variants"""
    H = inp.H
    r = R.att_eval(inp, dtype, bug=bug if bug in R.ATT_BUGS else None)
    bias = inp.bias_f.to(dtype) * (H if bug == "bias_times_heads" else 1)
    o = r.out.sum(1) if bug == "sum_not_mean" else r.out.mean(1)
    out = R.Box(out=o + bias, alpha=r.alpha)
    for k in GRAD_KEYS[inp.layer]:
        out[k] = r[k] if bug == "bwd_no_head_scale" else r[k] / H
    return out


def mean_reference(inp):
    """-> (ref, bounds) of the head-mean entries for `inp` (module docstring)"""
    H = inp.H
    ref = R.att_eval(inp, F64)
    b = R.att_bounds(inp, ref)
    out = R.Box(out=ref.out.mean(1) + inp.bias_f.double(), alpha=ref.alpha)
    bounds = R.Box(alpha=b.alpha,
                   out=R.fin(b.out).mean(1) + (H + 2) * U * (ref.out.abs().mean(1) + inp.bias_f.double().abs()))
    for k in GRAD_KEYS[inp.layer]:
        out[k] = ref[k] / H
        bounds[k] = R.fin(b[k]) / H + 2 * U * (ref[k] / H).abs()
    return out, bounds


def mean_ratios(got, ref, b):
    assert all(tuple(got[k].shape) == tuple(ref[k].shape) for k in b), {k: (tuple(got[k].shape), tuple(ref[k].shape)) for k in b}
    return {k: R.ratio(got[k], ref[k], b[k]) for k in b}


# ====================================================================================================== model level
def graphmil_mean_shapes(input_dim, cfg):
    """state-dict names / shapes of GraphMIL(gnn_type in {gat, gatv2, transformer}, gnn_concat=False): every width that
    concat=True multiplies by the head count is F, except the projections that feed the heads and the attention vectors"""
    c = dict(G.DEFAULT_CFG, **cfg)
    t, H, F_ = c["gnn_type"], c["gnn_heads"], c["gnn_hidden"]
    assert t in ("gat", "gatv2", "transformer"), t
    s = G.graphmil_shapes(input_dim, dict(cfg, gnn_heads=1))            # one head: every width is F
    for i in range(c["gnn_layers"]):
        pre = f"gnn_layers.{i}"
        if t == "gat":
            s[f"{pre}.att_src"] = s[f"{pre}.att_dst"] = (1, H, F_)
            s[f"{pre}.lin.weight"] = (H * F_, s[f"{pre}.lin.weight"][1])
        elif t == "gatv2":
            s[f"{pre}.att"] = (1, H, F_)
            for nm in ("lin_l", "lin_r"):
                s[f"{pre}.{nm}.weight"] = (H * F_, s[f"{pre}.{nm}.weight"][1])
                s[f"{pre}.{nm}.bias"] = (H * F_,)
        else:
            for nm in ("lin_key", "lin_query", "lin_value"):
                s[f"{pre}.{nm}.weight"] = (H * F_, s[f"{pre}.{nm}.weight"][1])
                s[f"{pre}.{nm}.bias"] = (H * F_,)
    return s


def _attention_dropout(c, drop, i):
    if drop is None or c["gnn_dropout"] <= 0:
        return None
    return {"p": c["gnn_dropout"], "seed": drop["seed"], "stream": drop["stream_base"] + 32 + i}


def _transformer_mean(h, edge_index, p, pre, heads, adrop):
    """TransformerConv(concat=False, beta=True, root_weight=True): the aggregate of oracle.gnn.transformer_conv averaged
    over the heads, then the gate on [N,F] with lin_skip Linear(in, F) and lin_beta Linear(3F, 1)"""
    n = h.size(0)
    lin = lambda name: Fn.linear(h, p[f"{pre}.{name}.weight"], p[f"{pre}.{name}.bias"])      # noqa: E731
    q, k, v = (lin(nm).view(n, heads, -1) for nm in ("lin_query", "lin_key", "lin_value"))
    src, dst = edge_index[0], edge_index[1]
    e = (q[dst] * k[src]).sum(-1) / math.sqrt(q.shape[-1])
    alpha = G._alpha_dropout(G._edge_softmax(e, dst, n), G._dst_major_slots(src, dst), adrop) if src.numel() else e
    out = torch.zeros(n, heads, v.shape[-1], dtype=h.dtype).index_add_(0, dst, alpha.unsqueeze(-1) * v[src]).mean(1)
    xr = lin("lin_skip")
    beta = torch.sigmoid(Fn.linear(torch.cat([out, xr, out - xr], dim=-1), p[f"{pre}.lin_beta.weight"]))
    return beta * xr + (1.0 - beta) * out


def graphmil_mean_forward(p, cfg, x, edge_index, drop=None):
    """GraphMIL.forward with gnn_concat=False for gat / gatv2 / transformer -> dict(probs, att, hs, z, logits);
    ``drop`` as in oracle.gnn.graphmil_forward"""
    c = dict(G.DEFAULT_CFG, **cfg)
    t, H = c["gnn_type"], c["gnn_heads"]
    x_in = Fn.linear(x, p["input_proj.weight"], p["input_proj.bias"]) if "input_proj.weight" in p else x
    h, hs = x_in, []
    for i in range(c["gnn_layers"]):
        h_prev, n, pre = h, h.size(0), f"gnn_layers.{i}"
        adrop = _attention_dropout(c, drop, i)
        if t == "gat":
            zero = torch.zeros(p[f"{pre}.lin.weight"].shape[0], dtype=h.dtype)
            o = G.gat_conv(h, edge_index, p[f"{pre}.lin.weight"], p[f"{pre}.att_src"], p[f"{pre}.att_dst"], zero, H, 0.2, adrop)
            h = o.view(n, H, -1).mean(1) + p[f"{pre}.bias"]
        elif t == "gatv2":
            zero = torch.zeros(p[f"{pre}.lin_l.weight"].shape[0], dtype=h.dtype)
            o = G.gatv2_conv(h, edge_index, p[f"{pre}.lin_l.weight"], p[f"{pre}.lin_l.bias"], p[f"{pre}.lin_r.weight"],
                             p[f"{pre}.lin_r.bias"], p[f"{pre}.att"], zero, H, 0.2, adrop)
            h = o.view(n, H, -1).mean(1) + p[f"{pre}.bias"]
        elif t == "transformer":
            h = _transformer_mean(h, edge_index, p, pre, H, adrop)
        else:
            raise ValueError(f"no heads to average in gnn_type {t}")
        if c["use_layer_norm"]:
            h = Fn.layer_norm(h, (h.shape[1],), p[f"layer_norms.{i}.weight"], p[f"layer_norms.{i}.bias"])
        h = Fn.relu(h)
        if drop is not None:
            h = _mil.dropout(h, c["gnn_dropout"], drop["seed"], drop["stream_base"] + i,
                             elem_offset=int(drop.get("node_offset", 0)) * h.shape[1])
        if c["use_residual"] and h_prev.shape == h.shape:
            h = h + h_prev
        hs.append(h)
    atts, pooled = [], []
    for hd in range(c["att_heads"]):
        tt = torch.tanh(Fn.linear(h, p[f"attention_layers.{hd}.0.weight"], p[f"attention_layers.{hd}.0.bias"]))
        a = torch.softmax(Fn.linear(tt, p[f"attention_layers.{hd}.2.weight"], p[f"attention_layers.{hd}.2.bias"]), dim=0)
        atts.append(a)
        pooled.append(torch.sum(a * h, dim=0))
    z = torch.stack(pooled, dim=0).mean(dim=0)
    att = torch.cat(atts, dim=1)
    u = Fn.relu(Fn.linear(z, p["classifier.0.weight"], p["classifier.0.bias"]))
    if drop is not None:
        u = _mil.dropout(u, c["pool_dropout"], drop["seed"], drop["stream_base"] + 64,
                         elem_offset=int(drop.get("graph_index", 0)) * u.shape[0])
    logits = Fn.linear(u, p["classifier.3.weight"], p["classifier.3.bias"])
    return {"probs": torch.softmax(logits, dim=0), "att": att, "hs": hs, "z": z, "logits": logits}


def graphmil_mean_loss_and_grads(p, cfg, x, edge_index, y):
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xx = x.detach().clone().requires_grad_(True)
    out = graphmil_mean_forward(q, cfg, xx, edge_index)
    loss = G.graph_loss(out["probs"], y)
    loss.backward()
    g = {k: (v.grad.detach() if v.grad is not None else torch.zeros_like(v)) for k, v in q.items()}
    g["x"] = xx.grad.detach()
    out = {k: ([t.detach() for t in v] if isinstance(v, list) else v.detach()) for k, v in out.items()}
    return loss.detach(), out, g
