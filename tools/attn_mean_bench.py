"""Times one head-averaged attention layer (``concat=False``), forward + backward, on the fused path against the composite
it replaces, on the MI355X only (no GPU -> exit 1).

Geometry of the graph benchmark: 668 graphs x 196 nodes, k-NN k = 8, H 4, F 128, for each of GATConv, GATv2Conv and
TransformerConv's attention.
  fused      ``gat_conv / gatv2_conv / transformer_attention(concat=False)``: the mean over heads inside the kernels, out and
             dout are [N,F]
  composite  the concat autograd functions with a zero [H*F] bias, then ``view(N,H,F).mean(1) + bias`` in torch: an
             [N,H,F] tensor written and re-read in the forward, an [N,H,F] broadcast of dout in the backward
The two alternate in one process after a warm-up call of each; every repetition is device-synchronised and timed with
device events; median and min-max of the repetitions.  There is no pass mark: the numbers are a record.

    python tools/attn_mean_bench.py [--reps 5] [--out profiles/attn_mean_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-isic_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GRAPHS, NODES, K, H, F = 668, 196, 8, 4, 128


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts))}


def layer_steps(kind, graph, gen):
    """-> (fused step, composite step): each runs forward + backward and returns (out, gradients of the inputs)"""
    from isic_hip.graph import gat_conv, gatv2_conv, transformer_attention
    N = GRAPHS * NODES
    mk = lambda *s: torch.randn(*s, generator=gen).cuda().requires_grad_(True)      # noqa: E731
    dout = torch.randn(N, F, generator=gen).cuda()
    bias = mk(F)
    zero = torch.zeros(H * F, device="cuda")
    if kind == "gat":
        ins = [mk(N, H * F), mk(1, H, F), mk(1, H, F)]
        layer = lambda b, concat: gat_conv(ins[0], ins[1], ins[2], b, graph, H, 0.2, None, concat=concat)      # noqa: E731
    elif kind == "gatv2":
        ins = [mk(N, H * F), mk(N, H * F), mk(1, H, F)]
        layer = lambda b, concat: gatv2_conv(ins[0], ins[1], ins[2], b, graph, H, 0.2, None, concat=concat)      # noqa: E731
    else:
        ins = [mk(N, H * F), mk(N, H * F), mk(N, H * F)]
        bias = None                                                    # TransformerConv's attention has no bias of its own
        layer = lambda b, concat: transformer_attention(ins[0], ins[1], ins[2], graph, H, None, concat=concat)      # noqa: E731
    leaves = ins + ([bias] if bias is not None else [])

    def fused():
        out = layer(bias, False)
        return out, torch.autograd.grad(out, leaves, dout)

    def composite():
        out = layer(zero if bias is not None else None, True).view(N, H, F).mean(1)
        if bias is not None:
            out = out + bias
        return out, torch.autograd.grad(out, leaves, dout)

    return fused, composite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("attn_mean_bench: no GPU found (this tool measures the MI355X only)", file=sys.stderr)
        sys.exit(1)
    import build_graphs as bg
    from isic_hip.graph import GraphBatch
    gen = torch.Generator().manual_seed(0)
    N = GRAPHS * NODES
    offs = np.arange(GRAPHS + 1) * NODES
    ei = bg.knn_edge_index_batched(torch.randn(N, 64, generator=gen).cuda(), offs, (K,))[K]
    res = {"tool": "attn_mean_bench", "device": torch.cuda.get_device_name(0), "graphs": GRAPHS, "nodes_per_graph": NODES,
           "knn_k": K, "heads": H, "features": F, "edges": int(ei.shape[1]), "reps": a.reps, "layers": {}}
    for kind, mode in (("gat", "gcn"), ("gatv2", "gcn"), ("transformer", "sum")):
        graph = GraphBatch(ei, N, None, mode=mode)
        fused, composite = layer_steps(kind, graph, gen)
        (of, gf), (oc, gc) = fused(), composite()                      # warm-up, and the two paths agree
        diff = max(float((of - oc).detach().abs().max()), max(float((x - y).abs().max()) for x, y in zip(gf, gc)))
        tf, tc = [], []
        for _ in range(a.reps):
            tf.append(timed(fused)[0])
            tc.append(timed(composite)[0])
        sf, sc = stats(tf), stats(tc)
        res["layers"][kind] = {"fused": sf, "composite": sc, "composite_over_fused": sc["ms_median"] / sf["ms_median"],
                               "fused_faster_by_more_than_composite_range": bool(sc["ms_median"] - sf["ms_median"]
                                                                                 > sc["ms_max"] - sc["ms_min"]),
                               "max_abs_diff": diff}
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
