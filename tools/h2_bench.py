"""Times H2GCN's device work (include/isic_hip_h2.h) on the MI355X only (no GPU -> exit 1), per graph variant -- grid8, knn8
and random8 over 668 graphs of 196 nodes, the bench's graph step:

  (a) the builder ``two_hop`` (count, scan, one read-back, write) against a device ``bmm`` restatement -- a dense [G, n, n]
      adjacency scattered from the edge list, its thresholded square, ``nonzero`` -- which is what this project would have to
      run without the bit-row kernels;
  (b) the bare ``isic_h2_prop_f32`` / ``isic_h2_prop_bwd_f32`` entries at F = 128 against the composed path (two
      ``isic_spmm_csr_f32`` calls plus ``torch.cat``), and forward + backward of both paths under autograd;
  (c) the whole ``GraphMIL[h2gcn]`` train step, L = 2, hidden 128 (forward + backward + AdamW under
      ``fused_grad_accumulation``, captured into a hipGraph and replayed) through each path, next to ``GraphMIL[gcn]``;
  (d) the mean and the longest row of both operators.
Everything that is compared is ALTERNATED in one process after a warm-up of all of it; medians and the run-to-run range
(min .. max) of each are reported.  The rule the default of ``h2_prop`` follows (isic_hip.graph.H2_RESIDENT_DEFAULT): the
resident kernel is the default only if its advantage on the WHOLE step exceeds three times the wider of the two ranges, on
every variant; ``verdict`` applies it to this run's numbers.

    python tools/h2_bench.py [--reps 7] [--steps 10] [--variants grid8 knn8 random8] [--out profiles/h2_bench.txt]
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

GRAPHS, NODES, FEAT, HIDDEN, LAYERS, CLASSES = 668, 196, 768, 128, 2, 7


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return {"ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)),
            "ms_range": float(np.max(ts) - np.min(ts))}


def alternate(fns, reps, n):
    """{name: stats} of n calls per repetition, the candidates taking turns inside every repetition"""
    for f in fns.values():
        f()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(timed(lambda: [f() for _ in range(n)]) / n)
    return {k: stats(v) for k, v in ts.items()}


def edges(variant, x):
    """the variant's edge list over the whole batch, GLOBAL ids, int64 [2, E] on the device"""
    import build_graphs as bg
    dev = x.device
    base = torch.arange(GRAPHS, device=dev, dtype=torch.int64) * NODES
    if variant == "grid8":
        ei = bg._grid_edge_index(True).to(dev)
        return (ei.unsqueeze(1) + base.view(1, GRAPHS, 1)).reshape(2, -1)
    if variant == "knn8":
        return bg.knn_edge_index_batched(x[:, :64].contiguous(), np.arange(GRAPHS + 1) * NODES, (8,))[8]
    if variant == "random8":
        per = bg.random_edge_index_batched(NODES, (8,), [1000 + g for g in range(GRAPHS)], device=dev)[8]
        return torch.cat([e.to(dev) + int(b) for e, b in zip(per, base.tolist())], dim=1)
    raise ValueError(variant)


def bmm_two_hop(ei, G, n):
    """the restatement on the device: dense adjacency, one bmm, thresholds, nonzero -> the entry counts of both operators"""
    g, s, d = ei[0] // n, ei[0] % n, ei[1] % n
    A = torch.zeros((G, n, n), device=ei.device, dtype=torch.float32)
    A[g, s, d] = 1.0
    A[g, d, s] = 1.0
    eye = torch.eye(n, device=ei.device, dtype=torch.bool)
    A1 = (A > 0) & ~eye
    A2 = (torch.bmm(A1.float(), A1.float()) > 0) & ~A1 & ~eye
    return A1.nonzero(), A2.nonzero()


def builder(ei, offs, reps, n):
    from isic_hip.graph import GraphBatch, two_hop
    graph = GraphBatch(ei, offs.total, None, mode="sum")
    pair = two_hop(graph, offs)
    n1, n2 = bmm_two_hop(ei, GRAPHS, NODES)
    assert n1.shape[0] == pair.a1.col.numel() and n2.shape[0] == pair.a2.col.numel()
    out = alternate({"two_hop": lambda: two_hop(graph, offs), "bmm_restatement": lambda: bmm_two_hop(ei, GRAPHS, NODES)}, reps, n)
    rows = {}
    for name, op in (("a1", pair.a1), ("a2", pair.a2)):
        d = torch.diff(op.rowptr).double()
        rows[name] = {"entries": int(op.col.numel()), "mean_row": float(d.mean()), "longest_row": int(d.max())}
    return pair, out, rows


def entries(pair, offs, reps, n):
    from isic_hip import graph as G
    from isic_hip.lib import call
    N, F = offs.total, HIDDEN
    gen = torch.Generator().manual_seed(0)
    h, dz = torch.randn(N, F, generator=gen).cuda(), torch.randn(N, 2 * F, generator=gen).cuda()
    z, dh = torch.empty(N, 2 * F, device="cuda"), torch.empty(N, F, device="cuda")
    bad = torch.zeros(1, device="cuda", dtype=torch.int32)
    a1, a2 = pair.a1, pair.a2
    csr = (a1.rowptr, a1.col, a1.val, int(a1.col.numel()), a2.rowptr, a2.col, a2.val, int(a2.col.numel()), offs.device,
           offs.num_bags, offs.max_bag, N)

    def fwd():
        call("isic_h2_prop_f32", *csr, h, F, F, z, 2 * F, bad)

    def bwd():
        call("isic_h2_prop_bwd_f32", *csr, dz, 2 * F, F, dh, F, bad)

    def composed_fwd():
        with torch.no_grad():
            G.h2_prop_composed(h, pair)

    def composed_bwd():
        with torch.no_grad():
            G.spmm(dz[:, :F].contiguous(), a1) + G.spmm(dz[:, F:].contiguous(), a2)

    out = alternate({"resident_fwd": fwd, "resident_bwd": bwd, "composed_fwd": composed_fwd, "composed_bwd": composed_bwd}, reps, n)
    assert int(bad.item()) == 0

    def fb(resident):
        hh = h.clone().requires_grad_(True)

        def run():
            hh.grad = None
            G.h2_prop(hh, pair, offs, resident=resident, bad=bad).backward(dz)
        return run
    out.update({"autograd_" + k: v for k, v in alternate({"resident_fwd_bwd": fb(True), "composed_fwd_bwd": fb(False)}, reps, n).items()})
    return out


def step(gtype, resident, x, y, offs, graph):
    from gnn_models import GraphMIL
    from isic_hip import graphs as GR, ops, optim
    torch.manual_seed(42)
    m = GraphMIL(input_dim=FEAT, gnn_type=gtype, gnn_hidden=HIDDEN, gnn_layers=LAYERS, gnn_dropout=0.5, att_dim=128, att_heads=4,
                 pool_dropout=0.2, classifier_dim=128, classifier_light=True, num_classes=CLASSES).cuda()
    m.h2_resident = resident
    m.train()
    m.set_dropout_state(seed=42, step=0)
    opt = optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    clock = GR.StepClock(x.device).attach(m, opt)

    def body():
        opt.zero_grad()
        with ops.fused_grad_accumulation():
            _, _, loss = m(x, offsets=offs, graph=graph, labels=y)
            ops.backward(loss)
        opt.step()
        clock.advance()
        return loss
    return GR.CapturedStep(body, optimizer=opt, clock=clock)


def verdict(res_s, com_s):
    adv = com_s["ms_median"] - res_s["ms_median"]
    wider = max(res_s["ms_range"], com_s["ms_range"])
    return {"advantage_ms": adv, "wider_range_ms": wider, "resident_is_default": bool(adv > 3.0 * wider)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--variants", nargs="+", default=["grid8", "knn8", "random8"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("h2_bench: no GPU found (this tool measures the MI355X only)", file=sys.stderr)
        sys.exit(1)
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import GraphBatch
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1234)
    T = GRAPHS * NODES
    y = torch.arange(GRAPHS, device=dev) % CLASSES
    x = (torch.randn(GRAPHS, NODES, FEAT, device=dev, generator=gen) + 0.25 * y.view(-1, 1, 1).float()).reshape(T, FEAT)
    offs = BagOffsets.uniform(GRAPHS, NODES, dev)
    res = {"tool": "h2_bench", "device": torch.cuda.get_device_name(0), "graphs": GRAPHS, "nodes": NODES, "F": HIDDEN,
           "layers": LAYERS, "reps": a.reps, "calls_per_rep": a.steps, "variants": {}}
    for variant in a.variants:
        ei = edges(variant, x)
        pair, b, rows = builder(ei, offs, a.reps, max(1, a.steps // 2))
        r = {"edges": int(ei.shape[1]), "rows": rows, "builder": b, "entries": entries(pair, offs, a.reps, a.steps)}
        steps = {"h2gcn_resident": step("h2gcn", True, x, y, offs, pair), "h2gcn_composed": step("h2gcn", False, x, y, offs, pair),
                 "gcn": step("gcn", None, x, y, offs, GraphBatch(ei, T, None, mode="gcn"))}
        r["train_step"] = alternate({k: s.replay for k, s in steps.items()}, a.reps, a.steps)
        r["loss"] = {k: float(s.replay().detach()) for k, s in steps.items()}
        r["verdict_entries_fwd_bwd"] = verdict(r["entries"]["autograd_resident_fwd_bwd"], r["entries"]["autograd_composed_fwd_bwd"])
        r["verdict_train_step"] = verdict(r["train_step"]["h2gcn_resident"], r["train_step"]["h2gcn_composed"])
        res["variants"][variant] = r
        del steps, pair
        torch.cuda.empty_cache()
    res["resident_is_default"] = all(v["verdict_train_step"]["resident_is_default"] for v in res["variants"].values())
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
