"""Times the ragged patch-graph route on the MI355X only (no GPU -> exit 1): GraphMIL[gcn] at the bench.py "gnn" geometry (196
nodes, 768 features, width 128, 3 layers, 668 graphs per step out of 1336 records), on two record sets whose graphs differ
in size:
  random8       the random (r = 8) graphs of 03_build_graphs.py: 196 nodes each, the edge count differs per image
  lesion-only   k-NN (k = 8) graphs restricted to a synthetic elliptic lesion mask per image (the shape SyntheticDermImages
                draws: random centre and half-axes), induced on the host with numpy so that every checkout sees one record set
Train steps (batch assembly + forward + backward + AdamW, run eagerly: a ragged step cannot be captured, its shapes change),
wall time per step with a device synchronise at the end of each timed run, the paths alternating run by run:
  slow          GraphStore.batch on a device index: per-step concatenation in a Python loop + isic_gcn_csr_build
  ragged        GraphStore(ragged_stack=True).batch_rows on a host index: one small upload + isic_csr_batch_assemble_ragged,
                the input projection reads through the row index (what train_gnn_fold runs)
  ragged_batch  ... .batch: the same assembly, node features gathered (the like-for-like of `slow`)
and the bare entries: graph.induced_subgraphs over all records (two launches, one cumsum, one read-back) and the two batch
assemblies on their own.  The difference of two paths counts when it exceeds three times the wider run-to-run range (max - min
of the runs) of the two: DESIGN.md §6.  There is no pass mark: the numbers are a record.

    python tools/ragged_graph_bench.py [--runs 5] [--steps 10] [--out profiles/ragged_graph_bench.txt]
    python tools/ragged_graph_bench.py --pkg OTHER_CHECKOUT/multimodal-isic_amd --label "parent commit" --slow-only --json-out parent.json
    python tools/ragged_graph_bench.py --parent-json parent.json [alone.json] --out ...     (slow-only runs -- another checkout
                                                       such as the parent commit, this one on its own -- on the same records, beside it)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GRAPHS, PER_STEP, NODES, FEAT, HIDDEN, LAYERS, CLASSES = 1336, 668, 196, 768, 128, 3, 7


def induce_on_host(src, dst, keep):
    k = keep if keep.any() else np.ones_like(keep)
    new = np.cumsum(k) - 1
    m = k[src] & k[dst]
    return np.stack([new[src[m]], new[dst[m]]]), np.nonzero(k)[0]


def elliptic_flags(rng, side=14):
    r, c = np.divmod(np.arange(side * side), side)
    cy, cx = rng.uniform(0.3 * side, 0.7 * side, 2)
    ry, rx = rng.uniform(0.15 * side, 0.45 * side, 2)
    return ((r - cy) / ry) ** 2 + ((c - cx) / rx) ** 2 <= 1.0


def record_sets(dev):
    import build_graphs as bg
    gen = torch.Generator(device=dev).manual_seed(1234)
    y = torch.arange(GRAPHS, device=dev) % CLASSES
    x = torch.randn(GRAPHS, NODES, FEAT, device=dev, generator=gen) + 0.25 * y.view(-1, 1, 1).float()
    rnd = bg.random_edge_index_batched(NODES, [8], list(range(1000, 1000 + GRAPHS)), device=dev)[8]
    random8 = [{"x": x[i], "edge_index": rnd[i], "y": int(y[i])} for i in range(GRAPHS)]
    knn = bg.knn_edge_index_batched(x.view(-1, FEAT)[:, :64].contiguous(), np.arange(GRAPHS + 1) * NODES, (8,))[8]
    knn = (knn.view(2, GRAPHS, -1) - (torch.arange(GRAPHS, device=dev) * NODES).view(1, -1, 1)).permute(1, 0, 2).cpu().numpy()
    rng = np.random.default_rng(7)
    flagged, induced = [], []
    for i in range(GRAPHS):
        keep = elliptic_flags(rng)
        ei, rows = induce_on_host(knn[i, 0], knn[i, 1], keep)
        flagged.append({"x": x[i], "edge_index": torch.from_numpy(knn[i]).to(dev), "y": int(y[i]), "keep": keep})
        induced.append({"x": x[i][torch.from_numpy(rows).to(dev)], "edge_index": torch.from_numpy(ei).to(dev), "y": int(y[i])})
    return random8, flagged, induced


def make_model(dev):
    from gnn_models import GraphMIL
    from isic_hip import optim
    torch.manual_seed(42)
    m = GraphMIL(input_dim=FEAT, gnn_type="gcn", gnn_hidden=HIDDEN, gnn_layers=LAYERS, gnn_dropout=0.5, gnn_heads=4, att_dim=128,
                 att_heads=4, pool_dropout=0.2, classifier_dim=128, classifier_light=True, num_classes=CLASSES).to(dev)
    m.train()
    m.set_dropout_state(seed=42, step=0)
    return m, optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)


def train_step(model, opt, store, path, idx_host, idx_dev):
    from isic_hip import ops
    xr = None
    if path == "slow":
        x, offs, g = store.batch(idx_dev)
    elif path == "ragged_batch":
        x, offs, g = store.batch(idx_host)
    else:
        x, rows, n_rows, offs, g = store.batch_rows(idx_host)
        xr = (rows, n_rows)
    opt.zero_grad()
    with ops.fused_grad_accumulation():
        _, _, loss = model(x, offsets=offs, graph=g, labels=store.y_dev[idx_dev], x_rows=xr)
        ops.backward(loss)
    opt.step()
    return loss


def wall_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def summary(ts):
    return {"runs_ms": [round(t, 4) for t in ts], "median_ms": float(np.median(ts)), "range_ms": float(np.max(ts) - np.min(ts))}


def time_paths(paths, runs, steps, dev):
    """paths: {name: (store, path)} -> {name: summary}; one model, the paths alternate run by run, same index draws per run."""
    model, opt = make_model(dev)
    rng = np.random.default_rng(3)
    draws = [[rng.integers(0, GRAPHS, PER_STEP).tolist() for _ in range(steps)] for _ in range(runs + 1)]
    draws_dev = [[torch.as_tensor(d, device=dev) for d in run] for run in draws]
    out = {k: [] for k in paths}
    for r in range(runs + 1):                                             # run 0 warms every path up
        for name, (store, path) in paths.items():
            t = wall_ms(lambda i: train_step(model, opt, store, path, draws[r][i], draws_dev[r][i]), steps)
            if r:
                out[name].append(t)
    return {k: summary(v) for k, v in out.items()}


def verdict(a, b):
    diff, bound = abs(a["median_ms"] - b["median_ms"]), 3.0 * max(a["range_ms"], b["range_ms"])
    return {"difference_ms": diff, "three_times_wider_range_ms": bound, "exceeds": bool(diff > bound)}


def bare_entries(flagged, stores, slows, runs, dev):
    from isic_hip.graph import induced_subgraphs
    ei = torch.cat([r["edge_index"] for r in flagged], dim=1)
    eoff = np.concatenate([[0], np.cumsum([r["edge_index"].shape[1] for r in flagged])])
    noff = np.arange(GRAPHS + 1) * NODES
    keep = torch.from_numpy(np.concatenate([r["keep"] for r in flagged])).to(dev)
    eoff_d, noff_d = torch.as_tensor(eoff, device=dev), torch.as_tensor(noff, device=dev)
    res = {"induced_subgraphs_all_records": summary([wall_ms(lambda i: induced_subgraphs(ei, eoff_d, noff_d, keep), 5)
                                                     for _ in range(runs + 1)][1:]),
           "graphs": GRAPHS, "edges_in": int(eoff[-1])}
    rng = np.random.default_rng(5)
    idx = rng.integers(0, GRAPHS, PER_STEP).tolist()
    for name, store in stores.items():
        res[f"assemble_ragged[{name}]"] = summary([wall_ms(lambda i: store._ragged_graph(idx, True), 10) for _ in range(runs + 1)][1:])
    idx_dev = torch.as_tensor(idx, device=dev)
    for name, store in slows.items():                                     # features concatenated + CSR rebuilt: GraphStore.batch
        res[f"batch_slow_path[{name}]"] = summary([wall_ms(lambda i: store.batch(idx_dev), 10) for _ in range(runs + 1)][1:])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "multimodal-isic_amd"), help="the package directory to import")
    ap.add_argument("--slow-only", action="store_true", help="time the slow path alone (a checkout without the ragged route)")
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--label", default="this checkout", help="what --pkg is, for the record (e.g. 'parent commit <sha>')")
    ap.add_argument("--parent-json", nargs="+", default=None,
                    help="--slow-only --json-out results of other runs (another checkout, this one's slow path alone), reported beside")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("ragged_graph_bench: no GPU found (this tool measures the MI355X only)", file=sys.stderr)
        sys.exit(1)
    for p in (os.path.dirname(os.path.abspath(a.pkg)), os.path.abspath(a.pkg)):
        sys.path.insert(0, p)
    from isic_hip import train as T
    dev = torch.device("cuda", 0)
    random8, flagged, induced = record_sets(dev)
    res = {"tool": "ragged_graph_bench", "device": torch.cuda.get_device_name(0), "package": a.label,
           "runs": a.runs, "steps_per_run": a.steps, "graphs_per_step": PER_STEP, "records": GRAPHS,
           "random8_edges_min_max": [min(r["edge_index"].shape[1] for r in random8), max(r["edge_index"].shape[1] for r in random8)],
           "lesion_nodes_min_mean_max": [min(r["x"].shape[0] for r in induced), float(np.mean([r["x"].shape[0] for r in induced])),
                                         max(r["x"].shape[0] for r in induced)]}
    for name, recs in (("random8", random8), ("lesion_only", induced)):
        slow = T.GraphStore(recs, dev, True, mode="gcn")
        assert slow._stack is None, "the record set is not ragged"
        paths = {"slow": (slow, "slow")}
        if not a.slow_only:
            fast = T.GraphStore(flagged, dev, True, mode="gcn", lesion_only=True, ragged_stack=True) if name == "lesion_only" \
                else T.GraphStore(recs, dev, True, mode="gcn", ragged_stack=True)
            assert fast._ragged is not None
            paths.update({"ragged": (fast, "ragged"), "ragged_batch": (fast, "ragged_batch")})
        res[name] = time_paths(paths, a.runs, a.steps, dev)
        if not a.slow_only:
            res[name]["slow_vs_ragged"] = verdict(res[name]["slow"], res[name]["ragged"])
            res[name]["slow_vs_ragged_batch"] = verdict(res[name]["slow"], res[name]["ragged_batch"])
            res.setdefault("stores", {})[name] = fast
            res.setdefault("slows", {})[name] = slow
    if not a.slow_only:
        stores = res.pop("stores")
        res["entries"] = bare_entries(flagged, stores, res.pop("slows"), a.runs, dev)
    if a.parent_json:
        res["slow_only_runs"] = []
        for path in a.parent_json:
            with open(path) as f:
                other = json.load(f)
            res["slow_only_runs"].append({k: other[k] for k in ("package", "random8", "lesion_only")})
            for name in ("random8", "lesion_only"):
                res["slow_only_runs"][-1][f"{name}_vs_ragged_here"] = verdict(other[name]["slow"], res[name]["ragged"])
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    for path in (a.out, a.json_out):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
