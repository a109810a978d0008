"""Times the k-NN build among the lesion patches of 2048 images (768 features; lesion sizes from the synthetic elliptic flags
that hetero_ragged_bench.py draws) on the MI355X only (no GPU -> exit 1), in four pairs:
  topk_lesion   isic_knn_graph (k = 16; the 208-node Gram kernel whatever the graph's size) against isic_knn_graph_ragged
                (work sized by each graph) on the same ragged batch, outputs allocated outside the timing
  edges_lesion  the ten edge lists (k = 1..8, 12, 16, each graph with its own clamp) by the torch ops of
                build_graphs.knn_edge_index_batched run once per group of graphs that share a clamped k (the groups' row
                indices are formed outside the timing), against isic_hip.graph.knn_edges_ragged (one launch, host-side
                offsets, the 4-byte check read-back included)
  topk_196      both top-16 entries on an equal-size batch of 2048 graphs of 196 nodes (the reference's case, which stays
                with isic_knn_graph)
  topk_128      ... and of 128 nodes: 64 of the 169 tiles, the largest graphs of the 8-wave class (the bound up to which
                isic_hip.graph.knn_indices_ragged takes the sized kernel, KNN_RAGGED_MAX_MEAN_TILES)
Wall time per call with a device synchronise at the end of each timed run of --reps calls; the two sides of a pair alternate
run by run; run 0 warms both up.  Before timing, the two sides of every pair are compared on the timed inputs: the top-k
outputs must be bit-equal and the edge lists identical.  Reported per side: the median over the runs, the run-to-run range
(max - min), and for every pair new / old; a difference counts when it exceeds three times the wider range of the two
(DESIGN.md §6).  There is no pass mark: the numbers are a record, and the dispatch of isic_hip.graph.knn_indices_ragged
(KNN_RAGGED_USE_SIZED_KERNEL, KNN_RAGGED_MAX_MEAN_TILES) is set by them.

    python tools/knn_ragged_bench.py [--runs 5] [--reps 200] [--out profiles/knn_ragged_bench.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "multimodal-isic_amd"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

IMAGES, NODES, FEAT, K = 2048, 196, 768, 16
K_VALUES = tuple(range(1, 9)) + (12, 16)


def wall_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def summary(ts):
    return {"runs_ms": [round(t, 4) for t in ts], "median_ms": float(np.median(ts)), "range_ms": float(np.max(ts) - np.min(ts))}


def compare(old, new):
    diff, bound = abs(old["median_ms"] - new["median_ms"]), 3.0 * max(old["range_ms"], new["range_ms"])
    return {"new_over_old": new["median_ms"] / old["median_ms"], "difference_ms": diff, "three_times_wider_range_ms": bound,
            "exceeds": bool(diff > bound)}


def time_pair(old, new, runs, reps):
    ts = {"old": [], "new": []}
    for r in range(runs + 1):                                             # run 0 warms both sides up
        for name, fn in (("old", old), ("new", new)) if r % 2 else (("new", new), ("old", old)):
            t = wall_ms(fn, reps)
            if r:
                ts[name].append(t)
    out = {k: summary(v) for k, v in ts.items()}
    out["new_vs_old"] = compare(out["old"], out["new"])
    return out


def torch_edge_lists(nn, groups, base):
    """The edge lists of every k by the ops of ``build_graphs.knn_edge_index_batched`` (slice, add, expand, stack, long), which
    need one k for all rows: run once per group of graphs that share a clamped k, the pieces joined per k."""
    out = {}
    for k, per_kk in groups.items():
        parts = []
        for kk, rows in per_kk:
            dst = nn[rows][:, :kk] + base[rows][:, None]
            src = rows[:, None].expand(-1, kk)
            parts.append(torch.stack([src.reshape(-1), dst.reshape(-1)], dim=0).long())
        out[k] = torch.cat(parts, dim=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="calls per side inside one timed run (a window of 0.04 .. 0.35 s)")
    ap.add_argument("--images", type=int, default=IMAGES)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("knn_ragged_bench: no GPU found (this tool measures the MI355X only)", file=sys.stderr)
        sys.exit(1)
    from hetero_ragged_bench import elliptic_flags
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import knn_edge_counts, knn_edges_ragged
    from isic_hip.lib import call
    dev = torch.device("cuda", 0)
    G = a.images
    rng = np.random.default_rng(7)
    sizes = np.asarray([max(1, int(elliptic_flags(rng).sum())) for _ in range(G)], dtype=np.int64)
    res = {"tool": "knn_ragged_bench", "device": torch.cuda.get_device_name(0), "runs": a.runs, "calls_per_side_and_run": a.reps,
           "images": G, "features": FEAT, "k": K, "k_values": list(K_VALUES), "unit": "ms of wall time per call",
           "lesion_nodes_min_mean_max": [int(sizes.min()), float(sizes.mean()), int(sizes.max())],
           "lesion_tiles_multiplied_of_169_mean": float((np.ceil(sizes / 16.0) ** 2).mean())}
    gen = torch.Generator(device=dev).manual_seed(1234)

    def topk_pair(offs):
        x = torch.randn(offs.total, FEAT, device=dev, generator=gen)
        T = offs.total
        oi, od = torch.empty((T, K), device=dev, dtype=torch.int64), torch.empty((T, K), device=dev, dtype=torch.float32)
        ni, nd = torch.empty_like(oi), torch.empty_like(od)
        ws = torch.empty(T, device=dev, dtype=torch.float32)
        old = lambda: call("isic_knn_graph", x, offs.device, offs.num_bags, FEAT, K, offs.max_bag, T, oi, od, ws)      # noqa: E731
        new = lambda: call("isic_knn_graph_ragged", x, offs.device, offs.num_bags, FEAT, K, offs.max_bag, T, ni, nd)   # noqa: E731
        old(), new()
        torch.cuda.synchronize()
        if not (torch.equal(oi, ni) and torch.equal(od, nd)):
            raise SystemExit("knn_ragged_bench: isic_knn_graph_ragged and isic_knn_graph differ on the timed batch")
        return time_pair(old, new, a.runs, a.reps), ni

    offs = BagOffsets.from_lengths(sizes, dev)
    res["topk_lesion"], nn = topk_pair(offs)
    res["topk_lesion"]["sides"] = {"old": "isic_knn_graph", "new": "isic_knn_graph_ragged"}

    # the torch route: per k, the graphs grouped by their clamped k (row indices formed here, outside the timing)
    node_graph = np.repeat(np.arange(G), sizes)
    base = torch.from_numpy(np.repeat(offs.host[:-1], sizes)).to(dev)
    cnt = knn_edge_counts(sizes, K_VALUES)
    groups = {}
    for q, k in enumerate(K_VALUES):
        kk_g = cnt[q] // np.maximum(sizes, 1)
        groups[k] = [(int(kk), torch.from_numpy(np.flatnonzero(kk_g[node_graph] == kk)).to(dev)) for kk in np.unique(kk_g) if kk > 0]
    res["edges_lesion_torch_groups"] = int(sum(len(v) for v in groups.values()))
    old = lambda: torch_edge_lists(nn, groups, base)                       # noqa: E731
    new = lambda: knn_edges_ragged(nn, offs, K_VALUES, global_ids=True)    # noqa: E731
    want, got = old(), new()
    for q, k in enumerate(K_VALUES):                                       # the torch pieces are grouped by kk: compare as edge sets per source
        a_, b_ = want[k], got[k][0]
        if a_.shape != b_.shape or not torch.equal(a_[:, torch.argsort(a_[0], stable=True)], b_.contiguous()):
            raise SystemExit(f"knn_ragged_bench: the edge lists of k = {k} differ between the two routes")
    res["edges_lesion"] = time_pair(old, new, a.runs, a.reps)
    res["edges_lesion"]["sides"] = {"old": "torch ops per constant-k group", "new": "isic_hip.graph.knn_edges_ragged"}
    res["edges_lesion"]["edges_total"] = int(cnt.sum())

    del nn, base, groups, want, got
    res["topk_196"], _ = topk_pair(BagOffsets.uniform(G, NODES, dev))
    res["topk_196"]["sides"] = {"old": "isic_knn_graph", "new": "isic_knn_graph_ragged"}
    res["topk_128"], _ = topk_pair(BagOffsets.uniform(G, 128, dev))
    res["topk_128"]["sides"] = {"old": "isic_knn_graph", "new": "isic_knn_graph_ragged"}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
