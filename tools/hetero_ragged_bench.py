"""Times the heterophily summaries of one chunk of 64 images (196 patches, 768 features, 7 classes) over the 22 graph variants
of 05_train_gnns.py (grid4, grid8, knn / random at 1..8, 12, 16) on the MI355X only (no GPU -> exit 1), three ways:
  device        measure_heterophily.heterophily_summary_device: the equal-size path (edge kernel + torch index bookkeeping)
  ragged        measure_heterophily.heterophily_summary_ragged on the same graphs with every node kept and the node count
                passed in: the same work through the entries of include/isic_hip_hetero_ragged.h
  lesion_only   measure_heterophily.heterophily_summary_lesion_only with a synthetic elliptic lesion mask per image
                (graph.induced_subgraphs with its one read-back, one gather, then the ragged path on smaller graphs)
Wall time per chunk (one call, one variant) with a device synchronise at the end of each timed run; a run walks all 22
variants and the three paths alternate variant by variant.  Reported: per path the median over the runs of the mean time per
chunk, the run-to-run range (max - min), and ragged / device.  A difference counts when it exceeds three times the wider range
of the two.  There is no pass mark: the numbers are a record.

    python tools/hetero_ragged_bench.py [--runs 5] [--reps 10] [--out profiles/hetero_ragged_bench.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "multimodal-isic_amd")):
    sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

IMAGES, NODES, FEAT, CLASSES = 64, 196, 768, 7
PARAMS = tuple(range(1, 9)) + (12, 16)
VARIANTS = ["grid4", "grid8"] + [f"knn{k}" for k in PARAMS] + [f"random{r}" for r in PARAMS]


def elliptic_flags(rng, side=14):
    r, c = np.divmod(np.arange(side * side), side)
    cy, cx = rng.uniform(0.3 * side, 0.7 * side, 2)
    ry, rx = rng.uniform(0.15 * side, 0.45 * side, 2)
    return ((r - cy) / ry) ** 2 + ((c - cx) / rx) ** 2 <= 1.0


def wall_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def summary(ts):
    return {"runs_ms": [round(t, 4) for t in ts], "median_ms": float(np.median(ts)), "range_ms": float(np.max(ts) - np.min(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="calls per variant and path inside one timed run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("hetero_ragged_bench: no GPU found (this tool measures the MI355X only)", file=sys.stderr)
        sys.exit(1)
    import measure_heterophily as mh
    from pipeline import DeviceTeacherOutputs
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(IMAGES, NODES, FEAT, device=dev, generator=gen)
    pp = torch.softmax(torch.randn(IMAGES, NODES, CLASSES, device=dev, generator=gen) * 2, dim=2)
    outs = DeviceTeacherOutputs(x, pp, torch.rand(IMAGES, NODES, device=dev), torch.arange(IMAGES, device=dev) % CLASSES,
                                [f"i{i}" for i in range(IMAGES)], kmax=16)
    rng = np.random.default_rng(7)
    keep = torch.from_numpy(np.stack([elliptic_flags(rng) for _ in range(IMAGES)])).to(dev)
    dom = outs.dominant_class
    xf, pf, df = x.reshape(-1, FEAT), pp.reshape(-1, CLASSES), dom.reshape(-1)
    noff = torch.arange(IMAGES + 1, device=dev, dtype=torch.int64) * NODES
    work = {}
    for v in VARIANTS:                                                    # the edges of a variant are built once, outside the timing
        ei = outs.edge_index(v)
        ei = ei.contiguous() if isinstance(ei, torch.Tensor) else ei
        flat, eoff = mh._concat_local_edges(ei, IMAGES, dev)
        work[v] = (ei, flat.contiguous(), eoff)
    paths = {
        "device": lambda v: mh.heterophily_summary_device(x, pp, dom, work[v][0]),
        "ragged": lambda v: mh.heterophily_summary_ragged(xf, pf, df, work[v][1], work[v][2], noff, max_nodes=NODES),
        "lesion_only": lambda v: mh.heterophily_summary_lesion_only(x, pp, dom, work[v][0], keep),
    }
    times = {k: [] for k in paths}
    for r in range(a.runs + 1):                                           # run 0 warms every path and variant up
        acc = {k: 0.0 for k in paths}
        for v in VARIANTS:
            for name, fn in paths.items():
                acc[name] += wall_ms(lambda: fn(v), a.reps)
        if r:
            for k in paths:
                times[k].append(acc[k] / len(VARIANTS))
    res = {"tool": "hetero_ragged_bench", "device": torch.cuda.get_device_name(0), "runs": a.runs, "calls_per_variant_and_run": a.reps,
           "images_per_chunk": IMAGES, "nodes": NODES, "features": FEAT, "classes": CLASSES, "variants": len(VARIANTS),
           "unit": "ms of wall time per chunk (one call, one variant), mean over the variants",
           "lesion_nodes_min_mean_max": [int(keep.sum(1).min()), float(keep.sum(1).float().mean()), int(keep.sum(1).max())]}
    res.update({k: summary(v) for k, v in times.items()})
    d, g = res["device"], res["ragged"]
    diff, bound = abs(d["median_ms"] - g["median_ms"]), 3.0 * max(d["range_ms"], g["range_ms"])
    res["ragged_over_device"] = {"ratio_of_medians": g["median_ms"] / d["median_ms"], "difference_ms": diff,
                                 "three_times_wider_range_ms": bound, "exceeds": bool(diff > bound)}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
