"""Times the build of the reference's random graphs AMONG the lesion patches of 2048 images (lesion sizes from the synthetic
elliptic flags of tools/ragged_graph_bench.py; the ten r values 1..8, 12, 16; image i seeded with 42 + i) on the MI355X only
(no GPU -> exit 1):
  lesion      three routes to the same edge lists, each ending with the lists on the device or, for the host loop, in host memory:
                host     build_graphs._random_edge_index(n_g, r, seed) per image and r (the reference's loop, torch on the CPU)
                grouped  what the library could do before: the graphs grouped by node count, isic_hip.graph.random_graphs
                         once per distinct count (a launch and a read-back each; the grouping is done outside the timing)
                ragged   isic_hip.graph.random_graphs_ragged (two launches, one read-back)
              and, as `lesion_launches`, the device work of the last two alone: the bare isic_random_graph_i64 launches of
              the grouped route (one per distinct count) against the bare count launch, the prefix sums on the device and
              the bare write launch, all into buffers allocated before -- no read-back, no slicing of results in Python
  equal_196   2048 graphs of 196 nodes, the reference's case: random_graphs against random_graphs_ragged (a 256-lane workgroup
              per graph on both sides), and `equal_196_launches`, the bare launches as above (one launch against count +
              prefix sums + write: the ragged route generates every graph twice), and `equal_196_one_pass`, one generation
              on each side: the old launch against the count launch with its prefix sums
  equal_64 / equal_32   ... of 64 and of 32 nodes: a workgroup per graph against a wave per graph, four to a workgroup -- the
              packing isic_hip.graph.RANDOM_RAGGED_PACK_NODES records
Wall time per call with a device synchronise at the end of each timed run of --reps calls (--launch-reps for the bare launches); the two device sides of a pair
alternate run by run; run 0 warms both up (every shape of the grouped route included).  The host loop is timed --host-runs
times after a warm-up on 64 images.  Before timing, the routes are compared on the timed inputs: grouped and ragged must be
identical per graph and r, the host loop identical on every 16th image.  Reported per side: the median over the runs, the
run-to-run range (max - min), and for every pair new / old; a difference counts when it exceeds three times the wider range
of the two.  There is no pass mark: the numbers are a record.

    python tools/rand_graph_ragged_bench.py [--runs 5] [--reps 20] [--launch-reps 200] [--host-runs 2] [--out profiles/rand_graph_ragged_bench.txt]
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

IMAGES, NODES = 2048, 196
R_VALUES = tuple(range(1, 9)) + (12, 16)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20, help="calls per side inside one timed run")
    ap.add_argument("--launch-reps", type=int, default=200, help="calls per side inside one timed run of a *_launches pair")
    ap.add_argument("--host-runs", type=int, default=2, help="timed passes of the host loop over all images")
    ap.add_argument("--images", type=int, default=IMAGES)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("rand_graph_ragged_bench: no GPU found (this tool measures the MI355X only)", file=sys.stderr)
        sys.exit(1)
    import build_graphs as bg
    from isic_hip import graph as IG
    from isic_hip.bags import BagOffsets
    from ragged_graph_bench import elliptic_flags
    dev = torch.device("cuda", 0)
    G = a.images
    rng = np.random.default_rng(7)
    sizes = np.asarray([max(1, int(elliptic_flags(rng).sum())) for _ in range(G)], dtype=np.int64)
    seeds = [42 + i for i in range(G)]
    offs = BagOffsets.from_lengths(sizes, dev)
    distinct = [int(n) for n in np.unique(sizes)]
    groups = [(n, np.flatnonzero(sizes == n)) for n in distinct]
    group_seeds = [(n, [seeds[i] for i in idx]) for n, idx in groups]
    res = {"tool": "rand_graph_ragged_bench", "device": torch.cuda.get_device_name(0), "runs": a.runs,
           "calls_per_side_and_run": a.reps, "calls_per_side_and_run_of_the_launches_pairs": a.launch_reps, "images": G, "r_values": list(R_VALUES), "unit": "ms of wall time per call",
           "lesion_nodes_min_mean_max": [int(sizes.min()), float(sizes.mean()), int(sizes.max())],
           "lesion_distinct_sizes": len(distinct), "lesion_graphs_above_pack_nodes": int((sizes > IG.RANDOM_RAGGED_PACK_NODES).sum()),
           "pack_nodes": IG.RANDOM_RAGGED_PACK_NODES, "graphs_per_workgroup_when_packed": IG.RANDOM_RAGGED_GRAPHS_PER_WORKGROUP}

    def host(images):
        return [{r: bg._random_edge_index(int(sizes[i]), r=r, seed=seeds[i]) for r in R_VALUES} for i in images]

    def grouped():
        return [IG.random_graphs(sd, n, R_VALUES, device=dev) for n, sd in group_seeds]

    def ragged():
        return IG.random_graphs_ragged(seeds, offs, R_VALUES)

    # ---- the three routes give the same lists
    got, per_size = ragged(), grouped()
    torch.cuda.synchronize()
    edges_total = 0
    for r in R_VALUES:
        ei, eo = got[r]
        edges_total += int(eo[-1])
        for (n, idx), out in zip(groups, per_size):
            for at, g in enumerate(idx):
                if not torch.equal(out[r][at], ei[:, int(eo[g]):int(eo[g + 1])]):
                    raise SystemExit(f"rand_graph_ragged_bench: grouped and ragged differ (n = {n}, r = {r}, image {g})")
    sample = list(range(0, G, 16))
    for i, per_r in zip(sample, host(sample)):
        for r in R_VALUES:
            ei, eo = got[r]
            if not torch.equal(per_r[r], ei[:, int(eo[i]):int(eo[i + 1])].cpu()):
                raise SystemExit(f"rand_graph_ragged_bench: the host loop and ragged differ (image {i}, r = {r})")
    res["lesion_edges_total"] = edges_total
    del got, per_size

    def launches_pair(groups_sd, offsets):
        """(old, new): the bare launches of both routes over buffers that exist; groups_sd: [(n, seeds)] of the old route."""
        sd_all = torch.tensor(seeds, dtype=torch.int64).to(dev)
        old_bufs = []
        for n, sd in groups_sd:
            _, total = IG.random_graph_layout(len(sd), n, R_VALUES)
            old_bufs.append((torch.tensor(sd, dtype=torch.int64).to(dev), n, torch.empty(max(total, 1), device=dev, dtype=torch.int64),
                             torch.empty((len(R_VALUES), len(sd)), device=dev, dtype=torch.int32)))
        head, bad, edge_off = IG.random_ragged_count_launch(sd_all, offsets, R_VALUES)
        flat = torch.empty((2, int(head[:-1].sum().item())), device=dev, dtype=torch.int64)

        def old():
            for sd, n, edges, counts in old_bufs:
                if n >= 2:
                    IG.random_graph_launch(sd, n, R_VALUES, edges, counts)

        def new():
            _, bad2, eo = IG.random_ragged_count_launch(sd_all, offsets, R_VALUES)
            IG.random_ragged_write_launch(sd_all, offsets, R_VALUES, eo, flat, bad2)

        def count_only():
            IG.random_ragged_count_launch(sd_all, offsets, R_VALUES)

        return old, new, count_only

    # ---- lesion sizes
    old, new, _ = launches_pair(group_seeds, offs)
    res["lesion_launches"] = time_pair(old, new, a.runs, a.launch_reps)
    res["lesion_launches"]["sides"] = {"old": f"{len(distinct)} bare isic_random_graph_i64 launches",
                                       "new": "bare count launch + prefix sums + bare write launch"}
    lesion = time_pair(grouped, ragged, a.runs, a.reps)
    lesion["sides"] = {"old": f"random_graphs once per distinct node count ({len(distinct)} calls)", "new": "random_graphs_ragged"}
    host(range(min(64, G)))
    ts = []
    for _ in range(a.host_runs):
        t0 = time.perf_counter()
        host(range(G))
        ts.append((time.perf_counter() - t0) * 1e3)
    lesion["host"] = summary(ts)
    lesion["host"]["images_per_second"] = G / (lesion["host"]["median_ms"] * 1e-3)
    lesion["ragged_vs_host"] = compare(lesion["host"], lesion["new"])
    res["lesion"] = lesion

    # ---- equal sizes
    for n in (NODES, 64, 32):
        eq = BagOffsets.uniform(G, n, dev)
        old = lambda: IG.random_graphs(seeds, n, R_VALUES, device=dev)          # noqa: E731
        new = lambda: IG.random_graphs_ragged(seeds, eq, R_VALUES)              # noqa: E731
        want, have = old(), new()
        for r in R_VALUES:
            if not torch.equal(torch.cat([want[r][g] for g in range(G)], dim=1), have[r][0]):
                raise SystemExit(f"rand_graph_ragged_bench: random_graphs and random_graphs_ragged differ (n = {n}, r = {r})")
        del want, have
        res[f"equal_{n}"] = time_pair(old, new, a.runs, a.reps)
        res[f"equal_{n}"]["sides"] = {"old": "random_graphs", "new": "random_graphs_ragged"}
        old, new, count_only = launches_pair([(n, seeds)], eq)
        res[f"equal_{n}_launches"] = time_pair(old, new, a.runs, a.launch_reps)
        res[f"equal_{n}_launches"]["sides"] = {"old": "one bare isic_random_graph_i64 launch",
                                               "new": "bare count launch + prefix sums + bare write launch"}
        res[f"equal_{n}_one_pass"] = time_pair(old, count_only, a.runs, a.launch_reps)
        res[f"equal_{n}_one_pass"]["sides"] = {"old": "one bare isic_random_graph_i64 launch (generates and writes)",
                                               "new": "bare count launch + prefix sums (generates and counts)"}
        del old, new, count_only

    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
