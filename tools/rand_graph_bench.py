"""Times the random patch graphs of `03_build_graphs.py:57-78` built on the host and on the device, on the MI355X only
(no GPU -> exit 1).

One line per G in {256, 2048} images of 196 nodes, the ten r values of ``build_graphs.DEFAULT_R_VALUES`` per image, seeds
42 + i as ``build_graph_records`` gives them:
  host     ``build_graphs._random_edge_index`` (torch's CPU generator: 196 ``randperm`` calls and one ``unique`` per graph),
           the ten r values of ``--host-sample`` images (default 32) with the host clock; reported per image and scaled to G.
  entry    the bare ``isic_random_graph_i64`` launch on buffers that exist, between device events: all G x 10 graphs.
  batched  ``build_graphs.random_edge_index_batched``: the allocation, the launch, the read-back of the edge counts and the
           per-graph views, with the host clock around it (it ends in a synchronising copy).
The device graphs of the first and last image are compared with the host's before anything is timed.  After a warm-up call
of each: median and min-max of the repetitions.  These are reported numbers: nothing in the tests asserts a ratio.

    python tools/rand_graph_bench.py [--reps 7] [--host-sample 32] [--out profiles/rand_graph_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-isic_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = (256, 2048)
N = 196


def event_timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def fmt(ts):
    return f"{np.median(ts):9.3f} ms (min {np.min(ts):.3f} max {np.max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-sample", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("rand_graph_bench: needs the MI355X")
        return 1
    import build_graphs as bg
    from isic_hip.graph import random_graph_launch, random_graph_layout
    dev = torch.device("cuda:0")
    rs = [int(r) for r in bg.DEFAULT_R_VALUES]
    lines = []
    for G in SIZES:
        seeds = [42 + i for i in range(G)]
        sd = torch.tensor(seeds, dtype=torch.int64).to(dev)
        _, total = random_graph_layout(G, N, rs)
        edges = torch.empty((total,), device=dev, dtype=torch.int64)
        counts = torch.empty((len(rs), G), device=dev, dtype=torch.int32)

        def entry():
            random_graph_launch(sd, N, rs, edges, counts)

        def batched():
            return bg.random_edge_index_batched(N, rs, seeds, device=dev)

        sample = min(G, args.host_sample)

        def host():
            return [{r: bg._random_edge_index(N, r=r, seed=seeds[i]) for r in rs} for i in range(sample)]

        entry()
        got, want = batched(), host()
        for i in (0, sample - 1):
            for r in rs:
                assert torch.equal(got[r][i].cpu(), want[i][r]), (G, i, r)
        n_edges = int(counts.sum())
        t = {"entry": [], "batched": [], "host": []}
        for _ in range(args.reps):
            t["entry"].append(event_timed(entry))
            t["batched"].append(host_timed(batched))
        for _ in range(max(1, min(3, args.reps))):
            t["host"].append(host_timed(host) / sample)
        med = {k: float(np.median(v)) for k, v in t.items()}
        line = (f"G {G:5d} x {len(rs)} r values, n {N} ({n_edges} edges, {16 * n_edges / 1e6:.0f} MB written) | host {fmt(t['host'])} "
                f"per image ({sample} images timed) = {med['host'] * G / 1e3:.1f} s per {G} | entry {fmt(t['entry'])} = "
                f"{G / med['entry'] / 1e3:.2f} M images/s, {16 * n_edges / (med['entry'] * 1e-3) / 1e9:.0f} GB/s of edges | batched "
                f"{fmt(t['batched'])} = {G / med['batched'] / 1e3:.3f} M images/s | host / batched {med['host'] * G / med['batched']:.0f} x")
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("python tools/rand_graph_bench.py --reps %d --host-sample %d   (one MI355X; medians; entry: device events; "
                    "batched and host: host clock, host = torch CPU ops on that machine's host)\n" % (args.reps, args.host_sample))
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
