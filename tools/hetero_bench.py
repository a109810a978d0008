"""Times the native heterophily stage against the routes it replaces, on the MI355X only (no GPU -> exit 1):

* lambda_2 of 256 knn8 graphs (the pipeline sub-line's batch) and of 6 680 graphs (668 images x the ten k of 03), on
  ``isic_laplacian_lambda2_f64`` and on dense fp64 Laplacians + ``torch.linalg.eigvalsh``;
* ``heterophily_summary_device`` (+ its one copy to the host) against ``compute_edge_heterophily_batch`` +
  ``summarize_image`` for 256 images.

Device events after warm-up, the two paths alternated in one process; median of the repetitions.  Prints one JSON line.

    python tools/hetero_bench.py [--reps 5] [--out profiles/hetero_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-isic_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, D, C = 196, 128, 7
K_VALUES = tuple(range(1, 9)) + (12, 16)                  # build_graphs.DEFAULT_K_VALUES (03)


def teacher(G, seed):
    from pipeline import DeviceTeacherOutputs
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(G, N, D, generator=gen).cuda()
    pp = torch.softmax(torch.randn(G, N, C, generator=gen) * 2, dim=2).cuda()
    return DeviceTeacherOutputs(x, pp, torch.rand(G, N).cuda(), torch.zeros(G, dtype=torch.int64).cuda(),
                                [str(i) for i in range(G)])


def global_edges(eis):
    """list of [G_i, 2, E_i] local edge tensors -> src, dst (global ids), offsets over all sum(G_i) graphs."""
    srcs, dsts, counts, g0 = [], [], [], 0
    for ei in eis:
        G, _, E = ei.shape
        off = (torch.arange(G, device=ei.device) + g0).view(G, 1) * N
        srcs.append((ei[:, 0] + off).reshape(-1))
        dsts.append((ei[:, 1] + off).reshape(-1))
        counts += [E] * G
        g0 += G
    offs = torch.as_tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64).cuda()
    return torch.cat(srcs), torch.cat(dsts), offs, g0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def ab(fa, fb, reps):
    """Alternate the two paths after one warm-up call of each; -> (median ms a, median ms b, last outputs)."""
    fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        t, oa = timed(fa)
        ta.append(t)
        t, ob = timed(fb)
        tb.append(t)
    return float(np.median(ta)), float(np.median(tb)), oa, ob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("hetero_bench: no GPU found (this tool measures the MI355X only)", file=sys.stderr)
        sys.exit(1)
    import measure_heterophily as mh
    from isic_hip import spectral
    flops = 4.0 / 3.0 * N ** 3
    res = {"tool": "hetero_bench", "device": torch.cuda.get_device_name(0), "nodes": N, "reps": a.reps,
           "flops_per_graph": flops}

    # ---- lambda_2: 256 knn8 graphs, and 668 images x ten k
    t256 = teacher(256, 1)
    t668 = teacher(668, 2)
    cases = {"knn8_256": [t256.knn_edge_index(8)], "k10_6680": [t668.knn_edge_index(k) for k in K_VALUES]}
    for name, eis in cases.items():
        src, dst, offs, G = global_edges(eis)
        reps = a.reps if G <= 256 else max(2, a.reps // 2)
        tn, te, ln, le = ab(lambda: spectral.laplacian_lambda2(src, dst, offs, G, N),
                            lambda: mh._lambda2_eigvalsh(src, dst, G, N), reps)
        res[f"lambda2_{name}"] = {"graphs": G, "native_ms": tn, "eigvalsh_ms": te, "speedup": te / tn,
                                  "native_gflops": G * flops / (tn * 1e6), "max_abs_diff": float((ln - le).abs().max())}

    # ---- per-image summaries of 256 images: device route vs the numpy route
    ei = t256.knn_edge_index(8)
    metas = [{} for _ in range(256)]

    def device_route():
        return mh.summary_records(mh.heterophily_summary_device(t256.x, t256.patch_probs, t256.dominant_class, ei), metas)

    def numpy_route():
        xs, ps = list(t256.x.cpu().numpy()), list(t256.patch_probs.cpu().numpy())
        ds, es = list(t256.dominant_class.cpu().numpy()), list(ei.cpu().numpy())
        return [mh.summarize_image(em, {}) for em in mh.compute_edge_heterophily_batch(xs, ps, ds, es)]

    t0 = time.perf_counter()
    tdev, tnp, rd, rn = ab(device_route, numpy_route, a.reps)
    worst = max(abs(x[k] - y[k]) / (abs(y[k]) + 1e-6) for x, y in zip(rd, rn) for k in mh.SUMMARY_STATS)
    res["summary_256"] = {"device_ms": tdev, "numpy_route_ms": tnp, "speedup": tnp / tdev, "max_rel_diff": float(worst),
                          "wall_s": time.perf_counter() - t0}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
