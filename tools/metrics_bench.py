"""Times the scoring of a validation set with the ``device_metrics`` switch off and on, on the MI355X only (no GPU -> exit 1).

One line per n in {256, 2048, 16384} validation samples, C = 7:
  entry     the metric set from resident scores [n, C], labels and per-sample losses.
            off: what the loops do today after their last chunk -- ``scores.cpu()``, ``loss.cpu()`` and
                 ``train.gnn_metrics`` (scikit-learn on the host).
            on:  ``metrics.class_counts`` (``isic_class_metrics_f32``, one read-back) and the floats of ``ClassMetrics``.
            kernels: the two launches of the entry alone, between device events (n^2 score comparisons).
  evaluate  ``train.evaluate_gnn`` of a GraphMIL[mlp] (16 nodes x 32 features per graph, width 32, chunk = 32) over a
            resident ``GraphStore`` of n graphs, switch off and on: the model's forward passes are in both, the switch
            removes two read-backs (two syncs) per chunk and the host metrics.
Off and on alternate in one process after a warm-up call of each; every call ends in a device synchronise (a read-back) and
is timed with the host clock around it; median and min-max of the repetitions.  These are reported numbers: nothing in the
tests asserts a ratio.

    python tools/metrics_bench.py [--reps 7] [--out profiles/metrics_bench.txt]
"""
import argparse
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-isic_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = (256, 2048, 16384)
C = 7


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def event_timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def fmt(ts):
    return f"{np.median(ts):9.3f} ms (min {np.min(ts):.3f} max {np.max(ts):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("metrics_bench: needs the MI355X")
        return 1
    warnings.simplefilter("ignore")
    from gnn_models import GraphMIL
    from isic_hip import train as T
    from isic_hip.lib import call
    from isic_hip.metrics import class_counts, class_counts_record
    dev = torch.device("cuda:0")
    lines = []
    for n in SIZES:
        rng = np.random.default_rng(n)
        y = rng.integers(0, C, size=n)
        logits = torch.from_numpy((2.0 * rng.standard_normal((n, C)) + 1.5 * np.eye(C)[y]).astype(np.float32)).to(dev)
        scores = torch.softmax(logits, dim=1).contiguous()
        yd = torch.from_numpy(y).to(dev)
        loss = -torch.log(scores[torch.arange(n, device=dev), yd] + 1e-9)
        out = torch.empty(C * C + C + 3, device=dev, dtype=torch.int64)
        ws = torch.empty(max(16, int(call("isic_class_metrics_f32_workspace_bytes", n, C))), device=dev, dtype=torch.uint8)
        res = {}

        def entry_off():
            s, l = scores.cpu().numpy(), loss.cpu()
            res["off"] = {"loss": float(l.mean()), **T.gnn_metrics(y, s, C)}

        def entry_on():
            res["on"] = class_counts(scores, yd, loss).as_dict()

        def kernels():
            class_counts_record(scores, yd, loss, out=out, workspace=ws)

        # the evaluation loop around it
        x = rng.standard_normal((n, 16, 32)).astype(np.float32)
        recs = [{"x": x[i], "edge_index": None, "y": int(y[i])} for i in range(n)]
        torch.manual_seed(0)
        model = GraphMIL(32, "mlp", 32, 2, 0.0, att_dim=16, att_heads=4, pool_dropout=0.0, classifier_dim=24,
                         classifier_light=True, num_classes=C).to(dev)
        store = T.GraphStore(recs, dev, False)

        def eval_off():
            res["eval_off"] = T.evaluate_gnn(model, store, C)

        def eval_on():
            res["eval_on"] = T.evaluate_gnn(model, store, C, device_metrics=True)

        for f in (entry_off, entry_on, kernels, eval_off, eval_on):
            f()
        torch.cuda.synchronize()
        for a, b in (("off", "on"), ("eval_off", "eval_on")):
            for k in ("accuracy", "bacc", "auc", "macro_f1"):
                assert abs(res[a][k] - res[b][k]) <= 1e-12, (n, a, k, res[a][k], res[b][k])
        t = {k: [] for k in ("entry_off", "entry_on", "kernels", "eval_off", "eval_on")}
        for _ in range(args.reps):
            t["entry_off"].append(host_timed(entry_off))
            t["entry_on"].append(host_timed(entry_on))
            t["kernels"].append(event_timed(kernels))
            t["eval_off"].append(host_timed(eval_off))
            t["eval_on"].append(host_timed(eval_on))
        med = {k: float(np.median(v)) for k, v in t.items()}
        line = (f"n {n:6d} C {C} | entry off {fmt(t['entry_off'])} | on {fmt(t['entry_on'])} | off / on "
                f"{med['entry_off'] / med['entry_on']:.2f} x | kernels {fmt(t['kernels'])} = "
                f"{n * n / (med['kernels'] * 1e-3) / 1e9:.1f} G comparisons/s | evaluate_gnn ({(n + 31) // 32} chunks) off "
                f"{fmt(t['eval_off'])} | on {fmt(t['eval_on'])} | off / on {med['eval_off'] / med['eval_on']:.2f} x")
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("python tools/metrics_bench.py --reps %d   (one MI355X; medians of interleaved repetitions, host clock around "
                    "calls that end in a device synchronise; kernels: device events)\n" % args.reps)
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
