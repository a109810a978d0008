"""Times gated attention pooling against the ungated pool on the same commit, on the MI355X only (no GPU -> exit 1).

Train steps (forward + backward + AdamW under ``fused_grad_accumulation``, captured into a hipGraph with the device step
clock and replayed), each with the gate off and on, alternating in one process after a warm-up of both:
  teacher H128/A64     AttentionMIL_teacher(768, 128, 64) on 668 bags of 196 x 768 fp32 latents (bench.py's teacher step)
  teacher H368/A772    ... at the reference's tuned widths
  graphmil gcn         GraphMIL[gcn], 3 layers, F 128, 4 pooling heads of width 128, 668 k-NN (k = 8) graphs of 196 nodes
                       (the BASELINE.json configs[3] shape)
The two entries of include/isic_hip_gated.h on their own at the three [T, heads * A] shapes: achieved bytes/s over the
algorithmic bytes (forward 20 nA, backward 16 nA + 4 heads per row, plus the slabs written and read once) as a fraction of
the 6.3 TB/s copy rate the other tools use.  The design predicts about 6 * nA * 4 bytes of extra traffic per row for the whole
gated step (the second half of the pre-activations written and read, t written, tv | sg read and d_p's second half written and
read); ``extra_ms_over_predicted`` sets the measured difference against that figure at 6.3 TB/s.
There is no pass mark: the numbers are a record.

    python tools/gated_pool_bench.py [--reps 5] [--steps 20] [--out profiles/gated_pool_bench.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/gated_pool_bench.py --trace on|off --steps 10     (per-kernel times of
                                                                   the tuned teacher step, run eagerly, in a run of its own)
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

HBM_BYTES_PER_S = 6.3e12
BAGS, PATCHES, FEAT, CLASSES = 668, 196, 768, 7


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


def teacher_step(H, A, gated, x, y, offs, capture=True):
    from isic_hip import graphs as G, ops, optim
    from utils_g_mil import AttentionMIL_teacher
    torch.manual_seed(42)
    m = AttentionMIL_teacher(FEAT, H, A, 0.5, CLASSES, gated=gated).cuda()
    m.train()
    m.set_dropout_state(seed=42, step=0)
    opt = optim.AdamW(m.parameters(), lr=2.2e-4, weight_decay=8.6e-4)
    clock = G.StepClock(x.device).attach(m, opt)

    def body():
        opt.zero_grad()
        with ops.fused_grad_accumulation():
            loss = ops.cross_entropy(m(x, offs)["bag_logits"], y)
            ops.backward(loss)
        opt.step()
        clock.advance()
        return loss
    return G.CapturedStep(body, optimizer=opt, clock=clock) if capture else body


def graphmil_step(gated, x, y, offs, graph, capture=True):
    from gnn_models import GraphMIL
    from isic_hip import graphs as G, ops, optim
    torch.manual_seed(42)
    m = GraphMIL(input_dim=FEAT, gnn_type="gcn", gnn_hidden=128, gnn_layers=3, gnn_dropout=0.5, gnn_heads=4, att_dim=128,
                 att_heads=4, pool_dropout=0.2, classifier_dim=128, classifier_light=True, num_classes=CLASSES,
                 att_gated=gated).cuda()
    m.train()
    m.set_dropout_state(seed=42, step=0)
    opt = optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    clock = G.StepClock(x.device).attach(m, opt)

    def body():
        opt.zero_grad()
        with ops.fused_grad_accumulation():
            _, _, loss = m(x, offsets=offs, graph=graph, labels=y)
            ops.backward(loss)
        opt.step()
        clock.advance()
        return loss
    return G.CapturedStep(body, optimizer=opt, clock=clock) if capture else body


def compare(off, on, reps, steps, T, nA):
    t_off, t_on = [], []
    for _ in range(reps):
        t_off.append(timed(lambda: [off.replay() for _ in range(steps)])[0] / steps)
        t_on.append(timed(lambda: [on.replay() for _ in range(steps)])[0] / steps)
    s_off, s_on = stats(t_off), stats(t_on)
    extra_ms = s_on["ms_median"] - s_off["ms_median"]
    predicted_ms = 6 * nA * 4 * T / HBM_BYTES_PER_S * 1e3
    return {"ungated": s_off, "gated": s_on, "gated_over_ungated": s_on["ms_median"] / s_off["ms_median"],
            "extra_ms": extra_ms, "predicted_extra_bytes": 6 * nA * 4 * T, "predicted_extra_ms_at_6.3_TB_s": predicted_ms,
            "extra_ms_over_predicted": extra_ms / predicted_ms, "loss_ungated": float(off.replay().detach()),
            "loss_gated": float(on.replay().detach())}


def entries(T, heads, A, reps):
    from isic_hip import lib
    nA = heads * A
    gen = torch.Generator().manual_seed(0)
    p0 = torch.randn(T, 2 * nA, generator=gen).cuda()
    d_s, w3 = torch.randn(T, heads, generator=gen).cuda(), torch.randn(heads, A, generator=gen).cuda()
    p, t, d_p = p0.clone(), torch.empty(T, nA, device="cuda"), torch.empty(T, 2 * nA, device="cuda")
    sums = torch.empty(3 * nA + heads, device="cuda")
    nws = lib.call("isic_gate_bwd_f32_workspace_bytes", T, heads, A)
    ws = torch.empty(nws, device="cuda", dtype=torch.uint8)
    fwd = lambda: lib.call("isic_gate_fwd_f32", p, T, heads, A, t)      # noqa: E731  (tv | sg fed back in: values stay in range)
    bwd = lambda: lib.call("isic_gate_bwd_f32", d_s, w3, p, T, heads, A, d_p, sums[:2 * nA], sums[2 * nA:3 * nA],      # noqa: E731
                           sums[3 * nA:], 0.0, ws, nws)
    fwd(), bwd()
    n = 10
    tf = [timed(lambda: [fwd() for _ in range(n)])[0] / n for _ in range(reps)]
    tb = [timed(lambda: [bwd() for _ in range(n)])[0] / n for _ in range(reps)]
    bf, bb = 20 * nA * T, (16 * nA + 4 * heads) * T + 2 * nws
    out = {"rows": T, "heads": heads, "A": A, "fwd": stats(tf), "bwd_with_reduce": stats(tb), "fwd_bytes": bf, "bwd_bytes": bb}
    out["fwd_bytes_per_s"] = bf / (out["fwd"]["ms_median"] * 1e-3)
    out["bwd_bytes_per_s"] = bb / (out["bwd_with_reduce"]["ms_median"] * 1e-3)
    out["fwd_fraction_of_6.3_TB_s"] = out["fwd_bytes_per_s"] / HBM_BYTES_PER_S
    out["bwd_fraction_of_6.3_TB_s"] = out["bwd_bytes_per_s"] / HBM_BYTES_PER_S
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", choices=("off", "on"), default=None,
                    help="instead of timing: run --steps eager steps of the tuned teacher (H368/A772) with the gate off / on and "
                         "exit, for a kernel trace of that step (rocprofv3 --kernel-trace --stats -- python tools/gated_pool_bench.py ...)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("gated_pool_bench: no GPU found (this tool measures the MI355X only)", file=sys.stderr)
        sys.exit(1)
    import build_graphs as bg
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import GraphBatch
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1234)
    T = BAGS * PATCHES
    y = torch.arange(BAGS, device=dev) % CLASSES
    x = (torch.randn(BAGS, PATCHES, FEAT, device=dev, generator=gen) + 0.25 * y.view(-1, 1, 1).float()).reshape(T, FEAT)
    offs = BagOffsets.uniform(BAGS, PATCHES, dev)
    if a.trace:
        body = teacher_step(368, 772, a.trace == "on", x, y, offs, capture=False)
        for _ in range(a.steps):
            body()
        torch.cuda.synchronize()
        return
    res = {"tool": "gated_pool_bench", "device": torch.cuda.get_device_name(0), "bags": BAGS, "rows_per_bag": PATCHES,
           "feat": FEAT, "reps": a.reps, "steps_per_rep": a.steps, "hbm_bytes_per_s": HBM_BYTES_PER_S, "steps": {}, "entries": {}}
    for H, A in ((128, 64), (368, 772)):
        off, on = teacher_step(H, A, False, x, y, offs), teacher_step(H, A, True, x, y, offs)
        res["steps"][f"teacher_H{H}_A{A}"] = compare(off, on, a.reps, a.steps, T, A)
        res["entries"][f"teacher_A{A}"] = entries(T, 1, A, a.reps)
        del off, on
    ei = bg.knn_edge_index_batched(x[:, :64].contiguous(), np.arange(BAGS + 1) * PATCHES, (8,))[8]
    graph = GraphBatch(ei, T, None, mode="gcn")
    off, on = graphmil_step(False, x, y, offs, graph), graphmil_step(True, x, y, offs, graph)
    res["steps"]["graphmil_gcn_F128_heads4_A128"] = compare(off, on, a.reps, a.steps, T, 4 * 128)
    res["entries"]["graphmil_heads4_A128"] = entries(T, 4, 128, a.reps)
    print(json.dumps(res, sort_keys=True))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
