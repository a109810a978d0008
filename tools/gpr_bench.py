"""Times the graph-resident K-hop kernel of GPR-GNN / APPNP (include/isic_hip_gpr.h) against the composed path (K calls of
``isic_spmm_csr_f32`` plus torch axpys) on the same commit, on the MI355X only (no GPU -> exit 1).

Geometry: the bench's graph step -- 668 k-NN (k = 8) graphs of 196 nodes, F = 128, three layers, K = 10.
  (a) the bare entries: ``isic_gpr_prop_f32`` and ``isic_gpr_prop_bwd_f32`` (dH and dgamma, with the slab reduction), each
      against its floor -- H (dZ and H) read once, Z (dH) written once, the CSR arrays read once -- at the 6.3 TB/s copy rate
      the other tools use;
  (b) the composed path for the same product: its forward without autograd, and forward + backward of both paths under
      autograd (``gpr_prop(resident=True | False)``);
  (c) the whole ``GraphMIL[gprgnn]`` train step (forward + backward + AdamW under ``fused_grad_accumulation``, captured into
      a hipGraph and replayed) with each path, and ``GraphMIL[gcn]`` from the same run for scale.
Everything that is compared is ALTERNATED in one process after a warm-up of all of it; medians and the run-to-run range
(min .. max) of each are reported.  The rule the default of ``gpr_prop`` follows (isic_hip.graph.GPR_RESIDENT_DEFAULT): the
resident kernel is the default only if its advantage on the WHOLE step exceeds three times the wider of the two ranges;
``verdict`` applies it to this run's numbers.

    python tools/gpr_bench.py [--reps 7] [--steps 10] [--out profiles/gpr_bench.txt]
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
GRAPHS, NODES, FEAT, HIDDEN, LAYERS, HOPS, KNN, CLASSES = 668, 196, 768, 128, 3, 10, 8, 7


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


def entries(graph, offs, reps, n):
    from isic_hip import graph as G
    from isic_hip.lib import call
    N, F, K = offs.total, HIDDEN, HOPS
    gen = torch.Generator().manual_seed(0)
    h, dz = torch.randn(N, F, generator=gen).cuda(), torch.randn(N, F, generator=gen).cuda()
    gamma, bias = G.gpr_gamma(K, 0.1).cuda(), torch.zeros(F, device="cuda")
    z, dh, dg = torch.empty_like(h), torch.empty_like(h), torch.empty(K + 1, device="cuda")
    bad = torch.zeros(1, device="cuda", dtype=torch.int32)
    nnz = int(graph.col.numel())
    nws = int(call("isic_gpr_prop_bwd_workspace_bytes", offs.num_bags, K, F))
    ws = torch.empty(nws, device="cuda", dtype=torch.uint8)

    def fwd():
        call("isic_gpr_prop_f32", graph.rowptr, graph.col, graph.val, nnz, offs.device, offs.num_bags, offs.max_bag, N, h, gamma,
             K, F, bias, z, bad)

    def bwd():
        call("isic_gpr_prop_bwd_f32", graph.rowptr_t, graph.col_t, graph.val_t, nnz, offs.device, offs.num_bags, offs.max_bag, N,
             dz, h, gamma, K, F, dh, dg, 0.0, ws, nws, bad)

    def bwd_dh_only():
        call("isic_gpr_prop_bwd_f32", graph.rowptr_t, graph.col_t, graph.val_t, nnz, offs.device, offs.num_bags, offs.max_bag, N,
             dz, h, gamma, K, F, dh, None, 0.0, None, 0, bad)

    def composed_fwd():
        with torch.no_grad():
            G.gpr_prop_composed(h, gamma, graph, bias)

    def spmm_once():
        with torch.no_grad():
            G.spmm(h, graph)

    out = alternate({"resident_fwd": fwd, "resident_bwd": bwd, "resident_bwd_dh_only": bwd_dh_only, "composed_fwd": composed_fwd,
                     "one_spmm": spmm_once}, reps, n)
    assert int(bad.item()) == 0
    csr = (N + 1) * 4 + nnz * 8
    floors = {"resident_fwd": 2 * N * F * 4 + csr, "resident_bwd": 3 * N * F * 4 + csr + 2 * nws,
              "resident_bwd_dh_only": 2 * N * F * 4 + csr}
    for k, b in floors.items():
        out[k]["floor_bytes"] = b
        out[k]["floor_ms_at_6.3_TB_s"] = b / HBM_BYTES_PER_S * 1e3
        out[k]["time_over_floor"] = out[k]["ms_median"] / out[k]["floor_ms_at_6.3_TB_s"]
    # per-hop traffic of the composed forward: one [N, F] read and write for the SpMM, two reads and a write for the axpy
    out["composed_fwd"]["bytes"] = K * (5 * N * F * 4 + csr)

    # forward + backward under autograd, both paths
    def fb(resident):
        hh, gg = h.clone().requires_grad_(True), gamma.clone().requires_grad_(True)

        def run():
            hh.grad = gg.grad = None
            G.gpr_prop(hh, gg, graph, offs, bias=bias, resident=resident, check=False).backward(dz)
        return run
    out.update({"autograd_" + k: v for k, v in alternate({"resident_fwd_bwd": fb(True), "composed_fwd_bwd": fb(False)}, reps, n).items()})
    return out


def step(gtype, resident, x, y, offs, graph):
    from gnn_models import GraphMIL
    from isic_hip import graphs as GR, ops, optim
    torch.manual_seed(42)
    m = GraphMIL(input_dim=FEAT, gnn_type=gtype, gnn_hidden=HIDDEN, gnn_layers=LAYERS, gnn_dropout=0.5, att_dim=128, att_heads=4,
                 pool_dropout=0.2, classifier_dim=128, classifier_light=True, num_classes=CLASSES, gpr_k=HOPS).cuda()
    m.gpr_resident = resident
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("gpr_bench: no GPU found (this tool measures the MI355X only)", file=sys.stderr)
        sys.exit(1)
    import build_graphs as bg
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import GraphBatch
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1234)
    T = GRAPHS * NODES
    y = torch.arange(GRAPHS, device=dev) % CLASSES
    x = (torch.randn(GRAPHS, NODES, FEAT, device=dev, generator=gen) + 0.25 * y.view(-1, 1, 1).float()).reshape(T, FEAT)
    offs = BagOffsets.uniform(GRAPHS, NODES, dev)
    ei = bg.knn_edge_index_batched(x[:, :64].contiguous(), np.arange(GRAPHS + 1) * NODES, (KNN,))[KNN]
    graph = GraphBatch(ei, T, None, mode="gcn")
    res = {"tool": "gpr_bench", "device": torch.cuda.get_device_name(0), "graphs": GRAPHS, "nodes": NODES, "F": HIDDEN,
           "layers": LAYERS, "K": HOPS, "knn": KNN, "reps": a.reps, "calls_per_rep": a.steps, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "longest_row": int(torch.diff(graph.rowptr).max()), "longest_row_transposed": int(torch.diff(graph.rowptr_t).max())}
    res["entries"] = entries(graph, offs, a.reps, a.steps)
    steps = {"gprgnn_resident": step("gprgnn", True, x, y, offs, graph), "gprgnn_composed": step("gprgnn", False, x, y, offs, graph),
             "appnp_resident": step("appnp", True, x, y, offs, graph), "appnp_composed": step("appnp", False, x, y, offs, graph),
             "gcn": step("gcn", None, x, y, offs, graph)}
    res["train_step"] = alternate({k: s.replay for k, s in steps.items()}, a.reps, a.steps)
    res["loss"] = {k: float(s.replay().detach()) for k, s in steps.items()}
    res["verdict_entries_fwd_bwd"] = verdict(res["entries"]["autograd_resident_fwd_bwd"], res["entries"]["autograd_composed_fwd_bwd"])
    res["verdict_train_step_gprgnn"] = verdict(res["train_step"]["gprgnn_resident"], res["train_step"]["gprgnn_composed"])
    res["verdict_train_step_appnp"] = verdict(res["train_step"]["appnp_resident"], res["train_step"]["appnp_composed"])
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
