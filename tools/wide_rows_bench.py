"""Times the wide GraphMIL rows (include/isic_hip_wide.h) on the MI355X only (no GPU -> exit 1): the three entries at the top
of the reference's search space -- gat 512 x 8 = 4096 feature columns, eight pooling heads of 512 (tune_mil.py:170-200),
graphs of 196 nodes -- next to the narrow kernels on the same machine at GraphMIL's ordinary shapes (attn_pool_fwd2_kernel /
attn_pool_bwd_kernel<true> at 128 columns, four heads of 128; layernorm_bwd_vec_kernel at 256 columns), and one whole train
step (forward, backward, AdamW) of GraphMIL[gat 512 x 8, att_heads = 8, att_dim = 512] on k-NN graphs (k = 8).

Every entry line gives the time per call and the rate over the ALGORITHMIC bytes of the call (what the arithmetic needs
once): t + h + att + z for the pool forward, h + t + att + d_z + d_u + d_s + d_h for its backward, x + dy + dx for the
LayerNorm backward -- to be read against the HBM peak of 8 TB/s.  A repetition is ``--inner`` back-to-back calls between two
device events, device-synchronised, after warm-up calls; median and min-max over ``--reps`` repetitions.

    python tools/wide_rows_bench.py [--graphs 64] [--reps 9] [--inner 20] [--out profiles/wide_rows_bench.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-isic_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_HBM = 8.0e12
NODES = 196


def timed(fn, inner):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def measure(fn, reps, inner):
    for _ in range(3):
        fn()
    return [timed(fn, inner) for _ in range(reps)]


def line(name, ts, nbytes):
    med = float(np.median(ts))
    rate = nbytes / (med * 1e-3)
    return (f"{name:58s} {1e3 * med:9.1f} us (min {1e3 * np.min(ts):.1f} max {1e3 * np.max(ts):.1f})  "
            f"{nbytes / 1e6:8.1f} MB  {rate / 1e12:5.2f} TB/s  {100 * rate / PEAK_HBM:4.1f} % of the HBM peak")


def pool_lines(call, dev, G, H, A, heads, wide, reps, inner):
    T, At = G * NODES, heads * A
    gen = torch.Generator().manual_seed(1)
    h = torch.randn(T, H, generator=gen).to(dev)
    t = torch.tanh(torch.randn(T, At, generator=gen)).to(dev)
    w3 = (torch.randn(heads, A, generator=gen) / A ** 0.5).to(dev)
    b3 = torch.randn(heads, generator=gen).to(dev)
    offsets = (torch.arange(G + 1, dtype=torch.int64) * NODES).to(dev)
    att, z = torch.empty(T, heads, device=dev), torch.empty(G, H, device=dev)
    dz = torch.randn(G, H, generator=gen).to(dev)
    d_h, d_u, d_s = torch.empty(T, H, device=dev), torch.empty(T, At, device=dev), torch.empty(T, heads, device=dev)
    if wide:
        fwd = lambda: call("isic_attn_pool_wide_fwd", h, t, w3, b3, offsets, G, H, A, heads, NODES, att, z)      # noqa: E731
        bwd = lambda: call("isic_attn_pool_wide_bwd", h, t, att, w3, offsets, G, H, A, heads, NODES, dz, d_h, 0, d_u, d_s)  # noqa: E731
        names = ("isic_attn_pool_wide_fwd", "isic_attn_pool_wide_bwd")
    else:
        fwd = lambda: call("isic_attn_pool_fwd", h, t, w3, b3, None, None, offsets, G, H, A, heads, 0, NODES, att, z, None, None,  # noqa: E731
                           None, None)
        bwd = lambda: call("isic_attn_pool_bwd", h, t, att, None, w3, None, offsets, G, H, A, heads, 0, NODES, None, dz, d_h, 0,  # noqa: E731
                           d_u, d_s, None)
        names = ("isic_attn_pool_fwd (attn_pool_fwd2_kernel)", "isic_attn_pool_bwd (attn_pool_bwd_kernel<true>)")
    shape = f" [{G} x {NODES} rows, H {H}, {heads} x {A}]"
    fb = 4 * (T * (At + H + heads) + G * H)
    bb = 4 * (T * (2 * H + 2 * At + 2 * heads) + G * H)
    return [line(names[0] + shape, measure(fwd, reps, inner), fb), line(names[1] + shape, measure(bwd, reps, inner), bb)]


def ln_line(call, dev, M, N, wide, reps, inner):
    gen = torch.Generator().manual_seed(2)
    x, dy = torch.randn(M, N, generator=gen).to(dev), torch.randn(M, N, generator=gen).to(dev)
    gamma, beta = (1 + 0.1 * torch.randn(N, generator=gen)).to(dev), (0.1 * torch.randn(N, generator=gen)).to(dev)
    y, mean, rstd = torch.empty(M, N, device=dev), torch.empty(M, device=dev), torch.empty(M, device=dev)
    thr, scale = int(0.5 * 2 ** 32), 2.0                        # ReLU and dropout 0.5 on, as in a train step
    call("isic_layernorm_fwd_clk", x, gamma, beta, None, y, mean, rstd, M, N, 1e-5, 1, thr, scale, 7, 3, None)
    dx, dg, db = torch.empty(M, N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    sfx = "_wide" if wide else ""
    nbytes = int(call(f"isic_layernorm_bwd{sfx}_workspace_bytes", N))
    ws = torch.empty(nbytes + 16, device=dev, dtype=torch.uint8)
    fn = lambda: call(f"isic_layernorm_bwd{sfx}_ws", dy, x, gamma, beta, mean, rstd, dx, dg, db, M, N, 1, thr, scale, 7, 3, None,  # noqa: E731
                      ws, nbytes)
    name = "isic_layernorm_bwd_wide_ws" if wide else "isic_layernorm_bwd_ws (layernorm_bwd_vec_kernel)"
    return line(f"{name} [{M} x {N}, relu, p 0.5, workspace]", measure(fn, reps, inner), 4 * 3 * M * N)


def step_line(dev, G, reps):
    from gnn_models import GraphMIL
    from isic_hip import ops, optim, train as T
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import knn_indices
    D, k, C = 768, 8, 7
    gen = torch.Generator().manual_seed(3)
    y = torch.arange(G) % C
    x = (torch.randn(G, NODES, D, generator=gen) + 0.25 * y.view(-1, 1, 1).float()).to(dev)
    nn_idx = knn_indices(x.view(-1, D), BagOffsets.from_lengths([NODES] * G, dev), k).view(G, NODES, k)
    src = torch.arange(NODES, device=dev).view(1, NODES, 1).expand(G, NODES, k)
    ei = torch.stack([src.reshape(G, -1), nn_idx.reshape(G, -1)], dim=1)
    torch.manual_seed(4)
    m = GraphMIL(input_dim=D, gnn_type="gat", gnn_hidden=512, gnn_layers=2, gnn_dropout=0.5, gnn_heads=8, att_dim=512, att_heads=8,
                 pool_dropout=0.2, classifier_dim=128, classifier_light=True, num_classes=C).to(dev)
    m.train()
    m.set_dropout_state(seed=5, step=0)
    opt = optim.AdamW(m.parameters(), lr=1e-4, weight_decay=1e-4)
    store = T.GraphStore([{"x": x[i], "edge_index": ei[i], "y": int(y[i])} for i in range(G)], dev, True, mode=m.graph_mode)
    idx = torch.arange(G, device=dev)

    def step():
        xb, ob, gb = store.batch(idx)
        opt.zero_grad()
        probs, _ = m(xb, offsets=ob, graph=gb)
        loss = ops.cross_entropy_from_probs(probs, store.y_dev[idx])
        loss.backward()
        opt.step()
    ts = measure(step, reps, 3)
    med = float(np.median(ts))
    return (f"train step GraphMIL[gat 512 x 8, 2 layers, att_heads 8, att_dim 512], {G} graphs of {NODES} nodes, k = {k}: "
            f"{med:8.2f} ms (min {np.min(ts):.2f} max {np.max(ts):.2f})  {G / (med * 1e-3):8.0f} graphs/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("wide_rows_bench: needs the MI355X")
        return 1
    from isic_hip.lib import call
    dev = torch.device("cuda:0")
    G = args.graphs
    lines = [f"wide_rows_bench: {torch.cuda.get_device_name(0)}, {G} graphs of {NODES} nodes, reps {args.reps}, inner {args.inner}"]
    lines += pool_lines(call, dev, G, 4096, 512, 8, True, args.reps, args.inner)
    lines += pool_lines(call, dev, G, 1152, 128, 8, True, args.reps, args.inner)
    lines += pool_lines(call, dev, G, 128, 128, 4, False, args.reps, args.inner)
    lines.append(ln_line(call, dev, G * NODES, 4096, True, args.reps, args.inner))
    lines.append(ln_line(call, dev, G * NODES, 1152, True, args.reps, args.inner))
    lines.append(ln_line(call, dev, G * NODES, 256, False, args.reps, args.inner))
    lines.append(step_line(dev, min(G, 32), args.reps))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
