"""ViT-S/16 encoder training throughput (ViTSmallEncoder(trainable=True), images of 224x224): images/s of forward +
backward, its ratio to the inference forward (the frozen default encoder) at the same N, interleaved over ``--repeats``
rounds in one process, and the per-class kernel times of one block's backward, with the weight-gradient GEMM's TFLOP/s as a
fraction of the ~2.5 PF dense fp16 MFMA peak.
Developer tool:
    python tools/vit_train_bench.py [--n 1024] [--iters 3] [--repeats 3]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
import torch
from isic_hip.lib import call
from isic_hip.vit import ViTSmallEncoder

DEV, F16 = "cuda:0", torch.float16
PEAK_F16_TFLOPS = 2500.0


def timeit(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    x = torch.randn(a.n, 3, 224, 224, device=DEV)
    frozen = ViTSmallEncoder().to(DEV)
    enc = ViTSmallEncoder(trainable=True).to(DEV)
    enc.load_state_dict(frozen.state_dict())
    enc.train()
    R = torch.randn(a.n, 384, device=DEV)

    def step():
        enc.zero_grad(set_to_none=False)
        (enc(x) * R).sum().backward()

    def infer():
        with torch.no_grad():
            frozen(x)
    fwd, trn = [], []
    for r in range(a.repeats):
        fwd.append(timeit(infer, a.iters))
        trn.append(timeit(step, a.iters))
        print(f"round {r}: inference forward {fwd[-1]:.2f} ms, forward + backward {trn[-1]:.2f} ms "
              f"({trn[-1] / fwd[-1]:.2f}x)")
    mf, mt = statistics.median(fwd), statistics.median(trn)
    print(f"ViT-S/16 inference forward, median: {mf:.2f} ms = {a.n / mf * 1e3:.0f} images/s")
    print(f"ViT-S/16 forward + backward, median: {mt:.2f} ms = {a.n / mt * 1e3:.0f} images/s, "
          f"{enc.train_flops_per_image() * a.n / mt / 1e9:.0f} TFLOP/s algorithmic")
    print(f"training step / inference forward (medians): {mt / mf:.2f}x")
    del frozen
    torch.cuda.empty_cache()
    kernels(a)


def kernels(a):
    M, D, Hm = a.n * 196, 384, 1536
    print(f"kernels of one block's training step at {a.n} images (M = {M} rows):")
    r = lambda *s: (torch.randn(*s, device=DEV) * 0.5).to(F16)
    x, h, att, g16, dD = r(M, D), r(M, D), r(M, D), r(M, D), torch.empty(M, D, device=DEV, dtype=F16)
    qkv, dqkv = r(M, 3 * D), torch.empty(M, 3 * D, device=DEV, dtype=F16)
    hid, pre, dmid = r(M, Hm), r(M, Hm), torch.empty(M, Hm, device=DEV, dtype=F16)
    gam, bet = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    totals = {}

    def rep(cls, name, t, flops=None):
        totals[cls] = totals.get(cls, 0.0) + t
        extra = ""
        if flops:
            tf = flops / t / 1e9
            extra = f"  {tf:6.0f} TFLOP/s ({tf / PEAK_F16_TFLOPS:.2f} of dense fp16 peak)"
        print(f"  {cls:9s} {name:34s} {t:7.3f} ms{extra}")
    # forward: the training forward of one block (unfolded LayerNorms, fc1 with its pre-activation)
    W = {n: (torch.randn(o, i, device=DEV) * 0.02).to(F16) for n, o, i in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", Hm, D),
                                                                          ("fc2", D, Hm))}
    Wt = {n: w.t().contiguous() for n, w in W.items()}
    b = {n: torch.zeros(w.shape[0], device=DEV) for n, w in W.items()}
    x2, out = torch.empty_like(x), torch.empty_like(x)

    def block_fwd():
        call("isic_layernorm_f16", x, gam, bet, h, None, M, D, 1e-6)
        call("isic_gemm_f16", h, W["qkv"], b["qkv"], None, qkv, M, 3 * D, D, 0, 0)
        call("isic_attention_f16", qkv, att, a.n, 196, 6, 64)
        call("isic_gemm_f16", att, W["proj"], b["proj"], x, x2, M, D, D, 0, 0)
        call("isic_layernorm_f16", x2, gam, bet, h, None, M, D, 1e-6)
        call("isic_gemm_f16_gelu_pre", h, W["fc1"], b["fc1"], hid, pre, M, Hm, D)
        call("isic_gemm_f16", hid, W["fc2"], b["fc2"], x2, out, M, D, Hm, 0, 0)
    rep("forward", "one block (training form)", timeit(block_fwd, a.iters))
    # data gradients
    rep("dgrad", "fc2^T + dGELU 384->1536", timeit(lambda: call("isic_gemm_f16_dgelu", g16, Wt["fc2"], pre, dmid, M, Hm, D), a.iters),
        2.0 * M * Hm * D)
    rep("dgrad", "fc1^T 1536->384", timeit(lambda: call("isic_gemm_f16", dmid, Wt["fc1"], None, None, dD, M, D, Hm, 0, 0), a.iters),
        2.0 * M * Hm * D)
    rep("dgrad", "proj^T 384->384", timeit(lambda: call("isic_gemm_f16", g16, Wt["proj"], None, None, dD, M, D, D, 0, 0), a.iters),
        2.0 * M * D * D)
    rep("dgrad", "qkv^T 1152->384", timeit(lambda: call("isic_gemm_f16", qkv, Wt["qkv"], None, None, dD, M, D, 3 * D, 0, 0), a.iters),
        2.0 * M * 3 * D * D)
    # weight gradients (+ bias)
    ws = torch.empty(max(call("isic_gemm_f16_wgrad_workspace_bytes", M, n_, k_) for n_, k_ in ((3 * D, D), (D, Hm), (Hm, D), (D, D))),
                     device=DEV, dtype=torch.uint8)
    wt = 0.0
    wf = 0.0
    for name, dy, xin, N, K in (("fc2 384x1536", g16, hid, D, Hm), ("fc1 1536x384", dmid, h, Hm, D), ("proj 384x384", g16, att, D, D),
                                ("qkv 1152x384", qkv, h, 3 * D, D)):
        dW, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
        t = timeit(lambda: call("isic_gemm_f16_wgrad", dy, xin, dW, db, M, N, K, 1.0, 1, ws, ws.numel()), a.iters)
        rep("wgrad", name, t, 2.0 * M * N * K)
        wt, wf = wt + t, wf + 2.0 * M * N * K
    tf = wf / wt / 1e9
    print(f"  wgrad total: {tf:.0f} TFLOP/s = {tf / PEAK_F16_TFLOPS:.3f} of the dense fp16 peak")
    rep("attn bwd", "6 heads x 196 tokens", timeit(lambda: call("isic_attention_bwd_f16", qkv, att, g16, dqkv, a.n, 196, 6, 64), a.iters))
    lws = torch.empty(call("isic_layernorm_add_bwd_f16_workspace_bytes", M, D), device=DEV, dtype=torch.uint8)
    g = torch.zeros(M, D, device=DEV)
    dg, dbt = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    t = timeit(lambda: call("isic_layernorm_add_bwd_f16", dD, 0, 1.0, x, None, None, gam, bet, 0, 1e-6, g, g, g16, dg, dbt, M, D,
                            1.0, 1, lws, lws.numel()), a.iters)
    rep("LN bwd", "384 (x2 per block)", t)
    totals["LN bwd"] += t
    print("per class, one block: " + ", ".join(f"{k} {v:.2f} ms" for k, v in totals.items()))


if __name__ == "__main__":
    main()
