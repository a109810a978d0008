"""ConvMAE-Base encoder training throughput (ConvMAEBaseEncoder(trainable=True), images of 224x224): images/s of forward +
backward, its ratio to the inference forward (the frozen default encoder) at the same N, interleaved over ``--repeats``
rounds in one process; the saved-activation bytes per image; per-class kernel times of one CBlock of each stage and one
blocks3 block; and the bytes/s of the three kernels of include/isic_hip_convmae_train.h over their compulsory bytes, as
a fraction of the 6.3 TB/s measured copy rate.  ``--step-only`` runs 1 + ``--iters`` training steps and nothing else (the
run to put under ``rocprofv3 --kernel-trace --stats``); ``--stats CSV --steps K`` reads that run's kernel statistics and
prints the measured time per step of the new kernels and their share of all kernel time.
Developer tool:
    python tools/convmae_train_bench.py [--n 256] [--iters 3] [--repeats 3]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/convmae_train_bench.py --step-only --iters 3
    python tools/convmae_train_bench.py --stats DIR/<host>/<pid>_kernel_stats.csv --steps 4"""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
import torch
from isic_hip.convmae import ConvMAEBaseEncoder
from isic_hip.lib import call

DEV, F16 = "cuda:0", torch.float16
PEAK_F16_TFLOPS = 2500.0
COPY_TBS = 6.3


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


def tape_bytes(tape):
    seen, total = set(), 0

    def walk(o):
        nonlocal total
        if isinstance(o, torch.Tensor):
            if o.data_ptr() not in seen:
                seen.add(o.data_ptr())
                total += o.numel() * o.element_size()
        elif isinstance(o, dict):
            for k, v in o.items():
                if k != "w":
                    walk(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
    walk(tape)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--stats", default=None)
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    if a.stats:
        return summarize(a.stats, a.steps)
    x = torch.randn(a.n, 3, 224, 224, device=DEV)
    frozen = ConvMAEBaseEncoder().to(DEV)
    enc = ConvMAEBaseEncoder(trainable=True).to(DEV)
    enc.load_state_dict(frozen.state_dict())
    enc.train()
    R = torch.randn(a.n, 768, device=DEV)
    if a.step_only:
        del frozen

        def only():
            enc.zero_grad(set_to_none=False)
            (enc(x) * R).sum().backward()
        print(f"{1 + a.iters} training steps at {a.n} images: {timeit(only, a.iters):.2f} ms per step (the last {a.iters})")
        return
    with torch.no_grad():
        _, tape = enc.run_forward_train(x)
    print(f"saved activations: {tape_bytes(tape) / a.n / 1e9:.3f} GB per image ({tape_bytes(tape) / 1e9:.1f} GB at {a.n} images)")
    del tape

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
    print(f"ConvMAE-Base inference forward, median: {mf:.2f} ms = {a.n / mf * 1e3:.0f} images/s")
    tf = enc.train_flops_per_image() * a.n / mt / 1e9
    print(f"ConvMAE-Base forward + backward, median: {mt:.2f} ms = {a.n / mt * 1e3:.0f} images/s, {tf:.0f} TFLOP/s "
          f"algorithmic ({tf / PEAK_F16_TFLOPS:.3f} of the dense fp16 peak)")
    print(f"training step / inference forward (medians): {mt / mf:.2f}x")
    del frozen, enc
    torch.cuda.empty_cache()
    new_ms = kernels(a)
    print(f"the three new kernels, ESTIMATED from the per-call times above x their calls per step (stand-in shapes for the "
          f"stage-2 decoder, the final norm and patch_embed3): {new_ms:.2f} ms = {new_ms / mt:.3f} of the step; the measured "
          f"share is the --stats summary of a --step-only rocprofv3 run")


NEW_KERNELS = ("dwconv5x5_wgrad_f16_kernel", "layernorm_add_bwd_f16_kernel", "patch_rows_bwd_kernel", "ct_slab_reduce_kernel")


def summarize(path, steps):
    """Per training step, from rocprofv3 kernel statistics of a --step-only run: every kernel's time, and the new kernels'
    (include/isic_hip_convmae_train.h, with their slab reducer) share of all kernel time."""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    new = {}
    for r in rows:
        for k in NEW_KERNELS:
            if k in r["Name"]:
                new[k] = new.get(k, 0.0) + float(r["TotalDurationNs"])
    print(f"measured over {steps} training steps (rocprofv3 kernel statistics): all kernels {total / steps / 1e6:.2f} ms per step")
    for k, v in new.items():
        print(f"  {k:32s} {v / steps / 1e6:7.2f} ms per step = {v / total:.3f} of kernel time")
    nt = sum(new.values())
    print(f"the three new kernels (with their slab reducer), measured: {nt / steps / 1e6:.2f} ms per step = {nt / total:.3f} "
          f"of kernel time")


def kernels(a):
    n, it = a.n, a.iters
    r = lambda *s: (torch.randn(*s, device=DEV) * 0.5).to(F16)       # noqa: E731
    nbytes = max(call("isic_gemm_f16_wgrad_workspace_bytes", n * 3136, 1024, 256),
                 call("isic_gemm_f16_wgrad_workspace_bytes", n * 196, 3072, 768),
                 call("isic_layernorm_add_bwd_f16_workspace_bytes", n * 3136, 256),
                 call("isic_dwconv5x5_wgrad_f16_workspace_bytes", n, 56, 56, 256),
                 call("isic_dwconv5x5_wgrad_f16_workspace_bytes", n, 28, 28, 384))
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    bw = {}

    def rep(totals, cls, name, t, flops=None, bytes_=None):
        totals[cls] = totals.get(cls, 0.0) + t
        extra = ""
        if flops:
            tf = flops / t / 1e9
            extra = f"  {tf:6.0f} TFLOP/s ({tf / PEAK_F16_TFLOPS:.2f} of dense fp16 peak)"
        if bytes_:
            tbs = bytes_ / t / 1e9
            extra = f"  {tbs:5.2f} TB/s = {tbs / COPY_TBS:.2f} of the copy rate"
            bw[name] = (t, tbs / COPY_TBS)
        print(f"  {cls:9s} {name:40s} {t:7.3f} ms{extra}")

    new_per_step = 0.0
    for g, C in ((56, 256), (28, 384)):
        M, Hd = n * g * g, 4 * C
        print(f"kernels of one CBlock's training step, {g}x{g}x{C} at {n} images (M = {M} rows):")
        totals = {}
        x, h, d, m, x2, g16, dD, dm = (r(M, C) for _ in range(8))
        hid, pre, dmid = r(M, Hd), r(M, Hd), r(M, Hd)
        gam, bet = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        W = {k: (torch.randn(o, i, device=DEV) * 0.05).to(F16) for k, o, i in (("c", C, C), ("fc1", Hd, C), ("fc2", C, Hd))}
        Wt = {k: w.t().contiguous() for k, w in W.items()}
        bias = {k: torch.zeros(w.shape[0], device=DEV) for k, w in W.items()}
        taps = torch.randn(25, C, device=DEV) * 0.1
        gf = torch.zeros(M, C, device=DEV)
        dg, dbt = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dw, db = torch.zeros(25, C, device=DEV), torch.zeros(C, device=DEV)

        def fwd():
            call("isic_layernorm_add_f16", x, None, None, gam, bet, h, None, M, C, 0, 1e-5)
            call("isic_gemm_f16", h, W["c"], bias["c"], None, d, M, C, C, 0, 0)
            call("isic_dwconv5x5_f16", d, taps, bias["c"], m, n, g, g, C)
            call("isic_gemm_f16", m, W["c"], bias["c"], x, x2, M, C, C, 0, 0)
            call("isic_layernorm_add_f16", x2, None, None, gam, bet, h, None, M, C, 0, 1e-5)
            call("isic_gemm_f16_gelu_pre", h, W["fc1"], bias["fc1"], hid, pre, M, Hd, C)
            call("isic_gemm_f16", hid, W["fc2"], bias["fc2"], x2, x, M, C, Hd, 0, 0)
        rep(totals, "forward", "one CBlock (training form)", timeit(fwd, it))
        rep(totals, "dgrad", f"fc2^T + dGELU {C}->{Hd}",
            timeit(lambda: call("isic_gemm_f16_dgelu", g16, Wt["fc2"], pre, dmid, M, Hd, C), it), 2.0 * M * Hd * C)
        rep(totals, "dgrad", f"fc1^T {Hd}->{C}",
            timeit(lambda: call("isic_gemm_f16", dmid, Wt["fc1"], None, None, dD, M, C, Hd, 0, 0), it), 2.0 * M * Hd * C)
        t = timeit(lambda: call("isic_gemm_f16", g16, Wt["c"], None, None, dD, M, C, C, 0, 0), it)
        rep(totals, "dgrad", f"conv2^T, conv1^T {C}->{C} (x2)", 2 * t, 4.0 * M * C * C)
        rep(totals, "dgrad", "depthwise 5x5, reversed taps",
            timeit(lambda: call("isic_dwconv5x5_f16", dm, taps, None, d, n, g, g, C), it))
        for name, dy, xin, N, K in ((f"fc2 {C}x{Hd}", g16, hid, C, Hd), (f"fc1 {Hd}x{C}", dmid, h, Hd, C),
                                    (f"conv2, conv1 {C}x{C} (x2)", g16, m, C, C)):
            dW, dbb = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
            t = timeit(lambda: call("isic_gemm_f16_wgrad", dy, xin, dW, dbb, M, N, K, 1.0, 1, ws, ws.numel()), it)
            k = 2 if "x2" in name else 1
            rep(totals, "wgrad", name, k * t, k * 2.0 * M * N * K)
        t = timeit(lambda: call("isic_dwconv5x5_wgrad_f16", d, dm, dw, db, n, g, g, C, 1.0, 1, ws, ws.numel()), it)
        rep(totals, "new", f"dwconv5x5 wgrad {g}x{g}x{C}", t, bytes_=2.0 * M * C * 2)
        new_per_step += 2 * t
        t = timeit(lambda: call("isic_layernorm_add_bwd_f16", dD, 0, 1.0, x, None, None, gam, bet, 0, 1e-5, gf, gf, g16, dg, dbt,
                                M, C, 1.0, 1, ws, ws.numel()), it)
        rep(totals, "new", f"LN-add bwd {C} (x2; dy fp16, g_in = g_out)", 2 * t, bytes_=2 * 14.0 * M * C)
        new_per_step += 5 * t                                          # 2 x 2 CBlock norms + the PatchEmbed norm
        print("  per class, one CBlock: " + ", ".join(f"{k} {v:.2f} ms" for k, v in totals.items()))
        del x, h, d, m, x2, g16, dD, dm, hid, pre, dmid, gf
        torch.cuda.empty_cache()
    # depth-to-space: the stage-1 decoder (P = 4, written) and patch_embed2 (P = 2, accumulated, with the fp16 copy)
    print(f"depth-to-space at {n} images:")
    totals = {}
    M1 = n * 3136
    gf, g16 = torch.zeros(M1, 256, device=DEV), torch.empty(M1, 256, device=DEV, dtype=F16)
    dr4, dr2 = r(n * 196, 16 * 256), r(n * 784, 4 * 256)
    t = timeit(lambda: call("isic_patch_rows_bwd_f16", dr4, gf, None, n, 56, 56, 256, 4, 0), it)
    rep(totals, "new", "patch rows bwd P=4 56x56x256 (write)", t, bytes_=6.0 * M1 * 256)
    new_per_step += 2 * t                                              # P = 4 and the stage-2 decoder's P = 2 write
    t = timeit(lambda: call("isic_patch_rows_bwd_f16", dr2, gf, g16, n, 56, 56, 256, 2, 1), it)
    rep(totals, "new", "patch rows bwd P=2 56x56x256 (accumulate)", t, bytes_=12.0 * M1 * 256)
    new_per_step += 2 * t
    del gf, g16, dr4, dr2
    torch.cuda.empty_cache()
    # one blocks3 block (the ViT-S backward at D = 768 with the LN-add backward)
    M, D, Hd = n * 196, 768, 3072
    print(f"kernels of one blocks3 block's training step at {n} images (M = {M} rows):")
    totals = {}
    x, h, att, g16, dD, x2 = (r(M, D) for _ in range(6))
    qkv, dqkv = r(M, 3 * D), torch.empty(M, 3 * D, device=DEV, dtype=F16)
    hid, pre, dmid = r(M, Hd), r(M, Hd), torch.empty(M, Hd, device=DEV, dtype=F16)
    gam, bet = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    W = {k: (torch.randn(o, i, device=DEV) * 0.02).to(F16) for k, o, i in (("qkv", 3 * D, D), ("proj", D, D), ("fc1", Hd, D),
                                                                           ("fc2", D, Hd))}
    Wt = {k: w.t().contiguous() for k, w in W.items()}
    bias = {k: torch.zeros(w.shape[0], device=DEV) for k, w in W.items()}

    def bfwd():
        call("isic_layernorm_add_f16", x, None, None, gam, bet, h, None, M, D, 0, 1e-6)
        call("isic_gemm_f16", h, W["qkv"], bias["qkv"], None, qkv, M, 3 * D, D, 0, 0)
        call("isic_attention_f16", qkv, att, n, 196, 12, 64)
        call("isic_gemm_f16", att, W["proj"], bias["proj"], x, x2, M, D, D, 0, 0)
        call("isic_layernorm_add_f16", x2, None, None, gam, bet, h, None, M, D, 0, 1e-6)
        call("isic_gemm_f16_gelu_pre", h, W["fc1"], bias["fc1"], hid, pre, M, Hd, D)
        call("isic_gemm_f16", hid, W["fc2"], bias["fc2"], x2, x, M, D, Hd, 0, 0)
    rep(totals, "forward", "one block (training form)", timeit(bfwd, it))
    for name, fn, fl in ((f"fc2^T + dGELU {D}->{Hd}", lambda: call("isic_gemm_f16_dgelu", g16, Wt["fc2"], pre, dmid, M, Hd, D), M * Hd * D),
                         (f"fc1^T {Hd}->{D}", lambda: call("isic_gemm_f16", dmid, Wt["fc1"], None, None, dD, M, D, Hd, 0, 0), M * Hd * D),
                         (f"proj^T {D}->{D}", lambda: call("isic_gemm_f16", g16, Wt["proj"], None, None, dD, M, D, D, 0, 0), M * D * D),
                         (f"qkv^T {3 * D}->{D}", lambda: call("isic_gemm_f16", qkv, Wt["qkv"], None, None, dD, M, D, 3 * D, 0, 0),
                          3 * M * D * D)):
        rep(totals, "dgrad", name, timeit(fn, it), 2.0 * fl)
    for name, dy, xin, N, K in ((f"fc2 {D}x{Hd}", g16, hid, D, Hd), (f"fc1 {Hd}x{D}", dmid, h, Hd, D), (f"proj {D}x{D}", g16, att, D, D),
                                (f"qkv {3 * D}x{D}", qkv, h, 3 * D, D)):
        dW, dbb = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
        rep(totals, "wgrad", name, timeit(lambda: call("isic_gemm_f16_wgrad", dy, xin, dW, dbb, M, N, K, 1.0, 1, ws, ws.numel()), it),
            2.0 * M * N * K)
    rep(totals, "attn bwd", "12 heads x 196 tokens",
        timeit(lambda: call("isic_attention_bwd_f16", qkv, att, g16, dqkv, n, 196, 12, 64), it))
    gf = torch.zeros(M, D, device=DEV)
    dg, dbt = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    t = timeit(lambda: call("isic_layernorm_add_bwd_f16", dD, 0, 1.0, x, None, None, gam, bet, 0, 1e-6, gf, gf, g16, dg, dbt, M, D,
                            1.0, 1, ws, ws.numel()), it)
    rep(totals, "new", f"LN-add bwd {D} (x2; dy fp16, g_in = g_out)", 2 * t, bytes_=2 * 14.0 * M * D)
    new_per_step += 24 * t                                             # 2 x 11 blocks, patch_embed3, the final norm
    print("  per class, one blocks3 block: " + ", ".join(f"{k} {v:.2f} ms" for k, v in totals.items()))
    print("new kernels, fraction of the 6.3 TB/s copy rate over compulsory bytes: "
          + ", ".join(f"{k}: {f:.2f}" for k, (t, f) in bw.items()))
    return new_per_step


if __name__ == "__main__":
    main()
