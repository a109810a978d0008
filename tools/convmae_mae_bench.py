"""ConvMAE-Base masked-autoencoder train step throughput (isic_hip/convmae_mae.py): forward, backward and both AdamW
steps (encoder lr 1e-5, decoder lr 1e-3) at ``--n`` images, mask_ratio 0.75, norm_pix_loss True; images/s and algorithmic
TFLOP/s from device events, the median of ``--repeats`` rounds of ``--iters`` steps.  ``--step-only`` runs 1 + ``--iters``
steps and nothing else (the run to put under ``rocprofv3 --kernel-trace --stats``); ``--stats CSV --steps K`` reads that
run's kernel statistics and prints the time per step of the kernels of include/isic_hip_mae.h (and the head-width-32
attention) with their share of all kernel time.
Developer tool:
    python tools/convmae_mae_bench.py [--n 256] [--iters 3] [--repeats 3]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/convmae_mae_bench.py --step-only --iters 3
    python tools/convmae_mae_bench.py --stats DIR/<host>/<pid>_kernel_stats.csv --steps 4"""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
import torch  # noqa: E402
from isic_hip import optim  # noqa: E402
from isic_hip.convmae_mae import ConvMAEBase  # noqa: E402

DEV = "cuda:0"
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


NEW_KERNELS = ("dwconv5x5_f16_kernel<1>", "dwconv5x5_f16_kernel<2>", "attention_f16_kernel<32>",
               "attention_bwd_f16_kernel<32>", "gather_rows_kernel", "scatter_rows_kernel", "unshuffle_kernel",
               "unshuffle_bwd_kernel", "mae_loss_kernel", "mae_loss_reduce_kernel")


def summarize(path, steps):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"measured over {steps} train steps (rocprofv3 kernel statistics): all kernels {total / steps / 1e6:.2f} ms per step")
    nt = 0.0
    for k in NEW_KERNELS:
        v = sum(float(r["TotalDurationNs"]) for r in rows if k in r["Name"].replace(" ", ""))
        calls = sum(int(r["Calls"]) for r in rows if k in r["Name"].replace(" ", ""))
        nt += v
        print(f"  {k:30s} {v / steps / 1e6:7.3f} ms per step = {v / total:.3f} of kernel time ({calls // max(steps, 1)} calls)")
    print(f"new kernels together: {nt / steps / 1e6:.2f} ms per step = {nt / total:.3f} of kernel time")


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
    torch.manual_seed(0)
    x = torch.randn(a.n, 3, 224, 224, device=DEV)
    m = ConvMAEBase(norm_pix_loss=True).to(DEV).train()
    enc = [p for k, p in m.named_parameters() if "decoder" not in k and p.requires_grad]
    dec = [p for k, p in m.named_parameters() if "decoder" in k and p.requires_grad]
    opts = [optim.AdamW(enc, lr=1e-5, betas=(0.9, 0.95), weight_decay=0.05),
            optim.AdamW(dec, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)]

    def step():
        for o in opts:
            o.zero_grad()
        loss, _, _ = m(x, mask_ratio=0.75)
        loss.backward()
        for o in opts:
            o.step()
    if a.step_only:
        print(f"{1 + a.iters} MAE train steps at {a.n} images: {timeit(step, a.iters):.2f} ms per step (the last {a.iters})")
        return
    ts = []
    for r in range(a.repeats):
        ts.append(timeit(step, a.iters))
        print(f"round {r}: MAE train step {ts[-1]:.2f} ms")
    mt = statistics.median(ts)
    tf = m.train_flops_per_image(0.75) * a.n / mt / 1e9
    print(f"ConvMAE-Base MAE train step (mask_ratio 0.75, norm_pix_loss, 2 x AdamW), median: {mt:.2f} ms = "
          f"{a.n / mt * 1e3:.0f} images/s, {tf:.0f} TFLOP/s algorithmic ({tf / PEAK_F16_TFLOPS:.3f} of the dense fp16 peak)")
    print(f"peak memory allocated: {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")


if __name__ == "__main__":
    main()
