"""ConvMAE-Base encoder throughput (ConvMAEBaseEncoder, images of 224x224) on the MI355X.

Reports, per batch size: images/s from the median of ``--repeats`` rounds in which the batch sizes are interleaved; the
time of each stage (blocks1, blocks2, blocks3 and the rest: patch embeddings, decodes, final norm) as differences of runs
with the stages cut off (``run_tokens(depth=...)``); the depthwise 5x5 convolution's GB/s over compulsory bytes (x read
once, y written once) against the 6.3 TB/s measured copy rate; and products' TFLOP/s as a fraction of the ~2.5 PF dense
fp16 MFMA peak.
``--precision mxfp8`` measures the opt-in MXFP8 path instead; ``--precision both`` runs the fp16 and the MXFP8 forward of
the same images alternately inside every round of one process and prints both medians, the range over the rounds and
their ratio, then the three MXFP8 kernels of the convolutional front against their algorithmic bytes.
Developer tool:
    python tools/convmae_bench.py [--sizes 256 1024 2048] [--iters 3] [--repeats 3] [--precision fp16|mxfp8|both]"""
import argparse
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


def stage_flops(enc):
    """products of each stage's blocks per image (the same counting as flops_per_image)"""
    (d1, d2, d3), (g1, g2, g3), r = enc.dims, enc.grids, enc.mlp_ratio
    T = g3 * g3
    return {"blocks1": enc.depths[0] * 2 * g1 * g1 * (2 * d1 * d1 + 25 * d1 + 2 * r * d1 * d1),
            "blocks2": enc.depths[1] * 2 * g2 * g2 * (2 * d2 * d2 + 25 * d2 + 2 * r * d2 * d2),
            "blocks3": enc.depths[2] * (2 * T * (4 * d3 * d3 + 2 * r * d3 * d3) + 4 * T * T * d3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024, 2048])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--precision", choices=("fp16", "mxfp8", "both"), default="fp16")
    a = ap.parse_args()
    paths = ("fp16", "mxfp8") if a.precision == "both" else (a.precision,)
    encs = {p: ConvMAEBaseEncoder(precision=p).to(DEV) for p in paths}
    enc = encs[paths[0]]
    g = torch.Generator(device=DEV).manual_seed(0)
    xs = {n: torch.randn(n, 3, 224, 224, device=DEV, generator=g) for n in a.sizes}
    cuts = {"stems": (0, 0, 0), "blocks1": (2, 0, 0), "blocks2": (2, 2, 0), "full": (2, 2, 11)}
    times = {(p, n, c): [] for p in paths for n in a.sizes for c in cuts}
    for r in range(a.repeats):
        for n in a.sizes:
            for c, d in cuts.items():
                for p in paths:                                   # the precisions alternate inside a round
                    times[(p, n, c)].append(timeit(lambda: encs[p].run_tokens(xs[n], depth=d), a.iters))
        print(f"round {r}: " + ", ".join(f"{p} {n} images {times[(p, n, 'full')][-1]:.1f} ms" for n in a.sizes for p in paths),
              flush=True)
    fl = enc.flops_per_image()
    sf = stage_flops(enc)
    print(f"ConvMAE-Base: {fl / 1e9:.1f} GFLOP per image; max_batch {enc.max_batch}")
    for n in a.sizes:
        med = {}
        for p in paths:
            m = med[p] = {c: statistics.median(times[(p, n, c)]) for c in cuts}
            full = times[(p, n, "full")]
            st = {"patch embeds / decodes / norm": m["stems"], "blocks1": m["blocks1"] - m["stems"],
                  "blocks2": m["blocks2"] - m["blocks1"], "blocks3": m["full"] - m["blocks2"]}
            tf = fl * n / m["full"] / 1e9
            print(f"{n:5d} images, {p}: {m['full']:.1f} ms (median of {a.repeats}, range {min(full):.1f} - {max(full):.1f}) = "
                  f"{n / m['full'] * 1e3:.0f} images/s, {tf:.0f} TFLOP/s = {tf / PEAK_F16_TFLOPS:.3f} of the dense fp16 peak")
            for k, v in st.items():
                extra = ""
                if k in sf:
                    t = sf[k] * n / v / 1e9
                    extra = f"  {t:6.0f} TFLOP/s ({t / PEAK_F16_TFLOPS:.3f} of peak)"
                print(f"    {k:30s} {v:8.2f} ms{extra}")
        if len(paths) == 2:
            f, q = med["fp16"], med["mxfp8"]
            stages = (("stems", None), ("blocks1", "stems"), ("blocks2", "blocks1"), ("full", "blocks2"))
            ratio = ", ".join(f"{c if c != 'full' else 'blocks3'} {(f[c] - (f[b] if b else 0)) / (q[c] - (q[b] if b else 0)):.2f}x"
                              for c, b in stages)
            print(f"{n:5d} images: mxfp8 / fp16 speed-up (medians) {f['full'] / q['full']:.3f}x; per stage: {ratio}")
    if a.precision in ("fp16", "both"):
        kernels(a)
    if a.precision in ("mxfp8", "both"):
        mxfp8_kernels(a)


def kernels(a):
    n = 256
    print(f"single launches at {n} images (one chunk):")
    for H, C in ((56, 256), (28, 384)):
        M = n * H * H
        x = (torch.randn(M, C, device=DEV) * 0.5).to(F16)
        y = torch.empty_like(x)
        w = torch.randn(25, C, device=DEV) * 0.2
        b = torch.zeros(C, device=DEV)
        t = timeit(lambda: call("isic_dwconv5x5_f16", x, w, b, y, n, H, H, C), a.iters * 4)
        gbs = 2 * M * C * 2 / t / 1e6
        print(f"  dwconv5x5 {H}x{H}x{C}: {t * 1e3:7.1f} us, {gbs:6.0f} GB/s = {gbs / 1e3 / COPY_TBS:.2f} of {COPY_TBS} TB/s")
    for name, M, N, K, act in (("blocks1 fc1 256->1024", n * 3136, 1024, 256, 1), ("blocks1 fc2 1024->256", n * 3136, 256, 1024, 0),
                               ("blocks3 qkv 768->2304", n * 196, 2304, 768, 0), ("blocks3 fc1 768->3072", n * 196, 3072, 768, 1),
                               ("blocks3 fc2 3072->768", n * 196, 768, 3072, 0), ("decode1 4096->768", n * 196, 768, 4096, 0)):
        A = (torch.randn(M, K, device=DEV) * 0.5).to(F16)
        W = (torch.randn(N, K, device=DEV) * 0.02).to(F16)
        C = torch.empty(M, N, device=DEV, dtype=F16)
        t = timeit(lambda: call("isic_gemm_f16", A, W, None, None, C, M, N, K, act, 0), a.iters * 2)
        tf = 2.0 * M * N * K / t / 1e9
        print(f"  gemm_f16 {name:24s} {t:7.3f} ms {tf:6.0f} TFLOP/s = {tf / PEAK_F16_TFLOPS:.3f} of peak")
        del A, C


def mxfp8_kernels(a):
    """the three MXFP8 kernels of the convolutional front at the encoder's shapes, against their algorithmic bytes (the
    fp16 input read once, one byte per element and one scale byte per 32 written) and the measured copy rate"""
    n, u8 = 256, torch.uint8
    print(f"mxfp8 single launches at {n} images (one chunk); bytes = fp16 in + 1 B / element + 1 B / 32 out:")

    def report(name, t, elems):
        gbs = elems * (2 + 1 + 1 / 32) / t / 1e6
        print(f"  {name:38s} {t * 1e3:7.1f} us, {gbs:6.0f} GB/s = {gbs / 1e3 / COPY_TBS:.2f} of {COPY_TBS} TB/s")
    for H, C in ((56, 256), (28, 384)):
        M = n * H * H
        x = (torch.randn(M, C, device=DEV) * 0.5).to(F16)
        q, s = torch.empty(M, C, device=DEV, dtype=u8), torch.empty(M, C // 32, device=DEV, dtype=u8)
        w, b = torch.randn(25, C, device=DEV) * 0.2, torch.zeros(C, device=DEV)
        gam, bet = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        t = timeit(lambda: call("isic_dwconv5x5_mxfp8_f16", x, w, b, q, s, n, H, H, C), a.iters * 4)
        report(f"dwconv5x5 -> mxfp8 {H}x{H}x{C}", t, M * C)
        t = timeit(lambda: call("isic_layernorm_act_mxfp8_f16", x, gam, bet, q, s, M, C, 0, 1e-5), a.iters * 4)
        report(f"layernorm -> mxfp8 {M} x {C}", t, M * C)
        for P in ((4, 2) if H == 56 else (2,)):
            t = timeit(lambda: call("isic_patch_rows_mxfp8_nhwc_f16", x, q, s, n, H, H, C, P), a.iters * 4)
            report(f"patch rows -> mxfp8 {H}x{H}x{C} P={P}", t, M * C)
        del x, q, s
    M, C = n * 196, 768
    x = (torch.randn(M, C, device=DEV) * 0.5).to(F16)
    q, s = torch.empty(M, C, device=DEV, dtype=u8), torch.empty(M, C // 32, device=DEV, dtype=u8)
    gam, bet = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    t = timeit(lambda: call("isic_layernorm_act_mxfp8_f16", x, gam, bet, q, s, M, C, 1, 1e-5), a.iters * 4)
    report(f"layernorm + GELU -> mxfp8 {M} x {C}", t, M * C)


if __name__ == "__main__":
    main()
