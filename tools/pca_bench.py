"""Times the shifted-Gram entry of the device PCA (``isic_gram_shifted_f32``) against the only way the library had to the
same matrix before it, on the MI355X only (no GPU -> exit 1).

One line per (M, D) in {(200 704, 768), (2 007 040, 768), (2 007 040, 384)} -- 1 024 and 10 240 images of 196 tokens:
  gram     ``isic_gram_shifted_f32``: one pass over the resident latents, shift subtracted while staging, one triangle of
           128 x 128 tiles, fp64 finish.  Its share of the fp32 matrix peak (157.3 TFLOP/s) is taken over the ALGORITHMIC
           M D (D + 1) flops of a symmetric product, not over the flops of the tiles it computes.
  parent   ``x - mean`` into a copy, then ``isic_gemm_f32_ws(transA=1)`` of the copy with itself (both triangles, fp32
           throughout).
The two alternate in one process after a warm-up call of each; every repetition is device-synchronised and timed with
device events; median and min-max of the repetitions.  At the first shape sklearn's ``PCA(0.90).fit`` on the host is timed
once for the record (the path ``pca: true`` takes without ``device_pca``).

    python tools/pca_bench.py [--reps 7] [--out profiles/pca_bench.txt]
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

SHAPES = ((200704, 768), (2007040, 768), (2007040, 384))
PEAK_F32_MATRIX = 157.3e12


def timed(fn):
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
        print("pca_bench: needs the MI355X")
        return 1
    from isic_hip import ops
    from isic_hip.lib import call
    dev = torch.device("cuda:0")
    lines = []
    for M, D in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(M + D)
        x = torch.empty((M, D), device=dev, dtype=torch.float32)
        for a in range(0, M, 1 << 18):                           # token-like: unit noise on a per-channel offset
            x[a:a + (1 << 18)].normal_(generator=gen)
        x += torch.linspace(-3.0, 3.0, D, device=dev)
        shift = (ops.colsum(x[: 50176]) / 50176.0).contiguous()  # the first encoder batch's column mean
        G = torch.empty((D, D), device=dev, dtype=torch.float64)
        cs = torch.empty((D,), device=dev, dtype=torch.float64)
        nbytes = int(call("isic_gram_shifted_f32_workspace_bytes", M, D))
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        xc = torch.empty_like(x)
        C = torch.empty((D, D), device=dev, dtype=torch.float32)

        def gram():
            call("isic_gram_shifted_f32", x, M, D, D, None, shift, G, cs, 0.0, ws, nbytes)

        def parent():
            torch.sub(x, shift, out=xc)
            ops.gemm(xc, xc, trans_a=True, out=C)

        gram(), parent()
        torch.cuda.synchronize()
        worst = float((G - C.double()).abs().max() / G.diagonal().max())
        tg, tp = [], []
        for _ in range(args.reps):
            tg.append(timed(gram))
            tp.append(timed(parent))
        flops = float(M) * D * (D + 1)
        frac = flops / (np.median(tg) * 1e-3) / PEAK_F32_MATRIX
        line = (f"M {M:8d} D {D:4d} | gram {fmt(tg)} = {100.0 * frac:5.1f} % of the fp32 matrix peak over M D (D + 1) flops, "
                f"workspace {nbytes / 2**20:.0f} MiB | parent {fmt(tp)} | parent / gram {np.median(tp) / np.median(tg):.2f} x | "
                f"max |G - parent| / max diag {worst:.1e}")
        if (M, D) == SHAPES[0]:
            from sklearn.decomposition import PCA
            xh = x.cpu().numpy()
            t0 = time.perf_counter()
            PCA(n_components=0.90).fit(xh)
            line += f" | sklearn PCA(0.90).fit on the host {1e3 * (time.perf_counter() - t0):.0f} ms"
        print(line, flush=True)
        lines.append(line)
        del x, xc, ws
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/pca_bench.py on one MI355X: medians of %d interleaved repetitions\n" % args.reps)
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
