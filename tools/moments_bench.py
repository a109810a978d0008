"""Times the token-statistics entry (``isic_token_moments_f32``) against the torch composition of the same six statistics
on the same device (``tests/moments_ref.py: torch_composition``: what a caller runs without the entry), on the MI355X only
(no GPU -> exit 1).

One line per latent shape [B, T, D] in {[64, 196, 768], [256, 196, 384], [64, 196, 256]} -- a validation batch of the
ConvMAE-Base, ViT-S/16 and ResNet-18 token grids:
  entry    one launch; its share of the HBM peak (8 TB/s) is taken over the ALGORITHMIC bytes B T D 4 + B 6 D 4 (the latent
           read once, the descriptor written once).
  torch    mean, amax, std, median (a sort per column), two power sums, clamp, divisions, cat.
The two alternate in one process after warm-up calls of each; a repetition is ``--inner`` back-to-back calls between two
device events, device-synchronised; median and min-max of the per-call times over the repetitions.  The outputs are compared
before anything is timed (max and median equal, the rest to 1e-4 of the descriptor's scale).

    python tools/moments_bench.py [--reps 9] [--inner 20] [--out profiles/moments_bench.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-isic_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = ((64, 196, 768), (256, 196, 384), (64, 196, 256))
PEAK_HBM = 8.0e12


def timed(fn, inner):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def fmt(ts):
    return f"{1e3 * np.median(ts):8.1f} us (min {1e3 * np.min(ts):.1f} max {1e3 * np.max(ts):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("moments_bench: needs the MI355X")
        return 1
    from isic_hip.moments import token_moments
    from moments_ref import torch_composition
    dev = torch.device("cuda:0")
    lines = []
    for B, T, D in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(B + T + D)
        x = torch.empty((B, T, D), device=dev, dtype=torch.float32).normal_(generator=gen)
        x += torch.linspace(-3.0, 3.0, D, device=dev)              # token-like: unit noise on a per-channel offset

        def entry():
            return token_moments(x)

        def composed():
            return torch_composition(x)

        a, b = entry(), composed()
        torch.cuda.synchronize()
        same = bool(torch.equal(a[:, D:2 * D], b[:, D:2 * D]) and torch.equal(a[:, 3 * D:4 * D], b[:, 3 * D:4 * D]))
        worst = float((a - b).abs().max())
        if not same or not worst <= 1e-4 * float(b.abs().max()):
            print(f"moments_bench: outputs differ at {(B, T, D)}: selections equal {same}, max |diff| {worst:.3e}")
            return 1
        for _ in range(3):
            entry(), composed()
        te, tt = [], []
        for _ in range(args.reps):
            te.append(timed(entry, args.inner))
            tt.append(timed(composed, args.inner))
        nbytes = B * T * D * 4 + B * 6 * D * 4
        share = nbytes / (np.median(te) * 1e-3) / PEAK_HBM
        line = (f"[{B:3d}, {T}, {D:3d}] | entry {fmt(te)} = {100.0 * share:5.1f} % of the HBM peak over {nbytes / 1e6:.1f} MB | "
                f"torch composition {fmt(tt)} | torch / entry {np.median(tt) / np.median(te):.1f} x | max |diff| {worst:.1e}")
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/moments_bench.py on one MI355X: per-call medians of %d interleaved repetitions of %d calls\n"
                    % (args.reps, args.inner))
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
