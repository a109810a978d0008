"""Times the token statistics over the lesion patches (``isic_token_moments_masked_f32`` through
``isic_hip.moments.token_moments(latent, keep=flags)``) on the MI355X only (no GPU -> exit 1).

Latent [64, 196, 768] (a validation batch of the ConvMAE-Base token grid) with the elliptic lesion flags of
``save_latent.SyntheticDermImages`` (every fifth image has no mask).  Four legs alternate in one process after warm-up calls:
  masked   one launch for the batch.
  loop     what a caller runs without the entry: per image a boolean gather of its kept tokens and one dense launch
           (``token_moments(latent[b][flags[b]][None])``; images without a kept token are skipped).
  torch    per image the same gather and the torch composition of the six statistics (``tests/moments_ref.py``).
and, with every flag set, the price of the mask:
  masked (all kept) against dense (``token_moments(latent)``) on the same latent.
A repetition is ``--inner`` back-to-back calls between two device events, device-synchronised (the loop legs synchronise
inside as well: a boolean gather reads its row count back); median and min-max of the per-call times over the repetitions.
Before anything is timed the masked rows are compared bit for bit with the loop's.

    python tools/lesion_moments_bench.py [--reps 9] [--inner 10] [--out profiles/lesion_moments_bench.txt]
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

B, T, D = 64, 196, 768


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
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("lesion_moments_bench: needs the MI355X")
        return 1
    import save_latent as sl
    from isic_hip.moments import token_moments
    from moments_ref import torch_composition
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B + T + D)
    x = torch.empty((B, T, D), device=dev, dtype=torch.float32).normal_(generator=gen)
    x += torch.linspace(-3.0, 3.0, D, device=dev)                  # token-like: unit noise on a per-channel offset
    data = sl.SyntheticDermImages(n=B)
    masks = torch.stack([data[i]["mask"] for i in range(B)]).to(dev)
    flags = sl.mask_patch_flags(masks).reshape(B, T)
    every = torch.ones_like(flags)
    counts = flags.sum(dim=1).cpu().numpy()
    nan_row = torch.full((6 * D,), float("nan"), device=dev)

    def masked():
        return token_moments(x, keep=flags)

    def loop():
        rows = []
        for b in range(B):
            kept = x[b][flags[b]]
            rows.append(token_moments(kept[None])[0] if kept.shape[0] else nan_row)
        return torch.stack(rows)

    def composed():
        rows = []
        for b in range(B):
            kept = x[b][flags[b]]
            rows.append(torch_composition(kept[None])[0] if kept.shape[0] else nan_row)
        return torch.stack(rows)

    def masked_all():
        return token_moments(x, keep=every)

    def dense():
        return token_moments(x)

    a, b_, c = masked(), loop(), composed()
    torch.cuda.synchronize()
    if not torch.equal(a.view(torch.int32), b_.view(torch.int32)):
        print("lesion_moments_bench: the masked rows differ from the per-image loop's")
        return 1
    if not torch.equal(masked_all().view(torch.int32), dense().view(torch.int32)):
        print("lesion_moments_bench: with every flag set the masked rows differ from the dense entry's")
        return 1
    live = torch.from_numpy(counts > 0).to(dev)
    worst = float((a[live] - c[live]).abs().max())
    legs = (("masked", masked), ("loop", loop), ("torch", composed), ("masked_all", masked_all), ("dense", dense))
    for _ in range(3):
        for _, fn in legs:
            fn()
    times = {name: [] for name, _ in legs}
    for _ in range(args.reps):
        for name, fn in legs:
            times[name].append(timed(fn, args.inner))
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = [
        f"latent [{B}, {T}, {D}], elliptic flags: {int(counts.sum())} of {B * T} tokens kept, {int((counts == 0).sum())} images "
        f"without one, per image min {int(counts.min())} median {int(np.median(counts))} max {int(counts.max())}",
        f"masked entry, one launch         {fmt(times['masked'])}",
        f"per-image gather + dense launch  {fmt(times['loop'])} | loop / masked {med['loop'] / med['masked']:.1f} x",
        f"per-image gather + torch         {fmt(times['torch'])} | torch / masked {med['torch'] / med['masked']:.1f} x | "
        f"max |masked - torch| {worst:.1e}",
        f"every flag set: masked           {fmt(times['masked_all'])}",
        f"every flag set: dense entry      {fmt(times['dense'])} | masked / dense {med['masked_all'] / med['dense']:.2f} x",
    ]
    for line in lines:
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("tools/lesion_moments_bench.py on one MI355X: per-call medians of %d interleaved repetitions of %d calls\n"
                    % (args.reps, args.inner))
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
