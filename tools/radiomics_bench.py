"""Times the radiomics entry (``isic_radiomics_u8``) on a resident pool of 450 x 450 images -- the reference's crop size --
against its byte floor, and the numpy restatement of the same features on the host (tests/radiomics_ref.py: what a caller
without the entry and without PyRadiomics runs), on the MI355X only (no GPU -> exit 1).

  entry    one launch over the whole pool, one workgroup per image.  Its floor is the pool's bytes, 4 per pixel (three colour
           bytes and the mask byte, each read once), at the device's MEASURED copy rate: a ``copy_`` between two buffers of the
           pool's size moves twice its bytes, and the rate is those bytes over its time.
  host     ``features_image`` of the restatement, fp64, per image (a few images: it takes a good part of a second each).
Pools of --images (default 256, one image per compute unit) and of 32 images (a launch that cannot fill the device).  The copy
rate is measured ONCE, on buffers of the whole pool's size (an HBM rate: a 32-image copy would sit in the last-level cache).  A
repetition is ``--inner`` back-to-back calls between two device events; median and min-max over the repetitions.  The counts
of two images are compared with the restatement's before anything is timed.

  phases   where the time of ONE image goes, by the inputs that switch a phase off (32 images of the same size each, one per
           compute unit, so every line is the latency of one workgroup):
             no ROI          all-zero masks: staging only, the workgroup leaves with its NaN row
             one level       a constant image, full ROI: staging + counting with EVERY pair on one diagonal cell (the worst
                             same-address contention of the LDS atomics) + features of one level (no Jacobi rotation)
             noise           uniform noise, full ROI: staging + counting spread over all cells + features of 26 levels
             lesion, full    the synthetic lesion images with every pixel in the ROI
             lesion          the synthetic lesion images under their elliptic masks (the pool of the lines above)

    python tools/radiomics_bench.py [--images 256] [--reps 7] [--inner 20] [--out profiles/radiomics_bench.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multimodal-isic_amd"), ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SIDE = 450


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
    return f"{1e3 * np.median(ts):9.1f} us (min {1e3 * np.min(ts):.1f} max {1e3 * np.max(ts):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("radiomics_bench: needs the MI355X")
        return 1
    import radiomics_ref as R
    from isic_hip.augment import ImagePool, SyntheticDermPixels
    from isic_hip.lib import call
    from isic_hip.radiomics import radiomic_features
    dev = torch.device("cuda:0")
    src = SyntheticDermPixels(n=2 * args.images, size=(SIDE, SIDE))
    items = []
    for i in range(len(src)):
        if i % 5 != 4 and len(items) < args.images:                # every fifth synthetic image has no mask
            it = src[i]
            items.append((it["image"].numpy(), it["mask"].numpy()))
    pool = ImagePool.from_arrays(items, dev)
    roi = float(np.mean([(m == 255).mean() for _, m in items]))

    _, c, _ = radiomic_features(pool, [0, len(pool) - 1], return_counts=True)
    for row, b in enumerate((0, len(pool) - 1)):
        if not np.array_equal(c[row].cpu().numpy(), R.count_image(*items[b])):
            print(f"radiomics_bench: the counts of image {b} differ from the restatement's")
            return 1
    t0 = time.perf_counter()
    for b in range(args.host_images):
        R.features_image(*items[b])
    host = (time.perf_counter() - t0) / args.host_images

    def time_entry(pl, B):
        out = torch.empty((B, 224), device=dev, dtype=torch.float64)
        n_empty = torch.zeros(1, device=dev, dtype=torch.int64)
        index_dev = torch.arange(B, device=dev)

        def entry():                                               # the bare entry: nothing allocated, nothing copied
            return call("isic_radiomics_u8", pl.pixels, pl.masks, pl.offsets, pl.hw, len(pl), index_dev, B, 10, 255,
                        out, None, n_empty)

        for _ in range(2):
            entry()
        return [timed(entry, args.inner) for _ in range(args.reps)]

    # the copy rate: buffers of the whole pool's size, far beyond the last-level cache
    nbytes_pool = 4 * len(pool) * SIDE * SIDE
    a, b = (torch.empty(nbytes_pool, dtype=torch.uint8, device=dev) for _ in range(2))
    for _ in range(2):
        b.copy_(a)
    tc = [timed(lambda: b.copy_(a), args.inner) for _ in range(args.reps)]
    rate = 2 * nbytes_pool / (np.median(tc) * 1e-3)
    del a, b

    lines = [f"pool: {len(pool)} images of {SIDE} x {SIDE}, {pool.nbytes / 1e6:.1f} MB, ROI {100 * roi:.0f} % of the pixels, bin width 10; "
             f"HBM copy rate {rate / 1e12:.2f} TB/s (a copy_ of {nbytes_pool / 1e6:.0f} MB, read + write)"]
    for B in sorted({min(32, len(pool)), len(pool)}):
        te = time_entry(pool, B)
        floor_ms = 4 * B * SIDE * SIDE / rate * 1e3
        line = (f"B = {B:4d} | entry {fmt(te)} = {1e3 * np.median(te) / B:7.1f} us per image | byte floor (4 B per pixel at the copy "
                f"rate) {1e3 * floor_ms:.1f} us: the floor is {100 * floor_ms / np.median(te):.2f} % of the entry's time | "
                f"numpy restatement {1e3 * host:.0f} ms per image = {1e3 * host * B / np.median(te):.0f} x the entry")
        print(line, flush=True)
        lines.append(line)

    # ---- phases: 32 images, one workgroup per compute unit
    P = min(32, len(pool))
    rng = np.random.default_rng(1)
    full, none = np.full((SIDE, SIDE), 255, np.uint8), np.zeros((SIDE, SIDE), np.uint8)
    variants = (("no ROI", [(items[i][0], none) for i in range(P)]),
                ("one level", [(np.full((SIDE, SIDE, 3), 100 + i, np.uint8), full) for i in range(P)]),
                ("noise", [(rng.integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8), full) for i in range(P)]),
                ("lesion, full", [(items[i][0], full) for i in range(P)]),
                ("lesion", items[:P]))
    for name, its in variants:
        t = time_entry(ImagePool.from_arrays(its, dev), P)
        line = f"phases, {P} images | {name:13s} {fmt(t)}"
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("tools/radiomics_bench.py on one MI355X: per-call medians of %d repetitions of %d calls\n" % (args.reps, args.inner))
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
