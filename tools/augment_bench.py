"""The device augmentation launch (isic_augment_u8, isic_hip/augment.py) against the HBM roof, against the CPU transform it
replaces, and as a share of one MAE train step.

  1. kernel: ``--n`` outputs of 224 x 224 from a pool of 450 x 450 uint8 images, four variants interleaved in one process --
     identity box or RandomResizedCrop boxes, k even (0, 2) or k odd (1, 3), flips random in the random-box variants --
     timed with device events around ``--iters`` launches (parameters already on the device), the median of ``--rounds``
     rounds.  Algorithmic bytes: writes of n * 4 * S^2 * 4 (three image planes and the mask, fp32) plus reads of
     4 * ch * cw per output (three pixel bytes and one mask byte per source pixel of the crop); the fraction is of 6.3 TB/s.
     ``augment()`` itself (host validation, parameter upload, launch, synchronise) is timed with a host clock beside it.
  2. cpu: the ``transform`` closure of ``train_ae.py`` (restated here: it is local to ``main``) on the same 450 x 450
     sources with ``--threads`` torch threads (the host quota, not ``os.cpu_count()``), images per second.  Decoding is
     excluded on both sides: the default path also pays it every epoch, the pool once.
  3. step: the MAE train step of tools/convmae_mae_bench.py at ``--n`` images, alone and with the augment launch (random
     boxes, all k) in front of it producing its input, interleaved; medians and the spread of the rounds.
Developer tool:
    python tools/augment_bench.py [--n 256] [--out profiles/augment_bench.json] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from isic_hip import augment as ag  # noqa: E402
from isic_hip.lib import call  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12
S = 224


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_section(a, pool):
    g = torch.Generator().manual_seed(0)
    index = torch.randint(0, len(pool), (a.n,), generator=g)
    hw = pool.hw_host[index]
    ibox, _ = ag.identity_params(hw)
    rbox, rop = ag.sample_params(hw, g)
    flips = rop & 3
    k_even = (torch.randint(0, 2, (a.n,), generator=g) * 2).to(torch.int32)
    k_odd = k_even + 1
    zero = torch.zeros(a.n, dtype=torch.int32)
    variants = {"identity_k_even": (ibox, zero), "identity_k_odd": (ibox, zero + 4),
                "random_box_k_even": (rbox, flips | (k_even << 2)), "random_box_k_odd": (rbox, flips | (k_odd << 2))}
    images = torch.empty((a.n, 3, S, S), device=DEV)
    masks = torch.empty((a.n, 1, S, S), device=DEV)
    idx_d = index.to(DEV)
    launch = {}
    for name, (box, op) in variants.items():
        box_d, op_d = box.to(DEV), op.to(DEV)
        launch[name] = (lambda b=box_d, o=op_d: call("isic_augment_u8", pool.pixels, pool.masks, pool.offsets, pool.hw,
                                                     len(pool), idx_d, b, o, *ag.MEAN, *ag.STD, images, masks, a.n, S))
    for fn in launch.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in launch}
    for _ in range(a.rounds):
        for name, fn in launch.items():
            times[name].append(events(fn, a.iters))
    out = {}
    for name, (box, op) in variants.items():
        ms = statistics.median(times[name])
        nbytes = a.n * 4 * S * S * 4 + 4 * int((box[:, 2].long() * box[:, 3].long()).sum())
        out[name] = {"ms_median": ms, "ms_min": min(times[name]), "ms_max": max(times[name]), "algorithmic_bytes": nbytes,
                     "fraction_of_6.3_TB_s": nbytes / (ms * 1e-3) / HBM_BYTES_PER_S}
        print(f"kernel {name:18s}: {ms * 1e3:8.1f} us median ({min(times[name]) * 1e3:.1f} .. {max(times[name]) * 1e3:.1f}), "
              f"{nbytes / 1e6:.0f} MB algorithmic = {out[name]['fraction_of_6.3_TB_s']:.3f} of 6.3 TB/s")
    for kind in ("identity", "random_box"):
        out[f"{kind}_odd_over_even"] = out[f"{kind}_k_odd"]["ms_median"] / out[f"{kind}_k_even"]["ms_median"]
        print(f"kernel {kind}: k odd / k even = {out[kind + '_odd_over_even']:.2f}")
    # the whole wrapper: host validation, three small uploads, the launch, one synchronise
    box, op = variants["random_box_k_even"]
    walls = []
    for _ in range(a.rounds * a.iters + 1):
        t0 = time.perf_counter()
        ag.augment(pool, index, box, op)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    out["augment_call_wall_ms_median"] = statistics.median(walls[1:])
    print(f"augment() wall time, {a.n} outputs, synchronised: {out['augment_call_wall_ms_median']:.3f} ms median")
    return out, (idx_d, variants)


def cpu_section(a):
    torch.set_num_threads(a.threads)

    def transform(image, mask):
        img = torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1).float().unsqueeze(0) / 255.0
        img = torch.nn.functional.interpolate(img, size=(224, 224), mode="bilinear", align_corners=False)[0]
        img = (img - torch.tensor(ag.MEAN).view(3, 1, 1)) / torch.tensor(ag.STD).view(3, 1, 1)
        return {"image": img, "mask": torch.from_numpy(np.ascontiguousarray(mask)).float()}
    rng = np.random.RandomState(0)
    srcs = [(rng.randint(0, 256, size=(450, 450, 3)).astype(np.uint8), np.zeros((450, 450), np.uint8)) for _ in range(32)]
    for im, m in srcs[:8]:
        transform(im, m)
    rates = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        for i in range(a.cpu_images):
            transform(*srcs[i % len(srcs)])
        rates.append(a.cpu_images / (time.perf_counter() - t0))
    out = {"threads": a.threads, "images_per_s_median": statistics.median(rates), "images_per_s_min": min(rates),
           "images_per_s_max": max(rates)}
    print(f"cpu transform of train_ae.py, 450 x 450 -> 224 x 224, {a.threads} threads: {out['images_per_s_median']:.0f} "
          f"images/s median ({min(rates):.0f} .. {max(rates):.0f})")
    return out


def step_section(a, pool, idx_d, variants):
    from isic_hip import optim
    from isic_hip.convmae_mae import ConvMAEBase
    torch.manual_seed(0)
    m = ConvMAEBase(norm_pix_loss=True).to(DEV).train()
    enc = [p for k, p in m.named_parameters() if "decoder" not in k and p.requires_grad]
    dec = [p for k, p in m.named_parameters() if "decoder" in k and p.requires_grad]
    opts = [optim.AdamW(enc, lr=1e-5, betas=(0.9, 0.95), weight_decay=0.05),
            optim.AdamW(dec, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)]
    box, op = variants["random_box_k_even"]
    op = (op & 3) | (torch.arange(a.n, dtype=torch.int32) % 4 << 2)
    box_d, op_d = box.to(DEV), op.to(DEV)
    x = torch.empty((a.n, 3, S, S), device=DEV)

    def fill():
        call("isic_augment_u8", pool.pixels, None, pool.offsets, pool.hw, len(pool), idx_d, box_d, op_d, *ag.MEAN, *ag.STD, x,
             None, a.n, S)

    def step():
        for o in opts:
            o.zero_grad()
        loss, _, _ = m(x, mask_ratio=0.75)
        loss.backward()
        for o in opts:
            o.step()

    def both():
        fill()
        step()
    fill()
    step()
    both()
    torch.cuda.synchronize()
    t = {"step": [], "augment_then_step": [], "augment": []}
    for _ in range(a.rounds):
        t["step"].append(events(step, a.step_iters))
        t["augment_then_step"].append(events(both, a.step_iters))
        t["augment"].append(events(fill, a.iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {k + "_ms": {"median": med[k], "min": min(v), "max": max(v)} for k, v in t.items()}
    out["augment_share_of_step"] = med["augment"] / med["step"]
    out["step_difference_ms"] = med["augment_then_step"] - med["step"]
    print(f"MAE train step at {a.n} images: {med['step']:.2f} ms median ({min(t['step']):.2f} .. {max(t['step']):.2f}); with "
          f"the augment launch in front {med['augment_then_step']:.2f} ms ({min(t['augment_then_step']):.2f} .. "
          f"{max(t['augment_then_step']):.2f}); the launch alone {med['augment'] * 1e3:.1f} us = "
          f"{out['augment_share_of_step']:.5f} of the step")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--pool", type=int, default=1024, help="450 x 450 images in the pool")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-images", type=int, default=200)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench needs the GPU: nothing is measured without one")
    torch.manual_seed(0)
    px = 450 * 450
    pool = ag.ImagePool(torch.randint(0, 256, (a.pool * px * 3,), device=DEV, dtype=torch.uint8),
                        torch.randint(0, 2, (a.pool * px,), device=DEV, dtype=torch.uint8) * 255, [(450, 450)] * a.pool)
    res = {"outputs": a.n, "size": S, "source": [450, 450], "pool_images": a.pool, "iters": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    res["kernel"], (idx_d, variants) = kernel_section(a, pool)
    res["cpu_transform"] = cpu_section(a)
    res["speedup_over_cpu_transform"] = (a.n / (res["kernel"]["random_box_k_even"]["ms_median"] * 1e-3)
                                         / res["cpu_transform"]["images_per_s_median"])
    if not a.no_step:
        res["mae_step"] = step_section(a, pool, idx_d, variants)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
