#!/usr/bin/env python3
"""Outputs of every entry whose kernels take their arithmetic from csrc/bn_bwd_math.inc, on fixed seeds, as files -- to
show that two builds of the library give the same bits (profiles/bn_bwd_math_equal.txt):

  tools/bn_bwd_bits.py dump DIR [--lib path/to/libisic_hip.so]     (on the GPU; one .npy per output array)
  tools/bn_bwd_bits.py compare DIR_A DIR_B                         (anywhere; lists every pair, exit status 1 on a difference)

Covered: the flat reduce and apply entries in every ReLU form and the pair (shapes of tests/test_bn_pair_gpu.py), the
64-channel weight gradient with the apply pass folded in (shapes of tests/test_wgrad_bnbwd_gpu.py), the stem chain max-pool
-> pooled reduce -> pooled apply -> fused stem weight gradient (shapes of tests/test_stem_wgrad_fused_gpu.py), and the
parameter gradients of one ResNet-18 encoder training step (4 images of 64 x 64)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-isic_amd")]

FLAT = [(1, 1, 1, 128), (3, 7, 7, 128), (2, 14, 14, 256), (3, 7, 7, 512), (5, 28, 28, 128)]
WGRAD = [(1, 4, 32), (2, 8, 32), (3, 9, 13), (2, 6, 40), (24, 56, 56)]
STEM = [(1, 14, 14), (1, 30, 46), (2, 31, 45), (5, 64, 64)]


def dump(out_dir, lib_path):
    import torch
    from isic_hip import lib
    if lib_path:
        lib.LIB_PATH = os.path.abspath(lib_path)
    call = lib.call
    dev, BF = "cuda:0", torch.bfloat16
    os.makedirs(out_dir, exist_ok=True)

    def save(name, t):
        t = t.detach().cpu()
        np.save(os.path.join(out_dir, name + ".npy"), (t.view(torch.int16) if t.dtype == BF else t).numpy())

    def params(C, gen):
        rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
        mean, rstd = 0.3 * rnd(C), 0.5 + torch.rand(C, device=dev, generator=gen)
        gamma, beta = 0.5 + torch.rand(C, device=dev, generator=gen), 0.2 * rnd(C)
        gamma[::5] *= -1.0
        return mean, rstd, gamma, gamma * rstd, beta - mean * gamma * rstd

    for N, H, W, C in FLAT:
        rows, tag = N * H * W, f"flat_{N}x{H}x{W}x{C}"
        gen = torch.Generator(device=dev).manual_seed(rows + C)
        g, x, x2, y = (torch.randn(rows, C, device=dev, generator=gen).to(BF) for _ in range(4))
        y = torch.relu(y)
        mask = torch.randint(0, 256, (rows * C // 8,), device=dev, dtype=torch.uint8, generator=gen)
        mean, rstd, gamma, scale, shift = params(C, gen)
        mean2, rstd2, gamma2, _, _ = params(C, gen)
        for form in ("none", "from_y", "from_x", "mask", "pair"):
            acc = torch.zeros(3, C, device=dev, dtype=torch.float64)
            dx, dres, dx2 = (torch.zeros(rows, C, device=dev, dtype=BF) for _ in range(3))
            f32 = [torch.ones(C, device=dev) for _ in range(4)]
            if form == "pair":
                call("isic_bn_bwd_reduce_pair_bf16", g, x, mask, mean, rstd, x2, mean2, rstd2, rows, C, acc[0], acc[1], acc[2])
                call("isic_bn_bwd_apply_pair_bf16", g, x, mask, mean, rstd, gamma, acc[0], acc[1], x2, mean2, rstd2, gamma2,
                     acc[2], rows, C, dx, dx2, *f32)
            elif form == "mask":
                call("isic_bn_bwd_reduce_mask_bf16", g, x, mask, mean, rstd, rows, C, acc[0], acc[1])
                call("isic_bn_bwd_apply_mask_bf16", g, x, mask, mean, rstd, gamma, acc[0], acc[1], rows, C, dx, dres, *f32[:2])
            else:
                relu, yy = int(form != "none"), y if form == "from_y" else None
                sc, sh = (scale, shift) if form == "from_x" else (None, None)
                call("isic_bn_bwd_reduce_bf16", g, x, yy, mean, rstd, rows, C, relu, sc, sh, acc[0], acc[1])
                call("isic_bn_bwd_apply_bf16", g, x, yy, mean, rstd, gamma, acc[0], acc[1], rows, C, relu, sc, sh, dx, dres,
                     *f32[:2])
            for k, t in (("sums", acc), ("dx", dx), ("dres", dres), ("dx2", dx2), ("f32", torch.stack(f32))):
                save(f"{tag}_{form}_{k}", t)

    for N, H, W in WGRAD:
        C, rows = 64, N * H * W
        gen = torch.Generator(device=dev).manual_seed(100 + rows)
        x, g, c = (torch.randn(N, H, W, C, device=dev, generator=gen).to(BF) for _ in range(3))
        mask = torch.randint(0, 256, (rows * C // 8,), device=dev, dtype=torch.uint8, generator=gen)
        mean, rstd, gamma, scale, shift = params(C, gen)
        ws = torch.empty(call("isic_conv2d_wgrad_workspace_bytes", N, C, H, W, C, 3, 3), device=dev, dtype=torch.uint8)
        for use_mask in (False, True):
            acc = torch.zeros(2, C, device=dev, dtype=torch.float64)
            if use_mask:
                call("isic_bn_bwd_reduce_mask_bf16", g, c, mask, mean, rstd, rows, C, acc[0], acc[1])
            else:
                call("isic_bn_bwd_reduce_bf16", g, c, None, mean, rstd, rows, C, 1, scale, shift, acc[0], acc[1])
            dc, dw = torch.zeros_like(c), torch.ones(C, 3, 3, C, device=dev)
            dg, db = torch.ones(C, device=dev), torch.ones(C, device=dev)
            call("isic_conv2d_wgrad_bnbwd_bf16", x, g, c, mask if use_mask else None, mean, rstd, gamma, acc[1], acc[0],
                 None if use_mask else scale, None if use_mask else shift, dc, dw, dg, db, N, H, W, ws, ws.numel())
            for k, t in (("dc", dc), ("dw", dw), ("f32", torch.stack([dg, db]))):
                save(f"wgrad_{N}x{H}x{W}_{'mask' if use_mask else 'from_x'}_{k}", t)

    for N, H, W in STEM:
        C = 64
        Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
        Hp, Wp = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
        gen = torch.Generator(device=dev).manual_seed(41 + N * H * W)
        x4 = torch.zeros(N, H, W, 4, device=dev)
        x4[..., :3] = torch.randn(N, H, W, 3, device=dev, generator=gen)
        x4 = x4.to(BF)
        y0 = torch.randn(N, Ho, Wo, C, device=dev, generator=gen).to(BF)
        gp = torch.randn(N, Hp, Wp, C, device=dev, generator=gen).to(BF)
        mean, rstd, gamma, scale, shift = params(C, gen)
        p, am = torch.empty(N, Hp, Wp, C, device=dev, dtype=BF), torch.empty(N, Hp, Wp, C, device=dev, dtype=torch.uint8)
        call("isic_bn_relu_maxpool3x3s2_fwd_bf16", y0, scale, shift, p, am, N, Ho, Wo, C, Hp, Wp)
        acc = torch.zeros(2, C, device=dev, dtype=torch.float64)
        call("isic_bn_bwd_reduce_pooled_bf16", am, gp, y0, mean, rstd, N, Ho, Wo, C, Hp, Wp, scale, shift, acc[0], acc[1])
        dy = torch.zeros_like(y0)
        f32 = [torch.ones(C, device=dev) for _ in range(4)]
        call("isic_bn_bwd_apply_pooled_bf16", am, gp, y0, mean, rstd, gamma, acc[0], acc[1], N, Ho, Wo, C, Hp, Wp, scale, shift,
             dy, *f32[:2])
        dw = torch.zeros(64, 3, 7, 7, device=dev).contiguous(memory_format=torch.channels_last)
        wsp = torch.empty(call("isic_conv_stem_wgrad_workspace_bytes"), device=dev, dtype=torch.uint8)
        call("isic_conv_stem_wgrad_bn_pooled_bf16", x4, y0, am, gp, mean, rstd, gamma, scale, shift, acc[0], acc[1], dw,
             *f32[2:], N, H, W, Ho, Wo, Hp, Wp, wsp, wsp.numel())
        for k, t in (("sums", acc), ("dy", dy), ("fused_dw", dw), ("f32", torch.stack(f32))):
            save(f"stem_{N}x{H}x{W}_{k}", t)

    from isic_hip.encoder import ResNet18Encoder
    torch.manual_seed(11)
    enc = ResNet18Encoder().to(dev)
    enc.train()
    gen = torch.Generator(device=dev).manual_seed(23)
    x = torch.randn(4, 3, 64, 64, device=dev, generator=gen).to(BF)
    dfeat = torch.randn(4, 512, device=dev, generator=gen) / 4
    _, tape = enc.run_forward(x, save=True)
    enc.run_backward(tape, dfeat)
    torch.cuda.synchronize()
    for k, prm in enc.named_parameters():
        save("encoder_step_grad_" + k, prm.grad)
    print(f"{len(os.listdir(out_dir))} arrays in {out_dir}")


def compare(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names, "the two directories hold different sets of arrays"
    bad = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        bad += not same
        print(f"{'equal ' if same else 'DIFFER'}  {n[:-4]}  {x.dtype}{list(x.shape)}  nonzero {int(np.count_nonzero(x))}")
    print(f"{len(names) - bad} of {len(names)} arrays bit-identical")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[4] if sys.argv[3:4] == ["--lib"] else None)
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
