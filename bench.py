"""Headline benchmark of the attention-MIL + patch-graph GNN training path on the MI355X.

    python bench.py --gpus 1 --steps 8 --warmup 2                     # configs[1]: attention-MIL, ResNet-18 encoder
    python bench.py --config gnn --gpus 1 --steps 20 --warmup 5       # configs[3]: patch-graph GNN (05_train_gnns.py path)
    python bench.py --config vit --gpus 1 --steps 10 --warmup 2       # configs[4]: frozen ViT-S/16 fp16 patch encoder (forward)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N --steps K --warmup W                     # bare: starts its own N child processes
    python bench.py --gpus 1 --steps 8 --warmup 2 --full              # + sub-benchmarks, rooflines, CPU baselines

A plain run sets up, warms up, times EXACTLY --steps steps and prints ONE JSON line on rank 0: whole-job units/s (bags or
graphs) with inputs resident in HBM when the timed region starts, and ms_per_step.  --dump-outputs DIR writes what the
last timed step computed (outputs, loss, parameters and gradients after the step; a fixed seeded sample of the larger
arrays, 64 MB in all) as DIR/<name>.npy in float32; inputs are seeded, so two builds run with the same arguments can be
compared file by file.

--full adds everything else: short runs of configs[3], configs[4], the teacher step, the k-NN build and the whole chain
as "gnn", "vit", "teacher", "knn" and "pipeline" sub-objects of the default (mil) line (--no-sublines to skip), and on
every line
  "roofline":     the dominant kernel's algorithmic FLOP/s (mil: implicit-GEMM convolution forward + data gradient
                  vs the dense bf16 MFMA peak) or GB/s (gnn: the segmented-sum SpMM vs the HBM peak), from HIP events
                  around every launch of that C-ABI entry INSIDE the timed region, on the stream it is launched on;
  "kernel_time":  per-class kernel time per step from an instrumented pass AFTER the timed region (every C-ABI
                  launch bracketed by HIP events), so that host gaps and clock throttling can be told apart:
                  gpu_busy_ms_per_step vs ms_per_step vs host_enqueue_ms_per_step;
  "cpu_baseline": the CPU oracle's per-bag / per-graph training loop (the reference's loop shape,
                  01_train_mil_teacher.py:235-246 / 05_train_gnns.py:336-346) timed on the host cores, rank 0, N = 1,
                  at all threads and at one thread.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

MFMA_BF16_PEAK_TFLOPS = 2500.0   # dense bf16, /opt/skills/guides/MI355X_MICROARCH.md
MFMA_F32_PEAK_TFLOPS = 157.3     # fp32 matrix core (v_mfma_f32_16x16x4_f32), same guide
HBM_PEAK_GBS = 8000.0            # HBM3E spec, same guide (6.3 TB/s measured streaming)
WORKLOAD_MIL = ("ISIC-shaped attention-MIL: 256 bags x 64x224x224 patches + 128-d radiomics, "
                "ResNet-18 encoder, bf16 (BASELINE.json configs[1])")
WORKLOAD_VIT = ("Frozen ViT-S/16 fp16 patch encoder of the full pipeline (BASELINE.json configs[4]): 224x224 images -> 196 x 384 "
                "tokens; forward only, as the reference runs its encoder (save_latent.py:51-53)")
WORKLOAD_GNN = ("Patch-graph GNN (05_train_gnns.py path): k-NN (k=8) graphs of 196 nodes on 768-d patch embeddings, "
                "3-layer GCN F=128, 4-head attention pool (BASELINE.json configs[3])")


# ----------------------------------------------------------------------------------------------- instrumentation
def conv_flops(a):
    """Algorithmic FLOPs of one isic_conv2d_igemm_bf16 launch (2*M*Cout*K of the convolution it implements; for a
    data-gradient launch that is the forward convolution's count).  ``a`` = the call's arguments after the three
    tensors: (N, Hin, Win, Cin, Hout, Wout, Cout, Kh, Kw, up, down, pad, ...)."""
    N, Hin, Win, Cin, Hout, Wout, Cout, Kh, Kw, up, down, pad = a[:12]
    f = 2.0 * N * Hout * Wout * Cout * Kh * Kw * Cin
    return f if down == 1 else f / (down * down)      # stride-`down` dgrad: 1/down^2 of the taps hit a real dY pixel


# forward + data gradient of every non-stem convolution; the second entry is the data gradient with the ReLU mask and
# the BatchNorm-backward sums in its epilogue (same geometry arguments, same FLOP accounting)
CONV_ENTRIES = ("isic_conv2d_igemm_bf16", "isic_conv2d_dgrad_bnbwd_bf16", "isic_conv2d_igemm_maskadd_bf16",
                "isic_conv2d_dgrad_pair_bf16")


def conv_entry_flops(name, a):
    """Algorithmic FLOPs of one launch of a CONV_ENTRIES entry (``a`` = the recorded call arguments)."""
    if name == "isic_conv2d_dgrad_pair_bf16":           # (dy, w, dy2, w2, dx, N, Ho, Wo, Co, H, W, C): 3x3 / 2 + 1x1 / 2 data gradients
        N, Ho, Wo, Co, _H, _W, C = a[5:12]
        return 2.0 * N * Ho * Wo * Co * C * (9 + 1)       # = the two forward convolutions' counts
    return conv_flops(a[3:])

KERNEL_CLASSES = (
    ("conv_fwd_dgrad", ("isic_conv2d_igemm_bf16", "isic_conv2d_dgrad_bnbwd_bf16", "isic_conv2d_igemm_maskadd_bf16",
                        "isic_conv2d_dgrad_pair_bf16")),
    ("conv_wgrad", ("isic_conv2d_wgrad",)),
    ("stem_conv", ("isic_conv_stem",)),
    ("bn_pool", ("isic_bn_", "isic_maxpool", "isic_avgpool")),
    ("graph", ("isic_spmm", "isic_gat", "isic_gcn_csr", "isic_knn", "isic_l2normalize", "isic_edge", "isic_fa",
               "isic_transformer", "isic_hetero")),
    ("attn_pool", ("isic_attn_pool",)),
    ("gemm_f16", ("isic_gemm_f16",)),
    ("vit_attention", ("isic_attention_f16",)),
    ("vit_layernorm_patchify", ("isic_layernorm_f16", "isic_row_stats_f16", "isic_vit_patchify")),
    ("gemm_f32", ("isic_gemm_f32", "isic_colsum")),
)


def kernel_class(name):
    for cls, prefixes in KERNEL_CLASSES:
        if any(name.startswith(p) for p in prefixes):
            return cls
    return "other"            # layer norm, cross entropy, dropout, AdamW, weight prep, layout packs


class KernelTimer:
    """HIP-event timing of C-ABI launches on the stream they are launched on.  ``names``: the entries to time
    (None = every entry).  Events come from a pool, so a timed launch costs two ``record`` calls and no allocation."""

    def __init__(self):
        self.names = None
        self.records = []
        self.active = False
        self._pool = []

    def _event(self):
        return self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)

    _installed = None          # the ONE timer wrapped around lib.call in this process (sub-benchmarks reuse it)

    @classmethod
    def get(cls):
        if cls._installed is None:
            cls._installed = cls()
            cls._installed.install()
        return cls._installed

    def install(self):
        from isic_hip import lib
        orig = lib.call
        timer = self

        def timed_call(name, *args, stream=None):
            if timer.active and (timer.names is None or name in timer.names):
                e0, e1 = timer._event(), timer._event()
                e0.record()
                rc = orig(name, *args, stream=stream)
                e1.record()
                # scalars only (a tensor argument is recorded as True, a NULL pointer as None): keeping the tensors would
                # pin every activation of the timed region
                timer.records.append((name, tuple(True if isinstance(a, torch.Tensor) else a for a in args), e0, e1))
                return rc
            return orig(name, *args, stream=stream)

        lib.call = timed_call
        import isic_hip
        for modname in ("encoder", "ops", "graph", "optim", "hetero", "vit"):
            mod = getattr(isic_hip, modname, None)
            if mod is None:
                try:
                    mod = __import__(f"isic_hip.{modname}", fromlist=[modname])
                except ImportError:
                    continue
            if hasattr(mod, "call"):
                mod.call = timed_call

    def start(self, names):
        self.names = None if names is None else set(names)
        self.records = []
        self.active = True

    def stop(self):
        """-> list of (name, args, ms); call after a device synchronisation."""
        self.active = False
        out = []
        for name, args, e0, e1 in self.records:
            out.append((name, args, e0.elapsed_time(e1)))
            self._pool += [e0, e1]
        self.records = []
        return out


def kernel_source_hash(prefixes=None):
    """Identity of the kernels a profile was taken with: sha256 over csrc/*.hip and csrc/*.h (``prefixes``: only the
    files whose name starts with one of them, plus every header)."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "multimodal-isic_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith(".h") or (f.endswith(".hip") and (prefixes is None or f.startswith(tuple(prefixes)))):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


# Which kernel files decide the HBM traffic of each roofline entry: a PMC profile stays valid while THESE are unchanged
# (tests/test_host_cpu.py fails when a committed profile no longer matches, so a kernel commit cannot silently null it).
TRAFFIC_PROFILE = os.path.join(ROOT, "profiles", "r04_pmc_traffic.json")
TRAFFIC_SOURCES = {
    "mil": ("conv_igemm", "conv_halo", "conv_pgemm", "conv_c64"),      # kernels behind isic_conv2d_igemm_bf16
    "gnn": ("graph.",),                                                 # isic_spmm_csr_f32
    "vit": ("gemm_f16",),                                               # isic_gemm_f16
}


def pmc_traffic(section, **match):
    """HBM bytes per launch of a roofline entry from the rocprofv3 PMC passes of THIS command (counters need runs of
    their own: tools/collect_traffic.sh writes profiles/r04_pmc_traffic.json).  Each section is stamped with the hash
    of the kernel sources behind that entry and with the workload; anything that does not match the code being run is
    refused (-> None)."""
    try:
        d = json.load(open(TRAFFIC_PROFILE))[section]
    except Exception:
        return None
    if d.get("kernel_source_hash") != kernel_source_hash(TRAFFIC_SOURCES[section]):
        return None
    if any(d.get("workload", {}).get(k) != v for k, v in match.items()):
        return None
    return d.get("hbm_bytes_per_launch")


def split_by_class(records, steps):
    per = {}
    for name, _a, ms in records:
        c = kernel_class(name)
        per[c] = per.get(c, 0.0) + ms
    out = {k: v / steps for k, v in sorted(per.items(), key=lambda kv: -kv[1])}
    out["gpu_busy_ms_per_step"] = sum(per.values()) / steps
    out["launches_per_step"] = len(records) / steps
    return out


# ----------------------------------------------------------------------------------------------- configs[1]: MIL
def run_mil(args, world, rank, dev):
    from isic_hip import ddp, ops, optim
    from model import MultiModalMILNet

    B, K, S, R, C = args.bags_per_step, args.patches, args.image_size, args.radiomics_dim, 7
    torch.manual_seed(42)
    model = MultiModalMILNet(hidden_dim=128, att_dim=64, dropout=0.5, radiomics_dim=R, num_classes=C).to(dev)
    model.train()
    model.set_dropout_state(seed=42, step=0)
    opt = optim.AdamW(model.parameters(), lr=2.2e-4, weight_decay=8.6e-4)
    flat = opt.flat
    ddp.broadcast_parameters(flat.data)
    sync = ddp.GradSync(flat.grad, world_size=world)
    ddp.attach(model.encoder, flat, sync)
    model.encoder.fuse_bn_backward = bool(args.bn_fusion)
    model.encoder.wgrad_stream = bool(args.wgrad_stream)

    # synthetic ISIC-shaped data, resident in HBM (bf16 images as the dataset loader would hand them over)
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    n_sets = 2
    labels = [(torch.arange(B, device=dev) + s + rank) % C for s in range(n_sets)]
    images = [(torch.randn(B, K, 3, S, S, device=dev, generator=g)
               + 0.25 * labels[s].view(B, 1, 1, 1, 1).float()).to(torch.bfloat16) for s in range(n_sets)]
    radiom = [torch.randn(B, R, device=dev, generator=g) + 0.25 * labels[s].view(B, 1).float() for s in range(n_sets)]

    timer = KernelTimer.get() if args.full else None
    last = {}

    def step(i):
        s = i % n_sets
        opt.zero_grad()
        sync.reset()
        with ops.fused_grad_accumulation():          # head gradients are added into the flat buffer by the kernels
            out = model(images[s], radiom[s])
            loss = model.loss(out, labels[s])
            ops.backward(loss)
        sync.finish()
        opt.step(grad_scale=1.0 / world)
        last.update((k, v.detach()) for k, v in out.items())
        return loss

    # two untimed settle steps (allocator growth, kernel attribute setup) precede the W warm-up steps
    for i in range(2 + args.warmup):
        step(i)
    elapsed, host_s, loss = timed_region(step, args, world, dev, timer, list(CONV_ENTRIES), 2 + args.warmup)
    if args.dump_outputs and rank == 0:
        running = torch.cat([v.reshape(-1).float() for k, v in model.state_dict().items() if "running_" in k])
        dump_outputs(args.dump_outputs, dict(last, loss=loss, params=flat.data, grads=flat.grad, bn_running_stats=running))
    final_loss = float(loss.detach())
    if args.full:
        conv = timer.stop()
        split = instrumented_pass(step, timer, dev, world, start=2 + args.warmup + args.steps)
    ddp.average_buffers(model)           # BatchNorm running statistics are per rank during training

    if rank != 0:
        return None
    line = base_line("bags/sec (train step) @ 64x224x224 patches/bag", "bags/s", world * B * args.steps / elapsed,
                     world, args, elapsed, "bf16")
    line["config"] = {"workload": WORKLOAD_MIL, "bags_per_step_per_gpu": B, "global_bags_per_step": B * world,
                      "patches_per_bag": K, "patch": f"3x{S}x{S}", "radiomics_dim": R, "parallelism": f"dp{world}",
                      "host_enqueue_ms_per_step": host_s * 1e3 / args.steps, "final_loss": final_loss}
    if not args.full:
        return line
    conv_ms = sum(ms for _n, _a, ms in conv)
    conv_fl = sum(conv_entry_flops(n_, a) for n_, a, _ms in conv)
    n_launch = len(conv)
    achieved = conv_fl / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    line["roofline"] = {
        "bound": "mfma", "kernel": "C-ABI entries isic_conv2d_igemm_bf16 + isic_conv2d_igemm_maskadd_bf16 + "
                                   "isic_conv2d_dgrad_bnbwd_bf16 + isic_conv2d_dgrad_pair_bf16 (forward + data gradient of every "
                                   "non-stem convolution: conv_halo / conv3x3_c64p / conv_pgemm / conv_igemm kernels; 35 launches "
                                   "per step -- the 1x1 downsample data gradients ride inside the 3x3 stride-2 ones)",
        "achieved": achieved, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
        "frac": achieved / MFMA_BF16_PEAK_TFLOPS,
        "traffic": pmc_traffic("mil", bags_per_step=B, patches=K, image_size=S),
        "launches": n_launch, "avg_launch_ms": conv_ms / max(n_launch, 1),
        "algorithmic_gflop_per_launch": conv_fl / max(n_launch, 1) / 1e9,
        "share_of_step_time": conv_ms * 1e-3 / elapsed, "measured": "HIP events inside the timed region",
    }
    line["kernel_time"] = split
    if world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline_mil(model, K, S, R, C, args.cpu_budget_s)
    return line


def cpu_baseline_mil(model, K, S, R, C, budget_s):
    """oracle/ per-bag loop on the host cores (kind "port": the build's CPU restatement of the reference loop; the
    reference itself cannot travel to the GPU box): per-bag optimizer steps on FULL bags (K patches, ~692 GFLOP of fp32
    convolution each) with as many threads as the box's CPU quota allows (`host_threads`), and the one-thread figure on
    bags reduced to 2 patches, scaled by 2 / K (the convolutions are >99.9 % of the work and linear in the patch count)."""
    from oracle import model as omodel
    p = {k: v.detach().float().cpu().contiguous() for k, v in model.state_dict().items()
         if v.dtype.is_floating_point and "running_" not in k}
    default_threads, threads = torch.get_num_threads(), host_threads()

    def run(k_patches, n_steps, nthreads, budget):
        torch.set_num_threads(nthreads)
        g = torch.Generator().manual_seed(7)
        bags = [(torch.randn(k_patches, 3, S, S, generator=g) + 0.25 * (i % C), torch.randn(1, R, generator=g) + 0.25 * (i % C),
                 i % C) for i in range(n_steps + 1)]
        sps, done = omodel.time_per_bag_train_loop(p, lambda i: bags[i], n_bags=n_steps, warmup=1, budget_s=budget)
        torch.set_num_threads(default_threads)
        return sps * k_patches / K, done

    k_one = 2
    v_all, d_all = run(K, 24, threads, budget_s)
    v_one, d_one = run(k_one, 6, 1, budget_s / 2)
    return {"value": v_all, "unit": "bags/s", "cores": threads, "kind": "port",
            "sample": f"{d_all} per-bag train steps on full bags ({K} patches of 3x{S}x{S}, fp32, torch CPU, {threads} threads = "
                      f"the box's CPU quota) after 1 warm-up step",
            "one_thread": {"value": v_one, "cores": 1,
                           "sample": f"{d_one} steps on bags of {k_one} patches, scaled by {k_one}/{K}"},
            "host_cpus": os.cpu_count(), "torch_default_threads": default_threads}


# ----------------------------------------------------------------------------------------------- configs[4]: ViT encoder
def run_vit(args, world, rank, dev):
    """A "step" = the frozen encoder's forward over one batch of --images-per-step images (per GPU; ranks are independent
    replicas: inference has no exchange step)."""
    from isic_hip.vit import ViTSmallEncoder
    n_img, S = args.images_per_step, args.image_size
    torch.manual_seed(42)
    enc = ViTSmallEncoder(img_size=S).to(dev)
    gen = torch.Generator(device=dev).manual_seed(99 + rank)
    x = torch.randn(n_img, 3, S, S, device=dev, generator=gen)
    timer = KernelTimer.get() if args.full else None
    last = {}

    def step(i):
        last["tokens"] = enc.run_tokens(x)
        return last["tokens"].sum()

    for i in range(2 + args.warmup):
        step(i)
    elapsed, host_s, total = timed_region(step, args, world, dev, timer, ["isic_gemm_f16", "isic_gemm_f16_stats",
                                                                          "isic_gemm_f16_ln"], 2 + args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(last, tokens_sum=total))
    if args.full:
        gemm = timer.stop()
        split = instrumented_pass(step, timer, dev, world, start=0)
    if rank != 0:
        return None
    line = base_line("images/sec (ViT-S/16 fp16 patch-encoder forward) @ 224x224", "images/s",
                     world * n_img * args.steps / elapsed, world, args, elapsed, "f16")
    line["scaling"] = "weak"
    line["config"] = {"workload": WORKLOAD_VIT, "images_per_step_per_gpu": n_img, "image": f"3x{S}x{S}", "tokens": enc.tokens,
                      "dim": enc.dim, "depth": enc.depth, "heads": enc.heads, "parallelism": f"replicas{world}",
                      "host_enqueue_ms_per_step": host_s * 1e3 / args.steps,
                      "whole_forward_algorithmic_tflops": enc.flops_per_image() * n_img * args.steps / elapsed / 1e12}
    if not args.full:
        return line

    def mnk(name, a):
        """(M, N, K, residual rows read, fp32 statistics bytes) of one launch of the three product entries"""
        if name == "isic_gemm_f16":            # (A, W, bias, residual, C, M, N, K, act, residual_rows)
            M, N, K = a[5], a[6], a[7]
            return M, N, K, (0 if a[3] is None else (a[9] if a[9] > 0 else M)), 0.0
        if name == "isic_gemm_f16_stats":      # (A, W, bias, residual, C, row_stats, M, N, K, act, residual_rows): + [M][2N/128][2] fp32
            M, N, K = a[6], a[7], a[8]
            return M, N, K, (0 if a[3] is None else (a[10] if a[10] > 0 else M)), 4.0 * M * (2 * N // 128) * 2
        M, N, K = a[7], a[8], a[9]             # isic_gemm_f16_ln(X, Wg, bias_b, ln_c, ln_stats, ln_parts, C, M, N, K, act, eps)
        return M, N, K, 0, 4.0 * M * max(a[5], 1) * 2
    ms = sum(m for _n, _a, m in gemm)
    fl = sum(2.0 * mnk(n, a)[0] * mnk(n, a)[1] * mnk(n, a)[2] for n, a, _m in gemm)
    # algorithmic bytes of a launch: A[M,K] + W[N,K] + C[M,N] (+ the residual: [M,N], or [residual_rows,N] broadcast) in fp16,
    # + the row statistics written / read by the LayerNorm-folded forms
    by = 0.0
    for n, a, _m in gemm:
        M, N, K, rr, sb = mnk(n, a)
        by += 2.0 * (M * K + N * K + M * N + rr * N) + sb
    achieved = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    gbs = by / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    # Which roofline binds these GEMMs?  Their arithmetic intensity is 2MNK / 2(MK + NK + MN [+ MN]) = 130-310 FLOP per
    # algorithmic byte at N, K in {384, 1152, 1536} -- below the machine balance of 2.5 PFLOP/s / 8 TB/s = 312 (403 against
    # the 6.2 TB/s a copy reaches): every one of them is HBM-bound by its own operands, so `bound` is "hbm" and the MFMA
    # figure is reported next to it.
    line["roofline"] = {
        "bound": "hbm", "kernel": "C-ABI entry isic_gemm_f16 (every Linear of the encoder with its bias / GELU / residual "
                                  "epilogue: 49 launches per forward; arithmetic intensity 130-310 FLOP per algorithmic "
                                  "byte < the machine balance 312)",
        "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
        "traffic": pmc_traffic("vit", images_per_step=n_img, image_size=S),
        "launches": len(gemm), "avg_launch_ms": ms / max(len(gemm), 1),
        "algorithmic_bytes_per_launch": by / max(len(gemm), 1),
        "algorithmic_gflop_per_launch": fl / max(len(gemm), 1) / 1e9, "share_of_step_time": ms * 1e-3 / elapsed,
        "mfma": {"achieved": achieved, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / MFMA_BF16_PEAK_TFLOPS},
        "measured": "HIP events inside the timed region",
    }
    line["kernel_time"] = split
    if world == 1 and not args.no_cpu_baseline:
        from oracle import vit as ovit
        p = {k: v.detach().float().cpu() for k, v in enc.state_dict().items()}
        default_threads, threads = torch.get_num_threads(), host_threads()
        torch.set_num_threads(threads)
        nb = 32
        xb = x[:nb].float().cpu()
        with torch.no_grad():
            ovit.forward_tokens(p, xb[:2])
            t0 = time.perf_counter()
            done = 0
            while done < 40 and time.perf_counter() - t0 < args.cpu_budget_s:
                ovit.forward_tokens(p, xb)
                done += 1
            dt = time.perf_counter() - t0
        torch.set_num_threads(default_threads)
        line["cpu_baseline"] = {"value": done * nb / dt, "unit": "images/s", "cores": threads, "kind": "port",
                                "sample": f"{done} forward passes of {nb} images (oracle/vit.py, fp32, torch CPU, {threads} "
                                          f"threads) after one warm-up pass", "host_cpus": os.cpu_count()}
    return line


def captured_stepper(fwd_bwd, opt, sync, clock, world):
    """A whole train step as hipGraph replays.  World size 1: ONE graph (forward, backward, AdamW, clock).  Data parallel: TWO
    graphs around the one thing that cannot be captured with the process group's own stream -- the bucketed gradient
    all-reduce (RCCL): [forward + backward] -> GradSync.finish() -> [AdamW + clock.advance()], so that a multi-GPU step costs
    the host two replays and one collective instead of ~80 launches (2.4 ms of enqueue for 1.2 ms of GPU work).
    CapturedStep restores parameters, moments and the clock after its warm-up steps.  -> (step(), label)"""
    from isic_hip import graphs as G

    def tail():
        opt.step(grad_scale=1.0 / world)
        clock.advance()
    if world == 1:
        def body():
            loss = fwd_bwd()
            tail()
            return loss
        cap = G.CapturedStep(body, optimizer=opt, clock=clock)
        return cap.replay, "hipGraph replay (device step clock)"
    cap_a = G.CapturedStep(fwd_bwd, optimizer=opt, clock=clock)
    cap_b = G.CapturedStep(tail, optimizer=opt, clock=clock)

    def step():
        loss = cap_a.replay()
        sync.reset()
        sync.finish()                      # sum all-reduce of the flat gradient buffer, waited for on this stream
        cap_b.replay()
        return loss
    return step, "two hipGraph replays around the gradient all-reduce (device step clock)"


# ----------------------------------------------------------------------------------------------- configs[3]: GNN
def run_gnn(args, world, rank, dev):
    import numpy as np
    from gnn_models import GraphMIL
    from isic_hip import ddp, ops, optim, train as T
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import knn_indices

    N, D, F, L, k, C = args.nodes, args.feat + args.node_radiomics, args.hidden, args.gnn_layers, args.knn_k, 7
    Gs = args.graphs_per_step
    n_graphs = max(2 * Gs, 512)
    torch.manual_seed(42)
    model = GraphMIL(input_dim=D, gnn_type="gcn", gnn_hidden=F, gnn_layers=L, gnn_dropout=0.5, gnn_heads=4, att_dim=128,
                     att_heads=4, pool_dropout=0.2, classifier_dim=128, classifier_light=True, num_classes=C).to(dev)
    model.train()
    model.set_dropout_state(seed=42, step=0)
    opt = optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    ddp.broadcast_parameters(opt.flat.data)
    sync = ddp.GradSync(opt.flat.grad, world_size=world)

    # synthetic graph records resident in HBM: node features with a class-dependent shift, k-NN edges built on device
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    y = (torch.arange(n_graphs, device=dev) + rank) % C
    x = torch.randn(n_graphs, N, D, device=dev, generator=gen) + 0.25 * y.view(-1, 1, 1).float()
    offs = BagOffsets.from_lengths([N] * n_graphs, dev)
    nn_idx = knn_indices(x.view(-1, D), offs, k).view(n_graphs, N, k)          # edges: k-NN of the patch embeddings
    if args.node_radiomics > 0:            # + a lesion-level radiomic vector on every node (pipeline.with_radiomic_node_features)
        import pipeline
        rad = torch.randn(n_graphs, args.node_radiomics, device=dev, generator=gen) + 0.25 * y.view(-1, 1).float()
        x = pipeline.with_radiomic_node_features(x, rad)
    src = torch.arange(N, device=dev).view(1, N, 1).expand(n_graphs, N, k)
    ei = torch.stack([src.reshape(n_graphs, -1), nn_idx.reshape(n_graphs, -1)], dim=1)      # [G, 2, N*k], local ids
    records = [{"x": x[i], "edge_index": ei[i], "y": int(y[i])} for i in range(n_graphs)]
    store = T.GraphStore(records, dev, True, mode=model.graph_mode)
    gidx = torch.Generator(device=dev).manual_seed(7 + rank)

    timer = KernelTimer.get() if args.full else None

    # One train step.  On one GPU the whole step (forward, autograd backward, AdamW) is captured into a hipGraph and
    # replayed: ~50 C-ABI launches + ~30 torch kernels for ~1.3 ms of GPU work cost the host more to enqueue than the GPU
    # to run.  The dropout stream id and Adam's step count come from a device step clock (isic_hip/graphs.py), the step's
    # graph indices from a static tensor refilled before each replay.  Multi-GPU runs (RCCL exchange) stay eager.
    from isic_hip import graphs as G
    use_graph = not args.no_graph
    idx_static = torch.zeros(Gs, device=dev, dtype=torch.int64)

    def fwd_bwd():
        xb, rows, n_rows, ob, gb = store.batch_rows(idx_static)      # no gather: the input projection reads through `rows`
        opt.zero_grad()
        with ops.fused_grad_accumulation():              # parameter gradients are added into the flat buffer by the kernels
            probs, _, loss = model(xb, offsets=ob, graph=gb, labels=store.y_dev[idx_static],      # head + loss: one node
                                   x_rows=(rows, n_rows))
            ops.backward(loss)
        return loss

    def body():
        loss = fwd_bwd()
        sync.reset()
        sync.finish()
        opt.step(grad_scale=1.0 / world)
        if clock is not None:
            clock.advance()
        return loss

    def draw():
        idx_static.random_(0, n_graphs, generator=gidx)              # drawn on the device, in place (one launch)

    def eager_step(i):
        draw()
        return body()

    clock = G.StepClock(dev).attach(model, opt) if use_graph else None
    for i in range(2):
        eager_step(i)
    captured, launch_label = captured_stepper(fwd_bwd, opt, sync, clock, world) if use_graph else (None, "eager")

    def step(i):
        if captured is None:
            return eager_step(i)
        draw()
        return captured()

    for i in range(args.warmup):
        step(i)
    SPMM = ["isic_spmm_csr_f32", "isic_gemm_f32_ws"]      # the roofline entry + the fp32 GEMMs (second-largest class)
    elapsed, host_s, loss = timed_region(step, args, world, dev, timer, SPMM, 2 + args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": loss, "params": opt.flat.data, "grads": opt.flat.grad})
    final_loss = float(loss.detach())
    # l1 norm of the parameters after settle + warm-up + timed steps: equal (to the AdamW step-size rounding, 1 ulp) for the
    # captured and the eager launch of the same run -- what the 2-rank rehearsal test compares
    param_l1 = float(opt.flat.data.double().abs().sum())
    if not args.full:
        if rank != 0:
            return None
        return gnn_line(args, world, elapsed, host_s, final_loss, param_l1, launch_label)
    spmm = timer.stop()
    measured = "HIP events inside the timed region"
    if captured is not None:
        # a replayed graph has no per-launch host call to bracket: the SAME step is run eagerly right after the timed
        # region with events around every launch of the entry (a kernel runs equally long from a graph)
        torch.cuda.synchronize()
        timer.start(SPMM)
        for i in range(args.steps):
            eager_step(i)
        torch.cuda.synchronize()
        spmm = timer.stop()
        measured = ("HIP events around every launch in an eager pass of the same steps right after the timed region "
                    "(the timed region replays a hipGraph of the step)")
    split = instrumented_pass(eager_step, timer, dev, world, start=0)
    if rank != 0:
        return None
    # The entry's launch duration proper: the step's six aggregation launches (three layers, forward operator and its
    # transpose, on the step's own batched graph) issued back to back, `reps` times, between ONE pair of HIP events on the
    # launch stream.  Events around a single 20 us launch also time the gap to the next enqueue (in_step_avg_launch_ms
    # below); rocprofv3's per-kernel average (profiles/r03_gnn_bench_kernel_stats.csv) is the number this one must match.
    from isic_hip.lib import call as _call
    _xb, _ob, gb = store.batch(idx_static)
    hb, ob_ = torch.randn(Gs * N, F, device=dev), torch.empty(Gs * N, F, device=dev)
    ops_ = [(gb.rowptr, gb.col, gb.val)] * L + [(gb.rowptr_t, gb.col_t, gb.val_t)] * L

    def six():
        for rp, c, v in ops_:
            _call("isic_spmm_csr_f32", rp, c, v, hb, None, ob_, Gs * N, F, 1.0, None, 0.0)
    reps = 20
    six()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        six()
    e1.record()
    torch.cuda.synchronize()
    batch_ms, batch_n = e0.elapsed_time(e1), reps * len(ops_)
    # compulsory bytes of one segmented-sum launch over the step's Gs graphs: read h + write out +
    # col + val + rowptr; E counts the self loops GCNConv adds
    E = N * k + N
    per_graph = 2 * N * F * 4 + 2 * E * 4 + (N + 1) * 4
    gemms = [(a, m) for n_, a, m in spmm if n_ == "isic_gemm_f32_ws"]
    spmm = [r for r in spmm if r[0] == "isic_spmm_csr_f32"]
    gemm_ms = sum(m for _a, m in gemms)
    gemm_fl = sum(2.0 * a[2] * a[3] * a[4] for a, _m in gemms)          # (transA, transB, M, N, K, ...)
    ms = sum(m for _n, _a, m in spmm)
    n_launch = len(spmm)
    # roofline.achieved = compulsory bytes of a launch / the launch duration measured INSIDE the step (HIP events around every
    # aggregation launch of the eager pass of the same steps); the back-to-back micro-loop (one 25.7 MB input / output pair
    # re-used by 120 launches: it sits in the 256 MB Infinity Cache) is kept as a labelled extra
    in_step_ms = ms / max(n_launch, 1)
    achieved = Gs * per_graph / (in_step_ms * 1e-3) / 1e9 if in_step_ms > 0 else 0.0
    b2b = Gs * per_graph * batch_n / (batch_ms * 1e-3) / 1e9 if batch_ms > 0 else 0.0
    line = gnn_line(args, world, elapsed, host_s, final_loss, param_l1, launch_label)
    line["roofline"] = {
        "bound": "hbm", "kernel": "C-ABI entry isic_spmm_csr_f32 (GCNConv aggregation: neighbour gather + segmented sum, "
                                  "forward and transposed backward)",
        "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
        "traffic": pmc_traffic("gnn", graphs_per_step=Gs, nodes=N, hidden=F, knn_k=k),
        "launches": n_launch, "avg_launch_ms": in_step_ms,
        "algorithmic_bytes_per_launch": Gs * per_graph, "compulsory_bytes_per_layer_per_graph": per_graph,
        "share_of_step_time": in_step_ms * 2 * L * args.steps * 1e-3 / elapsed,
        "measured": measured,
        "back_to_back": {"achieved": b2b, "frac": b2b / HBM_PEAK_GBS, "launches": batch_n, "avg_launch_ms": batch_ms / batch_n,
                         "measured": f"HIP events around {reps} x {len(ops_)} back-to-back launches of the step's own aggregations "
                                     f"({L} forward, {L} transposed) on ONE input / output pair right after the timed region: "
                                     f"a cache-resident best case, not the step"},
        # the step's largest kernel class next to it: every exact-fp32 GEMM launch of the step (v_mfma_f32_16x16x4_f32)
        "gemm_f32": {"bound": "mfma", "achieved": gemm_fl / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0,
                     "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": (gemm_fl / (gemm_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS) if gemm_ms > 0 else 0.0,
                     "launches": len(gemms), "ms_per_step": gemm_ms / max(args.steps, 1)},
    }
    line["kernel_time"] = split
    if world == 1 and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline_gnn(model, records, args.cpu_budget_s)
    return line


def gnn_line(args, world, elapsed, host_s, final_loss, param_l1, launch_label):
    """The configs[3] line without what --full adds."""
    Gs = args.graphs_per_step
    line = base_line("graphs/sec (GNN train step) @ 196-node k-NN patch graphs", "graphs/s",
                     world * Gs * args.steps / elapsed, world, args, elapsed, "f32")
    line["config"] = {"workload": WORKLOAD_GNN, "graphs_per_step_per_gpu": Gs, "nodes": args.nodes,
                      "feat": args.feat + args.node_radiomics, "node_radiomics": args.node_radiomics, "hidden": args.hidden,
                      "layers": args.gnn_layers, "knn_k": args.knn_k, "parallelism": f"dp{world}",
                      "host_enqueue_ms_per_step": host_s * 1e3 / args.steps, "final_loss": final_loss,
                      "step_launch": launch_label, "param_l1_after_run": param_l1}
    return line


def cpu_baseline_gnn(model, records, budget_s):
    """oracle/ per-graph 05 loop (`05_train_gnns.py:336-346`: one graph per optimizer step, fp32, torch CPU, AdamW)."""
    from oracle import gnn as ognn
    # dropout as in the GPU step beside it (gnn_dropout 0.5, classifier dropout 0.2; the oracle draws the same Philox words)
    cfg = dict(gnn_type="gcn", gnn_hidden=model.gnn_layers[0].lin.weight.shape[0], gnn_layers=len(model.gnn_layers),
               gnn_dropout=0.5, att_dim=128, classifier_dim=128, pool_dropout=0.2)
    p0 = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    recs = [{"x": r["x"].cpu(), "edge_index": r["edge_index"].cpu(), "y": r["y"]} for r in records[:64]]
    default_threads, threads = torch.get_num_threads(), host_threads()

    def run(nthreads, warm, n_steps, budget):
        torch.set_num_threads(nthreads)
        q = {k: torch.nn.Parameter(v.clone()) for k, v in p0.items()}
        opt = torch.optim.AdamW(list(q.values()), lr=1e-4, weight_decay=1e-4)

        def one(i):
            r = recs[i % len(recs)]
            opt.zero_grad()
            out = ognn.graphmil_forward(q, cfg, r["x"], r["edge_index"], drop={"seed": 42, "stream_base": i * 1024})
            ognn.graph_loss(out["probs"], r["y"]).backward()
            opt.step()
        for i in range(warm):
            one(i)
        t0 = time.perf_counter()
        done = 0
        for i in range(n_steps):
            one(warm + i)
            done += 1
            if time.perf_counter() - t0 > budget:
                break
        dt = time.perf_counter() - t0
        torch.set_num_threads(default_threads)
        return done / dt, done

    v_all, d_all = run(threads, 30, 400, budget_s / 2)
    v_one, d_one = run(1, 30, 400, budget_s / 2)
    # these steps are ~100 small ops: more threads are SLOWER (op-dispatch bound), so the headline
    # CPU figure is the faster setting and both are listed
    best, cores, done = (v_one, 1, d_one) if v_one >= v_all else (v_all, threads, d_all)
    return {"value": best, "unit": "graphs/s", "cores": cores, "kind": "port",
            "sample": f"{done} per-graph train steps (one 196-node graph per optimizer step, dropout 0.5 / 0.2 as the GPU step, "
                      f"fp32, torch CPU, {cores} thread(s)) after 30 warm-up steps",
            "all_threads": {"value": v_all, "cores": threads, "sample": f"{d_all} steps after 30 warm-up steps"},
            "one_thread": {"value": v_one, "cores": 1, "sample": f"{d_one} steps after 30 warm-up steps"},
            "host_cpus": os.cpu_count()}


# ----------------------------------------------------------------------------------------------- the reference's own hot loop
WORKLOAD_TEACHER = ("MIL teacher train step on resident [196, 768] fp32 latents (the reference's own hot loop, "
                    "01_train_mil_teacher.py:235-246 / utils_g_mil.py:66-105), B bags per optimizer step")


def run_teacher(args, world, rank, dev, H=None, A=None, with_cpu=True):
    """One step = forward + backward + AdamW of AttentionMIL_teacher over ``--teacher-bags-per-step`` bags of 196 x 768 fp32
    latents resident in HBM (mean of the per-bag losses of 01:244; SURVEY.md 7 "batch-vs-per-bag"), replayed as a hipGraph with
    the device step clock (dropout words and Adam's t follow the step).  Roofline ("MIL head + attention pool --
    HBM bound"): the head's kernels (fp32 GEMMs + attention pool, forward and backward) against the algorithmic bytes of a
    train step: x read by the forward projection and again by its weight gradient + the five outputs written."""
    from isic_hip import ddp, graphs as G, ops, optim
    from isic_hip.bags import BagOffsets
    from utils_g_mil import AttentionMIL_teacher
    N, D, C = 196, 768, 7
    H, A = H or args.teacher_hidden, A or args.teacher_att
    B = args.teacher_bags_per_step
    torch.manual_seed(42)
    model = AttentionMIL_teacher(D, H, A, 0.5, C).to(dev)
    model.train()
    model.set_dropout_state(seed=42, step=0)
    opt = optim.AdamW(model.parameters(), lr=2.2e-4, weight_decay=8.6e-4)        # the reference's tuned values (01:217-224)
    ddp.broadcast_parameters(opt.flat.data)
    sync = ddp.GradSync(opt.flat.grad, world_size=world)
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    n_sets = 4
    ys = [(torch.arange(B, device=dev) + s + rank) % C for s in range(n_sets)]
    xs = [(torch.randn(B, N, D, device=dev, generator=gen) + 0.25 * ys[s].view(B, 1, 1).float()).reshape(B * N, D)
          for s in range(n_sets)]
    offs = BagOffsets.uniform(B, N, dev)
    timer = KernelTimer.get() if args.full else None
    use_graph = not args.no_graph
    clock = G.StepClock(dev).attach(model, opt) if use_graph else None

    def make_fwd_bwd(s):
        def fwd_bwd():
            opt.zero_grad()
            with ops.fused_grad_accumulation():
                out = model(xs[s], offs)
                loss = ops.cross_entropy(out["bag_logits"], ys[s])
                ops.backward(loss)
            return loss
        return fwd_bwd
    fbs = [make_fwd_bwd(s) for s in range(n_sets)]

    def eager_step(i):
        loss = fbs[i % n_sets]()
        sync.reset()
        sync.finish()
        opt.step(grad_scale=1.0 / world)
        if clock is not None:
            clock.advance()
        return loss
    for i in range(2):
        eager_step(i)
    captured, launch_label = None, "eager"
    if use_graph:
        captured = []
        for fb in fbs:
            st, launch_label = captured_stepper(fb, opt, sync, clock, world)
            captured.append(st)

    def step(i):
        return captured[i % n_sets]() if captured is not None else eager_step(i)
    for i in range(args.warmup):
        step(i)
    elapsed, host_s, loss = timed_region(step, args, world, dev, timer, [], 0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": loss, "params": opt.flat.data, "grads": opt.flat.grad})
    final_loss = float(loss.detach())
    if args.full:
        timer.stop()
        # per-entry durations: the same steps launched eagerly right after the timed region, events around every launch
        n_inst = min(args.steps, 20)
        torch.cuda.synchronize()
        timer.start(None)
        for i in range(n_inst):
            eager_step(i)
        torch.cuda.synchronize()
        rec = timer.stop()
    if rank != 0:
        return None
    line = base_line("bags/sec (MIL teacher train step) @ 196x768 fp32 latents", "bags/s", world * B * args.steps / elapsed,
                     world, args, elapsed, "f32")
    line["config"] = {"workload": WORKLOAD_TEACHER, "bags_per_step_per_gpu": B, "patches_per_bag": N, "feat": D, "hidden": H,
                      "att_dim": A, "params": sum(p.numel() for p in model.parameters()), "parallelism": f"dp{world}",
                      "host_enqueue_ms_per_step": host_s * 1e3 / args.steps, "final_loss": final_loss,
                      "step_launch": launch_label}
    if not args.full:
        if clock is not None:
            G.StepClock.detach(model, opt)
        return line
    split = split_by_class(rec, n_inst)
    head = [(n_, a, m) for n_, a, m in rec if n_.startswith(("isic_gemm_f32", "isic_attn_pool", "isic_colsum"))]
    head_ms = sum(m for _n, _a, m in head) / n_inst
    gemm = [(a, m) for n_, a, m in rec if n_ in ("isic_gemm_f32_ws", "isic_gemm_f32")]
    gemm_ms = sum(m for _a, m in gemm)
    gemm_fl = sum(2.0 * a[2] * a[3] * a[4] for a, _m in gemm)                  # (transA, transB, M, N, K, ...)
    # algorithmic bytes of one TRAIN step per bag: forward reads x [N, D] fp32 and writes patch_logits,
    # patch_probs [N, C], attention [N], bag_logits, bag_probs [C]; backward reads x once more (dW1 = dh^T x; x needs no gradient)
    fwd_b = N * D * 4 + (2 * N * C + N + 2 * C) * 4
    bwd_b = N * D * 4
    step_bytes = B * (fwd_b + bwd_b)
    gbs = step_bytes / (head_ms * 1e-3) / 1e9 if head_ms > 0 else 0.0
    line["roofline"] = {
        "bound": "hbm", "kernel": "the head's C-ABI entries of one train step: isic_gemm_f32(_ws) (x W1^T + ReLU + dropout, "
                                  "h W2^T, their data / weight gradients), isic_attn_pool_fwd / _bwd, column sums",
        "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "traffic": None,
        "launches": len(head) // n_inst, "avg_launch_ms": head_ms / max(len(head) // n_inst, 1),
        "algorithmic_bytes_per_bag": fwd_b + bwd_b, "algorithmic_bytes_per_step": step_bytes,
        "kernel_ms_per_step": head_ms, "share_of_step_time": head_ms * 1e-3 * args.steps / elapsed,
        "mfma": {"achieved": gemm_fl / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0, "peak": MFMA_F32_PEAK_TFLOPS,
                 "unit": "TFLOP/s", "frac": (gemm_fl / (gemm_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS) if gemm_ms > 0 else 0.0,
                 "note": "the fp32 GEMMs alone (v_mfma_f32_16x16x4_f32): at 64-150 FLOP per algorithmic byte they sit above the "
                         "fp32 machine balance of 157.3 TF / 8 TB/s = 20, so the matrix core bounds them, not HBM"},
        "measured": "HIP events around every launch of an eager pass of the same steps right after the timed region "
                    "(the timed region replays hipGraphs of the step)" if captured is not None else "HIP events, eager steps",
    }
    line["kernel_time"] = split
    if world == 1 and with_cpu and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline_teacher(model, N, D, C, args.cpu_budget_s)
    if clock is not None:
        G.StepClock.detach(model, opt)
    return line


def cpu_baseline_teacher(model, N, D, C, budget_s):
    """oracle/mil.py per-bag loop (`01_train_mil_teacher.py:235-246`: one bag per optimizer step, fp32, torch CPU, AdamW),
    >= 200 steps after 30 warm-up steps, at one thread and at the box's CPU quota."""
    from oracle import mil as omil
    p0 = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    bags = [torch.randn(N, D, generator=g) + 0.25 * (i % C) for i in range(64)]
    default_threads, threads = torch.get_num_threads(), host_threads()

    def run(nthreads, warm, n_steps, budget):
        torch.set_num_threads(nthreads)
        q = {k: torch.nn.Parameter(v.clone()) for k, v in p0.items()}
        opt = torch.optim.AdamW(list(q.values()), lr=2.2e-4, weight_decay=8.6e-4)

        def one(i):
            opt.zero_grad()
            out = omil.teacher_forward(q, bags[i % len(bags)], drop={"p": 0.5, "seed": 42, "stream": i * 1024})
            omil.bag_loss(out["bag_logits"], torch.tensor(i % C)).backward()
            opt.step()
        for i in range(warm):
            one(i)
        t0 = time.perf_counter()
        done = 0
        for i in range(n_steps):
            one(warm + i)
            done += 1
            if done >= 200 and time.perf_counter() - t0 > budget:
                break
        dt = time.perf_counter() - t0
        torch.set_num_threads(default_threads)
        return done / dt, done
    v_all, d_all = run(threads, 30, 2000, budget_s / 2)
    v_one, d_one = run(1, 30, 2000, budget_s / 2)
    best, cores, done = (v_one, 1, d_one) if v_one >= v_all else (v_all, threads, d_all)
    return {"value": best, "unit": "bags/s", "cores": cores, "kind": "port",
            "sample": f"{done} per-bag train steps (one 196 x 768 bag per optimizer step, dropout 0.5 from the shared Philox "
                      f"stream, fp32, torch CPU, {cores} thread(s)) after 30 warm-up steps",
            "all_threads": {"value": v_all, "cores": threads, "sample": f"{d_all} steps after 30 warm-up steps"},
            "one_thread": {"value": v_one, "cores": 1, "sample": f"{d_one} steps after 30 warm-up steps"},
            "host_cpus": os.cpu_count()}


# ----------------------------------------------------------------------------------------------- the adjacency build of 03
WORKLOAD_KNN = ("k-NN adjacency build of 03_build_graphs.py:37-54 on 196 x 768 fp32 patch embeddings: the ten k values of "
                "03:104-105 (1..8, 12, 16) for every image, from ONE distance matrix + top-16 per image")


def run_knn(args, world, rank, dev):
    """One step = the ten k-NN edge lists (k = 1..8, 12, 16; `03_build_graphs.py:8-9,104-105`) of ``--knn-graphs-per-step``
    images: one isic_knn_graph launch (distance products on the fp32 matrix core + top-16 per node), then the ten
    ``edge_index[G, 2, 196 k]`` tensors (a smaller k is a prefix of the top-16).  Ranks are independent (03 is embarrassingly
    parallel over images: no exchange step)."""
    import build_graphs as bg
    import pipeline
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import knn_indices
    N, D = args.nodes, args.feat
    G_ = args.knn_graphs_per_step
    ks = [int(k) for k in bg.DEFAULT_K_VALUES]
    gen = torch.Generator(device=dev).manual_seed(4321 + rank)
    n_sets = 2
    xs = [torch.randn(G_, N, D, device=dev, generator=gen) for _ in range(n_sets)]
    offs = BagOffsets.uniform(G_, N, dev)
    src = {k: torch.arange(N, device=dev).view(1, N, 1).expand(G_, N, k).reshape(G_, -1) for k in ks}
    timer = KernelTimer.get() if args.full else None

    def step(i):
        nn = knn_indices(xs[i % n_sets].view(-1, D), offs, max(ks)).view(G_, N, max(ks))
        return {k: torch.stack([src[k], nn[:, :, :k].reshape(G_, -1)], dim=1) for k in ks}      # 03:52-53, source-major

    def step_k8(i):
        nn = knn_indices(xs[i % n_sets].view(-1, D), offs, 8).view(G_, N, 8)
        return torch.stack([src[8], nn.reshape(G_, -1)], dim=1)
    for i in range(2 + args.warmup):
        step(i)
        if args.full:
            step_k8(i)
    elapsed, host_s, edges = timed_region(step, args, world, dev, timer, ["isic_knn_graph"], 0)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {f"edge_index_knn{k}": e for k, e in edges.items()})
    if args.full:
        rec = timer.stop()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step_k8(i)
        torch.cuda.synchronize()
        k8_elapsed = time.perf_counter() - t0
    if rank != 0:
        return None
    line = base_line("graphs/sec (k-NN adjacency build, all ten k of 03_build_graphs.py) @ 196x768 patch embeddings",
                     "graphs/s", world * G_ * args.steps / elapsed, world, args, elapsed, "f32")
    line["config"] = {"workload": WORKLOAD_KNN, "graphs_per_step_per_gpu": G_, "nodes": N, "feat": D, "k_values": ks,
                      "parallelism": f"replicas{world}", "host_enqueue_ms_per_step": host_s * 1e3 / args.steps}
    if not args.full:
        return line
    line["config"]["k8_only_graphs_per_s"] = world * G_ * args.steps / k8_elapsed
    ms = sum(m for _n, _a, m in rec)
    fl = 2.0 * N * N * D * G_ * len(rec)                       # 2 N^2 D per image (59 MFLOP at 196 x 768)
    achieved = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
    line["roofline"] = {
        "bound": "mfma", "kernel": "C-ABI entry isic_knn_graph (row norms + per-image distance products x x^T on "
                                   "v_mfma_f32_16x16x4_f32 + top-16 selection, one launch per step)",
        "achieved": achieved, "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / MFMA_F32_PEAK_TFLOPS,
        "traffic": None, "launches": len(rec), "avg_launch_ms": ms / max(len(rec), 1),
        "algorithmic_gflop_per_launch": fl / max(len(rec), 1) / 1e9,
        "algorithmic_bytes_per_launch": G_ * (N * D * 4 + N * 16 * 8),
        "share_of_step_time": ms * 1e-3 / elapsed, "measured": "HIP events inside the timed region",
    }
    if world == 1 and not args.no_cpu_baseline:
        from oracle import graphs as ograph
        default_threads, threads = torch.get_num_threads(), host_threads()
        xc = xs[0][:64].cpu()

        def run(nthreads, budget):
            torch.set_num_threads(nthreads)
            for g in range(4):
                ograph.knn_edge_index(xc[g], 8)
            t0, done = time.perf_counter(), 0
            while done < 2000 and (done < 200 or time.perf_counter() - t0 < budget):
                for k in ks:                                   # the reference recomputes the distances for every k (03:104-105)
                    ograph.knn_edge_index(xc[done % 64], k)
                done += 1
            dt = time.perf_counter() - t0
            torch.set_num_threads(default_threads)
            return done / dt, done
        v_all, d_all = run(threads, args.cpu_budget_s / 2)
        v_one, d_one = run(1, args.cpu_budget_s / 2)
        best, cores, done = (v_one, 1, d_one) if v_one >= v_all else (v_all, threads, d_all)
        line["cpu_baseline"] = {"value": best, "unit": "graphs/s", "cores": cores, "kind": "port",
                                "sample": f"{done} images x the ten k values (oracle/graphs.knn_edge_index = 03:37-54 per k, fp32, "
                                          f"torch CPU, {cores} thread(s)) after 4 warm-up images",
                                "all_threads": {"value": v_all, "cores": threads, "sample": f"{d_all} images"},
                                "one_thread": {"value": v_one, "cores": 1, "sample": f"{d_one} images"},
                                "host_cpus": os.cpu_count()}
    return line


# ----------------------------------------------------------------------------------------------- configs[4]: the whole chain
WORKLOAD_PIPELINE = ("Full pipeline (BASELINE.json configs[4]): 224x224 images -> frozen ViT-S/16 fp16 tokens [196 x 384] -> "
                     "MIL teacher trained on the token bags (01) -> teacher outputs + dominant classes + all ten k-NN graphs on "
                     "the device (02 / 03) -> edge heterophily (04) -> heterophily-aware GCNII trained on the knn8 graphs (05)")


def run_pipeline(args, world, rank, dev):
    """Per-stage wall time of the configs[4] chain on ``--pipeline-images`` synthetic images per GPU, everything resident in HBM
    between the stages (pipeline.py).  Ranks are replicas of the chain (each on its own images); the value is images through
    the WHOLE chain per second."""
    import numpy as np
    import measure_heterophily as mh
    import pipeline
    from gnn_models import GraphMIL
    from isic_hip import train as T
    from isic_hip.vit import ViTSmallEncoder
    from utils_g_mil import AttentionMIL_teacher
    n_img, C = args.pipeline_images, 7
    n_val = max(C, n_img // 8)
    torch.manual_seed(42)
    enc = ViTSmallEncoder(img_size=224).to(dev)
    gen = torch.Generator(device=dev).manual_seed(77 + rank)
    labels = (np.arange(n_img) + rank) % C
    stages = {}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        stages[name] = time.perf_counter() - t0
        return out

    def encode():
        toks = []
        for lo in range(0, n_img, 512):                       # images are drawn on the device, 512 at a time (300 MB each)
            n = min(512, n_img - lo)
            x = torch.randn(n, 3, 224, 224, device=dev, generator=gen)
            y = torch.as_tensor(labels[lo:lo + n], device=dev)
            x += 0.6 * ((y.view(-1, 1, 1, 1) % 4).float() - 1.5)         # a class-dependent offset the teacher can learn
            toks.append(enc.run_tokens(x))
        return torch.cat(toks)                                 # [n_img, 196, 384] fp32, resident
    enc.run_tokens(torch.randn(8, 3, 224, 224, device=dev, generator=gen))                        # warm-up (weight preparation)
    tokens = timed("encode_vit_s16", encode)
    tr_i, va_i = np.arange(n_val, n_img), np.arange(0, n_val)
    teacher = AttentionMIL_teacher(384, 128, 64, dropout=0.5, num_classes=C).to(dev)
    t_epochs = 2
    timed("train_teacher", lambda: T.train_teacher_fold(teacher, [tokens[i] for i in tr_i], labels[tr_i], [tokens[i] for i in va_i],
                                                        labels[va_i], lr=2.2e-4, epochs=t_epochs, patience=t_epochs,
                                                        bags_per_step=256, device=dev, log=lambda *a, **k: None))
    ids = [f"img_{i}" for i in range(n_img)]
    outs = timed("teacher_outputs_and_all_k_knn", lambda: [
        pipeline.collect_teacher_outputs_device(teacher, tokens[idx], labels[idx], [ids[i] for i in idx], dev) for idx in (tr_i, va_i)])
    n_het = min(256, len(tr_i))

    def heterophily():
        ei = outs[0].knn_edge_index(8)[:n_het]
        return mh.compute_edge_heterophily_batch(list(outs[0].x[:n_het].cpu().numpy()), list(outs[0].patch_probs[:n_het].cpu().numpy()),
                                                 list(outs[0].dominant_class[:n_het].cpu().numpy()), list(ei.cpu().numpy()), device=str(dev))
    timed("edge_heterophily", heterophily)
    torch.manual_seed(1)
    gnn = GraphMIL(384, "gcnii", 128, 3, 0.5, att_dim=128, att_heads=4, pool_dropout=0.2, classifier_dim=128, classifier_light=True,
                   num_classes=C).to(dev)
    g_epochs = 2
    vm, _tm, _best = timed("train_gcnii_on_knn8", lambda: pipeline.train_gnn_from_teacher(
        gnn, outs[0], outs[1], outs[1], "knn8", lr=1e-4, epochs=g_epochs, graphs_per_step=256, num_classes=C, device=dev,
        rng=np.random.RandomState(2)))
    total = sum(stages.values())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"tokens": tokens, **{f"{name}_params": torch.cat([p.detach().reshape(-1) for p in m.parameters()])
                                                              for name, m in (("teacher", teacher), ("gnn", gnn))}})
    if world > 1:
        t = torch.tensor([total], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        total = float(t.item())
    if rank != 0:
        return None
    line = {"metric": "images/sec through the whole configs[4] chain (encode -> teacher -> graphs -> heterophily -> GNN)",
            "value": world * n_img / total, "unit": "images/s", "n_gpus": world, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16 encoder, f32 heads", "data": "synthetic",
            "config": {"workload": WORKLOAD_PIPELINE, "images_per_gpu": n_img, "validation_images": n_val, "teacher_epochs": t_epochs,
                       "gnn_epochs": g_epochs, "heterophily_images": n_het, "parallelism": f"replicas{world}",
                       "final_val_bacc_gnn": float(vm["bacc"])},
            "seconds_per_stage": {k: round(v, 4) for k, v in stages.items()},
            "per_stage_rate": {"encode_images_per_s": n_img / stages["encode_vit_s16"],
                               "teacher_bags_per_s": t_epochs * len(tr_i) / stages["train_teacher"],
                               "graph_build_images_per_s": n_img / stages["teacher_outputs_and_all_k_knn"],
                               "heterophily_images_per_s": n_het / stages["edge_heterophily"],
                               "gnn_graphs_per_s": g_epochs * len(tr_i) / stages["train_gcnii_on_knn8"]},
            "note": "stage times include their evaluation passes, host-side epoch bookkeeping and (heterophily) the export of its "
                    "inputs to numpy as 04's interface takes them; rooflines and CPU baselines of the kernels behind each stage "
                    "are on the vit / teacher / knn / gnn sub-lines"}
    return line


def host_threads():
    """CPUs this process may actually keep busy: the affinity mask clipped by the cgroup CPU quota.  On the GPU box
    `os.cpu_count()` is 256 and torch defaults to 128 threads, but the container's quota is 16 CPUs: measured there, a
    3x3 convolution runs at 3.3 TFLOP/s with 16 threads and at 0.04 with 128 (throttled) -- a CPU baseline taken with the
    default thread count understates the host by two orders of magnitude."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:                  # cgroup v2: "<quota> <period>" or "max <period>"
            q, per = f.read().split()
        if q != "max":
            n = min(n, max(1, -(-int(q) // int(per))))
    except (OSError, ValueError):
        try:                                                       # cgroup v1
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = int(f.read())
            if q > 0:
                n = min(n, max(1, -(-q // per)))
        except (OSError, ValueError):
            pass
    return n


# ----------------------------------------------------------------------------------------------- shared pieces
def timed_region(step, args, world, dev, timer, names, first):
    """EXACTLY ``args.steps`` steps between barrier + synchronize on both sides; MAX over ranks.  ``timer`` (--full only;
    None otherwise) brackets the launches of the entries ``names`` with HIP events."""
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    if timer is not None:
        timer.start(names)
    t0 = time.perf_counter()
    host_s = 0.0
    loss = None
    for i in range(args.steps):
        th = time.perf_counter()
        loss = step(first + i)
        host_s += time.perf_counter() - th          # host time to ENQUEUE the step (the GPU runs behind it)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if timer is not None:
        timer.active = False
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed, host_s, loss


def instrumented_pass(step, timer, dev, world, start, steps=3):
    """Untimed: ``steps`` more steps with EVERY C-ABI launch bracketed by HIP events -> kernel time per class."""
    torch.cuda.synchronize()
    timer.start(None)
    for i in range(steps):
        step(start + i)
    torch.cuda.synchronize()
    rec = timer.stop()
    if world > 1:
        dist.barrier()
    return split_by_class(rec, steps)


def base_line(metric, unit, value, world, args, elapsed, dtype):
    return {"metric": metric, "value": value, "unit": unit, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": dtype, "data": "synthetic"}


DUMP_BYTES = 64_000_000


def dump_outputs(dirname, arrays):
    """--dump-outputs: ``arrays`` (name -> tensor) as ``dirname/<name>.npy`` in float32, DUMP_BYTES in all.  The smallest
    arrays are written whole; one larger than its share of what is left becomes a fixed sample of its flattened elements
    (seed 0, indices ascending), so the same arguments pick the same elements in every build."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    left = DUMP_BYTES - 1024 * len(arrays)                  # the .npy headers
    items = sorted(arrays.items(), key=lambda kv: kv[1].numel())
    for i, (name, t) in enumerate(items):
        t = t.detach().float()
        cap = left // (len(items) - i) // 4
        if t.numel() > cap:
            idx = np.sort(np.random.default_rng(0).choice(t.numel(), cap, replace=False))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        a = t.cpu().numpy()
        np.save(os.path.join(dirname, f"{name}.npy"), a)
        left -= a.nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("mil", "gnn", "vit", "teacher", "knn", "pipeline"), default="mil")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bags-per-step", type=int, default=64,
                    help="mil: bags per optimizer step PER GPU (round 4: 64 = 4096 images of 224^2, every activation still "
                         "resident (~45 GB); 32 / 48 / 64 bags per step: 851 / 880 / 894 bags/s on one box -- the persistent "
                         "kernels' tails and the per-launch fixed costs are spread over more work; the pixel count of layer1, "
                         "4096 x 56 x 56 = 12.8 M, has to stay below the 2^24 of the kernels' 40-bit reciprocal division)")
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--radiomics-dim", type=int, default=128)
    ap.add_argument("--graphs-per-step", type=int, default=668,
                    help="gnn: graphs per optimizer step PER GPU (round 4: 668 x 196 nodes = 511.4 row tiles of 256 = two full "
                         "rounds over the 256 CUs; a replayed step costs >= 4.8 us per dependent kernel whatever its size, and at "
                         "256 graphs those fixed costs are a quarter of the step: 256 / 512 / 668 / 1024 graphs per step = 220 / "
                         "258 / 275 / 275 k graphs/s on one box)")
    ap.add_argument("--images-per-step", type=int, default=2048, help="vit: images per forward PER GPU")
    ap.add_argument("--teacher-bags-per-step", type=int, default=668,
                    help="teacher: bags of 196 x 768 latents per step PER GPU (as --graphs-per-step: 256 / 512 / 668 / 1024 = "
                         "413 / 485 / 503 / 514 k bags/s)")
    ap.add_argument("--teacher-hidden", type=int, default=128)
    ap.add_argument("--teacher-att", type=int, default=64)
    ap.add_argument("--knn-graphs-per-step", type=int, default=2048, help="knn: images per adjacency-build step PER GPU")
    ap.add_argument("--pipeline-images", type=int, default=2048, help="pipeline: images per GPU through the configs[4] chain")
    ap.add_argument("--nodes", type=int, default=196)
    ap.add_argument("--feat", type=int, default=768)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--gnn-layers", type=int, default=3)
    ap.add_argument("--knn-k", type=int, default=8)
    ap.add_argument("--node-radiomics", type=int, default=0,
                    help="gnn: append an R-d lesion-level radiomic vector to every node's features (configs[3] 'radiomic node "
                         "feats'; the reference's graph records carry patch embeddings only, so the default is 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--wgrad-stream", action="store_true",
                    help="mil: weight gradients on a second HIP stream (A/B; off by default: concurrent kernels blur the "
                         "per-kernel timings the roofline is computed from)")
    ap.add_argument("--bn-fusion", action="store_true",
                    help="mil: fold the BatchNorm-backward reductions of stages 2-4 into the data gradients (A/B; off by default)")
    ap.add_argument("--cpu-budget-s", type=float, default=20.0)
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="multi-rank REHEARSAL for a box with one GPU: every rank uses cuda:0 and the collectives run "
                         "over gloo.  Exercises sharding, the bucketed gradient exchange fired by a real backward and the "
                         "buffer averaging; the printed rate is NOT a scaling measurement (ranks share one GPU)")
    ap.add_argument("--no-graph", action="store_true", help="gnn: launch the step eagerly instead of replaying its hipGraph")
    ap.add_argument("--no-sublines", action="store_true",
                    help="mil: do not attach the short configs[3] (gnn) and configs[4] (vit) runs to the line")
    ap.add_argument("--sub-steps", type=int, default=20, help="timed steps of each attached sub-benchmark")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: sub-benchmarks, rooflines, per-class kernel time, "
                         "CPU baselines (off: set up, warm up, time --steps steps, print the line)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float32, 64 MB in all)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start one process per GPU "
                         f"(torch.distributed.run --nproc-per-node {args.gpus}, or plain `python bench.py --gpus N`)")
    if args.rehearse_on_one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.rehearse_on_one_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    def run_teacher_both(a, w, r, d):
        """the reference's default head (H128 / A64) with its tuned head (H368 / A772) attached as `tuned`"""
        line = run_teacher(a, w, r, d)
        if not a.full:
            return line
        release_device_memory()
        tuned = run_teacher(argparse.Namespace(**dict(vars(a), dump_outputs=None)), w, r, d, H=368, A=772)
        if r == 0:
            line["tuned"] = tuned
        return line
    runners = {"mil": run_mil, "gnn": run_gnn, "vit": run_vit, "teacher": run_teacher_both, "knn": run_knn,
               "pipeline": run_pipeline}
    line = runners[args.config](args, world, rank, dev)
    if args.config == "mil" and args.full and not args.no_sublines:
        # BASELINE.json configs[3] and configs[4] ride on the SAME line (the driver parses one line): short runs of the
        # graph step and of the ViT encoder, then the reference's OWN hot loop (the teacher step on resident latents) and the
        # adjacency build of 03, each with its own roofline and cpu_baseline
        sub_args = argparse.Namespace(**vars(args))
        sub_args.steps, sub_args.warmup = args.sub_steps, 3
        sub_args.dump_outputs = None
        sub_args.cpu_budget_s = min(args.cpu_budget_s, 10.0)
        for name in ("gnn", "vit", "teacher", "knn", "pipeline"):
            release_device_memory()
            try:
                sub = runners[name](sub_args, world, rank, dev)
            except Exception as e:                      # a sub-benchmark must never cost the headline line
                sub = {"error": f"{type(e).__name__}: {e}"}
                if world > 1:
                    raise
            if rank == 0:
                line[name] = sub
    if rank == 0:
        line["kernel_source_hash"] = kernel_source_hash()
        if args.rehearse_on_one_gpu:
            line["rehearsal"] = "all ranks on one GPU, gloo collectives: a functional check, not a scaling number"
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def release_device_memory():
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def self_launch(args):
    """``python bench.py --gpus N`` started bare (no torchrun): this parent has not touched the GPU (importing torch
    and parsing arguments does not), so it starts one CHILD process per GPU with the torchrun environment
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*), relays rank 0's JSON line and returns the worst exit code.  Children
    are new processes (subprocess), never an exec of this one."""
    import socket
    import subprocess
    n = args.gpus          # the parent never asks the runtime anything: a child whose device is missing exits non-zero
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL, text=True))
    out, _ = procs[0].communicate()
    rcs = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out or "")
    sys.stdout.flush()
    return max(abs(rc) for rc in rcs)


if __name__ == "__main__":
    main()
