"""ConvMAE-Base patch encoder, fp16 (or, opt-in, MXFP8) on gfx950 -- the encoder the reference makes its patch latents with.

The reference builds ``convmae_convvit_base_patch16_dec512d8b(with_decoder=False)``, loads a checkpoint of its
``train_ae.py`` with ``strict=False`` and runs ``forward(images, mask_ratio=0) -> latent[B, 196, 768]``
(`save_latent.py:17-18,42-60`).  This module restates the encoder of the published ConvMAE code (Gao et al. 2022,
``models_convmae.py`` / ``vision_transformer.py``), which neither the reference nor this tree vendors: PARITY IS UNPINNED,
as for the ViT-S/16 (isic_hip/vit.py).  ``tests/convmae_ref.py`` is the fp32 torch-CPU restatement it is checked against.
Parameter names and shapes are the checkpoint's, so a reference checkpoint loads (convolution weights keep their OIHW
shapes in the state dict).  Frozen by default; ``trainable=True`` fine-tunes it (below).

    patch_embed1   Conv2d(3->256, k4 s4) -> LayerNorm -> GELU                       56 x 56 x 256
    blocks1.0-1    CBlock(256): x += conv2(dw5x5(conv1(LN1(x)))); x += fc2(GELU(fc1(LN2(x))))   (1x1 convs, hidden 1024)
    stage1_output_decode  Conv2d(256->768, k4 s4) on the blocks1 output -> s1[N, 196, 768]
    patch_embed2   Conv2d(256->384, k2 s2) -> LN -> GELU                             28 x 28 x 384
    blocks2.0-1    CBlock(384), hidden 1536;  stage2_output_decode Conv2d(384->768, k2 s2) -> s2
    patch_embed3   Conv2d(384->768, k2 s2) -> LN -> GELU -> 196 tokens in raster order
    patch_embed4   Linear(768->768), + pos_embed[1, 196, 768]
    blocks3.0-10   pre-norm transformer blocks (timm names), 12 heads of 64, qkv bias, MLP 3072, erf-GELU
    output         norm(x + s1 + s2) -> latent fp32

Details the published code fixes only through its defaults, each a constructor argument:
  * ``ln_eps=1e-6`` -- the LayerNorms of ``blocks3`` and ``norm``: the factory passes ``partial(nn.LayerNorm, eps=1e-6)``;
  * ``conv_ln_eps=1e-5`` -- the LayerNorms of the CBlocks and PatchEmbeds, which build ``nn.LayerNorm(dim)`` themselves;
  * ``pos_embed``: MAE's fixed 2-D sin-cos table ``get_2d_sincos_pos_embed(768, 14)`` (computed in float64, stored fp32:
    with w_k = 10000^(-k/192), k < 192, token (row i, column j) is [sin(j w), cos(j w), sin(i w), cos(i w)]).  It is a
    parameter, so a checkpoint's own ``pos_embed`` overrides it.
No masking: at ``mask_ratio=0`` ConvMAE's convolution masks are all ones and its token shuffle is undone by the reference
itself through ``ids_keep`` (`save_latent.py:118-126`), so the tokens stay in raster order (identity ``ids_keep`` /
``ids_restore``, as ``save_latent._extract_from_loader`` writes them).

Tensors are NHWC inside (pixel rows of C channels, fp16 in HBM, fp32 arithmetic in the kernels).  The launches:
``isic_patch_rows_nchw_f32`` (the stem's 4 x 4 patches, K = 48 zero-padded to 64) and ``isic_patch_rows_nhwc_f16`` (the
other patch / decode convolutions as space-to-depth rows), ``isic_gemm_f16`` for every 1x1 / patch / decode convolution
and ``patch_embed4`` (whose ``residual_rows = 196`` adds the position embedding), ``isic_dwconv5x5_f16`` for the CBlock's
token mixer, ``isic_layernorm_add_f16`` for the PatchEmbed norms (+ GELU) and the final ``norm(x + s1 + s2)``, and the
ViT-B stage on ``isic_gemm_f16_ln`` / ``_stats`` and ``isic_attention_f16``.  No CPU fallback.

``fold_layernorm=True`` (default): the pre-norms of the CBlocks and of blocks3 are folded into the product that follows
(isic_hip/vit.py explains the algebra), with the row statistics out of the epilogue of the product that wrote the stream
(``isic_row_stats_f16`` for the first block of a stage, whose input a LayerNorm + GELU wrote).  ``False``: every pre-norm
is a pass of ``isic_layernorm_add_f16`` followed by a plain product -- the form to compare against when a pretrained
stream carries rows with large offsets, where the fold's E[x^2] - mean^2 cancels.

``precision="mxfp8"`` (opt-in, inference only; the default ``"fp16"`` is the path above, bit for bit): every product but
the stem's runs on the block-scaled FP8 MFMA (``isic_gemm_mxfp8``; OCP MX E4M3, one E8M0 scale per 32 elements along K,
csrc/mxfp8.hip), and the launch in front of a product writes its operand as MXFP8 straight from fp32 values
(include/isic_hip_convmae_mxfp8.h).  MX(.) = quantised, fp16(.) = rounded to fp16, the rounding points in order:
    stem        unchanged (K = 48 padded to 64 is no multiple of 128): fp16 rows, ``isic_gemm_f16``, LayerNorm + GELU -> fp16 x
    CBlock      h = MX(LN1(x)) (``isic_layernorm_act_mxfp8_f16``); d = fp16(conv1(h)); m = MX(dw5x5(d) + b)
                (``isic_dwconv5x5_mxfp8_f16``); x2 = fp16(x + conv2(m)); h2 = MX(LN2(x2)); hid = MX(GELU(fc1(h2))) (the
                product's MXFP8 output: the 1024 / 1536-wide hidden map crosses HBM at 1 + 1/32 byte per value);
                x = fp16(x2 + fc2(hid))
    stage outputs  ``isic_patch_rows_mxfp8_nhwc_f16`` per consumer: stage 1 with P = 4 (stage1_output_decode) and P = 2
                (patch_embed2), stage 2 with P = 2 once (stage2_output_decode and patch_embed3); decoders -> fp16 s1, s2
    patch_embed2   product -> fp16, ``isic_layernorm_add_f16`` + GELU -> fp16 x;   patch_embed3: product -> fp16, then
                MX(GELU(LN(.))) (its only reader is patch_embed4);   patch_embed4: + pos_embed (fp16) -> fp16 x
    blocks3     the ViT's MXFP8 block at D = 768 (``transformer.blocks_forward_mx``): LN -> MX, qkv -> fp16, ``isic_attention_f16``,
                ``isic_mxfp8_quantize``, proj + residual -> fp16, LN -> MX, fc1 + GELU -> MX, fc2 + residual -> fp16
    output      norm(x + s1 + s2) -> fp32, unchanged
The LayerNorms are passes of their own (no fold, no row statistics: isic_hip/vit.py says why), so ``fold_layernorm=False``
and ``trainable=True`` are ``ValueError`` with it.  The product matrices are quantised on the GPU from the fp32 masters in
their [O][kh][kw][I] row order, once per weight version (``load_state_dict`` invalidates them); biases, LayerNorm
affines and the depthwise taps stay fp32, ``pos_embed`` fp16.  ``max_batch`` and ``depth`` work as for fp16, and an
image's tokens do not depend on its batch or chunk.  ``tests/convmae_mxfp8_ref.py`` is the CPU emulation of these
rounding points: 0.091 relative Frobenius error and a minimum per-token cosine of 0.9946 against the fp32 restatement
(fp16: 1.1e-3).

``trainable=True`` (opt-in; the default stays the frozen encoder above, bit for bit): the parameters require grad,
``train()`` works (no dropout or drop-path: the mode changes no arithmetic) and the encoder runs the layer-by-layer form
(``fold_layernorm=False``).  Under grad, ``forward`` / ``forward_tokens`` go through ``transformer.EncoderFn``: a
forward that is bitwise ``run_tokens`` of the unfolded form and saves its activations (fp16: per CBlock x, LN1(x),
conv1's output, the depthwise output, x2, LN2(x2), fc1's pre-activation and GELU output; per transformer block the set
of isic_hip/transformer.py; the three PatchEmbed convolution outputs and the two stage outputs; about 0.12 GB per image,
31 GB at 256 images), and a native backward (include/isic_hip_convmae_train.h + include/isic_hip_vit_train.h) that
accumulates into ``param.grad``.  The backward runs in fp16 under a power-of-two loss scale S = 2^round(8 - log2 amax(d
tokens)), one device -> host read per call; every reduction into a parameter gradient multiplies by 1/S in fp32, so
gradients are exactly scale-equivariant.  An fp16 overflow is not retried: the backward checks the gradients once at its
end and raises ``FloatingPointError``.  The training forward does not chunk the batch (``max_batch`` applies to
``run_tokens``).

Memory: the batch runs in chunks of at most ``max_batch`` images (default 256); stage 1 holds about 15 MB of fp16
activations per image of a chunk (the fc1 output alone is 3136 x 1024 x 2 bytes), 3.9 GB at 256 images.  An image's
tokens do not depend on the batch or the chunk it is in.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from .lib import call
from .transformer import (Backward, Encoder, EncoderFn, blocks_backward, blocks_forward, blocks_forward_mx,
                          blocks_workspace_bytes, check_grads, embed, fold_layernorm, linear_ln, linear_res, loss_scale,
                          mx_weights, param_grads)

_F16 = torch.float16


def sincos_pos_embed(dim=768, grid=14):
    """MAE's ``get_2d_sincos_pos_embed(dim, grid)`` without a class token: [grid*grid, dim] float64 (numpy)."""
    q = dim // 4
    omega = 1.0 / 10000 ** (np.arange(q, dtype=np.float64) / q)
    gy, gx = np.meshgrid(np.arange(grid, dtype=np.float64), np.arange(grid, dtype=np.float64), indexing="ij")
    ow = np.einsum("m,d->md", gx.reshape(-1), omega)            # column j
    oh = np.einsum("m,d->md", gy.reshape(-1), omega)            # row i
    return np.concatenate([np.sin(ow), np.cos(ow), np.sin(oh), np.cos(oh)], axis=1)


class _PatchEmbed(nn.Module):
    def __init__(self, cin, cout, k, eps):
        super().__init__()
        self.proj = nn.Conv2d(cin, cout, k, stride=k)
        self.norm = nn.LayerNorm(cout, eps=eps)


class _CMlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Conv2d(dim, hidden, 1)
        self.fc2 = nn.Conv2d(hidden, dim, 1)


class _CBlock(nn.Module):
    def __init__(self, dim, hidden, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.conv1 = nn.Conv2d(dim, dim, 1)
        self.attn = nn.Conv2d(dim, dim, 5, padding=2, groups=dim)
        self.conv2 = nn.Conv2d(dim, dim, 1)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = _CMlp(dim, hidden)


class _Attention(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):
    def __init__(self, dim, hidden, eps):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = _Attention(dim)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = _Mlp(dim, hidden)


class ConvMAEBaseEncoder(Encoder):
    """Frozen ConvMAE-Base encoder (module docstring).  ``run_tokens(images[N,3,224,224]) -> [N, 196, 768]`` fp32.
    ``precision``: ``"fp16"`` (default) or ``"mxfp8"`` (the products on the block-scaled FP8 MFMA; inference only)."""

    _who = "ConvMAEBaseEncoder"
    img_size, in_ch, tokens = 224, 3, 196
    dims, depths, grids, patches = (256, 384, 768), (2, 2, 11), (56, 28, 14), (4, 2, 2)

    def __init__(self, seed=0, fold_layernorm=None, ln_eps=1e-6, conv_ln_eps=1e-5, heads=12, mlp_ratio=4, max_batch=256,
                 trainable=False, precision="fp16"):
        super().__init__()
        if trainable not in (True, False):
            raise ValueError("trainable: True or False")
        if precision not in ("fp16", "mxfp8"):
            raise ValueError("precision: 'fp16' or 'mxfp8'")
        if precision == "mxfp8" and trainable:
            raise ValueError("trainable=True: fp16 only (no MXFP8 training)")
        if precision == "mxfp8" and fold_layernorm not in (None, True):
            raise ValueError("precision='mxfp8' runs its LayerNorms as passes of their own: leave fold_layernorm at its default")
        if trainable and fold_layernorm not in (None, False):
            raise ValueError("trainable=True runs the layer-by-layer form: leave fold_layernorm unset (or False)")
        if fold_layernorm is None:
            fold_layernorm = not trainable
        if fold_layernorm not in (True, False):
            raise ValueError("fold_layernorm: True or False")
        if max_batch < 1:
            raise ValueError("max_batch >= 1")
        d1, d2, d3 = self.dims
        if d3 // heads != 64 or d3 % heads != 0:
            raise ValueError("ConvMAEBaseEncoder: head width 64 (isic_attention_f16)")
        self.fold_layernorm, self.ln_eps, self.conv_ln_eps = fold_layernorm, float(ln_eps), float(conv_ln_eps)
        self.heads, self.mlp_ratio, self.max_batch = heads, mlp_ratio, int(max_batch)
        self.precision = precision
        self.feature_dim = self.out_dim = d3
        self.patch_embed1 = _PatchEmbed(self.in_ch, d1, 4, conv_ln_eps)
        self.patch_embed2 = _PatchEmbed(d1, d2, 2, conv_ln_eps)
        self.patch_embed3 = _PatchEmbed(d2, d3, 2, conv_ln_eps)
        self.patch_embed4 = nn.Linear(d3, d3)
        self.stage1_output_decode = nn.Conv2d(d1, d3, 4, stride=4)
        self.stage2_output_decode = nn.Conv2d(d2, d3, 2, stride=2)
        self.pos_embed = nn.Parameter(torch.from_numpy(sincos_pos_embed(d3, self.grids[2])).float().unsqueeze(0))
        self.blocks1 = nn.ModuleList([_CBlock(d1, d1 * mlp_ratio, conv_ln_eps) for _ in range(self.depths[0])])
        self.blocks2 = nn.ModuleList([_CBlock(d2, d2 * mlp_ratio, conv_ln_eps) for _ in range(self.depths[1])])
        self.blocks3 = nn.ModuleList([_Block(d3, d3 * mlp_ratio, ln_eps) for _ in range(self.depths[2])])
        self.norm = nn.LayerNorm(d3, eps=ln_eps)
        self._seeded_init(seed)
        self.trainable = bool(trainable)
        for p in self.parameters():
            p.requires_grad_(self.trainable)            # frozen by default, as in save_latent.py:51-53
        self.grad_ready_hook = None                     # callable(list_of_param_names) fired as gradients complete (DDP overlap)
        self._ws = None                                 # backward workspace (slabs of the fixed-order reductions)
        self._w16, self._w16_key = None, None
        self._wmx, self._wmx_key = None, None           # MXFP8 (q, s) of the product matrices, once per weight version
        self.eval()

    def _seeded_init(self, seed):
        """Weights N(0, 1/fan_in), biases 0, LayerNorm (1, 0), pos_embed the sin-cos table: deterministic per seed."""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name == "pos_embed":
                    continue
                if p.dim() == 1:
                    p.fill_(1.0 if (".norm" in name or name.startswith("norm")) and name.endswith(".weight") else 0.0)
                else:
                    p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p[0].numel()))

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """nn.Module semantics (a wrong shape raises, also under strict=False).  A full MAE checkpoint loads with no
        missing keys; its decoder (``decoder_*``, ``mask_token``) comes back as the unexpected keys."""
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._w16_key = self._wmx_key = None
        return out

    # ------------------------------------------------------------------ weights, once per weight version
    def _prepare(self, device):
        params = list(self.parameters())
        key = tuple((p.data_ptr(), p._version) for p in params)
        # trainable: rebuilt on every forward -- an optimiser that writes a flat parameter buffer through a raw pointer
        # (isic_hip.optim.AdamW) bumps neither data_ptr nor _version (ViTSmallEncoder._prepare)
        if self._w16 is not None and key == self._w16_key and not self.trainable:
            return self._w16
        self._check_device(params, device)
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        w = {}

        def mat(name, k_pad=None):
            """OIHW / [O, I] -> [O, kh * kw * I] fp16 in the row order of the patch rows ([kh][kw][c])"""
            t = sd[name].float()
            t = t.permute(0, 2, 3, 1).reshape(t.shape[0], -1) if t.dim() == 4 else t
            if k_pad is not None and k_pad > t.shape[1]:
                t = torch.nn.functional.pad(t, (0, k_pad - t.shape[1]))
            return t.to(_F16).contiguous()

        for k, v in sd.items():
            if v.dim() == 1:
                w[k] = v.float().contiguous()                    # biases, LayerNorm affine: fp32
        w["patch_embed1.proj.weight"] = mat("patch_embed1.proj.weight", 64)
        for k in ("patch_embed2.proj.weight", "patch_embed3.proj.weight", "patch_embed4.weight",
                  "stage1_output_decode.weight", "stage2_output_decode.weight"):
            w[k] = mat(k)
        w["pos_embed"] = sd["pos_embed"].reshape(self.tokens, -1).to(_F16).contiguous()
        folds = []
        for s, stage in ((0, "blocks1"), (1, "blocks2")):
            for i in range(self.depths[s]):
                b = f"{stage}.{i}"
                for lin in ("conv1", "conv2", "mlp.fc1", "mlp.fc2"):
                    w[f"{b}.{lin}.weight"] = mat(f"{b}.{lin}.weight")
                C = self.dims[s]
                w[f"{b}.attn.weight"] = sd[f"{b}.attn.weight"].float().reshape(C, 25).t().contiguous()   # [25][C] fp32
                folds += [(f"{b}.norm1", f"{b}.conv1"), (f"{b}.norm2", f"{b}.mlp.fc1")]
        for i in range(self.depths[2]):
            b = f"blocks3.{i}"
            for lin in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"):
                w[f"{b}.{lin}.weight"] = mat(f"{b}.{lin}.weight")
            folds += [(f"{b}.norm1", f"{b}.attn.qkv"), (f"{b}.norm2", f"{b}.mlp.fc1")]
        for norm, lin in (folds if self.fold_layernorm and self.precision == "fp16" else ()):
            fold_layernorm(w, sd[lin + ".weight"], norm, lin)
        self._w16, self._w16_key = w, key
        return w

    def _prepare_mx(self, device):
        """(q, s) of every product matrix but the stem's, quantised on the GPU (isic_mxfp8_quantize) from the fp32 masters
        in the row order of the patch rows ([O][kh][kw][I]: a block is 32 input channels of one kernel position)."""
        key = tuple((p.data_ptr(), p._version) for p in self.parameters())
        if self._wmx is not None and key == self._wmx_key:
            return self._wmx

        def matrices():
            for name, v in self.state_dict().items():
                if v.dim() < 2 or name in ("pos_embed", "patch_embed1.proj.weight") or name.endswith(".attn.weight"):
                    continue
                t = v.detach().float()
                yield name, (t.permute(0, 2, 3, 1).reshape(t.shape[0], -1) if t.dim() == 4 else t)
        w = mx_weights(matrices(), device)
        self._wmx, self._wmx_key = w, key
        return w

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def run_tokens(self, images, depth=None):
        """images[N,3,224,224] (fp32, normalised) on the GPU -> tokens[N, 196, 768] fp32.  ``depth`` = (blocks1, blocks2,
        blocks3) runs only the first blocks of each stage (a test of the composition)."""
        depth = self._check(images, depth)
        dev = images.device
        w = self._prepare(dev)
        wmx = self._prepare_mx(dev) if self.precision == "mxfp8" else None
        x_in = images.float().contiguous()
        N = x_in.shape[0]
        out = torch.empty((N, self.tokens, self.out_dim), device=dev, dtype=torch.float32)
        for s in range(0, N, self.max_batch):
            e = min(N, s + self.max_batch)
            if wmx is None:
                self._run_chunk(x_in[s:e], w, out[s:e], depth)
            else:
                self._run_chunk_mx(x_in[s:e], w, wmx, out[s:e], depth)
        return out

    def _run_chunk_mx(self, img, w, wmx, out, depth):
        """The ``precision="mxfp8"`` forward of one chunk (module docstring): every product but the stem's on
        ``isic_gemm_mxfp8``, its operand written as MXFP8 by the launch before it."""
        dev = img.device
        n, T, r = img.shape[0], self.tokens, self.mlp_ratio
        (d1, d2, d3), (g1, g2, g3) = self.dims, self.grids
        M2, M3 = n * g2 * g2, n * g3 * g3
        ceps, eps = self.conv_ln_eps, self.ln_eps

        def e16(*shape):
            return torch.empty(shape, device=dev, dtype=_F16)

        def mx(M, K):
            return (torch.empty((M, K), device=dev, dtype=torch.uint8), torch.empty((M, K // 32), device=dev, dtype=torch.uint8))

        def gemm(a, name, M, Nout, K, out=None, out_mx=None, act=0, res=None, res_rows=0):
            (wq, ws), (oq, os_) = wmx[name + ".weight"], out_mx or (None, None)
            call("isic_gemm_mxfp8", a[0], a[1], wq, ws, w[name + ".bias"], res, out, oq, os_, M, Nout, K, act, res_rows)
            return out

        def ln_mx(x, name, h, M, C, act, e):
            call("isic_layernorm_act_mxfp8_f16", x, w[name + ".weight"], w[name + ".bias"], h[0], h[1], M, C, act, e)

        def patch_rows(x, g, C, P):
            rows = mx(n * (g // P) ** 2, P * P * C)
            call("isic_patch_rows_mxfp8_nhwc_f16", x, rows[0], rows[1], n, g, g, C, P)
            return rows

        def cblocks(x, stage, g, C, nblk):
            M, Hd = n * g * g, C * r
            if nblk:
                h, m, hid, d, x2 = mx(M, C), mx(M, C), mx(M, Hd), e16(M, C), e16(M, C)
            for i in range(nblk):
                b = f"{stage}.{i}"
                ln_mx(x, b + ".norm1", h, M, C, 0, ceps)
                gemm(h, b + ".conv1", M, C, C, out=d)
                call("isic_dwconv5x5_mxfp8_f16", d, w[b + ".attn.weight"], w[b + ".attn.bias"], m[0], m[1], n, g, g, C)
                gemm(m, b + ".conv2", M, C, C, out=x2, res=x)
                ln_mx(x2, b + ".norm2", h, M, C, 0, ceps)
                gemm(h, b + ".mlp.fc1", M, Hd, C, out_mx=hid, act=1)
                gemm(hid, b + ".mlp.fc2", M, C, Hd, out=x, res=x2)
            return x

        def patch_embed(rows, name, M, C, K):
            t, y = gemm(rows, name + ".proj", M, C, K, out=e16(M, C)), e16(M, C)
            call("isic_layernorm_add_f16", t, None, None, w[name + ".norm.weight"], w[name + ".norm.bias"], y, None, M, C, 1, ceps)
            return y

        # ---- stage 1: the stem stays fp16 (K = 48 padded to 64 is no multiple of 128)
        x = self._stem(img, w)
        x = cblocks(x, "blocks1", g1, d1, depth[0])
        s1 = gemm(patch_rows(x, g1, d1, 4), "stage1_output_decode", M3, d3, 16 * d1, out=e16(M3, d3))
        rows = patch_rows(x, g1, d1, 2)
        del x
        # ---- stage 2
        x = cblocks(patch_embed(rows, "patch_embed2", M2, d2, 4 * d1), "blocks2", g2, d2, depth[1])
        rows = patch_rows(x, g2, d2, 2)                               # shared by the stage decoder and patch_embed3
        del x
        s2 = gemm(rows, "stage2_output_decode", M3, d3, 4 * d2, out=e16(M3, d3))
        # ---- stage 3: patch_embed3's LayerNorm + GELU feeds patch_embed4 only, so it leaves as MXFP8
        t = gemm(rows, "patch_embed3.proj", M3, d3, 4 * d2, out=e16(M3, d3))
        del rows
        h = mx(M3, d3)
        ln_mx(t, "patch_embed3.norm", h, M3, d3, 1, ceps)
        x = gemm(h, "patch_embed4", M3, d3, d3, out=t, res=w["pos_embed"], res_rows=T)
        del h
        x = blocks_forward_mx(w, wmx, x, n, depth[2], self._blocks3_spec(T), self._layernorm_mx)
        call("isic_layernorm_add_f16", x, s1, s2, w["norm.weight"], w["norm.bias"], None, out, n * T, d3, 0, eps)

    @staticmethod
    def _layernorm_mx(x, gamma, beta, q, s, M, D, eps):
        """The LayerNorm -> MXFP8 pass of blocks3 (transformer.blocks_forward_mx): no GELU"""
        call("isic_layernorm_act_mxfp8_f16", x, gamma, beta, q, s, M, D, 0, eps)

    def _stem(self, img, w, save_into=None):
        """The stem, fp16 in every precision (K = 48 padded to 64 is no multiple of 128): the 4 x 4 patch rows of the
        image, patch_embed1's product and its LayerNorm + GELU -> x[n * 56 * 56, 256].  ``save_into``: a tape that keeps
        the product's output as ``t1`` for the backward."""
        n, d1, M1 = img.shape[0], self.dims[0], img.shape[0] * self.grids[0] ** 2
        rows, t, x = (torch.empty((M1, c), device=img.device, dtype=_F16) for c in (64, d1, d1))
        call("isic_patch_rows_nchw_f32", img, rows, n, self.in_ch, self.img_size, self.img_size, 4, 64)
        call("isic_gemm_f16", rows, w["patch_embed1.proj.weight"], w["patch_embed1.proj.bias"], None, t, M1, d1, 64, 0, 0)
        call("isic_layernorm_add_f16", t, None, None, w["patch_embed1.norm.weight"], w["patch_embed1.norm.bias"], x, None, M1, d1,
             1, self.conv_ln_eps)
        if save_into is not None:
            save_into["t1"] = t
        return x

    def _run_chunk(self, img, w, out, depth):
        n, fold, spec = img.shape[0], self.fold_layernorm, self._blocks3_spec(self.tokens)
        y3, s1, s2, _ = self._front(img, w, depth, fold)
        x, st = embed(w, y3, "patch_embed4", spec, fold)
        del y3
        x, _ = blocks_forward(w, x, st, n, depth[2], spec, fold=fold)
        call("isic_layernorm_add_f16", x, s1, s2, w["norm.weight"], w["norm.bias"], None, out, n * self.tokens, self.dims[2], 0,
             self.ln_eps)

    def _front(self, img, w, depth, fold, save=False, keep=None):
        """The convolutional front: the stem rows, patch_embed1, blocks1, patch_embed2, blocks2, patch_embed3 and the two
        stage decoders -> (patch_embed3's tokens [n * 196, 768], s1, s2, tape).  ``save``: tape holds what the backward
        reads of it (the PatchEmbed convolution outputs t1-t3, the stage outputs x1 / x2, the CBlocks' activations);
        else it is empty and every activation goes once it has been read.  ``keep``: ``_cblocks``."""
        dev = img.device
        n = img.shape[0]
        (d1, d2, d3), (g1, g2, g3) = self.dims, self.grids
        M2, M3 = n * g2 * g2, n * g3 * g3
        tape = {}

        def e16(*shape):
            return torch.empty(shape, device=dev, dtype=_F16)

        def patch_embed(rows, name, M, C, K):
            t, y = e16(M, C), e16(M, C)
            call("isic_gemm_f16", rows, w[name + ".proj.weight"], w[name + ".proj.bias"], None, t, M, C, K, 0, 0)
            call("isic_layernorm_add_f16", t, None, None, w[name + ".norm.weight"], w[name + ".norm.bias"], y, None, M, C, 1,
                 self.conv_ln_eps)
            if save:
                tape["t" + name[-1]] = t
            return y

        def decode(rows, name, K):
            s = e16(M3, d3)
            call("isic_gemm_f16", rows, w[name + ".weight"], w[name + ".bias"], None, s, M3, d3, K, 0, 0)
            return s

        # ---- stage 1: 56 x 56 x 256
        x = self._stem(img, w, tape if save else None)
        x, blocks1 = self._cblocks(x, w, "blocks1", n, g1, d1, depth[0], fold, save, keep)
        rows = e16(M3, 16 * d1)
        call("isic_patch_rows_nhwc_f16", x, rows, n, g1, g1, d1, 4)
        s1 = decode(rows, "stage1_output_decode", 16 * d1)
        rows = e16(M2, 4 * d1)
        call("isic_patch_rows_nhwc_f16", x, rows, n, g1, g1, d1, 2)
        if save:
            tape.update(blocks1=blocks1, x1=x)
        del x
        # ---- stage 2: 28 x 28 x 384
        x = patch_embed(rows, "patch_embed2", M2, d2, 4 * d1)
        del rows
        x, blocks2 = self._cblocks(x, w, "blocks2", n, g2, d2, depth[1], fold, save, keep)
        rows = e16(M3, 4 * d2)
        call("isic_patch_rows_nhwc_f16", x, rows, n, g2, g2, d2, 2)
        if save:
            tape.update(blocks2=blocks2, x2=x)
        del x
        s2 = decode(rows, "stage2_output_decode", 4 * d2)
        # ---- stage 3: 196 tokens x 768
        return patch_embed(rows, "patch_embed3", M3, d3, 4 * d2), s1, s2, tape

    def _cblocks(self, x, w, stage, n, g, C, nblk, fold, save=False, keep=None):
        """``nblk`` CBlocks over the NHWC stream x[n*g*g, C] -> (the output stream, the saved activations per block).
        ``fold`` / ``save`` as in ``transformer.blocks_forward``: without ``save`` x is updated in place and every block
        reuses one set of buffers.  ``keep`` (uint8 [n, 196], the MAE's token flags; None: no masking) masks the depthwise
        5x5's input per token."""
        if save and fold:
            raise ValueError("_cblocks: save=True runs the layer-by-layer form (fold=False)")
        dev = x.device
        M, Hd, eps = n * g * g, C * self.mlp_ratio, self.conv_ln_eps
        parts = 2 * C // 128
        st = st2 = None
        if fold and nblk:
            st = torch.empty((M, parts, 2), device=dev, dtype=torch.float32)
            st2 = torch.empty_like(st)
            call("isic_row_stats_f16", x, st, M, C, eps)      # (mean, rstd) of the PatchEmbed output: block 0 reads 0 parts

        def e16(cols):
            return torch.empty((M, cols), device=dev, dtype=_F16)

        saves = []
        for i in range(nblk):
            b = f"{stage}.{i}"
            if save or i == 0:
                h1, dd, x2, hid = e16(C), e16(C), e16(C), e16(Hd)
            m, h2, pre, xo = (e16(C), e16(C), e16(Hd), e16(C)) if save else (h1, h1, None, x)
            linear_ln(w, x, st, parts if i else 0, b + ".norm1", b + ".conv1", h1, dd, 0, eps)
            if keep is None:
                call("isic_dwconv5x5_f16", dd, w[b + ".attn.weight"], w[b + ".attn.bias"], m, n, g, g, C)
            else:                                       # saved: keep * dd, the input the weight gradient takes
                dk = torch.empty_like(dd)
                call("isic_dwconv5x5_masked_f16", dd, keep, g // self.grids[2], w[b + ".attn.weight"], w[b + ".attn.bias"],
                     dk, m, n, g, g, C)
                dd = dk
            linear_res(w, m, b + ".conv2", x, x2, st2, fold, eps)
            linear_ln(w, x2, st2, parts, b + ".norm2", b + ".mlp.fc1", h2, hid, 1, eps, pre=pre)
            linear_res(w, hid, b + ".mlp.fc2", x2, xo, st, fold, eps)
            if save:
                saves.append(dict(x=x, h1=h1, d=dd, m=m, x2=x2, h2=h2, pre=pre, hid=hid))
            x = xo
        return x, saves

    def forward_tokens(self, images, depth=None):
        """tokens[N, 196, 768] fp32; differentiable (``transformer.EncoderFn``) when the encoder is trainable and grad is enabled."""
        if self.trainable and torch.is_grad_enabled():
            return EncoderFn.apply(images, self, (depth,), *self.parameters())
        return self.run_tokens(images, depth=depth)

    def forward(self, images):
        """Mean-pooled 768-d feature per image (what a MIL bag of patches consumes)."""
        return self.forward_tokens(images).mean(dim=1)

    # ------------------------------------------------------------------ training (trainable=True)
    def _check(self, images, depth):
        self._check_images(images)
        depth = tuple(self.depths) if depth is None else tuple(depth)
        if len(depth) != 3 or any(not 0 <= d <= m for d, m in zip(depth, self.depths)):
            raise ValueError(f"depth: three block counts within {self.depths}")
        return depth

    def _prepare_train(self, device):
        """fp16 matrices for the forward, their transposes for the data gradients and the depthwise taps reversed."""
        w = self._prepare(device)
        for k in [k for k, v in w.items() if k.endswith(".weight") and v.dtype == _F16 and k != "patch_embed1.proj.weight"]:
            w[k + ".t"] = w[k].t().contiguous()
        for s, stage in ((0, "blocks1"), (1, "blocks2")):
            for i in range(self.depths[s]):
                w[f"{stage}.{i}.attn.weight.rev"] = w[f"{stage}.{i}.attn.weight"].flip(0).contiguous()
        return w

    def run_forward_train(self, images, depth=None, masking=None):
        """The layer-by-layer forward (bitwise ``run_tokens`` with fold_layernorm=False) that keeps what the backward needs.
        ``masking`` (the MAE, isic_hip/convmae_mae.py): dict(keep, ids_keep, ids_restore, L) -> the latent of the L kept
        tokens per image in ids_keep order (and its fp16 copy as tape["latent16"])."""
        depth = self._check(images, depth)
        dev = images.device
        w = self._prepare_train(dev)
        img = images.float().contiguous()
        n, d3 = img.shape[0], self.dims[2]
        keep, L = (masking["keep"], masking["L"]) if masking is not None else (None, self.tokens)
        y3, s1, s2, tape = self._front(img, w, depth, False, save=True, keep=keep)
        tape.update(n=n, img=img, depth=depth, w=w)
        x, _ = embed(w, y3, "patch_embed4", self._blocks3_spec(L), False)
        lat16 = None
        if masking is not None:                                            # the kept tokens of the stream, s1 and s2
            tape.update(keep=keep, ids_restore=masking["ids_restore"], L=L)
            xk, s1k, s2k, lat16 = (torch.empty((n * L, d3), device=dev, dtype=_F16) for _ in range(4))
            for a, b in ((x, xk), (s1, s1k), (s2, s2k)):
                call("isic_gather_rows_f16", a, masking["ids_keep"], b, n, self.tokens, L, d3)
            x, s1, s2 = xk, s1k, s2k
        x, tape["blocks3"] = blocks_forward(w, x, None, n, depth[2], self._blocks3_spec(L), save=True)
        out = torch.empty((n * L, d3), device=dev, dtype=torch.float32)
        call("isic_layernorm_add_f16", x, s1, s2, w["norm.weight"], w["norm.bias"], lat16, out, n * L, d3, 0, self.ln_eps)
        tape.update(y3=y3, x3=x, s1=s1, s2=s2, latent16=lat16)
        return out.view(n, L, d3), tape

    def _blocks3_spec(self, T):
        """blocks3 over T tokens per image, as isic_hip/transformer.py describes a stack of blocks."""
        return dict(prefix="blocks3", T=T, D=self.dims[2], H=self.heads, eps=self.ln_eps, total=self.depths[2])

    def _fire(self, names):
        if self.grad_ready_hook is not None:
            self.grad_ready_hook(list(names))

    def _block_names(self, prefix):
        return [prefix + "." + k for k, _ in self.get_submodule(prefix).named_parameters()]

    def run_backward(self, tape, dtok):
        """Accumulates every parameter gradient into ``param.grad`` from d loss / d tokens[N, 196, 768].

        ``grad_ready_hook`` fires with ``norm``, then each ViT block and each CBlock from the last back, then one group
        with the PatchEmbeds, the stage decoders and ``pos_embed``: their gradients are final earlier, but they sit in
        front of the blocks in registration order, and a group may only be reported once everything registered after it
        is final (isic_hip/ddp.py ``mark_ready``)."""
        dtok, S = loss_scale(dtok, type(self).__name__)   # the backward's one device -> host read before its final check
        bw = Backward(self, tape["w"], param_grads(self), 1.0 / S, self._encoder_workspace_bytes(tape), dtok.device)
        self._encoder_backward(tape, dtok, 1, S, bw)
        check_grads(self.parameters(), type(self).__name__)

    def _encoder_workspace_bytes(self, tape):
        """The slabs of the largest reduction of ``_encoder_backward``."""
        w, n = tape["w"], tape["n"]
        (d1, d2, d3), (g1, g2, g3) = self.dims, self.grids
        M1, M2, M3 = n * g1 * g1, n * g2 * g2, n * g3 * g3
        T, r = self.tokens, self.mlp_ratio
        nb = blocks_workspace_bytes(w, n, self._blocks3_spec(tape.get("L", T)))
        for M, C in ((M1, d1), (M2, d2)):
            for nk in ((C, C), (r * C, C), (C, r * C)):
                nb = max(nb, call("isic_gemm_f16_wgrad_workspace_bytes", M, *nk))
            nb = max(nb, call("isic_layernorm_add_bwd_f16_workspace_bytes", M, C), call("isic_colsum_f16_workspace_bytes", M, C))
        for M, nk in ((M3, (d3, 16 * d1)), (M3, (d3, 4 * d2)), (M2, (d2, 4 * d1)), (M1, (d1, 128)), (M3, (d3, d3))):
            nb = max(nb, call("isic_gemm_f16_wgrad_workspace_bytes", M, *nk))
        return max(nb, call("isic_layernorm_add_bwd_f16_workspace_bytes", M3, d3), call("isic_colsum_f16_workspace_bytes", M3, d3),
                   call("isic_colsum_f16_workspace_bytes", n, T * d3),
                   call("isic_dwconv5x5_wgrad_f16_workspace_bytes", n, g1, g1, d1),
                   call("isic_dwconv5x5_wgrad_f16_workspace_bytes", n, g2, g2, d2))

    def _encoder_backward(self, tape, dy, dy_is_f32, dy_mul, bw):
        """The encoder's backward from dy = d loss / d latent (times dy_mul: then the power-of-two scale S), every
        parameter-gradient reduction multiplied by ``bw.s`` (transformer.Backward).  With ``tape["ids_restore"]`` (the MAE's
        masked forward) the latent and blocks3 hold the kept tokens only: their gradients are scattered back onto the
        196-token grid (zeros at the removed tokens) for the stage decoders and patch_embed4, and the CBlocks take the
        masked depthwise gradient."""
        w, n, depth = tape["w"], tape["n"], tape["depth"]
        (d1, d2, d3), (g1, g2, g3) = self.dims, self.grids
        M1, M2, M3 = n * g1 * g1, n * g2 * g2, n * g3 * g3
        T, ceps = self.tokens, self.conv_ln_eps
        ids_restore, keep = tape.get("ids_restore"), tape.get("keep")
        L = tape.get("L", T)
        Mk = n * L
        dev = dy.device
        grad, wgrad, ln_add, ws, s = bw.grad, bw.wgrad, bw.ln_add, bw.ws, bw.s
        f32 = torch.float32

        def e16(*shape):
            return torch.empty(shape, device=dev, dtype=_F16)

        def wgrad_conv(dy, xin, name, Nout, K, M, P, Cin, keep=None):
            """a P x P patch convolution: the [O][kh][kw][I] gradient of the rows, permuted to the OIHW weight"""
            tmp = torch.empty((Nout, K), device=dev, dtype=f32)
            call("isic_gemm_f16_wgrad", dy, xin, tmp, None, M, Nout, K, s, 0, ws, ws.numel())
            tmp = tmp[:, :keep] if keep is not None else tmp
            grad(name + ".weight").add_(tmp.reshape(Nout, P, P, Cin).permute(0, 3, 1, 2))
            bw.colsum(dy, name + ".bias", M, Nout)

        rest = []
        # ---- norm(x + s1 + s2): one gradient g3 for the stream and both stage decoders
        g3, g3h = torch.empty((Mk, d3), device=dev, dtype=f32), e16(Mk, d3)
        ln_add(dy, dy_is_f32, dy_mul, tape["x3"], tape["s1"], tape["s2"], "norm", 0, self.ln_eps, None, g3, g3h, Mk, d3)
        self._fire(["norm.weight", "norm.bias"])
        gfull = g3h
        if ids_restore is not None:                                         # the kept rows back onto the token grid
            gfull = e16(M3, d3)
            call("isic_scatter_rows_f16", g3h, ids_restore, gfull, n, T, L, d3)
        # ---- stage decoders: s = rows . W^T + b, rows the space-to-depth of the stage output
        rows2 = e16(M3, 4 * d2)                                             # also the input rows of patch_embed3
        call("isic_patch_rows_nhwc_f16", tape["x2"], rows2, n, g2, g2, d2, 2)
        wgrad_conv(gfull, rows2, "stage2_output_decode", d3, 4 * d2, M3, 2, d2)
        dr2 = e16(M3, 4 * d2)
        call("isic_gemm_f16", gfull, w["stage2_output_decode.weight.t"], None, None, dr2, M3, 4 * d2, d3, 0, 0)
        gs2, gs2h = torch.empty((M2, d2), device=dev, dtype=f32), e16(M2, d2)
        call("isic_patch_rows_bwd_f16", dr2, gs2, None, n, g2, g2, d2, 2, 0)
        rows = e16(M3, 16 * d1)
        call("isic_patch_rows_nhwc_f16", tape["x1"], rows, n, g1, g1, d1, 4)
        wgrad_conv(gfull, rows, "stage1_output_decode", d3, 16 * d1, M3, 4, d1)
        call("isic_gemm_f16", gfull, w["stage1_output_decode.weight.t"], None, None, rows, M3, 16 * d1, d3, 0, 0)
        gs1, gs1h = torch.empty((M1, d1), device=dev, dtype=f32), e16(M1, d1)
        call("isic_patch_rows_bwd_f16", rows, gs1, None, n, g1, g1, d1, 4, 0)
        del rows
        rest += self._block_names("stage2_output_decode") + self._block_names("stage1_output_decode")
        # ---- blocks3, patch_embed4 + pos_embed
        blocks_backward(tape["blocks3"], g3, g3h, bw, n, depth[2], self._blocks3_spec(L), self._fire)
        if ids_restore is not None:
            call("isic_scatter_rows_f16", g3h, ids_restore, gfull, n, T, L, d3)
            g3h = gfull
        wgrad(g3h, tape["y3"], "patch_embed4", d3, d3, M3)
        bw.colsum(g3h, "pos_embed", n, T * d3)
        dt3 = e16(M3, d3)
        call("isic_gemm_f16", g3h, w["patch_embed4.weight.t"], None, None, dt3, M3, d3, d3, 0, 0)
        rest += self._block_names("patch_embed4") + ["pos_embed"]
        # ---- patch_embed3: conv -> LN -> GELU; its data gradient joins the stage-2 stream gradient
        ln_add(dt3, 0, 1.0, tape["t3"], None, None, "patch_embed3.norm", 1, ceps, None, None, g3h, M3, d3)
        wgrad_conv(g3h, rows2, "patch_embed3.proj", d3, 4 * d2, M3, 2, d2)
        call("isic_gemm_f16", g3h, w["patch_embed3.proj.weight.t"], None, None, dr2, M3, 4 * d2, d3, 0, 0)
        call("isic_patch_rows_bwd_f16", dr2, gs2, gs2h, n, g2, g2, d2, 2, 1)
        del rows2, dr2, dt3, g3, g3h, gfull
        rest += self._block_names("patch_embed3")
        # ---- blocks2, patch_embed2
        self._cblocks_backward(tape, "blocks2", gs2, gs2h, bw, n, g2, d2, depth[1], keep)
        ln_add(gs2, 1, 1.0, tape["t2"], None, None, "patch_embed2.norm", 1, ceps, None, None, gs2h, M2, d2)
        rows = e16(M2, 4 * d1)
        call("isic_patch_rows_nhwc_f16", tape["x1"], rows, n, g1, g1, d1, 2)
        wgrad_conv(gs2h, rows, "patch_embed2.proj", d2, 4 * d1, M2, 2, d1)
        call("isic_gemm_f16", gs2h, w["patch_embed2.proj.weight.t"], None, None, rows, M2, 4 * d1, d2, 0, 0)
        call("isic_patch_rows_bwd_f16", rows, gs1, gs1h, n, g1, g1, d1, 2, 1)
        del rows, gs2, gs2h
        rest += self._block_names("patch_embed2")
        # ---- blocks1, the stem (no data gradient; its rows are padded to K = 128 for the weight-gradient GEMM)
        self._cblocks_backward(tape, "blocks1", gs1, gs1h, bw, n, g1, d1, depth[0], keep)
        ln_add(gs1, 1, 1.0, tape["t1"], None, None, "patch_embed1.norm", 1, ceps, None, None, gs1h, M1, d1)
        rows = e16(M1, 128)
        call("isic_patch_rows_nchw_f32", tape["img"], rows, n, self.in_ch, self.img_size, self.img_size, 4, 128)
        wgrad_conv(gs1h, rows, "patch_embed1.proj", d1, 128, M1, 4, self.in_ch, keep=16 * self.in_ch)
        rest += self._block_names("patch_embed1")
        self._fire(rest)

    def _cblocks_backward(self, tape, stage, g, gh, bw, n, gr, C, nblk, keep=None):
        w, dev = tape["w"], g.device
        grad, wgrad, ln_add, ws, s = bw.grad, bw.wgrad, bw.ln_add, bw.ws, bw.s
        M, Hd, eps = n * gr * gr, C * self.mlp_ratio, self.conv_ln_eps
        dmid = torch.empty((M, Hd), device=dev, dtype=_F16)
        dD, dm, dd = (torch.empty((M, C), device=dev, dtype=_F16) for _ in range(3))
        dw, db = torch.empty((25, C), device=dev, dtype=torch.float32), torch.empty(C, device=dev, dtype=torch.float32)
        s_idx = 0 if stage == "blocks1" else 1
        for i in range(self.depths[s_idx] - 1, nblk - 1, -1):
            self._fire(self._block_names(f"{stage}.{i}"))
        for i in range(nblk - 1, -1, -1):
            b, sv = f"{stage}.{i}", tape[stage][i]
            wgrad(gh, sv["hid"], f"{b}.mlp.fc2", C, Hd, M)
            call("isic_gemm_f16_dgelu", gh, w[f"{b}.mlp.fc2.weight.t"], sv["pre"], dmid, M, Hd, C)
            wgrad(dmid, sv["h2"], f"{b}.mlp.fc1", Hd, C, M)
            call("isic_gemm_f16", dmid, w[f"{b}.mlp.fc1.weight.t"], None, None, dD, M, C, Hd, 0, 0)
            ln_add(dD, 0, 1.0, sv["x2"], None, None, f"{b}.norm2", 0, eps, g, g, gh, M, C)
            wgrad(gh, sv["m"], f"{b}.conv2", C, C, M)
            call("isic_gemm_f16", gh, w[f"{b}.conv2.weight.t"], None, None, dm, M, C, C, 0, 0)
            # depthwise 5x5: data gradient = the same convolution with the taps reversed, no bias; weight + bias gradient
            if keep is None:
                call("isic_dwconv5x5_f16", dm, w[f"{b}.attn.weight.rev"], None, dd, n, gr, gr, C)
            else:                                                           # its input was keep * d: so is its gradient
                call("isic_dwconv5x5_masked_dgrad_f16", dm, keep, gr // self.grids[2], w[f"{b}.attn.weight.rev"], dd, n, gr,
                     gr, C)
            call("isic_dwconv5x5_wgrad_f16", sv["d"], dm, dw, db, n, gr, gr, C, s, 0, ws, ws.numel())
            grad(f"{b}.attn.weight").add_(dw.t().reshape(C, 1, 5, 5))
            grad(f"{b}.attn.bias").add_(db)
            wgrad(dd, sv["h1"], f"{b}.conv1", C, C, M)
            call("isic_gemm_f16", dd, w[f"{b}.conv1.weight.t"], None, None, dD, M, C, C, 0, 0)
            ln_add(dD, 0, 1.0, sv["x"], None, None, f"{b}.norm1", 0, eps, g, g, gh, M, C)
            tape[stage][i] = None
            self._fire(self._block_names(b))

    def train_flops_per_image(self):
        """Forward + backward products: every product and convolution three times, except the stem's data gradient."""
        return 3 * self.flops_per_image() - 2 * self.grids[0] ** 2 * self.dims[0] * self.in_ch * 16

    def flops_per_image(self):
        """Multiply-adds x 2 of every product and convolution (the stem at its 48 real columns, not the padded 64)."""
        (d1, d2, d3), (g1, g2, g3) = self.dims, self.grids
        r = self.mlp_ratio
        f = 2 * g1 * g1 * d1 * self.in_ch * 16                                        # patch_embed1
        f += self.depths[0] * 2 * g1 * g1 * (2 * d1 * d1 + 25 * d1 + 2 * r * d1 * d1)  # blocks1
        f += 2 * g3 * g3 * d3 * 16 * d1                                               # stage1_output_decode
        f += 2 * g2 * g2 * d2 * 4 * d1                                                # patch_embed2
        f += self.depths[1] * 2 * g2 * g2 * (2 * d2 * d2 + 25 * d2 + 2 * r * d2 * d2)  # blocks2
        f += 2 * 2 * g3 * g3 * d3 * 4 * d2                                            # stage2_output_decode, patch_embed3
        T = g3 * g3
        f += 2 * T * d3 * d3                                                           # patch_embed4
        f += self.depths[2] * (2 * T * (4 * d3 * d3 + 2 * r * d3 * d3) + 4 * T * T * d3)   # blocks3
        return f

