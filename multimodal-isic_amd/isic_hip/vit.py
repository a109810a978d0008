"""ViT-S/16 patch encoder, fp16 on MFMA -- the frozen encoder of BASELINE.json configs[4].

The reference's patch encoder is an un-vendored ConvMAE conv-ViT run frozen: ``model.eval()``, ``torch.no_grad()``,
``forward(images, mask_ratio=0) -> latent[B, 196, 768]`` (`save_latent.py:42-60`).  Its code and weights are not in the
tree, so this is the build's own ViT-S/16 (timm `vit_small_patch16_224` parameter names, no class token: the reference
consumes the 196 patch tokens only, `save_latent.py:56-60,77`).  Inference only, like the reference's use of it.

Every layer is one launch of the C ABI: `isic_vit_patchify_f16`, `isic_gemm_f16` (bias, GELU, residual / position
embedding fused into the epilogue), `isic_layernorm_f16`, `isic_attention_f16`.  The residual stream and all
activations are fp16 in HBM ([N*196, 384] rows), arithmetic is fp32 inside the kernels.  No CPU fallback.

``fold_layernorm`` (default True, round 3): the two pre-norm LayerNorms of a block have no pass of their own.  With
W' = W diag(gamma), c = W' 1, b' = b + W beta:   LN(x) W^T + b = rstd (x W'^T - mean c) + b'   -- the product reads the RAW
residual stream (`isic_gemm_f16_ln`) and applies the row's (mean, rstd) in its epilogue; the row sums those need come
out of the epilogue of the product that WROTE the stream (`isic_gemm_f16_stats`: patch projection, attn.proj, mlp.fc2).
``"stats"`` keeps a statistics-only pass (`isic_row_stats_f16`, the LayerNorm kernel's two-pass text) in place of the epilogue
sums; ``False`` is the layer-by-layer form above.

``precision="mxfp8"`` (opt-in; the default ``"fp16"`` is the path above, unchanged): the four products of every block run
on the block-scaled FP8 MFMA (`isic_gemm_mxfp8`, OCP MX E4M3 with one E8M0 scale per 32 elements along K, csrc/mxfp8.hip).
Per block (``transformer.blocks_forward_mx``): LayerNorm quantised straight from fp32 (`isic_layernorm_mxfp8_f16`) -> qkv
(fp16 out) -> `isic_attention_f16`
-> `isic_mxfp8_quantize` -> proj (+ residual, fp16 out) -> LayerNorm -> fc1 + GELU (MXFP8 out: the 1536-wide hidden
activation crosses HBM as 1 byte + 1/32 scale byte per value) -> fc2 (+ residual, fp16 out).  The patch projection
(raw pixels, 1.3 % of the FLOPs), the attention and the final LayerNorm stay fp16, and so does the residual stream.  The
LayerNorm is never folded into the product here: the fold multiplies the RAW stream and subtracts mean * c afterwards, and
with 3 mantissa bits that cancellation loses the signal of rows with a large offset.  Weights are quantised from the fp32
masters once per weight version.

``trainable=True`` (opt-in; the default stays the frozen encoder above, bit for bit): the parameters require grad,
``train()`` works, and the encoder runs the layer-by-layer form (``fold_layernorm=False``).  Under grad, ``forward`` /
``forward_tokens`` go through ``transformer.EncoderFn``: patchify, the patch projection (+ pos_embed), then the block
stack and its backward of isic_hip/transformer.py, which the ConvMAE encoders share.  The forward saves its activations
(about 12 KB per token per block: x, LN1(x), qkv, the attention output, x2, LN2(x2), fc1's pre-activation and GELU
output, fp16; no LayerNorm statistics -- the backward recomputes them from x) and the native backward
(include/isic_hip_vit_train.h, ``isic_layernorm_add_bwd_f16``) accumulates into ``param.grad``.  The backward runs in
fp16 with a power-of-two loss scale S = 2^round(8 - log2 amax(d tokens)), one device -> host read per call; every
reduction into a parameter gradient multiplies by 1/S in fp32, so gradients are exactly scale-equivariant.  An fp16
overflow is not retried: it reaches the gradients as inf / NaN, and the backward checks them once at its end and raises
``FloatingPointError``.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from .lib import call
from .transformer import (Backward, Encoder, EncoderFn, blocks_backward, blocks_forward, blocks_forward_mx,
                          blocks_workspace_bytes, check_grads, embed, fold_layernorm, loss_scale, mx_weights, param_grads)

_F16 = torch.float16


class ViTSmallEncoder(Encoder):
    _who = "ViTSmallEncoder"

    def __init__(self, img_size=224, patch=16, in_ch=3, dim=384, depth=12, heads=6, mlp_ratio=4, seed=0,
                 fold_layernorm=None, precision="fp16", trainable=False):
        super().__init__()
        if trainable and precision != "fp16":
            raise ValueError("trainable=True: fp16 only (no MXFP8 or bf16 training)")
        if trainable and fold_layernorm not in (None, False):
            raise ValueError("trainable=True runs the layer-by-layer form: leave fold_layernorm unset (or False)")
        if fold_layernorm is None:
            fold_layernorm = not trainable
        if fold_layernorm not in (True, False, "stats"):
            raise ValueError("fold_layernorm: True, False or 'stats'")
        if precision not in ("fp16", "mxfp8"):
            raise ValueError("precision: 'fp16' or 'mxfp8'")
        if precision == "mxfp8" and fold_layernorm is not True:
            raise ValueError("precision='mxfp8' runs its LayerNorms as passes of their own: leave fold_layernorm at its default")
        if precision == "mxfp8" and dim != 384:
            raise ValueError("precision='mxfp8': dim 384 only (isic_layernorm_mxfp8_f16)")
        self.fold_layernorm = fold_layernorm
        self.precision = precision
        if dim % 128 != 0 or dim // heads != 64 or patch % 8 != 0 or img_size % patch != 0:
            raise ValueError("ViTSmallEncoder: dim % 128 == 0, head width 64, patch % 8 == 0, img_size % patch == 0")
        self.img_size, self.patch, self.in_ch, self.dim, self.depth, self.heads = img_size, patch, in_ch, dim, depth, heads
        self.mlp = dim * mlp_ratio
        self.tokens = (img_size // patch) ** 2
        if self.tokens > 208:
            raise ValueError("ViTSmallEncoder: at most 208 tokens per image (attention kernel)")
        self.feature_dim = self.out_dim = dim
        g = torch.Generator().manual_seed(seed)

        def P(*shape, scale):
            return nn.Parameter(torch.randn(*shape, generator=g) * scale)
        self._names = []

        def add(name, param):
            self._names.append(name)
            self.register_parameter(name.replace(".", "__"), param)
        add("patch_embed.proj.weight", P(dim, in_ch, patch, patch, scale=1.0 / math.sqrt(in_ch * patch * patch)))
        add("patch_embed.proj.bias", nn.Parameter(torch.zeros(dim)))
        add("pos_embed", P(1, self.tokens, dim, scale=0.02))
        for i in range(depth):
            b = f"blocks.{i}"
            add(f"{b}.norm1.weight", nn.Parameter(torch.ones(dim))); add(f"{b}.norm1.bias", nn.Parameter(torch.zeros(dim)))
            add(f"{b}.attn.qkv.weight", P(3 * dim, dim, scale=0.02)); add(f"{b}.attn.qkv.bias", nn.Parameter(torch.zeros(3 * dim)))
            add(f"{b}.attn.proj.weight", P(dim, dim, scale=0.02)); add(f"{b}.attn.proj.bias", nn.Parameter(torch.zeros(dim)))
            add(f"{b}.norm2.weight", nn.Parameter(torch.ones(dim))); add(f"{b}.norm2.bias", nn.Parameter(torch.zeros(dim)))
            add(f"{b}.mlp.fc1.weight", P(self.mlp, dim, scale=0.02)); add(f"{b}.mlp.fc1.bias", nn.Parameter(torch.zeros(self.mlp)))
            add(f"{b}.mlp.fc2.weight", P(dim, self.mlp, scale=0.02)); add(f"{b}.mlp.fc2.bias", nn.Parameter(torch.zeros(dim)))
        add("norm.weight", nn.Parameter(torch.ones(dim))); add("norm.bias", nn.Parameter(torch.zeros(dim)))
        self.trainable = bool(trainable)
        for p in self.parameters():
            p.requires_grad_(self.trainable)           # frozen by default, as in save_latent.py:51-53
        self.grad_ready_hook = None                    # callable(list_of_param_names) fired as gradients complete (DDP overlap)
        self._ws = None                                # backward workspace (slabs of the fixed-order reductions)
        self._w16 = None                               # fp16 copies of the matrices, made once per weight version
        self._w16_key = None
        self._wmx = None                               # MXFP8 (q, s) of the block matrices, made once per weight version
        self._wmx_key = None
        self.eval()

    # ------------------------------------------------------------------ timm-named state_dict
    def _get(self, name):
        return self._parameters[name.replace(".", "__")]

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = destination if destination is not None else {}
        for n in self._names:
            p = self._get(n)
            out[prefix + n] = p if keep_vars else p.detach()
        return out

    def load_state_dict(self, state_dict, strict=True, assign=False):
        # a timm vit_small_patch16_224 checkpoint carries a class token: ``cls_token`` [1,1,D] and a ``pos_embed`` of
        # tokens + 1 rows whose row 0 is the class token's position.  This encoder has no class token (the reference
        # keeps the 196 patch latents, `save_latent.py:60`): row 0 is dropped and ``cls_token`` ignored.
        state_dict = dict(state_dict)
        state_dict.pop("cls_token", None)
        pe = state_dict.get("pos_embed")
        if pe is not None and pe.dim() == 3 and pe.shape[1] == self.tokens + 1:
            state_dict["pos_embed"] = pe[:, 1:, :]
        missing = [n for n in self._names if n not in state_dict]
        unexpected = [k for k in state_dict if k not in self._names]
        if strict and (missing or unexpected):
            raise RuntimeError(f"ViTSmallEncoder.load_state_dict: missing {missing[:4]}, unexpected {unexpected[:4]}")
        with torch.no_grad():
            for n in self._names:
                if n in state_dict:
                    src = state_dict[n]
                    dst = self._get(n)
                    if tuple(src.shape) != tuple(dst.shape):
                        raise RuntimeError(f"size mismatch for {n}: {tuple(src.shape)} vs {tuple(dst.shape)}")
                    dst.copy_(src)
        self._w16_key = None
        self._wmx_key = None
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    # ------------------------------------------------------------------ forward
    def _prepare(self, device):
        key = tuple((self._get(n).data_ptr(), self._get(n)._version) for n in self._names)
        # trainable: rebuilt on every forward -- an optimiser that writes a flat parameter buffer through a raw pointer
        # (isic_hip.optim.AdamW) bumps neither data_ptr nor _version (ResNet18Encoder.prepare_weights)
        if self._w16 is not None and key == self._w16_key and not self.trainable:
            return self._w16
        self._check_device(self.parameters(), device)
        w = {}
        for n in self._names:
            p = self._get(n).detach()
            if n == "patch_embed.proj.weight":
                w[n] = p.reshape(self.dim, -1).to(_F16).contiguous()
            elif n == "pos_embed":
                w[n] = p.reshape(self.tokens, self.dim).to(_F16).contiguous()
            elif n.endswith(".weight") and p.dim() == 2:
                w[n] = p.to(_F16).contiguous()
            else:
                w[n] = p.float().contiguous()                                      # biases, LayerNorm affine: fp32
        for i in range(self.depth if self.fold_layernorm is not False else 0):      # module docstring
            for norm, lin in ((f"blocks.{i}.norm1", f"blocks.{i}.attn.qkv"), (f"blocks.{i}.norm2", f"blocks.{i}.mlp.fc1")):
                fold_layernorm(w, self._get(lin + ".weight").detach(), norm, lin)
        self._w16, self._w16_key = w, key
        return w

    def _prepare_mx(self, device):
        """(q, s) of every block matrix, quantised on the GPU from the fp32 masters (isic_mxfp8_quantize)."""
        key = tuple((self._get(n).data_ptr(), self._get(n)._version) for n in self._names)
        if self._wmx is not None and key == self._wmx_key:
            return self._wmx
        names = [f"blocks.{i}.{lin}.weight" for i in range(self.depth) for lin in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")]
        w = mx_weights(((n, self._get(n)) for n in names), device)
        self._wmx, self._wmx_key = w, key
        return w

    def _patch_stream(self, images, w, fold):
        """patchify and the patch projection (+ pos_embed) -> (the residual stream x[N * 196, 384] fp16, its row statistics
        as ``fold`` has them (transformer.embed), the patch rows: the backward's input, else to be dropped)."""
        x_in = images.float().contiguous()
        rows = torch.empty((x_in.shape[0] * self.tokens, self.in_ch * self.patch * self.patch), device=x_in.device, dtype=_F16)
        call("isic_vit_patchify_f16", x_in, rows, x_in.shape[0], self.in_ch, self.img_size, self.img_size, self.patch)
        return embed(w, rows, "patch_embed.proj", self._spec(), fold) + (rows,)

    def _final_norm(self, x, w, N):
        out = torch.empty((N * self.tokens, self.dim), device=x.device, dtype=torch.float32)
        call("isic_layernorm_f16", x, w["norm.weight"], w["norm.bias"], None, out, N * self.tokens, self.dim, 1e-6)
        return out.view(N, self.tokens, self.dim)

    @torch.no_grad()
    def run_tokens(self, images, depth=None):
        """images[N,3,H,W] (fp32; other float types are converted) on the GPU -> tokens[N, 196, 384] fp32."""
        self._check_images(images)
        w = self._prepare(images.device)
        if self.precision == "mxfp8":
            return self._run_tokens_mx(images, w, self._prepare_mx(images.device), depth)
        fold, N = self.fold_layernorm, images.shape[0]
        x, st, rows = self._patch_stream(images, w, fold)
        del rows
        x, _ = blocks_forward(w, x, st, N, self.depth if depth is None else depth, self._spec(), fold=fold,
                              layernorm=self._layernorm)
        return self._final_norm(x, w, N)

    def _run_tokens_mx(self, images, w, wmx, depth):
        N = images.shape[0]
        x, _, rows = self._patch_stream(images, w, False)
        del rows
        x = blocks_forward_mx(w, wmx, x, N, self.depth if depth is None else depth, self._spec(), self._layernorm_mx)
        return self._final_norm(x, w, N)

    def forward_tokens(self, images):
        """tokens[N, 196, 384] fp32; differentiable (``transformer.EncoderFn``) when the encoder is trainable and grad is enabled."""
        if self.trainable and torch.is_grad_enabled():
            return EncoderFn.apply(images, self, (), *self.parameters())
        return self.run_tokens(images)

    def forward(self, images):
        """Mean-pooled 384-d feature per image (what a MIL bag of patches consumes)."""
        return self.forward_tokens(images).mean(dim=1)

    # ------------------------------------------------------------------ training (trainable=True)
    def _prepare_train(self, device):
        """fp16 matrices for the forward and their transposes for the data gradients, from the current masters."""
        w = self._prepare(device)
        for i in range(self.depth):
            for lin in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2"):
                n = f"blocks.{i}.{lin}.weight"
                w[n + ".t"] = w[n].t().contiguous()
        return w

    def _fire(self, names):
        if self.grad_ready_hook is not None:
            self.grad_ready_hook([n.replace(".", "__") for n in names])

    def _spec(self):
        """The blocks as isic_hip/transformer.py describes a stack of them."""
        return dict(prefix="blocks", T=self.tokens, D=self.dim, H=self.heads, eps=1e-6, total=self.depth)

    @staticmethod
    def _layernorm(x, gamma, beta, y, M, D, eps):
        """The LayerNorm pass of this encoder's blocks (isic_hip/transformer.py explains why it is handed in)."""
        call("isic_layernorm_f16", x, gamma, beta, y, None, M, D, eps)

    @staticmethod
    def _layernorm_mx(x, gamma, beta, q, s, M, D, eps):
        """The LayerNorm -> MXFP8 pass of this encoder's blocks: ``_layernorm``'s kernel with the MXFP8 way out."""
        call("isic_layernorm_mxfp8_f16", x, gamma, beta, q, s, M, D, eps)

    def run_forward_train(self, images):
        """The layer-by-layer forward (bitwise ``run_tokens`` with fold_layernorm=False) that keeps what the backward needs."""
        self._check_images(images)
        w = self._prepare_train(images.device)
        N = images.shape[0]
        x, _, rows = self._patch_stream(images, w, False)
        x, blocks = blocks_forward(w, x, None, N, self.depth, self._spec(), save=True, layernorm=self._layernorm)
        return self._final_norm(x, w, N), dict(N=N, rows=rows, blocks=blocks, x=x, w=w)

    def run_backward(self, tape, dtok):
        """Accumulates every parameter gradient into ``param.grad`` from d loss / d tokens[N, T, D]."""
        w, N = tape["w"], tape["N"]
        T, D, K0 = self.tokens, self.dim, self.in_ch * self.patch ** 2
        M = N * T
        dev = dtok.device
        dtok, S = loss_scale(dtok, "ViTSmallEncoder")     # the backward's one device -> host read before its final check
        nb = max(blocks_workspace_bytes(w, N, self._spec()), call("isic_gemm_f16_wgrad_workspace_bytes", M, D, K0),
                 call("isic_colsum_f16_workspace_bytes", N, T * D))
        bw = Backward(self, w, param_grads(self, lambda n: n.replace(".", "__")), 1.0 / S, nb, dev)
        g = torch.empty((M, D), device=dev, dtype=torch.float32)          # d loss / d residual stream, x S, fp32
        g16 = torch.empty((M, D), device=dev, dtype=_F16)
        bw.ln_add(dtok, 1, S, tape["x"], None, None, "norm", 0, 1e-6, None, g, g16, M, D)
        self._fire(["norm.weight", "norm.bias"])
        blocks_backward(tape["blocks"], g, g16, bw, N, self.depth, self._spec(), self._fire)
        bw.wgrad(g16, tape["rows"], "patch_embed.proj", D, K0, M)
        bw.colsum(g16, "pos_embed", N, T * D)
        self._fire(["patch_embed.proj.weight", "patch_embed.proj.bias", "pos_embed"])
        check_grads(self.parameters(), "ViTSmallEncoder")

    def train_flops_per_image(self):
        """Forward + backward products (the patch projection has no data gradient)."""
        T, D = self.tokens, self.dim
        return 3 * self.flops_per_image() - 2 * T * D * self.in_ch * self.patch ** 2

    def flops_per_image(self):
        T, D, Hm = self.tokens, self.dim, self.mlp
        per_block = 2 * T * (D * 3 * D + D * D + 2 * D * Hm) + 4 * T * T * D
        return 2 * T * D * self.in_ch * self.patch ** 2 + self.depth * per_block

