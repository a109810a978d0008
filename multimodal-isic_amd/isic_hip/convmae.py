"""ConvMAE-Base patch encoder, fp16 on gfx950 -- the encoder the reference makes its patch latents with.

The reference builds ``convmae_convvit_base_patch16_dec512d8b(with_decoder=False)``, loads a checkpoint of its
``train_ae.py`` with ``strict=False`` and runs ``forward(images, mask_ratio=0) -> latent[B, 196, 768]``
(`save_latent.py:17-18,42-60`).  This module restates the encoder of the published ConvMAE code (Gao et al. 2022,
``models_convmae.py`` / ``vision_transformer.py``), which neither the reference nor this tree vendors: PARITY IS UNPINNED,
as for the ViT-S/16 (isic_hip/vit.py).  ``tests/convmae_ref.py`` is the fp32 torch-CPU restatement it is checked against.
Parameter names and shapes are the checkpoint's, so a reference checkpoint loads (convolution weights keep their OIHW
shapes in the state dict).  Inference only, frozen.

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

Memory: the batch runs in chunks of at most ``max_batch`` images (default 256); stage 1 holds about 15 MB of fp16
activations per image of a chunk (the fc1 output alone is 3136 x 1024 x 2 bytes), 3.9 GB at 256 images.  An image's
tokens do not depend on the batch or the chunk it is in.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from .lib import IsicHipError, call

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


class ConvMAEBaseEncoder(nn.Module):
    """Frozen ConvMAE-Base encoder (module docstring).  ``run_tokens(images[N,3,224,224]) -> [N, 196, 768]`` fp32."""

    img_size, in_ch, tokens = 224, 3, 196
    dims, depths, grids, patches = (256, 384, 768), (2, 2, 11), (56, 28, 14), (4, 2, 2)

    def __init__(self, seed=0, fold_layernorm=True, ln_eps=1e-6, conv_ln_eps=1e-5, heads=12, mlp_ratio=4, max_batch=256):
        super().__init__()
        if fold_layernorm not in (True, False):
            raise ValueError("fold_layernorm: True or False")
        if max_batch < 1:
            raise ValueError("max_batch >= 1")
        d1, d2, d3 = self.dims
        if d3 // heads != 64 or d3 % heads != 0:
            raise ValueError("ConvMAEBaseEncoder: head width 64 (isic_attention_f16)")
        self.fold_layernorm, self.ln_eps, self.conv_ln_eps = fold_layernorm, float(ln_eps), float(conv_ln_eps)
        self.heads, self.mlp_ratio, self.max_batch = heads, mlp_ratio, int(max_batch)
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
        for p in self.parameters():
            p.requires_grad_(False)                     # frozen, as in save_latent.py:51-53
        self._w16, self._w16_key = None, None
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

    def train(self, mode=True):
        if mode:
            raise IsicHipError("ConvMAEBaseEncoder is a frozen inference encoder (save_latent.py:51-53): no train() mode")
        return super().train(False)

    def load_state_dict(self, state_dict, strict=True, assign=False):
        """nn.Module semantics (a wrong shape raises, also under strict=False).  A full MAE checkpoint loads with no
        missing keys; its decoder (``decoder_*``, ``mask_token``) comes back as the unexpected keys."""
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self._w16_key = None
        return out

    # ------------------------------------------------------------------ weights, once per weight version
    def _prepare(self, device):
        params = list(self.parameters())
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._w16 is not None and key == self._w16_key:
            return self._w16
        if any(p.device != device for p in params):
            raise IsicHipError("ConvMAEBaseEncoder: move the module to the GPU first (.to('cuda'))")
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
        # LayerNorm folded into the next product: W' = W diag(gamma) fp16, c from the ROUNDED W', b' = b + W beta (fp32)
        for norm, lin in (folds if self.fold_layernorm else ()):
            W = sd[lin + ".weight"].float().reshape(sd[lin + ".weight"].shape[0], -1)
            Wg = (W * w[norm + ".weight"][None, :]).to(_F16).contiguous()
            w[lin + ".ln_weight"] = Wg
            w[lin + ".ln_c"] = Wg.float().sum(dim=1).contiguous()
            w[lin + ".ln_bias"] = (w[lin + ".bias"] + W @ w[norm + ".bias"]).contiguous()
        self._w16, self._w16_key = w, key
        return w

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def run_tokens(self, images, depth=None):
        """images[N,3,224,224] (fp32, normalised) on the GPU -> tokens[N, 196, 768] fp32.  ``depth`` = (blocks1, blocks2,
        blocks3) runs only the first blocks of each stage (a test of the composition)."""
        if images.dim() != 4 or tuple(images.shape[1:]) != (self.in_ch, self.img_size, self.img_size):
            raise ValueError(f"expected images[N,{self.in_ch},{self.img_size},{self.img_size}], got {tuple(images.shape)}")
        if not images.is_cuda:
            raise IsicHipError("ConvMAEBaseEncoder runs on the MI355X only (no CPU fallback)")
        depth = tuple(self.depths) if depth is None else tuple(depth)
        if len(depth) != 3 or any(not 0 <= d <= m for d, m in zip(depth, self.depths)):
            raise ValueError(f"depth: three block counts within {self.depths}")
        dev = images.device
        w = self._prepare(dev)
        x_in = images.float().contiguous()
        N = x_in.shape[0]
        out = torch.empty((N, self.tokens, self.out_dim), device=dev, dtype=torch.float32)
        for s in range(0, N, self.max_batch):
            e = min(N, s + self.max_batch)
            self._run_chunk(x_in[s:e], w, out[s:e], depth)
        return out

    def _run_chunk(self, img, w, out, depth):
        dev = img.device
        n = img.shape[0]
        (d1, d2, d3), (g1, g2, g3) = self.dims, self.grids
        M1, M2, M3 = n * g1 * g1, n * g2 * g2, n * g3 * g3
        T = self.tokens
        ceps = self.conv_ln_eps

        def e16(*shape):
            return torch.empty(shape, device=dev, dtype=_F16)

        def patch_embed(rows, name, M, C, K):
            t, y = e16(M, C), e16(M, C)
            call("isic_gemm_f16", rows, w[name + ".proj.weight"], w[name + ".proj.bias"], None, t, M, C, K, 0, 0)
            call("isic_layernorm_add_f16", t, None, None, w[name + ".norm.weight"], w[name + ".norm.bias"], y, None, M, C, 1, ceps)
            return y

        # ---- stage 1: 56 x 56 x 256
        rows = e16(M1, 64)
        call("isic_patch_rows_nchw_f32", img, rows, n, self.in_ch, self.img_size, self.img_size, 4, 64)
        x = patch_embed(rows, "patch_embed1", M1, d1, 64)
        del rows
        x = self._cblocks(x, w, "blocks1", n, g1, d1, depth[0])
        rows = e16(M3, 16 * d1)
        call("isic_patch_rows_nhwc_f16", x, rows, n, g1, g1, d1, 4)
        s1 = e16(M3, d3)
        call("isic_gemm_f16", rows, w["stage1_output_decode.weight"], w["stage1_output_decode.bias"], None, s1, M3, d3, 16 * d1, 0, 0)
        rows = e16(M2, 4 * d1)
        call("isic_patch_rows_nhwc_f16", x, rows, n, g1, g1, d1, 2)
        del x
        # ---- stage 2: 28 x 28 x 384
        x = patch_embed(rows, "patch_embed2", M2, d2, 4 * d1)
        del rows
        x = self._cblocks(x, w, "blocks2", n, g2, d2, depth[1])
        rows = e16(M3, 4 * d2)
        call("isic_patch_rows_nhwc_f16", x, rows, n, g2, g2, d2, 2)
        del x
        s2 = e16(M3, d3)
        call("isic_gemm_f16", rows, w["stage2_output_decode.weight"], w["stage2_output_decode.bias"], None, s2, M3, d3, 4 * d2, 0, 0)
        # ---- stage 3: 196 tokens x 768
        t3 = patch_embed(rows, "patch_embed3", M3, d3, 4 * d2)
        del rows
        x = self._vit_blocks(t3, w, n, depth[2])
        call("isic_layernorm_add_f16", x, s1, s2, w["norm.weight"], w["norm.bias"], None, out, M3, d3, 0, self.ln_eps)

    def _cblocks(self, x, w, stage, n, g, C, nblk):
        """CBlocks over the NHWC stream x[n*g*g, C] (updated in place; returned)."""
        dev = x.device
        M, Hd, eps, fold = n * g * g, C * self.mlp_ratio, self.conv_ln_eps, self.fold_layernorm
        parts = 2 * C // 128
        h = torch.empty((M, C), device=dev, dtype=_F16)
        d = torch.empty_like(h)
        x2 = torch.empty_like(h)
        hid = torch.empty((M, Hd), device=dev, dtype=_F16)
        st = st2 = None
        p_in = 0
        if fold and nblk:
            st = torch.empty((M, parts, 2), device=dev, dtype=torch.float32)
            st2 = torch.empty_like(st)
            call("isic_row_stats_f16", x, st, M, C, eps)                 # (mean, rstd) of the PatchEmbed output: ln_parts 0
        for i in range(nblk):
            b = f"{stage}.{i}"
            if fold:
                call("isic_gemm_f16_ln", x, w[b + ".conv1.ln_weight"], w[b + ".conv1.ln_bias"], w[b + ".conv1.ln_c"], st, p_in,
                     h, M, C, C, 0, eps)
                call("isic_dwconv5x5_f16", h, w[b + ".attn.weight"], w[b + ".attn.bias"], d, n, g, g, C)
                call("isic_gemm_f16_stats", d, w[b + ".conv2.weight"], w[b + ".conv2.bias"], x, x2, st2, M, C, C, 0, 0)
                call("isic_gemm_f16_ln", x2, w[b + ".mlp.fc1.ln_weight"], w[b + ".mlp.fc1.ln_bias"], w[b + ".mlp.fc1.ln_c"], st2,
                     parts, hid, M, Hd, C, 1, eps)
                call("isic_gemm_f16_stats", hid, w[b + ".mlp.fc2.weight"], w[b + ".mlp.fc2.bias"], x2, x, st, M, C, Hd, 0, 0)
                p_in = parts
            else:
                call("isic_layernorm_add_f16", x, None, None, w[b + ".norm1.weight"], w[b + ".norm1.bias"], h, None, M, C, 0, eps)
                call("isic_gemm_f16", h, w[b + ".conv1.weight"], w[b + ".conv1.bias"], None, d, M, C, C, 0, 0)
                call("isic_dwconv5x5_f16", d, w[b + ".attn.weight"], w[b + ".attn.bias"], h, n, g, g, C)
                call("isic_gemm_f16", h, w[b + ".conv2.weight"], w[b + ".conv2.bias"], x, x2, M, C, C, 0, 0)
                call("isic_layernorm_add_f16", x2, None, None, w[b + ".norm2.weight"], w[b + ".norm2.bias"], h, None, M, C, 0, eps)
                call("isic_gemm_f16", h, w[b + ".mlp.fc1.weight"], w[b + ".mlp.fc1.bias"], None, hid, M, Hd, C, 1, 0)
                call("isic_gemm_f16", hid, w[b + ".mlp.fc2.weight"], w[b + ".mlp.fc2.bias"], x2, x, M, C, Hd, 0, 0)
        return x

    def _vit_blocks(self, t3, w, n, nblk):
        """patch_embed4 (+ pos_embed) and the transformer blocks over t3[n*196, 768] -> the residual stream (fp16)."""
        dev = t3.device
        T, D, H = self.tokens, self.dims[2], self.heads
        M, Hd, eps, fold = n * T, D * self.mlp_ratio, self.ln_eps, self.fold_layernorm
        parts = 2 * D // 128
        x = torch.empty((M, D), device=dev, dtype=_F16)
        x2 = torch.empty_like(x)
        h = torch.empty_like(x) if not fold else None
        qkv = torch.empty((M, 3 * D), device=dev, dtype=_F16)
        att = torch.empty_like(x)
        hid = torch.empty((M, Hd), device=dev, dtype=_F16)
        st = torch.empty((M, parts, 2), device=dev, dtype=torch.float32) if fold else None
        st2 = torch.empty_like(st) if fold else None

        def linear_res(a, name, res, out, stats, K, res_rows=0):
            if fold:
                call("isic_gemm_f16_stats", a, w[name + ".weight"], w[name + ".bias"], res, out, stats, M, D, K, 0, res_rows)
            else:
                call("isic_gemm_f16", a, w[name + ".weight"], w[name + ".bias"], res, out, M, D, K, 0, res_rows)

        def linear_ln(xin, stats, norm, name, out, Nout, act):
            if fold:
                call("isic_gemm_f16_ln", xin, w[name + ".ln_weight"], w[name + ".ln_bias"], w[name + ".ln_c"], stats, parts, out,
                     M, Nout, D, act, eps)
            else:
                call("isic_layernorm_add_f16", xin, None, None, w[norm + ".weight"], w[norm + ".bias"], h, None, M, D, 0, eps)
                call("isic_gemm_f16", h, w[name + ".weight"], w[name + ".bias"], None, out, M, Nout, D, act, 0)

        linear_res(t3, "patch_embed4", w["pos_embed"], x, st, D, res_rows=T)
        for i in range(nblk):
            b = f"blocks3.{i}"
            linear_ln(x, st, f"{b}.norm1", f"{b}.attn.qkv", qkv, 3 * D, 0)
            call("isic_attention_f16", qkv, att, n, T, H, D // H)
            linear_res(att, f"{b}.attn.proj", x, x2, st2, D)
            linear_ln(x2, st2, f"{b}.norm2", f"{b}.mlp.fc1", hid, Hd, 1)
            linear_res(hid, f"{b}.mlp.fc2", x2, x, st, Hd)
        return x

    def forward_tokens(self, images):
        """tokens[N, 196, 768] fp32 (frozen: no autograd)."""
        return self.run_tokens(images)

    def forward(self, images):
        """Mean-pooled 768-d feature per image (what a MIL bag of patches consumes)."""
        return self.forward_tokens(images).mean(dim=1)

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
