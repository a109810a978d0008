"""ConvMAE-Base encoder on torch-CPU in fp32: the restatement ``isic_hip/convmae.py`` is checked against.

PARITY UNPINNED against the published ConvMAE code (``models_convmae.py`` / ``vision_transformer.py``), which neither the
reference nor this tree vendors; this restates it from the table in the module docstring of ``isic_hip/convmae.py``
(the same key names, OIHW convolution weights, ``nn.Conv2d`` semantics through ``F.conv2d`` with ``groups`` for the
depthwise 5x5, NCHW tensors as in the published code).

``emulate_fp16=True`` rounds to fp16 at exactly the points where the HIP path stores fp16 (the stem's input pixels, every
matrix weight, every convolution / Linear / LayerNorm / attention output, the residual streams, s1 and s2), with fp32
arithmetic in between; the depthwise weights, biases and LayerNorm affines stay fp32, as in the HIP path.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

DIMS, DEPTHS, GRIDS, HEADS, MLP_RATIO = (256, 384, 768), (2, 2, 11), (56, 28, 14), 12, 4
LN_EPS, CONV_LN_EPS = 1e-6, 1e-5


def convmae_shapes(dims=DIMS, depths=DEPTHS, in_ch=3, tokens=196, r=MLP_RATIO):
    """The encoder keys of a ConvMAE-Base checkpoint and their shapes."""
    d1, d2, d3 = dims
    s = OrderedDict()
    s["pos_embed"] = (1, tokens, d3)
    for name, cin, cout, k in (("patch_embed1", in_ch, d1, 4), ("patch_embed2", d1, d2, 2), ("patch_embed3", d2, d3, 2)):
        s[f"{name}.proj.weight"] = (cout, cin, k, k); s[f"{name}.proj.bias"] = (cout,)
        s[f"{name}.norm.weight"] = (cout,); s[f"{name}.norm.bias"] = (cout,)
    s["patch_embed4.weight"] = (d3, d3); s["patch_embed4.bias"] = (d3,)
    s["stage1_output_decode.weight"] = (d3, d1, 4, 4); s["stage1_output_decode.bias"] = (d3,)
    s["stage2_output_decode.weight"] = (d3, d2, 2, 2); s["stage2_output_decode.bias"] = (d3,)
    for stage, C, nb in (("blocks1", d1, depths[0]), ("blocks2", d2, depths[1])):
        for i in range(nb):
            b = f"{stage}.{i}"
            s[f"{b}.norm1.weight"] = (C,); s[f"{b}.norm1.bias"] = (C,)
            s[f"{b}.conv1.weight"] = (C, C, 1, 1); s[f"{b}.conv1.bias"] = (C,)
            s[f"{b}.attn.weight"] = (C, 1, 5, 5); s[f"{b}.attn.bias"] = (C,)
            s[f"{b}.conv2.weight"] = (C, C, 1, 1); s[f"{b}.conv2.bias"] = (C,)
            s[f"{b}.norm2.weight"] = (C,); s[f"{b}.norm2.bias"] = (C,)
            s[f"{b}.mlp.fc1.weight"] = (r * C, C, 1, 1); s[f"{b}.mlp.fc1.bias"] = (r * C,)
            s[f"{b}.mlp.fc2.weight"] = (C, r * C, 1, 1); s[f"{b}.mlp.fc2.bias"] = (C,)
    for i in range(depths[2]):
        b = f"blocks3.{i}"
        s[f"{b}.norm1.weight"] = (d3,); s[f"{b}.norm1.bias"] = (d3,)
        s[f"{b}.attn.qkv.weight"] = (3 * d3, d3); s[f"{b}.attn.qkv.bias"] = (3 * d3,)
        s[f"{b}.attn.proj.weight"] = (d3, d3); s[f"{b}.attn.proj.bias"] = (d3,)
        s[f"{b}.norm2.weight"] = (d3,); s[f"{b}.norm2.bias"] = (d3,)
        s[f"{b}.mlp.fc1.weight"] = (r * d3, d3); s[f"{b}.mlp.fc1.bias"] = (r * d3,)
        s[f"{b}.mlp.fc2.weight"] = (d3, r * d3); s[f"{b}.mlp.fc2.bias"] = (d3,)
    s["norm.weight"] = (d3,); s["norm.bias"] = (d3,)
    return s


def sincos_pos_embed(dim=768, grid=14):
    """[1, grid*grid, dim] fp32 from the formula: token (i, j) = [sin(j w), cos(j w), sin(i w), cos(i w)], w_k = 10000^(-k/(dim/4))."""
    q = dim // 4
    w = 1.0 / 10000 ** (torch.arange(q, dtype=torch.float64) / q)
    i = torch.arange(grid, dtype=torch.float64).repeat_interleave(grid)
    j = torch.arange(grid, dtype=torch.float64).repeat(grid)
    jw, iw = j[:, None] * w[None, :], i[:, None] * w[None, :]
    return torch.cat([jw.sin(), jw.cos(), iw.sin(), iw.cos()], dim=1).float().unsqueeze(0)


def init_params(seed=0):
    """Deterministic parameters for the tests: N(0, 1/fan_in) weights, LayerNorm affine and biases perturbed away from
    (1, 0) (so that a dropped bias or gamma shows up), the sin-cos position embedding."""
    g = torch.Generator().manual_seed(seed)
    p = OrderedDict()
    for k, shp in convmae_shapes().items():
        if k == "pos_embed":
            p[k] = sincos_pos_embed()
        elif "norm" in k and k.endswith(".weight"):
            p[k] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif len(shp) == 1:
            p[k] = 0.02 * torch.randn(shp, generator=g)
        else:
            fan = math.prod(shp[1:])
            p[k] = torch.randn(shp, generator=g) / math.sqrt(fan)
    return p


def _r(x, on):
    return x.half().float() if on else x


def _ln_c(x, w, b, eps):
    """LayerNorm over the channels of an NCHW map"""
    return F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), w, b, eps).permute(0, 3, 1, 2)


def forward_tokens(p, images, emulate_fp16=False, depth=None, heads=HEADS, ln_eps=LN_EPS, conv_ln_eps=CONV_LN_EPS):
    """images[N,3,224,224] fp32 -> latent[N, 196, 768] fp32 (the final LayerNorm unrounded).  ``depth`` = block counts per
    stage (default: all)."""
    e = emulate_fp16
    depth = DEPTHS if depth is None else depth
    W = {k: (_r(v, e) if (v.dim() > 1 and k != "pos_embed" and not k.endswith(".attn.weight")) else v) for k, v in p.items()}

    def patch_embed(x, name):
        k = p[f"{name}.proj.weight"].shape[-1]
        t = _r(F.conv2d(x, W[f"{name}.proj.weight"], p[f"{name}.proj.bias"], stride=k), e)
        return _r(F.gelu(_ln_c(t, p[f"{name}.norm.weight"], p[f"{name}.norm.bias"], conv_ln_eps)), e)

    def cblock(x, b):
        C = x.shape[1]
        h = _r(_ln_c(x, p[f"{b}.norm1.weight"], p[f"{b}.norm1.bias"], conv_ln_eps), e)
        h = _r(F.conv2d(h, W[f"{b}.conv1.weight"], p[f"{b}.conv1.bias"]), e)
        h = _r(F.conv2d(h, W[f"{b}.attn.weight"], p[f"{b}.attn.bias"], padding=2, groups=C), e)
        x = _r(x + F.conv2d(h, W[f"{b}.conv2.weight"], p[f"{b}.conv2.bias"]), e)
        h = _r(_ln_c(x, p[f"{b}.norm2.weight"], p[f"{b}.norm2.bias"], conv_ln_eps), e)
        h = _r(F.gelu(F.conv2d(h, W[f"{b}.mlp.fc1.weight"], p[f"{b}.mlp.fc1.bias"])), e)
        return _r(x + F.conv2d(h, W[f"{b}.mlp.fc2.weight"], p[f"{b}.mlp.fc2.bias"]), e)

    x = patch_embed(_r(images, e), "patch_embed1")
    for i in range(depth[0]):
        x = cblock(x, f"blocks1.{i}")
    s1 = _r(F.conv2d(x, W["stage1_output_decode.weight"], p["stage1_output_decode.bias"], stride=4), e).flatten(2).transpose(1, 2)
    x = patch_embed(x, "patch_embed2")
    for i in range(depth[1]):
        x = cblock(x, f"blocks2.{i}")
    s2 = _r(F.conv2d(x, W["stage2_output_decode.weight"], p["stage2_output_decode.bias"], stride=2), e).flatten(2).transpose(1, 2)
    x = patch_embed(x, "patch_embed3").flatten(2).transpose(1, 2)            # [N, 196, 768], raster order
    x = _r(F.linear(x, W["patch_embed4.weight"], p["patch_embed4.bias"]) + _r(p["pos_embed"], e), e)
    N, T, D = x.shape
    hd = D // heads
    for i in range(depth[2]):
        b = f"blocks3.{i}"
        h = _r(F.layer_norm(x, (D,), p[f"{b}.norm1.weight"], p[f"{b}.norm1.bias"], ln_eps), e)
        qkv = _r(F.linear(h, W[f"{b}.attn.qkv.weight"], p[f"{b}.attn.qkv.bias"]), e)
        q, k, v = qkv.view(N, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(hd), dim=-1)
        o = _r(a, e) @ v
        o = _r(o.transpose(1, 2).reshape(N, T, D), e)
        x = _r(x + F.linear(o, W[f"{b}.attn.proj.weight"], p[f"{b}.attn.proj.bias"]), e)
        h = _r(F.layer_norm(x, (D,), p[f"{b}.norm2.weight"], p[f"{b}.norm2.bias"], ln_eps), e)
        h = _r(F.gelu(F.linear(h, W[f"{b}.mlp.fc1.weight"], p[f"{b}.mlp.fc1.bias"])), e)
        x = _r(x + F.linear(h, W[f"{b}.mlp.fc2.weight"], p[f"{b}.mlp.fc2.bias"]), e)
    return F.layer_norm(x + s1 + s2, (D,), p["norm.weight"], p["norm.bias"], ln_eps)
