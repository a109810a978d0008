"""ConvMAE-Base encoder on torch-CPU with the rounding points of ``ConvMAEBaseEncoder(precision="mxfp8")``
(isic_hip/convmae.py), on top of ``convmae_ref`` (the fp32 restatement, its parameter layout) and ``mxfp8_ref.fake_quant``
(the quantisation rule).  MX(.) below is quantise-dequantise in blocks of 32 channels, fp16(.) a round trip through fp16:

    stem        unchanged: fp16 pixels and weight, conv -> fp16, LayerNorm + GELU -> fp16 stream x
    CBlock      h = MX(LN1(x)); d = fp16(conv1(h)); m = MX(dw5x5(d) + b); x2 = fp16(x + conv2(m));
                h2 = MX(LN2(x2)); hid = MX(GELU(fc1(h2))); x = fp16(x2 + fc2(hid))
    patch convs the stage output quantised per pixel (= the MXFP8 patch rows, C % 32 == 0), decoders -> fp16 s1, s2;
                patch_embed2: conv -> fp16, LayerNorm + GELU -> fp16; patch_embed3: conv -> fp16, MX(GELU(LN(.)))
    patch_embed4  fp16(linear + fp16(pos_embed))
    blocks3     the MXFP8 transformer block of mxfp8_ref.forward_tokens_mxfp8 at D = 768
    output      norm(x + s1 + s2) in fp32, unrounded

Maps are quantised along C per pixel and weights along I per (o, kh, kw); that equals the row form of the kernels (rows of
[kh][kw][c] columns) because C % 32 == 0.  Depthwise taps, biases and LayerNorm affines stay fp32.  ``products_fp64=True``
takes every product that runs on the scaled MFMA (and the fp16 stem product) in fp64 instead of fp32: the distance between
the two is what a change of summation order alone does to the output.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import convmae_ref as cr
from mxfp8_ref import fake_quant


def _r(x):
    return x.half().float()


def _mx_c(x):
    """NCHW map -> quantised along C per pixel"""
    return fake_quant(x.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)


def _mx_w(w):
    """OIHW or [O, I] weight -> quantised along I per (o, kh, kw)"""
    return fake_quant(w.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2) if w.dim() == 4 else fake_quant(w)


def forward_tokens_mxfp8(p, images, depth=None, products_fp64=False, heads=cr.HEADS, ln_eps=cr.LN_EPS,
                         conv_ln_eps=cr.CONV_LN_EPS):
    """images[N,3,224,224] fp32 -> latent[N, 196, 768] fp32 with the MXFP8 path's rounding points."""
    depth = cr.DEPTHS if depth is None else depth
    skip = ("pos_embed", "patch_embed1.proj.weight")
    W = {k: _mx_w(v) for k, v in p.items() if v.dim() > 1 and k not in skip and not k.endswith(".attn.weight")}
    W["patch_embed1.proj.weight"] = _r(p["patch_embed1.proj.weight"])

    def prod(fn, x, w, b, **kw):
        if products_fp64:
            return fn(x.double(), w.double(), b.double(), **kw).float()
        return fn(x, w, b, **kw)

    def conv(x, name, stride=1):
        return prod(F.conv2d, x, W[name + ".weight"], p[name + ".bias"], stride=stride)

    def linear(x, name):
        return prod(F.linear, x, W[name + ".weight"], p[name + ".bias"])

    def ln_c(x, name):
        return cr._ln_c(x, p[name + ".weight"], p[name + ".bias"], conv_ln_eps)

    def cblock(x, b):
        C = x.shape[1]
        h = _mx_c(ln_c(x, b + ".norm1"))
        d = _r(conv(h, b + ".conv1"))
        m = _mx_c(F.conv2d(d, p[b + ".attn.weight"], p[b + ".attn.bias"], padding=2, groups=C))
        x2 = _r(x + conv(m, b + ".conv2"))
        h2 = _mx_c(ln_c(x2, b + ".norm2"))
        hid = _mx_c(F.gelu(conv(h2, b + ".mlp.fc1")))
        return _r(x2 + conv(hid, b + ".mlp.fc2"))

    x = _r(conv(_r(images), "patch_embed1.proj", 4))
    x = _r(F.gelu(ln_c(x, "patch_embed1.norm")))
    for i in range(depth[0]):
        x = cblock(x, f"blocks1.{i}")
    xq = _mx_c(x)
    s1 = _r(conv(xq, "stage1_output_decode", 4)).flatten(2).transpose(1, 2)
    x = _r(F.gelu(ln_c(_r(conv(xq, "patch_embed2.proj", 2)), "patch_embed2.norm")))
    for i in range(depth[1]):
        x = cblock(x, f"blocks2.{i}")
    xq = _mx_c(x)
    s2 = _r(conv(xq, "stage2_output_decode", 2)).flatten(2).transpose(1, 2)
    x = _mx_c(F.gelu(ln_c(_r(conv(xq, "patch_embed3.proj", 2)), "patch_embed3.norm"))).flatten(2).transpose(1, 2)
    x = _r(linear(x, "patch_embed4") + _r(p["pos_embed"]))
    N, T, D = x.shape
    hd = D // heads
    for i in range(depth[2]):
        b = f"blocks3.{i}"
        h = fake_quant(F.layer_norm(x, (D,), p[f"{b}.norm1.weight"], p[f"{b}.norm1.bias"], ln_eps))
        qkv = _r(linear(h, b + ".attn.qkv"))
        q, k, v = qkv.view(N, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(hd), dim=-1)
        o = _r(_r(a) @ v)
        o = fake_quant(o.transpose(1, 2).reshape(N, T, D))
        x = _r(x + linear(o, b + ".attn.proj"))
        h = fake_quant(F.layer_norm(x, (D,), p[f"{b}.norm2.weight"], p[f"{b}.norm2.bias"], ln_eps))
        h = fake_quant(F.gelu(linear(h, b + ".mlp.fc1")))
        x = _r(x + linear(h, b + ".mlp.fc2"))
    return F.layer_norm(x + s1 + s2, (D,), p["norm.weight"], p["norm.bias"], ln_eps)
