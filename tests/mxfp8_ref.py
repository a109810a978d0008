"""MXFP8 on the CPU: the quantisation rule of the encoder's opt-in ``precision="mxfp8"`` path and an emulation of that
forward, for the tests (test_mxfp8_cpu.py, test_mxfp8_gpu.py).

Format: OCP MX with FP8 E4M3 elements (``torch.float8_e4m3fn``, not the MI300 ``fnuz`` encoding).  An operand x[rows][K]
becomes q[rows][K] uint8 (e4m3fn bytes) and s[rows][K / 32] uint8 (E8M0), one scale per block of 32 consecutive elements
along K, and dequantises to ``float(q) * 2^(s - 127)``.  A block quantises as follows:
  * amax = max |v| over the block, in fp32;
  * amax == 0: scale byte 0, every element +0;
  * otherwise e = the smallest integer with amax <= 448 * 2^e (the frexp exponent and one compare), clamped to
    [-127, 127] -- the clamp only binds below 448 * 2^-127, where it cannot saturate; scale byte e + 127;
  * element = round-to-nearest-even e4m3fn cast of v * 2^-e, as ``x.to(torch.float8_e4m3fn)`` does (subnormals
    included); |v * 2^-e| <= 448 by the choice of e, so nothing saturates.
The kernels of csrc/mxfp8.hip follow the same rule bit for bit.

``forward_tokens_mxfp8`` restates ``oracle/vit.py``'s forward on its parameter layout with the rounding points of the
MXFP8 path (isic_hip/vit.py): fp16 patch projection and residual stream, LayerNorm quantised from fp32, weights quantised
from the fp32 masters, attention in fp16, its output quantised before attn.proj, fc1 + GELU quantised for fc2.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

BLOCK = 32
E4M3_MAX = 448.0
_POW2 = torch.tensor([math.ldexp(1.0, b - 127) for b in range(256)], dtype=torch.float64)   # E8M0 byte -> 2^(b - 127)


def block_exponent(amax):
    """amax (fp32, > 0) -> the smallest integer e with amax <= 448 * 2^e, clamped to [-127, 127] (int32)."""
    m, E = torch.frexp(amax.float())                 # amax = m * 2^E, m in [0.5, 1); 448 = 0.875 * 2^9
    e = E - 9 + (m > 0.875).to(E.dtype)
    return e.clamp(-127, 127)


def quantize(x):
    """x[..., K] (any float dtype, finite; K % 32 == 0) -> (q[..., K] uint8, s[..., K / 32] uint8)."""
    K = x.shape[-1]
    if K % BLOCK:
        raise ValueError("K % 32 != 0")
    lead = x.shape[:-1]
    b = x.float().reshape(-1, K // BLOCK, BLOCK)
    amax = b.abs().amax(dim=-1)
    zero = amax == 0
    e = torch.where(zero, torch.zeros_like(amax, dtype=torch.int32), block_exponent(amax).to(torch.int32))
    inv = ((127 - e) << 23).view(torch.float32)      # 2^-e exactly (e <= 120 for any finite fp32 amax)
    q = (b * inv[..., None]).to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.where(zero[..., None], torch.zeros_like(q), q)
    s = torch.where(zero, torch.zeros_like(e), e + 127).to(torch.uint8)
    return q.reshape(*lead, K), s.reshape(*lead, K // BLOCK)


def dequantize(q, s):
    """(q[..., K] uint8, s[..., K / 32] uint8) -> fp32 values float(q) * 2^(s - 127) (exact in fp64, then fp32)."""
    K = q.shape[-1]
    v = q.contiguous().view(torch.float8_e4m3fn).double().reshape(*q.shape[:-1], K // BLOCK, BLOCK)
    return (v * _POW2[s.long()][..., None]).reshape(q.shape).float()


def fake_quant(x):
    """x -> dequantize(quantize(x)) in fp32."""
    return dequantize(*quantize(x))


def e4m3_step(q):
    """The spacing of e4m3fn values at the magnitude of the byte(s) q (the ulp one element byte may move by)."""
    mag = (q.long() & 0x7F)
    exp = mag >> 3
    return torch.where(exp == 0, torch.full_like(mag, 0, dtype=torch.float64) + 2.0 ** -9,
                       torch.pow(2.0, (exp - 7 - 3).double()))


def forward_tokens_mxfp8(p, images, heads=6, depth=None, eps=1e-6):
    """images[N,3,H,W] fp32 -> tokens[N, (H/16)*(W/16), 384] fp32 with the MXFP8 path's rounding points."""
    def r(t):
        return t.half().float()
    patch = p["patch_embed.proj.weight"].shape[-1]
    dim = p["patch_embed.proj.weight"].shape[0]
    N = images.shape[0]
    x = F.conv2d(r(images), r(p["patch_embed.proj.weight"]), p["patch_embed.proj.bias"], stride=patch)
    x = x.flatten(2).transpose(1, 2)
    x = r(x + r(p["pos_embed"]))
    T = x.shape[1]
    hd = dim // heads
    nblocks = depth if depth is not None else sum(1 for k in p if k.endswith(".norm1.weight"))
    for i in range(nblocks):
        b = f"blocks.{i}"
        w = {n: fake_quant(p[f"{b}.{n}.weight"]) for n in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")}
        h = fake_quant(F.layer_norm(x, (dim,), p[f"{b}.norm1.weight"], p[f"{b}.norm1.bias"], eps))
        qkv = r(F.linear(h, w["attn.qkv"], p[f"{b}.attn.qkv.bias"]))
        q, k, v = qkv.view(N, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
        a = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(hd), dim=-1)
        o = r(r(a) @ v)
        o = fake_quant(o.transpose(1, 2).reshape(N, T, dim))
        x = r(x + F.linear(o, w["attn.proj"], p[f"{b}.attn.proj.bias"]))
        h = fake_quant(F.layer_norm(x, (dim,), p[f"{b}.norm2.weight"], p[f"{b}.norm2.bias"], eps))
        h = fake_quant(F.gelu(F.linear(h, w["mlp.fc1"], p[f"{b}.mlp.fc1.bias"])))
        x = r(x + F.linear(h, w["mlp.fc2"], p[f"{b}.mlp.fc2.bias"]))
    return F.layer_norm(x, (dim,), p["norm.weight"], p["norm.bias"], eps)
