"""ConvMAE-Base masked autoencoder on torch-CPU: the restatement ``isic_hip/convmae_mae.py`` is checked against.

PARITY UNPINNED against the published ConvMAE code (``models_convmae.py``), which neither the reference nor this tree
vendors; this restates the definitions of the module docstring of ``isic_hip/convmae_mae.py`` (masking, masked CBlocks,
the gathered stage 3, the 8-block decoder, the reconstruction loss) on top of ``tests/convmae_ref.py``.

``emulate_fp16=True`` rounds to fp16 where the HIP path stores fp16 (as in convmae_ref, plus the latent handed to the
decoder, every decoder activation and pred), with fp32 arithmetic in between.  The rounding is a straight-through
``x + (fp16(x) - x).detach()``, so autograd through it gives the gradients of the rounded forward in fp32.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

import convmae_ref as cr

DEC_DIM, DEC_DEPTH, DEC_HEADS, PATCH = 512, 8, 16, 16


def decoder_shapes(depth=DEC_DEPTH, D=768, Dd=DEC_DIM, r=4, tokens=196, pred=PATCH * PATCH * 3):
    s = OrderedDict()
    s["mask_token"] = (1, 1, Dd)
    s["decoder_pos_embed"] = (1, tokens, Dd)
    s["decoder_embed.weight"] = (Dd, D); s["decoder_embed.bias"] = (Dd,)
    for i in range(depth):
        b = f"decoder_blocks.{i}"
        s[f"{b}.norm1.weight"] = (Dd,); s[f"{b}.norm1.bias"] = (Dd,)
        s[f"{b}.attn.qkv.weight"] = (3 * Dd, Dd); s[f"{b}.attn.qkv.bias"] = (3 * Dd,)
        s[f"{b}.attn.proj.weight"] = (Dd, Dd); s[f"{b}.attn.proj.bias"] = (Dd,)
        s[f"{b}.norm2.weight"] = (Dd,); s[f"{b}.norm2.bias"] = (Dd,)
        s[f"{b}.mlp.fc1.weight"] = (r * Dd, Dd); s[f"{b}.mlp.fc1.bias"] = (r * Dd,)
        s[f"{b}.mlp.fc2.weight"] = (Dd, r * Dd); s[f"{b}.mlp.fc2.bias"] = (Dd,)
    s["decoder_norm.weight"] = (Dd,); s["decoder_norm.bias"] = (Dd,)
    s["decoder_pred.weight"] = (pred, Dd); s["decoder_pred.bias"] = (pred,)
    return s


def mae_shapes():
    s = cr.convmae_shapes()
    s.update(decoder_shapes())
    return s


def init_params(seed=0):
    """Encoder as convmae_ref.init_params; decoder weights N(0, 1/fan_in), biases and LayerNorm affines perturbed."""
    p = cr.init_params(seed)
    g = torch.Generator().manual_seed(seed + 7)
    for k, shp in decoder_shapes().items():
        if k == "decoder_pos_embed":
            p[k] = cr.sincos_pos_embed(DEC_DIM, 14)
        elif k == "mask_token":
            p[k] = 0.02 * torch.randn(shp, generator=g)
        elif "norm" in k and k.endswith(".weight"):
            p[k] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        elif len(shp) == 1:
            p[k] = 0.02 * torch.randn(shp, generator=g)
        else:
            p[k] = torch.randn(shp, generator=g) / math.sqrt(math.prod(shp[1:]))
    return p


def masking(n, mask_ratio, noise=None, T=196):
    """-> (ids_shuffle, ids_restore, ids_keep, mask, len_keep) as in the module docstring."""
    if not 0 <= mask_ratio < 1:
        raise ValueError("mask_ratio")
    L = int(T * (1 - mask_ratio))
    if L < 1:
        raise ValueError("len_keep")
    ids_shuffle = torch.arange(T).expand(n, T) if noise is None else torch.argsort(noise, dim=1)
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    mask = torch.ones(n, T)
    mask[:, :L] = 0
    mask = torch.gather(mask, 1, ids_restore)
    return ids_shuffle, ids_restore, ids_shuffle[:, :L], mask, L


def patchify(imgs, p=PATCH):
    n, c, H, W = imgs.shape
    x = imgs.reshape(n, c, H // p, p, W // p, p)
    return torch.einsum("nchpwq->nhwpqc", x).reshape(n, (H // p) * (W // p), p * p * c)


def _r(x, on):
    return x + (x.half().float() - x).detach() if on else x


def _block(x, p, W, b, heads, eps, e):
    N, T, D = x.shape
    hd = D // heads
    h = _r(F.layer_norm(x, (D,), p[f"{b}.norm1.weight"], p[f"{b}.norm1.bias"], eps), e)
    qkv = _r(F.linear(h, W[f"{b}.attn.qkv.weight"], p[f"{b}.attn.qkv.bias"]), e)
    q, k, v = qkv.view(N, T, 3, heads, hd).permute(2, 0, 3, 1, 4)
    a = torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(hd), dim=-1)
    o = _r((_r(a, e) @ v).transpose(1, 2).reshape(N, T, D), e)
    x = _r(x + F.linear(o, W[f"{b}.attn.proj.weight"], p[f"{b}.attn.proj.bias"]), e)
    h = _r(F.layer_norm(x, (D,), p[f"{b}.norm2.weight"], p[f"{b}.norm2.bias"], eps), e)
    h = _r(F.gelu(F.linear(h, W[f"{b}.mlp.fc1.weight"], p[f"{b}.mlp.fc1.bias"])), e)
    return _r(x + F.linear(h, W[f"{b}.mlp.fc2.weight"], p[f"{b}.mlp.fc2.bias"]), e)


def forward(p, images, mask_ratio=0.75, noise=None, norm_pix_loss=False, emulate_fp16=False, depth=None, dec_depth=DEC_DEPTH):
    """-> dict(loss, pred [N, 196, 768], mask, latent [N, len_keep, 768]).  ``p``: tensors (requires_grad for gradients)."""
    e = emulate_fp16
    depth = cr.DEPTHS if depth is None else depth
    dec_depth = DEC_DEPTH if dec_depth is None else dec_depth
    W = {k: (_r(v, e) if (v.dim() > 1 and "pos_embed" not in k and k != "mask_token" and not k.endswith(".attn.weight"))
             else v) for k, v in p.items()}
    ce, le = cr.CONV_LN_EPS, cr.LN_EPS
    n = images.shape[0]
    ids_shuffle, ids_restore, ids_keep, mask, L = masking(n, mask_ratio, noise)
    keep = (1 - mask).view(n, 1, 14, 14)

    def patch_embed(x, name):
        k = p[f"{name}.proj.weight"].shape[-1]
        t = _r(F.conv2d(x, W[f"{name}.proj.weight"], p[f"{name}.proj.bias"], stride=k), e)
        return _r(F.gelu(cr._ln_c(t, p[f"{name}.norm.weight"], p[f"{name}.norm.bias"], ce)), e)

    def cblock(x, b):
        C, P = x.shape[1], x.shape[2] // 14
        km = keep.repeat_interleave(P, 2).repeat_interleave(P, 3)
        h = _r(cr._ln_c(x, p[f"{b}.norm1.weight"], p[f"{b}.norm1.bias"], ce), e)
        h = _r(F.conv2d(h, W[f"{b}.conv1.weight"], p[f"{b}.conv1.bias"]), e) * km
        h = _r(F.conv2d(h, W[f"{b}.attn.weight"], p[f"{b}.attn.bias"], padding=2, groups=C), e)
        x = _r(x + F.conv2d(h, W[f"{b}.conv2.weight"], p[f"{b}.conv2.bias"]), e)
        h = _r(cr._ln_c(x, p[f"{b}.norm2.weight"], p[f"{b}.norm2.bias"], ce), e)
        h = _r(F.gelu(F.conv2d(h, W[f"{b}.mlp.fc1.weight"], p[f"{b}.mlp.fc1.bias"])), e)
        return _r(x + F.conv2d(h, W[f"{b}.mlp.fc2.weight"], p[f"{b}.mlp.fc2.bias"]), e)

    def take(t, ids):
        return torch.gather(t, 1, ids[..., None].expand(-1, -1, t.shape[-1]))

    x = patch_embed(_r(images, e), "patch_embed1")
    for i in range(depth[0]):
        x = cblock(x, f"blocks1.{i}")
    s1 = _r(F.conv2d(x, W["stage1_output_decode.weight"], p["stage1_output_decode.bias"], stride=4), e).flatten(2).transpose(1, 2)
    x = patch_embed(x, "patch_embed2")
    for i in range(depth[1]):
        x = cblock(x, f"blocks2.{i}")
    s2 = _r(F.conv2d(x, W["stage2_output_decode.weight"], p["stage2_output_decode.bias"], stride=2), e).flatten(2).transpose(1, 2)
    x = patch_embed(x, "patch_embed3").flatten(2).transpose(1, 2)
    x = _r(F.linear(x, W["patch_embed4.weight"], p["patch_embed4.bias"]) + _r(p["pos_embed"], e), e)
    x, s1, s2 = take(x, ids_keep), take(s1, ids_keep), take(s2, ids_keep)
    for i in range(depth[2]):
        x = _block(x, p, W, f"blocks3.{i}", cr.HEADS, le, e)
    D = x.shape[-1]
    latent = F.layer_norm(x + s1 + s2, (D,), p["norm.weight"], p["norm.bias"], le)
    # ---- decoder
    z = _r(F.linear(_r(latent, e), W["decoder_embed.weight"], p["decoder_embed.bias"]), e)
    Dd = z.shape[-1]
    z = torch.cat([z, p["mask_token"].expand(n, 196 - L, Dd)], dim=1)
    z = _r(take(z, ids_restore) + p["decoder_pos_embed"], e)
    for i in range(dec_depth):
        z = _block(z, p, W, f"decoder_blocks.{i}", DEC_HEADS, le, e)
    z = _r(F.layer_norm(z, (Dd,), p["decoder_norm.weight"], p["decoder_norm.bias"], le), e)
    pred = _r(F.linear(z, W["decoder_pred.weight"], p["decoder_pred.bias"]), e)
    loss = mae_loss(images, pred, mask, norm_pix_loss)
    return dict(loss=loss, pred=pred, mask=mask, latent=latent, ids_restore=ids_restore)


def mae_loss(images, pred, mask, norm_pix_loss):
    target = patchify(images)
    if norm_pix_loss:
        mean = target.mean(dim=-1, keepdim=True)
        var = target.var(dim=-1, keepdim=True)                       # unbiased
        target = (target - mean) / (var + 1e-6) ** 0.5
    loss = ((pred - target) ** 2).mean(dim=-1)
    return (loss * mask).sum() / mask.sum()
