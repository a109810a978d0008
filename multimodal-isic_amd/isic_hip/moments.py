"""``token_moments``: the per-image descriptor of an encoder's token grid, the reference's ``concat_patch_moments``
(``utils.py:16-31``), in one launch.

``latent[B, T, D]`` fp32 -> ``[B, 6 D]`` fp32: mean, max, std, median, skewness and excess kurtosis of every channel over
the token axis, concatenated in that order.  ``isic_token_moments_f32`` (include/isic_hip_moments.h) reads the latent
once, stages one image's slab of channels in LDS and forms all six there; max and median are input elements (no rounding),
the median is the lower middle element of an even ``T`` as ``torch.median``.  There is no backward (the reference calls
the helper under ``no_grad``) and no CPU fallback.
"""
from __future__ import annotations

import torch

from .lib import IsicHipError, call

MAX_T = 1024                     # ISIC_MOMENTS_MAX_T
STATS = ("mean", "max", "std", "median", "skew", "kurtosis")


def token_moments(latent, eps=1e-6, unbiased=False):
    """latent [B, T, D] fp32 on the device -> [B, 6 D] fp32 (``STATS`` order), on the current stream.

    A latent whose tokens are ``ldx >= D`` floats apart (unit channel stride, images ``T ldx`` apart: a channel slice of a
    wider grid) is read in place; any other layout is made contiguous first."""
    if not isinstance(latent, torch.Tensor) or latent.dim() != 3:
        raise ValueError("token_moments: latent must be a 3-D tensor [B, T, D]")
    if latent.dtype != torch.float32:
        raise ValueError(f"token_moments: latent must be fp32, got {latent.dtype}")
    B, T, D = latent.shape
    if T < 1 or D < 1:
        raise ValueError("token_moments: T and D must be at least 1")
    if T > MAX_T:
        raise ValueError(f"token_moments: T = {T} exceeds {MAX_T} tokens")
    unbiased = bool(unbiased)
    if unbiased and T == 1:
        raise ValueError("token_moments: unbiased needs at least two tokens")
    if not float(eps) >= 0.0:
        raise ValueError("token_moments: eps must be non-negative")
    if latent.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("token_moments has no backward: call it under torch.no_grad() or on a detached tensor")
    if not latent.is_cuda:
        raise IsicHipError("token_moments: latent must be a device tensor (got a CPU tensor; there is no CPU fallback)")
    latent = latent.detach()
    sb, st, sd = latent.stride()
    if not ((sd == 1 or D == 1) and st >= D and (sb == T * st or B <= 1)):
        latent = latent.contiguous()
        st = D
    out = torch.empty((B, 6 * D), device=latent.device, dtype=torch.float32)
    if B > 0:
        with torch.cuda.device(latent.device):
            call("isic_token_moments_f32", latent.data_ptr(), B, T, D, st, float(eps), int(unbiased), out, 6 * D)
    return out
