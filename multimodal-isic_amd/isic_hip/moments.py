"""``token_moments``: the per-image descriptor of an encoder's token grid, the reference's ``concat_patch_moments``
(``utils.py:16-31``), in one launch.

``latent[B, T, D]`` fp32 -> ``[B, 6 D]`` fp32: mean, max, std, median, skewness and excess kurtosis of every channel over
the token axis, concatenated in that order.  ``isic_token_moments_f32`` (include/isic_hip_moments.h) reads the latent
once, stages one image's slab of channels in LDS and forms all six there; max and median are input elements (no rounding),
the median is the lower middle element of an even ``T`` as ``torch.median``.  There is no backward (the reference calls
the helper under ``no_grad``) and no CPU fallback.

The same descriptor over a SUBSET of each image's tokens -- the lesion patches -- comes from ``token_moments(latent,
keep=flags)`` (flags on the dense grid) and ``token_moments_ragged(x, offsets)`` (a compacted store), one launch each
(include/isic_hip_moments_ragged.h), bit-equal to the dense call on the kept tokens.
"""
from __future__ import annotations

import torch

from .lib import IsicHipError, call

MAX_T = 1024                     # ISIC_MOMENTS_MAX_T
STATS = ("mean", "max", "std", "median", "skew", "kurtosis")


MAX_NODES = 256                  # ISIC_MOMENTS_RAGGED_MAX_NODES: the token bound of the masked and ragged entries


def _check_eps(name, eps):
    if not float(eps) >= 0.0:
        raise ValueError(f"{name}: eps must be non-negative")


def _no_backward(name, x):
    if x.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{name} has no backward: call it under torch.no_grad() or on a detached tensor")


def _with_counts(out, counts, return_counts):
    return (out, counts) if return_counts else out


def token_moments(latent, eps=1e-6, unbiased=False, keep=None, return_counts=False):
    """latent [B, T, D] fp32 on the device -> [B, 6 D] fp32 (``STATS`` order), on the current stream.

    A latent whose tokens are ``ldx >= D`` floats apart (unit channel stride, images ``T ldx`` apart: a channel slice of a
    wider grid) is read in place; any other layout is made contiguous first.

    ``keep`` [B, T] (bool, or any integer or float dtype: non-zero keeps the token; on ``latent``'s device) restricts the
    statistics of image b to its kept tokens, in one ``isic_token_moments_masked_f32`` launch (T <= 256): bit for bit what the
    call without ``keep`` gives on ``latent[b:b+1, keep[b]]``.  An image without a kept token gets a NaN row; one kept token
    with ``unbiased`` gives NaN std, skewness and kurtosis (as torch).  ``return_counts``: also the int32 [B] numbers of kept
    tokens (``T`` everywhere without ``keep``)."""
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
    if keep is not None:
        if not isinstance(keep, torch.Tensor) or tuple(keep.shape) != (B, T):
            raise ValueError(f"token_moments: keep must be a tensor of shape [B, T] = [{B}, {T}]")
        if keep.is_complex():
            raise ValueError(f"token_moments: keep must be bool, integer or float, got {keep.dtype}")
        if T > MAX_NODES:
            raise ValueError(f"token_moments: T = {T} exceeds the {MAX_NODES} tokens of the masked entry")
        if keep.device != latent.device:
            raise ValueError(f"token_moments: keep is on {keep.device}, latent on {latent.device}")
    elif unbiased and T == 1:
        raise ValueError("token_moments: unbiased needs at least two tokens")
    _check_eps("token_moments", eps)
    _no_backward("token_moments", latent)
    if not latent.is_cuda:
        raise IsicHipError("token_moments: latent must be a device tensor (got a CPU tensor; there is no CPU fallback)")
    latent = latent.detach()
    sb, st, sd = latent.stride()
    if not ((sd == 1 or D == 1) and st >= D and (sb == T * st or B <= 1)):
        latent = latent.contiguous()
        st = D
    out = torch.empty((B, 6 * D), device=latent.device, dtype=torch.float32)
    if keep is None:
        if B > 0:
            with torch.cuda.device(latent.device):
                call("isic_token_moments_f32", latent.data_ptr(), B, T, D, st, float(eps), int(unbiased), out, 6 * D)
        counts = torch.full((B,), T, device=latent.device, dtype=torch.int32) if return_counts else None
        return _with_counts(out, counts, return_counts)
    # the kernel keeps a token whose byte is non-zero: bool and uint8 flags go in as they are (no launch), others through `!= 0`
    flags = keep if keep.dtype in (torch.bool, torch.uint8) else keep != 0
    flags = flags.detach().contiguous().view(torch.uint8)
    counts = torch.empty((B,), device=latent.device, dtype=torch.int32) if return_counts else None
    if B > 0:
        with torch.cuda.device(latent.device):
            call("isic_token_moments_masked_f32", latent.data_ptr(), flags, B, T, D, st, float(eps), int(unbiased), out,
                 6 * D, counts)
    return _with_counts(out, counts, return_counts)


def token_moments_ragged(x, offsets, eps=1e-6, unbiased=False, max_nodes=None, return_counts=False):
    """x [total, D] fp32 on the device, offsets int64 [G + 1] (host or device): graph g owns rows
    ``offsets[g]:offsets[g + 1]`` -> [G, 6 D] fp32, row g bit for bit ``token_moments(x[None, offsets[g]:offsets[g + 1]])``, in
    one ``isic_token_moments_ragged_f32`` launch; the NaN conventions of ``token_moments`` with ``keep`` for graphs of 0 or 1
    rows.  ``max_nodes`` (<= 256) bounds the rows of a graph; None takes it from the offsets (a read-back when they are on the
    device -- the only one).  Offsets that decrease, leave ``[0, total]`` or span more than ``max_nodes`` raise
    ``IsicHipError`` after the call.  ``return_counts``: also the int32 [G] row counts."""
    name = "token_moments_ragged"
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f"{name}: x must be a 2-D tensor [total, D]")
    if x.dtype != torch.float32:
        raise ValueError(f"{name}: x must be fp32, got {x.dtype}")
    total, D = x.shape
    if D < 1:
        raise ValueError(f"{name}: D must be at least 1")
    if not isinstance(offsets, torch.Tensor):
        offsets = torch.as_tensor(offsets)
    if offsets.dim() != 1 or offsets.numel() < 1 or offsets.dtype != torch.int64:
        raise ValueError(f"{name}: offsets must be int64 [G + 1], got {offsets.dtype} {tuple(offsets.shape)}")
    G = offsets.numel() - 1
    if max_nodes is None:
        host = offsets.cpu()                                                    # the one read-back (device offsets only)
        max_nodes = int((host[1:] - host[:-1]).max()) if G > 0 else 0
        max_nodes = max(max_nodes, 0)                                           # decreasing offsets: the kernel reports them
    max_nodes = int(max_nodes)
    if max_nodes < 0:
        raise ValueError(f"{name}: max_nodes must be non-negative")
    if max_nodes > MAX_NODES:
        raise ValueError(f"{name}: max_nodes = {max_nodes} exceeds {MAX_NODES} rows per graph")
    _check_eps(name, eps)
    _no_backward(name, x)
    if not x.is_cuda:
        raise IsicHipError(f"{name}: x must be a device tensor (got a CPU tensor; there is no CPU fallback)")
    x = x.detach()
    st, sd = x.stride()
    if not ((sd == 1 or D == 1) and st >= D):
        x = x.contiguous()
        st = D
    offsets = offsets.to(x.device).contiguous()
    out = torch.empty((G, 6 * D), device=x.device, dtype=torch.float32)
    counts = torch.empty((G,), device=x.device, dtype=torch.int32) if return_counts else None
    if G > 0:
        bad = torch.zeros(1, device=x.device, dtype=torch.int32)
        with torch.cuda.device(x.device):
            call("isic_token_moments_ragged_f32", x.data_ptr() if total else None, offsets, G, max_nodes, total, D, st,
                 float(eps), int(bool(unbiased)), out, 6 * D, counts, bad)
        nbad = int(bad.item())
        if nbad:
            raise IsicHipError(f"{name}: {nbad} graph(s) with offsets that decrease, leave [0, {total}] or span more than "
                               f"max_nodes = {max_nodes} rows")
    return _with_counts(out, counts, return_counts)
