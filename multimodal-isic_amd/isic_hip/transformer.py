"""The training path of a stack of pre-norm transformer blocks, fp16 on gfx950 -- shared by ``ViTSmallEncoder``
(isic_hip/vit.py), ``ConvMAEBaseEncoder`` (blocks3, isic_hip/convmae.py) and the MAE decoder (isic_hip/convmae_mae.py).

A block is x2 = x + proj(attention(qkv(LN1(x)))), out = x2 + fc2(GELU(fc1(LN2(x2)))) with timm's parameter names
(``BLOCK_PARAMS``).  A stack is described by ``spec = dict(prefix, T, D, H, eps, total)``: the blocks are ``prefix.i``,
i < total, in the weight dict ``w``; T tokens per image, width D, H heads of 64 (``isic_attention_f16``) or 32
(``isic_attention_d32_f16``), LayerNorm eps; the MLP width is fc1's.  The stream is fp16 rows [n * T, D].

Forward: ``isic_layernorm_add_f16`` (the ViT-S/16 hands in ``isic_layernorm_f16``, its frozen forward's kernel: the two are
the same two-pass arithmetic, but the compiler fuses the mean subtraction and the first squares into FMAs in one and not
in the other, and their outputs differ in the last bit), ``isic_gemm_f16`` (residual in the epilogue), the attention, and
``isic_gemm_f16_gelu_pre`` for fc1.  It saves per block x, LN1(x), qkv, the attention output, x2, LN2(x2), fc1's
pre-activation and GELU output (fp16), and no LayerNorm statistics: ``isic_layernorm_add_bwd_f16`` recomputes (mean, rstd)
from x in fp32.

Backward: on gradients multiplied by a power-of-two loss scale S (``loss_scale``); every reduction into a parameter
gradient multiplies by s = 1/S in fp32 and accumulates into ``param.grad`` (``Backward``), so gradients are exactly
scale-equivariant.  An fp16 overflow is not retried: ``check_grads`` looks at the gradients once at the end.  No CPU
fallback.
"""
from __future__ import annotations

import math

import torch

from .lib import call

_F16 = torch.float16

# a block's parameters in registration order (norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2)
BLOCK_PARAMS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def _attention(qkv, att, n, T, H, hd):
    if hd == 64:
        call("isic_attention_f16", qkv, att, n, T, H, hd)
    else:
        call("isic_attention_d32_f16", qkv, att, n, T, H)


def _attention_bwd(qkv, att, dout, dqkv, n, T, H, hd):
    if hd == 64:
        call("isic_attention_bwd_f16", qkv, att, dout, dqkv, n, T, H, hd)
    else:
        call("isic_attention_d32_bwd_f16", qkv, att, dout, dqkv, n, T, H)


def layernorm_add(x, gamma, beta, y, M, D, eps):
    call("isic_layernorm_add_f16", x, None, None, gamma, beta, y, None, M, D, 0, eps)


def blocks_forward_train(w, x, n, nblk, spec, layernorm=layernorm_add):
    """The first ``nblk`` blocks of the stack over the stream x[n * T, D] -> (the output stream, the saved activations per
    block).  ``layernorm(x, gamma, beta, y, M, D, eps)`` is the pre-norm pass: a caller whose frozen forward runs another
    LayerNorm kernel hands that one in, so that the training forward stays that forward bit for bit."""
    dev = x.device
    T, D, H, eps = spec["T"], spec["D"], spec["H"], spec["eps"]
    M = n * T
    saves = []
    for i in range(nblk):
        b = f"{spec['prefix']}.{i}"
        Hd = w[b + ".mlp.fc1.weight"].shape[0]
        h1, att, x2, h2, xo = (torch.empty((M, D), device=dev, dtype=_F16) for _ in range(5))
        qkv = torch.empty((M, 3 * D), device=dev, dtype=_F16)
        pre, hid = (torch.empty((M, Hd), device=dev, dtype=_F16) for _ in range(2))
        layernorm(x, w[b + ".norm1.weight"], w[b + ".norm1.bias"], h1, M, D, eps)
        call("isic_gemm_f16", h1, w[b + ".attn.qkv.weight"], w[b + ".attn.qkv.bias"], None, qkv, M, 3 * D, D, 0, 0)
        _attention(qkv, att, n, T, H, D // H)
        call("isic_gemm_f16", att, w[b + ".attn.proj.weight"], w[b + ".attn.proj.bias"], x, x2, M, D, D, 0, 0)
        layernorm(x2, w[b + ".norm2.weight"], w[b + ".norm2.bias"], h2, M, D, eps)
        call("isic_gemm_f16_gelu_pre", h2, w[b + ".mlp.fc1.weight"], w[b + ".mlp.fc1.bias"], hid, pre, M, Hd, D)
        call("isic_gemm_f16", hid, w[b + ".mlp.fc2.weight"], w[b + ".mlp.fc2.bias"], x2, xo, M, D, Hd, 0, 0)
        saves.append(dict(x=x, h1=h1, qkv=qkv, att=att, x2=x2, h2=h2, pre=pre, hid=hid))
        x = xo
    return x, saves


def blocks_workspace_bytes(w, n, spec):
    """What ``blocks_backward`` needs of ``Backward.ws``: the four weight gradients (with their bias column sums) and the
    LayerNorm backward of one block."""
    M, D = n * spec["T"], spec["D"]
    Hd = w[f"{spec['prefix']}.0.mlp.fc1.weight"].shape[0]
    nb = call("isic_layernorm_add_bwd_f16_workspace_bytes", M, D)
    for nk in ((3 * D, D), (D, D), (Hd, D), (D, Hd)):
        nb = max(nb, call("isic_gemm_f16_wgrad_workspace_bytes", M, *nk))
    return nb


def param_grads(module, rename=None):
    """-> grad(name): the fp32 ``.grad`` of the module's parameter ``name`` (``rename(name)`` if it registers it under
    another), created as zeros on first use."""
    params = dict(module.named_parameters())

    def grad(name):
        p = params[rename(name) if rename else name]
        if p.grad is None:
            p.grad = torch.zeros_like(p.data)
        return p.grad
    return grad


class Backward:
    """What one backward call shares between its layers: ``w`` the fp16 weight dict of the forward (with the ``.t``
    transposes), ``grad(name)`` the caller's lookup of a parameter's fp32 ``.grad`` (created on demand), ``s`` the factor of
    every parameter-gradient reduction, ``ws`` the workspace of their slabs (at least ``nbytes``; kept on ``owner._ws``
    between calls)."""

    def __init__(self, owner, w, grad, s, nbytes, device):
        ws = owner._ws
        if ws is None or ws.numel() < nbytes or ws.device != device:
            ws = owner._ws = torch.empty(max(int(nbytes), 16), device=device, dtype=torch.uint8)
        self.w, self.grad, self.s, self.ws = w, grad, s, ws

    def wgrad(self, dy, x, name, Nout, K, M):
        """``name``.weight += s dy^T x, ``name``.bias += s colsum(dy)"""
        call("isic_gemm_f16_wgrad", dy, x, self.grad(name + ".weight"), self.grad(name + ".bias"), M, Nout, K, self.s, 1,
             self.ws, self.ws.numel())

    def ln_add(self, dy, dy_f32, mul, x, a, b, norm, act, eps, g_in, g_out, g16, M, N):
        """Backward of act(LayerNorm ``norm`` of (x + a + b)) from dy * mul: g_out (fp32) / g16 = g_in + d loss / d x"""
        call("isic_layernorm_add_bwd_f16", dy, dy_f32, mul, x, a, b, self.w[norm + ".weight"], self.w[norm + ".bias"], act, eps,
             g_in, g_out, g16, self.grad(norm + ".weight"), self.grad(norm + ".bias"), M, N, self.s, 1, self.ws, self.ws.numel())

    def colsum(self, x, name, rows, cols):
        """``name`` += s colsum(x[rows, cols])"""
        call("isic_colsum_f16", x, self.grad(name), rows, cols, self.s, 1, self.ws, self.ws.numel())


def blocks_backward(saves, g, gh, bw, n, nblk, spec, fire):
    """Backward of ``blocks_forward_train``: g (fp32) / gh (its fp16 copy), the gradient of the output stream, become those
    of the input stream (in place); ``saves[i]`` is dropped once block i is done.  ``fire(names)`` is told the parameters
    of each finished block (``prefix.i.`` + ``BLOCK_PARAMS``), from the last block back."""
    dev, w = g.device, bw.w
    T, D, H, eps = spec["T"], spec["D"], spec["H"], spec["eps"]
    M = n * T

    def names(i):
        return [f"{spec['prefix']}.{i}.{k}" for k in BLOCK_PARAMS]
    for i in range(spec["total"] - 1, nblk - 1, -1):                    # blocks past ``nblk`` ran not: no gradient
        fire(names(i))
    Hd = w[f"{spec['prefix']}.0.mlp.fc1.weight"].shape[0]
    dmid = torch.empty((M, Hd), device=dev, dtype=_F16)
    dD = torch.empty((M, D), device=dev, dtype=_F16)
    dqkv = torch.empty((M, 3 * D), device=dev, dtype=_F16)
    for i in range(nblk - 1, -1, -1):
        b, sv = f"{spec['prefix']}.{i}", saves[i]
        bw.wgrad(gh, sv["hid"], f"{b}.mlp.fc2", D, Hd, M)
        call("isic_gemm_f16_dgelu", gh, w[f"{b}.mlp.fc2.weight.t"], sv["pre"], dmid, M, Hd, D)
        bw.wgrad(dmid, sv["h2"], f"{b}.mlp.fc1", Hd, D, M)
        call("isic_gemm_f16", dmid, w[f"{b}.mlp.fc1.weight.t"], None, None, dD, M, D, Hd, 0, 0)
        bw.ln_add(dD, 0, 1.0, sv["x2"], None, None, f"{b}.norm2", 0, eps, g, g, gh, M, D)
        bw.wgrad(gh, sv["att"], f"{b}.attn.proj", D, D, M)
        call("isic_gemm_f16", gh, w[f"{b}.attn.proj.weight.t"], None, None, dD, M, D, D, 0, 0)
        _attention_bwd(sv["qkv"], sv["att"], dD, dqkv, n, T, H, D // H)
        bw.wgrad(dqkv, sv["h1"], f"{b}.attn.qkv", 3 * D, D, M)
        call("isic_gemm_f16", dqkv, w[f"{b}.attn.qkv.weight.t"], None, None, dD, M, D, 3 * D, 0, 0)
        bw.ln_add(dD, 0, 1.0, sv["x"], None, None, f"{b}.norm1", 0, eps, g, g, gh, M, D)
        saves[i] = None                                  # its activations can go
        fire(names(i))


def loss_scale(dtok, who):
    """-> (dtok as contiguous fp32, S = 2^round(8 - log2 amax |dtok|)); one device -> host read."""
    dtok = dtok.float().contiguous()
    amax = float(dtok.abs().amax())
    if not math.isfinite(amax):
        raise FloatingPointError(f"{who} backward: the incoming gradient is not finite")
    return dtok, (2.0 ** round(8 - math.log2(amax)) if amax > 0 else 1.0)


def check_grads(params, who):
    """The backward's final check: one device -> host read over the norms of every gradient there is."""
    norms = torch._foreach_norm([p.grad for p in params if p.grad is not None])
    if not bool(torch.isfinite(torch.stack(norms)).all()):
        raise FloatingPointError(f"{who} backward: non-finite parameter gradient (fp16 overflow in the backward, or a "
                                 "non-finite gradient accumulated earlier)")


class EncoderFn(torch.autograd.Function):
    """Autograd edge: tokens -> encoder parameter gradients, for an encoder with ``run_forward_train(images, *args) ->
    (tokens, tape)`` and ``run_backward(tape, dtok)``.  The parameters are passed as inputs only so that autograd schedules
    this node; the kernels accumulate their gradients in place (``param.grad``), hence ``None`` is returned (the images get
    none either: a patch embedding has no data gradient)."""

    @staticmethod
    def forward(ctx, images, enc, args, *params):
        tok, tape = enc.run_forward_train(images, *args)
        ctx.enc, ctx.tape = enc, tape
        return tok

    @staticmethod
    def backward(ctx, dtok):
        enc, tape = ctx.enc, ctx.tape
        ctx.tape = None
        enc.run_backward(tape, dtok)
        return (None, None, None) + tuple(None for _ in enc.parameters())
