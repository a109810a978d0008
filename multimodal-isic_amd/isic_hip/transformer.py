"""A stack of pre-norm transformer blocks, fp16 on gfx950: its one forward (inference and training) and its backward --
shared by ``ViTSmallEncoder`` (isic_hip/vit.py), ``ConvMAEBaseEncoder`` (blocks3, isic_hip/convmae.py) and the MAE decoder
(isic_hip/convmae_mae.py).

A block is x2 = x + proj(attention(qkv(LN1(x)))), out = x2 + fc2(GELU(fc1(LN2(x2)))) with timm's parameter names
(``BLOCK_PARAMS``).  A stack is described by ``spec = dict(prefix, T, D, H, eps, total)``: the blocks are ``prefix.i``,
i < total, in the weight dict ``w``; T tokens per image, width D, H heads of 64 (``isic_attention_f16``) or 32
(``isic_attention_d32_f16``), LayerNorm eps; the MLP width is fc1's.  The stream is fp16 rows [n * T, D].

Forward (``blocks_forward``), layer by layer: ``isic_layernorm_add_f16`` (the ViT-S/16 hands in ``isic_layernorm_f16``, its
frozen forward's kernel.  The fp16 row LayerNorm kernels share one source text, csrc/ln_rows.inc: the same sums in the same
order, with two mean rules -- s * (1 / N) in the ViT-width kernels, s / N in the ``layernorm_add`` family -- and the
compiler contracts multiply-adds per kernel, so two kernels' statistics may differ in the last bit; DESIGN.md section 4,
and tests/test_ln_rows_gpu.py pins the bits of each), ``isic_gemm_f16`` (residual in the epilogue; GELU for fc1) and
the attention.  ``fold``: the pre-norms have no pass of their own (``isic_gemm_f16_ln`` on row statistics from
``isic_gemm_f16_stats`` or ``isic_row_stats_f16``; isic_hip/vit.py has the algebra, ``fold_layernorm`` the weights).
``save`` (training): fc1 through ``isic_gemm_f16_gelu_pre``, and per block x, LN1(x), qkv, the attention output, x2,
LN2(x2), fc1's pre-activation and GELU output (fp16) are kept, and no LayerNorm statistics:
``isic_layernorm_add_bwd_f16`` recomputes (mean, rstd) from x in fp32.

MXFP8 forward (``blocks_forward_mx``, inference; ``mx_weights`` quantises the matrices): the four products of a block on
``isic_gemm_mxfp8``, each operand written as MXFP8 by the launch before it -- LN -> MX, qkv (fp16 out), attention,
``isic_mxfp8_quantize``, proj + residual (fp16 out), LN -> MX, fc1 + GELU -> MX, fc2 + residual (fp16 out); the residual
stream stays fp16.  isic_hip/vit.py says why the LayerNorm is never folded here.

Backward: on gradients multiplied by a power-of-two loss scale S (``loss_scale``); every reduction into a parameter
gradient multiplies by s = 1/S in fp32 and accumulates into ``param.grad`` (``Backward``), so gradients are exactly
scale-equivariant.  An fp16 overflow is not retried: ``check_grads`` looks at the gradients once at the end.  No CPU
fallback.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from .lib import IsicHipError, call

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


def fold_layernorm(w, W, norm, lin):
    """LayerNorm ``norm`` folded into the product ``lin`` that follows it (isic_hip/vit.py has the algebra), from the fp32
    master W of ``lin``: W' = W diag(gamma) in fp16, c from the ROUNDED W' (it has to cancel what the MFMAs sum),
    b' = b + W beta in fp32."""
    W = W.float().reshape(W.shape[0], -1)
    Wg = (W * w[norm + ".weight"][None, :]).to(_F16).contiguous()
    w[lin + ".ln_weight"] = Wg
    w[lin + ".ln_c"] = Wg.float().sum(dim=1).contiguous()
    w[lin + ".ln_bias"] = (w[lin + ".bias"] + W @ w[norm + ".bias"]).contiguous()


def linear_res(w, a, name, res, out, st, fold, eps, res_rows=0):
    """out = a . W^T + b + res (``res_rows`` > 0: res repeats every ``res_rows`` rows) and, into ``st``, the LayerNorm
    statistics of out's rows for the product that reads it: partial sums per 64-column group out of the epilogue
    (``fold`` True), or (mean, rstd) from a statistics-only pass (``"stats"``)."""
    (M, K), N = a.shape, out.shape[1]
    if fold is True:
        call("isic_gemm_f16_stats", a, w[name + ".weight"], w[name + ".bias"], res, out, st, M, N, K, 0, res_rows)
    else:
        call("isic_gemm_f16", a, w[name + ".weight"], w[name + ".bias"], res, out, M, N, K, 0, res_rows)
        if fold == "stats":
            call("isic_row_stats_f16", out, st, M, N, eps)


def linear_ln(w, xin, st, parts, norm, name, h, out, act, eps, layernorm=layernorm_add, pre=None):
    """out = act(LayerNorm ``norm`` (xin) . W^T + b).  With xin's row statistics ``st`` (``parts`` partial sums per row; 0:
    (mean, rstd)) the LayerNorm is folded into the product; ``st`` None: a ``layernorm`` pass into h and a plain product,
    which also leaves fc1's pre-activation in ``pre`` if given (for the backward)."""
    (M, K), Nout = xin.shape, out.shape[1]
    if st is not None:
        call("isic_gemm_f16_ln", xin, w[name + ".ln_weight"], w[name + ".ln_bias"], w[name + ".ln_c"], st, parts, out, M, Nout,
             K, act, eps)
        return
    layernorm(xin, w[norm + ".weight"], w[norm + ".bias"], h, M, K, eps)
    if pre is not None:
        call("isic_gemm_f16_gelu_pre", h, w[name + ".weight"], w[name + ".bias"], out, pre, M, Nout, K)
    else:
        call("isic_gemm_f16", h, w[name + ".weight"], w[name + ".bias"], None, out, M, Nout, K, act, 0)


def embed(w, a, name, spec, fold):
    """The product that writes the stream ahead of block 0: a . ``name``^T + b + pos_embed -> (the stream, its row
    statistics for ``blocks_forward``: None when ``fold`` is False)."""
    M, D = a.shape[0], spec["D"]
    x = torch.empty((M, D), device=a.device, dtype=_F16)
    st = None
    if fold is not False:
        st = torch.empty((M, 2 * D // 128 if fold is True else 1, 2), device=a.device, dtype=torch.float32)
    linear_res(w, a, name, w["pos_embed"], x, st, fold, spec["eps"], res_rows=w["pos_embed"].shape[0])
    return x, st


def blocks_forward(w, x, st, n, nblk, spec, fold=False, save=False, layernorm=layernorm_add):
    """The first ``nblk`` blocks of the stack over the stream x[n * T, D] -> (the output stream, the saved activations per
    block).  ``fold`` False: the layer-by-layer form; True / ``"stats"``: the pre-norms folded into qkv and fc1
    (``fold_layernorm``), on the row statistics ``st`` of x that the product which wrote x left (``embed``).  ``save``
    False (inference): the stream ping-pongs between x and one second buffer, every block reuses one LN / qkv /
    attention / hidden buffer, and x is overwritten.  ``save`` True (training; the layer-by-layer form only): fresh
    tensors per block, fc1 through ``isic_gemm_f16_gelu_pre``, x is kept.  ``layernorm(x, gamma, beta, y, M, D, eps)`` is
    the pre-norm pass: a caller whose frozen forward runs another LayerNorm kernel hands that one in."""
    if save and fold is not False:
        raise ValueError("blocks_forward: save=True runs the layer-by-layer form (fold=False)")
    dev = x.device
    T, D, H, eps = spec["T"], spec["D"], spec["H"], spec["eps"]
    M = n * T
    parts = 2 * D // 128 if fold is True else 0
    st2 = torch.empty_like(st) if fold is not False else None

    def e16(cols):
        return torch.empty((M, cols), device=dev, dtype=_F16)

    saves = []
    for i in range(nblk):
        b = f"{spec['prefix']}.{i}"
        Hd = w[b + ".mlp.fc1.weight"].shape[0]
        if save or i == 0:
            h1, qkv, att, x2, hid = e16(D) if fold is False else None, e16(3 * D), e16(D), e16(D), e16(Hd)
        h2, pre, xo = (e16(D), e16(Hd), e16(D)) if save else (h1, None, x)
        linear_ln(w, x, st, parts, b + ".norm1", b + ".attn.qkv", h1, qkv, 0, eps, layernorm)
        _attention(qkv, att, n, T, H, D // H)
        linear_res(w, att, b + ".attn.proj", x, x2, st2, fold, eps)
        linear_ln(w, x2, st2, parts, b + ".norm2", b + ".mlp.fc1", h2, hid, 1, eps, layernorm, pre)
        linear_res(w, hid, b + ".mlp.fc2", x2, xo, st, fold, eps)
        if save:
            saves.append(dict(x=x, h1=h1, qkv=qkv, att=att, x2=x2, h2=h2, pre=pre, hid=hid))
        x = xo
    return x, saves


def mx_weights(named_matrices, device):
    """{name: (q, s)} of the [R, K] fp32 matrices ``named_matrices`` yields as (name, matrix), quantised on the GPU
    (``isic_mxfp8_quantize``: q[R, K] e4m3 bytes, s[R, K / 32] scale bytes).  Once per weight version: the caller keeps
    the key."""
    out = {}
    for name, t in named_matrices:
        t = t.detach().float().contiguous()
        R, K = t.shape
        q = torch.empty((R, K), device=device, dtype=torch.uint8)
        s = torch.empty((R, K // 32), device=device, dtype=torch.uint8)
        call("isic_mxfp8_quantize", t, 1, q, s, R, K)
        out[name] = (q, s)
    return out


def blocks_forward_mx(w, wmx, x, n, nblk, spec, layernorm_mx):
    """The first ``nblk`` blocks over the fp16 stream x[n * T, D] with their products on the block-scaled FP8 MFMA (module
    docstring) -> the output stream.  ``w``: the biases and LayerNorm affines, ``wmx``: ``mx_weights`` of the four
    matrices of every block.  The stream ping-pongs between x and one second buffer, every block reuses one MX operand /
    qkv / attention / MX hidden buffer, and x is overwritten.  ``layernorm_mx(x, gamma, beta, q, s, M, D, eps)`` is the
    LayerNorm -> MXFP8 pass, handed in as ``layernorm`` is for ``blocks_forward``."""
    dev = x.device
    T, D, H, eps = spec["T"], spec["D"], spec["H"], spec["eps"]
    M = n * T

    def mx(cols):
        return (torch.empty((M, cols), device=dev, dtype=torch.uint8), torch.empty((M, cols // 32), device=dev, dtype=torch.uint8))

    def gemm(a, name, Nout, K, act=0, res=None, out=None, out_mx=(None, None)):
        wq, ws = wmx[name + ".weight"]
        call("isic_gemm_mxfp8", a[0], a[1], wq, ws, w[name + ".bias"], res, out, out_mx[0], out_mx[1], M, Nout, K, act, 0)

    for i in range(nblk):
        b = f"{spec['prefix']}.{i}"
        Hd = wmx[b + ".mlp.fc1.weight"][0].shape[0]
        if i == 0:
            h, hid = mx(D), mx(Hd)
            qkv, att, x2 = (torch.empty((M, c), device=dev, dtype=_F16) for c in (3 * D, D, D))
        layernorm_mx(x, w[b + ".norm1.weight"], w[b + ".norm1.bias"], h[0], h[1], M, D, eps)
        gemm(h, b + ".attn.qkv", 3 * D, D, out=qkv)
        _attention(qkv, att, n, T, H, D // H)
        call("isic_mxfp8_quantize", att, 0, h[0], h[1], M, D)
        gemm(h, b + ".attn.proj", D, D, res=x, out=x2)
        layernorm_mx(x2, w[b + ".norm2.weight"], w[b + ".norm2.bias"], h[0], h[1], M, D, eps)
        gemm(h, b + ".mlp.fc1", Hd, D, act=1, out_mx=hid)
        gemm(hid, b + ".mlp.fc2", D, Hd, res=x2, out=x)
    return x


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
    """Backward of ``blocks_forward(save=True)``: g (fp32) / gh (its fp16 copy), the gradient of the output stream, become those
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


class Encoder(nn.Module):
    """What the fp16 patch encoders share: frozen unless ``trainable``, images[N, in_ch, img_size, img_size] on the GPU."""

    def train(self, mode=True):
        if mode and not self.trainable:
            raise IsicHipError(f"{self._who} is a frozen inference encoder (save_latent.py:51-53): no train() mode")
        return super().train(mode)

    def _check_images(self, images):
        if images.dim() != 4 or tuple(images.shape[1:]) != (self.in_ch, self.img_size, self.img_size):
            raise ValueError(f"expected images[N,{self.in_ch},{self.img_size},{self.img_size}], got {tuple(images.shape)}")
        if not images.is_cuda:
            raise IsicHipError(f"{self._who} runs on the MI355X only (no CPU fallback)")

    def _check_device(self, params, device):
        if any(p.device != device for p in params):
            raise IsicHipError(f"{self._who}: move the module to the GPU first (.to('cuda'))")


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
