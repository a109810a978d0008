"""The ConvMAE-Base masked autoencoder, fp16 on gfx950 -- the model the reference's ``train_ae.py`` fine-tunes.

``ConvMAEBase`` is the encoder of isic_hip/convmae.py (``ConvMAEBaseEncoder(trainable=True)``, whose keys it keeps at the
top level, as in a checkpoint) plus random masking, the 8-block decoder and the pixel-reconstruction loss.  This restates
the published ConvMAE code (Gao et al. 2022, ``models_convmae.py`` / ``vision_transformer.py``), which neither the
reference nor this tree vendors: PARITY IS UNPINNED.  ``tests/convmae_mae_ref.py`` is the torch-CPU restatement the tests
check it against.

1. Masking.  ``noise[N, 196]`` is the caller's or ``torch.rand``; ids_shuffle = argsort(noise, 1), ids_restore =
   argsort(ids_shuffle, 1), len_keep = int(196 (1 - mask_ratio)), ids_keep = ids_shuffle[:, :len_keep]; mask[N, 196] is
   1 for a removed token, in raster order.  0 <= mask_ratio < 1 and len_keep >= 1, else ValueError.  mask_ratio == 0
   without noise: the identity (raster order), the encoder's convention.  This index bookkeeping stays in torch.
2. Stages 1-2.  A token covers 4 x 4 pixels at 56 x 56 and 2 x 2 at 28 x 28; each CBlock multiplies conv1's output by
   keep = 1 - mask, upsampled to the pixel grid, before the depthwise 5x5: x += conv2(dw5x5(keep * conv1(LN1(x)))); the
   MLP half is unchanged.
3. Stage 3.  patch_embed3 -> patch_embed4 + pos_embed; the ids_keep rows of that stream and of the stage outputs s1, s2
   are gathered; blocks3 runs on len_keep tokens; latent = norm(x + s1 + s2) -> [N, len_keep, 768] in ids_keep order.
4. Decoder.  decoder_embed Linear 768 -> 512; 196 - len_keep copies of mask_token [1, 1, 512] appended; unshuffled by
   ids_restore; + decoder_pos_embed [1, 196, 512] (MAE's fixed 2-D sin-cos table at width 512, requires_grad=False; a
   checkpoint's value overrides it); decoder_blocks.0-7: timm pre-norm blocks of width 512, 16 heads of 32 (softmax
   scale 32^-0.5), qkv bias, MLP 2048, erf-GELU, LayerNorm eps 1e-6; decoder_norm (eps 1e-6); decoder_pred Linear
   512 -> 768 -> pred[N, 196, 768] (returned fp32).
5. Loss.  target = patchify(images), p = 16, a patch's values in (row, column, channel) order (einsum
   'nchpwq->nhwpqc'); with ``norm_pix_loss`` (t - mean) / sqrt(var + 1e-6) per patch, var unbiased;
   loss = sum_t mask_t mean_c (pred - target)^2 / sum_t mask_t.
6. ``lesion_mask``: the reference's fork adds this argument (train_ae.py), but its meaning is in no tree we have: any
   value other than None raises ValueError.

Launches: the encoder's (isic_hip/convmae.py) with ``isic_dwconv5x5_masked_f16`` in the CBlocks and
``isic_gather_rows_f16`` into blocks3; ``isic_mae_unshuffle_f16`` for the mask tokens and the position embedding; the
decoder blocks through the encoder's own ``transformer.blocks_forward`` with ``isic_attention_d32_f16``;
``isic_mae_loss_f16`` for the target, the loss and d loss / d pred in one pass.  No CPU fallback.

Training: ``loss.backward()`` runs one native backward (include/isic_hip_mae.h + the encoder's) that accumulates into
every ``param.grad``.  The loss kernel writes d loss / d pred already multiplied by the power-of-two loss scale
S = 2^(round(log2(768 * sum(mask))) + 4), so that its entries are about 32 (pred - target) -- unscaled they are
2 (pred - target) / (768 * sum(mask)), below the fp16 normal range at a few hundred images.  S needs no device -> host
read (sum(mask) = N (196 - len_keep)); every reduction into a parameter gradient multiplies by dloss / S in fp32 (the one
host read is the incoming dloss, 1 after ``loss.backward()``).  An fp16 overflow is not retried: the backward checks
the gradients once at its end and raises ``FloatingPointError``.  ``grad_ready_hook`` reports the decoder first
(decoder_pred + decoder_norm, each decoder block from the last back, then decoder_embed + mask_token +
decoder_pos_embed), then the encoder in its own order (ConvMAEBaseEncoder.run_backward): every parameter once.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from .convmae import ConvMAEBaseEncoder, _Block, _F16, sincos_pos_embed
from .lib import IsicHipError, call
from .transformer import Backward, blocks_backward, blocks_forward, blocks_workspace_bytes, check_grads, param_grads


class ConvMAEBase(ConvMAEBaseEncoder):
    """ConvMAE-Base encoder + decoder + reconstruction loss (module docstring).  Trainable; the encoder's parameters are
    those of ``ConvMAEBaseEncoder(seed=seed, trainable=True)`` exactly."""

    dec_dim, dec_depth, dec_heads, patch = 512, 8, 16, 16

    def __init__(self, norm_pix_loss=False, seed=0, ln_eps=1e-6, conv_ln_eps=1e-5):
        super().__init__(seed=seed, ln_eps=ln_eps, conv_ln_eps=conv_ln_eps, trainable=True)
        D, Dd, T = self.dims[2], self.dec_dim, self.tokens
        if Dd % self.dec_heads or Dd // self.dec_heads != 32:
            raise ValueError("ConvMAEBase: decoder head width 32 (isic_attention_d32_f16)")
        self.norm_pix_loss = bool(norm_pix_loss)
        self.pred_dim = self.patch * self.patch * self.in_ch
        self.decoder_embed = nn.Linear(D, Dd)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, Dd))
        self.decoder_pos_embed = nn.Parameter(torch.from_numpy(sincos_pos_embed(Dd, self.grids[2])).float().unsqueeze(0),
                                              requires_grad=False)
        self.decoder_blocks = nn.ModuleList([_Block(Dd, Dd * self.mlp_ratio, ln_eps) for _ in range(self.dec_depth)])
        self.decoder_norm = nn.LayerNorm(Dd, eps=ln_eps)
        self.decoder_pred = nn.Linear(Dd, self.pred_dim)
        self._seeded_init_decoder(seed)
        self.eval()

    def _decoder_params(self):
        return [(k, p) for k, p in self.named_parameters() if k.startswith("decoder") or k == "mask_token"]

    def _seeded_init_decoder(self, seed):
        """As the encoder's ``_seeded_init`` (weights N(0, 1/fan_in), biases 0, LayerNorm (1, 0)) from a generator seeded
        with seed + 1; mask_token N(0, 0.02^2) as in MAE; decoder_pos_embed keeps the sin-cos table."""
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name, p in self._decoder_params():
                if name == "decoder_pos_embed":
                    continue
                if name == "mask_token":
                    p.copy_(0.02 * torch.randn(p.shape, generator=g))
                elif p.dim() == 1:
                    p.fill_(1.0 if "norm" in name and name.endswith(".weight") else 0.0)
                else:
                    p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p[0].numel()))

    def _prepare(self, device):
        w = super()._prepare(device)
        sd = dict(self._decoder_params())
        for k in ["decoder_embed.weight", "decoder_pred.weight"] + [
                f"decoder_blocks.{i}.{lin}.weight" for i in range(self.dec_depth)
                for lin in ("attn.qkv", "attn.proj", "mlp.fc1", "mlp.fc2")]:
            w[k] = sd[k].detach().to(_F16).contiguous()
        w["mask_token"] = sd["mask_token"].detach().float().reshape(-1).contiguous()
        w["decoder_pos_embed"] = sd["decoder_pos_embed"].detach().float().reshape(self.tokens, -1).contiguous()
        return w

    def _decoder_spec(self):
        return dict(prefix="decoder_blocks", T=self.tokens, D=self.dec_dim, H=self.dec_heads, eps=self.ln_eps,
                    total=self.dec_depth)

    # ------------------------------------------------------------------ masking, patches
    def random_masking(self, n, mask_ratio, noise=None, device=None):
        """-> dict(L, ids_shuffle, ids_restore, ids_keep, mask fp32 [n, 196], keep uint8 [n, 196]) (module docstring, 1.)"""
        T = self.tokens
        if not (isinstance(mask_ratio, (int, float)) and 0 <= mask_ratio < 1):
            raise ValueError(f"mask_ratio must satisfy 0 <= mask_ratio < 1, got {mask_ratio!r}")
        L = int(T * (1 - mask_ratio))
        if L < 1:
            raise ValueError(f"mask_ratio {mask_ratio} keeps no token (len_keep = {L})")
        if noise is not None:
            if tuple(noise.shape) != (n, T):
                raise ValueError(f"noise: expected [{n}, {T}], got {tuple(noise.shape)}")
            ids_shuffle = torch.argsort(noise.to(device), dim=1)
        elif mask_ratio == 0:
            ids_shuffle = torch.arange(T, device=device).expand(n, T)
        else:
            ids_shuffle = torch.argsort(torch.rand(n, T, device=device), dim=1)
        ids_shuffle = ids_shuffle.contiguous()
        ids_restore = torch.argsort(ids_shuffle, dim=1).contiguous()
        mask = (ids_restore >= L).float().contiguous()
        return dict(L=L, ids_shuffle=ids_shuffle, ids_restore=ids_restore, ids_keep=ids_shuffle[:, :L].contiguous(),
                    mask=mask, keep=(mask == 0).to(torch.uint8).contiguous())

    def patchify(self, imgs):
        """imgs[N, 3, 224, 224] -> [N, 196, 768], a patch in (row, column, channel) order."""
        p, h = self.patch, imgs.shape[2] // self.patch
        x = imgs.reshape(imgs.shape[0], 3, h, p, h, p)
        return torch.einsum("nchpwq->nhwpqc", x).reshape(imgs.shape[0], h * h, p * p * 3)

    def unpatchify(self, x):
        """[N, 196, 768] -> imgs[N, 3, 224, 224] (the inverse of ``patchify``)."""
        p, h = self.patch, int(round(x.shape[1] ** 0.5))
        x = x.reshape(x.shape[0], h, h, p, p, 3)
        return torch.einsum("nhwpqc->nchpwq", x).reshape(x.shape[0], 3, h * p, h * p)

    # ------------------------------------------------------------------ forward
    def _loss_scale(self, mask_sum):
        return 2.0 ** (round(math.log2(self.pred_dim * mask_sum)) + 4)

    def _decoder(self, w, lat16, ids_restore, n, L, dd):
        """The decoder over the first ``dd`` blocks: latent (fp16 rows [n * L, 768]) -> (pred fp16 [n * 196, 768], what the
        backward reads of it).  ``forward_decoder`` drops the second result; its blocks run in the saving form all the
        same, so that it stays ``forward``'s launch sequence (fc1 through ``isic_gemm_f16_gelu_pre``)."""
        T, Dd, P, dev = self.tokens, self.dec_dim, self.pred_dim, lat16.device
        M = n * T
        z = torch.empty((n * L, Dd), device=dev, dtype=_F16)
        call("isic_gemm_f16", lat16, w["decoder_embed.weight"], w["decoder_embed.bias"], None, z, n * L, Dd, self.dims[2], 0, 0)
        xd = torch.empty((M, Dd), device=dev, dtype=_F16)
        call("isic_mae_unshuffle_f16", z, ids_restore, w["mask_token"], w["decoder_pos_embed"], xd, n, T, L, Dd)
        del z
        x, saves = blocks_forward(w, xd, None, n, dd, self._decoder_spec(), save=True)
        hn = torch.empty((M, Dd), device=dev, dtype=_F16)
        call("isic_layernorm_add_f16", x, None, None, w["decoder_norm.weight"], w["decoder_norm.bias"], hn, None, M, Dd, 0,
             self.ln_eps)
        pred = torch.empty((M, P), device=dev, dtype=_F16)
        call("isic_gemm_f16", hn, w["decoder_pred.weight"], w["decoder_pred.bias"], None, pred, M, P, Dd, 0, 0)
        return pred, dict(dd=dd, xd_out=x, hn=hn, blocks=saves)

    def _loss(self, pred, img, mask, mask_sum, S):
        """-> (loss[1] fp32, S d loss / d pred fp16) of pred (fp16 rows) against img (fp32), one launch."""
        n, dev = img.shape[0], img.device
        loss, dpred = torch.empty(1, device=dev, dtype=torch.float32), torch.empty_like(pred)
        nb = call("isic_mae_loss_f16_workspace_bytes", n, self.img_size, self.img_size, self.patch)
        ws = torch.empty(max(nb, 16), device=dev, dtype=torch.uint8)
        call("isic_mae_loss_f16", pred, img, mask, int(self.norm_pix_loss), mask_sum, S, dpred, loss, n, self.in_ch,
             self.img_size, self.img_size, self.patch, ws, ws.numel())
        return loss, dpred

    def _run_mae(self, images, mask_ratio, noise, depth, decoder_depth):
        depth = self._check(images, depth)
        dd = self.dec_depth if decoder_depth is None else int(decoder_depth)
        if not 0 <= dd <= self.dec_depth:
            raise ValueError(f"decoder_depth: 0..{self.dec_depth}")
        n = images.shape[0]
        m = self.random_masking(n, mask_ratio, noise, images.device)
        L, T = m["L"], self.tokens
        if L == T:
            raise ValueError("mask_ratio removes no token: the reconstruction loss has no term (use forward_encoder)")
        latent, tape = self.run_forward_train(images, depth, masking=m)
        pred, dec = self._decoder(tape["w"], tape["latent16"], m["ids_restore"], n, L, dd)
        mask_sum = float(n * (T - L))
        S = self._loss_scale(mask_sum)
        loss, dpred = self._loss(pred, tape["img"], m["mask"], mask_sum, S)
        dec.update(m=m, dpred=dpred, S=S)
        return loss.view(()), pred.view(n, T, self.pred_dim), m, latent, dict(enc=tape, dec=dec)

    def forward(self, imgs, mask_ratio=0.75, noise=None, lesion_mask=None, depth=None, decoder_depth=None):
        """-> (loss, pred[N, 196, 768] fp32, mask[N, 196]); ``loss.backward()`` fills every ``param.grad`` (native).
        ``depth`` / ``decoder_depth`` run only the first blocks of each stage / of the decoder (a test of the composition)."""
        if lesion_mask is not None:
            raise ValueError("lesion_mask is not supported: the reference's fork adds it to the MAE forward, but what it "
                             "does is defined in no code available to this project; pass lesion_mask=None")
        if torch.is_grad_enabled():
            return _MAEFn.apply(imgs, self, (mask_ratio, noise, depth, decoder_depth), *self.parameters())
        loss, pred, m, _, _ = self._run_mae(imgs, mask_ratio, noise, depth, decoder_depth)
        return loss, pred.float(), m["mask"]

    @torch.no_grad()
    def forward_encoder(self, imgs, mask_ratio, noise=None):
        """-> (latent[N, len_keep, 768] fp32 in ids_keep order, mask[N, 196], ids_restore[N, 196])."""
        m = self.random_masking(imgs.shape[0], mask_ratio, noise, imgs.device)
        latent, _ = self.run_forward_train(imgs, None, masking=m)
        return latent, m["mask"], m["ids_restore"]

    @torch.no_grad()
    def forward_decoder(self, latent, ids_restore):
        """latent[N, len_keep, 768] (fp32, rounded to fp16 as the encoder hands it on), ids_restore[N, 196] -> pred fp32."""
        n, L, D = latent.shape
        T, Dd, P = self.tokens, self.dec_dim, self.pred_dim
        if D != self.dims[2] or tuple(ids_restore.shape) != (n, T) or not 1 <= L <= T:
            raise ValueError("forward_decoder: latent[N, len_keep, 768] and ids_restore[N, 196]")
        if not latent.is_cuda:
            raise IsicHipError("ConvMAEBase runs on the MI355X only (no CPU fallback)")
        dev = latent.device
        pred, _ = self._decoder(self._prepare(dev), latent.reshape(n * L, D).to(_F16).contiguous(),
                                ids_restore.to(dev).long().contiguous(), n, L, self.dec_depth)
        return pred.float().view(n, T, P)

    @torch.no_grad()
    def forward_loss(self, imgs, pred, mask):
        """The reconstruction loss (module docstring, 5.) of pred[N, 196, 768] (rounded to fp16) against imgs."""
        n, T = mask.shape
        if tuple(pred.shape) != (n, T, self.pred_dim) or tuple(imgs.shape) != (n, self.in_ch, self.img_size, self.img_size):
            raise ValueError("forward_loss: imgs[N, 3, 224, 224], pred[N, 196, 768], mask[N, 196]")
        mask = mask.float().contiguous()
        mask_sum = float(mask.sum())
        if mask_sum <= 0:
            raise ValueError("forward_loss: the mask removes no token")
        loss, _ = self._loss(pred.to(_F16).contiguous(), imgs.float().contiguous(), mask, mask_sum, 1.0)
        return loss.view(())

    # ------------------------------------------------------------------ backward
    def _mae_backward(self, tape, dloss):
        enc, dec = tape["enc"], tape["dec"]
        w, n, m = enc["w"], enc["n"], dec["m"]
        T, L, Dd, D, P = self.tokens, m["L"], self.dec_dim, self.dims[2], self.pred_dim
        M, Mk, eps = n * T, n * L, self.ln_eps
        dev = dec["dpred"].device
        if not math.isfinite(dloss):
            raise FloatingPointError("ConvMAEBase backward: the incoming gradient is not finite")
        s = dloss / dec["S"]
        nb = max(self._encoder_workspace_bytes(enc), blocks_workspace_bytes(w, n, self._decoder_spec()),
                 call("isic_gemm_f16_wgrad_workspace_bytes", M, P, Dd), call("isic_gemm_f16_wgrad_workspace_bytes", Mk, Dd, D),
                 call("isic_colsum_f16_workspace_bytes", n * (T - L), Dd))
        bw = Backward(self, w, param_grads(self), s, nb, dev)
        # ---- decoder_pred, decoder_norm
        bw.wgrad(dec["dpred"], dec["hn"], "decoder_pred", P, Dd, M)
        dh = torch.empty((M, Dd), device=dev, dtype=_F16)
        call("isic_gemm_f16", dec["dpred"], w["decoder_pred.weight.t"], None, None, dh, M, Dd, P, 0, 0)
        g, gh = torch.empty((M, Dd), device=dev, dtype=torch.float32), torch.empty((M, Dd), device=dev, dtype=_F16)
        bw.ln_add(dh, 0, 1.0, dec["xd_out"], None, None, "decoder_norm", 0, eps, None, g, gh, M, Dd)
        del dh
        self._fire(self._block_names("decoder_norm") + self._block_names("decoder_pred"))
        # ---- decoder blocks
        blocks_backward(dec["blocks"], g, gh, bw, n, dec["dd"], self._decoder_spec(), self._fire)
        # ---- unshuffle: kept rows back to ids_keep order; mask_token's gradient is the sum over the removed rows
        dz, drem = torch.empty((Mk, Dd), device=dev, dtype=_F16), torch.empty((n * (T - L), Dd), device=dev, dtype=_F16)
        call("isic_mae_unshuffle_bwd_f16", gh, m["ids_shuffle"], dz, drem, n, T, L, Dd)
        bw.colsum(drem, "mask_token", n * (T - L), Dd)
        del g, gh, drem
        bw.wgrad(dz, enc["latent16"], "decoder_embed", Dd, D, Mk)
        dlat = torch.empty((Mk, D), device=dev, dtype=_F16)
        call("isic_gemm_f16", dz, w["decoder_embed.weight.t"], None, None, dlat, Mk, D, Dd, 0, 0)
        del dz
        self._fire(self._block_names("decoder_embed") + ["mask_token", "decoder_pos_embed"])
        # ---- the encoder, from d latent (already scaled by S)
        self._encoder_backward(enc, dlat, 0, 1.0, bw)
        check_grads(self.parameters(), "ConvMAEBase")

    def train_flops_per_image(self, mask_ratio=0.75):
        """Algorithmic forward + backward FLOPs of one MAE train step per image (products and convolutions, x 3 except the
        stem's data gradient): the encoder with blocks3 on len_keep tokens, the decoder on 196."""
        (d1, d2, d3), T, Dd, r = self.dims, self.tokens, self.dec_dim, self.mlp_ratio
        L = int(T * (1 - mask_ratio))
        enc = self.flops_per_image() - self.depths[2] * (2 * T * (4 * d3 * d3 + 2 * r * d3 * d3) + 4 * T * T * d3)
        enc += self.depths[2] * (2 * L * (4 * d3 * d3 + 2 * r * d3 * d3) + 4 * L * L * d3)
        dec = 2 * L * d3 * Dd + self.dec_depth * (2 * T * (4 * Dd * Dd + 2 * r * Dd * Dd) + 4 * T * T * Dd)
        dec += 2 * T * Dd * self.pred_dim
        return 3 * (enc + dec) - 2 * self.grids[0] ** 2 * d1 * self.in_ch * 16


class _MAEFn(torch.autograd.Function):
    """Autograd edge: loss -> every parameter gradient (accumulated in place by the kernels, hence ``None`` returned).
    pred and mask are outputs without a gradient."""

    @staticmethod
    def forward(ctx, images, model, args, *params):
        loss, pred, m, _, tape = model._run_mae(images, *args)
        ctx.model, ctx.tape = model, tape
        pred, mask = pred.float(), m["mask"]
        ctx.mark_non_differentiable(pred, mask)
        return loss, pred, mask

    @staticmethod
    def backward(ctx, dloss, dpred, dmask):
        model, tape = ctx.model, ctx.tape
        ctx.tape = None
        model._mae_backward(tape, float(dloss))
        return (None, None, None) + tuple(None for _ in model.parameters())


def convmae_convvit_base_patch16_dec512d8b(norm_pix_loss=False, with_decoder=True, **kw):
    """The reference's factory: ``with_decoder=False`` -> the frozen ``ConvMAEBaseEncoder`` (save_latent.py), else the
    trainable ``ConvMAEBase``."""
    if not with_decoder:
        return ConvMAEBaseEncoder(**kw)
    return ConvMAEBase(norm_pix_loss=norm_pix_loss, **kw)
