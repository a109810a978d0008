"""The ConvMAE-Base masked autoencoder (isic_hip/convmae_mae.py) on the MI355X: the kernels of include/isic_hip_mae.h
against fp32 / fp64 torch, and the whole model against the torch-CPU restatement tests/convmae_mae_ref.py.

Tolerances: movement kernels (gather, scatter, unshuffle's kept rows) are bitwise; the masked depthwise 5x5 is held to the
bounds of the unmasked one (tests/test_convmae_train_gpu.py); the head-width-32 attention to those of the head-width-64
tests (3e-3 of the output's scale forward, 5e-3 relative Frobenius backward); the loss to 1e-5 relative and d pred to
fp16 rounding.  The whole model stores every activation and gradient in fp16, so against the fp16-emulating restatement
at small depth its loss and pred are held to 2e-3 relative Frobenius and each parameter gradient to 3e-2 (the bound the
encoder's own backward tests use); at full depth every tensor keeps a cosine >= 0.99."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _relf(got, ref):
    got, ref = got.double().flatten().cpu(), ref.double().flatten().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def _cos(got, ref):
    got, ref = got.double().flatten().cpu(), ref.double().flatten().cpu()
    return float(got @ ref / (got.norm() * ref.norm() + 1e-30))


def _ids(n, T, L, seed):
    g = torch.Generator().manual_seed(seed)
    sh = torch.argsort(torch.rand(n, T, generator=g), dim=1)
    return sh.contiguous(), torch.argsort(sh, dim=1).contiguous(), sh[:, :L].contiguous()


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("H,C", [(56, 256), (28, 384)])
def test_masked_dwconv_forward_and_gradients(H, C):
    N, P = 2, H // 14
    g = torch.Generator().manual_seed(H + C)
    x = torch.randn(N, H, H, C, generator=g).to(F16)
    wt = torch.randn(C, 1, 5, 5, generator=g) / 5
    b = 0.1 * torch.randn(C, generator=g)
    keep = (torch.rand(N, 196, generator=g) > 0.75).to(torch.uint8)
    km = keep.view(N, 14, 14).repeat_interleave(P, 1).repeat_interleave(P, 2)[..., None].to(F16)
    taps = wt.reshape(C, 25).t().contiguous()
    y, xm = torch.empty(N, H, H, C, device=DEV, dtype=F16), torch.empty(N, H, H, C, device=DEV, dtype=F16)
    _call("isic_dwconv5x5_masked_f16", x.to(DEV), keep.to(DEV), P, taps.to(DEV), b.to(DEV), xm, y, N, H, H, C)
    assert torch.equal(xm.cpu(), x * km)                                         # exact: a multiply by 0 or 1
    plain = torch.empty_like(y)
    _call("isic_dwconv5x5_f16", xm, taps.to(DEV), b.to(DEV), plain, N, H, H, C)
    assert torch.equal(y, plain)                                                 # = the unmasked kernel on keep * x
    ref = F.conv2d((x * km).double().permute(0, 3, 1, 2), wt.double(), b.double(), padding=2, groups=C).permute(0, 2, 3, 1)
    assert float((y.double().cpu() - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    # data gradient: keep * conv(dy, reversed taps)
    dy = torch.randn(N, H, H, C, generator=g).to(F16)
    dx = torch.empty_like(y)
    _call("isic_dwconv5x5_masked_dgrad_f16", dy.to(DEV), keep.to(DEV), P, taps.flip(0).contiguous().to(DEV), dx, N, H, H, C)
    xr = (x * km).double().permute(0, 3, 1, 2).requires_grad_(True)
    F.conv2d(xr, wt.double(), None, padding=2, groups=C).backward(dy.double().permute(0, 3, 1, 2))
    refd = (xr.grad.permute(0, 2, 3, 1) * km.double())
    assert bool((dx.cpu()[km.expand_as(dx).cpu() == 0] == 0).all())
    assert float((dx.double().cpu() - refd).abs().max()) <= 2e-3 * float(refd.abs().max())
    # weight gradient of the masked input
    nb = _call("isic_dwconv5x5_wgrad_f16_workspace_bytes", N, H, H, C)
    ws = torch.empty(max(nb, 16), device=DEV, dtype=torch.uint8)
    dw, db = torch.empty(25, C, device=DEV), torch.empty(C, device=DEV)
    _call("isic_dwconv5x5_wgrad_f16", xm, dy.to(DEV), dw, db, N, H, H, C, 1.0, 0, ws, ws.numel())
    xr2 = (x * km).double().permute(0, 3, 1, 2)
    w2 = wt.double().requires_grad_(True)
    F.conv2d(xr2, w2, None, padding=2, groups=C).backward(dy.double().permute(0, 3, 1, 2))
    assert _relf(dw.t().reshape(C, 1, 5, 5), w2.grad) <= 1e-4


def test_gather_scatter_unshuffle_bitwise():
    n, T, L, C = 3, 196, 49, 512
    g = torch.Generator().manual_seed(4)
    sh, rest, keep_ids = _ids(n, T, L, 4)
    x = torch.randn(n * T, C, generator=g).to(F16)
    y = torch.empty(n * L, C, device=DEV, dtype=F16)
    _call("isic_gather_rows_f16", x.to(DEV), keep_ids.to(DEV), y, n, T, L, C)
    ref = torch.gather(x.view(n, T, C), 1, keep_ids[..., None].expand(-1, -1, C)).reshape(n * L, C)
    assert torch.equal(y.cpu(), ref)
    back = torch.full((n * T, C), float("nan"), device=DEV, dtype=F16)
    _call("isic_scatter_rows_f16", y, rest.to(DEV), back, n, T, L, C)
    kept = (rest < L).view(n * T)
    assert torch.equal(back.cpu()[kept], x[kept]) and bool((back.cpu()[~kept] == 0).all())
    # unshuffle: (kept ? y[rank] : mask_token) + pos, the sum in fp32 rounded once
    mt = torch.randn(C, generator=g)
    pos = torch.randn(T, C, generator=g)
    out = torch.empty(n * T, C, device=DEV, dtype=F16)
    _call("isic_mae_unshuffle_f16", y, rest.to(DEV), mt.to(DEV), pos.to(DEV), out, n, T, L, C)
    full = torch.cat([ref.view(n, L, C).float(), mt.expand(n, T - L, C)], dim=1)
    refu = (torch.gather(full, 1, rest[..., None].expand(-1, -1, C)) + pos).to(F16).reshape(n * T, C)
    assert torch.equal(out.cpu(), refu)
    # its adjoint: the kept rows in ids_keep order, the removed rows' column sum is mask_token's gradient
    dout = torch.randn(n * T, C, generator=g).to(F16)
    dk, dr = torch.empty(n * L, C, device=DEV, dtype=F16), torch.empty(n * (T - L), C, device=DEV, dtype=F16)
    _call("isic_mae_unshuffle_bwd_f16", dout.to(DEV), sh.to(DEV), dk, dr, n, T, L, C)
    assert torch.equal(dk.cpu(), torch.gather(dout.view(n, T, C), 1, keep_ids[..., None].expand(-1, -1, C)).reshape(n * L, C))
    nb = _call("isic_colsum_f16_workspace_bytes", n * (T - L), C)
    ws = torch.empty(max(nb, 16), device=DEV, dtype=torch.uint8)
    gm = torch.empty(C, device=DEV)
    _call("isic_colsum_f16", dr, gm, n * (T - L), C, 0.5, 0, ws, ws.numel())
    refm = 0.5 * dout.double().view(n, T, C)[(rest >= L)].sum(0)
    assert float((gm.double().cpu() - refm).abs().max()) <= 1e-5 * float(dout.double().abs().sum(0).max())


def _attn_ref(qkv, dout, n, T, H, hd):
    D = H * hd
    x = qkv.double().cpu().view(n, T, 3, H, hd).permute(2, 0, 3, 1, 4).requires_grad_(True)
    q, k, v = x[0], x[1], x[2]
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
    o = (a @ v).transpose(1, 2).reshape(n * T, D)
    o.backward(dout.double().cpu())
    return o.detach(), x.grad


@pytest.mark.parametrize("T", [49, 196])
def test_attention_head_width_32(T):
    n, H = 3, 16
    D, M = H * 32, n * T
    g = torch.Generator(device=DEV).manual_seed(T)
    qkv = (torch.randn(M, 3 * D, device=DEV, generator=g) * 1.5).to(F16)
    dout = torch.randn(M, D, device=DEV, generator=g).to(F16)
    out = torch.full((M, D), float("nan"), device=DEV, dtype=F16)
    _call("isic_attention_d32_f16", qkv, out, n, T, H)
    ref, gref = _attn_ref(qkv, dout, n, T, H, 32)
    assert float((out.double().cpu() - ref).abs().max()) <= 3e-3 * float(ref.abs().max()) + 1e-3
    dqkv = torch.empty(M, 3 * D, device=DEV, dtype=F16)
    _call("isic_attention_d32_bwd_f16", qkv, out, dout, dqkv, n, T, H)
    gref = gref.permute(1, 3, 0, 2, 4).reshape(M, 3 * D)
    for i, name in enumerate("qkv"):
        err = _relf(dqkv[:, i * D:(i + 1) * D], gref[:, i * D:(i + 1) * D])
        assert err <= 5e-3, f"d{name}: relative Frobenius error {err:.3e}"
    again = torch.empty_like(dqkv)
    _call("isic_attention_d32_bwd_f16", qkv, out, dout, again, n, T, H)
    assert torch.equal(dqkv, again)


@pytest.mark.parametrize("norm_pix", [0, 1])
def test_reconstruction_loss_and_dpred(norm_pix):
    from convmae_mae_ref import mae_loss
    n = 3
    g = torch.Generator().manual_seed(10 + norm_pix)
    img = torch.randn(n, 3, 224, 224, generator=g)
    pred = torch.randn(n, 196, 768, generator=g).to(F16)
    mask = (torch.rand(n, 196, generator=g) > 0.25).float()
    msum, S = float(mask.sum()), 2.0 ** 20
    loss, dpred = torch.empty(1, device=DEV), torch.empty(n * 196, 768, device=DEV, dtype=F16)
    ws = torch.empty(_call("isic_mae_loss_f16_workspace_bytes", n, 224, 224, 16), device=DEV, dtype=torch.uint8)
    _call("isic_mae_loss_f16", pred.to(DEV), img.to(DEV), mask.to(DEV), norm_pix, msum, S, dpred, loss, n, 3, 224, 224, 16,
          ws, ws.numel())
    p64 = pred.double().requires_grad_(True)
    ref = mae_loss(img.double(), p64, mask.double(), bool(norm_pix))
    ref.backward()
    assert abs(float(loss) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
    d_ref = (p64.grad * S).reshape(n * 196, 768)
    assert float((dpred.double().cpu() - d_ref).abs().max()) <= 2.0 ** -10 * float(d_ref.abs().max())
    assert bool((dpred.cpu().view(n, 196, 768)[mask == 0] == 0).all())
    loss2, dpred2 = torch.empty_like(loss), torch.empty_like(dpred)
    _call("isic_mae_loss_f16", pred.to(DEV), img.to(DEV), mask.to(DEV), norm_pix, msum, S, dpred2, loss2, n, 3, 224, 224, 16,
          ws, ws.numel())
    assert torch.equal(loss, loss2) and torch.equal(dpred, dpred2)


# ------------------------------------------------------------------ the model
def _model(seed=0, norm_pix=False):
    from isic_hip.convmae_mae import ConvMAEBase
    import convmae_mae_ref as mr
    m = ConvMAEBase(norm_pix_loss=norm_pix, seed=seed)
    p = mr.init_params(seed)
    m.load_state_dict({k: v.clone() for k, v in p.items()})
    return m.to(DEV).train(), p


def _images(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, 224, 224, generator=g)


def test_ratio_zero_is_the_trainable_encoder():
    from isic_hip.convmae import ConvMAEBaseEncoder
    m, p = _model(1)
    enc = ConvMAEBaseEncoder(trainable=True).to(DEV)
    enc.load_state_dict(m.state_dict(), strict=False)
    img = _images(2, 3).to(DEV)
    with torch.no_grad():
        lat, mask, rest = m.forward_encoder(img, 0.0)
        tok, _ = enc.run_forward_train(img)
    assert torch.equal(lat, tok) and not bool(mask.any()) and torch.equal(rest.cpu(), torch.arange(196).expand(2, 196))


def test_forward_is_encoder_then_decoder_then_loss():
    """forward() and the three public stages run the same launches: composed, they give forward()'s pred and loss bit for bit."""
    img = _images(2, 4).to(DEV)
    noise = torch.rand(2, 196, generator=torch.Generator().manual_seed(8)).to(DEV)
    for norm_pix in (False, True):
        m, _ = _model(2, norm_pix)
        with torch.no_grad():
            loss, pred, mask = m(img, mask_ratio=0.75, noise=noise)
            lat, mask2, ids_restore = m.forward_encoder(img, 0.75, noise=noise)
            pred2 = m.forward_decoder(lat, ids_restore)
            loss2 = m.forward_loss(img, pred2, mask2)
        assert math.isfinite(float(loss)) and float(loss) > 0
        assert torch.equal(mask2, mask) and torch.equal(pred2, pred) and torch.equal(loss2, loss)


def _grads_vs_ref(depth, dd, norm_pix, n, seed):
    import convmae_mae_ref as mr
    m, p = _model(seed, norm_pix)
    img = _images(n, seed)
    noise = torch.rand(n, 196, generator=torch.Generator().manual_seed(seed + 1))
    m.zero_grad(set_to_none=True)
    loss, pred, mask = m(img.to(DEV), mask_ratio=0.75, noise=noise.to(DEV), depth=depth, decoder_depth=dd)
    loss.backward()
    pr = {k: v.clone().requires_grad_(k != "decoder_pos_embed") for k, v in p.items()}
    ref = mr.forward(pr, img, 0.75, noise, norm_pix, emulate_fp16=True, depth=depth, dec_depth=dd)
    ref["loss"].backward()
    assert torch.equal(mask.cpu(), ref["mask"])
    return m, loss, pred, ref, pr


def test_small_depth_matches_the_restatement():
    depth, dd = (1, 1, 2), 2
    m, loss, pred, ref, pr = _grads_vs_ref(depth, dd, True, 2, 5)
    assert abs(float(loss) - float(ref["loss"])) <= 2e-3 * abs(float(ref["loss"]))
    assert _relf(pred, ref["pred"].detach()) <= 2e-3
    worst = []
    for k, prm in m.named_parameters():
        if k == "decoder_pos_embed":
            assert prm.grad is None
            continue
        r = pr[k].grad
        if r is None or float(r.abs().max()) == 0:                 # blocks past ``depth``: no gradient on either side
            assert prm.grad is None or float(prm.grad.abs().max()) == 0, k
            continue
        worst.append((_relf(prm.grad, r), k))
    worst.sort(reverse=True)
    assert worst[0][0] <= 3e-2, worst[:5]


def test_full_depth_cosine_and_reproducible():
    m, loss, pred, ref, pr = _grads_vs_ref(None, None, False, 2, 6)
    assert _cos(pred, ref["pred"].detach()) >= 0.99
    g1 = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    for k, gr in g1.items():
        assert _cos(gr, pr[k].grad) >= 0.99, k
    # bit-reproducible backward, and grad_ready_hook reports every parameter once: decoder first
    seen = []
    m.grad_ready_hook = lambda names: seen.extend(names)
    m.zero_grad(set_to_none=True)
    noise = torch.rand(2, 196, generator=torch.Generator().manual_seed(7))
    loss2, _, _ = m(_images(2, 6).to(DEV), mask_ratio=0.75, noise=noise.to(DEV))
    loss2.backward()
    assert torch.equal(loss2, loss)
    for k, p in m.named_parameters():
        if k in g1:
            assert torch.equal(p.grad, g1[k]), k
    names = [k for k, _ in m.named_parameters()]
    assert sorted(seen) == sorted(names) and len(seen) == len(set(seen))
    first_enc = min(i for i, k in enumerate(seen) if not (k.startswith("decoder") or k == "mask_token"))
    assert all(k.startswith("decoder") or k == "mask_token" for k in seen[:first_enc])
    assert seen[first_enc:first_enc + 2] == ["norm.weight", "norm.bias"]


def test_ten_adamw_steps_reduce_the_loss():
    """lr 1e-4 encoder / 1e-3 decoder (AdamW, weight decay 0.05, betas (0.9, 0.95)): one fixed batch, fixed noise."""
    from isic_hip import optim
    from isic_hip.convmae_mae import ConvMAEBase
    m = ConvMAEBase(norm_pix_loss=True, seed=0).to(DEV).train()
    dec = [p for k, p in m.named_parameters() if (k.startswith("decoder") or k == "mask_token") and p.requires_grad]
    enc = [p for k, p in m.named_parameters() if not (k.startswith("decoder") or k == "mask_token")]
    opts = [optim.AdamW(enc, lr=1e-4, betas=(0.9, 0.95), weight_decay=0.05),
            optim.AdamW(dec, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)]
    img = _images(4, 11).to(DEV)
    noise = torch.rand(4, 196, generator=torch.Generator().manual_seed(12)).to(DEV)
    losses = []
    for _ in range(10):
        for o in opts:
            o.zero_grad()
        loss, _, _ = m(img, mask_ratio=0.75, noise=noise)
        loss.backward()
        for o in opts:
            o.step()
        losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses) and losses[-1] < 0.9 * losses[0], losses


def test_train_ae_synthetic_end_to_end(tmp_path, capsys, monkeypatch):
    """2 epochs on 70 synthetic images (10 per class: the 10-fold split needs them), batch 8; the saved best state loads
    strictly into ConvMAEBase and through save_latent.extract_latents (model_path) into the encoder."""
    from isic_hip.convmae import ConvMAEBaseEncoder
    from isic_hip.convmae_mae import ConvMAEBase
    from save_latent import SyntheticDermImages, extract_latents
    script = os.path.join(ROOT, "multimodal-isic_amd", "train_ae.py")
    r = subprocess.run([sys.executable, script, "--synthetic", "--epochs", "2", "--batch-size", "8", "--n-images", "70",
                        "--out-dir", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("Train Loss") == 2 and "Saved Best Model" in r.stdout
    ckpts = [f for f in os.listdir(tmp_path / "models") if f.endswith(".pth")]
    assert len(ckpts) == 1
    sd = torch.load(tmp_path / "models" / ckpts[0], map_location="cpu")
    ConvMAEBase().load_state_dict(sd, strict=True)
    assert not torch.equal(sd["decoder_pred.weight"], ConvMAEBase().state_dict()["decoder_pred.weight"])   # it trained
    res = ConvMAEBaseEncoder().load_state_dict(sd, strict=False)
    assert not res.missing_keys and all(k.startswith("decoder") or k == "mask_token" for k in res.unexpected_keys)
    capsys.readouterr()
    monkeypatch.chdir(tmp_path)                                     # extract_latents writes dataframes_latents/ here
    cfg = {"encoder": "convmae_base", "model_path": str(tmp_path / "models"), "device": DEV, "seed": 1}
    extract_latents(cfg, ckpts[0], datasets=(SyntheticDermImages(n=4), SyntheticDermImages(n=2, seed=5)), batch_size=4)
    assert "not found" not in capsys.readouterr().out
