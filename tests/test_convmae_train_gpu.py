"""Training of the ConvMAE-Base patch encoder (ConvMAEBaseEncoder(trainable=True)) on the MI355X: the backward kernels of
include/isic_hip_convmae_train.h against fp64 / fp32 references, and the whole encoder's gradients against torch.autograd
through the fp32 CPU restatement (tests/convmae_ref.py).

Tolerances come from fp16 / fp32 rounding arithmetic, as in tests/test_vit_train_gpu.py: the depthwise weight gradient
sums fp16 products in fp32 (bounded by 1e-4 of sum |dy| |x|); the LayerNorm-add backward keeps fp32 inside and its fp32
output is held to 1e-4 of the gradient's scale (2^-11 for the fp16 copy); depth-to-space is a permutation (exact).  The
whole encoder stores every activation and gradient in fp16, so its parameter gradients are held to 3e-2 relative
Frobenius error per tensor at depth <= 2 per stage and cosine >= 0.99 at full depth, against the pure-fp32 oracle and
against its emulate_fp16 form."""
import math
import os
import sys

import numpy as np
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


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16), device=DEV, dtype=torch.uint8)


def _relf(got, ref):
    got, ref = got.double().flatten(), ref.double().flatten()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def _cos(got, ref):
    got, ref = got.double().flatten(), ref.double().flatten()
    return float(got @ ref / (got.norm() * ref.norm() + 1e-30))


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("N,H,W,C", [(4, 56, 56, 256), (4, 28, 28, 384), (3, 13, 9, 64)])
def test_dwconv_wgrad_matches_fp64(N, H, W, C):
    g = torch.Generator(device=DEV).manual_seed(N + H + W + C)
    x = torch.randn(N, H, W, C, device=DEV, generator=g).to(F16)
    dy = torch.randn(N, H, W, C, device=DEV, generator=g).to(F16)
    s = 0.25
    ws = _ws(_call("isic_dwconv5x5_wgrad_f16_workspace_bytes", N, H, W, C))
    dw, db = torch.empty(25, C, device=DEV), torch.empty(C, device=DEV)
    _call("isic_dwconv5x5_wgrad_f16", x, dy, dw, db, N, H, W, C, s, 0, ws, ws.numel())
    xp = F.pad(x.double().permute(0, 3, 1, 2), (2, 2, 2, 2))
    dyc = dy.double().permute(0, 3, 1, 2)
    ref = torch.stack([s * (dyc * xp[:, :, kh:kh + H, kw:kw + W]).sum((0, 2, 3)) for kh in range(5) for kw in range(5)])
    bound = torch.stack([1e-4 * s * (dyc.abs() * xp[:, :, kh:kh + H, kw:kw + W].abs()).sum((0, 2, 3))
                         for kh in range(5) for kw in range(5)]) + 1e-6
    assert bool(((dw.double() - ref).abs() <= bound).all()), float(((dw.double() - ref).abs() / bound).max())
    refb = s * dyc.sum((0, 2, 3))
    assert bool(((db.double() - refb).abs() <= 1e-4 * s * dyc.abs().sum((0, 2, 3)) + 1e-6).all())
    dw2, db2 = dw.clone(), db.clone()
    _call("isic_dwconv5x5_wgrad_f16", x, dy, dw2, db2, N, H, W, C, s, 1, ws, ws.numel())     # accumulate: adds
    assert torch.allclose(dw2, 2 * dw, rtol=1e-6, atol=0) and torch.allclose(db2, 2 * db, rtol=1e-6, atol=0)
    dw3, db3 = torch.empty_like(dw), torch.empty_like(db)
    _call("isic_dwconv5x5_wgrad_f16", x, dy, dw3, db3, N, H, W, C, s, 0, ws, ws.numel())
    assert torch.equal(dw3, dw) and torch.equal(db3, db)                                     # bit-reproducible


def test_dwconv_data_gradient_is_the_reversed_taps_convolution():
    N, H, W, C = 2, 28, 28, 128
    g = torch.Generator().manual_seed(1)
    wt = torch.randn(C, 1, 5, 5, generator=g) / 5
    x = torch.randn(N, C, H, W, generator=g, requires_grad=True)
    dy = torch.randn(N, C, H, W, generator=g).half().float()
    F.conv2d(x, wt, None, padding=2, groups=C).backward(dy)
    taps = wt.reshape(C, 25).t().flip(0).contiguous().to(DEV)
    dy16 = dy.permute(0, 2, 3, 1).contiguous().to(DEV).to(F16)
    dx = torch.empty_like(dy16)
    _call("isic_dwconv5x5_f16", dy16, taps, None, dx, N, H, W, C)
    ref = x.grad.permute(0, 2, 3, 1)
    assert (dx.float().cpu() - ref).abs().max() <= 2e-3 * ref.abs().max() + 1e-3


@pytest.mark.parametrize("M,N", [pytest.param(300, 256, id="256"), pytest.param(300, 384, id="384"),
                                 pytest.param(300, 768, id="768"), pytest.param(300, 1024, id="1024"),
                                 pytest.param(3001, 384, id="3001x384")])
@pytest.mark.parametrize("addends,dy_f32,act", [(0, 0, 0), (2, 1, 0), (0, 1, 1), (2, 0, 1)])
@pytest.mark.parametrize("mode", ["alias", "fresh", "f16_only"])
def test_layernorm_add_bwd_matches_fp32_autograd(M, N, addends, dy_f32, act, mode):
    """mode "alias": g_in aliases g_out, both outputs, accumulate = 1 (the CBlock / ViT block norms); "fresh": no g_in, both
    outputs, accumulate = 0; "f16_only": no g_in, no fp32 output, accumulate = 0 (the PatchEmbed norms).  M = 300 is 5 slabs
    of the parameter-gradient reduction; M = 3001 (the ViT-S width) is 47 with a ragged last chunk and rows that are not a
    multiple of 4."""
    eps, s, mul = 1e-6, 0.5, 4.0
    g = torch.Generator().manual_seed(N + 10 * addends + act)
    x, a, b = ((torch.randn(M, N, generator=g) * 2 + 0.5).half() for _ in range(3))
    gamma, beta = 1 + 0.1 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    dy = dy if dy_f32 else dy.half()
    g_in = torch.randn(M, N, generator=g) if mode == "alias" else torch.zeros(M, N)
    v = x.float() + (a.float() + b.float() if addends else 0.0)
    v.requires_grad_(True)
    gm, bt = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = F.layer_norm(v, (N,), gm, bt, eps)
    y = F.gelu(y) if act else y
    y.backward(dy.float() * mul)
    d = lambda t: t.to(DEV)                                         # noqa: E731
    ws = _ws(_call("isic_layernorm_add_bwd_f16_workspace_bytes", M, N))
    nan = float("nan")
    g_out = {"alias": d(g_in).clone(), "fresh": torch.full((M, N), nan, device=DEV), "f16_only": None}[mode]
    g16 = torch.full((M, N), nan, device=DEV, dtype=F16)
    acc = 1 if mode == "alias" else 0
    dg, dbt = (torch.full((N,), 1.0 if acc else nan, device=DEV) for _ in range(2))
    _call("isic_layernorm_add_bwd_f16", d(dy), dy_f32, mul, d(x), d(a) if addends else None, d(b) if addends else None,
          d(gamma), d(beta), act, eps, g_out if mode == "alias" else None, g_out, g16, dg, dbt, M, N, s, acc, ws, ws.numel())
    from f16_kernel_ref import layernorm_add_bwd_gout_tol, layernorm_add_bwd_param_tol    # the bounds this test set
    ref = g_in + v.grad
    if g_out is not None:
        assert float((g_out.cpu() - ref).abs().max()) <= layernorm_add_bwd_gout_tol(ref, v.grad, False)
        assert torch.equal(g16, g_out.to(F16))
    else:                                                           # the fp16 copy alone: the fp32 error + one rounding
        assert float((g16.float().cpu() - ref).abs().max()) <= layernorm_add_bwd_gout_tol(ref, v.grad, True)
    for got, want in ((dg, acc + s * gm.grad), (dbt, acc + s * bt.grad)):
        assert float((got.cpu() - want).abs().max()) <= layernorm_add_bwd_param_tol(want, s, M)


@pytest.mark.parametrize("P,H,C", [(2, 56, 256), (4, 56, 256), (2, 28, 384)])
def test_patch_rows_bwd_is_the_inverse_permutation(P, H, C):
    N = 3
    x = torch.randn(N, H, H, C, device=DEV).to(F16)
    rows = torch.empty(N * (H // P) ** 2, P * P * C, device=DEV, dtype=F16)
    _call("isic_patch_rows_nhwc_f16", x, rows, N, H, H, C, P)
    dx = torch.full((N, H, H, C), float("nan"), device=DEV)
    dx16 = torch.empty(N, H, H, C, device=DEV, dtype=F16)
    _call("isic_patch_rows_bwd_f16", rows, dx, dx16, N, H, H, C, P, 0)
    assert torch.equal(dx, x.float()) and torch.equal(dx16, x)
    base = torch.randn(N, H, H, C, device=DEV)
    acc = base.clone()
    _call("isic_patch_rows_bwd_f16", rows, acc, None, N, H, H, C, P, 1)
    assert torch.equal(acc, base + x.float())


def test_stem_weight_gradient_on_padded_rows_matches_fp64():
    n = 2
    img = torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(4))
    dy = torch.randn(n * 56 * 56, 256, generator=torch.Generator().manual_seed(5)).half()
    rows = torch.empty(n * 56 * 56, 128, device=DEV, dtype=F16)
    _call("isic_patch_rows_nchw_f32", img.to(DEV), rows, n, 3, 224, 224, 4, 128)
    ws = _ws(_call("isic_gemm_f16_wgrad_workspace_bytes", n * 56 * 56, 256, 128))
    dW = torch.empty(256, 128, device=DEV)
    _call("isic_gemm_f16_wgrad", dy.to(DEV), rows, dW, None, n * 56 * 56, 256, 128, 1.0, 0, ws, ws.numel())
    assert torch.equal(dW[:, 48:], torch.zeros_like(dW[:, 48:]))
    got = dW[:, :48].cpu().reshape(256, 4, 4, 3).permute(0, 3, 1, 2)
    dyc = dy.double().view(n, 56, 56, 256).permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(img.half().double(), (256, 3, 4, 4), dyc, stride=4)
    bound = 1e-4 * torch.nn.grad.conv2d_weight(img.half().double().abs(), (256, 3, 4, 4), dyc.abs(), stride=4) + 1e-6
    assert bool(((got.double() - ref).abs() <= bound).all())


# ------------------------------------------------------------------ whole encoder
def _enc(seed=0, **kw):
    import convmae_ref
    from isic_hip.convmae import ConvMAEBaseEncoder
    e = ConvMAEBaseEncoder(trainable=True, **kw).to(DEV)
    e.load_state_dict({k: v.to(DEV) for k, v in convmae_ref.init_params(seed).items()})
    return e


def _images(n, seed):
    return torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _oracle_grads(enc, images, R, depth, emulate=False):
    import convmae_ref
    p = {k: v.detach().cpu().float().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    tok = convmae_ref.forward_tokens(p, images.cpu(), emulate_fp16=emulate, depth=depth)
    (tok * R.cpu()).sum().backward()
    return {k: v.grad for k, v in p.items() if v.grad is not None}


def _gpu_grads(enc, images, R, depth=None):
    enc.zero_grad(set_to_none=True)
    tok = enc.forward_tokens(images, depth=depth)
    (tok * R).sum().backward()
    return {n: p.grad.detach().cpu().clone() for n, p in enc.named_parameters() if p.grad is not None}


def test_trainable_forward_is_the_unfolded_forward():
    from isic_hip.convmae import ConvMAEBaseEncoder
    enc = _enc()
    ref = ConvMAEBaseEncoder(fold_layernorm=False).to(DEV)
    ref.load_state_dict(enc.state_dict())
    x = _images(2, 1)
    for depth in ((1, 1, 1), None):
        want = ref.run_tokens(x, depth=depth)
        with torch.no_grad():
            assert torch.equal(enc.forward_tokens(x, depth=depth), want)
        enc.train()
        tok = enc.forward_tokens(x, depth=depth)
        assert tok.requires_grad and torch.equal(tok.detach(), want)


@pytest.mark.parametrize("depth", [(1, 1, 1), (2, 2, 2), (2, 2, 11)])
def test_encoder_gradients_match_oracle(depth):
    """Every parameter gradient against two yardsticks: the pure-fp32 oracle and its emulate_fp16 form, which rounds where
    the HIP path stores fp16.  Depth <= 2 per stage: relative Frobenius error <= 3e-2 per tensor against each (measured
    <= 1.8e-3 against either).  Full depth: cosine >= 0.99 per tensor against each."""
    enc = _enc()
    enc.train()
    n = 2
    x = _images(n, 2)
    R = torch.randn(n, 196, 768, generator=torch.Generator().manual_seed(3)).to(DEV)
    got = _gpu_grads(enc, x, R, depth)
    ref = _oracle_grads(enc, x, R, depth)
    ref16 = _oracle_grads(enc, x, R, depth, emulate=True)
    assert set(ref) == set(ref16) and set(ref) <= set(got)
    for k in set(got) - set(ref):                                   # blocks past ``depth``: reported, never touched
        assert not got[k].any(), k
    shallow = depth != (2, 2, 11)
    for name, yard in (("fp32", ref), ("emulate_fp16", ref16)):
        worst = max(yard, key=lambda k: _relf(got[k], yard[k]))
        msg = (f"vs {name} oracle: worst {worst} rel Frobenius {_relf(got[worst], yard[worst]):.3e}, min cosine "
               f"{min(_cos(got[k], yard[k]) for k in yard):.5f}")
        print(msg)
        for k in yard:
            if shallow:
                assert _relf(got[k], yard[k]) <= 3e-2, (k, msg)
            else:
                assert _cos(got[k], yard[k]) >= 0.99, (k, msg)


def test_loss_scale_equivariance_reproducibility_and_nonfinite_input():
    enc = _enc()
    enc.train()
    x = _images(2, 4)
    R = torch.randn(2, 196, 768, generator=torch.Generator().manual_seed(5)).to(DEV)
    d = (1, 1, 1)
    base = _gpu_grads(enc, x, R, d)
    assert all(torch.equal(v, w) for v, w in zip(base.values(), _gpu_grads(enc, x, R, d).values()))   # bit-reproducible
    for f in (2.0 ** -20, 2.0 ** 6):
        got = _gpu_grads(enc, x, R * f, d)
        for k in base:
            assert bool(torch.isfinite(got[k]).all()), k
            assert torch.equal(got[k], base[k] * f), (f, k)            # a power-of-two loss scale: exactly equivariant
    enc.zero_grad(set_to_none=True)
    bad = R.clone()
    bad[0, 0, 0] = float("inf")
    with pytest.raises(FloatingPointError):
        (enc.forward_tokens(x, depth=d) * bad).sum().backward()


def test_grad_ready_hook_reports_every_parameter_once_last_block_first():
    enc = _enc()
    enc.train()
    names = [n for n, _ in enc.named_parameters()]
    seen, snaps = [], {}
    params = dict(enc.named_parameters())

    def hook(group):
        torch.cuda.synchronize()
        for n in group:
            if params[n].grad is not None:
                snaps[n] = params[n].grad.detach().clone()
        seen.append(list(group))
    enc.grad_ready_hook = hook
    x = _images(2, 8)
    (enc.forward_tokens(x, depth=(2, 2, 2)) * 3.0).sum().backward()
    flat = [n for grp in seen for n in grp]
    assert sorted(flat) == sorted(names) and len(flat) == len(set(flat))
    assert seen[0] == ["norm.weight", "norm.bias"]
    order = [(grp[0].split(".")[0], int(grp[0].split(".")[1])) for grp in seen[1:-1]]
    assert order == [("blocks3", i) for i in range(10, -1, -1)] + [("blocks2", 1), ("blocks2", 0), ("blocks1", 1),
                                                                   ("blocks1", 0)], order
    assert "patch_embed1.proj.weight" in seen[-1] and "pos_embed" in seen[-1]
    for n in snaps:
        assert torch.equal(snaps[n], params[n].grad), n
    # ddp.attach: every group's first flat offset has everything registered after it final
    offs = {n: i for i, n in enumerate(names)}
    done = set()
    for grp in seen:
        done |= set(grp)
        lo = min(offs[n] for n in grp)
        assert all(n in done for n in names[lo:]), grp[0]


def test_fine_tuned_weights_load_into_the_frozen_encoder():
    from isic_hip import optim
    from isic_hip.convmae import ConvMAEBaseEncoder
    enc = _enc(seed=1)
    enc.train()
    x = _images(2, 6)
    R = torch.randn(2, 196, 768, generator=torch.Generator().manual_seed(7)).to(DEV)
    opt = optim.AdamW(enc.parameters(), lr=1e-3, weight_decay=1e-4)
    before = enc.run_tokens(x)
    for _ in range(3):
        opt.zero_grad()
        (enc.forward_tokens(x) * R).sum().backward()
        opt.step()
    with torch.no_grad():
        after = enc.forward_tokens(x)                 # the flat buffer was written in place: the new weights are used
    assert not torch.equal(after, before)
    frozen = ConvMAEBaseEncoder(fold_layernorm=False).to(DEV)
    frozen.load_state_dict(enc.state_dict())
    assert torch.equal(frozen.run_tokens(x), after)


def _milnet(seed=0):
    from model import MultiModalMILNet
    torch.manual_seed(seed)
    return MultiModalMILNet(hidden_dim=64, att_dim=32, dropout=0.0, radiomics_dim=16, num_classes=3,
                            encoder="convmae_base").to(DEV)


def test_milnet_convmae_loss_and_head_gradients_match_oracle():
    import convmae_ref
    from oracle import fusion, mil
    from oracle.model import milnet_loss, sub
    net = _milnet()
    net.encoder.load_state_dict({k: v.to(DEV) for k, v in convmae_ref.init_params(2).items()})
    net.eval()                                       # no dropout: the comparison is deterministic
    B, K = 3, 1
    g = torch.Generator().manual_seed(9)
    img = torch.randn(B, K, 3, 224, 224, generator=g)
    rad = torch.randn(B, 16, generator=g)
    y = torch.arange(B) % 3
    net.zero_grad(set_to_none=True)
    out = net(img.to(DEV), rad.to(DEV))
    loss = net.loss(out, y.to(DEV))
    loss.backward()

    def oracle(emulate):
        p = {k: v.detach().cpu().float().clone().requires_grad_(True) for k, v in net.state_dict().items()
             if v.dtype.is_floating_point}
        feats = convmae_ref.forward_tokens(sub(p, "encoder"), img.view(B * K, 3, 224, 224), emulate_fp16=emulate).mean(dim=1)
        offs = np.arange(B + 1) * K
        o = mil.teacher_forward_batched(sub(p, "mil"), feats, offs)
        z = torch.stack([(o["attention"][lo:hi, None] * o["hidden"][lo:hi]).sum(0) for lo, hi in zip(offs[:-1], offs[1:])])
        fused = torch.cat([fusion.mlp_ln_relu(p, "image_proj", z, None, (0.3, 0.2), 0),
                           fusion.mlp_ln_relu(p, "radiomics_mlp", rad, None, (0.4, 0.3), 2)], dim=1)
        o["logits"] = fusion.fusion_mlp(p, fused, None, 8)
        l = milnet_loss(o, y)
        l.backward()
        return l, {k: v.grad for k, v in p.items() if not k.startswith("encoder.")}
    ref_loss, ref = oracle(False)
    _, ref16 = oracle(True)
    assert abs(float(loss) - float(ref_loss)) <= 3e-2 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    named = dict(net.named_parameters())
    for k, v in ref.items():
        got = named[k].grad
        assert got is not None, k
        # the yardstick of test_milnet_vit_loss_and_head_gradients_match_oracle: 3x the oracle's own fp16 / fp32 spread
        err, spread = _relf(got.cpu(), v), _relf(ref16[k], v)
        assert err <= max(3e-2, 3.0 * spread), (k, err, spread)
    assert all(named["encoder." + k].grad is not None for k, _ in net.encoder.named_parameters())


def test_train_milnet_fold_runs_with_the_convmae_encoder():
    from isic_hip.train import train_milnet_fold
    net = _milnet(seed=1)
    g = torch.Generator().manual_seed(11)

    def split(n):
        y = torch.arange(n) % 3
        img = torch.randn(n, 2, 3, 224, 224, generator=g) + 0.5 * y.view(-1, 1, 1, 1, 1)
        rad = torch.randn(n, 16, generator=g) + 2.0 * torch.nn.functional.one_hot(y, 16).float()
        return img, rad, y
    res = train_milnet_fold(net, split(12), split(6), lr=1e-3, epochs=2, patience=10, bags_per_step=4, num_classes=3,
                            device=torch.device(DEV), log=None)
    hist = res["history"]
    assert len(hist) == 2
    l1, l2 = (float(np.mean(h["train_losses"])) for h in hist)
    assert math.isfinite(l1) and math.isfinite(l2) and l2 < l1, (l1, l2)
    assert net.encoder.grad_ready_hook is None
