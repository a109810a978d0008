"""Training of the ViT-S/16 patch encoder (ViTSmallEncoder(trainable=True)) on the MI355X: the backward kernels of
include/isic_hip_vit_train.h against fp64 / fp32 references, and the whole encoder's gradients against torch.autograd
through the fp32 CPU oracle (oracle/vit.py).

Tolerances come from fp16 / fp32 rounding arithmetic: the weight gradient sums fp16 products in fp32 (relative error of
a sum of |terms| about 2^-24 * sqrt(M) per partial, bounded by 1e-4 of sum |dY| |X|); the attention and LayerNorm
backward keep fp32 inside and store fp16 (2^-11); the whole encoder stores every activation and gradient in fp16, so its
parameter gradients are held to 3e-2 relative Frobenius error per tensor at depth <= 2 and cosine >= 0.99 at depth 12,
against the pure-fp32 oracle."""
import math
import os
import sys

import numpy as np
import pytest
import torch

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
@pytest.mark.parametrize("M", [1, 4097, 200704])
@pytest.mark.parametrize("N,K", [(1152, 384), (384, 1536), (1536, 384), (384, 768)])
def test_wgrad_matches_fp64(M, N, K):
    from f16_kernel_ref import wgrad_bound
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    dY = torch.randn(M, N, device=DEV, generator=g).to(F16)
    X = torch.randn(M, K, device=DEV, generator=g).to(F16)
    s = 0.25
    ws = _ws(_call("isic_gemm_f16_wgrad_workspace_bytes", M, N, K))
    dW = torch.empty(N, K, device=DEV)
    db = torch.empty(N, device=DEV)
    _call("isic_gemm_f16_wgrad", dY, X, dW, db, M, N, K, s, 0, ws, ws.numel())
    ref = s * (dY.double().t() @ X.double())
    bound = wgrad_bound(dY, X, s)                       # tests/f16_kernel_ref.py: 1e-4 s |dY|^T |X| + 1e-6
    assert bool(((dW.double() - ref).abs() <= bound).all()), float(((dW.double() - ref).abs() / bound).max())
    refb = s * dY.double().sum(0)
    boundb = 1e-4 * s * dY.double().abs().sum(0) + 1e-6
    assert bool(((db.double() - refb).abs() <= boundb).all())
    # bitwise reproducible
    dW2, db2 = torch.empty_like(dW), torch.empty_like(db)
    _call("isic_gemm_f16_wgrad", dY, X, dW2, db2, M, N, K, s, 0, ws, ws.numel())
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    # accumulate mode adds onto a non-zero buffer
    base = torch.randn(N, K, device=DEV, generator=g)
    baseb = torch.randn(N, device=DEV, generator=g)
    acc, accb = base.clone(), baseb.clone()
    _call("isic_gemm_f16_wgrad", dY, X, acc, accb, M, N, K, s, 1, ws, ws.numel())
    assert bool(((acc.double() - base.double() - ref).abs() <= bound + 1e-6 * base.double().abs()).all())
    assert bool(((accb.double() - baseb.double() - refb).abs() <= boundb + 1e-6 * baseb.double().abs()).all())


def _attn_ref(qkv, dout, N, T, H):
    D = H * 64
    q, k, v = qkv.float().view(N, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v
    o.backward(dout.float().view(N, T, H, 64).transpose(1, 2))
    return [t.grad.transpose(1, 2).reshape(N * T, D) for t in (q, k, v)]


@pytest.mark.parametrize("T", [4, 17, 196, 208])
def test_attention_bwd_matches_fp32_autograd(T):
    N, H = 3, 6
    D, M = H * 64, N * T
    g = torch.Generator(device=DEV).manual_seed(T)
    qkv = torch.randn(M, 3 * D, device=DEV, generator=g).to(F16)
    dout = torch.randn(M, D, device=DEV, generator=g).to(F16)
    out = torch.empty(M, D, device=DEV, dtype=F16)
    _call("isic_attention_f16", qkv, out, N, T, H, 64)
    dqkv = torch.empty(M, 3 * D, device=DEV, dtype=F16)
    _call("isic_attention_bwd_f16", qkv, out, dout, dqkv, N, T, H, 64)
    refs = _attn_ref(qkv, dout, N, T, H)
    for i, name in enumerate("qkv"):
        err = _relf(dqkv[:, i * D:(i + 1) * D].float(), refs[i])
        assert err <= 5e-3, f"d{name}: relative Frobenius error {err:.3e}"
    again = torch.empty_like(dqkv)
    _call("isic_attention_bwd_f16", qkv, out, dout, again, N, T, H, 64)
    assert torch.equal(dqkv, again)


def test_dgelu_epilogue_and_gelu_pre():
    M, N, K = 2100, 1536, 384
    g = torch.Generator(device=DEV).manual_seed(7)
    A = torch.randn(M, K, device=DEV, generator=g).to(F16)
    W = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(F16)
    aux = (torch.randn(M, N, device=DEV, generator=g) * 2).to(F16)
    C = torch.empty(M, N, device=DEV, dtype=F16)
    _call("isic_gemm_f16_dgelu", A, W, aux, C, M, N, K)
    a = aux.float()
    gp = 0.5 * (1 + torch.erf(a / math.sqrt(2))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)
    ref = (A.float() @ W.float().t()) * gp
    err, tol = (C.float() - ref).abs(), 2.0 ** -10 * ref.abs() + 2e-3        # test_gemm_f16_matches_fp32_matmul's bound
    assert bool((err <= tol).all()), float((err - tol).max())
    # the training forward's fc1: the GELU output bitwise isic_gemm_f16's, plus the fp16 pre-activation
    b = torch.randn(N, device=DEV, generator=g) * 0.1
    hid, pre, hid0 = (torch.empty(M, N, device=DEV, dtype=F16) for _ in range(3))
    _call("isic_gemm_f16_gelu_pre", A, W, b, hid, pre, M, N, K)
    _call("isic_gemm_f16", A, W, b, None, hid0, M, N, K, 1, 0)
    assert torch.equal(hid, hid0)
    ref = A.float() @ W.float().t() + b
    assert bool(((pre.float() - ref).abs() <= 2.0 ** -10 * ref.abs() + 2e-3).all())


# ------------------------------------------------------------------ whole encoder
def _enc(img=224, depth=2, seed=0, **kw):
    from isic_hip.vit import ViTSmallEncoder
    e = ViTSmallEncoder(img_size=img, depth=depth, seed=seed, trainable=True, **kw).to(DEV)
    # LayerNorm affine and biases away from their (1, 0) init, so that their gradients and the paths through them are tested
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for n, p in e.named_parameters():
            if p.dim() == 1:
                base = 1.0 if n.endswith("norm1__weight") or n.endswith("norm2__weight") or n == "norm__weight" else 0.0
                p.copy_((base + 0.1 * torch.randn(p.shape, generator=g)).to(DEV))
    return e


def _oracle_grads(enc, images, R, emulate=False):
    from oracle import vit as ovit
    p = {k: v.detach().cpu().float().clone().requires_grad_(True) for k, v in enc.state_dict().items()}
    tok = ovit.forward_tokens(p, images.cpu(), emulate_fp16=emulate)
    (tok * R.cpu()).sum().backward()
    return {k: v.grad for k, v in p.items()}


def _gpu_grads(enc, images, R):
    enc.zero_grad(set_to_none=True)
    tok = enc.forward_tokens(images)
    (tok * R).sum().backward()
    return {n: enc._get(n).grad.detach().cpu().clone() for n in enc._names}


def _images(n, img, seed):
    return torch.randn(n, 3, img, img, generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_trainable_forward_is_the_unfolded_forward():
    from isic_hip.vit import ViTSmallEncoder
    enc = _enc(img=224, depth=2)
    ref = ViTSmallEncoder(img_size=224, depth=2, fold_layernorm=False).to(DEV)
    ref.load_state_dict(enc.state_dict())
    x = _images(3, 224, 1)
    want = ref.run_tokens(x)
    with torch.no_grad():
        assert torch.equal(enc.forward_tokens(x), want)
    enc.train()
    tok = enc.forward_tokens(x)
    assert tok.requires_grad and torch.equal(tok.detach(), want)


@pytest.mark.parametrize("img,depth,n", [(224, 1, 3), (224, 2, 3), (32, 12, 5)])
def test_encoder_gradients_match_oracle(img, depth, n):
    enc = _enc(img=img, depth=depth)
    enc.train()
    x = _images(n, img, 2)
    R = torch.randn(n, enc.tokens, enc.dim, generator=torch.Generator().manual_seed(3)).to(DEV)
    got = _gpu_grads(enc, x, R)
    ref = _oracle_grads(enc, x, R)
    ref16 = _oracle_grads(enc, x, R, emulate=True)
    worst = max(enc._names, key=lambda k: _relf(got[k], ref[k]))
    msg = (f"worst {worst}: rel Frobenius {_relf(got[worst], ref[worst]):.3e} vs fp32 oracle, "
           f"{_relf(got[worst], ref16[worst]):.3e} vs emulate_fp16 oracle; min cosine "
           f"{min(_cos(got[k], ref[k]) for k in enc._names):.5f}")
    print(msg)
    if depth <= 2:
        assert _relf(got[worst], ref[worst]) <= 3e-2, msg
    else:
        assert all(_cos(got[k], ref[k]) >= 0.99 for k in enc._names), msg


def test_loss_scale_invariance():
    enc = _enc(img=224, depth=1)
    enc.train()
    x = _images(3, 224, 4)
    R = torch.randn(3, enc.tokens, enc.dim, generator=torch.Generator().manual_seed(5)).to(DEV)
    ref = _oracle_grads(enc, x, R)
    base = _gpu_grads(enc, x, R)
    for f in (2.0 ** -20, 2.0 ** 6):
        got = _gpu_grads(enc, x, R * f)
        for k in enc._names:
            assert bool(torch.isfinite(got[k]).all()), k
            assert _relf(got[k], ref[k] * f) <= 3e-2, (f, k, _relf(got[k], ref[k] * f))
            assert torch.equal(got[k], base[k] * f), (f, k)      # a power-of-two loss scale: exactly equivariant


def _adamw_step(enc, x, R, opt):
    opt.zero_grad()
    (enc.forward_tokens(x) * R).sum().backward()
    grads = [p.grad.detach().clone() for p in enc.parameters()]
    opt.step()
    return grads, [p.detach().clone() for p in enc.parameters()]


def test_reproducible_step_and_weight_refresh():
    from isic_hip import optim
    from isic_hip.vit import ViTSmallEncoder
    x = _images(3, 224, 6)
    R = torch.randn(3, 196, 384, generator=torch.Generator().manual_seed(7)).to(DEV)
    runs = []
    for _ in range(2):
        enc = _enc(img=224, depth=2, seed=1)
        enc.train()
        opt = optim.AdamW(enc.parameters(), lr=1e-3, weight_decay=1e-4)
        runs.append(_adamw_step(enc, x, R, opt))
    for a, b in zip(runs[0][0] + runs[0][1], runs[1][0] + runs[1][1]):
        assert torch.equal(a, b)
    # the step wrote the flat buffer in place: the next forward must use the new weights
    with torch.no_grad():
        after = enc.forward_tokens(x)
        fresh = ViTSmallEncoder(img_size=224, depth=2, trainable=True).to(DEV)
        fresh.load_state_dict(enc.state_dict())
        before = _enc(img=224, depth=2, seed=1).forward_tokens(x)
        assert not torch.equal(after, before)
        assert torch.equal(after, fresh.forward_tokens(x))


def test_grad_ready_hook_reports_every_parameter_once_in_reverse_block_order():
    enc = _enc(img=32, depth=3)
    enc.train()
    names = [n for n, _ in enc.named_parameters()]
    seen, snaps = [], {}

    def hook(group):
        torch.cuda.synchronize()
        for n in group:
            snaps[n] = getattr(enc, n).grad.detach().clone()
        seen.append(list(group))
    enc.grad_ready_hook = hook
    x = _images(4, 32, 8)
    (enc.forward_tokens(x) * 3.0).sum().backward()
    flat = [n for grp in seen for n in grp]
    assert sorted(flat) == sorted(names) and len(flat) == len(set(flat))
    order = [int(grp[0].split("__")[1]) for grp in seen if grp[0].startswith("blocks__")]
    assert order == sorted(order, reverse=True) == [2, 1, 0]
    assert seen[0][0].startswith("norm__") and "pos_embed" in seen[-1]
    for n in names:
        assert torch.equal(snaps[n], getattr(enc, n).grad), n


def _milnet(seed=0):
    from model import MultiModalMILNet
    torch.manual_seed(seed)
    return MultiModalMILNet(hidden_dim=64, att_dim=32, dropout=0.0, radiomics_dim=16, num_classes=3, encoder="vit_s16",
                            encoder_kwargs=dict(img_size=32, depth=2)).to(DEV)


def test_milnet_vit_loss_and_head_gradients_match_oracle():
    from oracle import fusion, mil
    from oracle.model import milnet_loss, sub
    from oracle import vit as ovit
    net = _milnet()
    net.eval()                                       # no dropout: the comparison is deterministic
    B, K = 4, 3
    g = torch.Generator().manual_seed(9)
    img = torch.randn(B, K, 3, 32, 32, generator=g)
    rad = torch.randn(B, 16, generator=g)
    y = torch.arange(B) % 3
    net.zero_grad(set_to_none=True)
    out = net(img.to(DEV), rad.to(DEV))
    loss = net.loss(out, y.to(DEV))
    loss.backward()
    def oracle(emulate):
        p = {k: v.detach().cpu().float().clone().requires_grad_(True) for k, v in net.state_dict().items()
             if v.dtype.is_floating_point}
        feats = ovit.forward_tokens(sub(p, "encoder"), img.view(B * K, 3, 32, 32), emulate_fp16=emulate).mean(dim=1)
        offs = np.arange(B + 1) * K
        o = mil.teacher_forward_batched(sub(p, "mil"), feats, offs)
        z = torch.stack([(o["attention"][lo:hi, None] * o["hidden"][lo:hi]).sum(0) for lo, hi in zip(offs[:-1], offs[1:])])
        fused = torch.cat([fusion.mlp_ln_relu(p, "image_proj", z, None, (0.3, 0.2), 0),
                           fusion.mlp_ln_relu(p, "radiomics_mlp", rad, None, (0.4, 0.3), 2)], dim=1)
        o["logits"] = fusion.fusion_mlp(p, fused, None, 8)
        l = milnet_loss(o, y)
        l.backward()
        return l, {k: v.grad for k, v in p.items()}
    ref_loss, ref = oracle(False)
    _, ref16 = oracle(True)
    assert abs(float(loss) - float(ref_loss)) <= 3e-2 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    named = dict(net.named_parameters())
    for k, v in ref.items():
        pk = "encoder." + k[len("encoder."):].replace(".", "__") if k.startswith("encoder.") else k
        got = named[pk].grad
        assert got is not None, k
        err = _relf(got.cpu(), v)
        if k.startswith("encoder."):
            assert _cos(got.cpu(), v) >= 0.99, (k, err)
        else:
            # measured yardstick: a head gradient moves with the fp16 rounding of the encoder's features by as much as the
            # oracle itself shows between its emulate_fp16 and fp32 forms (token-mean features of a random encoder are
            # close across images, so sum_b dh_b feat_b^T cancels: measured 1.9e-2, GPU 4.1e-2); held to 3x that spread, or 3e-2
            spread = _relf(ref16[k], v)
            assert err <= max(3e-2, 3.0 * spread), (k, err, spread)


def test_train_milnet_fold_runs_with_the_vit_encoder():
    from isic_hip.train import train_milnet_fold
    net = _milnet(seed=1)
    g = torch.Generator().manual_seed(11)

    def split(n):
        y = torch.arange(n) % 3
        img = torch.randn(n, 2, 3, 32, 32, generator=g) + 0.5 * y.view(-1, 1, 1, 1, 1)
        rad = torch.randn(n, 16, generator=g) + 2.0 * torch.nn.functional.one_hot(y, 16).float()
        return img, rad, y
    res = train_milnet_fold(net, split(24), split(9), lr=1e-3, epochs=2, patience=10, bags_per_step=4, num_classes=3,
                            device=torch.device(DEV), log=None)
    hist = res["history"]
    assert len(hist) == 2
    l1, l2 = (float(np.mean(h["train_losses"])) for h in hist)
    assert math.isfinite(l1) and math.isfinite(l2) and l2 < l1, (l1, l2)
    assert net.encoder.grad_ready_hook is None
