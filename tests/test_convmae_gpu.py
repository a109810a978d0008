"""ConvMAE-Base fp16 patch encoder through the C ABI vs the fp32 CPU restatement (tests/convmae_ref.py).

Single kernels are held to one fp16 rounding of the fp32 result computed from the same fp16 operands (patch rows: bit for
bit).  Every gemm_f16 shape the encoder adds is checked against an fp32 matmul before the encoder relies on it.  The whole
encoder is held to bounds set from the spreads measured on the MI355X (stated at the test)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-12))


# ---------------------------------------------------------------- the new kernels
@pytest.mark.parametrize("n,C,H,W", [(1, 256, 56, 56), (3, 384, 28, 28), (2, 256, 13, 13), (5, 384, 7, 7), (1, 64, 30, 9),
                                     (3, 128, 1, 33)])
def test_dwconv5x5_matches_grouped_conv2d(n, C, H, W):
    from isic_hip.lib import call
    g = torch.Generator().manual_seed(n * 1000 + C + H)
    x = torch.randn(n, H, W, C, generator=g).to(F16)
    w = torch.randn(C, 1, 5, 5, generator=g) / 5
    b = torch.randn(C, generator=g) * 0.1
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=2, groups=C).permute(0, 2, 3, 1)
    y = torch.full((n, H, W, C), float("nan"), device=DEV, dtype=F16)
    call("isic_dwconv5x5_f16", x.to(DEV), w.reshape(C, 25).t().contiguous().to(DEV), b.to(DEV), y, n, H, W, C)
    got = y.double().cpu()
    assert bool(torch.isfinite(got).all())
    tol = 2.0 ** -11 * ref.abs() + 1e-6 * float(ref.abs().max()) + 2.0 ** -24      # one fp16 rounding + fp32 summation
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() - tol).max())


@pytest.mark.parametrize("n,H,W,C,P", [(2, 56, 56, 256, 4), (3, 56, 56, 256, 2), (1, 28, 28, 384, 2), (2, 12, 8, 16, 4)])
def test_patch_rows_nhwc_match_unfold(n, H, W, C, P):
    from isic_hip.lib import call
    g = torch.Generator().manual_seed(H + C + P)
    x = torch.randn(n, H, W, C, generator=g).to(F16)
    u = F.unfold(x.float().permute(0, 3, 1, 2), kernel_size=P, stride=P)                  # [n, C*P*P, L], (c, kh, kw)
    ref = u.view(n, C, P, P, -1).permute(0, 4, 2, 3, 1).reshape(-1, P * P * C).to(F16)      # rows in (kh, kw, c) order
    rows = torch.empty(ref.shape, device=DEV, dtype=F16)
    call("isic_patch_rows_nhwc_f16", x.to(DEV), rows, n, H, W, C, P)
    assert torch.equal(rows.cpu().view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("n,C,H,W,P,K", [(3, 3, 224, 224, 4, 64), (1, 3, 224, 224, 4, 48), (2, 5, 16, 8, 2, 24)])
def test_patch_rows_nchw_match_unfold(n, C, H, W, P, K):
    from isic_hip.lib import call
    g = torch.Generator().manual_seed(C + H + K)
    img = torch.randn(n, C, H, W, generator=g)
    u = F.unfold(img, kernel_size=P, stride=P)
    ref = u.view(n, C, P, P, -1).permute(0, 4, 2, 3, 1).reshape(-1, P * P * C)
    ref = F.pad(ref, (0, K - P * P * C)).to(F16)
    rows = torch.full(ref.shape, float("nan"), device=DEV, dtype=F16)
    call("isic_patch_rows_nchw_f32", img.to(DEV), rows, n, C, H, W, P, K)
    assert torch.equal(rows.cpu().view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("N,addends,act", [(256, 0, 1), (384, 0, 1), (768, 2, 0), (768, 1, 1), (1024, 2, 0), (64, 0, 0)])
def test_layernorm_add_matches_torch(N, addends, act):
    from f16_kernel_ref import layernorm_add_fwd_errors, layernorm_add_ref
    from isic_hip.lib import call
    g = torch.Generator().manual_seed(N + addends)
    M = 777
    xs = [(torch.randn(M, N, generator=g) * 2 + torch.randn(M, 1, generator=g)).to(F16) for _ in range(1 + addends)]
    gm, bt = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    ref = layernorm_add_ref(xs, gm, bt, 1e-5, act)
    y = torch.empty(M, N, device=DEV, dtype=F16)
    y32 = torch.empty(M, N, device=DEV, dtype=torch.float32)
    d = [t.to(DEV) for t in xs] + [None, None]
    call("isic_layernorm_add_f16", d[0], d[1], d[2], gm.to(DEV), bt.to(DEV), y, y32, M, N, act, 1e-5)
    ok32, ok16 = layernorm_add_fwd_errors(y32, y, ref)           # tests/f16_kernel_ref.py: the bounds this test set
    assert ok32 and ok16


# ---------------------------------------------------------------- gemm_f16 at the shapes the encoder adds
def _rows(M):
    """rows checked against the CPU matmul: all of them for small M, a seeded sample + the first / last tiles otherwise"""
    if M <= 20000:
        return torch.arange(M)
    g = torch.Generator().manual_seed(M)
    return torch.cat([torch.arange(300), torch.randint(0, M, (4000,), generator=g), torch.arange(M - 300, M)])


@pytest.mark.parametrize("M,N,K,act,res", [
    (6272, 256, 64, 0, None),          # stem (K 48 padded to 64)
    (6272, 256, 256, 0, "full"),       # CBlock(256) conv2 + residual
    (6272, 1024, 256, 1, None),        # CBlock(256) fc1 + GELU (unfolded form)
    (6272, 256, 1024, 0, "full"),      # CBlock(256) fc2 + residual
    (1568, 384, 1024, 0, None),        # patch_embed2
    (1568, 1536, 384, 1, None),        # CBlock(384) fc1
    (1568, 384, 1536, 0, "full"),      # CBlock(384) fc2
    (392, 768, 4096, 0, None),         # stage1_output_decode
    (392, 768, 1536, 0, None),         # stage2_output_decode / patch_embed3
    (392, 768, 768, 0, "pos"),         # patch_embed4 + pos_embed
    (2744, 2304, 768, 0, None),        # blocks3 qkv (unfolded form)
    (2744, 3072, 768, 1, None),        # blocks3 fc1
    (2744, 768, 3072, 0, "full"),      # blocks3 fc2
    (802816, 256, 256, 0, "full"),     # a 256-image chunk of stage 1
    (802816, 1024, 256, 1, None),
])
def test_gemm_f16_at_the_encoder_shapes(M, N, K, act, res):
    from isic_hip.lib import call
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(F16)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(F16)
    b = torch.randn(N, generator=g) * 0.1
    rr = 196 if res == "pos" else 0
    R = None if res is None else torch.randn(rr or M, N, generator=g).to(F16)
    C = torch.full((M, N), float("nan"), device=DEV, dtype=F16)
    call("isic_gemm_f16", A.to(DEV), W.to(DEV), b.to(DEV), None if R is None else R.to(DEV), C, M, N, K, act, rr)
    idx = _rows(M)
    ref = A[idx].float() @ W.float().t() + b
    if act:
        ref = F.gelu(ref)
    if R is not None:
        ref = ref + (R.float()[idx] if rr == 0 else R.float()[idx % rr])
    got = C[idx.to(DEV)].float().cpu()
    assert bool(torch.isfinite(C).all())
    tol = 2.0 ** -10 * ref.abs() + 2e-3
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() - tol).max())
    if res == "full":           # the statistics epilogue at this shape: same C bit for bit, row sums of it
        parts = 2 * N // 128
        C1 = torch.empty_like(C)
        st = torch.empty((M, parts, 2), device=DEV)
        call("isic_gemm_f16_stats", A.to(DEV), W.to(DEV), b.to(DEV), R.to(DEV), C1, st, M, N, K, 0, 0)
        assert torch.equal(C.view(torch.int16), C1.view(torch.int16))
        grp = C1.cpu()[idx].double().view(-1, parts, 64)
        assert float((st.cpu()[idx, :, 0].double() - grp.sum(-1)).abs().max()) <= 1e-5 * float(grp.abs().sum(-1).max())


@pytest.mark.parametrize("M,N,K,act,parts", [(6272, 256, 256, 0, 0), (6272, 1024, 256, 1, 4), (1568, 384, 384, 0, 0),
                                             (1568, 1536, 384, 1, 6), (2744, 2304, 768, 0, 12), (2744, 3072, 768, 1, 12)])
def test_gemm_f16_ln_at_the_encoder_shapes(M, N, K, act, parts):
    """the folded LayerNorm with (mean, rstd) from isic_row_stats_f16 (parts 0: a stage's first block) or with the partial
    sums of a statistics epilogue (parts = 2 K / 128)"""
    from isic_hip.lib import call
    g = torch.Generator().manual_seed(M + N + K + act)
    x = (torch.randn(M, K, generator=g) * (1.0 + torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)).to(F16)
    gamma, beta = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.2
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(F16)
    b = torch.randn(N, generator=g) * 0.1
    eps = 1e-5
    ref = F.layer_norm(x.float(), (K,), gamma, beta, eps) @ W.float().t() + b
    if act:
        ref = F.gelu(ref)
    Wg = (W.float() * gamma[None, :]).to(F16)
    c, bb = Wg.float().sum(dim=1), b + W.float() @ beta
    xd = x.to(DEV)
    if parts == 0:
        st = torch.empty((M, 2), device=DEV)
        call("isic_row_stats_f16", xd, st, M, K, eps)
    else:                                 # partial (sum, sum of squares) per 64 columns, as the producing epilogue writes
        st = torch.empty((M, parts, 2), device=DEV)
        z = torch.zeros(M, 64, device=DEV, dtype=F16)
        copy = torch.empty_like(xd)
        call("isic_gemm_f16_stats", z, torch.zeros(K, 64, device=DEV, dtype=F16), torch.zeros(K, device=DEV), xd, copy, st,
             M, K, 64, 0, 0)
    C = torch.full((M, N), float("nan"), device=DEV, dtype=F16)
    call("isic_gemm_f16_ln", xd, Wg.to(DEV), bb.to(DEV), c.to(DEV), st, parts, C, M, N, K, act, eps)
    got = C.float().cpu()
    assert bool(torch.isfinite(got).all())
    tol = 2.0 ** -10 * ref.abs() + 3e-3
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() - tol).max())


# ---------------------------------------------------------------- the encoder
def _encoder(fold=True, seed=5, **kw):
    from isic_hip.convmae import ConvMAEBaseEncoder
    import convmae_ref as ref
    p = ref.init_params(seed)
    enc = ConvMAEBaseEncoder(fold_layernorm=fold, **kw).to(DEV)
    enc.load_state_dict(p)
    return enc, p, ref


def _images(n, seed=11):
    return torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("fold", [True, False])
def test_encoder_tokens_match_the_restatement(fold):
    """Bounds from the spreads measured on the MI355X (max |error| over max |reference|): full depth 1.9e-3 / 2.0e-3 (fold /
    unfolded) against the emulated-fp16 restatement and 1.5e-3 / 1.5e-3 against fp32 (the emulation itself sits 1.6e-3 from
    fp32 on the CPU); one block per stage 1.1e-3 / 0.8e-3.  Held at about 2.5x: 5e-3 full depth, 3e-3 one block per stage."""
    enc, p, ref = _encoder(fold)
    x = _images(2)
    got = enc.run_tokens(x.to(DEV)).cpu()
    assert got.shape == (2, 196, 768) and bool(torch.isfinite(got).all())
    e16, e32 = _rel(got, ref.forward_tokens(p, x, emulate_fp16=True)), _rel(got, ref.forward_tokens(p, x))
    one = enc.run_tokens(x.to(DEV), depth=(1, 1, 1)).cpu()
    e1 = _rel(one, ref.forward_tokens(p, x, emulate_fp16=True, depth=(1, 1, 1)))
    print(f"[convmae] fold={fold}: rel err vs emulated fp16 {e16:.3e}, vs fp32 {e32:.3e}, one block per stage {e1:.3e}")
    assert e16 <= 5e-3, e16
    assert e32 <= 5e-3, e32
    assert e1 <= 3e-3, e1


def test_checkpoint_round_trip(tmp_path):
    """a full MAE checkpoint (encoder + decoder keys) through torch.save / torch.load loads into a fresh encoder, which
    then gives the same tokens bit for bit"""
    from isic_hip.convmae import ConvMAEBaseEncoder
    enc, p, _ = _encoder(seed=7)
    sd = {k: v.clone() for k, v in p.items()}
    sd["mask_token"] = torch.zeros(1, 1, 512)
    sd["decoder_embed.weight"] = torch.randn(512, 768)
    path = tmp_path / "convmae.pth"
    torch.save(sd, path)
    fresh = ConvMAEBaseEncoder(seed=1).to(DEV)
    x = _images(2, seed=3).to(DEV)
    before = fresh.run_tokens(x)
    res = fresh.load_state_dict(torch.load(path, map_location=DEV, weights_only=True), strict=False)
    assert list(res.missing_keys) == [] and set(res.unexpected_keys) == {"mask_token", "decoder_embed.weight"}
    after = fresh.run_tokens(x)
    assert not torch.equal(before, after)                        # the prepared weights follow the load
    assert torch.equal(after, enc.run_tokens(x))


def test_batch_invariance_and_run_to_run_reproducibility():
    enc, _, _ = _encoder()
    x = _images(7, seed=4).to(DEV)
    a = enc.run_tokens(x)
    b = enc.run_tokens(x)
    assert torch.equal(a, b)
    one = enc.run_tokens(x[3:4])
    assert torch.equal(one, a[3:4])


def test_large_batch_in_chunks():
    """600 images in chunks of 256 (the default max_batch): finite, a chunk boundary does not change an image's tokens, and
    sampled images match the restatement at the bounds of test_encoder_tokens_match_the_restatement"""
    enc, p, ref = _encoder()
    n = 600
    x = _images(n, seed=9)
    got = enc.run_tokens(x.to(DEV))
    assert got.shape == (n, 196, 768) and bool(torch.isfinite(got).all())
    for i in (0, 255, 256, 599):
        assert _rel(got[i:i + 1].cpu(), ref.forward_tokens(p, x[i:i + 1], emulate_fp16=True)) <= 5e-3, i
    assert torch.equal(enc.run_tokens(x[250:262].to(DEV)), got[250:262])


def test_extract_latents_with_convmae_feeds_the_d768_teacher(tmp_path, monkeypatch):
    import save_latent as sl
    from utils_g_mil import AttentionMIL_teacher
    monkeypatch.chdir(tmp_path)
    cfg = {"device": DEV, "seed": 42, "pca": False, "encoder": "convmae_base"}
    tv, te = sl.SyntheticDermImages(n=5, seed=1), sl.SyntheticDermImages(n=3, seed=2)
    ptr, pte, pool_tr, pool_te, raw_tr, raw_te = sl.extract_latents(cfg, "missing.pth", datasets=(tv, te), batch_size=4)
    assert len(pool_tr) == 5 and len(raw_te) == 3 and raw_tr["latent"].iloc[0].shape == (196, 768)
    assert np.array_equal(raw_tr["ids_keep"].iloc[1], np.arange(196))
    assert len(ptr) == 5 * 196 and ptr["patch_latent"].iloc[0].shape == (768,)
    lat = np.stack(list(raw_tr["latent"]))
    assert np.isfinite(lat).all() and lat.std() > 0.1
    torch.manual_seed(0)
    teacher = AttentionMIL_teacher(768, 64, 32, dropout=0.0, num_classes=7).to(DEV).eval()
    bag = torch.from_numpy(np.stack(list(ptr["patch_latent"].iloc[:196]))).float().to(DEV)
    out = teacher(bag)
    assert all(bool(torch.isfinite(v).all()) for v in out.values() if isinstance(v, torch.Tensor))
