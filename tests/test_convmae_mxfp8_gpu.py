"""MXFP8 path of the ConvMAE-Base encoder (csrc/convmae_mxfp8.hip, isic_hip/convmae.py precision="mxfp8") against the
quantisation rule of tests/mxfp8_ref.py and the CPU emulation of tests/convmae_mxfp8_ref.py.

The three kernels are held bit for bit: the LayerNorm to the quantisation of what isic_layernorm_add_f16 writes in fp32,
the patch rows to the quantisation of isic_patch_rows_nhwc_f16's rows, the depthwise 5x5 on integer data (every fp32 sum
exact) to the quantisation of F.conv2d; on real data the depthwise output takes the criteria test_mxfp8_gpu.py applies to
the MXFP8 output of a product (a 25-term sum is less order-sensitive than the K = 384 products they were measured on).
The encoder bounds stand on the emulation's own figures, which test_convmae_mxfp8_cpu.py recomputes (E32: the emulation
against the fp32 oracle, E64: against itself with fp64 products).  No value measured on the MI355X stands next to a bound yet: each test prints its
figure before it asserts, to be recorded in its docstring from the first run."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convmae_mxfp8_ref as cmr
import convmae_ref as cr
import mxfp8_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16
U8 = torch.uint8
DW_TH, DW_TW = 7, 28                                # the depthwise kernel's tile (csrc/convmae_kernels.inc)


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _mx_out(M, K):
    return torch.full((M, K), 0xFF, device=DEV, dtype=U8), torch.full((M, K // 32), 0xFF, device=DEV, dtype=U8)


def _relf(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _assert_bits(q, s, rq, rs):
    assert torch.equal(s, rs), int((s != rs).sum())
    assert torch.equal(q, rq), int((q != rq).sum())


# ---------------------------------------------------------------- LayerNorm -> MX
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M", [1, 5, 1027])
@pytest.mark.parametrize("N", [64, 256, 384, 768, 1024])
def test_layernorm_act_mxfp8_is_the_quantised_fp32_layernorm(N, M, act):
    g = torch.Generator().manual_seed(N + 7 * M + act)
    x = (torch.randn(M, N, generator=g) * 2 + torch.randn(M, 1, generator=g) * 3).to(F16)
    if M >= 5:
        x[1, 17] = 300.0                                  # a massive channel
        x[2] = 1.375                                      # a constant row
        x[3] = 0.0                                        # an all-zero row
    else:
        x[0, N - 3] = 300.0
    gamma, beta = 1 + 0.3 * torch.randn(N, generator=g), 0.2 * torch.randn(N, generator=g)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y32 = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32)
    _call("isic_layernorm_add_f16", xd, None, None, gd, bd, None, y32, M, N, act, 1e-5)
    q, s = _mx_out(M, N)
    _call("isic_layernorm_act_mxfp8_f16", xd, gd, bd, q, s, M, N, act, 1e-5)
    y32 = y32.cpu()
    assert bool(torch.isfinite(y32).all())
    ref = F.layer_norm(x.float(), (N,), gamma, beta, 1e-5)
    ref = F.gelu(ref) if act else ref
    assert float((y32 - ref).abs().max()) <= 1e-3 * max(1.0, float(ref.abs().max()))     # the right function at all
    _assert_bits(q.cpu(), s.cpu(), *mr.quantize(y32))


# ---------------------------------------------------------------- depthwise 5x5 -> MX
# (2,1,1,64), (2,3,5,64): every pixel on a border.  (1,29,30,128): 29 = 4 DW_TH + 1 is one row past a tile edge and 30
# = DW_TW + 2 puts two columns in a second tile; (1,29,29,128) adds the column tile of width one.
DW_SHAPES = [(2, 1, 1, 64), (2, 3, 5, 64), (1, 7, 7, 384), (2, 14, 9, 256), (1, 29, 30, 128), (1, 29, 29, 128)]
assert 29 % DW_TH == 1 and 29 % DW_TW == 1 and DW_TW < 30 < 2 * DW_TW


def _dw_gpu(x, w, b):
    n, H, W, C = x.shape
    q, s = _mx_out(n * H * W, C)
    _call("isic_dwconv5x5_mxfp8_f16", x.to(DEV).contiguous(), w.reshape(C, 25).t().contiguous().to(DEV),
          None if b is None else b.to(DEV), q, s, n, H, W, C)
    return q.cpu(), s.cpu()


def _dw_ref(x, w, b, dtype=torch.float32):
    C = x.shape[-1]
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype), None if b is None else b.to(dtype), padding=2, groups=C)
    return y.permute(0, 2, 3, 1).reshape(-1, C).float()


@pytest.mark.parametrize("n,H,W,C", DW_SHAPES)
def test_dwconv5x5_mxfp8_integer_data_is_bit_exact(n, H, W, C):
    g = torch.Generator().manual_seed(n + H + W + C)
    x = torch.randint(-8, 9, (n, H, W, C), generator=g).to(F16)
    w = torch.randint(-4, 5, (C, 1, 5, 5), generator=g).float()
    b = torch.randint(-4, 5, (C,), generator=g).float()
    x[0, 0, 0, :32] = 0                                   # with zero taps and bias: an all-zero block
    w[:32], b[:32] = 0, 0
    ref = _dw_ref(x, w, b)                                # |sum| <= 25 * 32 + 4: exact in fp32 in any order
    _assert_bits(*_dw_gpu(x, w, b), *mr.quantize(ref))
    _assert_bits(*_dw_gpu(x, w, None), *mr.quantize(_dw_ref(x, w, None)))      # bias = NULL


@pytest.mark.parametrize("n,H,W,C", DW_SHAPES)
def test_dwconv5x5_mxfp8_real_data_matches_the_quantised_convolution(n, H, W, C):
    g = torch.Generator().manual_seed(3 * n + H + W + C)
    x = (torch.randn(n, H, W, C, generator=g) * (1 + 3 * torch.rand(1, 1, 1, C, generator=g))).to(F16)
    w = torch.randn(C, 1, 5, 5, generator=g) / 5
    b = torch.randn(C, generator=g) * 0.1
    q, s = _dw_gpu(x, w, b)
    ref = _dw_ref(x, w, b, torch.float64)
    rq, rs = mr.quantize(ref)
    assert (s != rs).float().mean().item() <= 1e-5
    assert (q == rq).float().mean().item() >= 0.998
    step = mr.e4m3_step(rq).float() * mr._POW2[rs.long()].float().repeat_interleave(32, 1)
    step = step + 1e-3 * ref.pow(2).mean().sqrt()
    ok = ((mr.dequantize(q, s) - mr.dequantize(rq, rs)).abs() <= step) | (s != rs).repeat_interleave(32, 1)
    assert bool(ok.all())
    if n == 2:                                            # an image's border does not read its neighbour in the batch
        for i in range(2):
            qi, si = _dw_gpu(x[i:i + 1], w, b)
            assert torch.equal(qi, q.view(2, -1, C)[i]) and torch.equal(si, s.view(2, -1, C // 32)[i])


# ---------------------------------------------------------------- patch rows -> MX
def _special_blocks(dtype):
    """the hand-made 32-element blocks of test_mxfp8_gpu._special_rows: all zero (with -0), amax = 448 * 2^e and just
    above, a lone outlier over tiny values (e4m3 subnormals), fp16 extremes"""
    b = torch.zeros(8, 32)
    b[0, :] = -0.0
    b[1, 8] = 448.0; b[1, 9] = -224.0; b[1, 10] = -0.0
    b[2, 0] = 448.0 * 2.0 ** -20 * (1 + 2.0 ** -9); b[2, 1] = 1e-9
    b[3, :] = 1e-3; b[3, 5] = 100.0
    b[4, 0] = 448.0; b[4, 1:6] = torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -11, -5 * 2.0 ** -10, -2.0 ** -12])
    b[5, 0] = 65504.0; b[5, 1] = 6e-8; b[5, 2] = -6e-8
    b[6, 8] = 6e-8
    b[7, 6] = -65504.0; b[7, 7] = 1.0
    return b.to(dtype)


@pytest.mark.parametrize("big", [False, True], ids=["one_patch", "2x3_patches"])
@pytest.mark.parametrize("C", [32, 96, 256])
@pytest.mark.parametrize("P", [2, 4])
def test_patch_rows_mxfp8_are_the_quantised_fp16_rows(P, C, big):
    n, (H, W) = 2, ((2 * P, 3 * P) if big else (P, P))
    g = torch.Generator().manual_seed(P + C + H)
    x = torch.randn(n, H, W, C, generator=g) * torch.exp2(torch.randint(-10, 10, (n, H, W, C // 32), generator=g).float()
                                                          ).repeat_interleave(32, 3)
    x = x.to(F16)
    blocks, sp = x.view(-1, 32), _special_blocks(F16)
    at = torch.arange(0, blocks.shape[0], max(1, blocks.shape[0] // 8))[:8]      # spread over pixels and images
    blocks[at] = sp[: len(at)]
    rows_n, K = n * (H // P) * (W // P), P * P * C
    rows = torch.full((rows_n, K), float("nan"), device=DEV, dtype=F16)
    _call("isic_patch_rows_nhwc_f16", x.to(DEV), rows, n, H, W, C, P)
    q, s = _mx_out(rows_n, K)
    _call("isic_patch_rows_mxfp8_nhwc_f16", x.to(DEV), q, s, n, H, W, C, P)
    rows = rows.cpu()
    assert bool(torch.isfinite(rows).all()) and sorted(rows.flatten().tolist()) == sorted(x.flatten().tolist())
    _assert_bits(q.cpu(), s.cpu(), *mr.quantize(rows))


# ---------------------------------------------------------------- isic_gemm_mxfp8 at the widths the encoder adds
def _quant_gpu(x):
    M, K = x.shape
    q, s = _mx_out(M, K)
    _call("isic_mxfp8_quantize", x.to(DEV).contiguous(), 1, q, s, M, K)
    return q, s


@pytest.mark.parametrize("M,N,K,rr", [(197, 256, 256, 0), (50, 768, 4096, 0), (393, 2304, 768, 0), (392, 768, 768, 196)])
def test_gemm_mxfp8_integer_operands_are_exact_at_the_convmae_widths(M, N, K, rr):
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randint(-8, 9, (M, K), generator=g).float()
    W = torch.randint(-8, 9, (N, K), generator=g).float()
    A = A * torch.exp2(torch.randint(-3, 3, (M, K // 32), generator=g).float()).repeat_interleave(32, 1)
    W = W * torch.exp2(torch.randint(-3, 3, (N, K // 32), generator=g).float()).repeat_interleave(32, 1)
    b = torch.randint(-4, 5, (N,), generator=g).float()
    R = torch.randint(-16, 17, (rr, N), generator=g).to(F16) if rr else None
    (Aq, As), (Wq, Ws) = _quant_gpu(A), _quant_gpu(W)
    C = torch.full((M, N), float("nan"), device=DEV, dtype=F16)
    _call("isic_gemm_mxfp8", Aq, As, Wq, Ws, b.to(DEV), None if R is None else R.to(DEV), C, None, None, M, N, K, 0, rr)
    ref = mr.dequantize(Aq.cpu(), As.cpu()).double() @ mr.dequantize(Wq.cpu(), Ws.cpu()).double().t() + b.double()
    if rr:
        ref = ref + R.double()[torch.arange(M) % rr]
    assert torch.equal(mr.dequantize(Aq.cpu(), As.cpu()), A) and torch.equal(mr.dequantize(Wq.cpu(), Ws.cpu()), W)
    # every term is a multiple of 2^-6 and every partial sum far below 2^18: exact in fp32 in any order; one fp16 rounding
    assert bool((ref.abs() < 60000).all())
    assert torch.equal(C.cpu(), ref.to(F16)), int((C.cpu() != ref.to(F16)).sum())


# ---------------------------------------------------------------- the encoder
def _images(n, seed=11):
    return torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _params(seed):
    return cr.init_params(seed)


@functools.lru_cache(maxsize=None)
def _emulation(seed, depth):
    """the CPU emulation for init_params(seed) and the two images of seed 11: computed once per (seed, depth)"""
    return cmr.forward_tokens_mxfp8(_params(seed), _images(2), depth=depth)


@functools.lru_cache(maxsize=None)
def _encoder(seed=0, **kw):
    from isic_hip.convmae import ConvMAEBaseEncoder
    enc = ConvMAEBaseEncoder(precision="mxfp8", **kw).to(DEV)
    enc.load_state_dict(_params(seed))
    return enc


def _tokens(depth, seed=0):
    got = _encoder(seed).run_tokens(_images(2).to(DEV), depth=depth).cpu()
    assert got.shape == (2, 196, 768) and bool(torch.isfinite(got).all())
    return got


E32 = {(1, 0, 0): 0.0666, (1, 1, 1): 0.0804}            # the emulation against the fp32 oracle at that depth (CPU figures)


def test_encoder_mxfp8_front_matches_the_emulation():
    """Depth (0,0,0): the stem, the MXFP8 patch rows, both decoders, patch_embed2-4.  <= 2e-2, the project's bound for one
    MXFP8 block (whose E64 is 6.1e-4; this depth's is 8.6e-4).  Not yet measured on the MI355X."""
    d = _relf(_tokens((0, 0, 0)), _emulation(0, (0, 0, 0)))
    print(f"depth (0,0,0) vs emulation: {d:.3e}")
    assert d <= 2e-2, d


@pytest.mark.parametrize("depth", [(1, 0, 0), (1, 1, 1)])
def test_encoder_mxfp8_sits_closer_to_the_emulation_than_the_format_to_fp32(depth):
    """<= E32 of the depth (0.0666 / 0.0804).  Not yet measured on the MI355X."""
    d = _relf(_tokens(depth), _emulation(0, depth))
    print(f"depth {depth} vs emulation: {d:.3e}")
    assert d <= E32[depth], d


def test_encoder_mxfp8_full_depth_matches_the_emulation_and_fp32():
    """Full depth.  Against the emulation <= 0.1 (the project's figure for a stack whose E64 is 0.044; here 0.046);
    against the fp32 oracle twice the emulation's own distance: relative Frobenius <= 0.18 (emulation 0.0914), min
    per-token cosine >= 0.989 (emulation 0.99459).  Not yet measured on the MI355X."""
    got = _tokens(None)
    d = _relf(got, _emulation(0, None))
    ref32 = cr.forward_tokens(_params(0), _images(2))
    d32 = _relf(got, ref32)
    cos = float(F.cosine_similarity(got.double(), ref32.double(), dim=-1).min())
    print(f"full depth: vs emulation {d:.4f}, vs fp32 {d32:.4f}, min cosine {cos:.5f}")
    assert d <= 0.1, d
    assert d32 <= 0.18, d32
    assert cos >= 0.989, cos


def test_encoder_mxfp8_is_deterministic_and_batch_and_chunk_invariant():
    x = _images(3, seed=2).to(DEV)
    enc, depth = _encoder(0), (1, 1, 1)
    a = enc.run_tokens(x, depth=depth)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, enc.run_tokens(x, depth=depth))
    assert torch.equal(a[1:3], enc.run_tokens(x[1:3], depth=depth))
    assert torch.equal(a, _encoder(0, max_batch=1).run_tokens(x, depth=depth))


def test_encoder_mxfp8_weights_follow_load_state_dict():
    from isic_hip.convmae import ConvMAEBaseEncoder
    depth, x = (1, 0, 0), _images(2).to(DEV)
    enc = ConvMAEBaseEncoder(precision="mxfp8").to(DEV)
    enc.load_state_dict(_params(0))
    a = enc.run_tokens(x, depth=depth).cpu()
    assert torch.equal(a, _tokens(depth))
    enc.load_state_dict(_params(1))
    b = enc.run_tokens(x, depth=depth).cpu()
    assert not torch.equal(a, b)
    d = _relf(b, _emulation(1, depth))                   # stale weights would be off by O(1)
    print(f"depth (1,0,0) after load_state_dict vs emulation: {d:.3e}")
    assert d <= E32[depth], d


def test_extract_latents_with_the_mxfp8_convmae_encoder():
    """MXFP8 against fp16 within the two fp32-oracle bounds above (fp16 is 1.1e-3 from fp32).  Not yet measured on the
    MI355X."""
    import save_latent as sl
    tv, te = sl.SyntheticDermImages(n=5, seed=1), sl.SyntheticDermImages(n=3, seed=2)
    out = {}
    for prec in ("fp16", "mxfp8"):
        cfg = {"device": DEV, "seed": 42, "pca": False, "encoder": "convmae_base", "encoder_precision": prec}
        out[prec] = sl.extract_latents(cfg, "missing.pth", datasets=(tv, te), batch_size=4)
    for a, b in zip(out["fp16"], out["mxfp8"]):
        assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for i, n in ((4, 5), (5, 3)):                        # the raw latents of the train_val and the test images
        raw16, rawmx = out["fp16"][i], out["mxfp8"][i]
        assert len(rawmx) == n and (raw16[["image_path", "target"]].values == rawmx[["image_path", "target"]].values).all()
        assert all(v.shape == (196, 768) for v in rawmx["latent"])
    l16, lmx = (torch.from_numpy(np.stack(list(out[k][4]["latent"]) + list(out[k][5]["latent"]))).double()
                for k in ("fp16", "mxfp8"))
    cos = float(F.cosine_similarity(lmx, l16, dim=-1).min())
    print(f"extract_latents mxfp8 vs fp16: {_relf(lmx, l16):.4f}, min cosine {cos:.5f}")
    assert _relf(lmx, l16) <= 0.18, _relf(lmx, l16)
    assert cos >= 0.989, cos
