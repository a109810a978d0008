"""MXFP8 path of the ViT-S/16 encoder (csrc/mxfp8.hip, isic_hip/vit.py precision="mxfp8") against the CPU reference of
tests/mxfp8_ref.py.

The quantiser is bit-exact.  The products: every e4m3 x e4m3 product and every power-of-two scale is exact in fp32, so
against the fp32 matmul of the dequantised operands only the summation order and the output rounding remain.
Encoder bounds (224^2 images, n = 3, oracle/vit.py init_params(5)), measured with the CPU emulation on the build host:
  * the emulated MXFP8 forward against the fp32 oracle: relative Frobenius error 0.031 (depth 1) / 0.078 (12 blocks),
    minimum per-token cosine 0.9993 / 0.9957 -- the quantisation noise of 3-bit mantissas (the fp16 emulation: 0.0011 /
    0.99999);
  * the emulation against ITSELF with its products summed in fp64 instead of fp32: 6.1e-4 (depth 1) / 0.044 (12 blocks).
    A summation-order difference moves values across e4m3 rounding ties, each move is a whole e4m3 step, and over 12
    blocks those steps grow to the size of the quantisation noise itself.  So the kernels (another summation order) can be
    held tightly to the emulation for one block only.  On the MI355X the first block differs from the emulation by 7.9e-3
    (13x the fp64-vs-fp32 figure: the scaled MFMA's sums and the attention kernel are further from the CPU's order than
    fp64 is from fp32), so the bound there is 2e-2 (2.5x); for 12 blocks 0.1 against the emulation (2.3x the 0.044), and
    against fp32 relative Frobenius <= 0.15 (1.9x the 0.078) and min cosine >= 0.99 (0.0057 below the measured 0.9957).
MXFP8 output of a product: 99.87-99.90 % of the element bytes equal the reference quantiser's on the MI355X (a byte moves
when the summation order carries a value across an e4m3 rounding tie), so >= 99.8 % is required, and every other byte
within one e4m3 step plus the fp16 test's summation allowance."""
import math

import numpy as np
import pytest
import torch

import mxfp8_ref as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16
U8 = torch.uint8


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _quant_gpu(x):
    M, K = x.shape
    q = torch.full((M, K), 0xFF, device=DEV, dtype=U8)
    s = torch.full((M, K // 32), 0xFF, device=DEV, dtype=U8)
    _call("isic_mxfp8_quantize", x.to(DEV).contiguous(), 1 if x.dtype == torch.float32 else 0, q, s, M, K)
    return q.cpu(), s.cpu()


def _special_rows(K, dtype):
    """rows of hand-made blocks: all zero (with -0), amax = 448 * 2^e and just above, a lone outlier over tiny values
    (e4m3 subnormals), fp16 extremes"""
    r = torch.zeros(4, K)
    r[0, :32] = -0.0
    r[0, 40] = 448.0; r[0, 41] = -224.0; r[0, 42] = -0.0
    r[0, 64] = 448.0 * 2.0 ** -20 * (1 + 2.0 ** -9); r[0, 65] = 1e-9
    r[1, :32] = 1e-3; r[1, 5] = 100.0
    r[1, 32] = 448.0; r[1, 33:38] = torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -11, -5 * 2.0 ** -10, -2.0 ** -12])
    r[2, 0] = 65504.0; r[2, 1] = 6e-8; r[2, 2] = -6e-8; r[2, 40] = 6e-8; r[2, 70] = -65504.0; r[2, 71] = 1.0
    r[3] = torch.linspace(-3, 3, K)
    return r.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("M,K", [(1, 384), (197, 1536), (4099, 384)])
def test_quantize_is_bit_exact(M, K, dtype):
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-12, 12, (M, K // 32), generator=g).float()).repeat_interleave(32, 1)
    x = x.to(dtype)
    x[: min(M, 4)] = _special_rows(K, dtype)[: min(M, 4)]
    q, s = _quant_gpu(x)
    rq, rs = mr.quantize(x)
    assert torch.equal(s, rs), int((s != rs).sum())
    assert torch.equal(q, rq), int((q != rq).sum())


def test_layernorm_mxfp8_matches_layernorm_then_quantiser():
    M, D = 3001, 384
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(M, D, generator=g) * 2 + torch.randn(M, 1, generator=g) * 5).to(F16)
    x[5, 17] = 300.0                                    # a massive channel
    gamma, beta = 1 + 0.3 * torch.randn(D, generator=g), 0.2 * torch.randn(D, generator=g)
    q = torch.empty(M, D, device=DEV, dtype=U8)
    s = torch.empty(M, D // 32, device=DEV, dtype=U8)
    _call("isic_layernorm_mxfp8_f16", x.to(DEV), gamma.to(DEV), beta.to(DEV), q, s, M, D, 1e-6)
    q, s = q.cpu(), s.cpu()
    ref = torch.nn.functional.layer_norm(x.float(), (D,), gamma, beta, 1e-6)
    rq, rs = mr.quantize(ref)
    assert torch.equal(s, rs)
    same = (q == rq).float().mean().item()
    assert same >= 0.999, same
    d, rd = mr.dequantize(q, s), mr.dequantize(rq, rs)
    step = mr.e4m3_step(rq).float() * mr._POW2[rs.long()].float().repeat_interleave(32, 1)
    assert bool(((d - rd).abs() <= step).all())


def _operands(M, N, K, seed, integer=False):
    g = torch.Generator().manual_seed(seed)
    if integer:
        # small integers times a power of two per 32-element block: exact after quantisation, exact sums in fp32;
        # W[n][k] != W[k][n] (asymmetric), per-block scales differ along both rows and K
        A = torch.randint(-8, 9, (M, K), generator=g).float()
        W = torch.randint(-8, 9, (N, K), generator=g).float()
        A = A * torch.exp2(torch.randint(-3, 3, (M, K // 32), generator=g).float()).repeat_interleave(32, 1)
        W = W * torch.exp2(torch.randint(-3, 3, (N, K // 32), generator=g).float()).repeat_interleave(32, 1)
        b = torch.randint(-4, 5, (N,), generator=g).float()
    else:
        A = torch.randn(M, K, generator=g) * (1 + torch.rand(M, 1, generator=g) * 4)
        W = torch.randn(N, K, generator=g) / math.sqrt(K)
        b = torch.randn(N, generator=g) * 0.1
    Aq, As = _quant_gpu(A)
    Wq, Ws = _quant_gpu(W)
    return (Aq, As), (Wq, Ws), b


def _run_gemm(a, w, b, M, N, K, act, R, rr, mxout):
    dev = lambda t: None if t is None else t.to(DEV)
    if mxout:
        Cq = torch.full((M, N), 0xFF, device=DEV, dtype=U8)
        Cs = torch.full((M, N // 32), 0xFF, device=DEV, dtype=U8)
        _call("isic_gemm_mxfp8", dev(a[0]), dev(a[1]), dev(w[0]), dev(w[1]), dev(b), dev(R), None, Cq, Cs, M, N, K, act, rr)
        return Cq.cpu(), Cs.cpu()
    C = torch.full((M, N), float("nan"), device=DEV, dtype=F16)
    _call("isic_gemm_mxfp8", dev(a[0]), dev(a[1]), dev(w[0]), dev(w[1]), dev(b), dev(R), C, None, None, M, N, K, act, rr)
    return C.cpu()


def _reference(a, w, b, M, act, R, rr):
    ref = mr.dequantize(*a) @ mr.dequantize(*w).t() + b
    if act:
        ref = torch.nn.functional.gelu(ref)
    if R is not None:
        ref = ref + (R.float() if rr == 0 else R.float()[torch.arange(M) % rr])
    return ref


@pytest.mark.parametrize("M,N,K", [(127, 1152, 384), (300, 384, 1536), (1, 128, 128)])
def test_gemm_mxfp8_integer_operands_are_exact(M, N, K):
    """pins the A / B / scale lane maps of the scaled MFMA: any wrong k, row, column or scale pairing changes a sum"""
    a, w, b = _operands(M, N, K, M + N + K, integer=True)
    got = _run_gemm(a, w, b, M, N, K, 0, None, 0, False)
    ref = _reference(a, w, b, M, 0, None, 0)
    # ref is exact in fp32 (at most 23 significant bits); the kernel's only rounding is the final one to fp16
    assert bool((ref.abs() < 60000).all())
    assert torch.equal(got, ref.to(F16)), int((got != ref.to(F16)).sum())


_CASES = [(M, N, K, 0, None) for M in (1, 127, 588) for (N, K) in ((1152, 384), (384, 384), (1536, 384), (384, 1536))]
_CASES += [(588, 1536, 384, 1, None), (127, 384, 384, 0, "full"), (588, 384, 1536, 0, "full"), (588, 384, 384, 0, "pos"),
           (127, 1536, 384, 1, "full"), (50000, 1152, 384, 0, None), (50000, 384, 1536, 0, "full")]


@pytest.mark.parametrize("M,N,K,act,res", _CASES)
def test_gemm_mxfp8_fp16_out_matches_fp32_matmul(M, N, K, act, res):
    a, w, b = _operands(M, N, K, 3 * M + N + K)
    g = torch.Generator().manual_seed(M)
    rr, R = 0, None
    if res == "full":
        R = torch.randn(M, N, generator=g).to(F16)
    elif res == "pos":
        rr, R = 196, torch.randn(196, N, generator=g).to(F16)
    got = _run_gemm(a, w, b, M, N, K, act, R, rr, False).float()
    ref = _reference(a, w, b, M, act, R, rr)
    assert bool(torch.isfinite(got).all())
    tol = 2.0 ** -10 * ref.abs() + 1e-3 * ref.pow(2).mean().sqrt()
    err = (got - ref).abs()
    assert bool((err <= tol).all()), float((err - tol).max())


@pytest.mark.parametrize("M,N,K,act", [(588, 1536, 384, 1), (127, 384, 1536, 0), (50000, 1536, 384, 1)])
def test_gemm_mxfp8_mx_out_matches_quantised_fp32_matmul(M, N, K, act):
    a, w, b = _operands(M, N, K, 5 * M + N)
    q, s = _run_gemm(a, w, b, M, N, K, act, None, 0, True)
    ref = _reference(a, w, b, M, act, None, 0)
    rq, rs = mr.quantize(ref)
    # a block's scale moves only if summation order carries its amax across 448 * 2^e: a few in a million blocks
    assert (s != rs).float().mean().item() <= 1e-5
    assert (q == rq).float().mean().item() >= 0.998
    # every other byte within one e4m3 step of the reference's, plus the summation-order allowance of the fp16-out test
    # (1e-3 rms): the small elements of a block have steps far below it (seen on GELU outputs near 0)
    step = mr.e4m3_step(rq).float() * mr._POW2[rs.long()].float().repeat_interleave(32, 1)
    step = step + 1e-3 * ref.pow(2).mean().sqrt()
    ok = ((mr.dequantize(q, s) - mr.dequantize(rq, rs)).abs() <= step) | (s != rs).repeat_interleave(32, 1)
    assert bool(ok.all())


def test_gemm_mxfp8_rejects_unsupported_shapes():
    from isic_hip.lib import IsicHipError
    A = torch.zeros(8, 192, device=DEV, dtype=U8)
    W = torch.zeros(256, 192, device=DEV, dtype=U8)
    S = torch.zeros(256, 6, device=DEV, dtype=U8)
    C = torch.zeros(8, 256, device=DEV, dtype=F16)
    with pytest.raises(IsicHipError) as e:
        _call("isic_gemm_mxfp8", A, S[:8], W, S, None, None, C, None, None, 8, 256, 192, 0, 0)      # K % 128
    assert e.value.code == -2
    with pytest.raises(IsicHipError) as e:
        _call("isic_gemm_mxfp8", A, S[:8], W, S, None, None, C, C, S, 8, 256, 256, 0, 0)            # both outputs
    assert e.value.code == -1


# ---------------------------------------------------------------- the encoder
def _encoders(img=224, depth=12):
    from isic_hip.vit import ViTSmallEncoder
    from oracle import vit as ov
    p = ov.init_params(5, img=img, depth=depth)
    enc = ViTSmallEncoder(img_size=img, depth=depth, precision="mxfp8").to(DEV)
    enc.load_state_dict(p)
    return enc, p, ov


def _relf(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_encoder_mxfp8_tokens_match_emulation_and_fp32():
    enc, p, ov = _encoders()
    x = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(11))
    got = enc.run_tokens(x.to(DEV)).cpu()
    assert got.shape == (3, 196, 384) and bool(torch.isfinite(got).all())
    emu = mr.forward_tokens_mxfp8(p, x)
    assert _relf(got, emu) <= 0.1, _relf(got, emu)
    ref32 = ov.forward_tokens(p, x)
    assert _relf(got, ref32) <= 0.15, _relf(got, ref32)
    cos = torch.nn.functional.cosine_similarity(got.double(), ref32.double(), dim=-1)
    assert float(cos.min()) >= 0.99, float(cos.min())
    one = enc.run_tokens(x.to(DEV), depth=1).cpu()
    assert _relf(one, mr.forward_tokens_mxfp8(p, x, depth=1)) <= 2e-2, _relf(one, mr.forward_tokens_mxfp8(p, x, depth=1))


def test_encoder_mxfp8_weights_follow_load_state_dict():
    enc, p, ov = _encoders(img=32, depth=2)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(4)).to(DEV)
    a = enc.run_tokens(x)
    p2 = ov.init_params(6, img=32, depth=2)
    enc.load_state_dict(p2)
    b = enc.run_tokens(x).cpu()
    assert not torch.equal(a.cpu(), b)
    assert _relf(b, mr.forward_tokens_mxfp8(p2, x.cpu())) <= 3e-2      # stale weights would be off by O(1)


def test_encoder_mxfp8_is_deterministic_and_batch_invariant():
    enc, _, _ = _encoders()
    x = torch.randn(5, 3, 224, 224, generator=torch.Generator().manual_seed(2)).to(DEV)
    a = enc.run_tokens(x)
    assert torch.equal(a, enc.run_tokens(x))
    assert torch.equal(a[1:3], enc.run_tokens(x[1:3]))


def test_extract_latents_with_the_mxfp8_vit_encoder():
    import save_latent as sl
    tv, te = sl.SyntheticDermImages(n=5, seed=1), sl.SyntheticDermImages(n=3, seed=2)
    out = {}
    for prec in ("fp16", "mxfp8"):
        cfg = {"device": DEV, "seed": 42, "pca": False, "encoder": "vit_s16", "encoder_precision": prec}
        out[prec] = sl.extract_latents(cfg, "missing.pth", datasets=(tv, te), batch_size=4)
    for a, b in zip(out["fp16"], out["mxfp8"]):
        assert list(a.columns) == list(b.columns) and len(a) == len(b)
    raw16, rawmx = out["fp16"][4], out["mxfp8"][4]
    assert (raw16[["image_path", "target"]].values == rawmx[["image_path", "target"]].values).all()
    assert rawmx["latent"].iloc[0].shape == (196, 384)
    l16 = torch.from_numpy(np.stack(list(raw16["latent"]))).double()
    lmx = torch.from_numpy(np.stack(list(rawmx["latent"]))).double()
    cos = torch.nn.functional.cosine_similarity(lmx, l16, dim=-1)
    assert float(cos.min()) >= 0.99, float(cos.min())
    assert _relf(lmx, l16) <= 0.15, _relf(lmx, l16)
