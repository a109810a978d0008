"""The fp16 transformer / MAE kernels over their documented domains on the MI355X, through the C ABI, against fp64
references with per-element bounds (tests/f16_kernel_ref.py; tests/test_f16_kernel_ref_cpu.py shows on the CPU that the
attention bounds admit a correct kernel and reject six wrong ones).

A  attention forward / backward, head widths 64 and 32: five input families x every tile-boundary token count x three
   (images, heads) shapes; NaN pre-filled outputs with guard rows, bit-reproducible backward, batch invariance.
B  isic_gemm_f16 at the MAE decoder's width 512 and the other production shapes no kernel test ran, the dGELU and
   GELU-with-pre-activation epilogues at four plans, the weight gradient at every (N, K) of the three encoders.
C  LayerNorm-add forward / backward at every supported width, past the 512-block cap, on constant rows (variance 0) and
   on rows with a large common offset.
D  non-square and small geometry: masked depthwise 5x5 (forward, data and weight gradient), the reconstruction loss,
   depth-to-space, the depthwise weight gradient at H = 1 / W = 1.
E  row movement with indices outside their range, L == T, L == 1, C == 8.
F  isic_colsum_f16 on its own.

Every case runs once.  Each attention case prints its worst error / bound ratio per output; the module prints the worst
per entry point and family at the end (visible with -s)."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f16_kernel_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16
NAN = float("nan")
GUARD = 3                                           # NaN rows before and after every guarded output


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16), device=DEV, dtype=torch.uint8)


def _guarded(rows, cols, dtype=F16):
    """(buffer, view of the `rows` rows in its middle): the buffer is NaN everywhere"""
    buf = torch.full((rows + 2 * GUARD, cols), NAN, device=DEV, dtype=dtype)
    return buf, buf[GUARD:GUARD + rows]


def _guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def _bits(t):
    return t.contiguous().view(torch.int16)


# ================================================================== A. attention
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        print("worst device ratio", key, {k: round(v, 3) for k, v in WORST[key].items()})


def _attn_calls(hd):
    if hd == 64:
        return (lambda q, o, n, T, H: _call("isic_attention_f16", q, o, n, T, H, 64),
                lambda q, o, do, dq, n, T, H: _call("isic_attention_bwd_f16", q, o, do, dq, n, T, H, 64))
    return (lambda q, o, n, T, H: _call("isic_attention_d32_f16", q, o, n, T, H),
            lambda q, o, do, dq, n, T, H: _call("isic_attention_d32_bwd_f16", q, o, do, dq, n, T, H))


ATT_SHAPES = R.ATT_SHAPES


@pytest.mark.parametrize("hd,n,H", ATT_SHAPES, ids=[f"d{hd}-n{n}-h{H}" for hd, n, H in ATT_SHAPES])
@pytest.mark.parametrize("T", R.T_LIST)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_attention_forward_and_backward_within_the_derived_bounds(family, T, hd, n, H):
    D, M = H * hd, n * T
    qkv_c, dout_c = R.attention_inputs(family, n, T, H, hd)
    ref = R.attention_ref(qkv_c, dout_c, n, T, H, hd)
    bounds = R.attention_bounds(ref)
    fwd, bwd = _attn_calls(hd)
    qkv, dout = qkv_c.to(DEV), dout_c.to(DEV)
    obuf, out = _guarded(M, D)
    fwd(qkv, out, n, T, H)
    gbuf, dqkv = _guarded(M, 3 * D)
    bwd(qkv, out, dout, dqkv, n, T, H)                     # the kernel's own forward output, as in training
    torch.cuda.synchronize()
    assert _guards_intact(obuf) and _guards_intact(gbuf)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dqkv).all())
    g = dqkv.cpu()
    got = dict(out=R.heads_of(out.cpu(), n, T, H, hd), dq=R.heads_of(g[:, :D], n, T, H, hd),
               dk=R.heads_of(g[:, D:2 * D], n, T, H, hd), dv=R.heads_of(g[:, 2 * D:], n, T, H, hd))
    ratios = R.attention_ratios(got, ref, bounds)
    print(f"{family} T={T} d{hd} n={n} heads={H}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    w = WORST.setdefault((f"d{hd}", family), {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), v)
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # bit-reproducible
    again = torch.full_like(dqkv, NAN)
    bwd(qkv, out, dout, again, n, T, H)
    assert torch.equal(_bits(dqkv), _bits(again))
    out2 = torch.full_like(out, NAN)
    fwd(qkv, out2, n, T, H)
    assert torch.equal(_bits(out), _bits(out2))
    if family == "const_v":                                # the exact answer is v0 whatever P is
        v0 = ref["v"]
        assert bool(((got["out"].double() - v0).abs() <= 2.0 ** -10 * v0.abs()).all())
    if T == 1:                                             # one key: P == 1 exactly
        assert torch.equal(_bits(out), _bits(qkv[:, 2 * D:]))
        assert torch.equal(_bits(dqkv[:, 2 * D:]), _bits(dout))
        assert bool((dqkv[:, :2 * D] == 0).all())
    if n > 1:                                              # a sub-batch: the same bits, the other images' rows untouched
        m1 = (n - 1) * T
        sub_o = torch.full((M, D), NAN, device=DEV, dtype=F16)
        sub_g = torch.full((M, 3 * D), NAN, device=DEV, dtype=F16)
        fwd(qkv, sub_o, n - 1, T, H)
        bwd(qkv, out, dout, sub_g, n - 1, T, H)
        assert torch.equal(_bits(sub_o[:m1]), _bits(out[:m1])) and bool(torch.isnan(sub_o[m1:]).all())
        assert torch.equal(_bits(sub_g[:m1]), _bits(dqkv[:m1])) and bool(torch.isnan(sub_g[m1:]).all())


# ================================================================== B. GEMM modes and the weight gradient
def _gemm_inputs(M, N, K, seed=0):
    g = torch.Generator(device=DEV).manual_seed(M + N + K + seed)
    A = torch.randn(M, K, device=DEV, generator=g).to(F16)
    W = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(F16)
    b = torch.randn(N, device=DEV, generator=g) * 0.1
    return g, A, W, b


def _gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


GEMM_SHAPES = [                                            # (N, K, act, residual, layer)
    (512, 768, 0, None, "decoder_embed"),
    (1536, 512, 0, None, "decoder qkv"),
    (512, 512, 0, "full", "decoder proj + residual"),
    (2048, 512, 1, None, "decoder fc1 + GELU"),
    (512, 2048, 0, "full", "decoder fc2 + residual"),
    (768, 512, 0, None, "decoder_pred"),
    (768, 2304, 0, None, "blocks3 qkv data gradient"),
    (512, 1536, 0, None, "decoder qkv data gradient"),
    (768, 3072, 0, "full", "blocks3 fc2 + residual"),
]


@pytest.mark.parametrize("M", [98, 392, 12544])
@pytest.mark.parametrize("N,K,act,res,layer", GEMM_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in GEMM_SHAPES])
def test_gemm_f16_at_the_decoder_and_data_gradient_shapes(M, N, K, act, res, layer):
    g, A, W, b = _gemm_inputs(M, N, K)
    Rs = None if res is None else torch.randn(M, N, device=DEV, generator=g).to(F16)
    cbuf, C = _guarded(M, N)
    _call("isic_gemm_f16", A, W, b, Rs, C, M, N, K, act, 0)
    ref = A.double() @ W.double().t() + b.double()
    if act:
        ref = _gelu64(ref)
    if Rs is not None:
        ref = ref + Rs.double()
    assert _guards_intact(cbuf) and bool(torch.isfinite(C).all())
    err, tol = (C.double() - ref).abs(), R.gemm_bound(ref)
    assert bool((err <= tol).all()), (layer, float((err / tol).max()))


EPI_SHAPES = [(3072, 768), (1024, 256), (2048, 512), (1536, 384)]


@pytest.mark.parametrize("M", [1, 5, 2100, 12544])
@pytest.mark.parametrize("N,K", EPI_SHAPES)
def test_dgelu_and_gelu_pre_epilogues_at_the_backward_plans(M, N, K):
    g, A, W, b = _gemm_inputs(M, N, K, seed=1)
    aux = (torch.randn(M, N, device=DEV, generator=g) * 2).to(F16)
    flat = aux.view(-1)
    flat[0::7], flat[1::7], flat[2::7] = 8.0, -8.0, 0.0   # derivative 1, 0 and 0.5
    cbuf, C = _guarded(M, N)
    _call("isic_gemm_f16_dgelu", A, W, aux, C, M, N, K)
    a = aux.double()
    gp = 0.5 * (1 + torch.erf(a / math.sqrt(2))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)
    assert float((gp.view(-1)[0::7] - 1).abs().max()) < 1e-12 and float(gp.view(-1)[1::7].abs().max()) < 1e-12
    prod = A.double() @ W.double().t()
    ref = prod * gp
    assert _guards_intact(cbuf) and bool(torch.isfinite(C).all())
    err, tol = (C.double() - ref).abs(), R.gemm_bound(ref)
    assert bool((err <= tol).all()), float((err / tol).max())
    # GELU with the pre-activation: C bit-equal to isic_gemm_f16's, pre = the rounded A . W^T + bias
    hbuf, hid = _guarded(M, N)
    pbuf, pre = _guarded(M, N)
    hid0 = torch.full((M, N), NAN, device=DEV, dtype=F16)
    _call("isic_gemm_f16_gelu_pre", A, W, b, hid, pre, M, N, K)
    _call("isic_gemm_f16", A, W, b, None, hid0, M, N, K, 1, 0)
    assert _guards_intact(hbuf) and _guards_intact(pbuf)
    assert torch.equal(_bits(hid), _bits(hid0))
    ref = prod + b.double()
    assert bool(((pre.double() - ref).abs() <= R.gemm_bound(ref)).all())
    refh = _gelu64(ref)
    assert bool(((hid.double() - refh).abs() <= R.gemm_bound(refh)).all())


WGRAD_SHAPES = [                                           # (N, K, the layers whose weight gradient has this shape)
    (1152, 384, "ViT-S qkv"), (384, 384, "ViT-S proj, CBlock(384) conv1 / conv2"),
    (1536, 384, "ViT-S fc1, CBlock(384) fc1"), (384, 1536, "ViT-S fc2, CBlock(384) fc2"), (384, 768, "ViT-S patch_embed"),
    (2304, 768, "blocks3 qkv"), (768, 768, "blocks3 proj, patch_embed4"), (3072, 768, "blocks3 fc1"),
    (768, 3072, "blocks3 fc2"), (1536, 512, "decoder qkv"), (512, 512, "decoder proj"), (2048, 512, "decoder fc1"),
    (512, 2048, "decoder fc2"), (768, 512, "decoder_pred"), (512, 768, "decoder_embed"),
    (256, 256, "CBlock(256) conv1 / conv2"), (1024, 256, "CBlock(256) fc1"), (256, 1024, "CBlock(256) fc2"),
    (768, 1536, "stage2_output_decode, patch_embed3"), (768, 4096, "stage1_output_decode"),
    (384, 1024, "patch_embed2"), (256, 128, "patch_embed1 (48 padded to 128)"),
]


@pytest.mark.parametrize("M", [0, 1, 127, 128, 129, 4097])
@pytest.mark.parametrize("N,K,layer", WGRAD_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in WGRAD_SHAPES])
def test_wgrad_at_every_shape_the_encoders_use(M, N, K, layer):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    dY = torch.randn(M, N, device=DEV, generator=g).to(F16)
    X = torch.randn(M, K, device=DEV, generator=g).to(F16)
    s = 0.25
    ws = _ws(_call("isic_gemm_f16_wgrad_workspace_bytes", M, N, K))
    base = torch.randn(N, K, device=DEV, generator=g)
    baseb = torch.randn(N, device=DEV, generator=g)
    ref = s * (dY.double().t() @ X.double())
    bound = R.wgrad_bound(dY, X, s)
    refb, boundb = s * dY.double().sum(0), 1e-4 * s * dY.double().abs().sum(0) + 1e-6
    for with_db in (True, False):
        wbuf, dW = _guarded(N, K, torch.float32)
        db = torch.full((N,), NAN, device=DEV) if with_db else None
        _call("isic_gemm_f16_wgrad", dY if M else None, X if M else None, dW, db, M, N, K, s, 0, ws, ws.numel())
        assert _guards_intact(wbuf), layer
        if M == 0:                                         # an empty sum
            assert bool((dW == 0).all()) and (db is None or bool((db == 0).all()))
        else:
            assert bool(((dW.double() - ref).abs() <= bound).all()), (layer, float(((dW.double() - ref).abs() / bound).max()))
            if with_db:
                assert bool(((db.double() - refb).abs() <= boundb).all()), layer
                first = dW.clone()
            else:
                assert torch.equal(dW, first)              # the bias reduction does not change dW; bit-reproducible
        acc, accb = base.clone(), (baseb.clone() if with_db else None)
        _call("isic_gemm_f16_wgrad", dY if M else None, X if M else None, acc, accb, M, N, K, s, 1, ws, ws.numel())
        if M == 0:                                         # nothing to add: the buffers keep their bits
            assert torch.equal(acc, base) and (accb is None or torch.equal(accb, baseb))
        else:
            assert bool(((acc.double() - base.double() - ref).abs() <= bound + 1e-6 * base.double().abs()).all()), layer
            if with_db:
                assert bool(((accb.double() - baseb.double() - refb).abs() <= boundb + 1e-6 * baseb.double().abs()).all())


# ================================================================== C. LayerNorm-add
def _ln_rows(kind, M, N, g):
    """x, a, b (fp16, CPU).  "gauss": the existing tests' rows; "const": every third row constant (v the same exactly
    summable value in every channel: variance exactly 0); "offset": mean 50, standard deviation 0.5 (a = b = 0 there)"""
    if kind == "offset":
        x = (50.0 + 0.5 * torch.randn(M, N, generator=g)).half()
        return x, torch.zeros_like(x), torch.zeros_like(x)
    x, a, b = ((torch.randn(M, N, generator=g) * 2 + 0.5).half() for _ in range(3))
    if kind == "const":
        for t, val in ((x, 2.0), (a, -1.0), (b, 1.0)):              # v = 2: N v / N is exact for every N
            t[::3] = val
    return x, a, b


def _ln_forward_case(M, N, addends, act, eps, kind="gauss"):
    g = torch.Generator().manual_seed(M + N + addends + act)
    x, a, b = _ln_rows(kind, M, N, g)
    xs = [x, a, b][:1 + addends]
    gm, bt = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.2
    d = [t.to(DEV) for t in xs] + [None, None]
    ybuf, y = _guarded(M, N)
    y32buf, y32 = _guarded(M, N, torch.float32)
    _call("isic_layernorm_add_f16", d[0], d[1], d[2], gm.to(DEV), bt.to(DEV), y, y32, M, N, act, eps)
    ref = R.layernorm_add_ref(d[:1 + addends], gm.to(DEV), bt.to(DEV), eps, act)
    assert _guards_intact(ybuf) and _guards_intact(y32buf)
    assert bool(torch.isfinite(y32).all()) and bool(torch.isfinite(y).all())
    ok32, ok16 = R.layernorm_add_fwd_errors(y32, y, ref)
    assert ok32, float((y32.double() - ref).abs().max() / ref.abs().max())
    assert ok16
    if kind == "const" and not act:                        # x^ == 0 exactly: the row is beta
        assert torch.equal(y32[::3], bt.to(DEV).expand(y32[::3].shape))


LN_WIDTHS = list(range(64, 1025, 64))


@pytest.mark.parametrize("M", [1, 3, 300])
@pytest.mark.parametrize("N", LN_WIDTHS)
def test_layernorm_add_forward_at_every_width(M, N):
    _ln_forward_case(M, N, 2, 0, 1e-5)
    _ln_forward_case(M, N, 0, 1, 1e-6)


@pytest.mark.parametrize("M", [32768, 32769, 50176])
@pytest.mark.parametrize("N", [256, 512, 768])
def test_layernorm_add_forward_at_production_row_counts(M, N):
    _ln_forward_case(M, N, 1, 0, 1e-6)


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("N", [64, 512, 768])
def test_layernorm_add_forward_on_constant_and_offset_rows(N, eps):
    """N = 768 at eps 1e-6 is the case that found a kernel bug: the mean was s * (1 / N), the compiler fused the
    subtraction "v - s * (1 / N)" into one FMA with the product unrounded, and with 1 / 768 inexact a constant row of 2.0
    came out as -2^-24 instead of 0 -- times rstd = 1000 an x^ of 6e-5 (1.5e-5 of the output's scale against the 2e-6
    allowed).  The kernel and its backward now divide: N c / N is exact."""
    _ln_forward_case(300, N, 2, 0, eps, kind="const")
    _ln_forward_case(300, N, 0, 0, eps, kind="offset")


def _ln_backward_case(M, N, addends, dy_f32, act, mode, eps=1e-6, mul=4.0, kind="gauss"):
    """modes as in test_layernorm_add_bwd_matches_fp32_autograd; the reference is fp64 autograd on the device, all rows"""
    s = 0.5
    g = torch.Generator().manual_seed(N + 10 * addends + act + M)
    x, a, b = (t.to(DEV) for t in _ln_rows(kind, M, N, g))
    gamma, beta = (1 + 0.1 * torch.randn(N, generator=g)).to(DEV), (0.1 * torch.randn(N, generator=g)).to(DEV)
    dy = torch.randn(M, N, generator=g).to(DEV)
    dy = dy if dy_f32 else dy.half()
    g_in = torch.randn(M, N, generator=g).to(DEV) if mode == "alias" else torch.zeros(M, N, device=DEV)
    xs = [x, a, b] if addends else [x]
    dv, dgm, dbt = R.layernorm_add_bwd_ref(dy, mul, xs, gamma, beta, act, eps)
    ws = _ws(_call("isic_layernorm_add_bwd_f16_workspace_bytes", M, N))
    obuf, g_out = _guarded(M, N, torch.float32)
    if mode == "alias":
        g_out.copy_(g_in)
    hbuf, g16 = _guarded(M, N)
    acc = 1 if mode == "alias" else 0
    dg, db_ = (torch.full((N,), 1.0 if acc else NAN, device=DEV) for _ in range(2))
    _call("isic_layernorm_add_bwd_f16", dy, dy_f32, mul, x, a if addends else None, b if addends else None, gamma, beta, act,
          eps, g_out if mode == "alias" else None, None if mode == "f16_only" else g_out, g16, dg, db_, M, N, s, acc, ws,
          ws.numel())
    ref = g_in.double() + dv
    assert _guards_intact(hbuf) and _guards_intact(obuf)
    if mode != "f16_only":
        assert float((g_out.double() - ref).abs().max()) <= R.layernorm_add_bwd_gout_tol(ref, dv, False)
        assert torch.equal(_bits(g16), _bits(g_out.to(F16)))
    else:
        assert bool(torch.isnan(g_out).all())              # not asked for: not written
        assert float((g16.double() - ref).abs().max()) <= R.layernorm_add_bwd_gout_tol(ref, dv, True)
    for got, want in ((dg, acc + s * dgm), (db_, acc + s * dbt)):
        assert float((got.double() - want).abs().max()) <= R.layernorm_add_bwd_param_tol(want, s, M)
    if mode == "fresh":                                    # bit-reproducible
        g2, dg2, db2 = torch.empty_like(g_out), torch.empty_like(dg), torch.empty_like(db_)
        _call("isic_layernorm_add_bwd_f16", dy, dy_f32, mul, x, a if addends else None, b if addends else None, gamma, beta,
              act, eps, None, g2, None, dg2, db2, M, N, s, 0, ws, ws.numel())
        assert torch.equal(g2, g_out) and torch.equal(dg2, dg) and torch.equal(db2, db_)


@pytest.mark.parametrize("M", [1, 3, 300])
@pytest.mark.parametrize("N", LN_WIDTHS)
def test_layernorm_add_backward_at_every_width(M, N):
    _ln_backward_case(M, N, 2, 0, 0, "fresh")


@pytest.mark.parametrize("M", [32768, 32769, 50176])
@pytest.mark.parametrize("N", [256, 512, 768])
def test_layernorm_add_backward_past_the_row_split_cap(M, N):
    """the parameter-gradient reduction caps at 512 blocks: from 32 769 rows on a block's chunk exceeds 64 rows and is no
    longer a multiple of the 4-wave stride"""
    _ln_backward_case(M, N, 2, 1, 0, "alias")


@pytest.mark.parametrize("N", [512, 64])
@pytest.mark.parametrize("addends,dy_f32,act", [(0, 0, 0), (2, 1, 0), (0, 1, 1), (2, 0, 1)])
@pytest.mark.parametrize("mode", ["alias", "fresh", "f16_only"])
def test_layernorm_add_backward_modes_at_the_decoder_width_and_the_smallest(N, addends, dy_f32, act, mode):
    _ln_backward_case(300, N, addends, dy_f32, act, mode)


@pytest.mark.parametrize("eps", [1e-6, 1e-5])
@pytest.mark.parametrize("N", [64, 512, 768])
def test_layernorm_add_backward_on_constant_and_offset_rows(N, eps):
    """a constant row has variance exactly 0: rstd = 1 / sqrt(eps), x^ = 0, g = rstd (g^ - mean(g^))"""
    _ln_backward_case(300, N, 2, 1, 0, "fresh", eps=eps, mul=1.0, kind="const")
    _ln_backward_case(300, N, 0, 0, 0, "fresh", eps=eps, mul=1.0, kind="offset")


# ================================================================== D. non-square and small geometry
def _keep(kind, N, T, g):
    if kind == "random":
        return (torch.rand(N, T, generator=g) > 0.6).to(torch.uint8)
    return torch.full((N, T), 1 if kind == "ones" else 0, dtype=torch.uint8)


def _dw_ref(x, dy):
    """fp64 depthwise 5x5 weight gradient [25][C] of NHWC x, dy, and the sum of |terms| for the bound"""
    H, W = x.shape[1], x.shape[2]
    xp = F.pad(x.double().permute(0, 3, 1, 2), (2, 2, 2, 2))
    dyc = dy.double().permute(0, 3, 1, 2)
    ref = torch.stack([(dyc * xp[:, :, kh:kh + H, kw:kw + W]).sum((0, 2, 3)) for kh in range(5) for kw in range(5)])
    mag = torch.stack([(dyc.abs() * xp[:, :, kh:kh + H, kw:kw + W].abs()).sum((0, 2, 3)) for kh in range(5) for kw in range(5)])
    return ref, mag, dyc


@pytest.mark.parametrize("keep_kind", ["random", "ones", "zeros"])
@pytest.mark.parametrize("H,W,P,C", [(56, 28, 4, 256), (28, 56, 2, 384), (8, 12, 4, 64), (12, 8, 2, 64)])
def test_masked_dwconv_on_non_square_images(H, W, P, C, keep_kind):
    N, gh, gw = 2, H // P, W // P
    g = torch.Generator().manual_seed(H + 3 * W + C)
    x = torch.randn(N, H, W, C, generator=g).to(F16)
    wt = torch.randn(C, 1, 5, 5, generator=g) / 5
    b = 0.1 * torch.randn(C, generator=g)
    keep = _keep(keep_kind, N, gh * gw, g)
    km = keep.view(N, gh, gw).repeat_interleave(P, 1).repeat_interleave(P, 2)[..., None].to(F16)      # token (h/P)*(W/P) + w/P
    taps = wt.reshape(C, 25).t().contiguous()
    ybuf, y = _guarded(N * H * W, C)
    mbuf, xm = _guarded(N * H * W, C)
    _call("isic_dwconv5x5_masked_f16", x.to(DEV), keep.to(DEV), P, taps.to(DEV), b.to(DEV), xm, y, N, H, W, C)
    assert _guards_intact(ybuf) and _guards_intact(mbuf)
    assert torch.equal(xm.cpu().view(N, H, W, C), x * km)
    ref = F.conv2d((x * km).double().permute(0, 3, 1, 2), wt.double(), b.double(), padding=2, groups=C).permute(0, 2, 3, 1)
    got = y.double().cpu().view(N, H, W, C)
    assert bool(torch.isfinite(got).all())
    assert float((got - ref).abs().max()) <= 2e-3 * float(ref.abs().max())
    # data gradient
    dy = torch.randn(N, H, W, C, generator=g).to(F16)
    dbuf, dx = _guarded(N * H * W, C)
    _call("isic_dwconv5x5_masked_dgrad_f16", dy.to(DEV), keep.to(DEV), P, taps.flip(0).contiguous().to(DEV), dx, N, H, W, C)
    xr = (x * km).double().permute(0, 3, 1, 2).requires_grad_(True)
    F.conv2d(xr, wt.double(), None, padding=2, groups=C).backward(dy.double().permute(0, 3, 1, 2))
    refd = xr.grad.permute(0, 2, 3, 1) * km.double()
    gotd = dx.cpu().view(N, H, W, C)
    assert _guards_intact(dbuf)
    assert bool((gotd[km.expand_as(gotd) == 0] == 0).all())
    assert float((gotd.double() - refd).abs().max()) <= 2e-3 * float(refd.abs().max())
    # weight gradient of the masked input
    ws = _ws(_call("isic_dwconv5x5_wgrad_f16_workspace_bytes", N, H, W, C))
    dw, db = torch.full((25, C), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    _call("isic_dwconv5x5_wgrad_f16", xm, dy.to(DEV), dw, db, N, H, W, C, 1.0, 0, ws, ws.numel())
    refw, mag, dyc = _dw_ref(x * km, dy)
    assert bool(((dw.double().cpu() - refw).abs() <= 1e-4 * mag + 1e-6).all())
    assert bool(((db.double().cpu() - dyc.sum((0, 2, 3))).abs() <= 1e-4 * dyc.abs().sum((0, 2, 3)) + 1e-6).all())


@pytest.mark.parametrize("N,H,W,C", [(2, 1, 33, 128), (1, 5, 1, 64), (1, 3, 15, 64)])
def test_dwconv_wgrad_at_one_row_and_one_column(N, H, W, C):
    g = torch.Generator().manual_seed(N + H + W + C)
    x = torch.randn(N, H, W, C, generator=g).to(F16)
    dy = torch.randn(N, H, W, C, generator=g).to(F16)
    s = 0.25
    ws = _ws(_call("isic_dwconv5x5_wgrad_f16_workspace_bytes", N, H, W, C))
    wbuf, dw = _guarded(25, C, torch.float32)
    db = torch.full((C,), NAN, device=DEV)
    _call("isic_dwconv5x5_wgrad_f16", x.to(DEV), dy.to(DEV), dw, db, N, H, W, C, s, 0, ws, ws.numel())
    ref, mag, dyc = _dw_ref(x, dy)
    assert _guards_intact(wbuf)
    assert bool(((dw.double().cpu() - s * ref).abs() <= 1e-4 * s * mag + 1e-6).all())
    assert bool(((db.double().cpu() - s * dyc.sum((0, 2, 3))).abs() <= 1e-4 * s * dyc.abs().sum((0, 2, 3)) + 1e-6).all())
    dw2, db2 = torch.empty_like(dw), torch.empty_like(db)
    _call("isic_dwconv5x5_wgrad_f16", x.to(DEV), dy.to(DEV), dw2, db2, N, H, W, C, s, 0, ws, ws.numel())
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def _patchify(img, P):
    """[n][C][H][W] -> [n][T][P*P*C], token (h/P)*(W/P) + w/P, values in (row, column, channel) order"""
    n, C, H, W = img.shape
    return img.view(n, C, H // P, P, W // P, P).permute(0, 2, 4, 3, 5, 1).reshape(n, (H // P) * (W // P), P * P * C)


@pytest.mark.parametrize("loss_scale", [1.0, 2.0 ** 20])
@pytest.mark.parametrize("mask_kind", ["random", "single", "all"])
@pytest.mark.parametrize("norm_pix", [0, 1])
@pytest.mark.parametrize("C,H,W,P", [(3, 224, 112, 16), (3, 112, 224, 16), (4, 32, 64, 16), (3, 16, 24, 8), (1, 8, 4, 2)])
def test_reconstruction_loss_on_non_square_images(C, H, W, P, norm_pix, mask_kind, loss_scale):
    """pred = target + a perturbation small enough that loss_scale * 2 (pred - target) / (K mask_sum) stays inside fp16 (at
    mask_sum = 1, K = 4 and loss_scale = 2^20 that is |pred - target| < 0.12), so d pred is finite by construction."""
    n, T, K = 2, (H // P) * (W // P), P * P * C
    g = torch.Generator().manual_seed(C + H + 2 * W + P + norm_pix)
    img = torch.randn(n, C, H, W, generator=g)
    img[0, :, :P, -P:] = 0.5                               # image 0, last patch of the first patch row: constant (variance 0)
    if mask_kind == "random":
        mask = (torch.rand(n, T, generator=g) > 0.25).float()
        mask[0, 0] = 1.0
    elif mask_kind == "single":
        mask = torch.zeros(n, T)
        mask[n - 1, T - 1] = 1.0
    else:
        mask = torch.ones(n, T)
    msum = float(mask.sum())
    tgt = _patchify(img.double(), P)
    if norm_pix:
        tgt = (tgt - tgt.mean(-1, keepdim=True)) / (tgt.var(-1, keepdim=True) + 1e-6) ** 0.5
        assert bool((tgt[0, W // P - 1] == 0).all())      # the constant patch
    amp = min(1.0, 0.2 * 65504.0 * K * msum / (2.0 * loss_scale))
    pred = (tgt + amp * torch.randn(n, T, K, generator=g).clamp(-2, 2).double()).to(F16)
    mult = loss_scale * 2.0 / (K * msum)
    d_ref = mult * mask.double()[..., None] * (pred.double() - tgt)
    assert float(d_ref.abs().max()) < 65504.0
    l_ref = float((((pred.double() - tgt) ** 2).mean(-1) * mask.double()).sum() / msum)
    loss = torch.full((1,), NAN, device=DEV)
    dbuf, dpred = _guarded(n * T, K)
    ws = _ws(_call("isic_mae_loss_f16_workspace_bytes", n, H, W, P))
    args = (pred.to(DEV), img.to(DEV), mask.to(DEV), norm_pix, msum, loss_scale)
    _call("isic_mae_loss_f16", *args, dpred, loss, n, C, H, W, P, ws, ws.numel())
    assert _guards_intact(dbuf) and bool(torch.isfinite(dpred).all())
    # the fp32 target (normalised: three roundings) is off by a few ulps, t_err = 1e-6 (|target| + 1); that moves
    # (pred - target)^2 by 2 |pred - target| t_err, which counts when pred is close to the target; the fp32 sums get 1e-5
    t_err = 1e-6 * (tgt.abs() + 1)
    l_tol = 1e-5 * abs(l_ref) + float(((2 * (pred.double() - tgt).abs() * t_err).mean(-1) * mask.double()).sum() / msum)
    assert abs(float(loss) - l_ref) <= l_tol, (float(loss), l_ref, l_tol)
    # per element: one fp16 store, plus the target's error
    got = dpred.double().cpu().view(n, T, K)
    bound = (2.0 ** -11 * d_ref.abs()).clamp(min=2.0 ** -25) + mult * t_err
    assert bool(((got - d_ref).abs() <= bound).all()), float(((got - d_ref).abs() / bound).max())
    assert bool((got[mask == 0] == 0).all())
    loss2, dpred2 = torch.empty_like(loss), torch.empty_like(dpred)
    _call("isic_mae_loss_f16", *args, dpred2, loss2, n, C, H, W, P, ws, ws.numel())
    assert torch.equal(loss, loss2) and torch.equal(_bits(dpred), _bits(dpred2))


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("H,W", [(8, 12), (12, 8)])
def test_patch_rows_bwd_on_non_square_images(H, W, P):
    N, C = 3, 16
    x = torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(H + P)).to(F16)
    rows = x.view(N, H // P, P, W // P, P, C).permute(0, 1, 3, 2, 4, 5).reshape(N * (H // P) * (W // P), P * P * C).contiguous()
    xbuf, dx = _guarded(N * H * W, C, torch.float32)
    hbuf, dx16 = _guarded(N * H * W, C)
    _call("isic_patch_rows_bwd_f16", rows.to(DEV), dx, dx16, N, H, W, C, P, 0)
    assert _guards_intact(xbuf) and _guards_intact(hbuf)
    assert torch.equal(dx.cpu().view(N, H, W, C), x.float()) and torch.equal(dx16.cpu().view(N, H, W, C), x)
    base = torch.randn(N * H * W, C, device=DEV)
    acc = base.clone()
    _call("isic_patch_rows_bwd_f16", rows.to(DEV), acc, None, N, H, W, C, P, 1)
    assert torch.equal(acc.cpu().view(N, H, W, C), base.cpu().view(N, H, W, C) + x.float())
    fwd = torch.full((rows.shape[0], rows.shape[1]), NAN, device=DEV, dtype=F16)      # and the forward it is the adjoint of
    _call("isic_patch_rows_nhwc_f16", x.to(DEV), fwd, N, H, W, C, P)
    assert torch.equal(fwd.cpu(), rows)


# ================================================================== E. row movement edges
def _take(src, ids, limit):
    """src [n][R][C], ids [n][J] -> [n][J][C]: row ids[n][j] of image n, a zero row for an index outside [0, limit)"""
    ok = (ids >= 0) & (ids < limit)
    safe = torch.where(ok, ids, torch.zeros_like(ids))
    out = torch.gather(src, 1, safe[..., None].expand(-1, -1, src.shape[-1]))
    return torch.where(ok[..., None], out, torch.zeros_like(out))


@pytest.mark.parametrize("bad", [False, True], ids=["valid", "out_of_range"])
@pytest.mark.parametrize("T,L,C", [(1, 1, 8), (49, 1, 8), (49, 49, 64), (196, 49, 512), (196, 196, 8), (196, 13, 72)])
def test_row_movement_edges_bitwise(T, L, C, bad):
    n = 3
    g = torch.Generator().manual_seed(T + L + C)
    sh = torch.argsort(torch.rand(n, T, generator=g), dim=1)
    rest = torch.argsort(sh, dim=1)
    keep_ids = sh[:, :L].clone()
    if bad:                                                # -1, T and 2^40 among the valid ones
        for t, vals in ((keep_ids, (-1, T, 2 ** 40)), (rest, (-1, T, 2 ** 40)), (sh, (-1, T, 2 ** 40))):
            flat = t.view(-1)
            for i, v in enumerate(vals):
                flat[(i * 5) % flat.numel()] = v
    sh, rest, keep_ids = sh.contiguous(), rest.contiguous(), keep_ids.contiguous()
    x = torch.randn(n, T, C, generator=g).to(F16)
    ybuf, y = _guarded(n * L, C)
    _call("isic_gather_rows_f16", x.to(DEV), keep_ids.to(DEV), y, n, T, L, C)
    ref = _take(x, keep_ids, T)
    assert _guards_intact(ybuf) and torch.equal(_bits(y.cpu()), _bits(ref.view(n * L, C)))
    # scatter: a rank outside [0, L) is a zero row
    yy = torch.randn(n, L, C, generator=g).to(F16)
    xbuf, back = _guarded(n * T, C)
    _call("isic_scatter_rows_f16", yy.to(DEV), rest.to(DEV), back, n, T, L, C)
    assert _guards_intact(xbuf) and torch.equal(_bits(back.cpu()), _bits(_take(yy, rest, L).view(n * T, C)))
    # unshuffle: a rank outside [0, L) is the mask token
    mt, pos = torch.randn(C, generator=g), torch.randn(T, C, generator=g)
    obuf, out = _guarded(n * T, C)
    _call("isic_mae_unshuffle_f16", yy.to(DEV), rest.to(DEV), mt.to(DEV), pos.to(DEV), out, n, T, L, C)
    inr = ((rest >= 0) & (rest < L))[..., None]
    refu = (torch.where(inr, _take(yy, rest, L).float(), mt.expand(n, T, C)) + pos).to(F16)
    assert _guards_intact(obuf) and torch.equal(_bits(out.cpu()), _bits(refu.view(n * T, C)))
    # its adjoint, split at L; d_removed may be NULL only when L == T
    dout = torch.randn(n, T, C, generator=g).to(F16)
    kbuf, dk = _guarded(n * L, C)
    rbuf, dr = _guarded(n * (T - L), C) if L < T else (None, None)
    _call("isic_mae_unshuffle_bwd_f16", dout.to(DEV), sh.to(DEV), dk, dr, n, T, L, C)
    moved = _take(dout, sh, T)
    assert _guards_intact(kbuf) and torch.equal(_bits(dk.cpu()), _bits(moved[:, :L].reshape(n * L, C)))
    if L < T:
        assert _guards_intact(rbuf) and torch.equal(_bits(dr.cpu()), _bits(moved[:, L:].reshape(n * (T - L), C)))


# ================================================================== F. column sums
@pytest.mark.parametrize("rows,cols", [(0, 64), (1, 8), (31, 72), (33, 72), (4096, 512), (4097, 512), (50176, 384),
                                       (256, 75264), (1048577, 8)])
def test_colsum_f16(rows, cols):
    g = torch.Generator(device=DEV).manual_seed(rows + cols)
    x = (torch.randn(rows, cols, device=DEV, generator=g) + 0.5).to(F16)
    s = 0.25
    ws = _ws(_call("isic_colsum_f16_workspace_bytes", rows, cols))
    obuf, out = _guarded(1, cols, torch.float32)
    _call("isic_colsum_f16", x if rows else None, out, rows, cols, s, 0, ws, ws.numel())
    ref, bound = s * x.double().sum(0), R.colsum_bound(x, s)
    assert _guards_intact(obuf)
    assert bool(((out[0].double() - ref).abs() <= bound).all()), float(((out[0].double() - ref).abs() / bound).max())
    if rows == 0:
        assert bool((out == 0).all())
    again = torch.full((cols,), NAN, device=DEV)
    _call("isic_colsum_f16", x if rows else None, again, rows, cols, s, 0, ws, ws.numel())
    assert torch.equal(again, out[0])
    base = torch.randn(cols, device=DEV, generator=g)
    acc = base.clone()
    _call("isic_colsum_f16", x if rows else None, acc, rows, cols, s, 1, ws, ws.numel())
    if rows == 0:
        assert torch.equal(acc, base)
    else:
        assert bool(((acc.double() - base.double() - ref).abs() <= bound + 1e-6 * base.double().abs()).all())
