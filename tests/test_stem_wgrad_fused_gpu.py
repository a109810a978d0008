"""The fused stem weight gradient (``isic_conv_stem_wgrad_bn_pooled_bf16``: max-pool backward -> BatchNorm(+ReLU)
backward formed in registers -> weight gradient) against the two-kernel path that materialises dY:
``isic_bn_relu_maxpool3x3s2_fwd_bf16`` -> ``isic_bn_bwd_reduce_pooled_bf16`` -> ``isic_bn_bwd_apply_pooled_bf16`` ->
``isic_conv_stem_wgrad_bf16``.

Bounds (those of ``test_encoder_gpu.py::test_stem_wgrad_from_pooled_gradient``): dgamma / dbeta equal exactly; dw within
rtol 1e-4, atol 1e-4 * max|dw_ref| (identical bf16 operands and tiles, fp32 accumulation); two calls of the fused entry
on the same inputs are bit-equal.

Shapes (N, H, W of the input image; the stem output is about half, the pooled map a quarter):
  (1, 14, 14)   one partial tile, Ho = Wo = 7
  (1, 30, 46)   Ho = 15, Wo = 23: odd output sizes, pooling windows clipped at bottom and right, ragged tiles
  (2, 31, 45)   odd input height and width: a 16-byte staging piece would straddle the right border (register-staged patch)
  (32, 96, 96)  576 tiles > the 512 persistent blocks: second grid-stride round, tile cursor crossing image boundaries
  (5, 64, 64)   fewer tiles than blocks
Operand cases: "random" on every shape; "peaks", "ties", "dead" on (1, 30, 46) and (32, 96, 96)."""
import functools

import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
C = 64

SHAPES = [(1, 14, 14), (1, 30, 46), (2, 31, 45), (32, 96, 96), (5, 64, 64)]
CASES = [(s, "random") for s in SHAPES] + [(s, c) for s in ((1, 30, 46), (32, 96, 96)) for c in ("peaks", "ties", "dead")]


def _operands(shape, case):
    N, H, W = shape
    g = torch.Generator().manual_seed(41)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    Hp, Wp = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
    x4 = torch.zeros(N, H, W, 4)
    x4[..., :3] = torch.randn(N, H, W, 3, generator=g)
    y0 = torch.randn(N, Ho, Wo, C, generator=g)
    scale = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.arange(C) % 5 == 0, -1.0, 1.0)
    shift = torch.randn(C, generator=g) * 0.3
    mean = torch.randn(C, generator=g) * 0.1
    rstd = torch.rand(C, generator=g) + 0.5
    gamma = torch.rand(C, generator=g) + 0.5
    gp = torch.randn(N, Hp, Wp, C, generator=g)
    if case == "peaks":
        # strict local peaks, period 8: at (1, 1) mod 8 -- odd/odd, the argmax of the four windows that cover it -- and
        # at (5, 4) mod 8 -- odd/even, the argmax of two; no window holds two peaks.  Positive scales keep them peaks
        # after BatchNorm + ReLU.  The covering windows carry gradients of mixed sign and magnitude: on even channels
        # 1, 2^-9, -1, 3 * 2^-8 (exact in fp32 in any order, not if a partial sum were rounded to bf16), on odd channels
        # 1, 2^-26, -1, 3 * 2^-25 (the fp32 sum depends on the order of the additions)
        scale = scale.abs()
        y0 = torch.rand(N, Ho, Wo, C, generator=g) * 0.5
        hh, ww = torch.arange(Ho).view(Ho, 1), torch.arange(Wo).view(1, Wo)
        peak = ((hh % 8 == 1) & (ww % 8 == 1)) | ((hh % 8 == 5) & (ww % 8 == 4))
        y0 = torch.where(peak.view(1, Ho, Wo, 1), y0 + 4.0, y0)
        even = torch.tensor([1.0, 2.0 ** -9, -1.0, 3 * 2.0 ** -8])
        odd = torch.tensor([1.0, 2.0 ** -26, -1.0, 3 * 2.0 ** -25])
        a, b_, c = torch.arange(Hp).view(Hp, 1, 1), torch.arange(Wp).view(1, Wp, 1), torch.arange(C).view(1, 1, C)
        k = ((a % 2) * 2 + (b_ % 2) + c // 2) % 4
        gp = torch.where(c % 2 == 0, even[k], odd[k]).expand(N, Hp, Wp, C).contiguous()
    elif case == "ties":
        y0 = (torch.randint(0, 3, (N, Ho, Wo, C), generator=g).float() - 1.0) * 0.5       # three levels: ties everywhere
    elif case == "dead":
        shift = torch.where(torch.arange(C) % 3 == 1, -100.0, shift)                      # ReLU-dead channels
        gp = torch.zeros(N, Hp, Wp, C)
    t = dict(x4=x4.to(DEV).to(BF), y0=y0.to(DEV).to(BF), gp=gp.to(DEV).to(BF))
    for k_, v in dict(scale=scale, shift=shift, mean=mean, rstd=rstd, gamma=gamma).items():
        t[k_] = v.to(DEV)
    t.update(dims=(N, H, W, Ho, Wo, Hp, Wp))
    return t


@functools.lru_cache(maxsize=None)
def _results(shape, case):
    """Reference and two fused calls, computed once per (shape, case) and shared by the tests below (read only)."""
    from isic_hip.lib import call
    t = _operands(shape, case)
    N, H, W, Ho, Wo, Hp, Wp = t["dims"]
    x4, y0, gp = t["x4"], t["y0"], t["gp"]
    scale, shift, mean, rstd, gamma = t["scale"], t["shift"], t["mean"], t["rstd"], t["gamma"]
    p, am = torch.empty(N, Hp, Wp, C, device=DEV, dtype=BF), torch.empty(N, Hp, Wp, C, device=DEV, dtype=torch.uint8)
    call("isic_bn_relu_maxpool3x3s2_fwd_bf16", y0, scale, shift, p, am, N, Ho, Wo, C, Hp, Wp)
    acc = torch.zeros(2, C, device=DEV, dtype=torch.float64)
    call("isic_bn_bwd_reduce_pooled_bf16", am, gp, y0, mean, rstd, N, Ho, Wo, C, Hp, Wp, scale, shift, acc[0], acc[1])
    dy = torch.empty_like(y0)
    dg_ref, db_ref = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    call("isic_bn_bwd_apply_pooled_bf16", am, gp, y0, mean, rstd, gamma, acc[0], acc[1], N, Ho, Wo, C, Hp, Wp, scale, shift,
         dy, dg_ref, db_ref)
    dw_ref = torch.zeros(64, 3, 7, 7, device=DEV).contiguous(memory_format=torch.channels_last)
    wsp = torch.empty(call("isic_conv_stem_wgrad_workspace_bytes"), device=DEV, dtype=torch.uint8)
    call("isic_conv_stem_wgrad_bf16", x4, dy, dw_ref, N, H, W, Ho, Wo, wsp, wsp.numel())
    fused = []
    for _ in range(2):
        dw = torch.zeros_like(dw_ref)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        wsp.fill_(0xAB)                                                   # the workspace carries nothing between calls
        call("isic_conv_stem_wgrad_bn_pooled_bf16", x4, y0, am, gp, mean, rstd, gamma, scale, shift, acc[0], acc[1], dw,
             dg, db, N, H, W, Ho, Wo, Hp, Wp, wsp, wsp.numel())
        fused.append((dw.cpu(), dg.cpu(), db.cpu()))
    return dict(dw_ref=dw_ref.cpu(), dg_ref=dg_ref.cpu(), db_ref=db_ref.cpu(), fused=fused, am=am.cpu(), dims=t["dims"])


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else v


@pytest.mark.parametrize("shape,case", CASES, ids=_ids)
def test_fused_equals_two_kernel_path(shape, case):
    r = _results(shape, case)
    dw, dg, db = r["fused"][0]
    print(f"{shape} {case}: max|dw - dw_ref| = {float((dw - r['dw_ref']).abs().max()):.3e}, "
          f"max|dw_ref| = {float(r['dw_ref'].abs().max()):.3e}")
    assert torch.isfinite(dw).all()
    assert torch.equal(dg, r["dg_ref"]) and torch.equal(db, r["db_ref"])
    assert_close(dw, r["dw_ref"], rtol=1e-4, atol=1e-4 * float(r["dw_ref"].abs().max()), what=f"fused stem wgrad {shape} {case}")


@pytest.mark.parametrize("shape,case", CASES, ids=_ids)
def test_fused_is_repeatable(shape, case):
    (dw1, dg1, db1), (dw2, dg2, db2) = _results(shape, case)["fused"]
    assert torch.equal(dw1, dw2) and torch.equal(dg1, dg2) and torch.equal(db1, db2)


@pytest.mark.parametrize("shape", [(1, 30, 46), (32, 96, 96)], ids=_ids)
def test_peaks_case_has_pixels_fed_by_three_or_more_windows(shape):
    """A condition on the INPUT of the "peaks" case, read from the argmax codes (kh * 3 + kw of window (a, b) points at
    pixel (2a - 1 + kh, 2b - 1 + kw)): at least 1 % of the (pixel, channel) entries receive three or more contributions."""
    r = _results(shape, "peaks")
    N, _, _, Ho, Wo, Hp, Wp = r["dims"]
    am = r["am"].long()
    hi = torch.arange(Hp).view(1, Hp, 1, 1) * 2 - 1 + am // 3
    wi = torch.arange(Wp).view(1, 1, Wp, 1) * 2 - 1 + am % 3
    assert int(hi.min()) >= 0 and int(hi.max()) < Ho and int(wi.min()) >= 0 and int(wi.max()) < Wo
    n_i = torch.arange(N).view(N, 1, 1, 1).expand_as(am)
    c_i = torch.arange(C).view(1, 1, 1, C).expand_as(am)
    flat = ((n_i * Ho + hi) * Wo + wi) * C + c_i
    cnt = torch.zeros(N * Ho * Wo * C, dtype=torch.long).index_add_(0, flat.reshape(-1), torch.ones(flat.numel(), dtype=torch.long))
    frac = float((cnt >= 3).float().mean())
    print(f"{shape}: {frac:.4f} of the entries receive >= 3 contributions")
    assert frac >= 0.01
