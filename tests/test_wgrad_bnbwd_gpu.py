"""The 64 -> 64 weight gradient with BatchNorm backward's apply pass folded into its staging waves
(isic_conv2d_wgrad_bnbwd_bf16) against the two launches it replaces: isic_bn_bwd_apply_bf16 / isic_bn_bwd_apply_mask_bf16
followed by isic_conv2d_wgrad_bf16.

Every comparison is exact.  The fused kernel evaluates the apply pass's expression on the same operands (dc: equal 16-bit
patterns), puts the same values into the same LDS slots, walks the same tiles and adds the same per-block partials in the
same order (dw: torch.equal), and adds the same fp64 sums into the fp32 parameter gradients (dgamma, dbeta: torch.equal)."""
import pytest
import torch

from isic_hip.lib import IsicHipError, call

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
C = 64

SHAPES = [            # N, H, W  (tiles are 4 rows x 32 columns; one persistent block per CU walks consecutive tiles)
    (1, 4, 32),       # one tile: the ring's prologue with a single tile per block
    (2, 8, 32),       # 4 tiles
    (3, 9, 13),       # ragged rows and columns, a tile cut by the border
    (2, 6, 40),       # the second column tile cut
    (24, 56, 56),     # 672 tiles, three per block on 256 CUs: the three-stage ring wraps
]


def _operands(N, H, W, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    x, g, c = (rnd(N, H, W, C).to(BF) for _ in range(3))
    mean, rstd = 0.3 * rnd(C), 0.5 + torch.rand(C, device=DEV, generator=gen)
    gamma, beta = 0.5 + torch.rand(C, device=DEV, generator=gen), 0.2 * rnd(C)
    gamma[::5] *= -1.0                                   # scale < 0 on every fifth channel: the recomputed mask flips there
    scale = gamma * rstd
    shift = beta - mean * scale
    mask = torch.randint(0, 256, (N * H * W * C // 8,), device=DEV, dtype=torch.uint8, generator=gen)
    start = {"dw": rnd(C, 3, 3, C), "dgamma": rnd(C), "dbeta": rnd(C)}          # running gradients: not zero
    return x, g, c, mean, rstd, gamma, scale, shift, mask, start


@pytest.mark.parametrize("mode", ["recompute", "maskbits"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_equals_apply_then_wgrad(shape, mode):
    N, H, W = shape
    rows = N * H * W
    x, g, c, mean, rstd, gamma, scale, shift, mask, start = _operands(N, H, W, 100 + rows)
    use_mask = mode == "maskbits"
    assert call("isic_conv2d_wgrad_bnbwd_supported", N, H, W, C, C, 3, 3, 1, 1, int(use_mask)) == 1
    acc = torch.zeros(2, C, device=DEV, dtype=torch.float64)                    # (sum dz * xhat, sum dz)
    if use_mask:
        call("isic_bn_bwd_reduce_mask_bf16", g, c, mask, mean, rstd, rows, C, acc[0], acc[1])
    else:
        call("isic_bn_bwd_reduce_bf16", g, c, None, mean, rstd, rows, C, 1, scale, shift, acc[0], acc[1])
    ws = torch.empty(call("isic_conv2d_wgrad_workspace_bytes", N, C, H, W, C, 3, 3), device=DEV, dtype=torch.uint8)

    ref = {k: v.clone() for k, v in start.items()}
    dc_ref = torch.empty_like(c)
    if use_mask:
        call("isic_bn_bwd_apply_mask_bf16", g, c, mask, mean, rstd, gamma, acc[0], acc[1], rows, C, dc_ref, None,
             ref["dgamma"], ref["dbeta"])
    else:
        call("isic_bn_bwd_apply_bf16", g, c, None, mean, rstd, gamma, acc[0], acc[1], rows, C, 1, scale, shift, dc_ref, None,
             ref["dgamma"], ref["dbeta"])
    call("isic_conv2d_wgrad_bf16", x, dc_ref, ref["dw"], N, H, W, C, H, W, C, 3, 3, 1, 1, ws, ws.numel())

    got = {k: v.clone() for k, v in start.items()}
    dc = torch.full_like(c, float("nan"))
    call("isic_conv2d_wgrad_bnbwd_bf16", x, g, c, mask if use_mask else None, mean, rstd, gamma, acc[1], acc[0],
         None if use_mask else scale, None if use_mask else shift, dc, got["dw"], got["dgamma"], got["dbeta"], N, H, W,
         ws, ws.numel())
    torch.cuda.synchronize()
    a, b = dc.view(torch.int16), dc_ref.view(torch.int16)
    assert torch.equal(a, b), f"dc: {int((a != b).sum())} of {a.numel()} bit patterns differ"
    assert float(dc_ref.float().abs().max()) > 0
    assert torch.equal(got["dw"], ref["dw"]), f"dw: max diff {float((got['dw'] - ref['dw']).abs().max()):.3e}"
    assert not torch.equal(ref["dw"], start["dw"])
    assert torch.equal(got["dgamma"], ref["dgamma"]) and torch.equal(got["dbeta"], ref["dbeta"])
    assert not torch.equal(ref["dgamma"], start["dgamma"])


def test_other_layers_and_relu_forms_are_refused():
    assert call("isic_conv2d_wgrad_bnbwd_supported", 2, 8, 8, 64, 128, 3, 3, 1, 1, 0) == 0
    assert call("isic_conv2d_wgrad_bnbwd_supported", 2, 8, 8, 128, 128, 3, 3, 1, 1, 1) == 0
    assert call("isic_conv2d_wgrad_bnbwd_supported", 2, 8, 8, 64, 64, 3, 3, 2, 1, 0) == 0
    assert call("isic_conv2d_wgrad_bnbwd_supported", 2, 8, 8, 64, 64, 1, 1, 1, 0, 0) == 0
    N, H, W = 1, 4, 32
    x, g, c, mean, rstd, gamma, scale, shift, mask, start = _operands(N, H, W, 7)
    acc = torch.zeros(2, C, device=DEV, dtype=torch.float64)
    ws = torch.empty(call("isic_conv2d_wgrad_workspace_bytes", N, C, H, W, C, 3, 3), device=DEV, dtype=torch.uint8)
    dc = torch.empty_like(c)
    with pytest.raises(IsicHipError) as e:              # neither mask bits nor the forward affine: no mask form to apply
        call("isic_conv2d_wgrad_bnbwd_bf16", x, g, c, None, mean, rstd, gamma, acc[1], acc[0], None, None, dc, start["dw"],
             None, None, N, H, W, ws, ws.numel())
    assert e.value.code == -2
    with pytest.raises(IsicHipError) as e:
        call("isic_conv2d_wgrad_bnbwd_bf16", x, g, c, mask, mean, rstd, gamma, acc[1], acc[0], None, None, dc, start["dw"],
             None, None, N, H, W, ws, 16)
    assert e.value.code == -3


def test_encoder_gradients_do_not_depend_on_the_fusion():
    """One forward + backward of layer1 and layer2 on 16 images of 64 x 64 with ``fuse_bn_apply_wgrad`` on, off, and on
    with the weight gradients on the side stream (which must take the two-launch path): every parameter gradient and the
    gradient that leaves the first block towards the stem are bit-identical."""
    from isic_hip.encoder import ResNet18Encoder
    torch.manual_seed(5)
    enc = ResNet18Encoder(layers=((64, 1), (128, 2))).to(DEV)
    enc.train()
    gen = torch.Generator(device=DEV).manual_seed(17)
    x = torch.randn(16, 3, 64, 64, device=DEV, generator=gen).to(BF)
    dfeat = torch.randn(16, 128, device=DEV, generator=gen) / 16
    calls = []
    inner = enc._bn_bwd_wgrad
    block = enc.block_backward_fused
    first = {}

    def counted(*a, **k):
        dc = inner(*a, **k)
        calls.append(dc is not None)
        return dc

    def recorded(g, pre, ds, saved, **k):
        out = block(g, pre, ds, saved, **k)
        if pre == "layer1.0":
            first["dx"] = out[0].clone()
        return out

    enc._bn_bwd_wgrad, enc.block_backward_fused = counted, recorded

    def run():
        del calls[:]
        for p in enc.parameters():
            p.grad = None
        _, tape = enc.run_forward(x, save=True)
        enc.run_backward(tape, dfeat)
        torch.cuda.synchronize()
        return {k: p.grad.detach().clone() for k, p in enc.named_parameters()}, first.pop("dx"), sum(calls)

    assert not enc.wgrad_stream
    enc.fuse_bn_apply_wgrad = True
    g_on, dx_on, n_on = run()
    enc.fuse_bn_apply_wgrad = False
    g_off, dx_off, n_off = run()
    enc.fuse_bn_apply_wgrad = True
    enc.wgrad_stream = True
    g_side, dx_side, n_side = run()
    enc.wgrad_stream = False
    assert n_on == 4 and n_off == 0 and n_side == 0       # layer1: two blocks x (bn2 -> conv2, bn1 -> conv1)
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in g_on.values())
    for what, g2, dx2 in (("off", g_off, dx_off), ("side stream", g_side, dx_side)):
        diff = [k for k in g_on if not torch.equal(g_on[k], g2[k])]
        assert not diff, f"fused vs {what}: parameter gradients differ: {diff}"
        assert torch.equal(dx_on.view(torch.int16), dx2.view(torch.int16)), f"fused vs {what}: input-side gradient differs"
    # a toggle between forward and backward must not split the pass: the tape decides
    for p in enc.parameters():
        p.grad = None
    _, tape = enc.run_forward(x, save=True)
    enc.fuse_bn_apply_wgrad = False
    del calls[:]
    enc.run_backward(tape, dfeat)
    enc.fuse_bn_apply_wgrad = True
    torch.cuda.synchronize()
    assert sum(calls) == 4
    assert all(torch.equal(g_on[k], p.grad) for k, p in enc.named_parameters())
