"""The stem's two forward kernels at small shapes where their tiling can go wrong: the 7x7/2 convolution with the
register-only epilogue (8 x 16 output tiles, permuted weight rows, paired 128-byte stores, fused BatchNorm sums) and the
tiled BatchNorm + ReLU + max-pool that normalises each pixel once (packed value/tap keys, argmax, raw value at the argmax).

References: the fp32 convolution on bf16-rounded operands with the tolerance of
``test_encoder_gpu.py::test_stem_forward_and_wgrad``; for the pool a torch restatement, element for element, and the
unfused kernels (``isic_bn_apply_bf16`` -> ``isic_maxpool3x3s2_fwd_bf16``) that
``test_encoder_gpu.py::test_stem_fused_bn_relu_maxpool_and_pooled_bn_backward`` pins it to."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from encoder_ops_ref import pool_restatement as _pool_restatement
from test_encoder_gpu import BF, DEV, bf16_close, from_nhwc, krsc, rb

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC1          # a bf16 NaN pattern no kernel writes


@pytest.mark.parametrize("shape", [(2, 32, 32),      # 16 x 16 outputs: exact 8 x 16 tiles
                                   (2, 38, 38),      # 19 x 19: ragged both ways
                                   (3, 34, 70),      # 17 x 35: three column tiles, the last with 3 columns
                                   (2, 37, 45)])     # odd width: 19 x 23
def test_stem_forward_register_epilogue(shape):
    from isic_hip.lib import call
    N, H, W = shape
    g = torch.Generator().manual_seed(11)
    x = rb(torch.randn(N, 3, H, W, generator=g))
    # a distinct scale per output channel: a channel landing in another channel's place cannot pass
    chan = (0.5 + torch.arange(64) / 16.0).view(64, 1, 1, 1)
    w = rb(torch.randn(64, 3, 7, 7, generator=g) / np.sqrt(147.0) * chan)
    y = F.conv2d(x, w, None, 2, 3)
    Ho, Wo = y.shape[2], y.shape[3]
    x4 = torch.empty(N, H, W, 4, device=DEV, dtype=BF)
    call("isic_nchw_to_nhwc4_bf16", x.to(DEV), 0, x4, N, 3, H, W)
    ws = torch.empty(64 * 7 * 8 * 4, device=DEV, dtype=BF)
    call("isic_conv_stem_pack_bf16", krsc(w), ws)
    n_out, guard = N * Ho * Wo * 64, 64 * 64
    outs = []
    for stats in (False, True):
        buf = torch.full((guard + n_out + guard,), SENTINEL, device=DEV, dtype=torch.int16)
        out = buf[guard:guard + n_out].view(BF).view(N, Ho, Wo, 64)
        st = torch.zeros(2, 32, 64, device=DEV, dtype=torch.float64)
        if stats:
            call("isic_conv_stem_fwd_stats_bf16", x4, ws, out, N, H, W, Ho, Wo, st[0], st[1], 32)
        else:
            call("isic_conv_stem_fwd_bf16", x4, ws, out, N, H, W, Ho, Wo)
        torch.cuda.synchronize()
        # ragged stores: nothing outside the tensor is touched, every element inside is written
        assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n_out:] == SENTINEL).all()), "store out of range"
        assert not bool((buf[guard:guard + n_out] == SENTINEL).any()), "output element not written"
        bf16_close(from_nhwc(out), y, f"stem fwd {shape} stats={stats}")
        outs.append(out.clone())
        if stats:
            # the fused sums are those of the kernel's own rounded output.  They differ from the float64 sums by the fp32
            # partials alone: a block (one tile each at these shapes) adds 2 values in a lane, 16 lanes by a butterfly and
            # 4 waves -- 7 fp32 roundings, each at most 2^-24 of the partial's magnitude <= sum |v|
            o = out.float().reshape(-1, 64).double()
            for got, vals, what in ((st[0].sum(0), o, "sum"), (st[1].sum(0), o * o, "sumsq")):
                err = (got - vals.sum(0)).abs()
                bound = 8 * 2.0 ** -24 * vals.abs().sum(0) + 1e-12
                assert bool((err <= bound).all()), f"stem fused {what} {shape}: {float(err.max()):.3e} > {float(bound.min()):.3e}"
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("hw", [(16, 16),     # Hp = Wp = 8
                                (19, 19),     # Hp = 10, last window clipped
                                (9, 35),      # Wp = 18
                                (8, 66)])     # Wp = 33: several column tiles and a ragged one
def test_fused_bn_relu_maxpool_normalises_once(hw):
    from isic_hip.lib import call
    N, C = 2, 64
    H, W = hw
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    g = torch.Generator().manual_seed(23)
    # a handful of bf16 values (ties are frequent); scale / shift on coarse grids, so that x * scale + shift is exact in
    # fp32 and the fused and unfused forms of the multiply-add agree
    vals = torch.tensor([-2.0, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 2.0])
    x = vals[torch.randint(0, len(vals), (N, H, W, C), generator=g)].to(DEV).to(BF)
    scale = torch.randint(4, 13, (C,), generator=g).float() / 8.0
    scale[torch.arange(C) % 5 == 0] *= -1.0
    shift = torch.randint(-16, 17, (C,), generator=g).float() / 16.0
    scale[3], shift[3] = 0.0, 0.25            # every window ties: the first valid tap must win
    scale[7], shift[7] = 0.0, -0.0            # ... at zero, formed as +0.0 and -0.0
    shift[11] = -100.0                        # all zero after the ReLU
    scale, shift = scale.to(DEV), shift.to(DEV)
    p = torch.full((N, Ho, Wo, C), SENTINEL, device=DEV, dtype=torch.int16).view(BF)
    xs = torch.full((N, Ho, Wo, C), SENTINEL, device=DEV, dtype=torch.int16).view(BF)
    am = torch.full((N, Ho, Wo, C), 0xEE, device=DEV, dtype=torch.uint8)
    call("isic_bn_relu_maxpool3x3s2_fwd_sel_bf16", x, scale, shift, p, am, xs, N, H, W, C, Ho, Wo)
    y_ref, am_ref, xs_ref = _pool_restatement(x, scale, shift, Ho, Wo)
    assert int(am_ref.max()) <= 8 and not bool(torch.isnan(xs_ref).any())
    assert torch.equal(am, am_ref), f"argmax {hw}: {int((am != am_ref).sum())} differ"
    assert torch.equal(p.view(torch.int16), y_ref.to(BF).view(torch.int16)), f"y {hw}"
    assert torch.equal(xs.view(torch.int16), xs_ref.to(BF).view(torch.int16)), f"x_sel {hw}"
    # the entry point without x_sel, and the unfused kernels
    p2, am2 = torch.empty_like(p), torch.empty_like(am)
    call("isic_bn_relu_maxpool3x3s2_fwd_bf16", x, scale, shift, p2, am2, N, H, W, C, Ho, Wo)
    assert torch.equal(p2.view(torch.int16), p.view(torch.int16)) and torch.equal(am2, am)
    yfull = torch.empty_like(x)
    call("isic_bn_apply_bf16", x, scale, shift, None, yfull, N * H * W, C, 1)
    p3, am3 = torch.empty_like(p), torch.empty_like(am)
    call("isic_maxpool3x3s2_fwd_bf16", yfull, p3, am3, N, H, W, C, Ho, Wo)
    assert torch.equal(p3.view(torch.int16), p.view(torch.int16)) and torch.equal(am3, am)
