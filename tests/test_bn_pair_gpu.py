"""BatchNorm backward of a downsample block's two norms in one reduce and one apply pass (isic_bn_bwd_reduce_pair_bf16,
isic_bn_bwd_apply_pair_bf16; include/isic_hip_bn_pair.h) against the four launches they replace:
isic_bn_bwd_reduce_mask_bf16 and isic_bn_bwd_apply_mask_bf16 with a residual gradient, then isic_bn_bwd_reduce_bf16 and
isic_bn_bwd_apply_bf16 (relu = 0) on that residual.

Every comparison is exact.  The pair kernels use the launch geometry and the thread -> (row, channel group) mapping of the
kernels they replace and evaluate the same expressions in the same order, so every per-thread partial sum, every fp64
block sum and every output element is the value the four launches give."""
import functools

import pytest
import torch

from isic_hip.lib import IsicHipError, call

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16

SHAPES = [               # N, H, W, C
    (1, 1, 1, 128),      # one row
    (3, 7, 7, 128),      # 147 rows: two reduce blocks, a ragged last apply block
    (2, 14, 14, 256),    # 256 channels
    (3, 7, 7, 512),      # 64 channel groups, 4 row lanes
    (5, 28, 28, 128),    # 31 reduce blocks, 62 apply blocks
]
GRADS = ("dgamma", "dbeta", "dgamma2", "dbeta2")


def _operands(N, H, W, C, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    uni = lambda *s: torch.rand(*s, device=DEV, generator=gen)
    g, c2, cd = (rnd(N, H, W, C).to(BF) for _ in range(3))
    mask = torch.randint(0, 256, (N * H * W * C // 8,), device=DEV, dtype=torch.uint8, generator=gen)
    norms = []
    for _ in range(2):
        mean, rstd, gamma = 0.3 * rnd(C), 0.5 + uni(C), 0.5 + uni(C)
        gamma[::5] *= -1.0                                # a negative scale on every fifth channel
        norms.append((mean, rstd, gamma))
    start = {k: rnd(C) for k in GRADS}                    # running parameter gradients: not zero
    return g, c2, cd, mask, norms, start


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Operands and the four-launch reference of one shape, computed once and shared (nothing below writes to them)."""
    N, H, W, C = shape
    rows = N * H * W
    g, c2, cd, mask, ((mean, rstd, gamma), (mean2, rstd2, gamma2)), start = _operands(N, H, W, C, 300 + rows + C)
    ref = {k: v.clone() for k, v in start.items()}
    acc = torch.zeros(2, C, device=DEV, dtype=torch.float64)          # bn2: sum dz * xhat, sum dz
    accd = torch.zeros(2, C, device=DEV, dtype=torch.float64)         # shortcut norm: the same two
    call("isic_bn_bwd_reduce_mask_bf16", g, c2, mask, mean, rstd, rows, C, acc[0], acc[1])
    dx, dres = torch.full_like(c2, float("nan")), torch.full_like(c2, float("nan"))
    call("isic_bn_bwd_apply_mask_bf16", g, c2, mask, mean, rstd, gamma, acc[0], acc[1], rows, C, dx, dres, ref["dgamma"],
         ref["dbeta"])
    call("isic_bn_bwd_reduce_bf16", dres, cd, None, mean2, rstd2, rows, C, 0, None, None, accd[0], accd[1])
    dx2 = torch.full_like(cd, float("nan"))
    call("isic_bn_bwd_apply_bf16", dres, cd, None, mean2, rstd2, gamma2, accd[0], accd[1], rows, C, 0, None, None, dx2, None,
         ref["dgamma2"], ref["dbeta2"])
    torch.cuda.synchronize()
    ref.update(sum_dzx=acc[0], sum_dz=acc[1], sum_dzx2=accd[0], sum_dz2=accd[1], dx=dx, dx2=dx2)
    return (g, c2, cd, mask, (mean, rstd, gamma), (mean2, rstd2, gamma2), start), ref


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair_equals_the_four_launches(shape):
    N, H, W, C = shape
    rows = N * H * W
    (g, c2, cd, mask, (mean, rstd, gamma), (mean2, rstd2, gamma2), start), ref = _case(shape)
    assert torch.equal(ref["sum_dz2"], ref["sum_dz"]), "the reference's two sums of dz differ"

    acc = torch.zeros(3, C, device=DEV, dtype=torch.float64)
    call("isic_bn_bwd_reduce_pair_bf16", g, c2, mask, mean, rstd, cd, mean2, rstd2, rows, C, acc[0], acc[1], acc[2])
    got = {k: v.clone() for k, v in start.items()}
    dx, dx2 = torch.full_like(c2, float("nan")), torch.full_like(cd, float("nan"))
    call("isic_bn_bwd_apply_pair_bf16", g, c2, mask, mean, rstd, gamma, acc[0], acc[1], cd, mean2, rstd2, gamma2, acc[2], rows,
         C, dx, dx2, got["dgamma"], got["dbeta"], got["dgamma2"], got["dbeta2"])
    torch.cuda.synchronize()

    for k, a in (("sum_dzx", acc[0]), ("sum_dz", acc[1]), ("sum_dzx2", acc[2])):
        print(f"{k}: max |pair - ref| = {float((a - ref[k]).abs().max()):.3e}")
        assert torch.equal(a, ref[k]), k
        assert bool((a != 0).any()), f"{k} was not accumulated"
    for k, a in (("dx", dx), ("dx2", dx2)):
        n = int((_bits(a) != _bits(ref[k])).sum())
        print(f"{k}: {n} of {a.numel()} bit patterns differ")
        assert not bool(torch.isnan(ref[k].float()).any()), f"reference {k} has unwritten elements"
        assert n == 0, f"{k}: {n} of {a.numel()} bit patterns differ"
        assert not bool(torch.isnan(a.float()).any()), f"{k} has unwritten elements"
        assert float(a.float().abs().max()) > 0
    for k in GRADS:
        assert torch.equal(got[k], ref[k]), f"{k}: max diff {float((got[k] - ref[k]).abs().max()):.3e}"
        assert not torch.equal(got[k], start[k]), f"{k} did not move from its starting value"


def test_unsupported_channel_count_and_null_operand_launch_nothing():
    N, H, W, C = 2, 3, 3, 24                               # 3 channel groups: 256 % 3 != 0
    rows = N * H * W
    g, c2, cd, mask, ((mean, rstd, gamma), (mean2, rstd2, gamma2)), start = _operands(N, H, W, C, 9)
    acc = torch.zeros(3, C, device=DEV, dtype=torch.float64)
    dx, dx2 = torch.full_like(c2, float("nan")), torch.full_like(cd, float("nan"))
    got = {k: v.clone() for k, v in start.items()}
    with pytest.raises(IsicHipError) as e:
        call("isic_bn_bwd_reduce_pair_bf16", g, c2, mask, mean, rstd, cd, mean2, rstd2, rows, C, acc[0], acc[1], acc[2])
    assert e.value.code == -2
    with pytest.raises(IsicHipError) as e:
        call("isic_bn_bwd_apply_pair_bf16", g, c2, mask, mean, rstd, gamma, acc[0], acc[1], cd, mean2, rstd2, gamma2, acc[2],
             rows, C, dx, dx2, got["dgamma"], got["dbeta"], got["dgamma2"], got["dbeta2"])
    assert e.value.code == -2

    (g, c2, cd, mask, (mean, rstd, gamma), (mean2, rstd2, gamma2), start2), _ = _case(SHAPES[1])
    N, H, W, C = SHAPES[1]
    rows = N * H * W
    acc2 = torch.zeros(3, C, device=DEV, dtype=torch.float64)
    dy, dy2 = torch.full_like(c2, float("nan")), torch.full_like(cd, float("nan"))
    got2 = {k: v.clone() for k, v in start2.items()}
    with pytest.raises(IsicHipError) as e:
        call("isic_bn_bwd_reduce_pair_bf16", g, c2, mask, mean, rstd, None, mean2, rstd2, rows, C, acc2[0], acc2[1], acc2[2])
    assert e.value.code == -1
    with pytest.raises(IsicHipError) as e:
        call("isic_bn_bwd_apply_pair_bf16", g, c2, mask, mean, rstd, gamma, acc2[0], acc2[1], None, mean2, rstd2, gamma2,
             acc2[2], rows, C, dy, dy2, got2["dgamma"], got2["dbeta"], got2["dgamma2"], got2["dbeta2"])
    assert e.value.code == -1
    torch.cuda.synchronize()
    for a, out, out2, gr, st in ((acc, dx, dx2, got, start), (acc2, dy, dy2, got2, start2)):
        assert not bool((a != 0).any())
        assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(out2.float()).all())
        assert all(torch.equal(gr[k], st[k]) for k in GRADS)


@pytest.mark.parametrize("fold", [True, False], ids=["folded_shortcut_norm", "materialised_shortcut_norm"])
def test_encoder_gradients_do_not_depend_on_the_pairing(fold):
    """Forward + backward of the whole ResNet-18 on 4 images of 64 x 64 (layer2.0 sees 16 x 16, layer4.0 4 x 4) from the same
    parameters, inputs and feature gradient with ``pair_shortcut_norm_backward`` on and off: every parameter gradient is
    bit-identical, and the pair ran once per downsample block when on and never when off."""
    from isic_hip.encoder import ResNet18Encoder
    torch.manual_seed(11)
    enc = ResNet18Encoder().to(DEV)
    enc.train()
    enc.fold_shortcut_norm = fold
    gen = torch.Generator(device=DEV).manual_seed(23)
    x = torch.randn(4, 3, 64, 64, device=DEV, generator=gen).to(BF)
    dfeat = torch.randn(4, 512, device=DEV, generator=gen) / 4
    served = []
    inner = enc._bn_bwd_pair

    def counted(*a, **k):
        out = inner(*a, **k)
        served.append(out is not None)
        return out

    enc._bn_bwd_pair = counted

    def run(on):
        del served[:]
        enc.pair_shortcut_norm_backward = on
        for p in enc.parameters():
            p.grad = None
        _, tape = enc.run_forward(x, save=True)
        enc.run_backward(tape, dfeat)
        torch.cuda.synchronize()
        return {k: p.grad.detach().clone() for k, p in enc.named_parameters()}, list(served)

    g_on, n_on = run(True)
    g_off, n_off = run(False)
    assert n_on == [True, True, True] and n_off == []
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in g_on.values())
    diff = [k for k in g_on if not torch.equal(g_on[k], g_off[k])]
    assert not diff, f"paired vs four launches: parameter gradients differ: {diff}"
