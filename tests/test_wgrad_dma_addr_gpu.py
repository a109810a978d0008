"""The all-taps weight-gradient kernels (conv_wgrad_c128b.hip, conv_wgrad_s2.hip) on the border geometries of their LDS-DMA
address arithmetic (csrc/wgrad_dma_addr.inc) that tests/test_conv_bf16_domain_gpu.py does not have: cut and empty column
groups, a bottom band with one valid row, a second tile in a row, packs of two and four images that are partly empty, blocks
with one tile (the prefetch is dead from the start) and a last block with fewer tiles than the others.

Method of tests/conv_bf16_ref.py: inputs for which fp32 accumulation is exact in any order (family I, dyadic; family P, one
non-zero gradient pixel per output channel), compared with == against the fp64 sum; every case also runs the per-tap kernel
(variant bit 4 of isic_test_conv2d_wgrad_variant_bf16) on the same inputs and requires the same bits.  The exactness condition
and the block shapes each case is meant for are checked on the CPU (the test without the gpu mark)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_bf16_ref as R  # noqa: E402
from helpers import DEV, stop_after_a_device_error  # noqa: E402

BF = torch.bfloat16


def _uneven_n(plan_of_n):
    """the smallest N whose blocks own two tiles except the last one, which owns one"""
    n = 1
    while True:
        p = plan_of_n(n)
        if p.tiles_per_block == 2 and p.total_tiles % 2 == 1:
            return n
        assert p.tiles_per_block <= 2, n
        n += 1


def cases(cus=R.CUS):
    """-> [Box(id, g, kernel, pack, tpb (tiles per block the case is meant for, None: not pinned), uneven)]; (W x H as in the
    kernels' tile: 32 columns by 4 (stride 1) or 2 (stride 2) output rows)"""
    C = []

    def add(cid, kernel, N, H, W, Ci, Co, pack, tpb=None, uneven=False):
        g = R.wgrad_geom(N, H, W, Ci, Co, 3, 1 if kernel == "wc128b" else 2, 1)
        C.append(R.Box(id=cid, g=g, kernel=kernel, pack=pack, tpb=tpb, uneven=uneven))
    add("c128b-28x28-bench-row", "wc128b", 3, 28, 28, 128, 64, 1)           # the right-hand groups cut, the last one outside
    add("c128b-32x5-one-row-band", "wc128b", 2, 5, 32, 128, 128, 1)
    add("c128b-40x4-second-tile", "wc128b", 2, 4, 40, 128, 128, 1)           # x0 = 32: eight columns
    add("c128b-14x14-pack2-half-empty", "wc128b", 3, 14, 14, 256, 128, 2)    # 2 x 2 (ci, co) pairs
    add("c128b-7x7-pack4-one-image", "wc128b", 5, 7, 7, 128, 192, 4)
    add("c128b-one-tile-per-block", "wc128b", 2, 6, 20, 128, 64, 1, tpb=1)   # 4 tiles on 4 blocks: no live prefetch at all
    n = _uneven_n(lambda n: R.wc128b_plan(n, 4, 8, 128, 256, cus))
    add("c128b-short-last-block", "wc128b", n, 4, 8, 128, 256, 2, tpb=2, uneven=True)
    add("s2-56x56-bench-layer2", "ws2", 2, 56, 56, 64, 128, 1)
    add("s2-28x28-pack2-4pairs", "ws2", 3, 28, 28, 128, 256, 2)
    add("s2-14x14-pack4-odd-rows", "ws2", 5, 14, 14, 128, 256, 4)            # Ho = 7: the last two-row band holds one row
    add("s2-80x8-second-tile", "ws2", 2, 8, 80, 64, 128, 1)
    return C


CASES = cases()


def _plan(c, cus):
    g = c.g
    return R.wc128b_plan(g.N, g.Hin, g.Win, g.Cin, g.Cout, cus) if c.kernel == "wc128b" else R.ws2_plan(g.N, g.Hin, g.Win, g.Cin, g.Cout, cus)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_case_is_exact_and_meets_the_block_shape_it_is_meant_for(c):
    g = c.g
    d = R.wgrad_dispatch(g, 0)
    p = _plan(c, R.CUS)
    assert (d.code, d.kernel, p.pack) == (R.OK, c.kernel, c.pack), (c.id, d, p)
    assert R.wgrad_dispatch(g, 16).kernel in ("wtap-big", "wtap-small")
    assert c.tpb is None or p.tiles_per_block == c.tpb, (c.id, p)
    if c.uneven:
        assert p.total_tiles - (p.blocks_per_pair - 1) * p.tiles_per_block < p.tiles_per_block, (c.id, p)
    if c.pack > 1:
        assert g.N % c.pack != 0, (c.id, "the last pack is meant to be partly empty")
    M = g.N * g.Hout * g.Wout
    assert R.exact_condition(M, 1, 1, 6, 4.0), (c.id, M)                     # family I on the 1/8 grid, dw0 within +-4
    assert R.wgrad_inputs(c.id, g, "I").grid == 3
    assert 2 ** 14 * 2 ** 8 <= 2 ** 24                                       # family P: one product s * x per element, |s| <= 2,
    #                                                                          x a multiple of 2^-13 below 2^7: 22 bits


@pytest.fixture
def _device_error_ends_the_session():
    yield
    stop_after_a_device_error()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_weight_gradient_equals_the_fp64_sum_and_the_per_tap_kernel(c, _device_error_ends_the_session):
    from isic_hip.lib import call
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = {k.id: k for k in cases(cus)}[c.id]
    g = c.g
    d, p = R.wgrad_dispatch(g, 0, cus), _plan(c, cus)
    assert (d.code, d.kernel) == (R.OK, c.kernel) and (c.tpb is None or p.tiles_per_block == c.tpb), (c.id, d, p)
    geo = (g.N, g.Hin, g.Win, g.Cin, g.Hout, g.Wout, g.Cout, g.Kh, g.Kw, g.stride, g.pad)
    nbytes = call("isic_conv2d_wgrad_workspace_bytes", g.N, g.Cin, g.Hout, g.Wout, g.Cout, g.Kh, g.Kw)
    assert nbytes == R.wgrad_workspace_bytes(g, cus)
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    for fam in ("I", "P"):
        inp = R.wgrad_inputs(c.id, g, fam)
        exact = inp.dw0.double() + R.wgrad_ref(g, inp.x, inp.dy)
        want = exact.float()
        assert torch.equal(want.double(), exact)
        x, dy = inp.x.to(DEV, BF), inp.dy.to(DEV, BF)
        got = []
        for entry, tail in (("isic_conv2d_wgrad_bf16", ()), ("isic_test_conv2d_wgrad_variant_bf16", (16,))):
            dw = inp.dw0.to(DEV).clone()
            call(entry, x, dy, dw, *geo, ws, nbytes, *tail)
            got.append(dw.cpu())
        for name, t in zip((c.kernel, "per-tap"), got):
            bad = (t != want) | t.isnan()
            idx = bad.nonzero()[:5].tolist()
            print(f"{c.id} family {fam} {name}: {int(bad.sum())} of {bad.numel()} elements differ from the fp64 sum")
            assert not bool(bad.any()), (c.id, fam, name, int(bad.sum()), idx, [(float(t[tuple(i)]), float(want[tuple(i)])) for i in idx])
        assert torch.equal(got[0], got[1]), (c.id, fam, "all-taps and per-tap kernels differ")
