"""The method of tests/conv_bf16_ref.py is sound, shown on the CPU: every case of every family meets its exactness condition,
for the small cases a plain fp32 convolution in two different summation orders equals the fp64 reference bit for bit (so a
device mismatch is a device error), the references agree with torch's own convolution / conv2d_input / conv2d_weight in
float64, the case table names the kernel the mirrored dispatch picks, and each emulated fault changes at least one expected
output of a case aimed at it."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conv_bf16_ref as R  # noqa: E402

CASES = R.conv_cases()
BY_ID = {c.id: c for c in CASES}
SMALL = [c for c in CASES if c.g.N * c.g.Hout * c.g.Wout * c.g.Cout * c.g.Kh * c.g.Kw * c.g.Cin <= 3e8]
WCASES = R.wgrad_cases()
WSMALL = [c for c in WCASES if c.g.N * c.g.Hout * c.g.Wout <= 2000]


def _fams(c):
    return ("I", "P", "S") if c.P else ("I", "S")


def _fp32_orders(g, x, w):
    """the convolution in fp32, every (tap, 64-channel chunk) product added to one fp32 accumulator: K-tiles ascending, and
    descending with the halves of every chunk swapped"""
    cv = R._canvas(g, x).float().permute(0, 2, 3, 1)                      # [N, Hc, Wc, C]
    tiles = [(kh, kw, c0) for kh in range(g.Kh) for kw in range(g.Kw) for c0 in range(0, g.Cin, 64)]
    outs = []
    for order in (tiles, tiles[::-1]):
        acc = torch.zeros(g.N * g.Hout * g.Wout, g.Cout)
        for kh, kw, c0 in order:
            xs = cv[:, kh:kh + g.up * (g.Hout - 1) + 1:g.up, kw:kw + g.up * (g.Wout - 1) + 1:g.up]
            halves = ((c0, c0 + 32), (c0 + 32, c0 + 64)) if order is tiles else ((c0 + 32, c0 + 64), (c0, c0 + 32))
            for a, b in halves:
                acc = acc + xs[..., a:b].reshape(-1, b - a) @ w[:, kh, kw, a:b].t()
        outs.append(acc.view(g.N, g.Hout, g.Wout, g.Cout))
    return outs


def test_every_case_of_every_family_meets_its_exactness_condition():
    """conv_inputs / wgrad_inputs assert the trivial bound themselves; the statistics cases add the pixels one fp32 partial
    covers in the kernel that runs (PIXELS_PER_PARTIAL x the tiles of a persistent block)"""
    for cus in (R.CUS, 304, 120):
        for c in R.conv_cases(cus):
            for epi in c.epi:
                add, stats = "add" in epi, "stats" in epi
                for v, _, _ in c.runs:
                    d = R.dispatch(c.g, v, add, stats, cus=cus)
                    assert d.code == R.OK, (c.id, v, epi)
                    if stats:
                        px = R.PIXELS_PER_PARTIAL[d.kernel] * d.tiles_per_block
                        assert R.stats_condition(px, 8.0 if add else 4.0, 3), (c.id, d.kernel, px)
        for c in R.bnbwd_cases(cus):
            px = R.PIXELS_PER_PARTIAL["halo-bnbwd"] * R.halo_plan(c.g.N, c.g.Hin, c.g.Win, c.g.Cin, c.g.Cout, 0, cus).tiles_per_block
            assert R.stats_condition(px, 8.0, 3) and px * 8.0 * 2.0 * 2 ** 5 < 2 ** 24, c.id      # dz y: multiples of 1/32, <= 16
    for c in CASES:
        if c.g.N * c.g.Hin * c.g.Win * c.g.Cin <= 2e6:
            for fam in _fams(c):
                inp = R.conv_inputs(c.id, c.g, fam, addend=True)
                for t in (inp.x, inp.w, inp.addend):
                    assert torch.equal(t.bfloat16().float(), t), (c.id, fam)
    for c in R.pair_cases():
        for fam in ("I", "P"):
            R.conv_inputs(c.id, c.g, fam, pair=True)
    for c in WCASES:
        for fam in ("I", "P"):
            inp = R.wgrad_inputs(c.id, c.g, fam)
            assert torch.equal(inp.x.bfloat16().float(), inp.x) and torch.equal(inp.dy.bfloat16().float(), inp.dy)
            if fam == "P":
                assert bool(((inp.dy != 0).sum((0, 1, 2)) == 1).all()), c.id
    # the coarser grids of the weight gradient are reached where 64 M >= 2^24
    assert R.wgrad_inputs("big", R.wgrad_geom(90, 56, 56, 64, 64, 3, 1, 1), "I").grid == 2


def test_the_case_table_names_the_kernel_the_mirrored_dispatch_picks():
    for cus in (R.CUS, 304, 120):
        for c in R.conv_cases(cus):
            for v, kernel, tpb in c.runs:
                d = R.dispatch(c.g, v, cus=cus)
                assert (d.code, d.kernel) == (R.OK, kernel), (c.id, v, d)
                assert tpb is None or d.tiles_per_block == tpb, (c.id, v, d)
        for c in R.pair_cases(cus):
            for v, kernel in c.runs:
                d = R.dispatch(c.g, v, pair=True, cus=cus)
                assert (d.code, d.kernel) == (R.OK, kernel), (c.id, v, d)
        for c in R.maskadd_cases(cus):
            d = R.dispatch(c.g, 0, addend=True, mask=True, cus=cus)
            assert (d.code, d.kernel) == (R.OK, c.kernel) and R.maskadd_supported(c.g) == 1, (c.id, d)
        for c in R.wgrad_cases(cus):
            for v, kernel, tpb in c.runs:
                d = R.wgrad_dispatch(c.g, v, cus)
                assert (d.code, d.kernel) == (R.OK, kernel), (c.id, v, d)
                assert tpb is None or d.tiles_per_block == tpb, (c.id, v, d)
                assert d.need <= R.wgrad_workspace_bytes(c.g, cus), c.id
            if "splits" in c:
                assert R.wgrad_dispatch(c.g, c.runs[0][0], cus).splits == c.splits, c.id
    kernels = {k for c in CASES for _, k, _ in c.runs}
    assert kernels == {"igemm64", "igemm128", "c64t", "c64p", "halo-k1", "halo-k2", "pgemm64", "pgemm128"}
    tiles = {(k, t) for c in CASES for _, k, t in c.runs if t}
    assert {("c64p", 2), ("c64p", 3), ("halo-k2", 2), ("halo-k1", 3), ("pgemm128", 2), ("pgemm128", 3)} <= tiles
    assert {k for c in WCASES for _, k, _ in c.runs} == {"wc64", "wc128b", "ws2", "wtap-big", "wtap-small"}
    packs = {(R.wgrad_dispatch(c.g, v).kernel, R.wgrad_dispatch(c.g, v).get("pack")) for c in WCASES for v, _, _ in c.runs}
    assert {("wc128b", 4), ("wc128b", 2), ("wc128b", 1), ("ws2", 4), ("ws2", 2), ("ws2", 1)} <= packs
    # the W = 63 / 64 border and the refusals the device test asserts
    assert R.halo_supported(1, 5, 63, 128, 128) and not R.halo_supported(1, 5, 64, 128, 128)
    g = R.fwd(2, 8, 8, 64, 64, 3, 1, 1)
    assert R.dispatch(g, 10000).code == R.BAD_ARG and R.dispatch(g, 5).code == R.BAD_ARG and R.dispatch(g, 40).code == R.BAD_ARG
    assert R.dispatch(g, 300).code == R.BAD_ARG and R.dispatch(g, 3000).code == R.BAD_ARG and R.dispatch(g, 20000).code == R.BAD_ARG
    assert R.dispatch(R.fwd(2, 8, 8, 32, 64, 3, 1, 1)).code == R.UNSUPPORTED
    assert R.dispatch(R.dgrad(2, 8, 8, 64, 64, 3, 2, 1), stats=True).code == R.BAD_ARG


@pytest.mark.parametrize("c", SMALL, ids=[c.id for c in SMALL])
def test_fp32_in_two_summation_orders_equals_the_fp64_reference(c):
    for fam in _fams(c):
        inp = R.conv_inputs(c.id, c.g, fam)
        ref = R.conv_ref(c.g, inp.x, inp.w)
        for got in _fp32_orders(c.g, inp.x, inp.w):
            assert torch.equal(got.double(), ref), (c.id, fam)
        if fam == "S":
            stored = R.round_bf16(ref)
            assert torch.equal(stored.double(), ref) and float(ref.abs().max()) <= 4.0, c.id          # none rounded
    if c.g.Kh * c.g.Kw * c.g.Cin >= 576 and c.g.N * c.g.Hout * c.g.Wout * c.g.Cout >= 4096:
        inp = R.conv_inputs(c.id, c.g, "I")
        ref = R.conv_ref(c.g, inp.x, inp.w)
        assert float((R.round_bf16(ref).double() != ref).double().mean()) > 0.1, c.id      # family I does exercise the rounding


def test_the_references_agree_with_torch_in_float64():
    for N, H, W, Ci, Co, k, s, p in ((2, 9, 11, 64, 128, 3, 2, 1), (2, 8, 8, 64, 64, 1, 2, 0), (2, 9, 10, 64, 64, 5, 2, 2),
                                     (2, 7, 9, 128, 64, 3, 1, 1)):
        rng = R._gen("torch", N, H, k, s)
        x = R.dyadic((N, H, W, Ci), 3, 1, rng)
        w = R.dyadic((Co, k, k, Ci), 3, 1, rng)                    # forward weight [Co][kh][kw][Ci]
        gf = R.fwd(N, H, W, Ci, Co, k, s, p)
        want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, s, p).permute(0, 2, 3, 1)
        assert torch.equal(R.conv_ref(gf, x, w), want)
        gd = R.dgrad(N, H, W, Ci, Co, k, s, p)
        dy = R.dyadic((N, gf.Hout, gf.Wout, Co), 3, 1, rng)
        wd = w.flip(1, 2).permute(3, 1, 2, 0).contiguous()         # the dgrad copy [Ci][kh][kw][Co], both taps flipped
        want = conv2d_input((N, Ci, H, W), w.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2), stride=s, padding=p)
        assert torch.equal(R.conv_ref(gd, dy, wd), want.permute(0, 2, 3, 1))
        gw = R.wgrad_geom(N, H, W, Ci, Co, k, s, p)
        want = conv2d_weight(x.double().permute(0, 3, 1, 2), (Co, Ci, k, k), dy.double().permute(0, 3, 1, 2), stride=s, padding=p)
        assert torch.equal(R.wgrad_ref(gw, x, dy), want.permute(0, 2, 3, 1))
        if k == 3 and s == 1:
            assert torch.equal(R.flat_conv3x3(x, w), R.conv_ref(gf, x, w))


@pytest.mark.parametrize("c", WSMALL, ids=[c.id for c in WSMALL])
def test_weight_gradient_in_fp32_equals_the_fp64_reference(c):
    for fam in ("I", "P"):
        inp = R.wgrad_inputs(c.id, c.g, fam)
        ref = inp.dw0.double() + R.wgrad_ref(c.g, inp.x, inp.dy)
        assert torch.equal(ref.float().double(), ref), (c.id, fam)
        g = c.g
        M = g.N * g.Hout * g.Wout
        xd = torch.zeros(g.N, max((g.Hout - 1) * g.stride + g.Kh, g.Hin + g.pad), max((g.Wout - 1) * g.stride + g.Kw, g.Win + g.pad), g.Cin)
        xd[:, g.pad:g.pad + g.Hin, g.pad:g.pad + g.Win] = inp.x
        for order in (range(0, M, 64), range((M - 1) // 64 * 64, -1, -64)):               # 64-pixel slabs, both directions
            acc = inp.dw0.clone()
            for kh in range(g.Kh):
                for kw in range(g.Kw):
                    xs = xd[:, kh:kh + g.stride * (g.Hout - 1) + 1:g.stride, kw:kw + g.stride * (g.Wout - 1) + 1:g.stride].reshape(M, g.Cin)
                    d2 = inp.dy.reshape(M, g.Cout)
                    part = torch.zeros(g.Cout, g.Cin)
                    for a in order:
                        part = part + d2[a:a + 64].t() @ xs[a:a + 64]
                    acc[:, kh, kw] += part
            assert torch.equal(acc.double(), ref), (c.id, fam)


def test_rounding_and_weight_prep_references():
    w = R.prep_master(64, 64, 3, 3)
    bits = R.rne_bits(w)
    assert torch.equal(bits, w.bfloat16().view(torch.int16).to(torch.int32) & 0xFFFF)
    ties = w.view(torch.int32).reshape(-1)[::4]
    assert bool(((ties & 0xFFFF) == 0x8000).all())
    up = (R.rne_bits(w).reshape(-1)[::4] != ((ties >> 16) & 0xFFFF))
    assert 0.3 < float(up.float().mean()) < 0.7                   # ties go both ways: to the even neighbour
    fwd_bits, dg = R.prep_ref(w)
    for o, kh, kw, i in ((0, 0, 0, 0), (5, 1, 2, 7), (63, 2, 0, 63)):
        assert int(dg[i, 2 - kh, 2 - kw, o]) == int(fwd_bits[o, kh, kw, i])


# ------------------------------------------------------------------ the emulated faults
def _differs(a, b):
    return bool((a != b).any())


def test_an_unmasked_border_tap_changes_an_expected_output():
    for cid in ("halo-w63", "halo-c192", "c64-9x33", "c64-tiny-2tiles"):
        c = BY_ID[cid]
        for fam in ("I", "P"):
            inp = R.conv_inputs(c.id, c.g, fam)
            good = R.round_bf16(R.conv_ref(c.g, inp.x, inp.w))
            assert _differs(good, R.flat_conv3x3(inp.x, inp.w, "left-unmasked").float().bfloat16()), (cid, fam)


def test_a_patch_row_shifted_across_a_tile_seam_changes_an_expected_output():
    for cid, tile in (("halo-c192", 256), ("c64-tiny-2tiles", 15), ("halo-w1", 64)):
        c = BY_ID[cid]
        for fam in ("I", "P"):
            inp = R.conv_inputs(c.id, c.g, fam)
            good = R.round_bf16(R.conv_ref(c.g, inp.x, inp.w))
            bad = R.flat_conv3x3(inp.x, inp.w, "seam-shift", tile).float().bfloat16()
            assert _differs(good, bad), (cid, fam)
            first = good.reshape(-1, c.g.Cout)[:tile]
            assert torch.equal(first, bad.reshape(-1, c.g.Cout)[:tile])        # ... and only behind the seam: multi-tile cases see it


def test_a_skipped_last_k_tile_changes_an_expected_output():
    for cid in ("halo-c192", "halo-w63", "c64-9x33"):
        c = BY_ID[cid]
        hit = False
        for fam in ("I", "P"):
            inp = R.conv_inputs(c.id, c.g, fam)
            good = R.round_bf16(R.conv_ref(c.g, inp.x, inp.w))
            hit |= _differs(good, R.flat_conv3x3(inp.x, inp.w, "skip-ktile").float().bfloat16())
        assert hit, cid
    # family P puts a selector into the last K-tile of every layer: tap (Kh - 1, Kw - 1), last channel
    for c in CASES:
        if c.P and c.g.Cout >= c.g.Kh * c.g.Kw:
            w = R.selector_weight(c.g.Cout, c.g.Kh, c.g.Kw, c.g.Cin)
            assert bool((w[:, -1, -1, c.g.Cin - 64:] != 0).any()) and bool((w[:, 0, 0, :64] != 0).any()), c.id


def test_a_parity_class_with_another_class_taps_changes_an_expected_output():
    for cid in ("g-dgrad-3x3s2-odd-co64", "pgemm-3x3s2-dgrad-odd", "g-dgrad-5x5s2"):
        c = BY_ID[cid]
        for fam in ("I", "P"):
            inp = R.conv_inputs(c.id, c.g, fam)
            assert _differs(R.round_bf16(R.conv_ref(c.g, inp.x, inp.w)), R.parity_fault(c.g, inp.x, inp.w).float().bfloat16()), (cid, fam)


def test_two_roundings_and_truncation_change_an_expected_output():
    for cid in ("g-m255", "c64-9x33", "halo-c192", "pgemm-3x3s2-fwd"):
        c = BY_ID[cid]
        inp = R.conv_inputs(c.id, c.g, "I", addend=True)
        conv = R.conv_ref(c.g, inp.x, inp.w)
        good = R.round_bf16(conv + inp.addend.double())
        assert _differs(good, R.two_roundings(conv, inp.addend)), cid
        assert _differs(good, R.truncate_bf16(conv + inp.addend.double())), cid
        plain = R.round_bf16(conv)
        assert _differs(plain, R.truncate_bf16(conv)), cid
        # ties are among the values: exactly half a bf16 ulp, where round-half-up and ties-to-even part
        f = conv.float().contiguous().view(torch.int32)
        assert bool(((f & 0xFFFF) == 0x8000).any()), cid
    inp = R.conv_inputs("g-m255", BY_ID["g-m255"].g, "P", addend=True)
    conv = R.conv_ref(BY_ID["g-m255"].g, inp.x, inp.w)
    assert _differs(R.round_bf16(conv + inp.addend.double()), R.truncate_bf16(conv + inp.addend.double()))


def test_a_packed_image_reading_its_neighbour_changes_an_expected_gradient():
    by = {c.id: c for c in WCASES}
    for cid in ("w-c128b-w7", "w-c128b-w15", "w-c128b-w14-odd", "w-s2-wo7", "w-s2-wo15"):
        c = by[cid]
        for fam in ("I", "P"):
            inp = R.wgrad_inputs(c.id, c.g, fam)
            assert _differs(R.wgrad_ref(c.g, inp.x, inp.dy), R.wgrad_ref(c.g, inp.x, inp.dy, gap_fault=True)), (cid, fam)


def test_a_dropped_split_k_slab_changes_an_expected_gradient():
    by = {c.id: c for c in WCASES}
    for cid in ("w-tap-small-8splits", "w-tap-1x1-33splits", "w-c64-tiny-2tiles"):
        c = by[cid]
        d = R.wgrad_dispatch(c.g, c.runs[0][0])
        M = c.g.N * c.g.Hout * c.g.Wout
        per = d.ktiles_per_split * d.bkp if d.kernel.startswith("wtap") else M // 2
        for a in range(0, M, per):                              # whichever slab is lost
            inp = R.wgrad_inputs(c.id, c.g, "I")
            assert _differs(R.wgrad_ref(c.g, inp.x, inp.dy), R.wgrad_ref(c.g, inp.x, inp.dy, drop=(a, a + per))), (cid, a)
