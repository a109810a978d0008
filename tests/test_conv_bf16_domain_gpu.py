"""The bf16 convolution family of the ResNet-18 patch encoder over its dispatch domains on the MI355X, bit-exactly: every case
pins its kernel through `variant` (include/isic_hip_test.h), asserts ISIC_OK and compares with the fp64 CPU references of
tests/conv_bf16_ref.py -- never with another kernel of the project.  The inputs are chosen so that fp32 accumulation is exact
in any order (tests/test_conv_bf16_ref_cpu.py shows it on the CPU): every output must EQUAL the correctly rounded exact sum,
every fused statistic the fp64 sum of the stored tensor, every weight gradient the fp64 sum.  There is no tolerance in this
module.

Around every call: the output lies between bands of a NaN sentinel pattern and is pre-filled with it (an element the kernel
does not write fails the comparison); the statistics rows lie between two guard rows; the weight-gradient workspace is exactly
isic_conv2d_wgrad_workspace_bytes(...) long between two sentinel bands.  A call that must refuse returns its code and leaves
the output untouched.

Cases per kernel (tests/conv_bf16_ref.py: 43 forward / data-gradient cases and 22 weight-gradient cases; a case runs every
epilogue the dispatch admits -- none, addend, statistics, statistics + addend -- in families I, P and S, the statistics with
stat_slots 1, 32, 256 and 300):
  conv_igemm_kernel<256, 64>    12 pinned: M = 1 and 257, pad 2, 1x3, 3x1, 7x7 pad 3, 2x2 / 2, stride-2 forward, the stride-2 data
                                gradients with odd H and W (5x5 as well), the 1x1 / 2 data gradient whose three tap-less classes
                                write zeros or the addend, Cin and Cout of 64, 128 and 192
  conv_igemm_kernel<256, 128>   6 pinned: M = 255 and 256, pad 0, 5x5 pad 2, an odd data gradient, and W = 64, which leaves conv_halo
  conv3x3_c64_kernel            7: images of 1x1, 8x32, 9x33, 7x31, 257 and 513 images of 3x5, 37 of 56x56; it also serves statistics
                                + addend under the persistent digit
  conv3x3_c64p_kernel           the same 7: 1, 2 and 3 tiles per block
  conv_halo_kernel<.., KPB 1>   13: every halo case through the ten-thousands digit, and the shipped loop at Cin = 64 / 192 and at
                                W = 63 (where the fourth weight stage does not fit); 64 -> 512 with 3 tiles per block; 1338 images
                                of 7x7 at Cout = 128 (257 tiles)
  conv_halo_kernel<.., KPB 2>   3: W = 1, 256 -> 256, 128 -> 512 with 2 tiles per block (+ the masked addend and STATS 2 below)
  conv_pgemm_kernel<128>        8: 3x3 / 2 forward, its data gradient with four classes (even and odd sizes), 1x1 / 2, 1x1 / 1,
                                a forced stride-1 layer, Cout = 512 with 2 (3x3) and 3 (1x1, one K-tile per tile) tiles per block
  conv_pgemm_kernel<64>         2: forward with statistics, the data gradient of a 64 -> 128 layer; + the 64-channel pair gradients
  pair gradient                 4 (64 and 128 channels, even and odd H, W) x variants 0 / 1000 / 2000 and the ABI entry
  masked addend                 5: c64p (1 and 2 tiles per block), conv_halo KPB 2, KPB 1 (Cin = 192; W = 63)
  isic_conv2d_dgrad_bnbwd_bf16  4 x with / without addend: 128 and 192 input channels, W = 63, 2 tiles per block
  wgrad_c64_kernel              4 runs on 3 cases: 1, 2 and 3 tiles per block
  wgrad_c128b_kernel            6: W = 7, 8, 14, 15, 16, 33, odd image counts (a pack partly empty), Cout = 64, 128, 192
  wgrad_s2_kernel               5: Wo = 7, 8, 15, 16 with 1, 2 and 4 pairs; 16 pairs through bit 5
  conv_wgrad_kernel             <true> 15 runs, <false> 5: bit 4 on every all-taps case, 1x1 / 2, 1x1 with 33 splits, 5x5, pad 0, one and
                                eight splits, a stride-2 layer with odd input sizes (which must fall to it)
  weight_prep_kernel            4 shapes (one above 2048 * 256 elements) x (both copies, either one alone)

Pixels per fp32 statistics partial, read from the kernels: conv_igemm and the tile-per-block 64 -> 64 kernel 64 (four threads
per channel, 64 rows each, joined in fp64); the persistent kernels (c64p, conv_halo forward and STATS 2, conv_pgemm) 256 x the
tiles of the block -- a lane keeps its four pixels of every tile, a DPP row adds 16 lanes, the four pixel waves are added in
fp32 before the fp64 row: 768 at three tiles per block, against the 2^14 (no addend) / 2^12 (addend) that family S allows.
Tiles per block reached on the device (256 CUs): c64p 3, conv_halo 3 (KPB 1) and 2 (KPB 2, STATS 2), conv_pgemm 3,
wgrad_c64 3; the module prints them at its end (visible with -s).

Faults found: none -- on the MI355X every kernel passed families I, P and S at the first run (so the premise holds: the MFMA
unit adds exactly where every partial sum is representable), no header sentence was found contradicted.
Of the emulated faults of tests/test_conv_bf16_ref_cpu.py, four were also tried in a scratch build of the kernels on the
device, and this module failed exactly the cases that run the edited kernel: the left border tap not masked in conv_halo
(all 8 halo cases, their statistics, the 3 masked-addend and 4 STATS 2 cases), truncation instead of ties-to-even in
conv3x3_c64p (all 7 c64 cases, family I, and the 2 masked-addend cases), the convolution rounded before the addend joins it
in conv_igemm (all 18 generic cases, at "addend"), the last split-K slab dropped in conv_wgrad (the three cases with more
than one split).  The patch row shifted across a tile seam, the skipped last K-tile, the parity class with another class's
taps and the packed image reading its neighbour rest on the CPU emulation only (an edit of the counted DMA loops can hang a
kernel).

Not expressible through the entry points: a second source together with an addend or statistics, or on a layer other than
3x3 / 2 (isic_conv2d_dgrad_pair_bf16 has no such arguments; conv2d_dispatch's own check is mirrored and CPU-tested)."""
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

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
BAND = 128                                         # sentinel elements before and after every guarded buffer
SENT = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5), torch.uint8: (torch.uint8, 0xA5),
        torch.int16: (torch.int16, 0x7FA5)}
PERSISTENT = ("c64p", "halo-k1", "halo-k2", "pgemm64", "pgemm128", "halo-bnbwd")
REACHED = {}                                       # kernel -> tiles per block reached
COUNT = {}                                         # kernel -> calls compared


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _code(*a):
    """the return code of a call"""
    from isic_hip.lib import IsicHipError
    try:
        _call(*a)
    except IsicHipError as e:
        return e.code
    return R.OK


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(COUNT):
        print(f"{k}: {COUNT[k]} calls compared, up to {REACHED.get(k, 1)} tiles per block")


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    stop_after_a_device_error()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Banded:
    """a device buffer of `shape` between two bands of a sentinel pattern, pre-filled with the pattern (NaN for bf16 and fp32)
    or with `init`"""

    def __init__(self, shape, dtype=BF, init=None):
        n = 1
        for s in shape:
            n *= s
        self.itype, self.sent = SENT[dtype]
        band = self.band = 256 if dtype == torch.uint8 else BAND          # bytes: the body stays 256-byte aligned
        self.buf = torch.empty(2 * band + n, device=DEV, dtype=dtype)
        self.bits = self.buf.view(self.itype)
        self.bits.fill_(self.sent)
        self.n = n
        self.t = self.buf[band:band + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def intact(self):
        return bool((self.bits[:self.band] == self.sent).all()) and bool((self.bits[self.band + self.n:] == self.sent).all())

    def untouched(self):
        return self.intact() and bool((self.bits[self.band:self.band + self.n] == self.sent).all())


class Stats:
    """stat_sum / stat_sumsq [slots][C] fp64, zeroed, each between two guard rows"""

    def __init__(self, slots, C):
        self.buf = torch.zeros(2, slots + 2, C, device=DEV, dtype=torch.float64)
        self.sum, self.sumsq = self.buf[0, 1:slots + 1], self.buf[1, 1:slots + 1]

    def intact(self):
        return not bool(self.buf[:, 0].any()) and not bool(self.buf[:, -1].any())

    def zero(self):
        return not bool(self.buf.any())


def _equal(got, want, what):
    """values with ==: the sign of an exact zero is not pinned, a NaN (an element not written) never passes"""
    if not torch.equal(got, want):
        bad = (got != want) | got.isnan()
        idx = bad.nonzero()[:5].tolist()
        raise AssertionError((what, f"{int(bad.sum())} of {bad.numel()} differ", idx,
                              [(float(got[tuple(i)]), float(want[tuple(i)])) for i in idx]))


def _note(kernel, tpb):
    COUNT[kernel] = COUNT.get(kernel, 0) + 1
    REACHED[kernel] = max(REACHED.get(kernel, 1), tpb)


def _conv_call(v, g, x, w, out, addend=None, s=None, slots=0):
    a = (x, w, out, *R.args(g), addend, s.sum if s else None, s.sumsq if s else None, slots)
    if v == "abi":
        return _code("isic_conv2d_igemm_bf16", *a)
    return _code("isic_test_conv2d_igemm_variant_bf16", *a, v)


def _runs(c):
    return list(c.runs) + ([(0, None, None), ("abi", None, None)] if c.abi else [])


CASES = R.conv_cases()


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_outputs_equal_the_rounded_exact_sum_on_the_pinned_kernel(c):
    cus = _cus()
    c = {k.id: k for k in R.conv_cases(cus)}[c.id]              # the N of a multi-tile case follows the device's CU count
    g = c.g
    for fam in ("I", "P") if c.P else ("I",):
        inp = R.conv_inputs(c.id, g, fam, addend=True)
        conv = R.conv_ref(g, inp.x, inp.w)
        x, w, addend = inp.x.to(DEV, BF), inp.w.to(DEV, BF), inp.addend.to(DEV, BF)
        for add in (False, True) if "add" in c.epi else (False,):
            want = R.round_bf16(conv + inp.addend.double() if add else conv).to(DEV)
            for v, kernel, tpb in _runs(c):
                d = R.dispatch(g, 0 if v == "abi" else v, addend=add, cus=cus)
                assert d.code == R.OK and (kernel is None or d.kernel == kernel) and (tpb is None or d.tiles_per_block == tpb), (c.id, v, d)
                out = Banded((g.N, g.Hout, g.Wout, g.Cout))
                rc = _conv_call(v, g, x, w, out.t, addend if add else None)
                assert rc == R.OK, (c.id, fam, v, "returned", rc)
                assert out.intact(), (c.id, fam, v, "a band around the output was written")
                _equal(out.t, want, (c.id, fam, "addend" if add else "plain", "variant", v, d.kernel))
                _note(d.kernel, d.tiles_per_block)


STAT_CASES = [c for c in CASES if "stats" in c.epi]


@pytest.mark.parametrize("c", STAT_CASES, ids=[c.id for c in STAT_CASES])
def test_fused_statistics_equal_the_fp64_sums_of_the_stored_tensor(c):
    cus = _cus()
    c = {k.id: k for k in R.conv_cases(cus)}[c.id]
    g = c.g
    inp = R.conv_inputs(c.id, g, "S", addend=True)
    conv = R.conv_ref(g, inp.x, inp.w)
    x, w, addend = inp.x.to(DEV, BF), inp.w.to(DEV, BF), inp.addend.to(DEV, BF)
    for add in (False, True) if "stats+add" in c.epi else (False,):
        exact = conv + inp.addend.double() if add else conv
        stored = R.round_bf16(exact)
        assert torch.equal(stored.double(), exact) and float(exact.abs().max()) <= (8.0 if add else 4.0)      # bf16-exact
        s_ref, q_ref = (t.to(DEV) for t in R.stats_ref(stored))
        want = stored.to(DEV)
        for v, _, _ in _runs(c):
            d = R.dispatch(g, 0 if v == "abi" else v, addend=add, stats=True, cus=cus)
            assert d.code == R.OK, (c.id, v, d)
            px = R.PIXELS_PER_PARTIAL[d.kernel] * d.tiles_per_block          # pixels one fp32 partial covers in this kernel
            assert R.stats_condition(px, 8.0 if add else 4.0, 3), (c.id, d.kernel, px)
            for slots in R.SLOTS:
                rows = []
                for rep in range(2 if slots >= 256 and d.kernel in PERSISTENT else 1):
                    out, s = Banded((g.N, g.Hout, g.Wout, g.Cout)), Stats(slots, g.Cout)
                    rc = _conv_call(v, g, x, w, out.t, addend if add else None, s, slots)
                    assert rc == R.OK and out.intact() and s.intact(), (c.id, v, slots, rc)
                    _equal(out.t, want, (c.id, "S", "addend" if add else "plain", "variant", v, d.kernel, "slots", slots))
                    _equal(s.sum.sum(0), s_ref, (c.id, "sum", "variant", v, d.kernel, "slots", slots, "px", px))
                    _equal(s.sumsq.sum(0), q_ref, (c.id, "sum of squares", "variant", v, d.kernel, "slots", slots, "px", px))
                    rows.append(s.buf.clone())
                if len(rows) == 2:                                 # every block owns its row: bit-reproducible, row for row
                    assert torch.equal(rows[0], rows[1]), (c.id, v, d.kernel, slots)
                    assert int((rows[0][0] != 0).any(1).sum()) <= d.blocks, (c.id, v, d.kernel, slots)
            _note(d.kernel + " statistics", d.tiles_per_block)


PAIRS = R.pair_cases()


@pytest.mark.parametrize("c", PAIRS, ids=[c.id for c in PAIRS])
def test_pair_gradient_equals_the_fp64_sum_of_the_two_transposed_convolutions(c):
    cus = _cus()
    g, g1 = c.g, c.g1
    shape = (g.N, g.Hin, g.Win, g.Cin, g.Hout, g.Wout, g.Cout)             # N, Ho, Wo, Co, H, W, C
    for fam in ("I", "P"):
        inp = R.conv_inputs(c.id, g, fam, pair=True)
        want = R.round_bf16(R.conv_ref(g, inp.x, inp.w) + R.conv_ref(g1, inp.x2, inp.w2)).to(DEV)
        dy, w, dy2, w2 = (t.to(DEV, BF) for t in (inp.x, inp.w, inp.x2, inp.w2))
        for v, kernel in c.runs:
            d = R.dispatch(g, v, pair=True, cus=cus)
            assert (d.code, d.kernel) == (R.OK, kernel), (c.id, v, d)
            for entry in ("isic_conv2d_dgrad_pair_bf16", "isic_test_conv2d_dgrad_pair_variant_bf16") if v == 0 else \
                    ("isic_test_conv2d_dgrad_pair_variant_bf16",):
                out = Banded((g.N, g.Hout, g.Wout, g.Cout))
                tail = () if entry == "isic_conv2d_dgrad_pair_bf16" else (v,)
                rc = _code(entry, dy, w, dy2, w2, out.t, *shape, *tail)
                assert rc == R.OK and out.intact(), (c.id, fam, v, rc)
                _equal(out.t, want, (c.id, fam, "variant", v, kernel))
                _note(kernel + " pair", d.tiles_per_block)
    out = Banded((g.N, g.Hout, g.Wout, g.Cout))
    for bad in (5, 3000, 300, 20000):
        assert _code("isic_test_conv2d_dgrad_pair_variant_bf16", dy, w, dy2, w2, out.t, *shape, bad) == R.BAD_ARG, bad
    assert _code("isic_test_conv2d_dgrad_pair_variant_bf16", dy, w, None, w2, out.t, *shape, 0) == R.BAD_ARG
    assert _code("isic_conv2d_dgrad_pair_bf16", dy, w, dy2, None, out.t, *shape) == R.BAD_ARG
    assert out.untouched()


MASKS = R.maskadd_cases()


@pytest.mark.parametrize("c", MASKS, ids=[c.id for c in MASKS])
def test_masked_addend_equals_conv_plus_the_addend_where_its_bit_is_set(c):
    cus = _cus()
    c = {k.id: k for k in R.maskadd_cases(cus)}[c.id]
    g = c.g
    d = R.dispatch(g, 0, addend=True, mask=True, cus=cus)
    assert (d.code, d.kernel) == (R.OK, c.kernel), (c.id, d)
    assert _call("isic_conv2d_maskadd_supported", *R.args(g)) == 1
    for fam in ("I", "P"):
        inp = R.conv_inputs(c.id, g, fam, addend=True)
        bits = torch.rand(inp.addend.shape, generator=R._gen(c.id, "bits")) > 0.4
        exact = R.conv_ref(g, inp.x, inp.w) + torch.where(bits, inp.addend.double(), torch.zeros((), dtype=R.F64))
        want = R.round_bf16(exact).to(DEV)
        out = Banded((g.N, g.Hout, g.Wout, g.Cout))
        rc = _code("isic_conv2d_igemm_maskadd_bf16", inp.x.to(DEV, BF), inp.w.to(DEV, BF), out.t, *R.args(g), inp.addend.to(DEV, BF),
                   R.pack_mask(bits).to(DEV))
        assert rc == R.OK and out.intact(), (c.id, fam, rc)
        _equal(out.t, want, (c.id, fam, c.kernel))
        _note(c.kernel + " masked addend", d.tiles_per_block)


def test_supported_queries_agree_with_the_mirror_and_unsupported_shapes_are_refused():
    for g in R.SUPPORT_PROBES:
        assert _call("isic_conv2d_maskadd_supported", *R.args(g)) == R.maskadd_supported(g), g
        assert _call("isic_conv2d_dgrad_bnbwd_supported", *R.args(g)) == R.bnbwd_supported(g), g
        if g.Cin >= 128 and R.same3x3(g):
            assert R.maskadd_supported(g) == R.bnbwd_supported(g) == int(R.halo_supported(g.N, g.Hin, g.Win, g.Cin, g.Cout)), g
        M = g.N * g.Hout * g.Wout
        x = torch.zeros(g.N, g.Hin, g.Win, g.Cin, device=DEV, dtype=BF)
        w = torch.zeros(g.Cout, g.Kh, g.Kw, g.Cin, device=DEV, dtype=BF)
        add = torch.zeros(M, g.Cout, device=DEV, dtype=BF)
        mask = torch.zeros(M, g.Cout // 8, device=DEV, dtype=torch.uint8)
        out = Banded((M, g.Cout))
        if not R.maskadd_supported(g):                              # a masked addend where no staged-once kernel runs
            assert _code("isic_conv2d_igemm_maskadd_bf16", x, w, out.t, *R.args(g), add, mask) == R.UNSUPPORTED, g
        if not R.bnbwd_supported(g):
            s = Stats(32, g.Cout)
            assert _code("isic_conv2d_dgrad_bnbwd_bf16", x, w, out.t, *R.args(g), None, mask, add, s.sum, s.sumsq, 32) == R.UNSUPPORTED, g
            assert s.zero()
        assert out.untouched(), g


BNBWD = R.bnbwd_cases()


@pytest.mark.parametrize("c", BNBWD, ids=[c.id for c in BNBWD])
def test_dgrad_bnbwd_stores_the_masked_gradient_and_exact_sums(c):
    cus = _cus()
    c = {k.id: k for k in R.bnbwd_cases(cus)}[c.id]
    g = c.g
    plan = R.halo_plan(g.N, g.Hin, g.Win, g.Cin, g.Cout, 0, cus)
    assert plan.tiles_per_block == c.tpb and _call("isic_conv2d_dgrad_bnbwd_supported", *R.args(g)) == 1
    px = R.PIXELS_PER_PARTIAL["halo-bnbwd"] * plan.tiles_per_block
    assert R.stats_condition(px, 8.0, 3) and px * 8.0 * 2.0 * 2 ** 5 < 2 ** 24       # dz y: multiples of 1/32 of magnitude <= 16
    inp = R.conv_inputs(c.id, g, "S", addend=True)
    rng = R._gen(c.id, "bnbwd")
    y = R.dyadic(inp.addend.shape, 2, 2, rng)
    bits = torch.rand(inp.addend.shape, generator=rng) > 0.4
    conv = R.conv_ref(g, inp.x, inp.w)
    x, w, addend, yd, mask = inp.x.to(DEV, BF), inp.w.to(DEV, BF), inp.addend.to(DEV, BF), y.to(DEV, BF), R.pack_mask(bits).to(DEV)
    for add in (False, True):
        exact = torch.where(bits, conv + inp.addend.double() if add else conv, torch.zeros((), dtype=R.F64))
        dz = R.round_bf16(exact)
        assert torch.equal(dz.double(), exact)
        s_ref = dz.double().reshape(-1, g.Cout).sum(0).to(DEV)
        q_ref = (dz.double() * y.double()).reshape(-1, g.Cout).sum(0).to(DEV)
        want = dz.to(DEV)
        for slots in R.SLOTS:
            rows = []
            for rep in range(2 if slots >= 256 else 1):
                out, s = Banded((g.N, g.Hout, g.Wout, g.Cout)), Stats(slots, g.Cout)
                rc = _code("isic_conv2d_dgrad_bnbwd_bf16", x, w, out.t, *R.args(g), addend if add else None, mask, yd, s.sum, s.sumsq, slots)
                assert rc == R.OK and out.intact() and s.intact(), (c.id, add, slots, rc)
                _equal(out.t, want, (c.id, "dz", "addend" if add else "plain", "slots", slots))
                _equal(s.sum.sum(0), s_ref, (c.id, "sum dz", add, "slots", slots, "px", px))
                _equal(s.sumsq.sum(0), q_ref, (c.id, "sum dz y", add, "slots", slots, "px", px))
                rows.append(s.buf.clone())
            if len(rows) == 2:
                assert torch.equal(rows[0], rows[1]), (c.id, add, slots)
        _note("halo-bnbwd", plan.tiles_per_block)


WCASES = R.wgrad_cases()


@pytest.mark.parametrize("c", WCASES, ids=[c.id for c in WCASES])
def test_weight_gradient_equals_the_fp64_sum(c):
    cus = _cus()
    c = {k.id: k for k in R.wgrad_cases(cus)}[c.id]
    g = c.g
    geo = (g.N, g.Hin, g.Win, g.Cin, g.Hout, g.Wout, g.Cout, g.Kh, g.Kw, g.stride, g.pad)
    nbytes = _call("isic_conv2d_wgrad_workspace_bytes", g.N, g.Cin, g.Hout, g.Wout, g.Cout, g.Kh, g.Kw)
    assert nbytes == R.wgrad_workspace_bytes(g, cus), (c.id, nbytes)
    for fam in ("I", "P"):
        inp = R.wgrad_inputs(c.id, g, fam)
        exact = inp.dw0.double() + R.wgrad_ref(g, inp.x, inp.dy)
        want = exact.float()
        assert torch.equal(want.double(), exact)
        want = want.to(DEV)
        x, dy, dw0 = inp.x.to(DEV, BF), inp.dy.to(DEV, BF), inp.dw0.to(DEV)
        for v, kernel, tpb in c.runs:
            d = R.wgrad_dispatch(g, v, cus)
            assert (d.code, d.kernel) == (R.OK, kernel) and (tpb is None or d.tiles_per_block == tpb) and d.need <= nbytes, (c.id, v, d)
            for entry in ("isic_conv2d_wgrad_bf16", "isic_test_conv2d_wgrad_variant_bf16") if v == 0 else ("isic_test_conv2d_wgrad_variant_bf16",):
                tail = () if entry == "isic_conv2d_wgrad_bf16" else (v,)
                dw, ws = Banded(tuple(dw0.shape), torch.float32, dw0), Banded((nbytes,), torch.uint8)
                rc = _code(entry, x, dy, dw.t, *geo, ws.t, nbytes, *tail)
                assert rc == R.OK, (c.id, fam, v, rc)
                assert dw.intact() and ws.intact(), (c.id, fam, v, "a band around dw or the workspace was written")
                _equal(dw.t, want, (c.id, fam, "variant", v, kernel))
                _note(kernel, d.tiles_per_block)
            # one byte less than the kernel that runs needs: refused, the running gradient untouched
            dw, ws = Banded(tuple(dw0.shape), torch.float32, dw0), Banded((nbytes,), torch.uint8)
            assert _code("isic_test_conv2d_wgrad_variant_bf16", x, dy, dw.t, *geo, ws.t, d.need - 1, v) == R.WORKSPACE, (c.id, v, d.need)
            assert dw.intact() and ws.untouched() and torch.equal(dw.t, dw0), (c.id, v)
    dw, ws = Banded(tuple(dw0.shape), torch.float32, dw0), Banded((nbytes,), torch.uint8)
    for bad in (1, 8, 64, 17):
        assert _code("isic_test_conv2d_wgrad_variant_bf16", x, dy, dw.t, *geo, ws.t, nbytes, bad) == R.BAD_ARG, bad
    assert ws.untouched() and torch.equal(dw.t, dw0)


def test_weight_gradient_refuses_channel_counts_that_are_no_multiple_of_64():
    for Ci, Co in ((32, 64), (64, 96)):
        g = R.wgrad_geom(2, 6, 6, Ci, Co, 3, 1, 1)
        x, dy = torch.zeros(2, 6, 6, Ci, device=DEV, dtype=BF), torch.zeros(2, 6, 6, Co, device=DEV, dtype=BF)
        dw, ws = Banded((Co, 3, 3, Ci), torch.float32), Banded((1 << 20,), torch.uint8)
        rc = _code("isic_conv2d_wgrad_bf16", x, dy, dw.t, g.N, g.Hin, g.Win, Ci, g.Hout, g.Wout, Co, 3, 3, 1, 1, ws.t, 1 << 20)
        assert rc == R.UNSUPPORTED and dw.untouched() and ws.untouched(), (Ci, Co, rc)


@pytest.mark.parametrize("shape", R.PREP_CASES, ids=["x".join(map(str, s)) for s in R.PREP_CASES])
def test_weight_prep_rounds_to_nearest_even_into_both_layouts(shape):
    O, I, Kh, Kw = shape
    w = R.prep_master(O, I, Kh, Kw)
    f_ref, d_ref = (t.to(torch.int16).to(DEV) for t in R.prep_ref(w))       # bit patterns (wrapped into int16)
    wd = w.to(DEV)
    for want_f, want_d in ((True, True), (True, False), (False, True)):
        f, d = Banded((O, Kh, Kw, I), torch.int16), Banded((I, Kh, Kw, O), torch.int16)
        rc = _code("isic_conv_weight_prep_bf16", wd, f.t if want_f else None, d.t if want_d else None, O, I, Kh, Kw)
        assert rc == R.OK and f.intact() and d.intact(), (shape, rc)
        assert torch.equal(f.t, f_ref) if want_f else f.untouched(), (shape, "forward copy")
        assert torch.equal(d.t, d_ref) if want_d else d.untouched(), (shape, "dgrad copy")
    assert _code("isic_conv_weight_prep_bf16", wd, None, None, O, I, Kh, Kw) == R.BAD_ARG


def test_refusals_of_the_convolution_dispatch_leave_the_output_untouched():
    def probe(g, code, variant=0, stats=(True, True), slots=32, use_stats=False, what=""):
        x = torch.zeros(g.N, g.Hin, g.Win, g.Cin, device=DEV, dtype=BF)
        w = torch.zeros(g.Cout, g.Kh, g.Kw, g.Cin, device=DEV, dtype=BF)
        out, s = Banded((g.N, g.Hout, g.Wout, g.Cout)), Stats(max(slots, 1), g.Cout)
        a = (x, w, out.t, *R.args(g), None, s.sum if use_stats and stats[0] else None, s.sumsq if use_stats and stats[1] else None,
             slots if use_stats else 0)
        assert _code("isic_test_conv2d_igemm_variant_bf16", *a, variant) == code, (what, g, variant)
        if variant == 0:
            assert _code("isic_conv2d_igemm_bf16", *a) == code, (what, g)
        assert out.untouched() and s.zero(), (what, g, variant)
        if not use_stats:
            assert R.dispatch(g, variant).code == code, (what, "mirror")
    base = R.fwd(2, 8, 8, 64, 64, 3, 1, 1)
    probe(R.fwd(2, 8, 8, 32, 64, 3, 1, 1), R.UNSUPPORTED, what="Cin % 64")
    probe(R.fwd(2, 8, 8, 64, 96, 3, 1, 1), R.UNSUPPORTED, what="Cout % 64")
    probe(R.fwd(2, 8, 8, 96, 128, 3, 1, 1), R.UNSUPPORTED, 200, what="Cin % 64 on the halo digit")
    probe(R.geom(2, 8, 8, 64, 8, 8, 64, 3, 3, 1, 3, 1), R.BAD_ARG, what="down = 3")
    for v in (5, 1, 40, 90, 300, 3000, 20000, 10000, 10030, -10):
        probe(base, R.BAD_ARG, v, what="variant digit")
    probe(R.fwd(2, 8, 8, 128, 128, 3, 1, 1), R.BAD_ARG, 3100, what="variant digit on a halo layer")
    dg = R.dgrad(2, 8, 8, 64, 128, 3, 2, 1)
    probe(dg, R.BAD_ARG, use_stats=True, what="statistics with down = 2")
    for g in (base, R.fwd(2, 8, 8, 128, 128, 3, 1, 1), R.fwd(2, 8, 8, 64, 128, 3, 2, 1), R.fwd(2, 8, 8, 64, 64, 5, 1, 2)):
        probe(g, R.BAD_ARG, stats=(True, False), use_stats=True, what="stat_sumsq NULL")
        probe(g, R.BAD_ARG, stats=(False, True), use_stats=True, what="stat_sum NULL")
        probe(g, R.BAD_ARG, slots=0, use_stats=True, what="stat_slots = 0")
