"""The method of tests/gemm_f32_ref.py is sound, shown on the CPU: for its inputs an fp32 evaluation in ANY order equals the
fp64 reference bit for bit (so a device mismatch is a device error), the emulated wrong kernels each change at least one output
of the family that targets them, the generators meet their stated conditions, and the case table covers every kernel
instantiation that tests/test_gemm_f32_domain_gpu.py lists."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_f32_ref as R  # noqa: E402

F32 = np.float32
# a sample of the table: every kernel, every epilogue, split and unsplit, short and long K (sized for a numpy loop over k)
SAMPLE = ("v1-NN-3x5x7-plain-beta1.0", "v1-TN-65x130x33-plain-beta0.5", "v1-NT-130x67x250-plain-beta0.5",
          "v1-split-NN-100x70x1000-wsfull-beta0.5", "v1-split-TN-128x200x20000-wsnone-beta1.0", "v3-64x64x4097", "v3-64x64x4292",
          "v2-split-NT-260x516x4100-relu-beta-2.0", "v4-K128-N192-M4109-T-beta0.0-e11-add1", "v4-K128-N192-M4109-T-beta0.0-e12-add0",
          "v4-K48-N128-M4099-N-beta0.5-e11-add1")


def _ordered(A, B, order):
    """sum over k in `order` of A[:, k] B[k, :], every product and every add rounded to fp32"""
    acc = np.zeros((A.shape[0], B.shape[1]), F32)
    for k in order:
        acc += A[:, k:k + 1] * B[k:k + 1, :]
    return acc


def _chunked(A, B, parts, reverse):
    K = A.shape[1]
    sums = [_ordered(A, B, range(i * K // parts, (i + 1) * K // parts)) for i in range(parts)]
    acc = np.zeros_like(sums[0])
    for s in (reversed(sums) if reverse else sums):
        acc += s
    return acc


def _pairwise(A, B, lo, hi):
    if hi - lo <= 8:
        return _ordered(A, B, range(lo, hi))
    mid = (lo + hi) // 2
    return _pairwise(A, B, lo, mid) + _pairwise(A, B, mid, hi)


def _orders(A, B):
    K = A.shape[1]
    rng = np.random.default_rng(K)
    yield "forward", _ordered(A, B, range(K))
    yield "reversed", _ordered(A, B, range(K - 1, -1, -1))
    yield "permuted", _ordered(A, B, rng.permutation(K))
    for parts in (7, 64):
        for rev in (False, True):
            yield f"chunked{parts}{'r' if rev else ''}", _chunked(A, B, min(parts, K), rev)
    yield "pairwise", _pairwise(A, B, 0, K)


def _epilogue32(c, inp, pre32):
    """the kernels' epilogue in fp32: act(pre + bias) + beta C0 + addend (tanh cases are held to TANH_BOUND, not here)"""
    v = pre32 + (inp.bias.numpy() if inp.bias is not None else F32(0))
    if c.act == R.ACT_RELU:
        v = np.maximum(v, F32(0))
    if c.beta != 0.0:
        v = v + F32(c.beta) * inp.C0.numpy()
    if inp.addend is not None:
        v = v + inp.addend.numpy()
    return v.astype(F32)


def _slim(c, rows=96):
    """the case with at most `rows` output rows (the order argument is per output element; the k range is kept whole)"""
    return R.Box(c, M=min(c.M, rows))


@pytest.mark.parametrize("cid", SAMPLE)
def test_family_I_is_exact_in_fp32_in_any_order(cid):
    c = _slim(R.BY_ID[cid])
    inp = R.inputs(c, "I")
    ref = R.reference(c, inp)
    assert R.exact_in_fp32(ref.pre) and float(ref.pre.abs().max()) <= c.K + 16
    A, B = inp.opA.numpy(), inp.opB.numpy()
    want_pre = (ref.pre - (inp.bias.to(R.F64) if inp.bias is not None else 0)).float().numpy()
    for name, got in _orders(A, B):
        assert got.dtype == F32 and np.array_equal(got, want_pre), (cid, name)
        if c.act != R.ACT_TANH:
            assert R.exact_in_fp32(ref.out)
            assert np.array_equal(_epilogue32(c, inp, got), ref.out.float().numpy()), (cid, name)


@pytest.mark.parametrize("cid", [s for s in SAMPLE if R.BY_ID[s].K <= 5000])
@pytest.mark.parametrize("family", ("PA", "PB"))
def test_family_P_is_exact_in_fp32_in_any_order(cid, family):
    c = _slim(R.family_p_case(R.BY_ID[cid]))
    inp = R.inputs(c, family)
    ref = R.reference(c, inp)
    assert R.exact_in_fp32(ref.out)
    # the closed form: one term per output, a power of two times an operand entry
    m, n = torch.arange(c.M), torch.arange(c.N)
    if family == "PA":
        closed = inp.opA[:, inp.ks] * inp.opB[inp.ks, n]
    else:
        closed = inp.opA[m, inp.ks].unsqueeze(1) * inp.opB[inp.ks, :]
    assert torch.equal(closed, ref.out.float())
    for name, got in _orders(inp.opA.numpy(), inp.opB.numpy()):
        assert np.array_equal(got, ref.out.float().numpy()), (cid, family, name)


def _differs(wrong, ref):
    return bool((torch.as_tensor(wrong).to(R.F64) != ref).any())


def test_wrong_kernels_change_an_output():
    # the last K % 4 rows dropped / the last row counted twice (a clamped row not zeroed): the A^T B kernel's k tail
    c = R.BY_ID["v3-64x64x4099"]
    inp = R.inputs(c, "I")
    ref = R.reference(c, inp)
    A, B, C0 = inp.opA.to(R.F64), inp.opB.to(R.F64), inp.C0.to(R.F64)
    tail = c.K % 4
    assert tail and _differs(A[:, :-tail] @ B[:-tail] + c.beta * C0, ref.out)
    assert _differs(A @ B + A[:, -1:] @ B[-1:] + c.beta * C0, ref.out)
    for fam in ("PA", "PB"):                                 # ... family P has selectors in the tail rows themselves
        cp = R.family_p_case(c)
        ip = R.inputs(cp, fam)
        assert _differs(ip.opA[:, :-tail].to(R.F64) @ ip.opB[:-tail].to(R.F64), R.reference(cp, ip).out)
    # one K-tile of a split skipped
    c = R.BY_ID["v2-split-NT-260x516x4100-relu-beta0.5"]
    inp = R.inputs(c, "I")
    ref = R.reference(c, inp)
    A, B = inp.opA.to(R.F64), inp.opB.to(R.F64)
    k0 = 32 * R.g32_plan(c.ta, c.tb, c.M, c.N, c.K).kt_per_split
    keep = torch.ones(c.K, dtype=torch.bool)
    keep[k0:k0 + 32] = False
    assert _differs(torch.relu(A[:, keep] @ B[keep] + inp.bias.to(R.F64)) + c.beta * inp.C0.to(R.F64), ref.out)
    cp = R.family_p_case(c)
    ip = R.inputs(cp, "PA")
    assert _differs(ip.opA[:, keep].to(R.F64) @ ip.opB[keep].to(R.F64), R.reference(cp, ip).out)
    # beta applied before the activation
    assert _differs(torch.relu(ref.pre + c.beta * inp.C0.to(R.F64)), ref.out)
    # the bias indexed by row in a swapped product
    c = R.BY_ID["v2-swap-TN-128x772x8200-bias"]
    assert R.g32_plan(c.ta, c.tb, c.M, c.N, c.K).swap
    inp = R.inputs(c, "I")
    ref = R.reference(c, inp)
    by_row = ref.pre - inp.bias.to(R.F64) + inp.bias.to(R.F64)[:c.M].unsqueeze(1)
    assert _differs(torch.relu(by_row), ref.out)


def _round_mantissa(t, bits):
    """fp32 rounded to `bits` explicit mantissa bits (round to nearest even): 7 = bf16, 10 = a 19-bit tf32-like format"""
    i = t.contiguous().numpy().view(np.uint32).astype(np.uint64)
    drop = 23 - bits
    i = ((i + np.uint64((1 << (drop - 1)) - 1) + ((i >> np.uint64(drop)) & np.uint64(1))) >> np.uint64(drop)) << np.uint64(drop)
    return torch.from_numpy(i.astype(np.uint32).view(np.float32).copy())


@pytest.mark.parametrize("bits", (7, 10))
@pytest.mark.parametrize("family", ("PA", "PB"))
def test_a_rounded_operand_changes_family_P(bits, family):
    c = R.family_p_case(R.BY_ID["v4-K128-N192-M4109-T-beta0.0-e12-add0"])
    inp = R.inputs(c, family)
    ref = R.reference(c, inp)
    full = "opA" if family == "PA" else "opB"
    rounded = _round_mantissa(inp[full], bits)
    assert float((rounded != inp[full]).float().mean()) > 0.99       # full-mantissa values: nearly every entry loses bits
    wrong = R.reference(c, R.Box(inp, **{full: rounded}))
    changed = float((wrong.out != ref.out).double().mean())
    assert changed > 0.99, changed                                   # ... and so does nearly every output


def _isic_tanhf(x):
    """csrc/common.h's isic_tanhf evaluated in numpy fp32 (exp through fp32 exp2 of the rounded product, as v_exp_f32 is fed)"""
    x = x.astype(F32)
    ax = np.abs(x)
    x2 = x * x
    poly = x * (F32(1) + x2 * (F32(-0.33333334) + x2 * (F32(0.13333334) + x2 * (F32(-0.053968254) + x2 * F32(0.021869488)))))
    with np.errstate(over="ignore"):
        e = np.exp2((F32(2) * ax) * F32(1.4426950408889634)).astype(F32)
        big = np.copysign(F32(1) - F32(2) / (e + F32(1)), x)
    return np.where(ax < F32(0.25), poly, big).astype(F32)


TANH_CASES = [c for c in R.CASES if c.act == R.ACT_TANH]


def test_tanh_bound_admits_fp32_and_rejects_a_clamp():
    assert R.TANH_BOUND == 1.5e-7 + 2.0 ** -25
    c = R.BY_ID["v2-split-NT-260x516x4100-tanh"]
    inp = R.inputs(c, "I")
    ref = R.reference(c, inp)
    got = torch.from_numpy(_isic_tanhf(ref.pre.float().numpy()))
    err, sat_ok, zero_ok = R.tanh_error(got, ref)
    assert err <= R.TANH_BOUND and sat_ok and zero_ok, err
    clamp, _, _ = R.tanh_error(ref.pre.clamp(-1, 1).float(), ref)
    assert clamp > 1000 * R.TANH_BOUND
    # a tanh off by 4 ulp of 0.5 .. 1 is outside the bound
    off, _, _ = R.tanh_error(got + got.sign() * 2.0 ** -22, ref)
    assert off > R.TANH_BOUND


@pytest.mark.parametrize("c", TANH_CASES, ids=[c.id for c in TANH_CASES])
def test_tanh_inputs_are_informative(c):
    assert c.beta == 0.0 and not c.add                     # the tanh bound stands alone: nothing is added afterwards
    inp = R.inputs(c, "I")
    assert int((inp.opB != 0).sum(0).max()) <= 16
    nz = (inp.opB != 0).nonzero()[:, 0]
    if c.K >= 64:                                          # spread over the whole k range
        assert int(nz.min()) < c.K // 8 and int(nz.max()) >= c.K - c.K // 8
    p = R.reference(c, inp).pre
    assert R.exact_in_fp32(p) and float(p.abs().max()) <= 9.5
    if c.M * c.N >= 100:
        assert float((p.abs() < 0.25).double().mean()) >= 0.05
    if R.tanh_informative(c):
        assert bool((p == 0).any()) and bool((p >= 9.25).any()) and bool((p <= -9.25).any())


def test_every_kernel_has_an_informative_tanh_case():
    for v in (1, 2, 4):
        assert any(c.variant == v and R.tanh_informative(c) for c in TANH_CASES), v
    assert any("reduce" in (c.inst or "") for c in TANH_CASES)


@pytest.mark.parametrize("c", R.CASES, ids=[c.id for c in R.CASES])
def test_generated_inputs_meet_the_stated_conditions(c):
    assert c.variant in (1, 2, 3, 4) and float(c.M) * c.N * c.K <= R.MAX_MACS
    assert 64 * (c.K + 16) < 2 ** 24 and c.beta in R.BETAS
    inp = R.inputs(c, "I")
    for name, lim in (("opA", 1), ("opB", 1), ("bias", 4), ("C0", 4), ("addend", 4)):
        t = inp[name]
        if t is not None:
            assert bool((t * 8 == (t * 8).round()).all()) and float(t.abs().max()) <= lim, name
    assert (inp.bias is not None) == bool(c.bias) and (inp.addend is not None) == bool(c.add)
    assert tuple(inp.opA.shape) == (c.M, c.K) and tuple(inp.opB.shape) == (c.K, c.N)


P_CASES = [c for c in R.CASES if c.P]


@pytest.mark.parametrize("c", P_CASES, ids=[c.id for c in P_CASES])
def test_selector_inputs_and_placement(c):
    cp = R.family_p_case(c)
    want = R.selector_ks(cp)
    for family, n_out in (("PA", c.N), ("PB", c.M)):
        inp = R.inputs(cp, family)
        sel, full = (inp.opB, inp.opA) if family == "PA" else (inp.opA.t(), inp.opB)
        assert bool(((sel != 0).sum(0) == 1).all())
        assert set(sel[sel != 0].abs().tolist()) <= {0.5, 1.0, 2.0}
        mant = full.contiguous().view(torch.int32) & 0xFF            # full mantissas: the low byte is not constant
        assert len(torch.unique(mant)) > 200 or full.numel() < 4096
        assert bool(torch.isfinite(full).all()) and float(full.abs().max()) < 2.0 ** 24
        ks = set(inp.ks.tolist())
        if n_out >= len(want.ends) + len(want.ring):
            assert set(want.ends) <= ks and set(want.ring) <= ks, (c.id, family)
        if n_out >= len(want.all):                                   # every split / slab / K-tile boundary, both sides
            assert set(want.all) <= ks, (c.id, family)
        else:                                                        # ... or as many as fit: the split boundaries first
            room = n_out - len(want.ends) - len(want.ring)
            assert len(ks & set(want.bounds)) >= min(room, len(want.bounds)), (c.id, family)
            assert len(ks & set(want.bounds + want.tiles)) >= min(room, len(want.bounds) + len(want.tiles)), (c.id, family)


def test_selectors_reach_every_ring_slot_both_k_groups_and_the_last_slab():
    for cid in ("v3-64x64x4097", "v3-64x64x4292", "v3-128x256x9001", "v3-forced-64x2048x5000"):
        c = R.family_p_case(R.BY_ID[cid])
        p = R.tn_plan(c.ta, c.tb, c.M, c.N, c.K, True)
        for family in ("PA", "PB"):
            ks = R.inputs(c, family).ks
            step = ks // 4
            in_slab = step % p.steps_per_slab
            first = step < p.steps_per_slab
            slots = {(int(s) & 1, (int(s) >> 1) % R.TP, int(s) >= 2 * R.TP) for s in in_slab[first]}
            assert len({(g, sl) for g, sl, _ in slots}) == 2 * R.TP, (cid, family)          # every slot of both K-groups
            if p.steps_per_slab > 2 * R.TP:                                                   # ... and a refilled slot
                assert any(again for _, _, again in slots), (cid, family)
            assert bool((step // p.steps_per_slab == p.slabs - 1).any())                      # the last (short) slab
            assert len(set((ks % 4).tolist())) == 4                                           # every row of a k-step
    # a slab with an odd step count, and a K-group with an odd one
    assert R.tn_plan(1, 0, 64, 64, 4097, True).total_steps % R.tn_plan(1, 0, 64, 64, 4097, True).steps_per_slab == 1
    assert R.tn_plan(1, 0, 128, 256, 9001, True).steps_per_slab // 2 % 2 == 1


def test_the_table_pins_the_plans_it_was_derived_from():
    """the hand-derived plans at 256 CUs (the device test asserts ISIC_OK of the pinned variant, whatever the CU count)"""
    for c in R.CASES:
        if c.refuse or c.forced_only:
            continue
        have_ws = c.ws == "full"
        choice = R.shipped_choice(c, have_ws=have_ws)
        if c.variant == 1:
            assert choice == 1, c.id
        elif have_ws:
            assert choice == c.variant, (c.id, choice)
    for cid, shape in R.V2_JUST_OVER.items():
        c = R.BY_ID[cid]
        assert R.g32_plan(c.ta, c.tb, c.M, c.N, c.K).why == c.why, cid
        assert R.g32_plan(c.ta, c.tb, *shape).ok, cid
    assert R.g32_plan(0, 1, 6148, 516, 260).splits == 1 and not R.g32_plan(0, 1, 6148, 516, 260).swap
    p = R.g32_plan(1, 0, 128, 772, 8200)
    assert p.ok and p.swap and p.splits == 29
    p = R.g32_plan(0, 1, 260, 516, 4100)
    assert p.ok and not p.swap and p.splits == 15 and p.kt_per_split == 9
    assert R.small_split_plan(100, 70, 1000, True) == (13, 80) and R.small_split_plan(128, 200, 20000, True) == (74, 272)
    assert 1000 % 80 and 20000 % 272 and 80 % 16 == 0 and 272 % 16 == 0
    for cid, want in (("v3-forced-512x256x4096", 1), ("v3-forced-64x2048x5000", 2)):
        c = R.BY_ID[cid]
        assert R.tn_plan(c.ta, c.tb, c.M, c.N, c.K, True) and R.shipped_choice(c) == want
        assert R.partial_floats(c, 3) != R.partial_floats(c, want)           # the workspace tells the two kernels apart
    assert R.tn_plan(1, 0, 128, 1088, 4096, True) is None
    for c, _ in R.ROWS_FORMS.values():
        assert R.g32_plan(c.ta, c.tb, c.M, c.N, c.K).ok
    assert R.ROWS_SWAP_NT.N % 8 and R.g32_plan(0, 1, 128, 772, 8200).swap
    # the persistent kernel's tile loop: a block walks two row tiles (with and without a gathered index)
    for c in [c for c in R.CASES if "tiles2" in c.id] + [R.ROWS_FWD_TILES2]:
        p = R.g32_plan(c.ta, c.tb, c.M, c.N, c.K)
        assert p.ok and p.splits == 1 and p.tiles_per_block == 2, c.id
    assert len([c for c in R.CASES if "tiles2" in c.id]) == 2
    # the row panel's steady state: a wave multiplies a prefetched unit (more than 8 units per block) in the first slice, on
    # the hand-counted path (beta = 0) and the drained one, with and without the addend
    steady = [c for c in R.CASES if "steady" in c.id]
    assert {(c.beta != 0.0, c.add) for c in steady} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    for c in steady:
        assert R.rp_ok(c.ta, c.M, c.N, c.K) and R.rp_units(c.M, c.N)[0] > 8 and c.M % 16, c.id
    assert any(min(R.rp_units(c.M, c.N)) > 8 and c.N == 192 for c in steady)          # ... and in the 64-wide second slice
    assert any(R.rp_units(c.M, c.N)[0] > 16 for c in steady)                          # a wave's third unit: a prefetch after a prefetch
    assert all(max(R.rp_units(c.M, c.N)) <= 8 for c in R.CASES if c.variant == 4 and "steady" not in c.id)
    assert R.ROWS_FWD.M % 8 and not R.g32_plan(0, 1, 6148, 516, 260).swap
    assert R.ROWS_WGRAD.K % 32 and R.ROWS_WGRAD.K % 8 and R.g32_plan(1, 0, 128, 772, 8204).swap


def test_every_listed_instantiation_has_a_case():
    doc = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gemm_f32_domain_gpu.py")).read().split('"""')[1]
    insts = [c.inst for c in R.CASES if c.inst]
    for name in R.INSTANTIATIONS:
        assert any(name in i for i in insts), name
        listed = name
        if name.startswith("gemm_rowpanel_kernel<"):                 # the docstring lists the eight KC of each ADD on one line
            listed = "gemm_rowpanel_kernel<1..8, " + name.split(", ")[1]
        assert listed in doc, name
    for c in R.CASES:                                      # a case meant for a kernel must say which instantiation it launches
        assert c.inst or c.refuse, c.id
