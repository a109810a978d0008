"""The bounds of tests/f32_kernel_ref.py, checked on the CPU: on every case of the device test's own case lists the same
formula evaluated in plain torch fp32 stays at error / bound <= 1 against the fp64 reference, every deliberately wrong
variant exceeds 1 on at least one of those cases, and the share of ambiguous entries left out of a gradient comparison
stays under the 1 % cap.  This is the evidence that tests/test_f32_kernel_domain_gpu.py would notice those faults."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_kernel_ref as R  # noqa: E402

F32, F64 = R.F32, R.F64


def _assert_within(ratios, what):
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


# ------------------------------------------------------------------ A. LayerNorm
@pytest.fixture(scope="module")
def ln_results():
    """(case, inputs, fp64 reference, forward bounds, backward bounds) of every LayerNorm case, computed once"""
    out = []
    for case in R.LN_CASES:
        inp = R.ln_inputs(case)
        ref = R.ln_eval(inp, F64)
        fb = R.ln_forward_bounds(inp, ref)
        out.append((case, inp, ref, fb, R.ln_backward_bounds(inp, ref, fb)))
    return out


def test_layernorm_fp32_evaluation_is_within_the_bounds(ln_results):
    for case, inp, ref, fb, bb in ln_results:
        assert bb.share <= R.AMBIGUOUS_CAP, (case["id"], bb.share)
        _assert_within(R.ln_ratios(R.ln_eval(inp, F32), ref, fb, bb), case["id"])
        # the documented backward arithmetic in fp64 is the autograd reference
        man = R.ln_eval(inp, F64, bug="none")
        for k in ("dx", "dgamma", "dbeta"):
            scale = float(ref[k].abs().max()) + 1e-30
            if torch.isfinite(fb.rstd).all():
                assert float((man[k] - ref[k]).abs().max()) <= 1e-9 * max(scale, 1.0), (case["id"], k)


@pytest.mark.parametrize("bug", R.LN_BUGS)
def test_layernorm_wrong_variants_exceed_the_bounds(ln_results, bug):
    worst = 0.0
    for case, inp, ref, fb, bb in ln_results:
        if case["M"] > 100:
            continue
        worst = max(worst, max(R.ln_ratios(R.ln_eval(inp, F32, bug=bug), ref, fb, bb).values()))
    assert worst > 1.0, (bug, worst)


def test_layernorm_bound_carries_the_conditioning():
    """a common offset of 1e4 widens the bound of y by orders of magnitude over the random family at the same width"""
    by = {}
    for fam in ("random", "offset"):
        case = next(c for c in R.LN_CASES if c["family"] == fam and c["N"] == 64 and c["M"] == 67 and not c["misalign"])
        inp = R.ln_inputs(case)
        ref = R.ln_eval(inp, F64)
        by[fam] = float(R.ln_forward_bounds(inp, ref).y.median())
    assert by["offset"] > 100 * by["random"] > 0


# ------------------------------------------------------------------ B. attention pool
@pytest.fixture(scope="module")
def pool_results():
    out = []
    for case in R.POOL_CASES:
        inp = R.pool_inputs(case)
        ref = R.pool_eval(inp, F64)
        out.append((case, inp, ref, R.pool_bounds(inp, ref)))
    return out


def test_pool_fp32_evaluation_is_within_the_bounds(pool_results):
    for case, inp, ref, b in pool_results:
        _assert_within(R.pool_ratios(R.pool_eval(inp, F32), ref, b, R.POOL_FWD_KEYS + R.POOL_BWD_KEYS), case["id"])


def test_pool_empty_bags_give_zero_pooled_features_and_uniform_bag_probs(pool_results):
    for case, inp, ref, b in pool_results:
        for bi, n in enumerate(case["bags"]):
            if n == 0:
                assert bool((ref.z[bi] == 0).all()) and bool((ref.psum[bi] == 0).all())
                if case["C"]:
                    assert bool((ref.bl[bi] == 0).all()) and bool((ref.bp[bi] == 1.0 / case["C"]).all())


@pytest.mark.parametrize("bug", R.POOL_BUGS)
def test_pool_wrong_variants_exceed_the_bounds(pool_results, bug):
    worst = 0.0
    for case, inp, ref, b in pool_results:
        worst = max(worst, max(R.pool_ratios(R.pool_eval(inp, F32, bug=bug), ref, b, R.POOL_FWD_KEYS + R.POOL_BWD_KEYS).values()))
    assert worst > 1.0, (bug, worst)


# ------------------------------------------------------------------ C. GAT, GATv2 / TransformerConv, FAConv
@pytest.fixture(scope="module")
def att_results():
    out = []
    for case in R.ATT_CASES:
        inp = R.att_inputs(case)
        ref = R.att_eval(inp, F64)
        out.append((case, inp, ref, R.att_bounds(inp, ref)))
    return out


def test_attention_graph_has_the_rows_the_kernels_branch_on():
    src, dst, w = R.att_graph(R.ATT_N)
    g0, g1 = R.csr_ref(src, dst, w, R.ATT_N, 0), R.csr_ref(src, dst, w, R.ATT_N, 1)
    assert {1, 2, 63, 64, 65, 512, 513, 700} <= set(g0.cnt_in.tolist())
    assert {0, 512, 513, 699} <= set(g1.cnt_in.tolist())
    assert int(g0.cnt_out.max()) >= 700                               # a source row past the 512 edges too
    pairs = list(zip(src.tolist(), dst.tolist()))
    assert len(pairs) > len(set(pairs))                                # duplicated edges
    assert bool((src == dst).any())                                    # self loops in the input


def test_attention_fp32_evaluation_is_within_the_bounds(att_results):
    for case, inp, ref, b in att_results:
        assert R.att_zero_pre_share(inp) <= R.AMBIGUOUS_CAP
        _assert_within(R.att_ratios(R.att_eval(inp, F32), ref, b), case["id"])
    for case, inp, ref, b in att_results:
        if case["layer"] in ("gat", "fa") and case["p"] == 0.0:
            sb, s64, s32 = R.att_scores_bounds(inp), R.att_scores(inp, F64), R.att_scores(inp, F32)
            _assert_within({k: R.ratio(s32[k], s64[k], sb[k]) for k in ("al", "ar")}, case["id"])


@pytest.mark.parametrize("layer,bug", [(layer, bug) for layer in ("gat", "gatv2", "dot", "fa") for bug in R.ATT_BUGS_OF[layer]])
def test_attention_wrong_variants_exceed_the_bounds(att_results, layer, bug):
    worst = 0.0
    for case, inp, ref, b in att_results:
        if case["layer"] == layer and case["p"] > 0 and (case["n"] == 5 or (case["H"], case["F"]) in ((3, 16), (1, 63))):
            worst = max(worst, max(R.att_ratios(R.att_eval(inp, F32, bug=bug), ref, b).values()))
    assert worst > 1.0, (layer, bug, worst)


# ------------------------------------------------------------------ D. SpMM and the CSR
def test_spmm_fp32_evaluation_is_within_the_bounds_and_out_degree_mean_is_rejected():
    worst_bug = 0.0
    for case in R.SPMM_CASES:
        inp = R.spmm_inputs(case)
        ref = R.spmm_eval(inp, F64)
        b = R.spmm_bounds(inp, ref)
        _assert_within({"out": R.ratio(R.spmm_eval(inp, F32).out, ref.out, b.out)}, case["id"])
        worst_bug = max(worst_bug, R.ratio(R.spmm_eval(inp, F32, bug=R.SPMM_BUGS[0]).out, ref.out, b.out))
    assert worst_bug > 1.0


def test_spmm_graph_has_rows_of_0_1_17_and_700_entries():
    case = next(c for c in R.SPMM_CASES if c["n"] == 801 and c["weighted"])
    src, dst, w = R.spmm_graph(case)
    lengths = set()
    for mode in (0, 1, 2):
        g = R.csr_ref(src, dst, w, 801, mode)
        lengths |= set(g.cnt_in.tolist())
        assert g.rowptr[-1] == g.nnz == g.rowptr_t[-1]
        # perm_t maps every transposed slot to the slot of the same edge
        assert bool((g.col[g.perm_t] == g.row_t).all()) and bool((g.row[g.perm_t] == g.col_t).all())
        assert sorted(g.perm_t.tolist()) == list(range(g.nnz))
    assert {0, 1, 17, 700} <= lengths


# ------------------------------------------------------------------ E. the small row-wise entries
def test_l2normalize_bounds():
    worst = 0.0
    for N in R.L2_WIDTHS:
        inp = R.l2_inputs(N)
        ref = R.l2_eval(inp, F64)
        b = R.l2_bounds(inp, ref)
        assert float(ref.norm[0]) == R.L2_EPS and float(ref.norm[1]) == R.L2_EPS and float(ref.norm[2]) > 1e5
        got = R.l2_eval(inp, F32)
        _assert_within({k: R.ratio(got[k], ref[k], b[k]) for k in b}, N)
        worst = max(worst, R.ratio(R.l2_eval(inp, F32, bug=R.L2_BUGS[0]).dx, ref.dx, b.dx))
    assert worst > 1.0


def test_softmax_rows_bounds():
    for M, N in R.SOFTMAX_SHAPES:
        inp = R.softmax_inputs(M, N)
        ref = R.softmax_eval(inp, F64)
        b = R.softmax_bounds(inp, ref)
        got = R.softmax_eval(inp, F32)
        _assert_within({k: R.ratio(got[k], ref[k], b[k]) for k in b}, (M, N))


def test_cross_entropy_bounds():
    worst = {bug: 0.0 for bug in R.CE_BUGS}
    for B, C in R.CE_SHAPES:
        for mode in (0, 1):
            inp = R.ce_inputs(B, C, mode)
            ref = R.ce_eval(inp, F64)
            b = R.ce_bounds(inp, ref)
            got = R.ce_eval(inp, F32)
            _assert_within({k: R.ratio(got[k], ref[k], b[k]) for k in b}, (B, C, mode))
            for bug in R.CE_BUGS:
                bad = R.ce_eval(inp, F32, bug=bug)
                worst[bug] = max(worst[bug], max(R.ratio(bad[k], ref[k], b[k]) for k in b))
    assert all(v > 1.0 for v in worst.values()), worst


def test_relu_dropout_tanh_and_colsum_bounds():
    for n in R.RD_SIZES:
        for p, clock in ((R.RD_P, R.RD_CLOCK), (R.RD_P, None), (0.0, None)):
            inp = R.rd_inputs(n, p, clock)
            ref, got = R.rd_eval(inp, F64), R.rd_eval(inp, F32)
            b = R.rd_bounds(inp, ref)
            _assert_within({k: R.ratio(got[k], ref[k], b[k]) for k in b}, (n, p))
    g = torch.Generator().manual_seed(3)
    dy, t = torch.randn(1025, generator=g), torch.tanh(torch.randn(1025, generator=g) * 2)
    ref = dy.double() * (1 - t.double() ** 2)
    assert R.ratio(dy * (1 - t * t), ref, R.tanh_bwd_bounds(dy, t, ref)) <= 1.0
    for M, N, ldx in R.COLSUM_SHAPES:
        inp = R.colsum_inputs(M, N, ldx)
        for beta in (0.0, 1.0):
            ref = R.colsum_eval(inp, F64, beta)
            assert R.ratio(R.colsum_eval(inp, F32, beta), ref, R.colsum_bounds(inp, ref, beta)) <= 1.0
