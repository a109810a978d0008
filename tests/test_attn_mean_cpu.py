"""CPU-only checks of the head-averaged attention path (``concat=False``): GraphMIL constructs with the narrower shapes,
the four C entries are declared and exported, the bounds of tests/attn_mean_ref.py admit a correct fp32 evaluation and
reject the wrong variants kept there, and the model-level restatement is pinned to oracle/gnn.py at one head."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_mean_ref as A  # noqa: E402
import f32_kernel_ref as R  # noqa: E402
from oracle import formula, gnn  # noqa: E402

F32, F64 = torch.float32, torch.float64
ENTRIES = ("isic_gat_fwd_mean", "isic_gat_bwd_mean", "isic_edge_attn_fwd_mean", "isic_edge_attn_bwd_mean")


@pytest.mark.parametrize("gtype", ("gat", "gatv2", "transformer"))
def test_graphmil_constructs_without_concat_with_the_narrow_shapes(gtype):
    from gnn_models import GraphMIL
    D, F_, L, H = 40, 24, 3, 4
    m = GraphMIL(D, gtype, F_, L, gnn_heads=H, gnn_concat=False, att_dim=16, classifier_dim=24, classifier_light=True)
    want = A.graphmil_mean_shapes(D, dict(gnn_type=gtype, gnn_hidden=F_, gnn_layers=L, gnn_heads=H, att_dim=16, classifier_dim=24))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(want)
    assert m.final_gnn_dim == F_ and want["classifier.0.weight"] == (24, F_)
    assert want[f"gnn_layers.{L - 1}.bias" if gtype != "transformer" else f"gnn_layers.{L - 1}.lin_skip.bias"] == (F_,)
    if gtype == "transformer":
        assert want["gnn_layers.1.lin_beta.weight"] == (1, 3 * F_) and want["gnn_layers.1.lin_key.weight"] == (H * F_, F_)


@pytest.mark.parametrize("gtype", ("gat", "gatv2", "transformer"))
def test_graphmil_concat_shapes_are_the_oracles_as_before(gtype):
    from gnn_models import GraphMIL
    D, F_, L, H = 40, 24, 2, 4
    m = GraphMIL(D, gtype, F_, L, gnn_heads=H, gnn_concat=True, att_dim=16, classifier_dim=24, classifier_light=True)
    want = gnn.graphmil_shapes(D, dict(gnn_type=gtype, gnn_hidden=F_, gnn_layers=L, gnn_heads=H, att_dim=16, classifier_dim=24))
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(want.items())


def test_the_four_mean_entries_are_declared_and_exported():
    from isic_hip import lib
    L = lib.lib()
    inc = os.path.join(R.ROOT, "include")
    declared = lib.parse_header(os.path.join(inc, "isic_hip_attn_mean.h"))
    assert set(declared) == set(ENTRIES)
    assert '#include "isic_hip_attn_mean.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(cdll, name) and name in L.extension and name in L.fn, name
        concat = L.protos[name[:-len("_mean")]]
        assert [a[0] for a in declared[name][1]] == [a[0] for a in concat[1]], name      # same argument list as the concat entry
    assert L.fn["isic_abi_version"]() == 1
    # arguments are checked before any device work: usable without a GPU
    assert L.fn["isic_gat_fwd_mean"](None, None, None, None, None, None, None, None, 4, 0, 8, 0.2, 0, 1.0, 0, 0, None) == -1
    assert L.fn["isic_gat_fwd_mean"](None, None, None, None, None, None, None, None, 0, 2, 8, 0.2, 0, 1.0, 0, 0, None) == 0
    assert L.fn["isic_edge_attn_fwd_mean"](2, None, None, None, None, None, None, None, None, None, 4, 2, 8, 0.2, 1.0, 0, 1.0, 0, 0,
                                           None) == -1


@pytest.fixture(scope="module")
def mean_results():
    out = []
    for case in A.MEAN_CASES:
        inp = A.mean_inputs(case)
        ref, b = A.mean_reference(inp)
        out.append((case, inp, ref, b))
    return out


def test_case_list_reaches_every_branch_of_the_kernels():
    hf = {(c["layer"], c["H"], c["F"]) for c in A.MEAN_CASES}
    for layer in ("gat", "gatv2", "dot"):
        assert {(layer, 1, 1), (layer, 3, 16), (layer, 4, 64), (layer, 2, 65), (layer, 8, 130)} <= hf
    assert {("gatv2", 4, 257), ("gatv2", 6, 168), ("dot", 4, 257), ("dot", 6, 168)} <= hf
    assert any(F <= 256 for _, _, F in hf) and any(F > 256 for _, _, F in hf)            # head sum in registers / in the row
    assert {c["n"] for c in A.MEAN_CASES} == {1, 5, R.ATT_N} and {c["p"] for c in A.MEAN_CASES} == {0.0, R.ATT_P}


def test_fp32_evaluation_is_within_the_bounds(mean_results):
    worst = 0.0
    for case, inp, ref, b in mean_results:
        assert R.att_zero_pre_share(inp) <= R.AMBIGUOUS_CAP
        assert set(b) == {"out", "alpha"} | set(A.GRAD_KEYS[case["layer"]])
        ratios = A.mean_ratios(A.mean_eval(inp, F32), ref, b)
        worst = max(worst, max(ratios.values()))
        assert all(v <= 1.0 for v in ratios.values()), (case["id"], ratios)
    print("worst fp32 ratio", round(worst, 3))


def _small(mean_results, layer):
    cases = [r for r in mean_results if r[0]["layer"] == layer and r[0] in A.SMALL_MULTI_HEAD and r[0]["p"] > 0]
    assert len(cases) == 3                                             # n = 1, 5 and 1100 at H 3, F 16
    return cases


@pytest.mark.parametrize("layer", ("gat", "gatv2", "dot"))
@pytest.mark.parametrize("bug", A.MEAN_BUGS)
def test_wrong_head_mean_variants_exceed_the_bounds_on_every_small_case(mean_results, layer, bug):
    for case, inp, ref, b in _small(mean_results, layer):
        worst = max(A.mean_ratios(A.mean_eval(inp, F32, bug=bug), ref, b).values())
        assert worst > 1.0, (case["id"], bug, worst)


@pytest.mark.parametrize("layer", ("gat", "gatv2", "dot"))
@pytest.mark.parametrize("bug", A.INHERITED_BUGS)
def test_inherited_wrong_variants_exceed_the_bounds(mean_results, layer, bug):
    worst = max(max(A.mean_ratios(A.mean_eval(inp, F32, bug=bug), ref, b).values()) for _, inp, ref, b in _small(mean_results, layer))
    assert worst > 1.0, (layer, bug, worst)


@pytest.mark.parametrize("gtype", ("gat", "gatv2", "transformer"))
def test_restatement_with_one_head_equals_the_committed_oracle(gtype):
    """heads = 1: the mean over one head and a zero bias added before the real one change nothing but one association,
    so outputs and every gradient agree with oracle.gnn.graphmil_forward(gnn_concat=True) to fp64 rounding"""
    D, F_, L, N = 20, 12, 2, 40
    cfg = dict(gnn_type=gtype, gnn_hidden=F_, gnn_layers=L, gnn_heads=1, att_dim=8, classifier_dim=10)
    shapes = gnn.graphmil_shapes(D, cfg)
    assert dict(A.graphmil_mean_shapes(D, cfg)) == dict(shapes)
    p = {k: v.double() for k, v in formula.formula_state_dict(shapes).items()}
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(N, D, generator=gen, dtype=F64)
    ei = torch.randint(0, N, (2, 5 * N), generator=gen)
    ei = ei[:, ei[1] % 7 != 3]                                         # nodes without incoming edges
    loss_o, out_o, g_o = gnn.graphmil_loss_and_grads(p, cfg, x, ei, 2)
    loss_m, out_m, g_m = A.graphmil_mean_loss_and_grads(p, cfg, x, ei, 2)
    # rtol 1e-12; the absolute term only admits the rounding noise of gradients that are zero in exact arithmetic (the
    # softmax-invariant attention_layers.*.2.bias), ten orders below the size of every other gradient here
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-15)      # noqa: E731
    close(loss_m, loss_o)
    for k in ("probs", "att", "z", "logits"):
        close(out_m[k], out_o[k])
    close(out_m["hs"][-1], out_o["hs"][-1])
    assert set(g_m) == set(g_o)
    for k in g_o:
        close(g_m[k], g_o[k])
    drop = {"seed": 55, "stream_base": 1024}
    close(A.graphmil_mean_forward(p, cfg, x, ei, drop=drop)["probs"], gnn.graphmil_forward(p, cfg, x, ei, drop=drop)["probs"])
