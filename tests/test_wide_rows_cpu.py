"""CPU-only checks of the wide GraphMIL rows (include/isic_hip_wide.h): the four entry points are declared, exported and
refuse what lies outside their documented domain before any device work, and the bounds of tests/f32_kernel_ref.py hold at
the new shapes (tests/wide_rows_cases.py): a plain fp32 evaluation stays at error / bound <= 1 against the fp64 reference
and every deliberately wrong variant exceeds 1 -- the evidence that tests/test_wide_rows_gpu.py would notice those faults."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_kernel_ref as R  # noqa: E402
import wide_rows_cases as W  # noqa: E402
from isic_hip import lib  # noqa: E402

NAMES = ("isic_attn_pool_wide_fwd", "isic_attn_pool_wide_bwd", "isic_layernorm_bwd_wide_workspace_bytes",
         "isic_layernorm_bwd_wide_ws")
BAD_ARG, UNSUPPORTED = -1, -2
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call
F32, F64 = R.F32, R.F64


# ------------------------------------------------------------------ (a) the ABI without a device
def test_wide_entry_points_are_declared_and_exported():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_wide.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = open(os.path.join(inc, "isic_hip_wide.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    for name, value in (("ISIC_WIDE_MAX_H", W.MAX_H), ("ISIC_WIDE_MAX_A", W.MAX_A), ("ISIC_WIDE_MAX_HEADS", W.MAX_HEADS),
                        ("ISIC_WIDE_MAX_BAG", W.MAX_BAG), ("ISIC_WIDE_MAX_N", W.MAX_N),
                        ("ISIC_WIDE_LN_MAX_BLOCKS", W.LN_MAX_BLOCKS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert W.MAX_BAG >= R.POOL_MAX_BAG                                   # the existing bag list fits
    L = lib.lib()
    assert os.path.join(inc, "isic_hip_wide.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name in L.fn and hasattr(cdll, name), name
        if not name.endswith("_workspace_bytes"):
            assert L.extension[name][1][-1][1] == "stream", name


def _fwd(B=3, H=2048, A=64, heads=8, max_bag=196, h=P, t=P, w3=P, b3=P, offsets=P, att=P, z=P):
    return lib.lib().fn["isic_attn_pool_wide_fwd"](h, t, w3, b3, offsets, B, H, A, heads, max_bag, att, z, None)


def _bwd(B=3, H=2048, A=64, heads=8, max_bag=196, h=P, t=P, att=P, w3=P, offsets=P, d_z=P, d_h=P, d_u=P, d_s=P):
    return lib.lib().fn["isic_attn_pool_wide_bwd"](h, t, att, w3, offsets, B, H, A, heads, max_bag, d_z, d_h, 0, d_u, d_s, None)


@pytest.mark.parametrize("f", (_fwd, _bwd), ids=("fwd", "bwd"))
def test_pool_argument_checks_without_a_device(f):
    for kw in (dict(H=W.MAX_H + 1), dict(heads=W.MAX_HEADS + 1), dict(A=W.MAX_A + 1), dict(max_bag=W.MAX_BAG + 1)):
        assert f(**kw) == UNSUPPORTED, kw
    for kw in (dict(B=-1), dict(H=0), dict(A=0), dict(heads=0), dict(max_bag=-1), dict(H=-5), dict(h=None), dict(t=None),
               dict(w3=None), dict(offsets=None), dict(att=None)):
        assert f(**kw) == BAD_ARG, kw
    assert f(B=0, h=None, t=None, w3=None, offsets=None, att=None) == 0          # no bags: nothing to do
    if f is _fwd:
        assert _fwd(b3=None) == BAD_ARG and _fwd(z=None) == BAD_ARG
    else:
        for k in ("d_z", "d_h", "d_u", "d_s"):
            assert _bwd(**{k: None}) == BAD_ARG, k


def test_layernorm_argument_checks_and_workspace_query_without_a_device():
    L = lib.lib().fn
    ws, f = L["isic_layernorm_bwd_wide_workspace_bytes"], L["isic_layernorm_bwd_wide_ws"]

    def call(M=5, N=2048, dy=P, dx=P, dgamma=P):
        return f(dy, P, P, P, P, P, dx, dgamma, P, M, N, 1, 0, 1.0, 0, 0, None, None, 0, None)
    assert call(N=W.MAX_N + 1) == UNSUPPORTED
    assert call(N=0) == BAD_ARG and call(N=-3) == BAD_ARG and call(M=-1) == BAD_ARG
    assert call(dy=None) == BAD_ARG and call(dx=None) == BAD_ARG and call(dgamma=None) == BAD_ARG
    assert call(M=0, dy=None, dx=None, dgamma=None) == 0                      # no rows: nothing to do
    assert ws(0) == 0 and ws(-1) == 0 and ws(W.MAX_N + 1) == 0
    sizes = [ws(n) for n in range(1, W.MAX_N + 1)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))        # monotone in N
    assert ws(W.MAX_N) == W.LN_MAX_BLOCKS * 2 * W.MAX_N * 4                   # a [2][N] row per block


# ------------------------------------------------------------------ (b) the bounds at the new shapes
def _assert_within(ratios, what):
    print(what, " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


@pytest.fixture(scope="module")
def ln_results():
    out = []
    for case in W.LN_CASES:
        inp = R.ln_inputs(case)
        ref = R.ln_eval(inp, F64)
        fb = R.ln_forward_bounds(inp, ref)
        out.append((case, inp, ref, fb, R.ln_backward_bounds(inp, ref, fb)))
    return out


def test_layernorm_fp32_evaluation_is_within_the_bounds_at_the_wide_shapes(ln_results):
    for case, inp, ref, fb, bb in ln_results:
        assert bb.share == 0.0, (case["id"], bb.share)                       # no ambiguous ReLU mask after resampling
        _assert_within(R.ln_ratios(R.ln_eval(inp, F32), ref, fb, bb), case["id"])


@pytest.mark.parametrize("bug", R.LN_BUGS)
def test_layernorm_wrong_variants_exceed_the_bounds_at_the_wide_shapes(ln_results, bug):
    worst = 0.0
    for case, inp, ref, fb, bb in ln_results:
        if case["M"] > 100:
            continue
        worst = max(worst, max(R.ln_ratios(R.ln_eval(inp, F32, bug=bug), ref, fb, bb).values()))
    assert worst > 1.0, (bug, worst)


@pytest.fixture(scope="module")
def pool_results():
    out = []
    for case in W.POOL_CASES:
        inp = R.pool_inputs(case)
        ref = R.pool_eval(inp, F64)
        out.append((case, inp, ref, R.pool_bounds(inp, ref)))
    return out


KEYS = ("att", "z", "d_h", "d_s", "d_u")


def test_pool_fp32_evaluation_is_within_the_bounds_at_the_wide_shapes(pool_results):
    for case, inp, ref, b in pool_results:
        _assert_within(R.pool_ratios(R.pool_eval(inp, F32), ref, b, KEYS), case["id"])
        for bi, n in enumerate(case["bags"]):
            if n == 0:
                assert bool((ref.z[bi] == 0).all())


@pytest.mark.parametrize("bug", R.POOL_BUGS)
def test_pool_wrong_variants_exceed_the_bounds_at_the_wide_shapes(pool_results, bug):
    for case, inp, ref, b in pool_results:
        if len(case["bags"]) == 1 and bug == "batch_softmax":
            continue                                                         # one bag: the batch IS the bag
        if case["heads"] == 1 and bug == "no_head_mean":
            continue                                                         # one head: the sum IS the mean
        worst = max(R.pool_ratios(R.pool_eval(inp, F32, bug=bug), ref, b, KEYS).values())
        assert worst > 1.0, (bug, case["id"], worst)
