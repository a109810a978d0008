"""The attention error model of tests/f16_kernel_ref.py is sound and sharp, without a GPU: the fp32 emulation of the
kernels' documented arithmetic stays inside the per-element bounds in two summation orders (so the device test is neither
vacuous nor flaky), and six deliberately wrong emulations -- each a plausible kernel bug -- are rejected by the same
checker.  Plus the argument checks that answer before any device work and that no other test asks.

Which family rejects which control (n = 2 images x 3 heads; the worst ratio over the outputs, bound = 1):
  (a) pad_key        one zero key row counted in every softmax: `shift` (every real score is far from 0; ratios > 2000 at
                     every T) and `gauss`; NOT `peaked` (the leaked weight is e^-|max|: below the bound, ratio 1.0).
  (b) tile_unmasked  the zero rows up to the end of the last 16-key tile seen by query tile 0 (T % 16 != 0): `shift` at every
                     T (> 590); `gauss` at most T but not at T = 207 (one leaked key of weight 1/208: 0.97).
  (c) delta_last     Delta of token T-1 taken as 0: every family at every T (T = 1 included: dq, dk must be 0); `gauss`.
  (d) dk_swap8       channels 0-7 and 8-15 of head 0 exchanged in dk (T >= 2; at T = 1 dk is 0): `gauss` (> 350).
  (e) scale_d32      softmax scale 1/8 at head width 32 (T >= 2; one key has no softmax): `gauss` (> 1e4).
  (f) dq_row_1p1     token row T/2 of image 0 scaled by 1.1 in dq (T >= 2): `gauss` (> 9); `const_v` cannot (dq = 0)."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f16_kernel_ref as R  # noqa: E402

N_IMG, HEADS = 2, 3                                  # the negative controls run at the device test's middle shape


def _case(family, T, hd, n=N_IMG, H=HEADS):
    qkv, dout = R.attention_inputs(family, n, T, H, hd)
    ref = R.attention_ref(qkv, dout, n, T, H, hd)
    return qkv, dout, ref, R.attention_bounds(ref)


def test_the_constant_is_the_calibrated_one_doubled_once():
    assert R.C_EPS == 2.0 * R.CALIBRATED_C_PASS and math.log2(R.CALIBRATED_C_PASS) == int(math.log2(R.CALIBRATED_C_PASS))


def test_reference_gradients_are_the_closed_form():
    qkv, dout, ref, _ = _case("gauss", 33, 32)
    dS, sc = ref["dS"], ref["sc"]
    assert torch.allclose(ref["dq"], sc * dS @ ref["k"], rtol=1e-12, atol=1e-14)
    assert torch.allclose(ref["dk"], sc * dS.transpose(-1, -2) @ ref["q"], rtol=1e-12, atol=1e-14)
    assert torch.allclose(ref["dv"], ref["P"].transpose(-1, -2) @ ref["do"], rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("hd,n,H", R.ATT_SHAPES, ids=[f"d{hd}-n{n}-h{H}" for hd, n, H in R.ATT_SHAPES])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulation_is_within_the_bounds_in_both_summation_orders(family, hd, n, H):
    """the inputs are the device test's own: same families, token counts, shapes and seeds.  Checked with C_EPS and with
    CALIBRATED_C_PASS (a passing value; that it is the smallest power of two is what the next test pins)"""
    worst = {}
    for T in R.T_LIST:
        qkv, dout, ref, bounds = _case(family, T, hd, n, H)
        tight = R.attention_bounds(ref, R.CALIBRATED_C_PASS)
        for reverse in (False, True):
            emu = R.attention_emulation(qkv, dout, n, T, H, hd, reverse=reverse)
            r = R.attention_ratios(emu, ref, bounds)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert all(v <= 1.0 for v in r.values()), (family, hd, T, reverse, r)
            r = R.attention_ratios(emu, ref, tight)
            assert all(v <= 1.0 for v in r.values()), (family, hd, T, reverse, r)
    print(family, hd, n, H, {k: round(v, 3) for k, v in worst.items()})


def test_half_the_calibrated_constant_is_too_tight_for_the_emulation():
    """sharpness: the bound is not a loose envelope -- at c = CALIBRATED_C_PASS / 2 the correct emulation itself exceeds it
    (peaked family, dv, T = 207, head width 64, 3 images x 6 heads: measured 1.07)"""
    qkv, dout, ref, _ = _case("peaked", 207, 64, 3, 6)
    b = R.attention_bounds(ref, R.CALIBRATED_C_PASS / 2)
    worst = max(max(R.attention_ratios(R.attention_emulation(qkv, dout, 3, 207, 6, 64, reverse=rev), ref, b).values())
                for rev in (False, True))
    assert worst > 1.0, worst


def test_const_v_forward_is_v0_to_one_rounding():
    for hd in (32, 64):
        for T in (1, 17, 196, 208):
            qkv, dout, ref, _ = _case("const_v", T, hd)
            out = R.attention_emulation(qkv, dout, N_IMG, T, HEADS, hd)["out"].double()
            v0 = ref["v"]
            assert bool(((out - v0).abs() <= 2.0 ** -10 * v0.abs()).all())
            assert bool((ref["dq"].abs() <= 1e-12).all()) and bool((ref["dk"].abs() <= 1e-12).all())


# (control, families that must each reject it, the T it applies to)
CONTROLS = [
    ("pad_key", ("shift", "gauss"), R.T_LIST),
    ("tile_unmasked", ("shift",), tuple(T for T in R.T_LIST if T % 16)),
    ("delta_last", ("gauss", "peaked", "shift", "last_max", "const_v"), R.T_LIST),
    ("dk_swap8", ("gauss",), tuple(T for T in R.T_LIST if T >= 2)),
    ("scale_d32", ("gauss",), tuple(T for T in R.T_LIST if T >= 2)),
    ("dq_row_1p1", ("gauss",), tuple(T for T in R.T_LIST if T >= 2)),
]


@pytest.mark.parametrize("bug,families,Ts,hd", [c + (hd,) for c in CONTROLS for hd in (32, 64)
                                                if not (c[0] == "scale_d32" and hd == 64)],       # (e) is a width-32 bug
                         ids=lambda v: str(v) if isinstance(v, (str, int)) else "")
def test_negative_controls_are_rejected(bug, families, Ts, hd):
    for family in families:
        for T in Ts:
            qkv, dout, ref, bounds = _case(family, T, hd)
            r = R.attention_ratios(R.attention_emulation(qkv, dout, N_IMG, T, HEADS, hd, bug=bug), ref, bounds)
            assert max(r.values()) > 1.0, (bug, family, T, hd, r)


def test_what_gauss_alone_would_miss():
    """why the families exist: the padding leak is invisible to peaked rows, and the unmasked tile at T = 207 to gauss"""
    qkv, dout, ref, bounds = _case("peaked", 196, 64)
    r = R.attention_ratios(R.attention_emulation(qkv, dout, N_IMG, 196, HEADS, 64, bug="pad_key"), ref, bounds)
    assert max(r.values()) <= 1.0
    qkv, dout, ref, bounds = _case("gauss", 207, 64)
    r = R.attention_ratios(R.attention_emulation(qkv, dout, N_IMG, 207, HEADS, 64, bug="tile_unmasked"), ref, bounds)
    assert max(r.values()) <= 1.0
    qkv, dout, ref, bounds = _case("shift", 207, 64)
    r = R.attention_ratios(R.attention_emulation(qkv, dout, N_IMG, 207, HEADS, 64, bug="tile_unmasked"), ref, bounds)
    assert r["out"] > 100.0


def test_the_old_whole_tensor_metric_passes_a_row_that_is_ten_percent_wrong():
    """documentation of why the metric changed: control (f) at T = 196, 3 images x 6 heads is 4e-3 relative Frobenius, under
    the 5e-3 of test_attention_bwd_matches_fp32_autograd; the per-element bound rejects it"""
    n, T, H, hd = 3, 196, 6, 64
    qkv, dout, ref, bounds = _case("gauss", T, hd, n, H)
    emu = R.attention_emulation(qkv, dout, n, T, H, hd, bug="dq_row_1p1")
    frob = float((emu["dq"].double() - ref["dq"]).norm() / ref["dq"].norm())
    assert frob <= 5e-3, frob
    assert R.attention_ratios(emu, ref, bounds)["dq"] > 1.0


# ------------------------------------------------------------------ argument checks, before any device work
BAD_ARG, UNSUPPORTED = -1, -2
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call


def _fn(name):
    from isic_hip import lib
    return lib.lib().fn[name]


def test_attention_forward_treats_an_empty_batch_as_a_no_op():
    f, f32 = _fn("isic_attention_f16"), _fn("isic_attention_d32_f16")
    assert f(None, None, 0, 196, 6, 64, None) == 0
    assert f32(None, None, 0, 196, 16, None) == 0
    assert f(P, P, -1, 196, 6, 64, None) == BAD_ARG and f32(P, P, -1, 196, 16, None) == BAD_ARG
    assert f(None, P, 2, 196, 6, 64, None) == BAD_ARG and f32(P, None, 2, 196, 16, None) == BAD_ARG
    assert f(P, P, 0, 209, 6, 64, None) == UNSUPPORTED                 # the shape rules come first, as in the backward
    assert f(P, P, 2, 196, 6, 32, None) == UNSUPPORTED
    b, b32 = _fn("isic_attention_bwd_f16"), _fn("isic_attention_d32_bwd_f16")
    assert b(None, None, None, None, 0, 196, 6, 64, None) == 0 and b32(None, None, None, None, 0, 196, 16, None) == 0


def test_head_width_32_attention_rejects_209_tokens():
    assert _fn("isic_attention_d32_f16")(P, P, 2, 209, 16, None) == UNSUPPORTED
    assert _fn("isic_attention_d32_bwd_f16")(P, P, P, P, 2, 209, 16, None) == UNSUPPORTED
    assert _fn("isic_attention_d32_bwd_f16")(P, P, P, P, -1, 196, 16, None) == BAD_ARG


def test_layernorm_add_width_rules():
    f, b = _fn("isic_layernorm_add_f16"), _fn("isic_layernorm_add_bwd_f16")
    for N in (96, 1088):
        assert f(P, None, None, P, P, P, None, 10, N, 0, 1e-6, None) == UNSUPPORTED, N
        assert b(P, 0, 1.0, P, None, None, P, P, 0, 1e-6, None, P, None, P, P, 10, N, 1.0, 0, None, 0, None) == UNSUPPORTED, N
    assert f(P, None, None, P, P, None, None, 10, 128, 0, 1e-6, None) == BAD_ARG          # no output at all
    assert b(P, 0, 1.0, P, None, None, P, P, 0, 1e-6, None, None, None, P, P, 10, 128, 1.0, 0, None, 0, None) == BAD_ARG


def test_mae_loss_patch_size_rules():
    f = _fn("isic_mae_loss_f16")

    def call(C, H, W, Pp):
        return f(P, P, P, 0, 1.0, 1.0, P, P, 1, C, H, W, Pp, None, 0, None)
    assert call(5, 32, 32, 16) == UNSUPPORTED             # K = 1280 > 1024
    assert call(1, 8, 8, 1) == UNSUPPORTED                # K = 1: no unbiased variance
    assert call(3, 30, 32, 16) == UNSUPPORTED             # H % P
    assert call(3, 32, 30, 16) == UNSUPPORTED             # W % P


def test_masked_dwconv_rejects_a_height_or_width_that_is_not_whole_tokens():
    f, d = _fn("isic_dwconv5x5_masked_f16"), _fn("isic_dwconv5x5_masked_dgrad_f16")
    for H, W in ((30, 28), (28, 30)):
        assert f(P, P, 4, P, None, None, P, 1, H, W, 64, None) == UNSUPPORTED
        assert d(P, P, 4, P, P, 1, H, W, 64, None) == UNSUPPORTED
    assert f(P, P, 4, P, None, None, P, 1, 28, 28, 72, None) == UNSUPPORTED               # C % 64
