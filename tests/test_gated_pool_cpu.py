"""CPU-only checks of gated attention pooling (include/isic_hip_gated.h, tests/gated_pool_ref.py): the three entry points are
declared, exported and refuse bad arguments before any device work; the models' state_dict is unchanged with the gate off
and gains exactly the gate keys with it on; checkpoints move between the two as plain nn.Module rules say; and the fp64
restatement that defines the gate agrees with the reference's oracle where the gate is off and with closed forms where the
gate saturates."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gated_pool_ref as G  # noqa: E402
from helpers import load_golden, shapes_from_blob  # noqa: E402
from isic_hip import lib  # noqa: E402
from oracle import formula, mil  # noqa: E402

NAMES = ("isic_gate_fwd_f32", "isic_gate_bwd_f32_workspace_bytes", "isic_gate_bwd_f32")
OK, BAD_ARG, WORKSPACE = 0, -1, -3
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call


# ------------------------------------------------------------------ the ABI without a device
def test_gate_entry_points_are_declared_and_exported():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_gated.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(inc, "isic_hip_gated.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    assert os.path.join(inc, "isic_hip_gated.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    L = lib.lib()
    assert len(L.public) == 96                                           # isic_hip.h keeps its own declarations
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name not in L.public and name in L.fn and hasattr(cdll, name), name
        if not name.endswith("_workspace_bytes"):
            assert L.extension[name][1][-1][1] == "stream", name


def _fwd(T=5, heads=2, A=8, p=P, t=P):
    return lib.lib().fn["isic_gate_fwd_f32"](p, T, heads, A, t, None)


def _bwd(T=5, heads=2, A=8, d_s=P, w3=P, a=P, d_p=P + 0x10000, d_bias=P, d_w3=P, d_b3=P, beta=0.0, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.lib().fn["isic_gate_bwd_f32_workspace_bytes"](T, heads, A)
    return lib.lib().fn["isic_gate_bwd_f32"](d_s, w3, a, T, heads, A, d_p, d_bias, d_w3, d_b3, beta, ws, ws_bytes, None)


@pytest.mark.parametrize("f", (_fwd, _bwd), ids=("fwd", "bwd"))
def test_gate_argument_checks_without_a_device(f):
    for kw in (dict(T=-1), dict(heads=0), dict(heads=-2), dict(A=0), dict(A=-7)):
        assert f(**kw) == BAD_ARG, kw
    if f is _fwd:
        assert _fwd(p=None) == BAD_ARG and _fwd(t=None) == BAD_ARG
        assert _fwd(T=0, p=None, t=None) == OK                           # no rows: nothing to do, nothing touched
    else:
        for k in ("d_s", "w3", "a", "d_p", "d_bias", "d_w3", "d_b3"):
            assert _bwd(**{k: None}) == BAD_ARG, k
        assert _bwd(beta=0.5) == BAD_ARG
        assert _bwd(T=0, d_s=None, w3=None, a=None, d_p=None, d_bias=None, d_w3=None, d_b3=None, ws=None, ws_bytes=0) == OK


def test_gate_workspace_query_and_refusal_without_a_device():
    ws = lib.lib().fn["isic_gate_bwd_f32_workspace_bytes"]
    assert ws(0, 1, 8) == 0 and ws(-1, 1, 8) == 0 and ws(5, 0, 8) == 0 and ws(5, 1, 0) == 0
    for T, chunks in ((1, 1), (16, 1), (17, 2), (257, 17), (4097, 257), (16 * 2048, 2048), (10 ** 6, 2048)):
        for heads, A in ((1, 1), (3, 33), (8, 16), (1, 772)):
            assert ws(T, heads, A) == chunks * (3 * heads * A + heads) * 4, (T, heads, A)   # [chunks][3 nA + heads]: T alone
    need = ws(4097, 3, 33)
    assert _bwd(T=4097, heads=3, A=33, ws_bytes=need - 1) == WORKSPACE
    assert _bwd(T=4097, heads=3, A=33, ws=None) == WORKSPACE
    assert _bwd(T=4097, heads=3, A=33, ws=P + 4) == WORKSPACE               # not 16-byte aligned


# ------------------------------------------------------------------ state_dict and checkpoints
def _models(gated):
    import gnn_models
    import model
    import utils_g_mil
    gt, ga, gg = (load_golden(f) for f in ("teacher_ref.npz", "attmil_ref.npz", "graphmil_mlp_ref.npz"))
    _, D, H, A, C = (int(v) for v in gt["dims"])
    teacher = utils_g_mil.AttentionMIL_teacher(D, H, A, 0.5, C, gated=gated)
    _, D2, H2, A2, C2 = (int(v) for v in ga["dims"])
    attmil = utils_g_mil.AttentionMIL(D2, H2, A2, 0.5, C2, gated=gated)
    _, Dg, Fg, Lg = (int(v) for v in gg["dims"])
    graphmil = gnn_models.GraphMIL(input_dim=Dg, gnn_type="mlp", gnn_hidden=Fg, gnn_layers=Lg, gnn_dropout=0.5, gnn_heads=4,
                                   gnn_concat=True, att_dim=int(gg["att_dim"]), att_heads=4, pool_dropout=0.2,
                                   classifier_dim=int(gg["classifier_dim"]), classifier_light=True, num_classes=7,
                                   use_residual=True, use_layer_norm=True, att_gated=gated)
    assert model.MultiModalMILNet.__init__.__defaults__[-1] is False          # mil_gated, last and off
    return ((teacher, shapes_from_blob(gt["names"]), [("attention_gate.0.weight", (A, H)), ("attention_gate.0.bias", (A,))]),
            (attmil, shapes_from_blob(ga["names"]), [("attention_gate.0.weight", (A2, H2)), ("attention_gate.0.bias", (A2,))]),
            (graphmil, shapes_from_blob(gg["names"]),
             [(f"attention_gates.{k}.0.{n}", s) for k in range(4) for n, s in (("weight", (int(gg["att_dim"]), Fg)), ("bias", (int(gg["att_dim"]),)))]))


def test_state_dict_is_unchanged_with_the_gate_off():
    for m, golden, _ in _models(False):
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(golden.items()), type(m).__name__


def test_state_dict_gains_exactly_the_gate_keys_with_the_gate_on():
    for m, golden, gate in _models(True):
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(golden.items()) + gate, type(m).__name__


def test_lazily_built_graphmil_and_milnet_take_the_keyword():
    import utils_g_mil
    m = utils_g_mil.GraphMIL(12, "mlp", 8, 1, 0.0, att_dim=4, att_heads=2, classifier_dim=4, classifier_light=True,
                             att_gated=True)
    assert [k for k in m.state_dict() if k.startswith("attention_gates.")] == [
        "attention_gates.0.0.weight", "attention_gates.0.0.bias", "attention_gates.1.0.weight", "attention_gates.1.0.bias"]
    import model
    net = model.MultiModalMILNet(hidden_dim=16, att_dim=8, dropout=0.0, radiomics_dim=4, num_classes=3, mil_gated=True)
    assert tuple(net.state_dict()["mil.attention_gate.0.weight"].shape) == (8, 16)
    assert "mil.attention_gate.0.weight" not in model.MultiModalMILNet(hidden_dim=16, att_dim=8, radiomics_dim=4).state_dict()


def test_checkpoints_between_gated_and_ungated_models():
    import utils_g_mil
    torch.manual_seed(0)
    plain = utils_g_mil.AttentionMIL_teacher(12, 8, 4, 0.0, 3)
    gated = utils_g_mil.AttentionMIL_teacher(12, 8, 4, 0.0, 3, gated=True)
    init = {k: v.clone() for k, v in gated.state_dict().items()}
    res = gated.load_state_dict(plain.state_dict(), strict=False)          # ungated checkpoint -> gated model
    assert sorted(res.missing_keys) == ["attention_gate.0.bias", "attention_gate.0.weight"] and not res.unexpected_keys
    for k, v in gated.state_dict().items():
        assert torch.equal(v, init[k] if k.startswith("attention_gate.") else plain.state_dict()[k]), k
    with pytest.raises(RuntimeError, match="attention_gate"):
        plain.load_state_dict(gated.state_dict(), strict=True)             # gated checkpoint -> ungated model


# ------------------------------------------------------------------ the restatement against the oracle and closed forms
LENS = [0, 1, 5, 64]


def _teacher_params(gated, D=32, H=16, A=8, C=3):
    import utils_g_mil
    m = utils_g_mil.AttentionMIL_teacher(D, H, A, 0.0, C, gated=gated)
    return formula.formula_state_dict(formula.shapes_of(m))


def test_restatement_with_the_gate_off_is_the_oracle():
    p = G.f64(_teacher_params(False))
    offs = G.offsets_of(LENS)
    x = formula.formula_input(int(offs[-1]), 32, phase=0.7).double()
    ours = G.teacher_forward(p, x, offs)
    theirs = mil.teacher_forward_batched(p, x, offs)
    for k in ("bag_logits", "bag_probs", "attention", "patch_logits", "patch_probs"):
        # the same formulas in fp64; only the row blocking of the matrix products differs (all rows at once / bag by bag)
        assert ours[k].shape == theirs[k].shape and float((ours[k] - theirs[k]).abs().max()) <= 1e-13, k


def test_restatement_of_attention_mil_and_graphmil_with_the_gate_off_is_the_oracle():
    import gnn_models
    import utils_g_mil
    from oracle import gnn
    offs = G.offsets_of(LENS[1:])
    x = formula.formula_input(int(offs[-1]), 32, phase=0.7).double()
    p = G.f64(formula.formula_state_dict(formula.shapes_of(utils_g_mil.AttentionMIL(32, 16, 8, 0.0, 3))))
    probs, a = G.attention_mil_forward(p, x, offs)
    for b in range(len(offs) - 1):
        pb, ab, _, _ = mil.attention_mil_forward(p, x[offs[b]:offs[b + 1]])
        assert float((probs[b] - pb).abs().max()) <= 1e-13 and float((a[offs[b]:offs[b + 1]] - ab).abs().max()) <= 1e-13
    cfg = dict(gnn_type="mlp", gnn_hidden=16, gnn_layers=1, gnn_dropout=0.0, att_dim=8, att_heads=4, classifier_dim=8,
               classifier_light=True, num_classes=7, use_residual=True, use_layer_norm=True)
    m = gnn_models.GraphMIL(32, "mlp", 16, 1, 0.0, att_dim=8, att_heads=4, classifier_dim=8, classifier_light=True)
    p = G.f64(formula.formula_state_dict(formula.shapes_of(m)))
    probs, att = G.graphmil_mlp_forward(p, x, offs, 4)
    for b in range(len(offs) - 1):
        o = gnn.graphmil_forward(p, cfg, x[offs[b]:offs[b + 1]])
        assert float((probs[b] - o["probs"]).abs().max()) <= 1e-13
        assert float((att[offs[b]:offs[b + 1]] - o["att"]).abs().max()) <= 1e-13


def test_entry_backward_formulas_are_the_autograd_gradient():
    heads, A, T = 3, 5, 11
    p, d_s, w3 = G.entry_inputs(T, heads, A, planted=False)
    pre = p.double().requires_grad_(True)
    w = w3.double().requires_grad_(True)
    c = torch.zeros(heads, dtype=torch.float64, requires_grad=True)
    tv, sg, t = G.gate_fwd(pre, heads, A)
    s = (t.reshape(T, heads, A) * w).sum(-1) + c                          # [T, heads]
    (s * d_s.double()).sum().backward()
    r = G.gate_bwd(d_s, w3, torch.cat([tv, sg], 1).detach(), heads, A)
    for got, want in ((r["d_p"], pre.grad), (r["d_w3"], w.grad), (r["d_b3"], c.grad),
                      (r["d_bias"], pre.grad.sum(0))):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("gate, uniform", [(40.0, False), (-40.0, True)])
def test_restatement_at_a_saturated_gate(gate, uniform):
    """Gate pre-activation +40: sigmoid = 1 to the last bit of fp64 (1 + e^-40 rounds to 1), so t == tv and the gated head IS
    the ungated one, bit for bit.  -40: sigmoid = 4.2e-18, which no IEEE format rounds to 0, so |t| <= 4.3e-18 is what
    "t is 0" can mean here; it IS exactly 0 for the scores: t w (< 1e-16) is absorbed by the bias 0.25 (half an ulp: 2.8e-17),
    every score equals the bias bit for bit and the attention is exactly 1 / n."""
    p = G.f64(_teacher_params(True))
    p["attention_gate.0.weight"] = torch.zeros_like(p["attention_gate.0.weight"])
    p["attention_gate.0.bias"] = torch.full_like(p["attention_gate.0.bias"], gate)
    p["attention.2.bias"] = torch.full_like(p["attention.2.bias"], 0.25)
    p["attention.2.weight"] = p["attention.2.weight"].clamp(-1.0, 1.0)
    offs = G.offsets_of(LENS)
    x = formula.formula_input(int(offs[-1]), 32, phase=0.7).double()
    h = G._hidden(p, x)
    pre = torch.cat([torch.nn.functional.linear(h, p["attention.0.weight"], p["attention.0.bias"]),
                     torch.nn.functional.linear(h, p["attention_gate.0.weight"], p["attention_gate.0.bias"])], 1)
    tv, sg, t = G.gate_fwd(pre, 1, 8)
    out = G.teacher_forward(p, x, offs)
    if not uniform:
        assert torch.equal(t, tv)
        plain = {k: v for k, v in p.items() if not k.startswith("attention_gate.")}
        ref = G.teacher_forward(plain, x, offs)
        for k in ref:
            assert torch.equal(out[k], ref[k]), k
    else:
        assert float(t.abs().max()) <= 4.3e-18
        s = G.scores(h, p["attention.0.weight"], p["attention.0.bias"], p["attention.2.weight"], p["attention.2.bias"],
                     p["attention_gate.0.weight"], p["attention_gate.0.bias"])
        assert bool((s == 0.25).all())
        want = torch.cat([torch.full((n,), 1.0 / n, dtype=torch.float64) for n in LENS if n])
        assert torch.equal(out["attention"], want)
    assert bool((out["bag_logits"][0] == 0).all()) and np.allclose(out["bag_probs"][0].numpy(), 1.0 / 3)  # the empty bag
