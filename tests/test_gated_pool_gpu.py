"""Gated attention pooling on the MI355X (include/isic_hip_gated.h, csrc/gated_pool.hip, ops.attn_pool(Wg=, bg=) and the
gated models) against the fp64 restatement tests/gated_pool_ref.py, which defines the gate (the reference has none).

Tolerances are not chosen here: they are FOUR TIMES the error that the existing ungated path shows on this GPU against
fp64 (one extra transcendental and two extra products per element), measured by the fixtures of this file and printed by
every test before it asserts:
  * entries: ``e_tanh`` = max |isic_gemm_f32(act = tanh)(x I) - tanh(x)| (exact products, so the epilogue's tanh alone) and
    ``e_tb`` = max |isic_tanh_bwd_f32 - dy (1 - t^2)| / max |dy (1 - t^2)|, each the largest over the 32 shapes of ENTRY_CASES.
    tv, sg, t: absolute error <= 4 e_tanh.  d_p: <= 4 e_tb max|d_p|.  Column sums over T rows of summands x:
    <= 4 e_tb T max|x| + T eps sum_n |x_n|   (eps = 2^-24: the T-term fp32 summation bound).
  * models: ``e_f`` / ``e_g`` = the largest error / max|reference| over the outputs / the gradients of the UNGATED model of
    the same sizes against the gate-off restatement (the oracle's arithmetic in fp64: tests/test_gated_pool_cpu.py);
    gated outputs and gradients: <= 4 e_f (4 e_g) max|reference|.

Measured on an MI355X (the tests print the current figures):
  e_tanh 1.076e-07, e_tb 6.669e-08 -> forward bound 4.30e-07; the gate entries' worst over the 32 cases: tv 1.07e-07,
  sg 9.45e-08, t 1.53e-07; d_p 1.04e-06 against 2.26e-06 (h3 A33 T4097); every column sum below 1e-3 of its bound at T = 4097.
  teacher: ungated e_f 2.07e-07, e_g 1.94e-06; gated worst 2.07e-07 (bag_logits), 1.96e-06 (attention.0.bias).
  AttentionMIL: e_f 1.01e-07, e_g 8.97e-07; gated worst 1.13e-07, 2.71e-06.
  GraphMIL h1: e_f 1.64e-07, e_g 1.01e-06; gated 1.47e-07, 1.01e-06.   h4: 7.70e-07, 3.38e-06; gated 7.75e-07, 4.11e-06.
  wide (8 heads, width 1152): 2.61e-07, 6.36e-06; gated 2.58e-07, 9.74e-06.
  open gate: the five outputs bit-equal to the ungated teacher; the shared gradients within 6.1e-07 of their scale (not bit-equal:
  d_h passes through one GEMM over [V ; U] instead of V alone).
"""
import numpy as np
import pytest
import torch

import gated_pool_ref as G
from oracle import formula

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ENTRY_SHAPES = [(1, 1), (1, 5), (1, 64), (3, 33), (4, 128), (1, 129), (8, 16), (1, 772)]      # (heads, A)
ENTRY_ROWS = [1, 7, 257, 4097]
ENTRY_CASES = [(h, a, t) for (h, a) in ENTRY_SHAPES for t in ENTRY_ROWS]


def _call(name, *args):
    from isic_hip import lib
    return lib.call(name, *args)


def _dev(t):
    return t.to(DEV).contiguous()


def _workspace(T, heads, A):
    n = _call("isic_gate_bwd_f32_workspace_bytes", T, heads, A)
    return torch.empty(max(int(n), 16), device=DEV, dtype=torch.uint8), int(n)


def _gate_fwd(p, heads, A):
    a = _dev(p).clone()
    t = torch.empty(p.shape[0], heads * A, device=DEV)
    _call("isic_gate_fwd_f32", a, p.shape[0], heads, A, t)
    return a, t


def _gate_bwd(d_s, w3, a, heads, A, beta=0.0, out=None):
    T, nA = a.shape[0], heads * A
    ws, nbytes = _workspace(T, heads, A)
    d_p = torch.empty(T, 2 * nA, device=DEV)
    d_bias, d_w3, d_b3 = out if out is not None else (torch.empty(2 * nA, device=DEV), torch.empty(heads, A, device=DEV),
                                                      torch.empty(heads, device=DEV))
    _call("isic_gate_bwd_f32", d_s, w3, a, T, heads, A, d_p, d_bias, d_w3, d_b3, beta, ws, nbytes)
    return d_p, d_bias, d_w3, d_b3


# ------------------------------------------------------------------ 1. the entries against the restatement
@pytest.fixture(scope="module")
def entry_baseline():
    """e_tanh, e_tb: the existing tanh epilogue and tanh backward against fp64, the largest over ENTRY_CASES' shapes."""
    from isic_hip import ops
    e_tanh = e_tb = 0.0
    for heads, A, T in ENTRY_CASES:
        nA = heads * A
        p, _, _ = G.entry_inputs(T, heads, A, seed=1, planted=False)
        x = p[:, :nA].contiguous()
        got = ops.gemm(_dev(x), torch.eye(nA, device=DEV), act=ops.ACT_TANH).cpu().double()
        e_tanh = max(e_tanh, float((got - torch.tanh(x.double())).abs().max()))
        dy, t = p[:, nA:].contiguous(), torch.tanh(x)
        dx = torch.empty(T, nA, device=DEV)
        _call("isic_tanh_bwd_f32", _dev(dy), _dev(t), dx, T * nA)
        ref = dy.double() * (1.0 - t.double() ** 2)
        e_tb = max(e_tb, float((dx.cpu().double() - ref).abs().max()) / float(ref.abs().max()))
    print(f"\nentry baseline: e_tanh {e_tanh:.3e} (gemm act=tanh, absolute)  e_tb {e_tb:.3e} (tanh_bwd / max|ref|)")
    assert 0.0 < e_tanh < 1e-6 and 0.0 < e_tb < 1e-6                      # fp32 figures, or the baseline itself is broken
    return e_tanh, e_tb


@pytest.mark.parametrize("heads, A, T", ENTRY_CASES, ids=[f"h{h}A{a}T{t}" for h, a, t in ENTRY_CASES])
def test_gate_entries_match_the_restatement(entry_baseline, heads, A, T):
    e_tanh, e_tb = entry_baseline
    nA = heads * A
    p, d_s, w3 = G.entry_inputs(T, heads, A)
    a, t = _gate_fwd(p, heads, A)
    ac, tc = a.cpu(), t.cpu()
    assert bool(torch.isfinite(ac).all()) and bool(torch.isfinite(tc).all())          # +-inf, +-90 in p: no NaN, no inf
    tv, sg, t64 = G.gate_fwd(p, heads, A)
    fe = {"tv": float((ac[:, :nA].double() - tv).abs().max()), "sg": float((ac[:, nA:].double() - sg).abs().max()),
          "t": float((tc.double() - t64).abs().max())}
    # the backward from what the forward saved (fp32 tv | sg), so that both sides start from the same numbers
    ref = G.gate_bwd(d_s, w3, ac, heads, A)
    d_p, d_bias, d_w3, d_b3 = (v.cpu().double() for v in _gate_bwd(_dev(d_s), _dev(w3), a, heads, A))
    assert all(bool(torch.isfinite(v).all()) for v in (d_p, d_bias, d_w3, d_b3))
    x_max = float(ref["d_p"].abs().max())                                               # largest summand of d_bias
    xw_max = float(d_s.abs().max())                                                     # ... of d_w3: |d_s t| <= |d_s|
    be = {"d_p": (float((d_p - ref["d_p"]).abs().max()), 4 * e_tb * x_max)}
    for key, xm in (("d_bias", x_max), ("d_w3", xw_max), ("d_b3", 0.0)):
        got = {"d_bias": d_bias, "d_w3": d_w3, "d_b3": d_b3}[key]
        bound = 4 * e_tb * T * xm + T * G.EPS32 * ref["abs_" + key]
        err = (got - ref[key]).abs()
        worst = int(torch.argmax(err - bound))
        be[key] = (float(err.reshape(-1)[worst]), float(bound.reshape(-1)[worst]))
    print(f"\nh{heads} A{A} T{T}: forward " + " ".join(f"{k} {v:.2e}" for k, v in fe.items()) + f" (bound {4 * e_tanh:.2e});"
          " backward " + " ".join(f"{k} {e:.2e}/{b:.2e}" for k, (e, b) in be.items()))
    assert all(v <= 4 * e_tanh for v in fe.values()), fe
    assert all(e <= b for e, b in be.values()), be


# ------------------------------------------------------------------ 2. determinism and beta
@pytest.mark.parametrize("heads, A", [(3, 33), (4, 128)], ids=["scalar", "vector"])
def test_gate_bwd_is_bit_reproducible_and_beta_one_adds_in_place(heads, A):
    T, nA = 4097, heads * A
    p, d_s, w3 = G.entry_inputs(T, heads, A, seed=2, planted=False)
    a, _ = _gate_fwd(p, heads, A)
    ds, w = _dev(d_s), _dev(w3)
    first, second = _gate_bwd(ds, w, a, heads, A), _gate_bwd(ds, w, a, heads, A)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    gen = torch.Generator().manual_seed(5)
    fill = [_dev(torch.randn(s, generator=gen)) for s in ((2 * nA,), (heads, A), (heads,))]
    out = [f.clone() for f in fill]
    _gate_bwd(ds, w, a, heads, A, beta=1.0, out=out)
    for f, o, s in zip(fill, out, first[1:]):
        assert torch.equal(o, f + s)                                      # one IEEE add per element on top of what was there


# ------------------------------------------------------------------ 3. exact cases
@pytest.mark.parametrize("heads, A", [(3, 33), (4, 128)], ids=["scalar", "vector"])
def test_saturated_gate_is_exact(heads, A):
    T, nA = 257, heads * A
    p, _, _ = G.entry_inputs(T, heads, A, seed=3, planted=False)
    opened, closed = p.clone(), p.clone()
    opened[:, nA:] = 40.0 + p[:, nA:].abs()                                # every gate pre-activation >= 40
    closed[:, nA:] = -110.0 - p[:, nA:].abs()                              # ... <= -110
    a, t = _gate_fwd(opened, heads, A)
    assert bool((a[:, nA:] == 1.0).all()) and torch.equal(t, a[:, :nA])    # sg == 1: t and tv bit-equal
    a, t = _gate_fwd(closed, heads, A)
    assert bool((a[:, nA:] == 0.0).all()) and bool((t == 0.0).all())       # sg == 0: t exactly 0


# ------------------------------------------------------------------ 4. the models against the restatement
LENS = [0, 1, 5, 64]
_ZERO = (".2.bias",)      # d loss / d (score bias) = 0 analytically (softmax shift invariance): both sides hold rounding noise


def _params(module):
    return formula.formula_state_dict(formula.shapes_of(module))


def _rel(got, ref):
    ref = ref.detach().double()
    return float((got.detach().cpu().double().reshape(ref.shape) - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _model_errors(model, forward, loss_dev, loss_ref, x, outputs):
    """-> ({output: error / max|ref|}, {parameter or 'x': error / max|ref|}) of one forward + backward against fp64."""
    p = _params(model)
    model.load_state_dict(p)
    model.to(DEV).eval()
    xd = _dev(x).requires_grad_(True)
    out = forward(model, xd)
    loss_dev(out).backward()
    _, ref, grads = G.loss_and_grads(lambda q, xx: outputs(q, xx), loss_ref, p, x)
    ef = {k: _rel(out[k], ref[k]) for k in ref}
    eg = {k: _rel(prm.grad, grads[k]) for k, prm in model.named_parameters() if not k.endswith(_ZERO)}
    eg["x"] = _rel(xd.grad, grads["x"])
    for k, prm in model.named_parameters():
        if k.endswith(_ZERO):
            assert float(prm.grad.abs().max()) < 1e-5, k
    return ef, eg


def _check_against_ungated(tag, plain, gated):
    (ef0, eg0), (ef1, eg1) = plain, gated
    e_f, e_g = max(ef0.values()), max(eg0.values())
    print(f"\n{tag}: ungated e_f {e_f:.3e} e_g {e_g:.3e};  gated forward " + " ".join(f"{k} {v:.2e}" for k, v in ef1.items())
          + ";  gated gradients " + " ".join(f"{k} {v:.2e}" for k, v in eg1.items()))
    assert 0.0 < e_f < 1e-4 and 0.0 < e_g < 1e-3                          # fp32 figures, or the baseline itself is broken
    assert all(v <= 4 * e_f for v in ef1.values()), (e_f, ef1)
    assert all(v <= 4 * e_g for v in eg1.values()), (e_g, eg1)


def _teacher_case(gated):
    import utils_g_mil
    from isic_hip import ops
    offs = G.offsets_of(LENS)
    x = formula.formula_input(int(offs[-1]), 32, phase=1.3)
    y = torch.tensor([i % 3 for i in range(len(LENS))])
    m = utils_g_mil.AttentionMIL_teacher(32, 16, 8, 0.0, 3, gated=gated)
    return _model_errors(m, lambda mod, xd: mod(xd, offs), lambda o: ops.cross_entropy(o["bag_logits"], y.to(DEV)),
                         lambda o: torch.nn.functional.cross_entropy(o["bag_logits"], y), x,
                         lambda q, xx: G.teacher_forward(q, xx, offs))


def test_gated_teacher_matches_the_restatement():
    """Ragged bags [0, 1, 5, 64]: the empty bag pools nothing (bag_logits 0, bag_probs 1 / C), as the ungated head."""
    _check_against_ungated("teacher", _teacher_case(False), _teacher_case(True))


def _attmil_case(gated):
    import utils_g_mil
    from isic_hip import ops
    offs = G.offsets_of(LENS)
    x = formula.formula_input(int(offs[-1]), 32, phase=1.3)
    y = torch.tensor([i % 3 for i in range(len(LENS))])
    m = utils_g_mil.AttentionMIL(32, 16, 8, 0.0, 3, gated=gated)

    def fwd(mod, xd):
        probs, a = mod(xd, offs)
        return {"probs": probs, "a": a}

    def ref(q, xx):
        probs, a = G.attention_mil_forward(q, xx, offs)
        return {"probs": probs, "a": a}
    return _model_errors(m, fwd, lambda o: ops.cross_entropy_from_probs(o["probs"], y.to(DEV)),
                         lambda o: G.graph_loss(o["probs"], y), x, ref)


def test_gated_attention_mil_matches_the_restatement():
    _check_against_ungated("attention_mil", _attmil_case(False), _attmil_case(True))


GRAPH_CASES = {"h1": (16, 1, [5, 1, 40]), "h4": (16, 4, [5, 1, 40]), "wide": (1152, 8, [5, 1, 40])}   # gnn_hidden, att_heads, nodes


def _graphmil_case(tag, gated):
    import gnn_models
    from isic_hip import ops
    hidden, heads, nodes = GRAPH_CASES[tag]
    offs = G.offsets_of(nodes)
    x = formula.formula_input(int(offs[-1]), 24, phase=0.9)
    y = torch.tensor([i % 7 for i in range(len(nodes))])
    m = gnn_models.GraphMIL(24, "mlp", hidden, 1, 0.0, att_dim=8, att_heads=heads, classifier_dim=8, classifier_light=True,
                            att_gated=gated)

    def fwd(mod, xd):
        probs, att = mod(xd, offsets=offs)
        return {"probs": probs, "att": att}

    def ref(q, xx):
        probs, att = G.graphmil_mlp_forward(q, xx, offs, heads)
        return {"probs": probs, "att": att}
    return _model_errors(m, fwd, lambda o: ops.cross_entropy_from_probs(o["probs"], y.to(DEV)),
                         lambda o: G.graph_loss(o["probs"], y), x, ref)


@pytest.mark.parametrize("tag", list(GRAPH_CASES))
def test_gated_graphmil_matches_the_restatement(tag):
    """h1 / h4: one and four pooling heads at width 16; wide: eight heads at width 1152 (the wide pool kernels)."""
    _check_against_ungated(f"graphmil[{tag}]", _graphmil_case(tag, False), _graphmil_case(tag, True))


# ------------------------------------------------------------------ 5. an open gate is no gate
def test_open_gate_equals_the_ungated_teacher():
    import utils_g_mil
    from isic_hip import ops
    offs = G.offsets_of(LENS)
    x = formula.formula_input(int(offs[-1]), 32, phase=1.3)
    y = torch.tensor([i % 3 for i in range(len(LENS))]).to(DEV)
    plain = utils_g_mil.AttentionMIL_teacher(32, 16, 8, 0.0, 3)
    p = _params(plain)
    plain.load_state_dict(p)
    gated = utils_g_mil.AttentionMIL_teacher(32, 16, 8, 0.0, 3, gated=True)
    gated.load_state_dict(p, strict=False)
    with torch.no_grad():
        gated.attention_gate[0].weight.zero_()
        gated.attention_gate[0].bias.fill_(40.0)
    outs, grads = [], []
    for m in (plain, gated):
        m.to(DEV).eval()
        o = m(_dev(x), offs)
        ops.cross_entropy(o["bag_logits"], y).backward()
        outs.append(o)
        grads.append(dict(m.named_parameters()))
    (ef0, eg0) = _teacher_case(False)
    e_f, e_g = max(ef0.values()), max(eg0.values())
    keys = ("bag_logits", "bag_probs", "attention", "patch_logits", "patch_probs")
    ef = {k: _rel(outs[1][k], outs[0][k].detach().cpu()) for k in keys}
    eg = {k: _rel(grads[1][k].grad, grads[0][k].grad.cpu()) for k in grads[0] if not k.endswith(_ZERO)}
    bit = all(torch.equal(outs[0][k], outs[1][k]) for k in keys), all(torch.equal(grads[0][k].grad, grads[1][k].grad) for k in grads[0])
    print(f"\nopen gate: outputs bit-equal {bit[0]}, shared gradients bit-equal {bit[1]}; forward {ef}; gradients {eg}; "
          f"bounds {4 * e_f:.2e} / {4 * e_g:.2e}")
    assert all(v <= 4 * e_f for v in ef.values()) and all(v <= 4 * e_g for v in eg.values())
    assert float(gated.attention_gate[0].weight.grad.abs().max()) == 0.0      # sg == 1: sg (1 - sg) = 0, the gate learns nothing


# ------------------------------------------------------------------ 6. gradients accumulated in place
@pytest.mark.parametrize("model", ["teacher", "graphmil"])
def test_gated_gradients_accumulated_in_place_equal_autograd_accumulation(model):
    """Under ``ops.fused_grad_accumulation`` with the flat gradient buffer the gated backward adds its parameter gradients in
    place; two backward passes leave the same ``.grad``, bit for bit, as autograd's own accumulation."""
    import gnn_models
    import utils_g_mil
    from isic_hip import ops, optim
    from isic_hip.bags import BagOffsets
    torch.manual_seed(3)
    B, K, D, C = 9, 20, 24, 5
    if model == "teacher":
        m = utils_g_mil.AttentionMIL_teacher(D, 40, 12, 0.3, C, gated=True).to(DEV)
    else:
        # (without LayerNorm, whose dgamma / dbeta meet through fp32 atomics in this backward: not bit-reproducible)
        m = gnn_models.GraphMIL(D, "mlp", 40, 1, 0.3, att_dim=12, att_heads=3, classifier_dim=8, classifier_light=True,
                                num_classes=C, use_layer_norm=False, att_gated=True).to(DEV)
    m.train()
    opt = optim.AdamW(m.parameters(), lr=1e-3)
    x = _dev(torch.randn(B * K, D, generator=torch.Generator().manual_seed(4)))
    y = (torch.arange(B) % C).to(DEV)
    offs = BagOffsets.uniform(B, K, torch.device(DEV))

    def loss():
        if model == "teacher":
            return ops.cross_entropy(m(x, offs)["bag_logits"], y)
        return ops.cross_entropy_from_probs(m(x, offsets=offs)[0], y)

    def grads(fused, times):
        opt.zero_grad()
        for _ in range(times):
            m.set_dropout_state(seed=8, step=0)
            with ops.fused_grad_accumulation(fused):
                loss().backward()
        torch.cuda.synchronize()
        return opt.flat.grad.clone()
    for times in (1, 2):
        a, b = grads(False, times), grads(True, times)
        assert float(a.abs().max()) > 0
        gate = torch.cat([p.grad.reshape(-1) for k, p in m.named_parameters() if "attention_gate" in k])
        assert float(gate.abs().max()) > 0
        assert torch.equal(a, b), (model, times, float((a - b).abs().max()))


# ------------------------------------------------------------------ 7. the captured step
def test_captured_gated_teacher_step_equals_the_eager_step_bit_for_bit():
    import utils_g_mil
    from isic_hip import graphs as Gr, ops, optim
    from isic_hip.bags import BagOffsets
    dev = torch.device(DEV)
    B, K, D, C, steps = 8, 16, 32, 3, 2
    gen = torch.Generator().manual_seed(11)
    x_all = torch.randn(steps, B * K, D, generator=gen).to(dev)
    y_all = torch.randint(0, C, (steps, B), generator=gen).to(dev)
    offs = BagOffsets.uniform(B, K, dev)
    xs, ys = torch.zeros(B * K, D, device=dev), torch.zeros(B, device=dev, dtype=torch.int64)

    def load(s):
        xs.copy_(x_all[s])
        ys.copy_(y_all[s])

    def run(captured):
        torch.manual_seed(4)
        m = utils_g_mil.AttentionMIL_teacher(D, 16, 8, 0.3, C, gated=True).to(dev)
        m.train()
        m.set_dropout_state(seed=99, step=0)
        opt = optim.AdamW(m.parameters(), lr=3e-3, weight_decay=1e-3)
        clock = Gr.StepClock(dev).attach(m, opt)

        def body():
            opt.zero_grad()
            with ops.fused_grad_accumulation():
                loss = ops.cross_entropy(m(xs, offs)["bag_logits"], ys)
                loss.backward()
            opt.step()
            clock.advance()
            return loss
        load(0)
        cap = Gr.CapturedStep(body, optimizer=opt, clock=clock) if captured else None
        losses = []
        for s in range(steps):
            load(s)
            losses.append(float((cap.replay() if captured else body()).detach()))
        assert clock.read() == (steps, steps)
        Gr.StepClock.detach(m, opt)
        return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}

    l_eager, p_eager = run(False)
    l_cap, p_cap = run(True)
    l_cap2, p_cap2 = run(True)
    print("\nlosses: eager", l_eager, "captured", l_cap)
    assert l_cap == l_eager and l_cap2 == l_cap
    for k, v in p_cap.items():
        assert torch.equal(v, p_eager[k]), (k, float((v - p_eager[k]).abs().max()))
        assert torch.equal(v, p_cap2[k]), k


# ------------------------------------------------------------------ 8. a tiny training run
def test_gated_teacher_trains_on_synthetic_bags():
    """64 synthetic bags with the planted class shift of 01's synthetic path, 30 AdamW steps of 16 bags: the loss falls and
    the gate's parameters move.  No claim about accuracy."""
    import utils_g_mil
    from dataset import synthetic_latent_bags
    from isic_hip import ops, optim
    from isic_hip.bags import BagOffsets
    dev = torch.device(DEV)
    n, K, D, C, per_step = 64, 12, 32, 7, 16
    bags, labels = synthetic_latent_bags(n, K, D, classes=C, shift=0.8, seed=8)
    x_all = torch.from_numpy(np.stack(bags)).float().to(dev)
    y_all = torch.as_tensor(np.asarray(labels), device=dev).long()
    torch.manual_seed(6)
    m = utils_g_mil.AttentionMIL_teacher(D, 32, 16, 0.0, C, gated=True).to(dev)
    m.train()
    gate0 = [p.detach().clone() for p in m.attention_gate.parameters()]
    opt = optim.AdamW(m.parameters(), lr=3e-3, weight_decay=1e-4)
    offs = BagOffsets.uniform(per_step, K, dev)
    losses = []
    for s in range(30):
        idx = torch.arange(per_step, device=dev) + (s % (n // per_step)) * per_step
        opt.zero_grad()
        with ops.fused_grad_accumulation():
            loss = ops.cross_entropy(m(x_all[idx].reshape(-1, D), offs)["bag_logits"], y_all[idx])
            loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    first, last = sum(losses[:4]) / 4, sum(losses[-4:]) / 4               # one pass over the four batches each
    print(f"\nloss {first:.4f} -> {last:.4f}")
    assert np.isfinite(losses).all() and last < first and last < losses[0]
    for p0, p in zip(gate0, m.attention_gate.parameters()):
        assert float((p.detach() - p0).abs().max()) > 1e-4
