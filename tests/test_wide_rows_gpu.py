"""The wide GraphMIL rows on the MI355X (include/isic_hip_wide.h, csrc/wide_rows.hip): attention pooling beyond 1024
feature columns / four pooling heads and the LayerNorm backward beyond 1024 columns.

A  through the C ABI against the fp64 references and derived per-element bounds of tests/f32_kernel_ref.py on the cases of
   tests/wide_rows_cases.py (tests/test_wide_rows_cpu.py shows on the CPU that those bounds admit a correct fp32
   evaluation and reject the wrong variants at these shapes); outputs are pre-filled with NaN between guard areas; the
   order-fixed forms are bit-equal across two runs; out-of-domain calls answer -2 and touch nothing.
B  through GraphMIL against oracle/gnn.py in fp64 on configurations of the reference's search space (tune_mil.py:170-200)
   that raised RuntimeError before these entries existed: forward, every gradient, a ragged batch, train-mode dropout, the
   top of the space, a captured AdamW step; and which entries the Python layer calls for which shape.

Model tolerance: every quantity is measured as max|got - ref| / max|ref| against the fp64 oracle and may reach the larger
of the rtol tests/test_graph_gpu.py uses for it (5e-5 forward, 5e-4 gradients) and 4 x the same figure of the fp32 CPU
oracle on the same inputs (two independent fp32 evaluations can each be off by that much in opposite directions, and the
device sums in a different order).  Both figures are printed (visible with -s)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_kernel_ref as R  # noqa: E402
import wide_rows_cases as W  # noqa: E402
from helpers import assert_close  # noqa: E402
from oracle import formula, gnn  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
PAD = 64                                            # NaN floats before and after every guarded output (a multiple of 4)
F64 = torch.float64
UNSUPPORTED = -2
WIDE = ("isic_attn_pool_wide_fwd", "isic_attn_pool_wide_bwd", "isic_layernorm_bwd_wide_ws")


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _code(*a):
    """the return code of a call that is expected to be refused"""
    from isic_hip.lib import IsicHipError
    try:
        _call(*a)
    except IsicHipError as e:
        return e.code
    return 0


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further GPU work: {e}", returncode=3)


def _check(what, ratios):
    print(what, " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


class Guarded:
    """an fp32 output of `shape`, NaN pre-filled, with PAD NaN floats before and after it (the helper of
    tests/test_f32_kernel_domain_gpu.py, restated)"""

    def __init__(self, shape, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((2 * PAD + n + 4,), NAN, device=DEV, dtype=torch.float32)
        self.lo = PAD
        self.n = n
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def ok(self, finite=True):
        intact = bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())
        return intact and (not finite or bool(torch.isfinite(self.t).all()))

    def untouched(self):
        return bool(torch.isnan(self.buf).all())

    def cpu(self):
        return self.t.detach().cpu()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ================================================================== A1. attention pool
@pytest.mark.parametrize("case", W.POOL_CASES, ids=[c["id"] for c in W.POOL_CASES])
def test_wide_attention_pool_forward_and_backward(case):
    inp = R.pool_inputs(case)
    ref = R.pool_eval(inp, F64)
    b = R.pool_bounds(inp, ref)
    H, A, heads, T, B = inp.H, inp.A, inp.heads, inp.T, inp.B
    h, t, w3, b3, offsets = _dev(inp.h), _dev(inp.t), _dev(inp.w3), _dev(inp.b3), inp.offsets.to(DEV)
    max_bag = max(case["bags"])
    att, z = Guarded((T, heads)), Guarded((B, H))
    if case["fwd"] == "wide":
        _call("isic_attn_pool_wide_fwd", h, t, w3, b3, offsets, B, H, A, heads, max_bag, att.t, z.t)
    else:                                                  # heads > 4 at ordinary width: the existing forward's launches
        _call("isic_attn_pool_fwd", h, t, w3, b3, None, None, offsets, B, H, A, heads, 0, max_bag, att.t, z.t, None, None, None, None)
    assert att.ok() and z.ok()
    got = dict(att=att.cpu(), z=z.cpu())
    ratios = R.pool_ratios(got, ref, b, ("att", "z"))
    for bi, n in enumerate(case["bags"]):                  # an empty bag: zeros
        if n == 0:
            assert bool((got["z"][bi] == 0).all())
    dz = _dev(inp.dz)

    def backward():
        d_h = Guarded((T, H), init=inp.dh0 if inp.accumulate_dh else None)
        d_u, d_s = Guarded((T, heads * A)), Guarded((T, heads))
        _call("isic_attn_pool_wide_bwd", h, t, att.t, w3, offsets, B, H, A, heads, max_bag, dz, d_h.t, inp.accumulate_dh,
              d_u.t, d_s.t)
        o = dict(d_h=d_h, d_u=d_u, d_s=d_s)
        assert all(g.ok() for g in o.values())
        return {k: g.cpu() for k, g in o.items()}
    r1, r2 = backward(), backward()
    for k, v in R.pool_ratios(r1, ref, b, ("d_h", "d_s", "d_u")).items():
        ratios[f"bwd.{k}"] = v
    for k in r1:                                           # no atomics, fixed summation order: bit-equal across two runs
        assert torch.equal(_bits(r1[k]), _bits(r2[k])), k
    if case["fwd"] == "wide":                              # ... the forward too
        att2, z2 = Guarded((T, heads)), Guarded((B, H))
        _call("isic_attn_pool_wide_fwd", h, t, w3, b3, offsets, B, H, A, heads, max_bag, att2.t, z2.t)
        assert torch.equal(_bits(att2.cpu()), _bits(got["att"])) and torch.equal(_bits(z2.cpu()), _bits(got["z"]))
    _check(case["id"] + " [" + case["arm"] + "]", ratios)


def test_wide_attention_pool_refuses_outside_its_domain_and_touches_nothing():
    case = dict(H=64, A=32, heads=2, C=0, family="random", bags=(3, 5), arm="", accumulate_dh=0)
    inp = R.pool_inputs(case)
    h, t, w3, b3, offsets = _dev(inp.h), _dev(inp.t), _dev(inp.w3), _dev(inp.b3), inp.offsets.to(DEV)
    dz = _dev(inp.dz)
    for kw in (dict(H=W.MAX_H + 1), dict(A=W.MAX_A + 1), dict(heads=W.MAX_HEADS + 1), dict(max_bag=W.MAX_BAG + 1)):
        d = dict(H=64, A=32, heads=2, max_bag=5)
        d.update(kw)
        g = Guarded((8, 64))
        assert _code("isic_attn_pool_wide_fwd", h, t, w3, b3, offsets, 2, d["H"], d["A"], d["heads"], d["max_bag"], g.t, g.t) == UNSUPPORTED, kw
        assert g.untouched(), kw
        assert _code("isic_attn_pool_wide_bwd", h, t, g.t, w3, offsets, 2, d["H"], d["A"], d["heads"], d["max_bag"], dz, g.t, 0, g.t,
                     g.t) == UNSUPPORTED, kw
        assert g.untouched(), kw


# ================================================================== A2. LayerNorm backward
def _ln_backward(form, inp, x, dy, gamma, beta, mean, rstd, clock, thr):
    M, N = inp.M, inp.N
    dx = Guarded((M, N))
    dgamma, dbeta = Guarded((N,), init=inp.dgamma0), Guarded((N,), init=inp.dbeta0)    # accumulated into non-zero buffers
    tail = (M, N, inp.relu, thr, inp.scale, R.LN_SEED, R.LN_STREAM, clock)
    if form == "atomic":
        _call("isic_layernorm_bwd_wide_ws", dy, x, gamma, beta, mean, rstd, dx.t, dgamma.t, dbeta.t, *tail, None, 0)
    else:
        nbytes = _call("isic_layernorm_bwd_wide_workspace_bytes", N)
        assert nbytes == W.LN_MAX_BLOCKS * 2 * N * 4
        ws = torch.empty(nbytes + 16, device=DEV, dtype=torch.uint8)
        _call("isic_layernorm_bwd_wide_ws", dy, x, gamma, beta, mean, rstd, dx.t, dgamma.t, dbeta.t, *tail, ws, nbytes)
    assert dx.ok() and dgamma.ok() and dbeta.ok(), form
    return dict(dx=dx.cpu(), dgamma=dgamma.cpu(), dbeta=dbeta.cpu())


@pytest.mark.parametrize("case", W.LN_CASES, ids=[c["id"] for c in W.LN_CASES])
def test_wide_layernorm_backward_with_and_without_a_workspace(case):
    inp = R.ln_inputs(case)
    ref = R.ln_eval(inp, F64)
    fb = R.ln_forward_bounds(inp, ref)
    bb = R.ln_backward_bounds(inp, ref, fb)
    assert bb.share <= R.AMBIGUOUS_CAP
    M, N = inp.M, inp.N
    x, dy, gamma, beta, res = _dev(inp.x), _dev(inp.dy), _dev(inp.gamma), _dev(inp.beta), _dev(inp.res)
    y, mean, rstd = Guarded((M, N)), Guarded((M,)), Guarded((M,))
    clock = None if inp.clock is None else torch.tensor([inp.clock, 0], dtype=torch.int64, device=DEV)
    thr = R.drop_threshold(inp.p)
    _call("isic_layernorm_fwd_clk", x, gamma, beta, res, y.t, mean.t, rstd.t, M, N, R.LN_EPS, inp.relu, thr, inp.scale,
          R.LN_SEED, R.LN_STREAM, clock)
    assert y.ok() and mean.ok() and rstd.ok()
    got = dict(y=y.cpu(), mean=mean.cpu().view(M, 1), rstd=rstd.cpu().view(M, 1))
    args = (inp, x, dy, gamma, beta, mean.t, rstd.t, clock, thr)
    runs = {"atomic": _ln_backward("atomic", *args), "ws": _ln_backward("ws", *args)}
    ratios = R.ln_ratios(got, ref, fb)
    for form, out in runs.items():
        for k, v in R.ln_ratios({**got, **out}, ref, fb, bb).items():
            if k not in ("y", "mean", "rstd"):
                ratios[f"{form}.{k}"] = v
    again = _ln_backward("ws", *args)                      # the partial rows are added in block order: bit-equal across two runs
    for k, v in again.items():
        assert torch.equal(_bits(v), _bits(runs["ws"][k])), k
    _check(case["id"], ratios)


def test_wide_layernorm_backward_refuses_width_4097_and_touches_nothing():
    N, M = W.MAX_N + 1, 2
    x = torch.randn(M, N, device=DEV)
    v = torch.ones(N, device=DEV)
    r = torch.ones(M, device=DEV)
    d, g = Guarded((M, N)), Guarded((N,))
    assert _call("isic_layernorm_bwd_wide_workspace_bytes", N) == 0
    assert _code("isic_layernorm_bwd_wide_ws", x, x, v, v, r, r, d.t, g.t, g.t, M, N, 0, 0, 1.0, 0, 0, None, None, 0) == UNSUPPORTED
    assert d.untouched() and g.untouched()


# ================================================================== B. GraphMIL
CONFIGS = {
    "gat-288x4-att8": dict(gnn_type="gat", gnn_hidden=288, gnn_heads=4, gnn_layers=2, att_heads=8),        # 1152 columns
    "transformer-136x8-att2": dict(gnn_type="transformer", gnn_hidden=136, gnn_heads=8, gnn_layers=2, att_heads=2),   # 1088
    "mlp-1032-att8": dict(gnn_type="mlp", gnn_hidden=1032, gnn_heads=4, gnn_layers=2, att_heads=8),
    "gcn-64-att8": dict(gnn_type="gcn", gnn_hidden=64, gnn_heads=4, gnn_layers=2, att_heads=8),            # narrow: backward route only
}
TOP = dict(gnn_type="gat", gnn_hidden=512, gnn_heads=8, gnn_layers=1, att_heads=8, att_dim=512)           # 4096 columns
FWD_RTOL, GRAD_RTOL = 5e-5, 5e-4
LABEL = 4


def _cfg(c):
    return dict(dict(att_dim=32, classifier_dim=48), **c)


def _model(cfg, D, train=False):
    from gnn_models import GraphMIL
    m = GraphMIL(input_dim=D, gnn_type=cfg["gnn_type"], gnn_hidden=cfg["gnn_hidden"], gnn_layers=cfg["gnn_layers"], gnn_dropout=0.5,
                 gnn_heads=cfg["gnn_heads"], att_dim=cfg["att_dim"], att_heads=cfg["att_heads"], pool_dropout=0.2,
                 classifier_dim=cfg["classifier_dim"], classifier_light=True, num_classes=7)
    shapes = gnn.graphmil_shapes(D, cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(shapes.items())
    p = formula.formula_state_dict(shapes)
    m.load_state_dict(p)
    m = m.to(DEV)
    return (m.train() if train else m.eval()), p


def _zero_by_shift_invariance(k):
    return (k.startswith("attention_layers") and k.endswith("2.bias")) or k.endswith("lin_key.bias")


def _rel(a, ref):
    a = a.detach().cpu().double()
    ref = ref.detach().double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


_ORACLE = {}
RELU_MARGIN = 5e-5


class _ReluInputs:
    """records the smallest |input| of every F.relu the oracle evaluates (the LayerNorm outputs and the classifier's hidden)"""

    def __enter__(self):
        self.min, self._relu = float("inf"), gnn.F.relu

        def spy(x, *a, **kw):
            self.min = min(self.min, float(x.detach().abs().min()))
            return self._relu(x, *a, **kw)
        gnn.F.relu = spy
        return self

    def __exit__(self, *exc):
        gnn.F.relu = self._relu


def _oracle(name, cfg, N, D, k):
    """x, edge index, and the oracle in fp64 and fp32 (loss, outputs, gradients), once per configuration.

    A ReLU input of an fp32 evaluation departs from the fp64 one by up to ~2e-5 (node embeddings: 1.7e-5 on values of
    magnitude 5); an input closer to zero than that may take either mask, and one flipped mask moves a row of a gradient
    by percents of its largest entry (seen between the fp32 and the fp64 CPU oracle).  At 40 x 1152 x 2 inputs a random x
    has such an element more often than not, so x is the first seed from 2 upward at which every ReLU input of the fp64
    oracle stays RELU_MARGIN away from zero: the comparison is then one of summation order alone."""
    if name not in _ORACLE:
        import build_graphs as bg
        p = formula.formula_state_dict(gnn.graphmil_shapes(D, cfg))
        p64 = {kk: v.double() for kk, v in p.items()}
        for seed in range(2, 400):
            x = torch.randn(N, D, generator=torch.Generator().manual_seed(seed))
            ei = bg._knn_edge_index(x, k).cpu()
            with _ReluInputs() as seen, torch.no_grad():
                gnn.graphmil_forward(p64, cfg, x.double(), ei)
            if seen.min >= RELU_MARGIN:
                break
        else:
            raise AssertionError("no input with every ReLU input %g away from zero" % RELU_MARGIN)
        print(f"{name}: x from seed {seed}, smallest |ReLU input| {seen.min:.2e}")
        o64 = gnn.graphmil_loss_and_grads(p64, cfg, x.double(), ei, LABEL)
        o32 = gnn.graphmil_loss_and_grads(p, cfg, x, ei, LABEL)
        _ORACLE[name] = (x, ei, o64, o32)
    return _ORACLE[name]


def _compare_with_oracle(name, cfg, N, D, k):
    from isic_hip import ops
    x, ei, (loss64, out64, g64), (loss32, out32, g32) = _oracle(name, cfg, N, D, k)
    m, _ = _model(cfg, D)
    xd = x.to(DEV).requires_grad_(True)
    probs, att = m(xd, ei.to(DEV))
    loss = ops.cross_entropy_from_probs(probs.unsqueeze(0), torch.tensor([LABEL], device=DEV))
    loss.backward()
    rows = [("probs", probs, out64["probs"], out32["probs"], FWD_RTOL), ("att", att, out64["att"], out32["att"], FWD_RTOL),
            ("emb", m.last_node_embeddings, out64["hs"][-1], out32["hs"][-1], FWD_RTOL),
            ("loss", loss.reshape(()), loss64.reshape(()), loss32.reshape(()), FWD_RTOL)]
    for kk, prm in m.named_parameters():
        if _zero_by_shift_invariance(kk):
            continue
        rows.append((kk, prm.grad, g64[kk], g32[kk], GRAD_RTOL))
    rows.append(("x", xd.grad, g64["x"], g32["x"], GRAD_RTOL))
    bad = []
    for what, got, r64, r32, rtol in rows:
        dev_fig, cpu_fig = _rel(got, r64), _rel(r32, r64)
        allowed = max(rtol, 4 * cpu_fig)
        print(f"{name} {what}: device {dev_fig:.3e}  fp32 oracle {cpu_fig:.3e}  allowed {allowed:.3e}")
        if not dev_fig <= allowed:
            bad.append((what, dev_fig, allowed))
    assert not bad, bad


@pytest.mark.parametrize("name", list(CONFIGS))
def test_wide_graphmil_forward_and_every_gradient_vs_the_fp64_oracle(name):
    _compare_with_oracle(name, _cfg(CONFIGS[name]), 40, 96, 5)


def test_graphmil_at_the_top_of_the_search_space_vs_the_fp64_oracle():
    """gat 512 x 8 = 4096 columns, eight pooling heads of 512: the largest width, head count and attention width at once"""
    _compare_with_oracle("top", dict(dict(classifier_dim=48), **TOP), 20, 96, 5)


def _rand_graph(n, e, gen):
    src = torch.randint(0, n, (e,), generator=gen)
    dst = torch.randint(0, n, (e,), generator=gen)
    keep = src != dst
    return torch.stack([src[keep], dst[keep]])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_wide_graphmil_ragged_batch_equals_per_graph_and_dropout_equals_the_oracle(name):
    cfg = _cfg(CONFIGS[name])
    D = 48
    m, p = _model(cfg, D)
    gen = torch.Generator().manual_seed(8)
    sizes = [20, 7, 33]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    xs = [torch.randn(n, D, generator=gen) for n in sizes]
    eis = [_rand_graph(n, 4 * n, gen) for n in sizes]
    big_x = torch.cat(xs).to(DEV)
    big_e = torch.cat([e + int(o) for e, o in zip(eis, offs[:-1])], dim=1).to(DEV)
    probs_b, att_b = m(big_x, big_e, offsets=offs)
    for i, (xg, eg) in enumerate(zip(xs, eis)):
        pr, at = m(xg.to(DEV), eg.to(DEV))
        assert_close(probs_b[i], pr, rtol=1e-5, atol=1e-6, what="batched probs")          # tests/test_graph_gpu.py:254-255
        assert_close(att_b[offs[i]:offs[i + 1]], at, rtol=1e-5, atol=1e-6, what="batched att")
    # train mode (a single graph, so that the element indices coincide with the oracle's per-graph call)
    m.train()
    m.set_dropout_state(seed=321, step=3)
    pr, _ = m(xs[0].to(DEV), eis[0].to(DEV))
    drop = {"seed": 321, "stream_base": 3 * 1024}
    ocfg = dict(cfg, gnn_dropout=0.5, pool_dropout=0.2)
    o64 = gnn.graphmil_forward({kk: v.double() for kk, v in p.items()}, ocfg, xs[0].double(), eis[0], drop=drop)["probs"]
    o32 = gnn.graphmil_forward(p, ocfg, xs[0], eis[0], drop=drop)["probs"]
    dev_fig, cpu_fig = _rel(pr, o64), _rel(o32, o64)
    print(f"{name} dropout probs: device {dev_fig:.3e}  fp32 oracle {cpu_fig:.3e}")
    assert dev_fig <= max(FWD_RTOL, 4 * cpu_fig)


def test_captured_wide_step_equals_eager_steps():
    """Two AdamW steps of GraphMIL[mlp, 1152 columns, eight pooling heads] (LayerNorm + dropout on), three ways: eager with
    the host clock, eager with the device step clock, and captured into a hipGraph with the device clock and replayed (the wide
    pool and LayerNorm entries allocate nothing of their own inside the capture, and the LayerNorm backward replays the
    dropout words of the step the device clock shows).

    Captured and eager-with-the-device-clock run the same kernels with the same arguments and no kernel on this path joins
    partial sums through atomics: losses and parameters are bit-equal.  Against the host clock only the place where Adam's
    bias correction is evaluated differs, an ulp per parameter after the first step; Adam then divides every gradient element
    by its own magnitude, so elements that are a cancellation of 1152 terms carry that ulp many orders larger into their
    update.  Held there: the losses to 2e-5 (the first, before any update, to 1e-6) and every parameter to 5 % of ONE update
    (lr) -- a replay with the wrong dropout words or step moves a large share of the elements by a whole update or two.

    mlp, because the attention-coefficient dropout of the GAT / TransformerConv layers takes no device clock
    (isic_hip/graph.py), at any width."""
    from dataset import synthetic_latent_bags
    from gnn_models import GraphMIL
    from isic_hip import graphs as G, ops, optim
    from isic_hip.bags import BagOffsets
    dev = torch.device(DEV)
    n, D, Gs, steps, lr = 30, 32, 6, 2, 3e-3
    bags, labels = synthetic_latent_bags(12, n, D, classes=7, shift=0.8, seed=8)
    x_all = torch.from_numpy(np.stack(bags)).float().to(dev)                   # [12, n, D]
    y_all = torch.as_tensor(np.asarray(labels), device=dev).long()
    batches = [torch.as_tensor(np.random.RandomState(40 + s).permutation(len(bags))[:Gs], device=dev) for s in range(steps)]
    offs = BagOffsets.uniform(Gs, n, dev)
    xs, ys = torch.zeros(Gs * n, D, device=dev), torch.zeros(Gs, device=dev, dtype=torch.int64)     # the step's static inputs

    def load(s):
        xs.copy_(x_all[batches[s]].reshape(-1, D))
        ys.copy_(y_all[batches[s]])

    def run(device_clock, captured):
        torch.manual_seed(4)
        m = GraphMIL(D, "mlp", 1152, 2, 0.5, att_dim=16, att_heads=8, pool_dropout=0.2, classifier_dim=24,
                     classifier_light=True, num_classes=7).to(dev)
        m.train()
        m.set_dropout_state(seed=99, step=0)
        opt = optim.AdamW(m.parameters(), lr=lr, weight_decay=1e-3)
        clock = G.StepClock(dev).attach(m, opt) if device_clock else None

        def body():
            opt.zero_grad()
            probs, _ = m(xs, offsets=offs)
            loss = ops.cross_entropy_from_probs(probs, ys)
            loss.backward()
            opt.step()
            if clock is not None:
                clock.advance()
            return loss
        load(0)
        cap = G.CapturedStep(body, optimizer=opt, clock=clock) if captured else None
        losses = []
        for s in range(steps):
            load(s)
            losses.append(float((cap.replay() if captured else body()).detach()))
        if clock is not None:
            assert clock.read() == (steps, steps)
            G.StepClock.detach(m, opt)
        return losses, {k: v.detach().clone() for k, v in m.state_dict().items()}

    l_host, p_host = run(False, False)
    l_dev, p_dev = run(True, False)
    l_cap, p_cap = run(True, True)
    print("losses: host clock", l_host, "device clock", l_dev, "captured", l_cap)
    assert l_cap == l_dev, (l_cap, l_dev)
    for k, v in p_cap.items():
        assert torch.equal(v, p_dev[k]), (k, float((v - p_dev[k]).abs().max()))
    assert abs(l_cap[0] - l_host[0]) <= 1e-6 * max(1.0, abs(l_host[0])), (l_cap, l_host)
    assert abs(l_cap[1] - l_host[1]) <= 2e-5 * max(1.0, abs(l_host[1])), (l_cap, l_host)
    assert abs(l_cap[0] - l_cap[1]) > 1e-3                 # different batches and different dropout words per step
    worst = {}
    for k, v in p_cap.items():
        if _zero_by_shift_invariance(k):
            continue      # analytically zero gradient (softmax shift invariance): Adam amplifies its rounding noise to +-lr
        worst[k] = float((v - p_host[k]).abs().max()) / lr
    print("parameters after two steps, max |captured - host clock| / lr:", {k: f"{v:.1e}" for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if not v <= 0.05}
    assert not bad, bad


def _entries_called(monkeypatch, cfg, D=48, N=20):
    from isic_hip import ops
    m, _ = _model(cfg, D)
    served = []
    real_call = ops.call

    def spy(name, *a, **kw):
        rc = real_call(name, *a, **kw)
        served.append(name)                                   # reached only when the entry did not raise
        return rc
    monkeypatch.setattr(ops, "call", spy)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, D, generator=gen).to(DEV).requires_grad_(True)
    probs, _ = m(x, _rand_graph(N, 4 * N, gen).to(DEV))
    ops.cross_entropy_from_probs(probs.unsqueeze(0), torch.tensor([LABEL], device=DEV)).backward()
    torch.cuda.synchronize()
    return served


def test_dispatch_the_narrow_model_calls_no_wide_entry_and_the_wide_models_do(monkeypatch):
    narrow = _entries_called(monkeypatch, _cfg(dict(gnn_type="gat", gnn_hidden=64, gnn_heads=4, gnn_layers=2, att_heads=4)))
    assert not any(n in narrow for n in WIDE) and "isic_layernorm_bwd_wide_workspace_bytes" not in narrow
    assert {"isic_attn_pool_fwd", "isic_layernorm_bwd_ws"} <= set(narrow)
    assert "isic_attn_pool_bwd" in narrow or "isic_attn_pool_bwd_sums" in narrow
    monkeypatch.undo()
    wide = _entries_called(monkeypatch, _cfg(CONFIGS["gat-288x4-att8"]))
    assert set(WIDE) <= set(wide)
    assert not any(n in wide for n in ("isic_attn_pool_fwd", "isic_attn_pool_bwd", "isic_attn_pool_bwd_sums", "isic_layernorm_bwd_ws"))
    monkeypatch.undo()
    heads8 = _entries_called(monkeypatch, _cfg(CONFIGS["gcn-64-att8"]))         # ordinary width, eight pooling heads
    assert "isic_attn_pool_fwd" in heads8 and "isic_attn_pool_wide_bwd" in heads8
    assert "isic_attn_pool_wide_fwd" not in heads8 and "isic_layernorm_bwd_wide_ws" not in heads8
