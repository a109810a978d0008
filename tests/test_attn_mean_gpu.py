"""Head-averaged attention (``concat=False``) on the MI355X: the four ``isic_*_mean`` entries through the C ABI against
the fp64 reference and derived bounds of tests/attn_mean_ref.py (tests/test_attn_mean_cpu.py shows on the CPU that the
bounds admit a correct fp32 evaluation and reject the wrong variants), GraphMIL(gnn_concat=False) against the model-level
restatement, its batch form, and one epoch of the packaged fold loop.

Kernel template instantiation -> a case that launches it:
  gat_fwd / gat_bwd_dst / gat_bwd_src <MEAN>                    gat-*: head sum and dout row in registers (F <= 256)
  edge_attn_fwd / _bwd_dst / _bwd_src <0|1, MEAN>               gatv2-* | dot-*: registers up to F 168, the read-modify-write of
                                                                the out row and the re-read dout row at F 257; d att in
                                                                registers up to H8-F130, atomic at H4-F257 and H6-F168
Rows of 1 ... 700 stored entries: both sides of the 512 entries kept in LDS, in both sweeps.

Worst device error / bound ratio over the case list, MI355X: out 0.19, alpha 0.05, every gradient at most 0.04 (the table
per layer is printed at the module's end, visible with -s)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_mean_ref as A  # noqa: E402
import f32_kernel_ref as R  # noqa: E402
from helpers import assert_close  # noqa: E402
from oracle import formula  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
PAD = 64
WORST = {}


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        print("worst device ratio", key, {k: round(v, 3) for k, v in WORST[key].items()})


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further GPU work: {e}", returncode=3)


class Guarded:
    """an fp32 output of `shape`, NaN pre-filled, with PAD NaN floats before and after it"""

    def __init__(self, shape, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((2 * PAD + n + 4,), NAN, device=DEV, dtype=torch.float32)
        self.n = n
        self.t = self.buf[PAD:PAD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def ok(self):
        intact = bool(torch.isnan(self.buf[:PAD]).all()) and bool(torch.isnan(self.buf[PAD + self.n:]).all())
        return intact and bool(torch.isfinite(self.t).all())

    def cpu(self):
        return self.t.detach().cpu()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ================================================================== 1. the kernels over their domain, through the C ABI
_CSR = {}


def _build_csr(inp, mode):
    """isic_gcn_csr_build on the device (compared with the numpy CSR in tests/test_f32_kernel_domain_gpu.py; here the
    structure arrays are checked again because everything below indexes through them)"""
    key = (inp.n, mode)
    if key in _CSR:
        return _CSR[key]
    src, dst, w, n = inp.src, inp.dst, inp.w, inp.n
    E, ref = int(src.size), inp.csr
    cap = E + n
    mk = lambda m: torch.full((m + 8,), -7, device=DEV, dtype=torch.int32)      # noqa: E731
    d = R.Box(rowptr=mk(n + 1), col=mk(cap), rowptr_t=mk(n + 1), col_t=mk(cap), perm_t=mk(cap),
              val=torch.full((cap + 8,), NAN, device=DEV), val_t=torch.full((cap + 8,), NAN, device=DEV))
    nbytes = _call("isic_gcn_csr_workspace_bytes", n, E)
    ws = torch.empty(max(int(nbytes), 16) + 16, device=DEV, dtype=torch.uint8)
    _call("isic_gcn_csr_build", torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV),
          torch.from_numpy(w).to(DEV) if w is not None else None, E, n, mode, d.rowptr, d.col, d.val, d.rowptr_t, d.col_t,
          d.val_t, d.perm_t, ws, nbytes)
    for name in ("rowptr", "rowptr_t"):
        assert np.array_equal(d[name][:n + 1].cpu().numpy(), ref[name]), name
    for name in ("col", "col_t", "perm_t"):
        assert np.array_equal(d[name][:ref.nnz].cpu().numpy(), ref[name]), name
    _CSR[key] = d
    return d


def _mean_run(inp, d):
    """one forward and one backward of the case's head-mean entries -> outputs on the CPU"""
    layer, n, H, F = inp.layer, inp.n, inp.H, inp.F
    nnz = inp.csr.nnz
    drop = (R.drop_threshold(inp.p), inp.scale, R.ATT_SEED, R.ATT_STREAM)
    dout, bias = _dev(inp.dmean), _dev(inp.bias_f)
    node = lambda: Guarded((n, H, F))            # noqa: E731
    out, alpha, de = Guarded((n, F)), Guarded((nnz, H)), Guarded((nnz, H))
    o = dict(out=out, alpha=alpha, de=de)
    if layer == "gat":
        xp, al, ar = _dev(inp.xp), _dev(inp.al), _dev(inp.ar)
        dar, dal, dxp = Guarded((n, H)), Guarded((n, H)), node()
        _call("isic_gat_fwd_mean", xp, al, ar, d.rowptr, d.col, bias, out.t, alpha.t, n, H, F, R.ATT_SLOPE, *drop)
        _call("isic_gat_bwd_mean", dout, xp, alpha.t, al, ar, _dev(inp.att_src), _dev(inp.att_dst), d.rowptr, d.col, d.rowptr_t,
              d.col_t, d.perm_t, de.t, dar.t, dal.t, dxp.t, n, H, F, R.ATT_SLOPE, *drop)
        o.update(dar=dar, dal=dal, dxp=dxp)
    else:
        mode = 0 if layer == "gatv2" else 1
        ks, qd = _dev(inp.ks), _dev(inp.qd)
        v = ks if mode == 0 else _dev(inp.v)
        att = _dev(inp.att) if mode == 0 else None
        dqd, dks = node(), node()
        dv = node() if mode == 1 else None
        datt = Guarded((H, F), init=torch.zeros(H, F)) if mode == 0 else None
        _call("isic_edge_attn_fwd_mean", mode, ks, qd, v, att, d.rowptr, d.col, bias, out.t, alpha.t, n, H, F, R.ATT_SLOPE,
              inp.dot_scale, *drop)
        _call("isic_edge_attn_bwd_mean", mode, dout, ks, qd, v, att, alpha.t, d.rowptr, d.col, d.rowptr_t, d.col_t, d.perm_t,
              de.t, dqd.t, dks.t, None if dv is None else dv.t, None if datt is None else datt.t, n, H, F, R.ATT_SLOPE,
              inp.dot_scale, *drop)
        o.update(dqd=dqd, dks=dks)
        if dv is not None:
            o["dv"] = dv
        if datt is not None:
            o["datt"] = datt
    assert all(g.ok() for g in o.values()), [k for k, g in o.items() if not g.ok()]
    return {k: g.cpu() for k, g in o.items()}


@pytest.mark.parametrize("case", A.MEAN_CASES, ids=[c["id"] for c in A.MEAN_CASES])
def test_head_mean_entries_forward_and_backward(case):
    inp = A.mean_inputs(case)
    layer, n, H, F = inp.layer, inp.n, inp.H, inp.F
    mode = R.att_csr_mode(layer)
    d = _build_csr(inp, mode)
    if layer == "gat":                                     # the device's own fp32 scores are the layer's inputs
        al, ar = Guarded((n, H)), Guarded((n, H))
        _call("isic_gat_scores", _dev(inp.xp), _dev(inp.att_src), _dev(inp.att_dst), al.t, ar.t, n, H, F)
        assert al.ok() and ar.ok()
        inp.al, inp.ar = al.cpu(), ar.cpu()
    assert R.att_zero_pre_share(inp) <= R.AMBIGUOUS_CAP
    ref, b = A.mean_reference(inp)
    got = _mean_run(inp, d)
    assert set(got) == set(b), sorted(set(got) ^ set(b))
    ratios = A.mean_ratios(got, ref, b)
    print(case["id"], " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    w = WORST.setdefault((layer, f"p{inp.p}"), {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), v)
    assert all(v <= 1.0 for v in ratios.values()), (case["id"], ratios)
    if layer == "dot" and n == R.ATT_N:                    # a node without incoming edges: out = bias, zero gradients
        assert int(inp.csr.cnt_in[0]) == 0
        assert torch.equal(got["out"][0], inp.bias_f) and bool((got["dqd"][0] == 0).all())
    again = _mean_run(inp, d)                              # bit-equal, except datt (every path ends in fp32 atomics)
    for k, v in again.items():
        if k != "datt":
            assert torch.equal(_bits(v), _bits(got[k])), k


# ================================================================== 2. the whole model against the restatement
def _model(gtype, D, F_, heads, L=2, dropout=0.5):
    from gnn_models import GraphMIL
    return GraphMIL(input_dim=D, gnn_type=gtype, gnn_hidden=F_, gnn_layers=L, gnn_dropout=dropout, gnn_heads=heads,
                    gnn_concat=False, att_dim=16, att_heads=4, pool_dropout=0.2, classifier_dim=24, classifier_light=True,
                    num_classes=7)


@pytest.mark.parametrize("gtype,F_,heads", [("gat", 64, 4), ("gat", 32, 8), ("gatv2", 64, 4), ("gatv2", 168, 6),
                                            ("transformer", 32, 4), ("transformer", 48, 2)])
def test_graphmil_without_concat_vs_restatement(gtype, F_, heads):
    """forward + every gradient vs tests/attn_mean_ref.graphmil_mean_forward (PARITY UNPINNED: torch_geometric absent) on
    the graph of test_graphmil_edge_attention_models_vs_oracle: k-NN with nodes stripped of their incoming edges, added
    self loops and duplicated edges; then train mode with the oracle's Philox streams.  That test's tolerances."""
    import build_graphs as bg
    from isic_hip import ops
    N, D, L = 150, 40, 2
    cfg = dict(gnn_type=gtype, gnn_hidden=F_, gnn_layers=L, gnn_heads=heads, att_dim=16, classifier_dim=24)
    shapes = A.graphmil_mean_shapes(D, cfg)
    p = formula.formula_state_dict(shapes)
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(6))
    ei = bg._knn_edge_index(x, 5).cpu()
    ei = ei[:, ei[1] % 7 != 3]
    ei = torch.cat([ei, torch.tensor([[2, 9, 9], [2, 9, 17]]), ei[:, :4]], dim=1)
    loss_o, out_o, grads_o = A.graphmil_mean_loss_and_grads(p, cfg, x, ei, 2)
    m = _model(gtype, D, F_, heads, L)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(shapes.items())
    m.load_state_dict(p)
    m = m.to(DEV).eval()
    xd = x.to(DEV).requires_grad_(True)
    probs, att = m(xd, ei.to(DEV))
    assert m.last_node_embeddings.shape == (N, F_)
    assert_close(probs, out_o["probs"], rtol=5e-5, atol=2e-6, what="probs")
    assert_close(att, out_o["att"], rtol=5e-5, atol=2e-6, what="att")
    assert_close(m.last_node_embeddings, out_o["hs"][-1], rtol=5e-5, atol=5e-6, what="node embeddings")
    loss = ops.cross_entropy_from_probs(probs.unsqueeze(0), torch.tensor([2], device=DEV))
    assert_close(loss, loss_o, rtol=5e-5)
    loss.backward()
    for k, prm in m.named_parameters():
        if k.startswith("attention_layers") and k.endswith("2.bias"):
            continue
        assert_close(prm.grad, grads_o[k], rtol=5e-4, atol=3e-6, what=k)
    assert_close(xd.grad, grads_o["x"], rtol=5e-4, atol=3e-6, what="x")
    m.train()
    m.set_dropout_state(seed=55, step=1)
    pr, _ = m(x.to(DEV), ei.to(DEV))
    o = A.graphmil_mean_forward(p, dict(cfg, gnn_dropout=0.5, pool_dropout=0.2), x, ei, drop={"seed": 55, "stream_base": 1024})
    assert_close(pr, o["probs"], rtol=5e-5, atol=2e-6, what="dropout probs")


# ================================================================== 3. batch form
@pytest.mark.parametrize("gtype", ("gat", "gatv2", "transformer"))
def test_batched_graphs_equal_the_per_graph_calls(gtype):
    D, F_, H = 24, 32, 4
    torch.manual_seed(3)
    m = _model(gtype, D, F_, H).to(DEV).eval()
    gen = torch.Generator().manual_seed(8)
    sizes = [20, 7, 33]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    xs = [torch.randn(n, D, generator=gen) for n in sizes]
    eis = []
    for n in sizes:
        e = torch.randint(0, n, (2, 4 * n), generator=gen)
        eis.append(e[:, e[0] != e[1]])
    big_x = torch.cat(xs).to(DEV)
    big_e = torch.cat([e + int(o) for e, o in zip(eis, offs[:-1])], dim=1).to(DEV)
    probs_b, att_b = m(big_x, big_e, offsets=offs)
    assert probs_b.shape == (3, 7)
    for i, (xg, eg) in enumerate(zip(xs, eis)):
        pr, at = m(xg.to(DEV), eg.to(DEV))
        assert_close(probs_b[i], pr, rtol=1e-5, atol=1e-6, what="batched probs")
        assert_close(att_b[offs[i]:offs[i + 1]], at, rtol=1e-5, atol=1e-6, what="batched att")


# ================================================================== 4. train loop
def test_fold_loop_trains_a_gat_without_concat_and_repeats_bit_for_bit():
    import build_graphs as bg
    from dataset import synthetic_latent_bags
    from isic_hip import train as T
    bags, labels = synthetic_latent_bags(12, 20, 16, classes=7, shift=0.8, seed=5)
    recs = [{"x": b, "edge_index": bg._knn_edge_index(torch.from_numpy(b), 4).numpy(), "y": int(y)} for b, y in zip(bags, labels)]

    def run():
        torch.manual_seed(1)
        m = _model("gat", 16, 16, 4, dropout=0.1)
        p0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
        m = m.to(DEV)
        m.set_dropout_state(7, 0)
        vm, _, _ = T.train_gnn_fold(m, recs[:8], recs[8:], recs[8:], lr=1e-3, epochs=1, graphs_per_step=4, num_classes=7,
                                    device=torch.device(DEV), rng=np.random.RandomState(0))
        return vm, p0, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}

    vm, p0, p1 = run()
    assert np.isfinite(vm["loss"])
    for k, v in p1.items():
        assert bool(torch.isfinite(v).all()) and not torch.equal(v, p0[k]), k
    _, _, p2 = run()
    for k, v in p1.items():
        assert torch.equal(_bits(v), _bits(p2[k])), k
