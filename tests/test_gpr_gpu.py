"""GPR-GNN / APPNP on the device, everything through the C ABI (include/isic_hip_gpr.h): the graph-resident K-hop kernel and
its backward against the fp64 restatement (tests/gpr_ref.py) under a derived dot-product bound, bit-reproducibility, the
bookkeeping of bad graphs, the composed fallback, and ``GraphMIL(gnn_type='gprgnn' | 'appnp')`` forward and backward."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gpr_ref as R  # noqa: E402
from helpers import assert_close, stop_after_a_device_error  # noqa: E402
from oracle import formula  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0


@pytest.fixture(autouse=True)
def _no_gpu_work_after_a_device_error():
    yield
    stop_after_a_device_error()


# ---------------------------------------------------------------------------------------------- the kernel's batch, built once
class _Batch:
    """The batch of gpr_ref.kernel_batch on the device, with the device's own CSR values read back: the bound is about the
    K-hop sums, so the fp64 restatement takes A^ exactly as the kernel holds it (fp32 values are exact in fp64; the CSR build
    has its own tests in test_graph_gpu.py, and ``adjacency_close`` below compares it with the per-edge loop once)."""

    def __init__(self):
        from isic_hip.bags import BagOffsets
        from isic_hip.graph import GraphBatch
        self.sizes, self.offsets, self.eis, self.ews = R.kernel_batch()
        ei, ew = R.batch_edges(self.offsets, self.eis, self.ews)
        self.N = self.offsets[-1]
        self.graph = GraphBatch(ei.to(DEV), self.N, ew.to(DEV))
        self.offs = BagOffsets(self.offsets, DEV)
        self.A = self._dense(self.graph.rowptr, self.graph.col, self.graph.val)          # per graph, row = destination
        self.At = self._dense(self.graph.rowptr_t, self.graph.col_t, self.graph.val_t)   # per graph, row = source
        self.d = int(torch.diff(self.graph.rowptr).max())
        self.d_t = int(torch.diff(self.graph.rowptr_t).max())

    def _dense(self, rowptr, col, val):
        rp, c, v = rowptr.cpu().long(), col.cpu().long(), val.cpu().double()
        row = torch.repeat_interleave(torch.arange(self.N), torch.diff(rp))
        out = []
        for lo, hi in zip(self.offsets[:-1], self.offsets[1:]):
            sel = (row >= lo) & (row < hi)
            assert bool(((c[sel] >= lo) & (c[sel] < hi)).all())
            out.append(torch.zeros((hi - lo, hi - lo), dtype=torch.float64)
                       .index_put_((row[sel] - lo, c[sel] - lo), v[sel], accumulate=True))
        return out


@pytest.fixture(scope="module")
def batch():
    return _Batch()


def _inputs(N, F, K, seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(N, F, generator=gen), torch.randn(N, F, generator=gen), torch.randn(F, generator=gen),
            R.mixed_sign_gamma(K, seed))


def _forward_ref(b, h, gamma, bias):
    zs, bs = [], []
    for g, (lo, hi) in enumerate(zip(b.offsets[:-1], b.offsets[1:])):
        hg = h[lo:hi].double()
        zs.append(R.gpr_propagate(hg, b.A[g], gamma.double(), bias.double() if bias is not None else None))
        bs.append(R.propagate_bound(hg, b.A[g], gamma.double(), b.d, bias.double() if bias is not None else None)[0])
    return torch.cat(zs), torch.cat(bs)


def _backward_ref(b, dz, h, gamma):
    K = gamma.numel() - 1
    dhs, bhs = [], []
    dg, dgb = torch.zeros(K + 1, dtype=torch.float64), torch.zeros(K + 1, dtype=torch.float64)
    for g, (lo, hi) in enumerate(zip(b.offsets[:-1], b.offsets[1:])):
        dzg, hg = dz[lo:hi].double(), h[lo:hi].double()
        dhs.append(R.gpr_propagate(dzg, b.At[g], gamma.double()))
        bhs.append(R.propagate_bound(dzg, b.At[g], gamma.double(), b.d_t)[0])
        ref, bound = R.dgamma_ref_and_bound(dzg, b.At[g].t(), hg, K, b.d_t, dot_len=dz.numel())
        dg, dgb = dg + ref, dgb + bound
    return torch.cat(dhs), torch.cat(bhs), dg, dgb


def _inside(got, ref, bound, what):
    err = (got.detach().cpu().double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{what}: worst error / bound {ratio:.3f}"


def test_adjacency_close(batch):
    """the device's A^ against the per-edge loop of the restatement (fp32 normalisation: a few ulps per entry)"""
    for n, ei, ew, A in zip(batch.sizes, batch.eis, batch.ews, batch.A):
        ref = R.dense_adj(ei, n, ew)
        assert A.shape == ref.shape and float((A - ref).abs().max() if n else 0.0) <= 2e-6
    assert batch.d == 17 and batch.d_t > 64                      # the repeated edges; a hub row of the transpose
    assert batch.A[2][5].count_nonzero() == 1                    # no in-edge beyond the self loop


@pytest.mark.parametrize("K", R.KERNEL_K)
@pytest.mark.parametrize("F", R.KERNEL_F)
def test_kernel_against_the_fp64_restatement(batch, F, K):
    """Z, dH and dgamma of the resident kernel inside the dot-product bound -- any summation order, any FMA contraction:
    |Z^ - Z| <= sum_k c(k (d + 1) + K + 3) |gamma[k]| |A^|^k |H| + u |bias|, c(m) = m u / (1 - m u), u = 2^-24, d the longest
    CSR row of the batch; dH likewise on the transpose; dgamma with N F more roundings."""
    from isic_hip.graph import gpr_prop
    h, dz, bias, gamma = _inputs(batch.N, F, K, seed=100 * F + K)
    hd, bd, gd = (t.to(DEV).requires_grad_(True) for t in (h, bias, gamma))
    z = gpr_prop(hd, gd, batch.graph, batch.offs, bias=bd, resident=True)
    z.backward(dz.to(DEV))
    ref, bound = _forward_ref(batch, h, gamma, bias)
    _inside(z, ref, bound, "Z")
    dh, bh, dg, dgb = _backward_ref(batch, dz, h, gamma)
    _inside(hd.grad, dh, bh, "dH")
    _inside(gd.grad, dg, dgb, "dgamma")
    # (the dgamma bound is loose by its N F term; next to it, the tolerance of the existing SpMM tests, test_graph_gpu.py)
    assert_close(gd.grad, dg, rtol=2e-5, atol=2e-6, what="dgamma (relative to its largest entry)")
    assert_close(bd.grad, dz.double().sum(0), rtol=2e-5, atol=2e-5, what="dbias")
    # gamma without a gradient (appnp): the same Z and dH, no dgamma
    h2 = h.to(DEV).requires_grad_(True)
    z2 = gpr_prop(h2, gamma.to(DEV), batch.graph, batch.offs, bias=bias.to(DEV), resident=True)
    z2.backward(dz.to(DEV))
    assert torch.equal(z2, z) and torch.equal(h2.grad, hd.grad)


def test_two_identical_calls_give_identical_bits(batch):
    from isic_hip.graph import gpr_prop
    h, dz, bias, gamma = _inputs(batch.N, 68, 10, seed=5)
    outs = []
    for _ in range(2):
        hd, bd, gd = (t.to(DEV).requires_grad_(True) for t in (h, bias, gamma))
        z = gpr_prop(hd, gd, batch.graph, batch.offs, bias=bd, resident=True)
        z.backward(dz.to(DEV))
        outs.append((z.detach(), hd.grad, gd.grad, bd.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_composed_path_agrees_with_the_resident_kernel(batch):
    """the two paths within the SUM of their bounds (the composed one is K fp32 SpMMs: the same dot products)"""
    from isic_hip.graph import gpr_prop
    h, dz, bias, gamma = _inputs(batch.N, 36, 10, seed=6)
    res = {}
    for resident in (True, False):
        hd, bd, gd = (t.to(DEV).requires_grad_(True) for t in (h, bias, gamma))
        z = gpr_prop(hd, gd, batch.graph, batch.offs, bias=bd, resident=resident)
        z.backward(dz.to(DEV))
        res[resident] = (z.detach().cpu().double(), hd.grad.cpu().double(), gd.grad.cpu().double())
    _, bound = _forward_ref(batch, h, gamma, bias)
    _, bh, _, dgb = _backward_ref(batch, dz, h, gamma)
    for a, b, bnd, what in zip(res[True], res[False], (bound, bh, dgb), ("Z", "dH", "dgamma")):
        assert bool(((a - b).abs() <= 2 * bnd).all()), what


def test_bad_graphs_are_counted_and_write_nothing():
    """one graph whose offsets span 257 nodes and one that holds a column id of its neighbour: bad[0] == 2, their rows keep
    the sentinel, every other graph is inside the bound; the Python wrapper raises"""
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import GraphBatch, gpr_prop
    from isic_hip.lib import call
    sizes = [10, 257, 12, 12, 7]
    _, offsets, eis, ews = R.kernel_batch(seed=3, sizes=sizes, k=4)
    eis[3] = torch.cat([eis[3], torch.tensor([[-2], [4]])], dim=1)       # source: local -2 = node 10 of graph 2
    ei, _ = R.batch_edges(offsets, eis, ews)
    N, F, K = offsets[-1], 36, 3
    graph = GraphBatch(ei.to(DEV), N)
    h, dz, bias, gamma = _inputs(N, F, K, seed=7)
    off_dev = torch.tensor(offsets, device=DEV)
    z = torch.full((N, F), SENTINEL, device=DEV)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    call("isic_gpr_prop_f32", graph.rowptr, graph.col, graph.val, int(graph.col.numel()), off_dev, len(sizes), 256, N, h.to(DEV),
         gamma.to(DEV), K, F, bias.to(DEV), z, bad)
    assert int(bad.item()) == 2
    rp, c, v = graph.rowptr.cpu().long(), graph.col.cpu().long(), graph.val.cpu().double()
    row = torch.repeat_interleave(torch.arange(N), torch.diff(rp))
    d = int(torch.diff(rp).max())
    for g, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
        if g in (1, 3):
            assert bool((z[lo:hi] == SENTINEL).all()), g
            continue
        sel = (row >= lo) & (row < hi)
        A = torch.zeros((hi - lo, hi - lo), dtype=torch.float64).index_put_((row[sel] - lo, c[sel] - lo), v[sel], accumulate=True)
        ref = R.gpr_propagate(h[lo:hi].double(), A, gamma.double(), bias.double())
        bound = R.propagate_bound(h[lo:hi].double(), A, gamma.double(), d, bias.double())[0]
        _inside(z[lo:hi], ref, bound, f"graph {g}")
    # the backward: graph 1 is bad by its offsets; in the TRANSPOSED CSR the stray edge sits in a row of graph 2
    dh = torch.full((N, F), SENTINEL, device=DEV)
    dg = torch.full((K + 1,), SENTINEL, device=DEV)
    bad.zero_()
    nbytes = int(call("isic_gpr_prop_bwd_workspace_bytes", len(sizes), K, F))
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    call("isic_gpr_prop_bwd_f32", graph.rowptr_t, graph.col_t, graph.val_t, int(graph.col_t.numel()), off_dev, len(sizes), 256, N,
         dz.to(DEV), h.to(DEV), gamma.to(DEV), K, F, dh, dg, 0.0, ws, nbytes, bad)
    assert int(bad.item()) == 2 and bool(torch.isfinite(dg).all()) and bool((dg != SENTINEL).all())
    for g, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
        assert bool((dh[lo:hi] == SENTINEL).all()) == (g in (1, 2)), g
    # the wrapper: without the 257-node graph the batch is inside the kernel's domain, and the stray column id raises
    keep = [0, 2, 3, 4]
    offs2 = BagOffsets(np.concatenate([[0], np.cumsum([sizes[g] for g in keep])]), DEV)
    ei2, _ = R.batch_edges(offs2.host.tolist(), [eis[g] for g in keep], [None] * 4)
    g2 = GraphBatch(ei2.to(DEV), offs2.total)
    with pytest.raises(ValueError, match="column id"):
        gpr_prop(h[:offs2.total].to(DEV), gamma.to(DEV), g2, offs2, resident=True)


def test_a_graph_whose_row_pointers_are_wrong_is_counted_and_writes_nothing():
    """the row-pointer checks of both entries: in the forward a row pointer of graph 1 above its successor, in the backward a
    row pointer of graph 2 (transposed CSR) beyond nnz.  bad == 1, the graph's rows of Z / dH keep the sentinel, the other
    graphs' rows are the bits of a clean run, dgamma is finite"""
    from isic_hip.graph import GraphBatch
    from isic_hip.lib import call
    sizes = [10, 12, 7]
    _, offsets, eis, ews = R.kernel_batch(seed=3, sizes=sizes, k=4)
    ei, _ = R.batch_edges(offsets, eis, ews)
    N, F, K = offsets[-1], 36, 3
    graph = GraphBatch(ei.to(DEV), N)
    h, dz, bias, gamma = (t.to(DEV) for t in _inputs(N, F, K, seed=9))
    off_dev = torch.tensor(offsets, device=DEV)
    nnz, nnz_t = int(graph.col.numel()), int(graph.col_t.numel())
    nbytes = int(call("isic_gpr_prop_bwd_workspace_bytes", len(sizes), K, F))
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)

    def forward(rowptr):
        z = torch.full((N, F), SENTINEL, device=DEV)
        bad = torch.zeros(1, device=DEV, dtype=torch.int32)
        call("isic_gpr_prop_f32", rowptr, graph.col, graph.val, nnz, off_dev, len(sizes), 256, N, h, gamma, K, F, bias, z, bad)
        return z, int(bad.item())

    def backward(rowptr_t):
        dh = torch.full((N, F), SENTINEL, device=DEV)
        dg = torch.full((K + 1,), SENTINEL, device=DEV)
        bad = torch.zeros(1, device=DEV, dtype=torch.int32)
        call("isic_gpr_prop_bwd_f32", rowptr_t, graph.col_t, graph.val_t, nnz_t, off_dev, len(sizes), 256, N, dz, h, gamma, K, F,
             dh, dg, 0.0, ws, nbytes, bad)
        return dh, dg, int(bad.item())

    rp, rpt = graph.rowptr.clone(), graph.rowptr_t.clone()
    rp[offsets[1] + 2] = rp[offsets[1] + 3] + 1
    rpt[offsets[2] + 3] = nnz_t + 1000
    good_z, n_bad = forward(graph.rowptr)
    assert n_bad == 0 and bool((good_z != SENTINEL).all())
    good_dh, _, n_bad = backward(graph.rowptr_t)
    assert n_bad == 0 and bool((good_dh != SENTINEL).all())
    z, n_bad = forward(rp)
    dh, dg, n_bad_t = backward(rpt)
    assert n_bad == 1 and n_bad_t == 1
    assert bool(torch.isfinite(dg).all()) and bool((dg != SENTINEL).all())
    for out, good, refused in ((z, good_z, 1), (dh, good_dh, 2)):
        for g, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
            if g == refused:
                assert bool((out[lo:hi] == SENTINEL).all()), g
            else:
                assert torch.equal(out[lo:hi], good[lo:hi]), g


def test_a_graph_beyond_256_nodes_takes_the_composed_path():
    from isic_hip import graph as G
    from isic_hip.bags import BagOffsets
    n, F, K = 300, 8, 3
    _, offsets, eis, ews = R.kernel_batch(seed=4, sizes=[n], k=6)
    gb = G.GraphBatch(eis[0].to(DEV), n)
    h, dz, bias, gamma = _inputs(n, F, K, seed=8)
    hd, gd = h.to(DEV).requires_grad_(True), gamma.to(DEV).requires_grad_(True)
    z = G.gpr_prop(hd, gd, gb, BagOffsets(offsets, DEV), bias=bias.to(DEV), resident=True)
    assert G.gpr_last_path() == "composed"
    z.backward(dz.to(DEV))
    A = R.dense_adj(eis[0], n)
    ref = R.gpr_propagate(h.double(), A, gamma.double(), bias.double())
    assert_close(z, ref, rtol=2e-5, atol=2e-6, what="composed Z")
    assert_close(hd.grad, R.gpr_propagate(dz.double(), A.t(), gamma.double()), rtol=2e-5, atol=2e-6, what="composed dH")
    assert_close(gd.grad, R.dgamma_ref_and_bound(dz.double(), A, h.double(), K, 1)[0], rtol=2e-5, atol=2e-6, what="composed dgamma")
    G.gpr_prop(h[:200].to(DEV), gamma.to(DEV), G.GraphBatch(R.kernel_batch(seed=4, sizes=[200], k=6)[2][0].to(DEV), 200),
               BagOffsets([0, 200], DEV), resident=True)
    assert G.gpr_last_path() == "resident"
    G.gpr_prop(h[:200].to(DEV), gamma.to(DEV), G.GraphBatch(R.kernel_batch(seed=4, sizes=[200], k=6)[2][0].to(DEV), 200),
               None, resident=True)
    assert G.gpr_last_path() == "composed"                       # no per-graph offsets


# ---------------------------------------------------------------------------------------------- the whole model
FWD_TOL = dict(rtol=5e-5, atol=2e-6)        # tests/test_graph_gpu.py, whole-model forward
GRAD_TOL = dict(rtol=5e-4, atol=3e-6)       # ... gradients
CFG = dict(gnn_layers=2, att_heads=4, use_layer_norm=True, use_residual=True)


def _model(gtype, seed=0, **kw):
    from gnn_models import GraphMIL
    m = GraphMIL(32, gtype, 64, 2, gpr_k=4, **kw)
    p = formula.formula_state_dict(formula.shapes_of(m))
    for i in range(2):
        # gprgnn: coefficients of mixed sign, as trained ones are; appnp keeps the PPR buffer it was built with
        p[f"gnn_layers.{i}.gamma"] = R.mixed_sign_gamma(4, seed + i) if gtype == "gprgnn" else m.gnn_layers[i].gamma.clone()
    m.load_state_dict(p)
    return m.to(DEV).eval(), p


def _graphs(sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    _, offsets, eis, _ = R.kernel_batch(seed=seed, sizes=sizes, k=8)
    return offsets, eis, [torch.randn(n, 32, generator=gen) for n in sizes]


@pytest.mark.parametrize("resident", (True, False))
@pytest.mark.parametrize("sizes", ([196], [196, 40, 1, 133, 77]))
@pytest.mark.parametrize("gtype", ("gprgnn", "appnp"))
def test_graphmil_against_the_restatement(gtype, sizes, resident):
    """probs, attention and every parameter gradient (gnn_layers.*.gamma included) of GraphMIL(32, t, 64, 2, gpr_k=4) in eval
    mode, one 196-node graph and a batch of 5 graphs of unequal size, against tests/gpr_ref.py in fp64, at the tolerances of
    the existing whole-model tests (tests/test_graph_gpu.py: rtol 5e-5 / atol 2e-6 forward, rtol 5e-4 / atol 3e-6
    gradients, relative to the largest entry of each tensor)."""
    from isic_hip import ops
    m, p = _model(gtype)
    m.gpr_resident = resident
    offsets, eis, xs = _graphs(sizes, seed=11)
    ys = [(3 * g + 1) % 7 for g in range(len(sizes))]
    loss_o, probs_o, att_o, grads_o = R.graphmil_batch_loss_and_grads(p, CFG, xs, eis, ys)
    xd = torch.cat(xs).to(DEV).requires_grad_(True)
    ei = torch.cat([e + o for e, o in zip(eis, offsets[:-1])], dim=1).to(DEV)
    if len(sizes) == 1:
        probs, att = m(xd, ei)
        probs = probs.unsqueeze(0)
    else:
        probs, att = m(xd, ei, offsets=np.asarray(offsets))
    assert_close(probs, probs_o, what="probs", **FWD_TOL)
    assert_close(att, att_o, what="att", **FWD_TOL)
    loss = ops.cross_entropy_from_probs(probs, torch.tensor(ys, device=DEV))
    assert_close(loss, loss_o, rtol=5e-5)
    loss.backward()
    named = dict(m.named_parameters())
    assert ("gnn_layers.0.gamma" in named) == (gtype == "gprgnn")
    for k, prm in named.items():
        if k.startswith("attention_layers") and k.endswith("2.bias"):
            continue                                             # analytically zero (softmax shift invariance)
        assert_close(prm.grad, grads_o[k], what=k, **GRAD_TOL)
    assert_close(xd.grad, torch.cat(grads_o["x"]), what="x", **GRAD_TOL)
    if gtype == "appnp":
        assert m.gnn_layers[0].gamma.grad is None and not m.gnn_layers[0].gamma.requires_grad


def test_appnp_gamma_is_untouched_by_an_optimiser_step():
    from isic_hip import optim
    m, p = _model("appnp")
    m.gpr_resident = True
    offsets, eis, xs = _graphs([50, 31], seed=12)
    before = [m.gnn_layers[i].gamma.clone() for i in range(2)]
    opt = optim.AdamW(m.parameters(), lr=1e-2, weight_decay=1e-2)
    opt.zero_grad()
    ei = torch.cat([e + o for e, o in zip(eis, offsets[:-1])], dim=1).to(DEV)
    _, _, loss = m(torch.cat(xs).to(DEV), ei, offsets=np.asarray(offsets), labels=torch.tensor([1, 2], device=DEV))
    loss.backward()
    opt.step()
    for i in range(2):
        assert m.gnn_layers[i].gamma.grad is None and torch.equal(m.gnn_layers[i].gamma, before[i])
    assert not torch.equal(m.gnn_layers[0].lin.weight.detach().cpu(), p["gnn_layers.0.lin.weight"])


def test_lesion_only_store_batch_equals_the_single_graph_forwards():
    import build_graphs as bg
    from isic_hip import train as T
    rng = np.random.default_rng(4)
    side, D = 6, 32
    n = side * side
    ei = bg._grid_edge_index(True, side=side).numpy()
    r, c = np.divmod(np.arange(n), side)
    recs = []
    for i in range(8):
        cy, cx, ry, rx = rng.uniform(1.5, side - 2.5, 2).tolist() + rng.uniform(1.0, 2.6, 2).tolist()
        keep = ((r - cy) / ry) ** 2 + ((c - cx) / rx) ** 2 <= 1.0
        recs.append({"x": rng.standard_normal((n, D)).astype(np.float32), "edge_index": ei.copy(), "y": i % 3, "keep": keep})
    store = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True)
    m, _ = _model("gprgnn")
    m.gpr_resident = True
    x, offs, graph = store.batch(list(range(8)))
    assert len(set(np.diff(offs.host).tolist())) > 2             # graphs of unequal size
    probs = m(x, offsets=offs, graph=graph)[0]
    for i in range(8):
        xi, oi, gi = store.batch([i])
        assert_close(probs[i], m(xi, graph=gi)[0], what=f"record {i}", **FWD_TOL)


def test_three_adamw_steps_change_gamma_and_repeat_bit_for_bit():
    from gnn_models import GraphMIL
    from isic_hip import optim
    sizes = [40 + 3 * g for g in range(16)]
    offsets, eis, xs = _graphs(sizes, seed=13)
    x = torch.cat(xs).to(DEV)
    ei = torch.cat([e + o for e, o in zip(eis, offsets[:-1])], dim=1).to(DEV)
    y = torch.tensor([g % 7 for g in range(16)], device=DEV)

    def run():
        torch.manual_seed(5)
        m = GraphMIL(32, "gprgnn", 64, 2, gpr_k=4).to(DEV).train()
        m.gpr_resident = True
        m.set_dropout_state(9, 0)
        g0 = m.gnn_layers[0].gamma.detach().clone()
        opt = optim.AdamW(m.parameters(), lr=1e-2, weight_decay=1e-4)
        for _ in range(3):
            opt.zero_grad()
            _, _, loss = m(x, ei, offsets=np.asarray(offsets), labels=y)
            loss.backward()
            opt.step()
        return g0, {k: v.detach().clone() for k, v in m.state_dict().items()}

    g0, a = run()
    _, b = run()
    assert not torch.equal(a["gnn_layers.0.gamma"], g0) and bool(torch.isfinite(a["gnn_layers.0.gamma"]).all())
    for k in a:
        assert torch.equal(a[k], b[k]), k
