"""H2GCN on the device, everything through the C ABI (include/isic_hip_h2.h): the 2-hop builder against the numpy restatement
as integers and bits, the bookkeeping of bad graphs, the two-operator propagation and its backward against fp64 under a
derived dot-product bound, and ``GraphMIL(gnn_type='h2gcn')`` / ``GraphStore(mode='h2')`` / ``train_gnn_fold``."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import h2gcn_ref as R  # noqa: E402
from helpers import assert_close, stop_after_a_device_error  # noqa: E402
from oracle import formula  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
ISENT = -7


@pytest.fixture(autouse=True)
def _no_gpu_work_after_a_device_error():
    yield
    stop_after_a_device_error()


# ---------------------------------------------------------------------------------------------- the kernels' batch, built once
class _Batch:
    """The batch of h2gcn_ref.kernel_batch on the device, its pair built by ``two_hop`` and the numpy restatement of both
    operators.  The propagation tests take each operator exactly as the device holds it (fp32 values are exact in fp64): the
    builder has its own bit-exact test below."""

    def __init__(self):
        from isic_hip.bags import BagOffsets
        from isic_hip.graph import GraphBatch, two_hop
        self.sizes, self.offsets, self.eis = R.kernel_batch()
        self.N = int(self.offsets[-1])
        self.graph = GraphBatch(R.batch_edges(self.offsets, self.eis).to(DEV), self.N, mode="sum")
        self.offs = BagOffsets(self.offsets, DEV)
        self.pair = two_hop(self.graph, self.offs)
        self.ref = R.batch_csr(self.offsets, self.eis)
        self.dense = [self._dense(op) for op in (self.pair.a1, self.pair.a2)]           # per operator, per graph
        self.longest = [int(torch.diff(op.rowptr).max()) for op in (self.pair.a1, self.pair.a2)]

    def _dense(self, op):
        rp, c, v = op.rowptr.cpu().long(), op.col.cpu().long(), op.val.cpu().double()
        row = torch.repeat_interleave(torch.arange(self.N), torch.diff(rp))
        out = []
        for lo, hi in zip(self.offsets[:-1].tolist(), self.offsets[1:].tolist()):
            sel = (row >= lo) & (row < hi)
            assert bool(((c[sel] >= lo) & (c[sel] < hi)).all())
            out.append(torch.zeros((hi - lo, hi - lo), dtype=torch.float64)
                       .index_put_((row[sel] - lo, c[sel] - lo), v[sel], accumulate=True))
        return out

    def apply(self, q, x):
        """(A^ x, |A^| |x|) of operator q per graph, fp64"""
        zs, bs = [], []
        for A, lo, hi in zip(self.dense[q], self.offsets[:-1].tolist(), self.offsets[1:].tolist()):
            zs.append(A @ x[lo:hi].double())
            bs.append(A.abs() @ x[lo:hi].double().abs())
        return torch.cat(zs), torch.cat(bs)


@pytest.fixture(scope="module")
def batch():
    return _Batch()


def _c(m):
    return m * R.U32 / (1.0 - m * R.U32)


def _inside(got, ref, bound, what):
    err = (got.detach().cpu().double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{what}: worst error / bound {ratio:.3f}"


# ---------------------------------------------------------------------------------------------- the builder
def _count(graph, off_dev, G, max_nodes, N, deg, bad):
    from isic_hip.lib import call
    call("isic_two_hop_count", graph.rowptr, graph.col, int(graph.col.numel()), off_dev, G, max_nodes, N, deg[0], deg[1], bad)


def _write(graph, off_dev, G, max_nodes, N, rp, nnz, outs, bad):
    from isic_hip.lib import call
    call("isic_two_hop_write", graph.rowptr, graph.col, int(graph.col.numel()), off_dev, G, max_nodes, N, rp[0], rp[1], nnz[0], nnz[1],
         *outs[0], *outs[1], bad)


def test_builder_equals_the_numpy_restatement_as_integers_and_bits(batch):
    deg = torch.full((2, batch.N), ISENT, device=DEV, dtype=torch.int32)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    _count(batch.graph, batch.offs.device, len(batch.sizes), 256, batch.N, deg, bad)
    assert int(bad.item()) == 0
    for q, (op, ref) in enumerate(zip((batch.pair.a1, batch.pair.a2), batch.ref)):
        assert np.array_equal(deg[q].cpu().numpy(), ref["deg"]), q
        assert np.array_equal(op.rowptr.cpu().numpy(), ref["rowptr"]), q
        assert np.array_equal(op.col.cpu().numpy(), ref["col"]), q
        assert np.array_equal(op.perm_t.cpu().numpy(), ref["perm"]), q
        assert np.array_equal(op.val.cpu().numpy().view(np.int32), ref["val"].view(np.int32)), q      # bit for bit
        # perm is an involution that takes the slot of (i, j) to the slot of (j, i)
        col, perm = op.col.long(), op.perm_t.long()
        row = torch.repeat_interleave(torch.arange(batch.N, device=DEV), torch.diff(op.rowptr.long()))
        assert torch.equal(perm[perm], torch.arange(col.numel(), device=DEV))
        assert torch.equal(col[perm], row) and torch.equal(row[perm], col)
        assert op.mode == "sym" and op.rowptr_t is op.rowptr and op.col_t is op.col and op.val_t is op.val
    assert batch.longest[1] == 254 and batch.pair.mode == "h2"          # the leaves of the 256-node star
    star = batch.sizes.index(256)
    lo = int(batch.offsets[star])
    assert int(deg[0][lo]) == 255 and int(deg[1][lo]) == 0 and int(deg[1][lo + 1]) == 254
    full = batch.sizes.index(65)
    assert int(deg[1][int(batch.offsets[full]):int(batch.offsets[full + 1])].max()) == 0   # complete graph: no 2-hop pair


def test_two_builds_give_identical_bytes(batch):
    from isic_hip.graph import two_hop
    again = two_hop(batch.graph, batch.offs)
    for a, b in zip((batch.pair.a1, batch.pair.a2), (again.a1, again.a2)):
        for k in ("rowptr", "col", "perm_t"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert torch.equal(a.val.view(torch.int32), b.val.view(torch.int32))


def test_bad_graphs_are_counted_and_write_nothing():
    """six graphs of 10, 13, 12, 7, 9 and 8 nodes with max_nodes = 12: graph 1 spans 13 nodes, graph 2 holds a column id of
    graph 1, the offsets of graph 5 decrease (its rows belong to no graph then), and -- the write only -- a row pointer of
    graph 3 lies beyond nnz1.  bad == 3 resp. 4, the sentinels of those graphs are untouched, graphs 0 and 4 (and 3 in the
    count) are exact.  No value is used as an index unchecked: the stray column id and the stray row pointer would index
    another graph's bit rows resp. 10^6 entries past the outputs."""
    from isic_hip.graph import GraphBatch
    rng = np.random.default_rng(5)
    sizes = [10, 13, 12, 7, 9, 8]
    true_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    eis = [R.knn_like_edges(n, 4, rng) for n in sizes]
    N = int(true_off[-1])
    ei = R.batch_edges(true_off, eis)
    ei = torch.cat([ei, torch.tensor([[int(true_off[1]) + 2], [int(true_off[2]) + 3]])], dim=1)      # graph 1 -> graph 2
    graph = GraphBatch(ei.to(DEV), N, mode="sum")
    off = true_off.copy()
    off[6] = off[5] - 5                                                   # graph 5: [51, 46)
    off_dev = torch.as_tensor(off, device=DEV)
    ref = R.batch_csr(true_off, eis)
    deg = torch.full((2, N), ISENT, device=DEV, dtype=torch.int32)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    _count(graph, off_dev, 6, 12, N, deg, bad)
    assert int(bad.item()) == 3
    good_count, good_write = (0, 3, 4), (0, 4)
    rows = lambda gs: np.concatenate([np.arange(true_off[g], true_off[g + 1]) for g in gs])
    for q in range(2):
        got = deg[q].cpu().numpy()
        assert np.array_equal(got[rows(good_count)], ref[q]["deg"][rows(good_count)])
        assert (got[rows((1, 2, 5))] == ISENT).all()
    # the write behind the TRUE row pointers, one of graph 3's first operator pushed out of [0, nnz1]
    rp = torch.as_tensor(np.stack([ref[0]["rowptr"], ref[1]["rowptr"]]), dtype=torch.int32).to(DEV)
    nnz = [int(ref[q]["rowptr"][-1]) for q in range(2)]
    rp[0, int(true_off[3]) + 2] = nnz[0] + 1_000_000
    outs = [(torch.full((z,), ISENT, device=DEV, dtype=torch.int32), torch.full((z,), SENTINEL, device=DEV),
             torch.full((z,), ISENT, device=DEV, dtype=torch.int32)) for z in nnz]
    bad.zero_()
    _write(graph, off_dev, 6, 12, N, rp, nnz, outs, bad)
    assert int(bad.item()) == 4
    for q in range(2):
        col, val, perm = (t.cpu().numpy() for t in outs[q])
        slot_rows = np.repeat(np.arange(N), ref[q]["deg"])
        good = np.isin(slot_rows, rows(good_write))
        assert np.array_equal(col[good], ref[q]["col"][good]) and np.array_equal(perm[good], ref[q]["perm"][good])
        assert np.array_equal(val[good].view(np.int32), ref[q]["val"][good].view(np.int32))
        assert (col[~good] == ISENT).all() and (perm[~good] == ISENT).all() and (val[~good] == SENTINEL).all()
    # row pointers inside [0, nnz] that do not belong to the counts: no bad graph, and a store outside its row's segment is dropped
    rp2 = torch.as_tensor(np.stack([ref[0]["rowptr"], ref[1]["rowptr"]]), dtype=torch.int32).to(DEV)
    r0 = int(true_off[4]) + 1
    b, e = int(ref[0]["rowptr"][r0]), int(ref[0]["rowptr"][r0 + 1])
    assert e - b >= 2 and ref[0]["deg"][r0 + 1] >= 1
    rp2[0, r0] = b + 1                                                    # row r0 starts one slot late: its last store would land in row r0 + 1
    outs2 = [(torch.full((z,), ISENT, device=DEV, dtype=torch.int32), torch.full((z,), SENTINEL, device=DEV),
              torch.full((z,), ISENT, device=DEV, dtype=torch.int32)) for z in nnz]
    bad.zero_()
    _write(graph, off_dev, 6, 12, N, rp2, nnz, outs2, bad)
    assert int(bad.item()) == 3
    col = outs2[0][0].cpu().numpy()
    assert col[b] == ISENT and np.array_equal(col[b + 1:e], ref[0]["col"][b:e - 1]) and col[e] == ref[0]["col"][e]
    # the wrapper raises on a refused graph
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import two_hop
    with pytest.raises(ValueError, match="column id"):
        two_hop(graph, BagOffsets(true_off, DEV))


def test_builder_refuses_a_graph_whose_own_row_pointers_are_wrong():
    """the INPUT CSR's row pointers, in count and write: graph 0 holds a row pointer above its successor (row 3 then ends
    before it begins), graph 2 ends beyond nnz, graph 3 holds a negative one.  bad == 3, their outputs keep the sentinel,
    graph 1 is exact.  A row pointer is compared with the graph's entry range before it bounds a loop over col."""
    from types import SimpleNamespace
    from isic_hip.graph import GraphBatch
    rng = np.random.default_rng(6)
    sizes = [10, 12, 9, 11]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    eis = [R.knn_like_edges(n, 4, rng) for n in sizes]
    N = int(off[-1])
    graph = GraphBatch(R.batch_edges(off, eis).to(DEV), N, mode="sum")
    ref = R.batch_csr(off, eis)
    rp = graph.rowptr.clone()
    rp[3] = rp[4] + 2                                                     # graph 0: decreasing
    rp[int(off[3])] = int(graph.col.numel()) + 5                          # the end of graph 2 (and start of graph 3): beyond nnz
    rp[int(off[3]) + 4] = -1                                              # graph 3: negative
    broken = SimpleNamespace(rowptr=rp, col=graph.col)
    off_dev = torch.as_tensor(off, device=DEV)
    deg = torch.full((2, N), ISENT, device=DEV, dtype=torch.int32)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    _count(broken, off_dev, 4, 16, N, deg, bad)
    assert int(bad.item()) == 3
    g1 = np.arange(off[1], off[2])
    others = np.setdiff1d(np.arange(N), g1)
    for q in range(2):
        got = deg[q].cpu().numpy()
        assert np.array_equal(got[g1], ref[q]["deg"][g1]) and (got[others] == ISENT).all()
    rps = torch.as_tensor(np.stack([ref[0]["rowptr"], ref[1]["rowptr"]]), dtype=torch.int32).to(DEV)
    nnz = [int(ref[q]["rowptr"][-1]) for q in range(2)]
    outs = [(torch.full((z,), ISENT, device=DEV, dtype=torch.int32), torch.full((z,), SENTINEL, device=DEV),
             torch.full((z,), ISENT, device=DEV, dtype=torch.int32)) for z in nnz]
    bad.zero_()
    _write(broken, off_dev, 4, 16, N, rps, nnz, outs, bad)
    assert int(bad.item()) == 3
    for q in range(2):
        col, val, perm = (t.cpu().numpy() for t in outs[q])
        good = np.isin(np.repeat(np.arange(N), ref[q]["deg"]), g1)
        assert np.array_equal(col[good], ref[q]["col"][good]) and np.array_equal(perm[good], ref[q]["perm"][good])
        assert np.array_equal(val[good].view(np.int32), ref[q]["val"][good].view(np.int32))
        assert (col[~good] == ISENT).all() and (perm[~good] == ISENT).all() and (val[~good] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------- the propagation
def _padded(x, ld):
    buf = torch.full((x.shape[0], ld), SENTINEL, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf


def _launch(name, batch, x_buf, ldx, F, out_buf, ldo, max_nodes=256):
    from isic_hip.lib import call
    a1, a2 = batch.pair.a1, batch.pair.a2
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    call(name, a1.rowptr, a1.col, a1.val, int(a1.col.numel()), a2.rowptr, a2.col, a2.val, int(a2.col.numel()), batch.offs.device,
         len(batch.sizes), max_nodes, batch.N, x_buf, ldx, F, out_buf, ldo, bad)
    return int(bad.item())


@pytest.mark.parametrize("F", R.KERNEL_F)
def test_kernels_against_fp64_inside_the_dot_product_bound(batch, F):
    """Z and dH of the resident kernels, H / dH with row stride F + 3 and Z / dZ with 2 F + 5 (the padding keeps its sentinel):
    |Z^ - Z| <= c(m) |A^| |H| with c(m) = m u / (1 - m u), u = 2^-24 -- any summation order, any FMA contraction -- m = the
    operator's longest row + 2 forward and the longest rows of both operators + 3 backward.  A Z with ONE 2-hop entry left out
    exceeds the bound."""
    gen = torch.Generator().manual_seed(100 + F)
    h, dz = torch.randn(batch.N, F, generator=gen), torch.randn(batch.N, 2 * F, generator=gen)
    ldh, ldz = F + 3, 2 * F + 5
    z = torch.full((batch.N, ldz), SENTINEL, device=DEV)
    assert _launch("isic_h2_prop_f32", batch, _padded(h, ldh), ldh, F, z, ldz) == 0
    assert bool((z[:, 2 * F:] == SENTINEL).all())
    for q in range(2):
        ref, ab = batch.apply(q, h)
        bound = _c(batch.longest[q] + 2) * ab
        _inside(z[:, q * F:(q + 1) * F], ref, bound, f"Z, operator {q + 1}")
        if q == 1:                               # one entry of the 196-node graph's A2 left out
            g = batch.sizes.index(196)
            lo, hi = int(batch.offsets[g]), int(batch.offsets[g + 1])
            A = batch.dense[1][g].clone()
            i, j = (int(v[0]) for v in torch.nonzero(A, as_tuple=True))
            A[i, j] = 0.0
            wrong = (A @ h[lo:hi].double() - ref[lo:hi]).abs() / bound[lo:hi].clamp_min(1e-300)
            assert float(wrong.max()) > 100.0
    dh = torch.full((batch.N, ldh), SENTINEL, device=DEV)
    assert _launch("isic_h2_prop_bwd_f32", batch, _padded(dz, ldz), ldz, F, dh, ldh) == 0
    assert bool((dh[:, F:] == SENTINEL).all())
    (r1, b1), (r2, b2) = batch.apply(0, dz[:, :F]), batch.apply(1, dz[:, F:])
    _inside(dh[:, :F], r1 + r2, _c(batch.longest[0] + batch.longest[1] + 3) * (b1 + b2), "dH")


def test_resident_and_composed_agree_and_identical_calls_give_identical_bits(batch):
    from isic_hip import graph as G
    F = 33
    gen = torch.Generator().manual_seed(7)
    h, dz = torch.randn(batch.N, F, generator=gen), torch.randn(batch.N, 2 * F, generator=gen)
    res = {}
    for key, resident in (("resident", True), ("again", True), ("composed", False)):
        hd = h.to(DEV).requires_grad_(True)
        z = G.h2_prop(hd, batch.pair, batch.offs, resident=resident)
        assert G.h2_last_path() == ("resident" if resident else "composed")
        z.backward(dz.to(DEV))
        res[key] = (z.detach(), hd.grad)
    assert torch.equal(res["resident"][0], res["again"][0]) and torch.equal(res["resident"][1], res["again"][1])
    (r1, b1), (r2, b2) = batch.apply(0, h), batch.apply(1, h)
    zb = torch.cat([_c(batch.longest[0] + 2) * b1, _c(batch.longest[1] + 2) * b2], dim=1)
    (g1, c1), (g2, c2) = batch.apply(0, dz[:, :F]), batch.apply(1, dz[:, F:])
    hb = _c(batch.longest[0] + batch.longest[1] + 3) * (c1 + c2)
    _inside(res["composed"][0], torch.cat([r1, r2], dim=1), zb, "composed Z")
    _inside(res["composed"][1], g1 + g2, hb, "composed dH")
    _inside(res["resident"][0], res["composed"][0].cpu().double(), zb, "resident Z against composed Z")
    _inside(res["resident"][1], res["composed"][1].cpu().double(), hb, "resident dH against composed dH")


def test_max_nodes_257_takes_the_composed_path(batch):
    """offsets that join the 1-node and the 256-node graph into one of 257: the entry answers ISIC_ERR_UNSUPPORTED, h2_prop
    runs the composed path (which needs no offsets) and gives the same Z; without offsets likewise"""
    from isic_hip import graph as G
    from isic_hip.bags import BagOffsets
    from isic_hip.lib import IsicHipError
    sizes, offsets, eis = R.kernel_batch(graphs=((1, "none"), (256, "star"), (40, "knn")))
    gb = G.GraphBatch(R.batch_edges(offsets, eis).to(DEV), int(offsets[-1]), mode="sum")
    pair = G.two_hop(gb, BagOffsets(offsets, DEV))
    h = torch.randn(int(offsets[-1]), 9, generator=torch.Generator().manual_seed(1)).to(DEV)
    z = G.h2_prop(h, pair, BagOffsets(offsets, DEV), resident=True)
    assert G.h2_last_path() == "resident"
    joined = BagOffsets([0, 257, 297], DEV)
    z2 = G.h2_prop(h, pair, joined, resident=True)
    assert G.h2_last_path() == "composed"
    assert_close(z2, z, rtol=2e-6, atol=1e-7, what="composed Z")
    G.h2_prop(h, pair, None, resident=True)
    assert G.h2_last_path() == "composed"
    with pytest.raises(IsicHipError):
        G.two_hop(gb, joined)


def test_propagation_counts_a_graph_whose_operator_leaves_it(batch):
    """an operator entry pointing into another graph: the graph is counted, its rows of Z keep the sentinel, the others are
    written as before"""
    from isic_hip import graph as G
    from isic_hip.lib import call
    F = 5
    h = torch.randn(batch.N, F, generator=torch.Generator().manual_seed(2)).to(DEV)
    good = torch.full((batch.N, 2 * F), SENTINEL, device=DEV)
    assert _launch("isic_h2_prop_f32", batch, h, F, F, good, 2 * F) == 0
    a1, a2 = batch.pair.a1, batch.pair.a2
    g = batch.sizes.index(64)
    lo, hi = int(batch.offsets[g]), int(batch.offsets[g + 1])
    col2 = a2.col.clone()
    col2[int(a2.rowptr[lo + 3])] = hi + 1                        # a column id of the NEXT graph
    z = torch.full((batch.N, 2 * F), SENTINEL, device=DEV)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    call("isic_h2_prop_f32", a1.rowptr, a1.col, a1.val, int(a1.col.numel()), a2.rowptr, col2, a2.val, int(col2.numel()),
         batch.offs.device, len(batch.sizes), 256, batch.N, h, F, F, z, 2 * F, bad)
    assert int(bad.item()) == 1
    assert bool((z[lo:hi] == SENTINEL).all())
    assert torch.equal(z[:lo], good[:lo]) and torch.equal(z[hi:], good[hi:])
    bad_pair = G.TwoHopGraph(a1, G.GraphBatch.from_parts(batch.N, int(col2.numel()), "sym", {
        "rowptr": a2.rowptr, "col": col2, "val": a2.val, "rowptr_t": a2.rowptr, "col_t": col2, "val_t": a2.val, "perm_t": a2.perm_t}))
    with pytest.raises(ValueError, match="column id"):
        G.h2_prop(h, bad_pair, batch.offs, resident=True)


def test_propagation_counts_a_graph_whose_operator_row_pointers_are_wrong(batch):
    """the row-pointer checks of both entries: a row pointer of A1 above its successor in the 63-node graph, a row pointer of
    A2 beyond nnz2 in the first 64-node graph.  bad == 2, their rows of Z and dH keep the sentinel, the others are written as
    before"""
    from isic_hip.lib import call
    F = 5
    gen = torch.Generator().manual_seed(4)
    h, dz = torch.randn(batch.N, F, generator=gen).to(DEV), torch.randn(batch.N, 2 * F, generator=gen).to(DEV)
    good_z = torch.full((batch.N, 2 * F), SENTINEL, device=DEV)
    good_dh = torch.full((batch.N, F), SENTINEL, device=DEV)
    assert _launch("isic_h2_prop_f32", batch, h, F, F, good_z, 2 * F) == 0
    assert _launch("isic_h2_prop_bwd_f32", batch, dz, 2 * F, F, good_dh, F) == 0
    a1, a2 = batch.pair.a1, batch.pair.a2
    ga, gb = batch.sizes.index(63), batch.sizes.index(64)
    la, lb = int(batch.offsets[ga]), int(batch.offsets[gb])
    rp1, rp2 = a1.rowptr.clone(), a2.rowptr.clone()
    rp1[la + 2] = rp1[la + 3] + 1
    rp2[lb + 7] = int(a2.col.numel()) + 1000
    spans = [(la, int(batch.offsets[ga + 1])), (lb, int(batch.offsets[gb + 1]))]
    owned = torch.zeros(batch.N, dtype=torch.bool, device=DEV)
    for lo, hi in spans:
        owned[lo:hi] = True
    for name, x, ldx, out_w, ldo, good in (("isic_h2_prop_f32", h, F, 2 * F, 2 * F, good_z),
                                           ("isic_h2_prop_bwd_f32", dz, 2 * F, F, F, good_dh)):
        out = torch.full((batch.N, out_w), SENTINEL, device=DEV)
        bad = torch.zeros(1, device=DEV, dtype=torch.int32)
        call(name, rp1, a1.col, a1.val, int(a1.col.numel()), rp2, a2.col, a2.val, int(a2.col.numel()), batch.offs.device,
             len(batch.sizes), 256, batch.N, x, ldx, F, out, ldo, bad)
        assert int(bad.item()) == 2, name
        assert bool((out[owned] == SENTINEL).all()) and torch.equal(out[~owned], good[~owned]), name


# ---------------------------------------------------------------------------------------------- the whole model
FWD_TOL = dict(rtol=5e-5, atol=2e-6)        # tests/test_graph_gpu.py, whole-model forward
GRAD_TOL = dict(rtol=5e-4, atol=3e-6)       # ... gradients
CFG = dict(gnn_layers=2, att_heads=4, use_layer_norm=True, use_residual=True)


def _model(layers=2):
    from gnn_models import GraphMIL
    m = GraphMIL(32, "h2gcn", 64, layers, classifier_light=True)
    p = formula.formula_state_dict(formula.shapes_of(m))
    m.load_state_dict(p)
    return m.to(DEV).eval(), p


def _graphs(sizes, seed):
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    eis = [R.knn_like_edges(n, 8, rng) for n in sizes]
    return offsets, eis, [torch.randn(n, 32, generator=gen) for n in sizes]


@pytest.mark.parametrize("resident", (True, False))
@pytest.mark.parametrize("sizes", ([196], [196, 40, 1, 133, 77]))
def test_graphmil_against_the_restatement(sizes, resident):
    """probs, attention, loss and every parameter gradient of GraphMIL(32, 'h2gcn', 64, 2) in eval mode, one 196-node graph and
    a ragged batch of 5 graphs, against tests/h2gcn_ref.py in fp64, at the tolerances of the existing whole-model tests
    (tests/test_graph_gpu.py: rtol 5e-5 / atol 2e-6 forward, rtol 5e-4 / atol 3e-6 gradients, relative to the largest entry of
    each tensor)."""
    from isic_hip import graph as G
    from isic_hip import ops
    m, p = _model()
    m.h2_resident = resident
    offsets, eis, xs = _graphs(sizes, seed=11)
    ys = [(3 * g + 1) % 7 for g in range(len(sizes))]
    loss_o, probs_o, att_o, grads_o = R.graphmil_batch_loss_and_grads(p, CFG, xs, eis, ys)
    xd = torch.cat(xs).to(DEV).requires_grad_(True)
    ei = R.batch_edges(offsets, eis).to(DEV)
    if len(sizes) == 1:
        probs, att = m(xd, ei)
        probs = probs.unsqueeze(0)
    else:
        probs, att = m(xd, ei, offsets=offsets)
    assert G.h2_last_path() == ("resident" if resident else "composed")
    assert m.last_node_embeddings.shape == (sum(sizes), 7 * 64)
    assert_close(probs, probs_o, what="probs", **FWD_TOL)
    assert_close(att, att_o, what="att", **FWD_TOL)
    loss = ops.cross_entropy_from_probs(probs, torch.tensor(ys, device=DEV))
    assert_close(loss, loss_o, rtol=5e-5)
    loss.backward()
    for k, prm in m.named_parameters():
        if k.startswith("attention_layers") and k.endswith("2.bias"):
            continue                                             # analytically zero (softmax shift invariance)
        assert_close(prm.grad, grads_o[k], what=k, **GRAD_TOL)
    assert_close(xd.grad, torch.cat(grads_o["x"]), what="x", **GRAD_TOL)


def _records(count, lesion, n_side=6, D=32, seed=4):
    import build_graphs as bg
    rng = np.random.default_rng(seed)
    n = n_side * n_side
    ei = bg._grid_edge_index(True, side=n_side).numpy()
    r, c = np.divmod(np.arange(n), n_side)
    recs = []
    for i in range(count):
        cy, cx, ry, rx = rng.uniform(1.5, n_side - 2.5, 2).tolist() + rng.uniform(1.0, 2.6, 2).tolist()
        keep = ((r - cy) / ry) ** 2 + ((c - cx) / rx) ** 2 <= 1.0
        y = i % 3
        x = (rng.standard_normal((n, D)) + 0.8 * y * keep[:, None]).astype(np.float32)
        rec = {"x": x, "edge_index": ei.copy(), "y": y}
        if lesion:
            rec.update(keep=keep, graph_seed=100 + i)
        recs.append(rec)
    return recs


@pytest.mark.parametrize("kw", (dict(), dict(lesion_only=True), dict(lesion_only=True, lesion_knn=4),
                                dict(lesion_only=True, lesion_random=2)), ids=("full", "lesion", "lesion_knn", "lesion_random"))
def test_store_step_equals_the_same_graphs_built_directly(kw):
    """a step of GraphStore(mode='h2') -- two ragged assembly launches out of the pair built once over the record set --
    against ``two_hop`` on the step's concatenated edge lists: every array of both operators bit for bit, and so the
    probabilities"""
    from isic_hip import graph as G
    from isic_hip import train as T
    recs = _records(8, lesion=bool(kw))
    store = T.GraphStore(recs, torch.device(DEV), True, mode="h2", **kw)
    assert store._ragged is not None and store._stack is None
    idx = [5, 0, 3, 3, 7]
    x, offs, pair = store.batch(idx)
    if kw:
        assert len(set(np.diff(offs.host).tolist())) > 1         # graphs of unequal size
    ei = torch.cat([store.ei[i] + int(o) for i, o in zip(idx, offs.host[:-1])], dim=1)
    direct = G.two_hop(G.GraphBatch(ei, offs.total, mode="sum"), offs)
    assert pair.mode == "h2" and pair.n_nodes == offs.total
    for a, b in ((pair.a1, direct.a1), (pair.a2, direct.a2)):
        assert a.mode == "sym"
        for k in ("rowptr", "col", "perm_t", "rowptr_t", "col_t"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert torch.equal(a.val.view(torch.int32), b.val.view(torch.int32)) and torch.equal(a.val_t, b.val_t)
    assert torch.equal(x, torch.cat([store.x[i] for i in idx]))
    m, _ = _model()
    for resident in (True, False):
        m.h2_resident = resident
        assert torch.equal(m(x, offsets=offs, graph=pair)[0], m(x, offsets=offs, graph=direct)[0])
    # one record alone, and the index-only form of the train loop
    xi, oi, gi = store.batch([3])
    assert_close(m(xi, graph=gi)[0], m(x, offsets=offs, graph=pair)[0][2], what="record 3", **FWD_TOL)
    xs, rows, n_rows, offs2, pair2 = store.batch_rows(idx)
    assert n_rows == offs.total and torch.equal(xs[rows[:n_rows].long()], x) and torch.equal(pair2.a2.col, pair.a2.col)
    with pytest.raises(ValueError, match="h2"):
        m(x, offsets=offs, graph=G.GraphBatch(ei, offs.total, mode="gcn"))


def test_store_without_a_ragged_stack_builds_the_pair_from_the_concatenated_batch():
    """GraphStore(mode='h2', ragged_stack=False): no stack of either kind, so a step goes through ``_make_graph`` -- the pair
    of the step's concatenated edge lists -- and equals the step of a store that has the ragged stack, bit for bit"""
    from isic_hip import train as T
    recs = _records(8, lesion=True)
    slow = T.GraphStore(recs, torch.device(DEV), True, mode="h2", lesion_only=True, ragged_stack=False)
    fast = T.GraphStore(recs, torch.device(DEV), True, mode="h2", lesion_only=True)
    assert slow._ragged is None and slow._stack is None and fast._ragged is not None
    idx = [5, 0, 3, 3, 7]
    (x, offs, pair), (x2, offs2, pair2) = slow.batch(idx), fast.batch(idx)
    assert torch.equal(x, x2) and np.array_equal(offs.host, offs2.host) and pair.mode == "h2"
    for a, b in ((pair.a1, pair2.a1), (pair.a2, pair2.a2)):
        for k in ("rowptr", "col", "perm_t"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert torch.equal(a.val.view(torch.int32), b.val.view(torch.int32))
    assert slow.batch_rows(idx) is None                          # the index-only form needs a stack
    m, _ = _model()
    assert torch.equal(m(x, offsets=offs, graph=pair)[0], m(x2, offsets=offs2, graph=pair2)[0])


def test_a_short_train_gnn_fold_run_lowers_the_loss():
    from gnn_models import GraphMIL
    from isic_hip import train as T
    recs = _records(24, lesion=True)
    torch.manual_seed(3)
    model = GraphMIL(input_dim=32, gnn_type="h2gcn", gnn_hidden=32, gnn_layers=2, gnn_dropout=0.1, att_dim=16, att_heads=2,
                     classifier_dim=32, classifier_light=True, num_classes=3).to(DEV)
    model.set_dropout_state(3, 0)
    before = T.evaluate_gnn(model, T.GraphStore(recs[:16], torch.device(DEV), True, mode="h2", lesion_only=True), 3)["loss"]
    hist = []
    vm, tm, best = T.train_gnn_fold(model, recs[:16], recs[:16], recs[16:], lr=5e-3, epochs=4, graphs_per_step=4, num_classes=3,
                                    rng=np.random.RandomState(0), history=hist, lesion_only=True, patience=10)
    print("loss before", before, "history", hist)
    assert len(hist) == 4 and all(np.isfinite(h["val_loss"]) for h in hist) and np.isfinite(tm["loss"])
    assert hist[-1]["val_loss"] < before
