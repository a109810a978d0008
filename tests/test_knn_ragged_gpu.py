"""k-NN graphs among patch sets of unequal size on the MI355X (include/isic_hip_knn_ragged.h, csrc/knn_ragged.hip):
``isic_knn_graph_ragged`` bit-equal to ``isic_knn_graph`` (same MFMA order, norms from the Gram diagonal) and against the
oracle under the tie guard of tests/test_graph_gpu.py; the tie rule of all three k-NN kernels on exact integer inputs;
``isic_knn_edges_ragged`` exactly equal to the per-graph reference
loop (tests/knn_ragged_ref.py); the argument rules at the ABI; and the routes built on the two entries --
``build_graph_records(per_graph_k=True)``, ``GraphStore(lesion_only=True, lesion_knn=k)``, ``05_train_gnns.py --lesion-knn``,
``04_measure_heterophily.py --lesion-knn`` and the resident pipeline's ``keep`` / ``lesion_knn`` switches."""
import ctypes
import functools
import importlib.util
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import knn_ragged_ref as KR
from helpers import assert_close
from oracle import formula, graphs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimodal-isic_amd")

SMALL = (1, 2, 15, 16, 17, 33, 48, 64)                      # the 4-wave instantiation: max_nodes <= 64
MEDIUM = SMALL + (65, 100, 128)                             # 8 waves: <= 128
LARGE = MEDIUM + (129, 196, 208)                            # 13 waves: <= 208
SENTINEL = -7


def _offsets(sizes):
    from isic_hip.bags import BagOffsets
    return BagOffsets(np.concatenate([[0], np.cumsum(sizes)]), DEV)


def _ragged(x, offs, k, max_nodes=None, dev_offsets=None, total=None, fill=None):
    """The bare ``isic_knn_graph_ragged`` launch (``knn_indices_ragged`` may dispatch elsewhere)."""
    from isic_hip.lib import call
    T, D = x.shape
    idx = torch.full((T, k), SENTINEL if fill is None else fill, device=DEV, dtype=torch.int64)
    dist = torch.full((T, k), float(SENTINEL if fill is None else fill), device=DEV, dtype=torch.float32)
    o = offs.device if dev_offsets is None else dev_offsets
    call("isic_knn_graph_ragged", x, o, int(o.numel()) - 1, D, k, offs.max_bag if max_nodes is None else max_nodes,
         T if total is None else total, idx, dist)
    return idx, dist


def _assert_bit_equal(sizes, D, seed):
    from isic_hip.graph import knn_indices
    offs = _offsets(sizes)
    x = torch.randn(offs.total, D, generator=torch.Generator().manual_seed(seed)).to(DEV)
    top16 = None
    for k in (16, 1):
        want_i, want_d = knn_indices(x, offs, k, return_dist=True)
        top16 = want_i if top16 is None else top16
        got_i, got_d = _ragged(x, offs, k)
        assert torch.equal(got_i, want_i), (D, k, int((got_i != want_i).sum()))      # padding columns (-1 / +inf) included
        assert torch.equal(got_d, want_d), (D, k, int((got_d != want_d).sum()))
        from isic_hip.lib import call
        only_i = torch.full_like(got_i, SENTINEL)
        call("isic_knn_graph_ragged", x, offs.device, offs.num_bags, D, k, offs.max_bag, offs.total, only_i, None)
        assert torch.equal(only_i, want_i)                                           # nn_dist == NULL: the other instantiation
    return top16


# ------------------------------------------------------------------ bit-equality with isic_knn_graph
@pytest.mark.parametrize("D", [32, 96])                      # one K-chunk; three, so that the two-stage ring wraps
@pytest.mark.parametrize("sizes", [SMALL, MEDIUM, LARGE], ids=["4waves", "8waves", "13waves"])
def test_ragged_entry_equals_isic_knn_graph_bit_for_bit(sizes, D):
    nn = _assert_bit_equal(sizes, D, seed=11)
    assert (nn[:1] == -1).all() and (nn[1:3, 1:] == -1).all() and (nn[1:3, 0] >= 0).all()   # the 1-node and 2-node graphs


def test_many_small_graphs_and_an_empty_one_bit_for_bit():
    """600 graphs of 1 to 20 nodes with a 0-node graph in the middle, then 5000 of them with empty graphs at both ends and in
    the middle: many more workgroups than a launch holds at once (a workgroup takes ONE graph, the grid is G), so graphs
    start as others retire and the workgroups of empty graphs leave at once."""
    rng = np.random.RandomState(5)
    sizes = rng.randint(1, 21, 600)
    sizes[300] = 0
    _assert_bit_equal(sizes.tolist(), 64, seed=12)
    sizes = rng.randint(1, 21, 5000)
    sizes[[0, 2500, 4999]] = 0
    _assert_bit_equal(sizes.tolist(), 32, seed=13)


# ------------------------------------------------------------------ the tie rule: equal distances -> the lower index
TIE_SIZES = (1, 2, 3, 16, 17, 64, 65, 128, 129, 208)


@functools.lru_cache(maxsize=None)
def _tie_batch(sizes, D):
    """Integer coordinates out of {-2 .. 2} with n // 8 rows of every graph overwritten by copies of other rows: every product
    and every sum is an integer below 2^24, exact in fp32 in any summation order, so the device's distances ARE the int64
    ones and nearly every row has equal distances among its first k + 1 neighbours, a quarter of them a distance of 0 off
    the diagonal.  -> x float32, and per row the other nodes of its graph sorted by (distance, index): the first 16 of them
    (LOCAL ids, -1 past the n - 1 that exist), their distances (+inf there) and the share of rows of >= 17 nodes with a tie."""
    rng = np.random.RandomState(1000 * len(sizes) + D)
    xs, want_i, want_d, tied, rows = [], [], [], 0, 0
    for n in sizes:
        xg = rng.randint(-2, 3, (n, D))
        dup = rng.permutation(n)[:2 * (n // 8)]
        xg[dup[:n // 8]] = xg[dup[n // 8:]]
        xg = torch.from_numpy(xg).long()
        d = ((xg[:, None, :] - xg[None, :, :]) ** 2).sum(-1)                   # int64, exact
        d[torch.arange(n), torch.arange(n)] = 1 << 40                          # a node is not its own neighbour: sorts last
        dv, di = torch.sort(d, dim=1, stable=True)                             # stable: equal distances keep the index order
        kk = min(16, n - 1)
        wi, wd = torch.full((n, 16), -1, dtype=torch.int64), torch.full((n, 16), float("inf"))
        wi[:, :kk], wd[:, :kk] = di[:, :kk], dv[:, :kk].float()
        if n >= 17:
            tied += int((dv[:, 1:17] == dv[:, :16]).any(1).sum())
            rows += n
        xs.append(xg.float()), want_i.append(wi), want_d.append(wd)
    return torch.cat(xs), torch.cat(want_i), torch.cat(want_d), tied / max(rows, 1)


def _assert_tie_rule(sizes, D, run):
    x, want_i, want_d, tied = _tie_batch(tuple(sizes), D)
    assert tied >= 0.98, tied                                                  # the inputs do what they are made for
    offs = _offsets(sizes)
    for k in (16, 1):
        got_i, got_d = run(x.to(DEV), offs, k)
        assert torch.equal(got_i.cpu(), want_i[:, :k]), (D, k, int((got_i.cpu() != want_i[:, :k]).sum()))
        assert torch.equal(got_d.cpu(), want_d[:, :k]), (D, k, int((got_d.cpu() != want_d[:, :k]).sum()))


def _knn_indices_with_dist(x, offs, k):
    from isic_hip.graph import knn_indices
    return knn_indices(x, offs, k, return_dist=True)


@pytest.mark.parametrize("D", [32, 96])
def test_tie_rule_of_the_gram_kernel(D):
    """``topk(largest=False)`` on equal distances: the lower index comes first (03_build_graphs.py:50), which the selection
    of csrc/knn_tile.inc states as "strict < inside a lane, (value, index) across the lanes"."""
    _assert_tie_rule(TIE_SIZES, D, _knn_indices_with_dist)


@pytest.mark.parametrize("D", [32, 96])
@pytest.mark.parametrize("count", [6, 8, 10], ids=["4waves", "8waves", "13waves"])
def test_tie_rule_of_the_ragged_entry(count, D):
    _assert_tie_rule(TIE_SIZES[:count], D, _ragged)


@pytest.mark.parametrize("sizes,D", [((240, 30), 32), ((50, 196), 24)], ids=["above_208_nodes", "D_not_multiple_of_32"])
def test_tie_rule_of_the_row_tile_kernel(sizes, D):
    """knn_kernel of csrc/graph.hip (its norms come from a sum of their own: exact here like every other sum)."""
    _assert_tie_rule(sizes, D, _knn_indices_with_dist)


# ------------------------------------------------------------------ against the oracle, with the tie guard
@pytest.mark.parametrize("D", [32, 96])
def test_ragged_entry_against_the_oracle_with_gap_guard(D):
    """Neighbour j must equal the oracle's wherever the oracle's distances j - 1, j, j + 1 are more than 1e-3 apart (fp32
    summation noise, tests/test_graph_gpu.py::test_knn_random_batched_with_gap_guard), distances at rtol 1e-4 / atol 1e-3;
    the guard must leave at least 98 % of the positions checked (the oracle alone leaves 0.27 % / 0.15 % unguarded)."""
    sizes, k = (1, 2, 15, 16, 17, 33, 64, 65, 100, 128, 129, 196, 208, 3, 40, 25), 16
    offs = _offsets(sizes)
    x = torch.randn(offs.total, D, generator=torch.Generator().manual_seed(3))
    nn, dist = (t.cpu() for t in _ragged(x.to(DEV), offs, k))
    checked = total = 0
    for gi, n in enumerate(sizes):
        lo, hi = int(offs.host[gi]), int(offs.host[gi + 1])
        mine, md = nn[lo:hi], dist[lo:hi]
        if n == 1:
            assert (mine == -1).all() and torch.isinf(md).all()
            continue
        kk = min(k, n - 1)
        d = graphs.pairwise_sqdist(x[lo:hi])
        dv, di = torch.topk(d, kk + (1 if kk < n - 1 else 0), dim=1, largest=False)
        assert (mine[:, kk:] == -1).all() and torch.isinf(md[:, kk:]).all()
        gap = (dv[:, 1:] - dv[:, :-1]) > 1e-3                                  # gap[j]: between positions j and j + 1
        ok = torch.ones(n, kk, dtype=torch.bool)
        ok[:, 1:] &= gap[:, :kk - 1]
        ok[:, :gap.shape[1]] &= gap[:, :kk]
        assert torch.equal(mine[:, :kk][ok], di[:, :kk][ok]), gi
        checked += int(ok.sum())
        total += n * kk
        assert_close(md[:, :kk], dv[:, :kk], rtol=1e-4, atol=1e-3, what="knn distances")
    print(f"D={D}: {checked} of {total} positions checked ({100.0 * checked / total:.2f} %)")
    assert checked >= 0.98 * total, (checked, total)


# ------------------------------------------------------------------ edge lists
EDGE_SIZES = (0, 1, 2, 5, 17, 40, 196)
EDGE_KS = (1, 3, 8, 16)


@pytest.fixture(scope="module")
def gapped_batch():
    x = torch.cat([formula.gapped_points(n, 32, seed=n) for n in EDGE_SIZES if n])
    offs = _offsets(EDGE_SIZES)
    from isic_hip.graph import knn_indices_ragged
    nn = knn_indices_ragged(x.to(DEV), offs, 16)
    return x, offs, nn


@pytest.mark.parametrize("global_ids", [False, True])
def test_edge_lists_equal_the_per_graph_reference_loop(gapped_batch, global_ids):
    from isic_hip.graph import knn_edge_offsets, knn_edges_ragged
    x, offs, nn = gapped_batch
    out = knn_edges_ragged(nn, offs, EDGE_KS, global_ids=global_ids)
    want_off = knn_edge_offsets(EDGE_SIZES, EDGE_KS)
    assert list(out) == list(EDGE_KS)
    base = out[1][0].untyped_storage().data_ptr()
    for k in EDGE_KS:
        ei, eo = out[k]
        want, wo = KR.knn_edges_ragged(x, offs.host, k, global_ids=global_ids)
        assert eo.tolist() == wo.tolist() == want_off[k].tolist()
        assert ei.dtype == torch.int64 and torch.equal(ei.cpu(), want), k
        assert ei.untyped_storage().data_ptr() == base                           # views of ONE flat buffer


def test_corrupted_neighbour_id_is_stored_as_minus_one_and_raises(gapped_batch):
    from isic_hip.graph import knn_edge_offsets, knn_edges_ragged
    x, offs, nn = gapped_batch
    lo5 = int(offs.host[3])                                                      # the 5-node graph
    for value in (5, -2, 10 ** 12):                                              # n_g itself; negative; far outside every array
        bad = nn.clone()
        bad[lo5 + 2, 1] = value
        with pytest.raises(ValueError, match="outside their graph"):
            knn_edges_ragged(bad, offs, EDGE_KS)
        out = knn_edges_ragged(bad, offs, EDGE_KS, check=False)
        for k in EDGE_KS:
            ei, eo = out[k]
            want, _ = KR.knn_edges_ragged(x, offs.host, k)
            kk = min(k, 4)
            if kk > 1:
                want[1, int(eo[3]) + 2 * kk + 1] = -1
            assert torch.equal(ei.cpu(), want), (value, k)


def test_a_clamped_k_above_the_table_width_is_rejected(gapped_batch):
    from isic_hip.graph import knn_edges_ragged
    from isic_hip.lib import IsicHipError
    _, offs, nn = gapped_batch
    with pytest.raises(IsicHipError) as e:
        knn_edges_ragged(nn[:, :4].contiguous(), offs, (3, 8))
    assert e.value.code == -1
    assert 3 in knn_edges_ragged(nn[:, :4].contiguous(), offs, (3, 4))            # kk <= 4 everywhere: fine


def _edges_call(nn, offs_dev, G, total_nodes, ks, base, total_edges, src, dst, bad):
    from isic_hip.lib import call
    kv = (ctypes.c_int32 * len(ks))(*ks)
    call("isic_knn_edges_ragged", nn, int(nn.shape[1]), offs_dev, G, total_nodes, ctypes.addressof(kv), len(ks), base, total_edges,
         0, src, dst, bad)


def test_edges_kernel_refuses_offsets_and_segments_that_do_not_fit(gapped_batch):
    """A graph whose offsets leave [0, total_nodes] and a segment that is not n_g * kk long write nothing and are counted."""
    from isic_hip.graph import knn_edge_counts
    _, offs, nn = gapped_batch
    G, T = offs.num_bags, offs.total
    cnt = knn_edge_counts(np.diff(offs.host), (8,))
    base_h = np.concatenate([[0], np.cumsum(cnt[0])]).astype(np.int64)
    E = int(base_h[-1])

    def run(offs_h, base_hh):
        src = torch.full((E,), SENTINEL, device=DEV, dtype=torch.int64)
        dst = torch.full((E,), SENTINEL, device=DEV, dtype=torch.int64)
        bad = torch.zeros(1, device=DEV, dtype=torch.int32)
        _edges_call(nn, torch.from_numpy(offs_h).to(DEV), G, T, (8,), torch.from_numpy(base_hh.reshape(1, -1)).to(DEV), E, src, dst, bad)
        return src.cpu(), dst.cpu(), int(bad.item())

    good = run(offs.host, base_h)
    assert good[2] == 0 and (good[0] >= 0).all()
    past = offs.host.copy()
    past[-1] = T + 3                                                              # the last graph ends past total_nodes
    s, d, nbad = run(past, base_h)
    lo = int(base_h[G - 1])
    assert nbad == 1 and (s[lo:] == SENTINEL).all() and (d[lo:] == SENTINEL).all()
    assert torch.equal(s[:lo], good[0][:lo]) and torch.equal(d[:lo], good[1][:lo])
    short = base_h.copy()
    short[5:] -= 1                                                                # graph 4's segment is one edge short
    s, d, nbad = run(offs.host, short)
    a, b = int(base_h[4]), int(base_h[5])
    assert nbad == 1 and (s[a:b - 1] == SENTINEL).all()
    assert torch.equal(s[:a], good[0][:a]) and torch.equal(d[b - 1:E - 1], good[1][b:])
    far = base_h.copy()
    far[-1] = E + 8                                                               # the last segment leaves total_edges
    s, d, nbad = run(offs.host, far)
    assert nbad == 1 and (s[lo:] == SENTINEL).all() and torch.equal(s[:lo], good[0][:lo])


# ------------------------------------------------------------------ argument rules at the ABI
def test_unsupported_and_null_arguments_are_refused():
    from isic_hip.lib import IsicHipError, call
    offs = _offsets((5, 7))
    x = torch.randn(12, 64, device=DEV)
    idx = torch.empty((12, 4), device=DEV, dtype=torch.int64)
    for D, k, max_nodes in ((48, 4, 7), (16, 4, 7), (64, 17, 7), (64, 4, 209)):
        with pytest.raises(IsicHipError) as e:
            call("isic_knn_graph_ragged", x, offs.device, 2, D, k, max_nodes, 12, idx, None)
        assert e.value.code == -2, (D, k, max_nodes)
    for args in ((None, offs.device, idx), (x, None, idx), (x, offs.device, None)):
        with pytest.raises(IsicHipError) as e:
            call("isic_knn_graph_ragged", args[0], args[1], 2, 64, 4, 7, 12, args[2], None)
        assert e.value.code == -1
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    out = torch.empty(40, device=DEV, dtype=torch.int64)
    base = torch.zeros((1, 3), device=DEV, dtype=torch.int64)
    for nn_, offs_, base_, src_, dst_, bad_ in ((None, offs.device, base, out, out, bad), (idx, None, base, out, out, bad),
                                                (idx, offs.device, None, out, out, bad), (idx, offs.device, base, None, out, bad),
                                                (idx, offs.device, base, out, None, bad), (idx, offs.device, base, out, out, None)):
        with pytest.raises(IsicHipError) as e:
            kv = (ctypes.c_int32 * 1)(3)
            call("isic_knn_edges_ragged", nn_, 4, offs_, 2, 12, ctypes.addressof(kv), 1, base_, 40, 0, src_, dst_, bad_)
        assert e.value.code == -1


@pytest.mark.parametrize("case", ["decreasing", "past_total", "span_above_max_nodes_middle", "span_above_max_nodes_last"])
def test_a_graph_with_bad_offsets_writes_nothing_and_its_neighbours_are_intact(case):
    from isic_hip.graph import knn_indices
    sizes = {"span_above_max_nodes_middle": (5, 7, 4), "span_above_max_nodes_last": (5, 4, 7)}.get(case, (5, 7, 4))
    offs = _offsets(sizes)
    T = offs.total
    x = torch.randn(T, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    want_i, want_d = knn_indices(x, offs, 3, return_dist=True)
    o = offs.host.copy()
    max_nodes, refused = 7, 2
    if case == "decreasing":
        o[3] = o[2] - 3                                     # [0, 5, 12, 9]
    elif case == "past_total":
        o[3] = T + 24                                       # [0, 5, 12, 40]
    else:
        max_nodes, refused = 5, sizes.index(7)
    got_i, got_d = _ragged(x, offs, 3, max_nodes=max_nodes, dev_offsets=torch.from_numpy(o).to(DEV), total=T)
    lo, hi = int(offs.host[refused]), int(offs.host[refused + 1])
    assert (got_i[lo:hi] == SENTINEL).all() and (got_d[lo:hi] == float(SENTINEL)).all()
    keep = torch.ones(T, dtype=torch.bool, device=DEV)
    keep[lo:hi] = False
    assert torch.equal(got_i[keep], want_i[keep]) and torch.equal(got_d[keep], want_d[keep])


# ------------------------------------------------------------------ build_graph_records(per_graph_k=True)
def test_build_graph_records_with_the_clamp_of_every_image():
    import pandas as pd
    import build_graphs as bg
    ns = (1, 2, 9, 196)
    xs = [formula.gapped_points(n, 32, seed=20 + n).numpy() for n in ns]
    frame = pd.DataFrame({"image_id": [f"img{i}" for i in range(len(ns))], "patch_embeddings": xs})
    recs = bg.build_graph_records(frame, "m", 0, "train", list(EDGE_KS), [1], 42, per_graph_k=True)
    assert [r["image_id"] for r in recs] == list(frame["image_id"])
    for r, xg in zip(recs, xs):
        for k in EDGE_KS:
            want = graphs.knn_edge_index(torch.from_numpy(xg), k).numpy()       # the per-image loop of 03_build_graphs.py:104-105
            got = r["knn_edge_indices"][k]
            assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), (xg.shape[0], k)
    assert recs[0]["knn_edge_indices"][8].shape == (2, 0) and recs[1]["knn_edge_indices"][8].shape == (2, 2)
    with pytest.raises(ValueError, match="at least 2 nodes"):
        bg.build_graph_records(frame, "m", 0, "train", list(EDGE_KS), [1], 42)
    rag = bg.knn_edge_index_ragged(torch.from_numpy(np.concatenate(xs)), np.concatenate([[0], np.cumsum(ns)]), EDGE_KS)
    for k in EDGE_KS:
        want, wo = KR.knn_edges_ragged(torch.from_numpy(np.concatenate(xs)), np.concatenate([[0], np.cumsum(ns)]), k)
        assert torch.equal(rag[k][0].cpu(), want) and rag[k][1].tolist() == wo.tolist()


# ------------------------------------------------------------------ GraphStore(lesion_only=True, lesion_knn=8)
def _lesion_knn_records(count, n=40, D=32, seed=6):
    """Gapped features; keep patterns: all, none (keeps all), one node, then random."""
    rng = np.random.RandomState(seed)
    recs = []
    for i in range(count):
        keep = [np.ones(n, bool), np.zeros(n, bool), np.arange(n) == 17][i] if i < 3 else rng.rand(n) < rng.uniform(0.15, 0.8)
        x = formula.gapped_points(n, D, seed=100 + i).numpy()
        full = graphs.knn_edge_index(torch.from_numpy(x), 8).numpy()            # what a record of the full frame carries: ignored
        recs.append({"x": x, "edge_index": full, "y": i % 3, "keep": keep, "image_id": f"IMG_{i:04d}"})
    return recs


def test_lesion_knn_store_equals_the_reference_loop_among_the_kept_patches():
    from isic_hip import train as T
    recs = _lesion_knn_records(9)
    store = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True, lesion_knn=8)
    sizes = set()
    for i, r in enumerate(recs):
        xs, ei, rows = KR.lesion_knn_record(r["x"], r["keep"], 8)
        assert torch.equal(store.x[i].cpu(), xs) and torch.equal(store.ei[i].cpu(), ei), i
        assert store.rows[i].dtype == torch.int64 and np.array_equal(store.rows[i].cpu().numpy(), rows), i
        sizes.add(len(rows))
    assert store.x[1].shape[0] == 40 and store.x[2].shape[0] == 1 and store.ei[2].shape == (2, 0) and len(sizes) > 3
    induced = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True)
    assert any(a.shape != b.shape for a, b in zip(induced.ei, store.ei))          # the induced subgraph is another graph
    with pytest.raises(ValueError, match="lesion_only"):
        T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_knn=8)


def test_graphmil_step_on_the_lesion_knn_store_ragged_stack_equals_the_slow_path():
    """One GraphMIL[gcn] train step, as tests/test_ragged_graph_gpu.py checks it for induced graphs: the same kernels on
    identical operands, so probabilities, attention, loss and every gradient are equal exactly."""
    from gnn_models import GraphMIL
    from isic_hip import train as T
    recs = _lesion_knn_records(9)
    torch.manual_seed(5)
    model = GraphMIL(input_dim=32, gnn_type="gcn", gnn_hidden=64, gnn_layers=2, gnn_dropout=0.3, att_dim=32, att_heads=2,
                     pool_dropout=0.2, classifier_dim=64, classifier_light=True, num_classes=3).to(DEV)
    model.train()
    slow = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True, lesion_knn=8, ragged_stack=False)
    fast = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True, lesion_knn=8, ragged_stack=True)
    assert slow._ragged is None and fast._ragged is not None
    idx = [4, 2, 7, 0, 4, 1]
    y = slow.y_dev[torch.tensor(idx, device=DEV)]
    params = list(model.parameters())

    def run(store):
        model.set_dropout_state(seed=9, step=0)
        x, offs, g = store.batch(idx)
        probs, att, loss = model(x, offsets=offs, graph=g, labels=y)
        return probs.detach().clone(), att.detach().clone(), loss.detach().clone(), torch.autograd.grad(loss, params)

    ref, got = run(slow), run(fast)
    assert bool(torch.isfinite(ref[2])) and ref[1].shape[0] == sum(int(slow.x[i].shape[0]) for i in idx)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
    for (name, _), u, v in zip(model.named_parameters(), ref[3], got[3]):
        assert torch.equal(u, v), (name, (u - v).abs().max().item())


# ------------------------------------------------------------------ the two scripts
def _load_script(name, alias):
    spec = importlib.util.spec_from_file_location(alias, os.path.join(PKG, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_05_train_gnns_lesion_knn_runs_one_epoch_and_writes_its_csv(tmp_path):
    import pandas as pd
    m05 = _load_script("05_train_gnns.py", "train_gnns_05_knn")
    recs = _lesion_knn_records(24, n=36)
    splits = ["train"] * 12 + ["val"] * 6 + ["test"] * 6
    gdir, sdir = tmp_path / "graph_outputs" / "synth", tmp_path / "patch_stats" / "synth"
    gdir.mkdir(parents=True), sdir.mkdir(parents=True)
    rows = [{"model_name": "synth", "fold": 0, "split": s, "image_id": r["image_id"], "grid4_edge_index": r["edge_index"],
             "grid8_edge_index": r["edge_index"], "knn_edge_indices": {8: r["edge_index"]}, "random_edge_indices": {}}
            for r, s in zip(recs, splits)]
    pickle.dump(pd.DataFrame(rows), open(gdir / "graph_dataset.pkl", "wb"))
    for split in ("train", "val", "test"):
        part = [{"image_id": r["image_id"], "label": r["y"], "patch_embeddings": r["x"]} for r, s in zip(recs, splits) if s == split]
        pickle.dump(pd.DataFrame(part), open(sdir / f"patch_stats_fold_0_{split}.pkl", "wb"))
    patch = [{"image_path": f"/data/{r['image_id']}.jpg", "segmentation_path": "", "target": r["y"], "patch_id": p,
              "patch_latent": r["x"][p], "patch_in_mask": int(r["keep"][p])} for r in recs for p in range(36)]
    pickle.dump(pd.DataFrame(patch), open(tmp_path / "patch_flags.pkl", "wb"))
    common = ["--root", str(tmp_path), "--gnn", "gcn", "--variants", "knn8", "--folds", "0", "--epochs", "1", "--hidden-dim", "32",
              "--graphs-per-step", "4", "--results-csv", "knn/common_results.csv"]
    with pytest.raises(SystemExit):
        m05.parse_args(common + ["--lesion-knn"])                               # needs --lesion-flags
    args = m05.parse_args(common + ["--lesion-flags", str(tmp_path / "patch_flags.pkl"), "--lesion-knn"])
    assert m05.lesion_knn_k(args, "knn8") == 8 and m05.lesion_knn_k(args, "grid8") is None
    assert m05.lesion_knn_k(m05.parse_args(common + ["--lesion-flags", str(tmp_path / "patch_flags.pkl")]), "knn8") is None
    m05.main(common + ["--lesion-flags", str(tmp_path / "patch_flags.pkl"), "--lesion-knn"])
    out = pd.read_csv(tmp_path / "knn" / "results_job_0.csv")
    assert len(out) == 1 and out["graph_variant"].iloc[0] == "knn8"
    assert np.isfinite(out[["val_accuracy_mean", "test_bacc_mean"]].values).all()


def test_04_measure_heterophily_lesion_knn_counts_nodes_and_edges(tmp_path, monkeypatch):
    import pandas as pd
    import build_graphs as bg
    h04 = _load_script("04_measure_heterophily.py", "h04_knn")
    rs = np.random.RandomState(8)
    N, C = 196, 5
    r, c = np.divmod(np.arange(N), 14)
    ellipse = lambda cy, cx, ry, rx: ((r - cy) / ry) ** 2 + ((c - cx) / rx) ** 2 <= 1.0      # noqa: E731
    keep = [ellipse(6.5, 6.5, 4.2, 3.1), np.zeros(N, bool), np.arange(N) == 77, ellipse(3.0, 9.0, 1.2, 1.6)]
    grows, prows, frows = [], [], []
    for i, kp in enumerate(keep):
        emb = rs.randn(N, 32).astype(np.float32)
        pp = torch.softmax(torch.from_numpy(rs.randn(N, C).astype(np.float32)) * 2, dim=1).numpy()
        grows.append({"model_name": "m", "fold": 0, "split": "train", "image_id": f"img{i}",
                      "grid4_edge_index": bg._grid_edge_index(False).numpy(), "grid8_edge_index": bg._grid_edge_index(True).numpy(),
                      "knn_edge_indices": {8: graphs.knn_edge_index(torch.from_numpy(emb), 8).numpy()}, "random_edge_indices": {}})
        prows.append({"image_id": f"img{i}", "label": i % 2, "patch_embeddings": emb, "patch_probs": pp,
                      "dominant_class": pp.argmax(axis=1).astype(np.int64)})
        frows += [{"image_path": f"/data/img{i}.jpg", "patch_id": p, "patch_in_mask": int(kp[p])} for p in range(N)]
    os.makedirs(tmp_path / "g" / "m")
    os.makedirs(tmp_path / "p" / "m")
    pickle.dump(grows, open(tmp_path / "g" / "m" / "graph_dataset.pkl", "wb"))
    pickle.dump(prows, open(tmp_path / "p" / "m" / "patch_stats_fold_0_train.pkl", "wb"))
    pickle.dump(pd.DataFrame(frows), open(tmp_path / "flags.pkl", "wb"))
    base = ["04", "--graph-outputs-root", str(tmp_path / "g"), "--patch-stats-root", str(tmp_path / "p"), "--images-per-launch", "3",
            "--lesion-flags", str(tmp_path / "flags.pkl")]
    monkeypatch.setattr(sys, "argv", base + ["--out-csv", str(tmp_path / "knn.csv"), "--lesion-knn"])
    h04.main()
    monkeypatch.setattr(sys, "argv", base + ["--out-csv", str(tmp_path / "induced.csv")])
    h04.main()
    knn, induced = pd.read_csv(tmp_path / "knn.csv"), pd.read_csv(tmp_path / "induced.csv")
    assert list(knn.columns) == list(induced.columns) and list(knn["graph_variant"]) == list(induced["graph_variant"])
    other = knn["graph_variant"] != "knn8"
    pd.testing.assert_frame_equal(knn[other], induced[other])                     # other variants keep the induced subgraph
    rows = knn[knn["graph_variant"] == "knn8"].reset_index(drop=True)
    assert len(rows) == len(keep)
    for i, kp in enumerate(keep):
        n = int(kp.sum()) or N
        kk = 0 if n < 2 else max(1, min(8, n - 1))
        assert int(rows["num_nodes"][i]) == n and int(rows["num_edges"][i]) == n * kk, i
    assert int(rows["num_edges"].sum()) == sum((int(k.sum()) or N) * (0 if (int(k.sum()) or N) < 2 else min(8, (int(k.sum()) or N) - 1))
                                               for k in keep)
    assert int(rows["num_edges"][0]) > int(induced[induced["graph_variant"] == "knn8"]["num_edges"].iloc[0])
    monkeypatch.setattr(sys, "argv", ["04", "--lesion-knn"])
    with pytest.raises(SystemExit):
        h04.main()


# ------------------------------------------------------------------ the resident pipeline (pipeline.py)
def _teacher_outputs(G, N, D, C, seed):
    from pipeline import DeviceTeacherOutputs
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(G, N, D, generator=gen).to(DEV)
    pp = torch.softmax(torch.randn(G, N, C, generator=gen) * 2, dim=2).to(DEV)
    return DeviceTeacherOutputs(x, pp, torch.rand(G, N, generator=gen).to(DEV), (torch.arange(G) % C).to(DEV),
                                [f"i{seed}_{i}" for i in range(G)], kmax=16)


def _keep_rows(G, N, seed):
    rng = np.random.RandomState(seed)
    keep = rng.rand(G, N) < rng.uniform(0.15, 0.7, (G, 1))
    keep[0], keep[1] = False, np.arange(N) == 5                               # no flag (keeps all); one patch
    return keep


def test_resident_heterophily_summary_with_lesion_knn():
    import measure_heterophily as mh
    G, N = 5, 196
    outs = _teacher_outputs(G, N, 32, 4, seed=21)
    keep = torch.from_numpy(_keep_rows(G, N, 3)).to(DEV)
    got = outs.heterophily_summary("knn8", keep=keep, lesion_knn=True)
    want = mh.heterophily_summary_lesion_knn(outs.x, outs.patch_probs, outs.dominant_class, keep, 8)
    n = np.where(keep.cpu().numpy().any(1), keep.cpu().numpy().sum(1), N)
    kk = np.where(n < 2, 0, np.minimum(8, n - 1))
    assert got["num_nodes"].cpu().tolist() == n.tolist() and got["num_edges"].cpu().tolist() == (n * kk).tolist()
    for key in want:                                                            # the same launches on the same operands (NaN: no edge)
        assert torch.equal(torch.nan_to_num(got[key].double(), nan=-123.0), torch.nan_to_num(want[key].double(), nan=-123.0)), key
    # another variant keeps the induced subgraph; the switch needs keep
    a, b = outs.heterophily_summary("grid4", keep=keep, lesion_knn=True), outs.heterophily_summary("grid4", keep=keep)
    assert a["num_edges"].cpu().tolist() == b["num_edges"].cpu().tolist()
    induced = outs.heterophily_summary("knn8", keep=keep)
    assert int(induced["num_edges"][2]) < int(got["num_edges"][2])
    with pytest.raises(ValueError, match="keep"):
        outs.heterophily_summary("knn8", lesion_knn=True)


def test_train_gnn_from_teacher_with_keep_and_lesion_knn():
    """The fold fed from resident outputs with ``keep`` / ``lesion_knn`` is the fold ``train_gnn_fold`` runs on the same records
    with ``lesion_only=True, lesion_knn=8``: the same model, order and kernels, so the metrics are equal exactly."""
    import pipeline
    from gnn_models import GraphMIL
    from isic_hip import train as T
    N = 36
    outs = [_teacher_outputs(g, N, 32, 3, seed=30 + i) for i, g in enumerate((12, 6, 6))]
    keeps = [_keep_rows(o.x.shape[0], N, 40 + i) for i, o in enumerate(outs)]

    def model():
        torch.manual_seed(3)
        m = GraphMIL(input_dim=32, gnn_type="gcn", gnn_hidden=32, gnn_layers=2, gnn_dropout=0.1, att_dim=16, att_heads=2,
                     classifier_dim=32, classifier_light=True, num_classes=3).to(DEV)
        m.set_dropout_state(3, 0)
        return m

    fit = dict(epochs=1, graphs_per_step=4, num_classes=3)
    got = pipeline.train_gnn_from_teacher(model(), *outs, "knn8", keep=keeps, lesion_knn=True, rng=np.random.RandomState(0), **fit)
    recs = [o.graph_records("knn8") for o in outs]
    for rs, kp in zip(recs, keeps):
        for r, k in zip(rs, kp):
            r["keep"] = k
    want = T.train_gnn_fold(model(), *recs, lesion_only=True, lesion_knn=8, rng=np.random.RandomState(0), **fit)
    assert np.isfinite(got[0]["loss"]) and np.isfinite(got[1]["loss"]) and got[2] == want[2]
    for a, b in zip(got[:2], want[:2]):
        assert set(a) == set(b) and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)
    # keep alone: the induced subgraphs (another graph, so in general other numbers); lesion_knn needs keep
    ind = pipeline.train_gnn_from_teacher(model(), *outs, "knn8", keep=keeps, rng=np.random.RandomState(0), **fit)
    ref = T.train_gnn_fold(model(), *recs, lesion_only=True, rng=np.random.RandomState(0), **fit)
    assert ind[0]["loss"] == ref[0]["loss"] and ind[1]["loss"] == ref[1]["loss"]
    with pytest.raises(ValueError, match="keep"):
        pipeline.train_gnn_from_teacher(model(), *outs, "knn8", lesion_knn=True, **fit)
    with pytest.raises(ValueError, match="train, val, test"):
        pipeline.train_gnn_from_teacher(model(), *outs, "knn8", keep=keeps[:2], **fit)
