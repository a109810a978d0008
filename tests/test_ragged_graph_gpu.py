"""The ragged patch graphs on the MI355X (include/isic_hip_ragged.h, csrc/ragged_graph.hip): induced subgraphs bit-equal to
tests/ragged_graph_ref.py, the ragged batch assembly element for element against the CSR built from the batch's concatenated
edge lists and against the equal-size assembly, GraphMIL over the ragged stack against the slow path, and the lesion-only
route end to end (GraphStore, train_gnn_fold, 05_train_gnns.py --lesion-flags).  Everything compared is an integer or a copied
float, or the output of the same kernels on identical operands: every comparison is exact."""
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

import ragged_graph_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimodal-isic_amd")

SIZES = (1, 2, 37, 196, 257)                  # nodes per graph
EDGES = (0, 255, 256, 257, 1025)              # edges per graph: around one and several 256-edge scan chunks
PATTERNS = ("all", "none", "one", "cut")      # every flag; no flag (keeps all); one node; a pattern that removes every edge


def _graph(n, E, pattern, rng):
    """(src, dst, keep, weight) of one graph.  'cut': every edge joins an even and an odd node and only the even ones are
    kept.  The others get a duplicated edge and a self loop."""
    if pattern == "cut" and n >= 2:
        ev, od = np.arange(0, n, 2), np.arange(1, n, 2)
        a, b = rng.choice(ev, E), rng.choice(od, E)
        flip = rng.random(E) < 0.5
        src, dst = np.where(flip, a, b), np.where(flip, b, a)
        keep = np.arange(n) % 2 == 0
    else:
        src, dst = rng.integers(0, n, E), rng.integers(0, n, E)
        if E > 4:
            src[E // 2], dst[E // 2] = src[0], dst[0]                      # a duplicated edge
            dst[E - 1] = src[E - 1]                                        # a self loop
        keep = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "one": np.arange(n) == n // 2,
                "cut": np.ones(n, bool), "random": rng.random(n) < 0.5}[pattern]
    return src.astype(np.int64), dst.astype(np.int64), keep, rng.random(E).astype(np.float32)


def _graph_set():
    rng = np.random.default_rng(20)
    graphs = [_graph(n, E, PATTERNS[(i + j) % 4], rng) for i, n in enumerate(SIZES) for j, E in enumerate(EDGES)]
    graphs += [_graph(n, E, p, rng) for n, E in ((37, 257), (257, 1025)) for p in PATTERNS + ("random",)]
    return graphs


def _flat(graphs):
    noff = np.concatenate([[0], np.cumsum([len(g[2]) for g in graphs])]).astype(np.int64)
    eoff = np.concatenate([[0], np.cumsum([len(g[0]) for g in graphs])]).astype(np.int64)
    cat = lambda j: np.concatenate([g[j] for g in graphs])               # noqa: E731
    return cat(0), cat(1), eoff, noff, cat(2), cat(3)


def _induced_on_device(src, dst, eoff, noff, keep, weight=None):
    from isic_hip.graph import induced_subgraphs
    ei = torch.from_numpy(np.stack([src, dst])).to(DEV)
    out = induced_subgraphs(ei, eoff, noff, torch.from_numpy(keep).to(DEV),
                            None if weight is None else torch.from_numpy(weight).to(DEV))
    return [t.cpu().numpy() for t in out]


# ------------------------------------------------------------------ induced subgraphs
def test_induced_subgraphs_equal_the_reference_bit_for_bit():
    graphs = _graph_set()
    assert {len(g[2]) for g in graphs} == set(SIZES) and {len(g[0]) for g in graphs} == set(EDGES)
    src, dst, eoff, noff, keep, w = _flat(graphs)
    want = R.induced_subgraphs(src, dst, eoff, noff, keep, w)
    got = _induced_on_device(src, dst, eoff, noff, keep, w)
    assert len(got) == 5
    for name, a, b in zip(("edge_index", "edge_offsets", "node_offsets", "rows", "edge_weight"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
    cut = [i for i, g in enumerate(graphs) if not g[2].all() and g[2].any() and len(g[0]) and np.diff(want[1])[i] == 0]
    assert len(cut) >= 4                                                 # the patterns that remove every edge did
    got4 = _induced_on_device(src, dst, eoff, noff, keep)                # without weights: the 4-tuple
    assert len(got4) == 4 and all(np.array_equal(a, b) for a, b in zip(got4, want[:4]))


def test_induced_subgraphs_of_the_builders_edge_lists():
    """grid4, grid8, knn8 and random8 edge lists of 196 nodes from the project's own builders, under an elliptic lesion
    mask, a random one and none at all."""
    import build_graphs as bg
    gen = torch.Generator().manual_seed(3)
    eis = [bg._grid_edge_index(False).numpy(), bg._grid_edge_index(True).numpy(),
           bg._knn_edge_index(torch.randn(196, 32, generator=gen).to(DEV), 8).cpu().numpy(),
           bg._random_edge_index(196, 8, seed=11).numpy()]
    r, c = np.divmod(np.arange(196), 14)
    rng = np.random.default_rng(5)
    masks = [((r - 6.5) / 4.0) ** 2 + ((c - 7.5) / 5.5) ** 2 <= 1.0, rng.random(196) < 0.4, np.zeros(196, bool)]
    graphs = [(e[0], e[1], m, None) for e in eis for m in masks]
    src, dst, eoff, noff, keep, _ = _flat([g[:3] + (np.zeros(0, np.float32),) for g in graphs])
    want = R.induced_subgraphs(src, dst, eoff, noff, keep)
    got = _induced_on_device(src, dst, eoff, noff, keep)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert 0 < np.diff(want[2])[0] < 196 and np.diff(want[2])[2] == 196


def test_out_of_range_endpoint_is_counted_never_used_and_raises():
    from isic_hip.graph import induced_subgraphs
    from isic_hip.lib import call
    graphs = _graph_set()[10:16]
    src, dst, eoff, noff, keep, _ = _flat(graphs)
    g_bad = 3
    n_bad = len(graphs[g_bad][2])
    src, dst = src.copy(), dst.copy()
    src[eoff[g_bad] + 1] = n_bad                                         # one past the graph's last node
    dst[eoff[g_bad] + 5] = -1
    dst[eoff[g_bad] + 9] = 2 ** 40
    ei = torch.from_numpy(np.stack([src, dst])).to(DEV)
    with pytest.raises(ValueError, match="endpoint"):
        induced_subgraphs(ei, eoff, noff, torch.from_numpy(keep).to(DEV))
    # the entries themselves: the three edges are counted in bad[g], kept nowhere, and no other graph's counts move
    G, T, E = len(graphs), int(noff[-1]), int(eoff[-1])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    new_id = torch.full((T,), -7, device=DEV, dtype=torch.int32)
    kn, ke = torch.zeros(G + 1, device=DEV, dtype=torch.int64), torch.zeros(G + 1, device=DEV, dtype=torch.int64)
    bad = torch.zeros(G, device=DEV, dtype=torch.int32)
    call("isic_induced_subgraph_count", d(noff), d(eoff), ei[0], ei[1], d(keep.astype(np.uint8)), G, T, E, new_id, kn, ke, bad)
    ok = np.ones(E, bool)
    ok[[eoff[g_bad] + 1, eoff[g_bad] + 5, eoff[g_bad] + 9]] = False
    s2, d2 = src.copy(), dst.copy()
    s2[~ok], d2[~ok] = 0, 0
    eoff2 = np.concatenate([[0], np.cumsum([ok[eoff[g]:eoff[g + 1]].sum() for g in range(G)])])
    want = R.induced_subgraphs(s2[ok], d2[ok], eoff2, noff, keep)        # the same record set without the three edges
    assert bad.cpu().tolist() == [3 if g == g_bad else 0 for g in range(G)]
    assert ke[:G].cpu().tolist() == np.diff(want[1]).tolist() and kn[:G].cpu().tolist() == np.diff(want[2]).tolist()
    # ... and a write over these counts stays inside its outputs: the guard elements after E' and T' keep their value
    noo, eoo = d(want[2]), d(want[1])
    t_out, e_out = int(want[2][-1]), int(want[1][-1])
    so = torch.full((e_out + 64,), -5, device=DEV, dtype=torch.int64)
    do = torch.full((e_out + 64,), -5, device=DEV, dtype=torch.int64)
    ro = torch.full((t_out + 64,), -5, device=DEV, dtype=torch.int64)
    call("isic_induced_subgraph_write", d(noff), d(eoff), ei[0], ei[1], None, new_id, G, T, E, noo, eoo, t_out, e_out, so, do,
         None, ro)
    assert np.array_equal(so[:e_out].cpu().numpy(), want[0][0]) and np.array_equal(do[:e_out].cpu().numpy(), want[0][1])
    assert np.array_equal(ro[:t_out].cpu().numpy(), want[3])
    assert bool((so[e_out:] == -5).all()) and bool((do[e_out:] == -5).all()) and bool((ro[t_out:] == -5).all())


# ------------------------------------------------------------------ ragged batch assembly
def _records(graphs, D=8, seed=1):
    gen = torch.Generator().manual_seed(seed)
    return [{"x": torch.randn(len(k), D, generator=gen), "edge_index": torch.from_numpy(np.stack([s, d_])), "y": i % 3}
            for i, (s, d_, k, _) in enumerate(graphs)]


def _assert_batch_equals_built(store, idx, g, rows, x=None):
    from isic_hip.graph import GraphBatch
    ns = [int(store.x[i].shape[0]) for i in idx]
    base = np.concatenate([[0], np.cumsum(ns)])
    ei = torch.cat([store.ei[i] + int(b) for i, b in zip(idx, base[:-1])], dim=1)
    ref = GraphBatch(ei, int(base[-1]), mode=store.mode)
    used = int(ref.rowptr[-1])
    assert g.n_nodes == int(base[-1]) and g.num_edges == ref.num_edges and g.mode == store.mode
    assert g.col.numel() == used                                          # the assembled arrays hold the stored entries only
    for k in ("rowptr", "rowptr_t"):
        assert torch.equal(getattr(g, k), getattr(ref, k)), k
    for k in ("col", "val", "col_t", "val_t", "perm_t"):
        assert torch.equal(getattr(g, k), getattr(ref, k)[:used]), k
    off = np.concatenate([[0], np.cumsum([int(t.shape[0]) for t in store.x])])
    want_rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx])
    assert rows.dtype == torch.int32 and np.array_equal(rows[:len(want_rows)].cpu().numpy(), want_rows)
    assert torch.equal(store._ragged["x"][rows[:len(want_rows)].long()], torch.cat([store.x[i] for i in idx]))
    if x is not None:
        assert torch.equal(x, torch.cat([store.x[i] for i in idx]))
    return used


@pytest.fixture(scope="module")
def graph_records():
    return _records(_graph_set())


@pytest.mark.parametrize("mode", ["gcn", "sum", "mean"])
def test_ragged_assembly_equals_the_csr_built_from_the_concatenated_edge_lists(graph_records, mode):
    from isic_hip import train as T
    store = T.GraphStore(graph_records, torch.device(DEV), True, mode=mode, ragged_stack=True)
    assert store._ragged is not None and store._stack is None
    empty = [i for i, r in enumerate(graph_records) if r["edge_index"].shape[1] == 0]
    assert len(empty) == len(SIZES)
    idx = [18, empty[3], 3, 18, 0, 34, empty[0], 24, 18, 7]              # a repeated index, graphs without an edge
    offs, g, rows = store._ragged_graph(idx, True)
    _assert_batch_equals_built(store, idx, g, rows)
    assert offs.host.tolist() == np.concatenate([[0], np.cumsum([int(store.x[i].shape[0]) for i in idx])]).tolist()
    assert torch.equal(offs.device.cpu(), torch.from_numpy(offs.host))
    x, offs2, g2 = store.batch(idx)                                       # the public route, host and device index
    _assert_batch_equals_built(store, idx, g2, rows, x)
    x3, _, g3 = store.batch(torch.tensor(idx, device=DEV))
    assert torch.equal(x3, x) and torch.equal(g3.col, g2.col) and torch.equal(g3.rowptr_t, g2.rowptr_t)
    xs, rows4, n_rows, offs4, g4 = store.batch_rows(idx)
    assert n_rows == offs.total and xs is store._ragged["x"] and torch.equal(rows4[:n_rows], rows[:n_rows])
    assert torch.equal(g4.perm_t, g2.perm_t) and rows4.numel() >= (n_rows + 7) // 8 * 8
    for one in (18, empty[4], 0):                                         # B = 1
        _, g1, rows1 = store._ragged_graph([one], True)
        used = _assert_batch_equals_built(store, [one], g1, rows1)
        assert mode == "gcn" or one != empty[4] or used == 0
    if mode == "sum":                                                     # a selection with a graph of zero stored entries,
        for sel in ([empty[2], 18, empty[1]], [empty[1], empty[2]]):      # and one with no stored entry at all
            _, gz, rz = store._ragged_graph(sel, True)
            _assert_batch_equals_built(store, sel, gz, rz)


def test_ragged_entry_equals_the_equal_size_entry_bit_for_bit():
    import build_graphs as bg
    from dataset import synthetic_latent_bags
    from isic_hip import train as T
    bags, labels = synthetic_latent_bags(12, 30, 8, classes=3, shift=0.5, seed=2)
    recs = [{"x": b, "edge_index": bg._knn_edge_index(torch.from_numpy(b), 5).numpy(), "y": int(y)} for b, y in zip(bags, labels)]
    for mode in ("gcn", "sum", "mean"):
        a = T.GraphStore(recs, torch.device(DEV), True, mode=mode)
        b = T.GraphStore(recs, torch.device(DEV), True, mode=mode, ragged_stack=True)
        assert a._stack is not None and a._ragged is None and b._ragged is not None
        idx = [7, 2, 11, 2, 0]
        rows_a = torch.zeros(5 * 30 + 16, device=DEV, dtype=torch.int32)
        ga = a._stacked_graph(torch.tensor(idx, device=DEV), rows_out=rows_a)
        _, gb, rows_b = b._ragged_graph(idx, True)
        for k in ("rowptr", "rowptr_t", "col", "val", "col_t", "val_t", "perm_t"):
            assert torch.equal(getattr(ga, k), getattr(gb, k)), (mode, k)
        assert torch.equal(rows_a[:150], rows_b[:150]) and ga.num_edges == gb.num_edges and ga.n_nodes == gb.n_nodes
        xa, _, _ = a.batch(idx)
        xb, _, _ = b.batch(idx)
        assert torch.equal(xa, xb)


# ------------------------------------------------------------------ GraphMIL over the ragged stack
@pytest.mark.parametrize("gnn_type", ["gcn", "gat"])
def test_graphmil_on_the_ragged_stack_equals_the_slow_path(graph_records, gnn_type):
    """Forward and backward of GraphMIL (width 64, two layers) on a ragged selection of five graphs: ``batch()`` out of the
    ragged stack against ``batch()`` on the slow path -- the same kernels on identical operands, so probabilities, attention
    and every parameter gradient are equal exactly -- and the ``batch_rows()`` route (the input projection reads the
    concatenated feature store through the row index), held to what tests/test_graph_gpu.py::
    test_batch_rows_path_equals_gathered_batch asks of the equal-size ``batch_rows`` path: ``torch.equal``."""
    from gnn_models import GraphMIL
    from isic_hip import train as T
    torch.manual_seed(5)
    model = GraphMIL(input_dim=8, gnn_type=gnn_type, gnn_hidden=64, gnn_layers=2, gnn_dropout=0.3, gnn_heads=2, att_dim=32,
                     att_heads=2, pool_dropout=0.2, classifier_dim=64, classifier_light=True, num_classes=3).to(DEV)
    model.train()
    mode = model.graph_mode or "gcn"
    slow = T.GraphStore(graph_records, torch.device(DEV), True, mode=mode)
    fast = T.GraphStore(graph_records, torch.device(DEV), True, mode=mode, ragged_stack=True)
    assert slow._ragged is None and slow._stack is None and fast._ragged is not None
    idx = [18, 7, 34, 18, 12]
    y = slow.y_dev[torch.tensor(idx, device=DEV)]
    params = list(model.parameters())

    def run(store, rows_path):
        model.set_dropout_state(seed=9, step=0)
        if rows_path:
            xs, rows, nr, offs, g = store.batch_rows(idx)
            probs, att, loss = model(xs, offsets=offs, graph=g, labels=y, x_rows=(rows, nr))
        else:
            x, offs, g = store.batch(idx)
            probs, att, loss = model(x, offsets=offs, graph=g, labels=y)
        return probs.detach().clone(), att.detach().clone(), loss.detach().clone(), torch.autograd.grad(loss, params)

    assert slow.batch_rows(idx) is None
    ref = run(slow, False)
    assert bool(torch.isfinite(ref[2])) and ref[1].shape[0] == sum(int(slow.x[i].shape[0]) for i in idx)
    for rows_path in (False, True):
        got = run(fast, rows_path)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]), rows_path
        for (name, _), u, v in zip(model.named_parameters(), ref[3], got[3]):
            assert torch.equal(u, v), (rows_path, name, (u - v).abs().max().item())


# ------------------------------------------------------------------ lesion-only, end to end
def _lesion_records(count, n_side=6, D=12, seed=4):
    """Small grid-graph records with an elliptic lesion flag per patch (one record without a lesion: it keeps every patch)."""
    import build_graphs as bg
    rng = np.random.default_rng(seed)
    n = n_side * n_side
    ei = bg._grid_edge_index(True, side=n_side).numpy()
    r, c = np.divmod(np.arange(n), n_side)
    recs = []
    for i in range(count):
        cy, cx, ry, rx = rng.uniform(1.5, n_side - 2.5, 2).tolist() + rng.uniform(1.0, 2.6, 2).tolist()
        keep = ((r - cy) / ry) ** 2 + ((c - cx) / rx) ** 2 <= 1.0
        if i == 2:
            keep = np.zeros(n, bool)
        y = i % 3
        x = (rng.standard_normal((n, D)) + 0.8 * y * keep[:, None]).astype(np.float32)
        recs.append({"x": x, "edge_index": ei.copy(), "y": y, "keep": keep, "image_id": f"IMG_{i:04d}"})
    return recs


def test_lesion_only_store_equals_a_store_of_host_induced_records():
    from isic_hip import train as T
    recs = _lesion_records(8)
    host = []
    for r in recs:
        s, d_, rows = R.induced_subgraph(r["edge_index"][0], r["edge_index"][1], r["keep"])
        host.append({"x": r["x"][rows], "edge_index": np.stack([s, d_]), "y": r["y"]})
    assert len({h["x"].shape[0] for h in host}) > 2 and host[2]["x"].shape[0] == 36
    a = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True)
    b = T.GraphStore(host, torch.device(DEV), True, mode="gcn")
    assert a._ragged is not None or not T.RAGGED_STACK_DEFAULT_LESION_ONLY
    assert b._ragged is None
    for i in range(8):
        assert torch.equal(a.x[i], b.x[i]) and torch.equal(a.ei[i], b.ei[i]), i
        assert np.array_equal(a.rows[i].cpu().numpy(), np.nonzero(recs[i]["keep"] if recs[i]["keep"].any() else np.ones(36))[0])
    idx = [5, 2, 5, 0]
    (xa, oa, ga), (xb, ob, gb) = a.batch(idx), b.batch(idx)
    assert torch.equal(xa, xb) and oa.host.tolist() == ob.host.tolist()
    used = int(gb.rowptr[-1])
    for k in ("rowptr", "rowptr_t"):
        assert torch.equal(getattr(ga, k), getattr(gb, k)), k
    for k in ("col", "val", "col_t", "val_t", "perm_t"):
        assert torch.equal(getattr(ga, k)[:used], getattr(gb, k)[:used]), k
    forced = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True, ragged_stack=True)
    assert forced._ragged is not None and torch.equal(forced.batch(idx)[0], xb)
    with pytest.raises(ValueError, match="keep"):
        T.GraphStore([{k: v for k, v in r.items() if k != "keep"} for r in recs], torch.device(DEV), True, lesion_only=True)


def test_train_gnn_fold_lesion_only_trains_one_epoch():
    from gnn_models import GraphMIL
    from isic_hip import train as T
    recs = _lesion_records(24)
    torch.manual_seed(3)
    model = GraphMIL(input_dim=12, gnn_type="gcn", gnn_hidden=32, gnn_layers=2, gnn_dropout=0.1, att_dim=16, att_heads=2,
                     classifier_dim=32, classifier_light=True, num_classes=3).to(DEV)
    model.set_dropout_state(3, 0)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    hist = []
    vm, tm, best = T.train_gnn_fold(model, recs[:12], recs[12:18], recs[18:], epochs=1, graphs_per_step=4, num_classes=3,
                                    rng=np.random.RandomState(0), history=hist, lesion_only=True, ragged_stack=True)
    assert np.isfinite(vm["loss"]) and np.isfinite(tm["loss"]) and len(hist) == 1 and np.isfinite(hist[0]["val_loss"])
    assert any(not torch.equal(v, before[k]) for k, v in model.state_dict().items())


def _write_tree(root, recs, model_name="synth"):
    import pandas as pd
    splits = ["train"] * 12 + ["val"] * 6 + ["test"] * 6
    gdir, sdir = root / "graph_outputs" / model_name, root / "patch_stats" / model_name
    gdir.mkdir(parents=True), sdir.mkdir(parents=True)
    rows = [{"model_name": model_name, "fold": 0, "split": s, "image_id": r["image_id"], "grid4_edge_index": r["edge_index"],
             "grid8_edge_index": r["edge_index"], "knn_edge_indices": {}, "random_edge_indices": {}} for r, s in zip(recs, splits)]
    with open(gdir / "graph_dataset.pkl", "wb") as f:
        pickle.dump(pd.DataFrame(rows), f)
    for split in ("train", "val", "test"):
        part = [{"image_id": r["image_id"], "label": r["y"], "patch_embeddings": r["x"]} for r, s in zip(recs, splits) if s == split]
        with open(sdir / f"patch_stats_fold_0_{split}.pkl", "wb") as f:
            pickle.dump(pd.DataFrame(part), f)
    # the patch-level frame of save_latent.extract_latents, rows shuffled: the loader orders them by patch_id
    n = recs[0]["x"].shape[0]
    patch = [{"image_path": f"/data/{r['image_id']}.jpg", "segmentation_path": "", "target": r["y"], "patch_id": p,
              "patch_latent": r["x"][p], "patch_in_mask": int(r["keep"][p])} for r in recs for p in range(n)]
    frame = pd.DataFrame(patch).sample(frac=1.0, random_state=0).reset_index(drop=True)
    with open(root / "patch_flags.pkl", "wb") as f:
        pickle.dump(frame, f)
    return root / "patch_flags.pkl"


def test_05_train_gnns_with_and_without_lesion_flags(tmp_path):
    import pandas as pd
    spec = importlib.util.spec_from_file_location("train_gnns_05", os.path.join(PKG, "05_train_gnns.py"))
    m05 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m05)
    recs = _lesion_records(24)
    flags = _write_tree(tmp_path, recs)
    common = ["--root", str(tmp_path), "--gnn", "gcn", "--variants", "grid8", "--folds", "0", "--epochs", "1", "--hidden-dim",
              "32", "--graphs-per-step", "4"]
    loaded = m05.load_fold_records(tmp_path, "synth", 0, "train", "grid8", m05.load_lesion_flags([flags]))
    assert [r["image_id"] for r in loaded] == [r["image_id"] for r in recs[:12]]
    for a, b in zip(loaded, recs[:12]):
        assert a["keep"].dtype == bool and np.array_equal(a["keep"], b["keep"])
    assert "keep" not in m05.load_fold_records(tmp_path, "synth", 0, "train", "grid8")[0]
    with pytest.raises(ValueError, match="IMG_0003"):
        m05.load_fold_records(tmp_path, "synth", 0, "train", "grid8",
                              {k: v for k, v in m05.load_lesion_flags([flags]).items() if k != "IMG_0003"})
    m05.main(common + ["--results-csv", "lesion/common_results.csv", "--lesion-flags", str(flags)])
    lesion = pd.read_csv(tmp_path / "lesion" / "results_job_0.csv")
    assert len(lesion) == 1 and np.isfinite(lesion[["val_accuracy_mean", "test_bacc_mean"]].values).all()
    # without the option: the run is the one the unchanged route gives -- records without flags, the fold trained by
    # train_one_fold with no lesion option at all -- number for number
    m05.main(common + ["--results-csv", "plain/common_results.csv"])
    plain = pd.read_csv(tmp_path / "plain" / "results_job_0.csv", float_precision="round_trip")   # (the default parser drops a digit)
    args = m05.parse_args(common)
    args.gnn = "gcn"
    assert args.lesion_flags is None
    del args.lesion_flags                                                # the namespace a caller of the old CLI holds
    tr, va, te = (m05.load_fold_records(tmp_path, "synth", 0, s, "grid8") for s in ("train", "val", "test"))
    vm, tm, be = m05.train_one_fold(tr, va, te, args, 0, 3, 12, torch.device(DEV))
    for k in m05.METRICS:
        for prefix, got in (("val", vm), ("test", tm)):
            a, b = float(plain[f"{prefix}_{k}_mean"].iloc[0]), float(got[k])
            assert a == b or (np.isnan(a) and np.isnan(b)), (prefix, k, a, b)
    assert float(plain["best_epoch_mean"].iloc[0]) == be
