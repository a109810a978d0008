"""The reference's random patch graphs over graphs of unequal size on the MI355X (include/isic_hip_randgraph_ragged.h,
csrc/rand_graph_ragged.hip): ``random_graphs_ragged`` equal, integer by integer, to the per-graph restatement
(tests/rand_graph_ragged_ref.py: own n, own clamp, own seed) and, at equal sizes, to ``random_graphs``; the behaviour on bad
offsets at the ABI; and the routes built on the two entries -- ``GraphStore(lesion_only=True, lesion_random=r)``,
``05_train_gnns.py --lesion-random``, ``04_measure_heterophily.py --lesion-random`` and the resident pipeline's switch."""
import ctypes
import importlib.util
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import rand_graph_ragged_ref as RGR
import rand_graph_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimodal-isic_amd")

# no word consumed (2), one word per node (3), the first state regeneration (27), two bitmap words (33), the wave boundary
# (64 / 65: the packed class and the workgroup class), the reference's 196, the maximum (256), and graphs without an edge
SIZES = [0, 1, 2, 3, 4, 5, 17, 26, 27, 33, 64, 65, 129, 196, 255, 256]
R_VALUES = (1, 2, 4, 8, 12, 16, 300)                   # the clamp makes 12, 16 and 300 coincide on small graphs
TEN_R = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16)               # 03_build_graphs.py's DEFAULT_R_VALUES
SENTINEL = -7


def _offsets(sizes):
    from isic_hip.bags import BagOffsets
    return BagOffsets.from_lengths(sizes, DEV)


def _seeds(count):
    return [RR.SEEDS[i % len(RR.SEEDS)] for i in range(count)]


def _assert_equals_restatement(got, seeds, sizes, r_values, global_ids=False):
    want = RGR.random_graphs_ragged(seeds, sizes, r_values, global_ids)
    assert list(got) == list(want)
    for r in want:
        ei, eo = got[r]
        assert ei.dtype == torch.int64 and isinstance(eo, np.ndarray) and eo.dtype == np.int64
        assert eo.tolist() == want[r][1].tolist(), r
        assert np.array_equal(ei.cpu().numpy(), want[r][0]), r


# ------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("global_ids", [False, True])
def test_one_batch_of_every_size_class_equals_the_restatement(global_ids):
    from isic_hip.graph import random_graphs_ragged
    seeds = _seeds(len(SIZES))
    got = random_graphs_ragged(seeds, _offsets(SIZES), R_VALUES, global_ids=global_ids)
    _assert_equals_restatement(got, seeds, SIZES, R_VALUES, global_ids)
    e12, e16, e300 = (got[r][0].cpu().numpy() for r in (12, 16, 300))
    o12, o16, o300 = (got[r][1] for r in (12, 16, 300))
    g5 = SIZES.index(5)                                  # r clamps to 4 for all three: the complete graph on 5 nodes
    assert o12[g5 + 1] - o12[g5] == o16[g5 + 1] - o16[g5] == o300[g5 + 1] - o300[g5] == 20
    g256 = SIZES.index(256)                              # r = 300 clamps to 255: complete
    assert o300[g256 + 1] - o300[g256] == 256 * 255 and o16[g256 + 1] - o16[g256] < 2 * 256 * 16 + 1
    assert e12.shape[1] < e16.shape[1] < e300.shape[1]
    # one flat buffer
    base = got[R_VALUES[0]][0].untyped_storage().data_ptr()
    assert all(got[r][0].untyped_storage().data_ptr() == base for r in R_VALUES)


def test_equal_sizes_equal_random_graphs_bit_for_bit():
    from isic_hip.graph import random_graphs, random_graphs_ragged
    G, n = 64, 196
    seeds = [42 + 10_000 * (i % 3) + i for i in range(G)]
    want = random_graphs(seeds, n, TEN_R, device=DEV)
    got = random_graphs_ragged(seeds, _offsets([n] * G), TEN_R)
    for r in TEN_R:
        ei, eo = got[r]
        per_graph = [want[r][g] for g in range(G)]
        assert eo.tolist() == np.concatenate([[0], np.cumsum([int(e.shape[1]) for e in per_graph])]).tolist(), r
        assert torch.equal(ei, torch.cat(list(per_graph), dim=1)), r
    # and the reference's own number for one of them
    assert np.array_equal(got[4][0][:, :int(got[4][1][1])].cpu().numpy(), RR.graph(196, 4, seeds[0]))


def test_packs_of_unequal_graphs_and_their_permutation():
    """About 300 graphs of 0..40 nodes in an order that puts unequal sizes and an empty graph into every pack of four; the
    same batch permuted gives the permuted result (a graph does not depend on its neighbours in the pack)."""
    from isic_hip.graph import random_graphs_ragged
    G = 300
    sizes = [0 if i % 4 == 2 else (i * 7) % 41 for i in range(G)]
    assert all(len(set(sizes[i:i + 4])) >= 3 and 0 in sizes[i:i + 4] for i in range(0, G, 4)) and max(sizes) == 40
    seeds = [1000 + 37 * i for i in range(G)]
    rs = (1, 4, 16)
    got = random_graphs_ragged(seeds, _offsets(sizes), rs)
    _assert_equals_restatement(got, seeds, sizes, rs)
    perm = np.random.RandomState(0).permutation(G)
    got_p = random_graphs_ragged([seeds[i] for i in perm], _offsets([sizes[i] for i in perm]), rs)
    for r in rs:
        (ei, eo), (ep, op) = got[r], got_p[r]
        ei, ep = ei.cpu().numpy(), ep.cpu().numpy()
        for at, g in enumerate(perm):
            assert np.array_equal(ep[:, op[at]:op[at + 1]], ei[:, eo[g]:eo[g + 1]]), (r, at, g)


def test_two_calls_give_identical_buffers():
    from isic_hip.graph import random_graphs_ragged
    sizes = [(i * 11) % 70 for i in range(97)]
    seeds = [7 * i for i in range(97)]
    a = random_graphs_ragged(seeds, _offsets(sizes), TEN_R, global_ids=True)
    b = random_graphs_ragged(seeds, _offsets(sizes), TEN_R, global_ids=True)
    for r in TEN_R:
        assert torch.equal(a[r][0], b[r][0]) and a[r][1].tolist() == b[r][1].tolist()


# ------------------------------------------------------------------ bad offsets at the ABI
def _count_write(seeds, dev_off, max_nodes, rs, edge_off=None, fill=SENTINEL):
    """The two bare launches over sentinel-filled buffers -> (counts [n_r, G], bad after count, src, dst, bad after write,
    edge_off [n_r, G+1]); ``edge_off``: a callable that alters the prefix sums before the write."""
    from isic_hip.lib import call
    G = int(dev_off.numel()) - 1
    rv = (ctypes.c_int * len(rs))(*rs)
    sd = torch.tensor(seeds, dtype=torch.int64).to(DEV)
    counts = torch.full((len(rs), G), fill, device=DEV, dtype=torch.int64)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    call("isic_random_graph_ragged_count", sd, dev_off, G, max_nodes, ctypes.addressof(rv), len(rs), counts, bad)
    cnt, bad_count = counts.cpu().numpy(), int(bad.item())
    assert (cnt >= 0).all()
    eo = np.concatenate([[0], np.cumsum(cnt.reshape(-1))]).astype(np.int64)
    off = np.stack([eo[j * G:j * G + G + 1] for j in range(len(rs))])
    total = int(eo[-1])
    if edge_off is not None:
        off = edge_off(off)
    src = torch.full((total,), fill, device=DEV, dtype=torch.int64)
    dst = torch.full((total,), fill, device=DEV, dtype=torch.int64)
    bad.zero_()
    call("isic_random_graph_ragged_write", sd, dev_off, G, max_nodes, ctypes.addressof(rv), len(rs),
         torch.from_numpy(off).to(DEV), total, 0, src, dst, bad)
    return cnt, bad_count, src.cpu().numpy(), dst.cpu().numpy(), int(bad.item()), off


GOOD = [5, 30, 70, 12, 40]                                # the packed class and the workgroup class
GOOD_OFF = np.concatenate([[0], np.cumsum(GOOD)])         # [0, 5, 35, 105, 117, 157]


@pytest.mark.parametrize("offsets,max_nodes,bad_graphs,host_offsets", [
    ([0, 5, 35, 20, 117, 157], 100, (2,), GOOD_OFF),                          # decreasing; graph 3 = [20, 117) is legal again
    ([0, 5, 35, 300, 117, 157], 100, (2, 3), GOOD_OFF),                       # past the total; graph 3 then runs backwards
    ([0, 5, 35, 105, 117, 157], 64, (2,), [0, 5, 35, 99, 117, 157]),          # a span of 70 > max_nodes = 64 in the middle
    ([0, 5, 35, 52, 64, 157], 64, (4,), [0, 5, 35, 52, 64, 128]),             # a span of 93 > 64 at the end
], ids=["decreasing", "past_the_total", "span_in_the_middle", "span_at_the_end"])
def test_a_bad_graph_writes_nothing_and_leaves_its_neighbours_intact(offsets, max_nodes, bad_graphs, host_offsets):
    from isic_hip.bags import BagOffsets
    from isic_hip.graph import random_graphs_ragged
    rs = (2, 16)
    seeds = [42, 43, 44, 45, 46]
    dev_off = torch.tensor(offsets, dtype=torch.int64).to(DEV)
    cnt, bad_count, src, dst, bad_write, off = _count_write(seeds, dev_off, max_nodes, rs)
    assert bad_count == len(bad_graphs) and bad_write == len(bad_graphs)
    for j, r in enumerate(rs):
        for g in range(5):
            lo, hi = int(off[j][g]), int(off[j][g + 1])
            if g in bad_graphs:
                assert cnt[j][g] == 0 and lo == hi
                continue
            want = RR.graph(offsets[g + 1] - offsets[g], r, seeds[g])
            assert cnt[j][g] == want.shape[1] and np.array_equal(src[lo:hi], want[0]) and np.array_equal(dst[lo:hi], want[1]), (j, g)
    assert len(src) == int(cnt.sum()) and (src != SENTINEL).all() and (dst != SENTINEL).all()
    # the Python surface raises: offsets whose host copy looks fine and whose device copy is the bad one
    with pytest.raises(ValueError, match="graph"):
        random_graphs_ragged(seeds, BagOffsets.from_uploaded(np.asarray(host_offsets), dev_off), rs)


def test_a_segment_one_short_is_left_untouched_and_raised():
    rs = (2, 16)
    seeds = [42, 43, 44, 45, 46]
    dev_off = torch.from_numpy(GOOD_OFF).to(DEV)

    def shorten(off):                                     # graph 1 of r = 16 loses its last slot to graph 2 (then one too long)
        off = off.copy()
        off[1][2] -= 1
        return off

    cnt, bad_count, src, dst, bad_write, off = _count_write(seeds, dev_off, 100, rs, edge_off=shorten)
    assert bad_count == 0 and bad_write == 2               # the short segment and its neighbour that grew
    for j, r in enumerate(rs):
        for g in range(5):
            lo, hi = int(off[j][g]), int(off[j][g + 1])
            if j == 1 and g in (1, 2):
                assert (src[lo:hi] == SENTINEL).all() and (dst[lo:hi] == SENTINEL).all()
                continue
            want = RR.graph(GOOD[g], r, seeds[g])
            assert np.array_equal(src[lo:hi], want[0]) and np.array_equal(dst[lo:hi], want[1]), (j, g)


# ------------------------------------------------------------------ GraphStore(lesion_only=True, lesion_random=4)
def _lesion_random_records(count, n=40, D=32, seed=6):
    """Keep patterns: all, none (keeps all), one node, then random; every record with its own seed and an ``edge_index`` of
    the full frame that the store must ignore."""
    rng = np.random.RandomState(seed)
    recs = []
    for i in range(count):
        keep = [np.ones(n, bool), np.zeros(n, bool), np.arange(n) == 17][i] if i < 3 else rng.rand(n) < rng.uniform(0.15, 0.8)
        x = rng.randn(n, D).astype(np.float32)
        recs.append({"x": x, "edge_index": RR.graph(n, 4, 42 + i).copy(), "y": i % 3, "keep": keep, "image_id": f"IMG_{i:04d}",
                     "graph_seed": 42 + 10_000 + i})
    return recs


def test_lesion_random_store_equals_the_reference_loop_among_the_kept_patches():
    from isic_hip import train as T
    recs = _lesion_random_records(9)
    store = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True, lesion_random=4)
    sizes = set()
    for i, r in enumerate(recs):
        xs, rows, ei = RGR.lesion_random_record(r["x"], r["keep"], 4, r["graph_seed"])
        assert np.array_equal(store.x[i].cpu().numpy(), xs) and np.array_equal(store.ei[i].cpu().numpy(), ei), i
        assert store.rows[i].dtype == torch.int64 and np.array_equal(store.rows[i].cpu().numpy(), rows), i
        sizes.add(len(rows))
    assert store.x[1].shape[0] == 40 and store.x[2].shape[0] == 1 and store.ei[2].shape == (2, 0) and len(sizes) > 3
    induced = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True)
    assert sum(int(e.shape[1]) for e in induced.ei[3:]) < sum(int(e.shape[1]) for e in store.ei[3:])   # the induced graph is sparser
    with pytest.raises(ValueError, match="lesion_only"):
        T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_random=4)
    with pytest.raises(ValueError, match="exclude"):
        T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True, lesion_knn=8, lesion_random=4)
    with pytest.raises(ValueError, match="graph_seed"):
        T.GraphStore([{k: v for k, v in r.items() if k != "graph_seed"} for r in recs], torch.device(DEV), True, mode="gcn",
                     lesion_only=True, lesion_random=4)


def test_graphmil_step_on_the_lesion_random_store_ragged_stack_equals_the_slow_path():
    """One GraphMIL[gcn] train step, as tests/test_knn_ragged_gpu.py checks it for the lesion k-NN store: the same kernels on
    identical operands, so probabilities, attention, loss and every gradient are equal exactly."""
    from gnn_models import GraphMIL
    from isic_hip import train as T
    recs = _lesion_random_records(9)
    torch.manual_seed(5)
    model = GraphMIL(input_dim=32, gnn_type="gcn", gnn_hidden=64, gnn_layers=2, gnn_dropout=0.3, att_dim=32, att_heads=2,
                     pool_dropout=0.2, classifier_dim=64, classifier_light=True, num_classes=3).to(DEV)
    model.train()
    slow = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True, lesion_random=4, ragged_stack=False)
    fast = T.GraphStore(recs, torch.device(DEV), True, mode="gcn", lesion_only=True, lesion_random=4, ragged_stack=True)
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


def test_05_train_gnns_lesion_random_runs_one_epoch_and_writes_its_csv(tmp_path):
    import pandas as pd
    m05 = _load_script("05_train_gnns.py", "train_gnns_05_random")
    recs = _lesion_random_records(24, n=36)
    splits = ["train"] * 12 + ["val"] * 6 + ["test"] * 6
    gdir, sdir = tmp_path / "graph_outputs" / "synth", tmp_path / "patch_stats" / "synth"
    gdir.mkdir(parents=True), sdir.mkdir(parents=True)
    rows = [{"model_name": "synth", "fold": 0, "split": s, "image_id": r["image_id"], "grid4_edge_index": r["edge_index"],
             "grid8_edge_index": r["edge_index"], "knn_edge_indices": {}, "random_edge_indices": {4: r["edge_index"]}}
            for r, s in zip(recs, splits)]
    pickle.dump(pd.DataFrame(rows), open(gdir / "graph_dataset.pkl", "wb"))
    for split in ("train", "val", "test"):
        part = [{"image_id": r["image_id"], "label": r["y"], "patch_embeddings": r["x"]} for r, s in zip(recs, splits) if s == split]
        pickle.dump(pd.DataFrame(part), open(sdir / f"patch_stats_fold_0_{split}.pkl", "wb"))
    patch = [{"image_path": f"/data/{r['image_id']}.jpg", "segmentation_path": "", "target": r["y"], "patch_id": p,
              "patch_latent": r["x"][p], "patch_in_mask": int(r["keep"][p])} for r in recs for p in range(36)]
    pickle.dump(pd.DataFrame(patch), open(tmp_path / "patch_flags.pkl", "wb"))
    common = ["--root", str(tmp_path), "--gnn", "gcn", "--variants", "random4", "--folds", "0", "--epochs", "1", "--hidden-dim", "32",
              "--graphs-per-step", "4", "--results-csv", "random/common_results.csv"]
    flags = ["--lesion-flags", str(tmp_path / "patch_flags.pkl")]
    with pytest.raises(SystemExit):
        m05.parse_args(common + ["--lesion-random"])                            # needs --lesion-flags
    args = m05.parse_args(common + flags + ["--lesion-random"])
    assert m05.lesion_random_r(args, "random4") == 4 and m05.lesion_random_r(args, "knn8") is None
    # the records the run trains on carry flags and the seeds of 03:136 (row labels 0.. of each split's frame)
    val = m05.load_fold_records(tmp_path, "synth", 0, "val", "random4", m05.load_lesion_flags(args.lesion_flags), graph_seed=42)
    assert [r["graph_seed"] for r in val] == [42 + i for i in range(6)] and all(r["keep"].shape == (36,) for r in val)
    m05.main(common + flags + ["--lesion-random"])
    out = pd.read_csv(tmp_path / "random" / "results_job_0.csv")
    assert len(out) == 1 and out["graph_variant"].iloc[0] == "random4"
    assert np.isfinite(out[["val_accuracy_mean", "test_bacc_mean"]].values).all()


def test_04_measure_heterophily_lesion_random_counts_nodes_and_edges(tmp_path, monkeypatch):
    import pandas as pd
    import build_graphs as bg
    from oracle import graphs
    h04 = _load_script("04_measure_heterophily.py", "h04_random")
    rs = np.random.RandomState(8)
    N, C, fold = 196, 5, 2
    r, c = np.divmod(np.arange(N), 14)
    ellipse = lambda cy, cx, ry, rx: ((r - cy) / ry) ** 2 + ((c - cx) / rx) ** 2 <= 1.0      # noqa: E731
    keep = [ellipse(6.5, 6.5, 4.2, 3.1), np.zeros(N, bool), np.arange(N) == 77, ellipse(3.0, 9.0, 1.2, 1.6)]
    labels = [5, 0, 9, 3]                                                       # index labels of the patch-statistics frame
    grows, prows, frows = [], [], []
    for i, kp in enumerate(keep):
        emb = rs.randn(N, 32).astype(np.float32)
        pp = torch.softmax(torch.from_numpy(rs.randn(N, C).astype(np.float32)) * 2, dim=1).numpy()
        grows.append({"model_name": "m", "fold": fold, "split": "train", "image_id": f"img{i}",
                      "grid4_edge_index": bg._grid_edge_index(False).numpy(), "grid8_edge_index": bg._grid_edge_index(True).numpy(),
                      "knn_edge_indices": {8: graphs.knn_edge_index(torch.from_numpy(emb), 8).numpy()},
                      "random_edge_indices": {4: RR.graph(N, 4, 42 + fold * 10_000 + labels[i]).copy()}})
        prows.append({"image_id": f"img{i}", "label": i % 2, "patch_embeddings": emb, "patch_probs": pp,
                      "dominant_class": pp.argmax(axis=1).astype(np.int64)})
        frows += [{"image_path": f"/data/img{i}.jpg", "patch_id": p, "patch_in_mask": int(kp[p])} for p in range(N)]
    os.makedirs(tmp_path / "g" / "m")
    os.makedirs(tmp_path / "p" / "m")
    pickle.dump(grows, open(tmp_path / "g" / "m" / "graph_dataset.pkl", "wb"))
    pickle.dump(pd.DataFrame(prows, index=labels), open(tmp_path / "p" / "m" / f"patch_stats_fold_{fold}_train.pkl", "wb"))
    pickle.dump(pd.DataFrame(frows), open(tmp_path / "flags.pkl", "wb"))
    base = ["04", "--graph-outputs-root", str(tmp_path / "g"), "--patch-stats-root", str(tmp_path / "p"), "--images-per-launch", "3",
            "--lesion-flags", str(tmp_path / "flags.pkl")]
    monkeypatch.setattr(sys, "argv", base + ["--out-csv", str(tmp_path / "random.csv"), "--lesion-random"])
    h04.main()
    monkeypatch.setattr(sys, "argv", base + ["--out-csv", str(tmp_path / "induced.csv")])
    h04.main()
    rnd, induced = pd.read_csv(tmp_path / "random.csv"), pd.read_csv(tmp_path / "induced.csv")
    assert list(rnd.columns) == list(induced.columns) and list(rnd["graph_variant"]) == list(induced["graph_variant"])
    other = rnd["graph_variant"] != "random4"
    assert set(rnd["graph_variant"][other]) == {"grid4", "grid8", "knn8"}
    pd.testing.assert_frame_equal(rnd[other], induced[other])                     # grid* / knn* rows are as without the option
    rows = rnd[rnd["graph_variant"] == "random4"].reset_index(drop=True)
    assert len(rows) == len(keep)
    for i, kp in enumerate(keep):
        n = int(kp.sum()) or N
        edges = RR.graph(n, 4, 42 + fold * 10_000 + labels[i]).shape[1] if n >= 2 else 0
        assert int(rows["num_nodes"][i]) == n and int(rows["num_edges"][i]) == edges, i
    assert int(rows["num_edges"][0]) > 3 * int(induced[induced["graph_variant"] == "random4"]["num_edges"].iloc[0])
    monkeypatch.setattr(sys, "argv", ["04", "--lesion-random"])
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


def test_resident_heterophily_summary_with_lesion_random():
    import measure_heterophily as mh
    from isic_hip.bags import BagOffsets
    G, N, fold, seed = 5, 196, 1, 7
    outs = _teacher_outputs(G, N, 32, 4, seed=21)
    kh = _keep_rows(G, N, 3)
    keep = torch.from_numpy(kh).to(DEV)
    got = outs.heterophily_summary("random4", fold=fold, seed=seed, keep=keep, lesion_random=True)
    # heterophily_summary_ragged on the restated graphs
    kh2 = kh.copy()
    kh2[~kh2.any(axis=1)] = True
    n = kh2.sum(axis=1)
    seeds = [seed + fold * 10_000 + i for i in range(G)]
    ei, eo = RGR.random_graphs_ragged(seeds, n, (4,))[4]
    flat = np.flatnonzero(kh2.reshape(-1))
    idx = torch.from_numpy(flat).to(DEV)
    offs = BagOffsets.from_lengths(n, DEV)
    want = mh.heterophily_summary_ragged(outs.x.reshape(G * N, -1)[idx].contiguous(), outs.patch_probs.reshape(G * N, -1)[idx],
                                         outs.dominant_class.reshape(G * N)[idx], torch.from_numpy(ei).to(DEV),
                                         torch.from_numpy(eo).to(DEV), offs.device, patch_pos=torch.from_numpy(flat % N).to(DEV),
                                         max_nodes=N)
    assert got["num_nodes"].cpu().tolist() == n.tolist() and got["num_edges"].cpu().tolist() == np.diff(eo).tolist()
    assert set(got) == set(want)
    for key in want:                                                            # the same launches on the same operands (NaN: no edge)
        assert torch.equal(torch.nan_to_num(got[key].double(), nan=-123.0), torch.nan_to_num(want[key].double(), nan=-123.0)), key
    # another variant keeps the induced subgraph; the switch needs keep
    a, b = outs.heterophily_summary("grid4", keep=keep, lesion_random=True), outs.heterophily_summary("grid4", keep=keep)
    assert a["num_edges"].cpu().tolist() == b["num_edges"].cpu().tolist()
    induced = outs.heterophily_summary("random4", fold=fold, seed=seed, keep=keep)
    assert int(induced["num_edges"][2]) < int(got["num_edges"][2])
    with pytest.raises(ValueError, match="keep"):
        outs.heterophily_summary("random4", lesion_random=True)


def test_train_gnn_from_teacher_with_keep_and_lesion_random():
    """The fold fed from resident outputs with ``keep`` / ``lesion_random`` is the fold ``train_gnn_fold`` runs on the same
    records with ``lesion_only=True, lesion_random=4``: the same model, order and kernels, so the metrics are equal exactly."""
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
    got = pipeline.train_gnn_from_teacher(model(), *outs, "random4", fold=2, keep=keeps, lesion_random=True,
                                          rng=np.random.RandomState(0), **fit)
    recs = [o.graph_records("random4", fold=2) for o in outs]
    assert [r["graph_seed"] for r in recs[1]] == [42 + 20_000 + i for i in range(6)]
    for rs, kp in zip(recs, keeps):
        for r, k in zip(rs, kp):
            r["keep"] = k
    want = T.train_gnn_fold(model(), *recs, lesion_only=True, lesion_random=4, rng=np.random.RandomState(0), **fit)
    assert np.isfinite(got[0]["loss"]) and np.isfinite(got[1]["loss"]) and got[2] == want[2]
    for a, b in zip(got[:2], want[:2]):
        assert set(a) == set(b) and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)
    with pytest.raises(ValueError, match="keep"):
        pipeline.train_gnn_from_teacher(model(), *outs, "random4", lesion_random=True, **fit)
