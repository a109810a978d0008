"""The native heterophily stage on the MI355X: ``isic_laplacian_lambda2_f64`` (lambda_2 of the symmetrised normalised
Laplacian, 04_measure_heterophily.py:149-159) against a dense fp64 eigensolve of the same Laplacian built on the host,
``isic_segment_stats_f32`` (04:172-181) against numpy, and ``heterophily_summary_device`` / the 04 script against the
numpy summaries and the reference golden."""
import os
import pickle

import numpy as np
import pytest
import torch

from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 196


def host_lambda2(src, dst, n):
    """The reference's construction (04:149-159) in numpy fp64: summed duplicates, no self loops, max(A, A^T)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    keep = src != dst
    A = np.zeros((n, n))
    np.add.at(A, (src[keep], dst[keep]), 1.0)
    A = np.maximum(A, A.T)
    deg = A.sum(axis=1)
    dis = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    L = np.eye(n) - dis[:, None] * A * dis[None, :]
    return float(np.linalg.eigvalsh(L)[1]) if n > 1 else 0.0


def native(graphs, n):
    """graphs: list of local edge arrays [2, E_i] -> lambda_2 of every graph from ONE launch."""
    from isic_hip import spectral
    src = np.concatenate([np.asarray(e[0], dtype=np.int64) + i * n for i, e in enumerate(graphs)])
    dst = np.concatenate([np.asarray(e[1], dtype=np.int64) + i * n for i, e in enumerate(graphs)])
    offs = np.concatenate([[0], np.cumsum([np.asarray(e).shape[1] for e in graphs])]).astype(np.int64)
    t = lambda a: torch.as_tensor(a).to(DEV)
    return spectral.laplacian_lambda2(t(src), t(dst), t(offs), len(graphs), n).cpu().numpy()


def check(graphs, n, atol=1e-10):
    got = native(graphs, n)
    ref = np.array([host_lambda2(e[0], e[1], n) for e in graphs])
    np.testing.assert_allclose(got, ref, rtol=0, atol=atol)
    return got


def golden_row():
    import build_graphs as bg
    from oracle import formula
    g = load_golden("heterophily.npz")
    n, D, C = int(g["N"]), int(g["D"]), int(g["C"])
    emb = formula.formula_input(n, D, phase=0.4).numpy()
    pp = torch.softmax(formula.formula_input(n, C, phase=1.1) * 3.0, dim=1).numpy()
    row = {"patch_embeddings": emb, "patch_probs": pp, "dominant_class": pp.argmax(axis=1).astype(np.int32),
           "edge_index": g["edge_index"], "grid4_edge_index": bg._grid_edge_index(False).numpy(),
           "grid8_edge_index": bg._grid_edge_index(True).numpy(),
           "knn_edge_indices": {k: bg._knn_edge_index(torch.from_numpy(emb), k).cpu().numpy() for k in (3, 8)},
           "random_edge_indices": {2: bg._random_edge_index(n, 2, 44).numpy()}}
    return g, row


VARIANTS = (None, "grid4", "grid8", "knn3", "knn8", "random2")


def test_lambda2_golden_variants_vs_host_and_reference():
    import measure_heterophily as mh
    g, row = golden_row()
    eis = [np.asarray(row["edge_index"]) if v is None else mh.edge_index_from_variant(row, v) for v in VARIANTS]
    got = check(eis, N)
    for v, lam in zip(VARIANTS, got):
        np.testing.assert_allclose(lam, float(np.asarray(g[f"{v or 'raw'}.lambda_2"]).reshape(-1)[0]), rtol=1e-5, atol=1e-6)


def test_lambda2_knn_and_random_graphs():
    import build_graphs as bg
    rs = np.random.RandomState(5)
    emb = torch.from_numpy(rs.randn(N, 32).astype(np.float32))
    eis = [bg._knn_edge_index(emb, k).cpu().numpy() for k in (1, 2, 4, 8, 16)]
    eis += [bg._random_edge_index(N, r, 7 + r).numpy() for r in (1, 16)]
    check(eis, N)


def test_lambda2_multiplicities_isolated_and_disconnected():
    n = 6
    # (0,1) twice and (1,0) once -> weight 2 both ways; (1,2) three times and (2,1) twice -> 3; chain to 3; 4, 5 isolated
    asym = np.array([[0, 0, 1, 1, 1, 1, 2, 2, 2, 3], [1, 1, 0, 2, 2, 2, 1, 1, 3, 2]])
    got = check([asym], n)
    # max differs from sum and from OR: the three constructions give three different lambda_2 (here the isolated nodes
    # make lambda_2 = 0, so compare on the connected part)
    sub = asym.copy()
    lam_max = check([sub], 4)[0]
    A = np.zeros((4, 4))
    np.add.at(A, (sub[0], sub[1]), 1.0)
    for W in (A + A.T, ((A + A.T) > 0).astype(float)):
        d = W.sum(1)
        Ls = np.eye(4) - W / np.sqrt(np.outer(d, d))
        assert abs(np.linalg.eigvalsh(Ls)[1] - lam_max) > 1e-3
    # isolated nodes 4, 5: identity rows of L (d^-1/2 = 0) add the eigenvalue 1, lambda_2 stays the connected part's
    assert abs(got[0] - lam_max) < 1e-12
    two = np.array([[0, 1, 2, 3, 4, 5], [1, 2, 0, 4, 5, 3]])           # two triangles: disconnected, lambda_2 = 0
    lam = check([two, np.zeros((2, 0), np.int64)], n)
    assert abs(lam[0]) < 1e-12 and abs(lam[1] - 1.0) < 1e-12         # no edges at all: L = I


@pytest.mark.parametrize("n", [1, 2, 3, 64, 195, 196])
def test_lambda2_node_counts(n):
    rs = np.random.RandomState(n)
    graphs = [rs.randint(0, n, size=(2, 4 * n)) for _ in range(3)]
    graphs.append(np.stack([np.arange(n), (np.arange(n) + 1) % n]))     # a cycle (with self loops for n == 1)
    got = check(graphs, n)
    if n == 1:
        assert (got == 0.0).all()


def test_lambda2_batch_of_1000_graphs():
    rs = np.random.RandomState(11)
    graphs = [rs.randint(0, N, size=(2, int(rs.randint(0, 8 * N)))) for _ in range(1000)]
    got = native(graphs, N)
    for i in np.random.RandomState(12).choice(1000, 12, replace=False):
        assert abs(got[i] - host_lambda2(graphs[i][0], graphs[i][1], N)) < 1e-10, i
    assert np.array_equal(got, native(graphs, N))                   # fixed order: bit-identical from run to run


def test_lambda2_errors_and_bad_ids():
    import measure_heterophily as mh
    from isic_hip import lib, spectral
    L = lib.lib()
    z = torch.zeros(4, dtype=torch.int64, device=DEV)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    rc = L.fn["isic_laplacian_lambda2_f64"](z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 197, out.data_ptr(), None)
    assert rc == -2
    with pytest.raises(lib.IsicHipError) as ei:
        spectral.laplacian_lambda2(z, z, z[:2], 1, 197)
    assert ei.value.code == -2
    # lambda2_batch still answers above 196 nodes (eigvalsh)
    rs = np.random.RandomState(2)
    e = rs.randint(0, 197, size=(2, 800))
    e = e[:, e[0] != e[1]]
    got = mh.lambda2_batch(torch.as_tensor(e[0]).to(DEV), torch.as_tensor(e[1]).to(DEV), 1, 197)
    assert abs(float(got[0]) - host_lambda2(e[0], e[1], 197)) < 1e-10
    # an id outside its graph: NaN for that graph only
    graphs = [rs.randint(0, 50, size=(2, 200)) for _ in range(3)]
    bad = [g.copy() for g in graphs]
    bad[1][1, 7] = 50
    lam = native(bad, 50)
    assert np.isnan(lam[1]) and np.isfinite(lam[[0, 2]]).all()
    np.testing.assert_allclose(lam[[0, 2]], [host_lambda2(g[0], g[1], 50) for g in (graphs[0], graphs[2])], atol=1e-10)
    bad[1][1, 7] = -1
    assert np.isnan(native(bad, 50)[1])
    # decreasing offsets: NaN, neighbours unaffected
    src = torch.as_tensor(np.concatenate([g[0] + i * 50 for i, g in enumerate(graphs)])).to(DEV)
    dst = torch.as_tensor(np.concatenate([g[1] + i * 50 for i, g in enumerate(graphs)])).to(DEV)
    offs = torch.tensor([0, 200, 150, 600], dtype=torch.int64, device=DEV)
    lam = spectral.laplacian_lambda2(src, dst, offs, 3, 50).cpu().numpy()
    assert np.isnan(lam[1]) and np.isfinite(lam[0])
    # lambda2_batch accepts edges in any order
    perm = torch.randperm(src.numel(), generator=torch.Generator().manual_seed(0)).to(DEV)
    got = mh.lambda2_batch(src[perm], dst[perm], 3, 50).cpu().numpy()
    np.testing.assert_allclose(got, [host_lambda2(g[0], g[1], 50) for g in graphs], atol=1e-10)


def test_segment_stats_vs_numpy():
    from isic_hip import lib, spectral
    rs = np.random.RandomState(9)
    lens = [7, 8, 0, 1, 2, 5, 16384, 1000, 33]
    M = 3
    segs = [[rs.randn(n).astype(np.float32) for n in lens] for _ in range(M)]
    segs[1][5] = np.array([2, 2, 1, 2, 1], np.float32)              # ties
    segs[2][1] = np.array([3, 3, 3, 3, 1, 1, 1, 1], np.float32)
    vals = np.stack([np.concatenate(s) for s in segs])
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    mean, std, med = spectral.segment_stats(torch.as_tensor(vals).to(DEV), torch.as_tensor(offs).to(DEV), max(lens))
    mean, std, med = (t.cpu().numpy() for t in (mean, std, med))
    for m in range(M):
        for g, n in enumerate(lens):
            if n == 0:
                assert np.isnan(mean[m, g]) and np.isnan(std[m, g]) and np.isnan(med[m, g])
                continue
            x = segs[m][g].astype(np.float64)
            for got, ref in ((mean[m, g], np.mean(x)), (std[m, g], np.std(x)), (med[m, g], np.median(x))):
                assert abs(got - ref) <= 1e-12 * max(abs(ref), 1e-300) + 1e-15, (m, g, got, ref)
    big = torch.zeros((1, 16385), device=DEV)
    two = torch.tensor([0, 16385], dtype=torch.int64, device=DEV)
    with pytest.raises(lib.IsicHipError) as ei:
        spectral.segment_stats(big, two, 16385)
    assert ei.value.code == -2
    # a wrong bound: the over-long segment gets NaN instead of a fault
    out = spectral.segment_stats(big, two, 100)
    assert all(bool(torch.isnan(t).all()) for t in out)


def _numpy_summaries(embs, pps, doms, eis):
    import measure_heterophily as mh
    return [mh.summarize_image(em, {}) for em in mh.compute_edge_heterophily_batch(embs, pps, doms, eis)]


def _assert_summary(dev_sum, refs, tag=""):
    import measure_heterophily as mh
    assert all(v.is_cuda for v in dev_sum.values())
    rows = mh.summary_records(dev_sum, [{} for _ in refs])
    for i, (row, ref) in enumerate(zip(rows, refs)):
        assert row["num_edges"] == ref["num_edges"]
        for k in mh.SUMMARY_STATS[1:]:
            a, b = row[k], ref[k]
            if np.isnan(b):
                assert np.isnan(a), (tag, i, k)
                continue
            assert abs(a - b) <= 2e-5 * abs(b) + 2e-6, (tag, i, k, a, b)
        np.testing.assert_allclose(row["H_compat_matrix"], ref["H_compat_matrix"], rtol=2e-5, atol=2e-6)


def test_device_summary_vs_numpy_and_golden():
    import measure_heterophily as mh
    g, row = golden_row()
    for v in VARIANTS:
        ei = np.asarray(row["edge_index"]) if v is None else mh.edge_index_from_variant(row, v)
        t = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a)).to(DEV, dt).unsqueeze(0)
        sm = mh.heterophily_summary_device(t(row["patch_embeddings"]), t(row["patch_probs"]), t(row["dominant_class"], torch.int32),
                                           [torch.as_tensor(ei).to(DEV)])
        ref = _numpy_summaries([row["patch_embeddings"]], [row["patch_probs"]], [row["dominant_class"]], [ei])
        _assert_summary(sm, ref, v)
        rec = mh.summary_records(sm, [{}])[0]
        tag = v or "raw"
        assert rec["num_edges"] == int(g[f"{tag}.sum.num_edges"])
        for k in ("H_kl_mean", "H_kl_std", "H_kl_median", "H_dirichlet_mean", "H_spatial_median", "H_adj_mean", "lambda_2_mean"):
            assert abs(rec[k] - float(g[f"{tag}.sum.{k}"])) <= 2e-5 * abs(float(g[f"{tag}.sum.{k}"])) + 2e-6, (tag, k)
    # a batch: ragged list (with self loops, an empty graph) and the [G, 2, E] form
    import build_graphs as bg
    rs = np.random.RandomState(4)
    G, C = 6, 7
    embs = [rs.randn(N, 24).astype(np.float32) for _ in range(G)]
    pps = [torch.softmax(torch.from_numpy(rs.randn(N, C).astype(np.float32)) * 2, dim=1).numpy() for _ in range(G)]
    doms = [p.argmax(axis=1).astype(np.int32) for p in pps]
    eis = [bg._knn_edge_index(torch.from_numpy(e), k).cpu().numpy() for e, k in zip(embs, (1, 2, 4, 8, 16, 3))]
    eis[2] = np.concatenate([eis[2], np.stack([np.arange(10), np.arange(10)])], axis=1)      # self loops
    eis[4] = np.zeros((2, 0), np.int64)
    X = torch.as_tensor(np.stack(embs)).to(DEV)
    P = torch.as_tensor(np.stack(pps)).to(DEV)
    Dm = torch.as_tensor(np.stack(doms)).to(DEV)
    sm = mh.heterophily_summary_device(X, P, Dm, [torch.as_tensor(e).to(DEV) for e in eis])
    _assert_summary(sm, _numpy_summaries(embs, pps, doms, eis), "ragged")
    eis8 = [bg._knn_edge_index(torch.from_numpy(e), 8).cpu().numpy() for e in embs]
    sm = mh.heterophily_summary_device(X, P, Dm, torch.as_tensor(np.stack(eis8)).to(DEV))
    _assert_summary(sm, _numpy_summaries(embs, pps, doms, eis8), "dense")


def test_device_teacher_outputs_heterophily_summary():
    from pipeline import DeviceTeacherOutputs
    gen = torch.Generator().manual_seed(6)
    G, D, C = 5, 32, 7
    x = torch.randn(G, N, D, generator=gen).to(DEV)
    pp = torch.softmax(torch.randn(G, N, C, generator=gen) * 2, dim=2).to(DEV)
    outs = DeviceTeacherOutputs(x, pp, torch.rand(G, N).to(DEV), torch.arange(G).to(DEV), [f"i{i}" for i in range(G)])
    sm = outs.heterophily_summary("knn8")
    assert all(v.is_cuda for v in sm.values())
    assert sm["lambda_2_mean"].shape == (G,) and sm["H_compat_matrix"].shape == (G, C, C)
    ei = outs.edge_index("knn8").cpu().numpy()
    ref = _numpy_summaries(list(x.cpu().numpy()), list(pp.cpu().numpy()), list(outs.dominant_class.cpu().numpy()), list(ei))
    _assert_summary(sm, ref, "knn8")


def test_04_build_master_summary_matches_per_image_numpy(tmp_path):
    import importlib.util
    import build_graphs as bg
    import measure_heterophily as mh
    spec = importlib.util.spec_from_file_location("h04", os.path.join(os.path.dirname(mh.__file__), "04_measure_heterophily.py"))
    h04 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(h04)
    rs = np.random.RandomState(8)
    C, n_img = 7, 5
    grows, prows = [], []
    for i in range(n_img):
        emb = rs.randn(N, 16).astype(np.float32)
        pp = torch.softmax(torch.from_numpy(rs.randn(N, C).astype(np.float32)) * 2, dim=1).numpy()
        grows.append({"model_name": "m", "fold": 0, "split": "train", "image_id": f"img{i}",
                      "grid4_edge_index": bg._grid_edge_index(False).numpy(), "grid8_edge_index": bg._grid_edge_index(True).numpy(),
                      "knn_edge_indices": {k: bg._knn_edge_index(torch.from_numpy(emb), k).cpu().numpy() for k in (2, 8)},
                      "random_edge_indices": {r: bg._random_edge_index(N, r, 100 + 10 * i + r).numpy() for r in (1, 3)}})
        prows.append({"image_id": f"img{i}", "label": i % 2, "patch_embeddings": emb, "patch_probs": pp,
                      "dominant_class": pp.argmax(axis=1).astype(np.int64)})
    os.makedirs(tmp_path / "g" / "m")
    os.makedirs(tmp_path / "p" / "m")
    pickle.dump(grows, open(tmp_path / "g" / "m" / "graph_dataset.pkl", "wb"))
    pickle.dump(prows, open(tmp_path / "p" / "m" / "patch_stats_fold_0_train.pkl", "wb"))
    df = h04.build_master_summary(str(tmp_path / "g"), str(tmp_path / "p"), images_per_launch=3)
    variants = ["grid4", "grid8", "knn2", "knn8", "random1", "random3"]
    assert len(df) == n_img * len(variants)
    assert list(df["graph_variant"]) == [v for v in variants for _ in range(n_img)]
    i = 0
    for v in variants:
        for gr, pr in zip(grows, prows):
            row = {**gr, **pr}
            ref = mh.summarize_image(mh.compute_edge_heterophily(row, graph_variant=v), {})
            got = df.iloc[i]
            assert got["image_id"] == pr["image_id"] and got["label"] == pr["label"]
            assert int(got["num_edges"]) == ref["num_edges"]
            for k in mh.SUMMARY_STATS[1:]:
                assert abs(got[k] - ref[k]) <= 2e-5 * abs(ref[k]) + 2e-6, (v, i, k)
            np.testing.assert_allclose(got["H_compat_matrix"], ref["H_compat_matrix"], rtol=2e-5, atol=2e-6)
            i += 1
    cols = list(df.columns)
    assert cols[:8] == ["model_name", "fold", "split", "image_id", "label", "graph_variant", "graph_type", "graph_param"]
    assert cols[8:] == mh.SUMMARY_STATS + ["H_compat_matrix"]


def test_laplacian_lambda2_torch_op():
    from torch.library import opcheck
    from isic_hip import torch_ops  # noqa: F401
    rs = np.random.RandomState(1)
    n, G = 40, 4
    e = rs.randint(0, n, size=(2, G * 100)) + np.repeat(np.arange(G) * n, 100)
    src, dst = (torch.as_tensor(a).to(DEV) for a in e)
    offs = torch.arange(0, G * 100 + 1, 100, dtype=torch.int64, device=DEV)
    opcheck(torch.ops.isic_hip.laplacian_lambda2.default, (src, dst, offs, n))
    got = torch.ops.isic_hip.laplacian_lambda2(src, dst, offs, n).cpu().numpy()
    ref = [host_lambda2(e[0, g * 100:(g + 1) * 100] - g * n, e[1, g * 100:(g + 1) * 100] - g * n, n) for g in range(G)]
    np.testing.assert_allclose(got, ref, atol=1e-10)
