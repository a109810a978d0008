"""The heterophily stage on ragged patch graphs on the MI355X (include/isic_hip_hetero_ragged.h) against the numpy definition
of tests/hetero_ragged_ref.py: one launch of mixed graphs, the uniform case against ``heterophily_summary_device`` bit for
bit, lesion-only graphs through every public layer, invalid input, the size limit, determinism and the 04 script.

Tolerances: per-edge values and their mean / std / median 2e-5 |ref| + 2e-6 (fp32 sums against numpy's, the existing path's
bound); lambda_2 1e-10 absolute against the host fp64 eigensolve; num_edges / num_nodes exact; H_adj, expected and the
compatibility matrix 1e-12 relative plus absolute (integer counts finished in a handful of fp64 operations; 1 - expected >=
0.01 for n <= 196 unless it is exactly 0)."""
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hetero_ragged_ref as HR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 196
STATS = [f"{m}_{s}" for m in ("H_kl", "H_dirichlet", "H_spatial") for s in ("mean", "std", "median")]


def _dev(a, dt=None):
    t = torch.as_tensor(np.asarray(a))
    return t.to(DEV) if dt is None else t.to(DEV, dt)


def _close(a, b, rel, ab):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= rel * abs(b) + ab


# ------------------------------------------------------------------ one launch of mixed graphs
def _edges(rng, n, E, loops=()):
    """E random edges among n nodes without self loops (n == 1: self loops only), then self loops at positions ``loops``."""
    src = rng.integers(0, n, E)
    dst = (src + rng.integers(1, max(n, 2), E)) % n if n > 1 else src.copy()
    for p in loops:
        if p < E:
            dst[p] = src[p]
    return np.stack([src, dst]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def mixed_case(D, C):
    """Node counts 1, 2, 3, 63, 64, 65, 195, 196 and edge counts 0, 1, 255, 256, 257, 513 (either side of the 256-edge chunk of
    the per-graph kernels), self loops at positions 255 and 256, a graph of self loops only, duplicated and antiparallel
    edges, isolated nodes, two components, a one-class graph, shuffled lattice positions.  Returns the host arrays and the
    reference dicts (computed once per (D, C))."""
    rng = np.random.default_rng(100 * D + C)
    graphs = [(1, _edges(rng, 1, 1)),                                             # self loops only
              (1, _edges(rng, 1, 0)),
              (2, _edges(rng, 2, 1)),
              (3, _edges(rng, 3, 255)),
              (63, _edges(rng, 63, 256, loops=(255,))),
              (64, _edges(rng, 64, 257, loops=(255, 256))),
              (65, _edges(rng, 65, 513, loops=(0, 255, 256, 512))),
              (195, _edges(rng, 195, 513)),
              (196, _edges(rng, 196, 257, loops=(256,))),
              (196, _edges(rng, 196, 0)),                                         # isolated nodes only
              (64, _edges(rng, 64, 255, loops=tuple(range(255)))),                # 255 self loops: no edge survives
              (196, _edges(rng, 98, 513))]                                        # nodes 98..195 isolated
    two = _edges(rng, 32, 256)                                                    # two components: 0..31 and 32..63
    two[:, 128:] += 32
    graphs.append((64, two))
    dup = _edges(rng, 65, 257)
    dup[:, 1] = dup[:, 0]                                                         # duplicated
    dup[:, 2] = dup[::-1, 0]                                                      # antiparallel
    dup[:, 3] = dup[::-1, 0]
    graphs.append((65, dup))
    graphs.append((63, _edges(rng, 63, 256)))                                     # the one-class graph (below)
    ns = [n for n, _ in graphs]
    noff = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    eoff = np.concatenate([[0], np.cumsum([e.shape[1] for _, e in graphs])]).astype(np.int64)
    T = int(noff[-1])
    x = rng.standard_normal((T, D)).astype(np.float32)
    probs = torch.softmax(torch.from_numpy(rng.standard_normal((T, C)).astype(np.float32)) * 2, dim=1).numpy()
    dom = rng.integers(0, C, T).astype(np.int32)
    dom[noff[-2]:] = C - 1                                                        # expected = 1 -> H_adj = 1
    pos = np.concatenate([rng.permutation(N)[:n] for n in ns]).astype(np.int32)
    ei = np.concatenate([e for _, e in graphs], axis=1)
    ref = HR.ragged_measures(x, probs, dom, ei, eoff, noff, pos)
    return dict(x=x, probs=probs, dom=dom, ei=ei, eoff=eoff, noff=noff, pos=pos, ns=ns, ref=ref)


def _run_measures(c, max_nodes=N, **over):
    import measure_heterophily as mh
    a = {k: c[k] for k in ("x", "probs", "dom", "ei", "eoff", "noff", "pos")}
    a.update(over)
    return mh._ragged_measures(_dev(a["x"]), _dev(a["probs"]), _dev(a["dom"]), _dev(a["ei"]), _dev(a["eoff"]), _dev(a["noff"]),
                               None if a["pos"] is None else _dev(a["pos"]), max_nodes)


def _assert_graph_outputs(rm, refs, skip=()):
    ne, h_adj, ex = rm["num_edges"].cpu().numpy(), rm["H_adj"].cpu().numpy(), rm["expected"].cpu().numpy()
    compat, lam, bad = rm["H_compat_matrix"].cpu().numpy(), rm["lambda_2"].cpu().numpy(), rm["bad"].cpu().numpy()
    vals, ko = rm["values"].cpu().numpy(), rm["kept_offsets"].cpu().numpy()
    for g, ref in enumerate(refs):
        if g in skip:
            continue
        assert bad[g] == 0 and ne[g] == ref["num_edges"] and ko[g + 1] - ko[g] == ref["num_edges"], g
        print(f"graph {g}: H_adj {h_adj[g]!r} ref {ref['H_adj']!r}  lambda_2 {lam[g]!r} ref {float(ref['lambda_2'][0])!r}")
        assert abs(h_adj[g] - ref["H_adj"]) <= 1e-12 * abs(ref["H_adj"]) + 1e-12, (g, h_adj[g], ref["H_adj"])
        assert abs(ex[g] - ref["expected"]) <= 1e-12 * abs(ref["expected"]) + 1e-12, g
        np.testing.assert_allclose(compat[g], ref["H_compat_matrix"], rtol=1e-12, atol=1e-12)
        assert abs(lam[g] - float(ref["lambda_2"][0])) <= 1e-10, (g, lam[g], ref["lambda_2"])
        for i, k in enumerate(("H_kl", "H_dirichlet", "H_spatial")):
            got, want = vals[i, ko[g]:ko[g + 1]].astype(np.float64), np.asarray(ref[k], np.float64)
            assert (np.abs(got - want) <= 2e-5 * np.abs(want) + 2e-6).all(), (g, k, np.abs(got - want).max())


def _assert_summary(sm, refs, tag=""):
    import measure_heterophily as mh
    assert all(v.is_cuda for v in sm.values())
    rows = mh.summary_records(sm, [{"i": i} for i in range(len(refs))])            # accepts the ragged result unchanged
    for g, (row, ref) in enumerate(zip(rows, refs)):
        want = HR.summarize(ref)
        assert list(row)[:3] == ["i", "num_edges", "num_nodes"]
        assert row["num_edges"] == want["num_edges"] and row["num_nodes"] == want["num_nodes"], (tag, g)
        for k in STATS:
            assert _close(row[k], want[k], 2e-5, 2e-6), (tag, g, k, row[k], want[k])
        for k in ("H_adj_mean", "H_adj_median"):
            assert _close(row[k], want[k], 1e-12, 1e-12), (tag, g, k, row[k], want[k])
        for k in ("lambda_2_mean", "lambda_2_median"):
            assert _close(row[k], want[k], 0.0, 1e-10), (tag, g, k, row[k], want[k])
        assert row["H_adj_std"] == 0.0 and row["lambda_2_std"] == 0.0
        np.testing.assert_allclose(row["H_compat_matrix"], want["H_compat_matrix"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("D, C", [(3, 1), (24, 7), (768, 64)])
def test_one_launch_of_mixed_graphs_equals_the_definition(D, C):
    import measure_heterophily as mh
    c = mixed_case(D, C)
    rm = _run_measures(c)
    _assert_graph_outputs(rm, c["ref"])
    assert abs(float(rm["H_adj"][-1]) - 1.0) == 0.0 and float(rm["expected"][-1]) == 1.0      # the one-class graph
    sm = mh.heterophily_summary_ragged(_dev(c["x"]), _dev(c["probs"]), _dev(c["dom"]), _dev(c["ei"]), _dev(c["eoff"]),
                                       _dev(c["noff"]), patch_pos=_dev(c["pos"]))             # max_nodes read back
    assert set(sm) == set(mh.SUMMARY_STATS) | {"num_nodes", "H_compat_matrix"}
    assert sm["num_nodes"].tolist() == c["ns"]
    _assert_summary(sm, c["ref"], f"mixed D={D} C={C}")


def test_caller_supplied_edge_graph_ids_equal_the_offset_search():
    from isic_hip.lib import call
    c = mixed_case(24, 7)
    E, T, G = c["ei"].shape[1], len(c["dom"]), len(c["ns"])
    gid = np.repeat(np.arange(G), np.diff(c["eoff"])).astype(np.int32)
    x, p, dom, pos, ei, eoff, noff = (_dev(c[k]) for k in ("x", "probs", "dom", "pos", "ei", "eoff", "noff"))
    outs = []
    for g in (None, _dev(gid)):
        o = torch.empty((4, E), device=DEV)
        call("isic_edge_heterophily_ragged_f32", x, p, dom, pos, ei[0], ei[1], eoff, noff, g, G, T, E, 24, 7, 14, 1e-8, o[0], o[1],
             o[2], o[3])
        outs.append(o)
    assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]).all())
    bad = gid.copy()
    bad[5], bad[6] = G, -1                                                        # a graph id outside [0, G): NaN, no read
    o = torch.empty((4, E), device=DEV)
    call("isic_edge_heterophily_ragged_f32", x, p, dom, pos, ei[0], ei[1], eoff, noff, _dev(bad), G, T, E, 24, 7, 14, 1e-8, o[0],
         o[1], o[2], o[3])
    assert bool(torch.isnan(o[:, 5:7]).all())
    keep = torch.ones(E, dtype=torch.bool, device=DEV)
    keep[5:7] = False
    assert torch.equal(o[:, keep], outs[0][:, keep])


def test_two_runs_are_bit_equal():
    c = mixed_case(24, 7)
    a, b = _run_measures(c), _run_measures(c)
    for k in a:
        assert torch.equal(a[k].nan_to_num(nan=-7.0), b[k].nan_to_num(nan=-7.0)), k


# ------------------------------------------------------------------ uniform sizes: the existing path, bit for bit
def test_uniform_graphs_equal_the_equal_size_path_bit_for_bit():
    import build_graphs as bg
    import measure_heterophily as mh
    rs = np.random.RandomState(4)
    G, D, C = 5, 24, 7
    embs = [rs.randn(N, D).astype(np.float32) for _ in range(G)]
    pps = [torch.softmax(torch.from_numpy(rs.randn(N, C).astype(np.float32)) * 2, dim=1).numpy() for _ in range(G)]
    eis = [bg._knn_edge_index(torch.from_numpy(e), k).cpu().numpy() for e, k in zip(embs, (1, 2, 8, 16, 3))]
    eis[2] = np.concatenate([eis[2], np.stack([np.arange(10), np.arange(10)])], axis=1)      # self loops
    eis[3] = np.zeros((2, 0), np.int64)
    X, P = _dev(np.stack(embs)), _dev(np.stack(pps))
    Dm = P.argmax(dim=2).to(torch.int32)
    old = mh.heterophily_summary_device(X, P, Dm, [_dev(e) for e in eis])
    eoff = np.concatenate([[0], np.cumsum([e.shape[1] for e in eis])]).astype(np.int64)
    new = mh.heterophily_summary_ragged(X.reshape(G * N, D), P.reshape(G * N, C), Dm.reshape(-1), _dev(np.concatenate(eis, axis=1)),
                                        _dev(eoff), torch.arange(G + 1, device=DEV) * N, patch_pos=None, max_nodes=N)
    assert torch.equal(new["num_edges"], old["num_edges"]) and new["num_nodes"].tolist() == [N] * G
    for k in STATS + ["lambda_2_mean", "lambda_2_median", "lambda_2_std", "H_adj_std"]:
        assert torch.equal(new[k].nan_to_num(nan=-7.0), old[k].nan_to_num(nan=-7.0)), k
    for k in ("H_adj_mean", "H_adj_median", "H_compat_matrix"):
        assert bool(((new[k] - old[k]).abs() <= 1e-12 * old[k].abs() + 1e-12).all()), k


# ------------------------------------------------------------------ lesion-only graphs through the public layers
def _ellipse(cx, cy, a, b):
    i = np.arange(N)
    return (((i % 14 - cx) / a) ** 2 + ((i // 14 - cy) / b) ** 2 <= 1.0)


@functools.lru_cache(maxsize=None)
def lesion_case():
    from pipeline import DeviceTeacherOutputs
    gen = torch.Generator().manual_seed(6)
    G, D, C = 5, 24, 7
    x = torch.randn(G, N, D, generator=gen).to(DEV)
    pp = torch.softmax(torch.randn(G, N, C, generator=gen) * 2, dim=2).to(DEV)
    outs = DeviceTeacherOutputs(x, pp, torch.rand(G, N).to(DEV), torch.arange(G).to(DEV), [f"i{i}" for i in range(G)])
    keep = np.stack([_ellipse(6.5, 6.5, 4.2, 3.1), np.zeros(N, bool), _ellipse(3.0, 9.0, 2.5, 5.0), np.arange(N) == 77,
                     _ellipse(10.0, 4.0, 6.0, 6.0)])
    return outs, keep


@functools.lru_cache(maxsize=None)
def lesion_ref(variant):
    outs, keep = lesion_case()
    ei = outs.edge_index(variant)
    x, pp, dom = outs.x.cpu().numpy(), outs.patch_probs.cpu().numpy(), outs.dominant_class.cpu().numpy()
    return [HR.lesion_only_measures(x[i], pp[i], dom[i], ei[i].cpu().numpy(), keep[i]) for i in range(len(keep))]


@pytest.mark.parametrize("variant", ["grid8", "knn8", "random3"])
def test_lesion_only_summary_equals_the_definition(variant):
    import measure_heterophily as mh
    outs, keep = lesion_case()
    refs = lesion_ref(variant)
    assert [r["num_nodes"] for r in refs] == [int(keep[0].sum()), N, int(keep[2].sum()), 1, int(keep[4].sum())]
    ei = outs.edge_index(variant)
    sm = mh.heterophily_summary_lesion_only(outs.x, outs.patch_probs, outs.dominant_class, ei, _dev(keep))
    _assert_summary(sm, refs, variant)
    if isinstance(ei, torch.Tensor):                                              # the list form gives the same bits
        sm2 = mh.heterophily_summary_lesion_only(outs.x, outs.patch_probs, outs.dominant_class, [e for e in ei], _dev(keep))
        for k in sm:
            assert torch.equal(sm[k].nan_to_num(nan=-7.0), sm2[k].nan_to_num(nan=-7.0)), k


def test_device_teacher_outputs_heterophily_summary_with_keep():
    outs, keep = lesion_case()
    sm = outs.heterophily_summary("knn8", keep=_dev(keep))
    _assert_summary(sm, lesion_ref("knn8"), "pipeline knn8")
    assert "num_nodes" not in outs.heterophily_summary("knn8")                    # without keep: the equal-size path


def test_compute_edge_heterophily_batch_with_keep_and_unequal_sizes():
    import measure_heterophily as mh
    outs, keep = lesion_case()
    refs = lesion_ref("knn8")
    x, pp, dom = outs.x.cpu().numpy(), outs.patch_probs.cpu().numpy(), outs.dominant_class.cpu().numpy()
    ei = outs.edge_index("knn8").cpu().numpy()
    got = mh.compute_edge_heterophily_batch(list(x), list(pp), list(dom), list(ei), keep=list(keep))
    plain = mh.compute_edge_heterophily_batch(list(x), list(pp), list(dom), list(ei))
    for g, ref, pl in zip(got, refs, plain):
        assert list(g) == list(pl) == ["H_kl", "H_dirichlet", "H_spatial", "H_adj", "lambda_2", "H_compat_matrix"]   # 04:162-169
        for k in ("H_kl", "H_dirichlet", "H_spatial"):                            # the surviving edges, in the reference's order
            want = np.asarray(ref[k], np.float64)
            assert g[k].shape == want.shape and (np.abs(g[k] - want) <= 2e-5 * np.abs(want) + 2e-6).all(), k
        assert abs(g["H_adj"] - ref["H_adj"]) <= 1e-12 * abs(ref["H_adj"]) + 1e-12
        assert g["lambda_2"].shape == (1,) and abs(g["lambda_2"][0] - ref["lambda_2"][0]) <= 1e-10
        np.testing.assert_allclose(g["H_compat_matrix"], ref["H_compat_matrix"], rtol=1e-12, atol=1e-12)
    # images of unequal node count (np.stack would raise): the mixed graphs, one image each, lattice position = node id
    c = mixed_case(24, 7)
    sl = lambda a, off: [a[o0:o1] for o0, o1 in zip(off[:-1], off[1:])]   # noqa: E731
    eis = [c["ei"][:, e0:e1] for e0, e1 in zip(c["eoff"][:-1], c["eoff"][1:])]
    got = mh.compute_edge_heterophily_batch(sl(c["x"], c["noff"]), sl(c["probs"], c["noff"]), sl(c["dom"], c["noff"]), eis)
    refs = HR.ragged_measures(c["x"], c["probs"], c["dom"], c["ei"], c["eoff"], c["noff"], None)
    for g, ref in zip(got, refs):
        want = np.asarray(ref["H_spatial"], np.float64)
        assert g["H_spatial"].shape == want.shape and (np.abs(g["H_spatial"] - want) <= 2e-5 * want + 2e-6).all()
        assert abs(g["H_adj"] - ref["H_adj"]) <= 1e-12 * abs(ref["H_adj"]) + 1e-12


# ------------------------------------------------------------------ invalid input, the size limit
def test_bad_graphs_get_nan_and_their_neighbours_are_unaffected():
    from isic_hip import spectral
    c = mixed_case(24, 7)
    clean = _run_measures(c)
    g, G = 6, len(c["ns"])                                                        # the 65-node graph with 513 edges
    e0, n0 = int(c["eoff"][g]), int(c["noff"][g])

    def check(rm, bad_graph, lam_nan=True, edge=None):
        assert rm["bad"].cpu().tolist() == [1 if i == bad_graph else 0 for i in range(G)]
        assert int(rm["num_edges"][bad_graph]) == 0
        assert bool(torch.isnan(rm["H_adj"][bad_graph])) and bool(torch.isnan(rm["expected"][bad_graph]))
        assert bool(torch.isnan(rm["H_compat_matrix"][bad_graph]).all())
        assert bool(torch.isnan(rm["lambda_2"][bad_graph])) == lam_nan
        others = torch.arange(G, device=DEV) != bad_graph
        for k in ("num_edges", "H_adj", "expected", "H_compat_matrix", "lambda_2"):
            assert torch.equal(rm[k][others], clean[k][others]), k
        # the neighbours' compacted values: the same bits, moved up by the bad graph's missing edges
        ko, kc = rm["kept_offsets"].cpu().numpy(), clean["kept_offsets"].cpu().numpy()
        for i in range(G):
            if i != bad_graph:
                assert torch.equal(rm["values"][:, ko[i]:ko[i + 1]], clean["values"][:, kc[i]:kc[i + 1]]), i

    for v in (65, -1, 2 ** 40):                                                   # an endpoint outside [0, n)
        ei = c["ei"].copy()
        ei[1, e0 + 7] = v
        check(_run_measures(c, ei=ei), g)
    for v in (7, -1, 2 ** 31 - 1):                                                # a class outside [0, C): lambda_2 knows no class
        dom = c["dom"].copy()
        dom[n0 + 3] = v
        check(_run_measures(c, dom=dom), g, lam_nan=False)
    eoff = c["eoff"].copy()
    eoff[-1] += 5                                                                 # the last graph's edges leave the arrays
    check(_run_measures(c, eoff=eoff), G - 1)
    noff = c["noff"].copy()
    noff[-1] += 3                                                                 # the last graph's nodes leave the arrays
    check(_run_measures(c, noff=noff), G - 1, lam_nan=False)
    eoff = c["eoff"].copy()
    eoff[g + 1] = eoff[g] - 1                                                     # decreasing offsets: graph g and, as its own
    rm = _run_measures(c, eoff=eoff)                                              # segment now starts early, nothing else
    assert rm["bad"][g] == 1 and bool(torch.isnan(rm["lambda_2"][g])) and bool(torch.isnan(rm["H_adj"][g]))
    # a graph above the stated max_nodes: NaN for that graph, no fault
    lam = spectral.laplacian_lambda2_ragged(_dev(c["ei"][0]), _dev(c["ei"][1]), _dev(c["eoff"]), _dev(c["noff"]), 64).cpu().numpy()
    for i, n in enumerate(c["ns"]):
        assert np.isnan(lam[i]) == (n > 64), i
        if n <= 64:
            assert lam[i] == float(clean["lambda_2"][i])


def test_graphs_above_196_nodes_are_unsupported():
    import measure_heterophily as mh
    from isic_hip import lib, spectral
    c = mixed_case(24, 7)
    args = [_dev(c[k]) for k in ("x", "probs", "dom", "ei", "eoff", "noff")]
    with pytest.raises(lib.IsicHipError) as ei:
        mh.heterophily_summary_ragged(*args, max_nodes=197)
    assert ei.value.code == -2
    with pytest.raises(lib.IsicHipError) as ei:
        spectral.laplacian_lambda2_ragged(args[3][0], args[3][1], args[4], args[5], 197)
    assert ei.value.code == -2
    z = torch.zeros((2, 197, 4), device=DEV)
    with pytest.raises(lib.IsicHipError) as ei:
        mh.heterophily_summary_lesion_only(z, z, z[:, :, 0], torch.zeros((2, 2, 0), dtype=torch.int64, device=DEV),
                                           torch.ones((2, 197), device=DEV))
    assert ei.value.code == -2
    none = mh.heterophily_summary_ragged(*[a[:0] for a in args[:3]], args[3][:, :0], args[4][:1], args[5][:1])
    assert none["num_nodes"].numel() == 0 and none["H_compat_matrix"].shape == (0, 7, 7)       # no graphs: nothing launched


# ------------------------------------------------------------------ the 04 script
def test_04_lesion_flags_csv_and_the_unchanged_default(tmp_path, monkeypatch):
    import importlib.util
    import build_graphs as bg
    import measure_heterophily as mh
    import pandas as pd
    spec = importlib.util.spec_from_file_location("h04_ragged", os.path.join(os.path.dirname(mh.__file__), "04_measure_heterophily.py"))
    h04 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(h04)
    rs = np.random.RandomState(8)
    C, n_img = 7, 5
    keep = [_ellipse(6.5, 6.5, 4.2, 3.1), np.zeros(N, bool), _ellipse(3.0, 9.0, 2.5, 5.0), np.arange(N) == 77,
            _ellipse(10.0, 4.0, 6.0, 6.0)]
    grows, prows, frows = [], [], []
    for i in range(n_img):
        emb = rs.randn(N, 16).astype(np.float32)
        pp = torch.softmax(torch.from_numpy(rs.randn(N, C).astype(np.float32)) * 2, dim=1).numpy()
        grows.append({"model_name": "m", "fold": 0, "split": "train", "image_id": f"img{i}",
                      "grid4_edge_index": bg._grid_edge_index(False).numpy(), "grid8_edge_index": bg._grid_edge_index(True).numpy(),
                      "knn_edge_indices": {8: bg._knn_edge_index(torch.from_numpy(emb), 8).cpu().numpy()},
                      "random_edge_indices": {3: bg._random_edge_index(N, 3, 100 + 10 * i).numpy()}})
        prows.append({"image_id": f"img{i}", "label": i % 2, "patch_embeddings": emb, "patch_probs": pp,
                      "dominant_class": pp.argmax(axis=1).astype(np.int64)})
        frows += [{"image_path": f"/data/img{i}.jpg", "patch_id": p, "patch_in_mask": int(keep[i][p])} for p in range(N)]
    os.makedirs(tmp_path / "g" / "m")
    os.makedirs(tmp_path / "p" / "m")
    pickle.dump(grows, open(tmp_path / "g" / "m" / "graph_dataset.pkl", "wb"))
    pickle.dump(prows, open(tmp_path / "p" / "m" / "patch_stats_fold_0_train.pkl", "wb"))
    pickle.dump(pd.DataFrame(frows), open(tmp_path / "flags.pkl", "wb"))
    base = ["04", "--graph-outputs-root", str(tmp_path / "g"), "--patch-stats-root", str(tmp_path / "p"), "--images-per-launch", "3"]
    monkeypatch.setattr(sys, "argv", base + ["--out-csv", str(tmp_path / "lesion.csv"), "--lesion-flags", str(tmp_path / "flags.pkl")])
    h04.main()
    monkeypatch.setattr(sys, "argv", base + ["--out-csv", str(tmp_path / "full.csv")])
    h04.main()
    lesion, full = pd.read_csv(tmp_path / "lesion.csv"), pd.read_csv(tmp_path / "full.csv")
    meta = ["model_name", "fold", "split", "image_id", "label", "graph_variant", "graph_type", "graph_param"]
    assert list(full.columns) == meta + mh.SUMMARY_STATS                          # without the flag: today's CSV
    assert list(lesion.columns) == meta + ["num_edges", "num_nodes"] + mh.SUMMARY_STATS[1:]
    today = h04.build_master_summary(str(tmp_path / "g"), str(tmp_path / "p"), images_per_launch=3)
    assert list(today.columns) == meta + mh.SUMMARY_STATS + ["H_compat_matrix"]
    pd.testing.assert_frame_equal(full, pd.read_csv(_csv(today.drop(columns=["H_compat_matrix"]), tmp_path / "today.csv")))
    variants = ["grid4", "grid8", "knn8", "random3"]
    assert list(lesion["graph_variant"]) == [v for v in variants for _ in range(n_img)]
    i = 0
    for v in variants:
        for k, (gr, pr) in enumerate(zip(grows, prows)):
            ei = mh.edge_index_from_variant({**gr, **pr}, v)
            for frame, kp in ((lesion, keep[k]), (full, np.ones(N, bool))):
                want = HR.summarize(HR.lesion_only_measures(pr["patch_embeddings"], pr["patch_probs"], pr["dominant_class"], ei, kp))
                got = frame.iloc[i]
                assert got["image_id"] == pr["image_id"] and int(got["num_edges"]) == want["num_edges"]
                if frame is lesion:
                    assert int(got["num_nodes"]) == want["num_nodes"]
                for s in STATS:
                    assert _close(got[s], want[s], 2e-5, 2e-6), (v, k, s, got[s], want[s])
                assert _close(got["H_adj_mean"], want["H_adj_mean"], 1e-12, 1e-12) and _close(got["lambda_2_mean"], want["lambda_2_mean"], 0.0, 1e-10)
            i += 1


def _csv(df, path):
    df.to_csv(path, index=False)
    return path
