"""CPU-only checks of the heterophily stage on ragged patch graphs (include/isic_hip_hetero_ragged.h,
tests/hetero_ragged_ref.py): the numpy definition against a per-edge loop and, with every node kept, against the reference's
own output; the four entry points declared, exported and known to the header parser; and their argument checks -- BAD_ARG
before UNSUPPORTED, the no-op cases -- which all answer before any device work."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hetero_ragged_ref as HR  # noqa: E402
from helpers import load_golden  # noqa: E402
from isic_hip import lib  # noqa: E402

NAMES = ("isic_edge_heterophily_ragged_f32", "isic_graph_homophily_ragged", "isic_edge_values_compact_ragged_f32",
         "isic_laplacian_lambda2_ragged_f64")
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call
BIG = 2 ** 31


# ------------------------------------------------------------------ the definition against a per-edge loop
def _brute(x, probs, dom, src, dst, pos, C):
    n = len(dom)
    kl, di, sp, same = [], [], [], []
    pair = [[0] * C for _ in range(C)]
    for s, d in zip(src, dst):
        if s == d:
            continue
        kl.append(sum(float(probs[s][c]) * math.log((float(probs[s][c]) + 1e-8) / (float(probs[d][c]) + 1e-8)) for c in range(C)))
        di.append(0.5 * sum((float(a) - float(b)) ** 2 for a, b in zip(x[s], x[d])))
        sp.append(math.hypot(pos[s] % 14 - pos[d] % 14, pos[s] // 14 - pos[d] // 14))
        same.append(dom[s] == dom[d])
        pair[dom[s]][dom[d]] += 1
    edge_h = sum(same) / len(same) if same else 0.0
    expected = sum((sum(1 for v in dom if v == k) / max(1, n)) ** 2 for k in range(C))
    h_adj = (edge_h - expected) / (1.0 - expected) if expected < 1.0 else 1.0
    compat = [[v / sum(row) if sum(row) else 0.0 for v in row] for row in pair]
    return kl, di, sp, h_adj, expected, compat


@pytest.mark.parametrize("n, E, C, D, keep", [(1, 3, 1, 3, "all"), (2, 5, 7, 3, "none"), (37, 300, 7, 24, "random"),
                                              (37, 300, 3, 5, "one"), (64, 0, 7, 4, "random"), (50, 257, 64, 8, "alternate")])
def test_definition_equals_a_per_edge_loop(n, E, C, D, keep):
    rng = np.random.default_rng(n * 1000 + E)
    x = rng.standard_normal((n, D)).astype(np.float32)
    probs = torch.softmax(torch.from_numpy(rng.standard_normal((n, C)).astype(np.float32)) * 2, dim=1).numpy()
    dom = probs.argmax(axis=1).astype(np.int32)
    src, dst = rng.integers(0, n, E), rng.integers(0, n, E)
    if E > 4:
        src[1], dst[1] = src[0], dst[0]                                  # a duplicated edge
        dst[2] = src[2]                                                  # a self loop
    k = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "random": rng.random(n) < 0.5, "one": np.arange(n) == n // 2,
         "alternate": np.arange(n) % 2 == 0}[keep]
    got = HR.lesion_only_measures(x, probs, dom, np.stack([src, dst]), k)
    kk = k if k.any() else np.ones(n, bool)
    rows = np.nonzero(kk)[0]
    new = {int(r): i for i, r in enumerate(rows)}
    es = [(new[int(s)], new[int(d)]) for s, d in zip(src, dst) if kk[s] and kk[d]]
    kl, di, sp, h_adj, expected, compat = _brute(x[rows], probs[rows], dom[rows].tolist(), [e[0] for e in es], [e[1] for e in es],
                                                 rows.tolist(), C)
    assert got["num_nodes"] == len(rows) and got["num_edges"] == len(kl)
    np.testing.assert_allclose(got["H_kl"], kl, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["H_dirichlet"], di, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["H_spatial"], sp, rtol=1e-12, atol=0)
    assert abs(got["H_adj"] - h_adj) < 1e-12 and abs(got["expected"] - expected) < 1e-12
    np.testing.assert_allclose(got["H_compat_matrix"], compat, rtol=1e-12, atol=0)


def test_every_node_kept_is_the_reference_output():
    """N = 196, every node kept, patch_pos = the node id: the definition is the oracle, which tests/golden/heterophily.npz (the
    reference's own compute_edge_heterophily) pins; checked directly here on the raw edge list (self loops, duplicates)."""
    from oracle import formula, heterophily
    g = load_golden("heterophily.npz")
    N, D, C = int(g["N"]), int(g["D"]), int(g["C"])
    emb = formula.formula_input(N, D, phase=0.4).numpy()
    pp = torch.softmax(formula.formula_input(N, C, phase=1.1) * 3.0, dim=1).numpy()
    dom = pp.argmax(axis=1).astype(np.int32)
    ei = np.asarray(g["edge_index"])
    ref = heterophily.edge_heterophily(emb, pp, dom, ei)
    for got in (HR.lesion_only_measures(emb, pp, dom, ei, np.ones(N, bool)), HR.lesion_only_measures(emb, pp, dom, ei, np.zeros(N, bool)),
                HR.ragged_measures(emb, pp, dom, ei, [0, ei.shape[1]], [0, N])[0]):
        assert got["num_nodes"] == N
        for k in ("H_kl", "H_dirichlet", "H_spatial", "H_compat_matrix", "lambda_2"):
            assert np.array_equal(got[k], ref[k]), k
        assert got["H_adj"] == ref["H_adj"]
        for k in ("H_kl", "H_dirichlet", "H_spatial", "H_compat_matrix"):
            np.testing.assert_allclose(got[k], g[f"raw.{k}"], rtol=1e-5, atol=1e-6, err_msg=k)
        assert abs(got["H_adj"] - float(g["raw.H_adj"])) < 1e-9
        np.testing.assert_allclose(got["lambda_2"], g["raw.lambda_2"], rtol=1e-5, atol=1e-6)
        s = HR.summarize(got)
        assert s["num_edges"] == int(g["raw.sum.num_edges"])
        for k in ("H_kl_mean", "H_kl_std", "H_kl_median", "H_dirichlet_mean", "H_spatial_median", "H_adj_mean", "lambda_2_mean"):
            assert abs(s[k] - float(g[f"raw.sum.{k}"])) <= 2e-5 * abs(float(g[f"raw.sum.{k}"])) + 2e-6, k


def test_lesion_flag_helpers_are_shared_by_the_two_scripts():
    import importlib.util
    import lesion_flags
    pkg = os.path.join(ROOT, "multimodal-isic_amd")
    spec = importlib.util.spec_from_file_location("gnn05_for_flags", os.path.join(pkg, "05_train_gnns.py"))
    m05 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m05)
    assert m05.load_lesion_flags is lesion_flags.load_lesion_flags and m05._keep_flags is lesion_flags._keep_flags
    text = open(os.path.join(pkg, "04_measure_heterophily.py")).read()
    assert "from lesion_flags import" in text and "--lesion-flags" in text


# ------------------------------------------------------------------ the ABI without a device
def test_hetero_ragged_entry_points_are_declared_exported_and_parsed():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_hetero_ragged.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(inc, "isic_hip_hetero_ragged.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    assert os.path.join(inc, "isic_hip_hetero_ragged.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    protos = lib.parse_header(os.path.join(inc, "isic_hip_hetero_ragged.h"))
    assert set(protos) == set(NAMES)
    assert [len(protos[n][1]) for n in NAMES] == [21, 15, 10, 9]
    for n in NAMES:
        assert protos[n][0] is ctypes.c_int and protos[n][1][-1][1] == "stream", n
    edge = {a[1]: a for a in protos[NAMES[0]][1]}
    assert edge["patch_pos"][2] and edge["edge_graph"][2] and edge["T"][0] is ctypes.c_int64 and edge["eps"][0] is ctypes.c_float
    lam = {a[1]: a for a in protos[NAMES[3]][1]}
    assert lam["max_nodes"][0] is ctypes.c_int and lam["node_offsets"][2] and lam["E"][0] is ctypes.c_int64
    L = lib.lib()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name not in L.public and name in L.fn and hasattr(cdll, name), name
    from isic_hip import spectral
    import measure_heterophily as mh
    for f in (spectral.laplacian_lambda2_ragged, mh.heterophily_summary_ragged, mh.heterophily_summary_lesion_only):
        assert callable(f)


_EDGE_PTRS = ("x", "probs", "dominant_class", "patch_pos", "src", "dst", "edge_offsets", "node_offsets", "edge_graph")
_EDGE_OUTS = ("h_kl", "h_dirichlet", "h_spatial", "same_class")


def _edge(G=3, T=10, E=20, D=8, C=7, grid_w=14, **kw):
    a = {k: P for k in _EDGE_PTRS + _EDGE_OUTS}
    a.update(kw)
    return lib.lib().fn[NAMES[0]](*[a[k] for k in _EDGE_PTRS], G, T, E, D, C, grid_w, 1e-8, *[a[k] for k in _EDGE_OUTS], None)


_HOMO_PTRS = ("dominant_class", "src", "dst", "edge_offsets", "node_offsets")
_HOMO_OUTS = ("num_edges", "h_adj", "expected", "compat", "bad")


def _homophily(G=3, T=10, E=20, C=7, **kw):
    a = {k: P for k in _HOMO_PTRS + _HOMO_OUTS}
    a.update(kw)
    return lib.lib().fn[NAMES[1]](*[a[k] for k in _HOMO_PTRS], G, T, E, C, *[a[k] for k in _HOMO_OUTS], None)


_COMPACT_PTRS = ("values", "src", "dst", "edge_offsets", "kept_offsets")


def _compact(G=3, M=3, E=20, **kw):
    a = {k: P for k in _COMPACT_PTRS + ("out",)}
    a.update(kw)
    return lib.lib().fn[NAMES[2]](*[a[k] for k in _COMPACT_PTRS], G, M, E, a["out"], None)


_LAM_PTRS = ("src", "dst", "edge_offsets", "node_offsets")


def _lambda2(G=3, E=20, max_nodes=196, **kw):
    a = {k: P for k in _LAM_PTRS + ("lambda2",)}
    a.update(kw)
    return lib.lib().fn[NAMES[3]](*[a[k] for k in _LAM_PTRS], G, E, max_nodes, a["lambda2"], None)


def test_edge_heterophily_ragged_argument_checks_without_a_device():
    for kw in (dict(G=-1), dict(T=-1), dict(E=-1), dict(D=0), dict(C=0), dict(grid_w=0)):
        assert _edge(**kw) == BAD_ARG, kw
    for k in set(_EDGE_PTRS + _EDGE_OUTS) - {"patch_pos", "edge_graph"}:
        assert _edge(**{k: None}) == BAD_ARG, k
    assert _edge(T=BIG) == UNSUPPORTED and _edge(E=BIG) == UNSUPPORTED
    assert _edge(D=0, E=BIG) == BAD_ARG and _edge(x=None, T=BIG) == BAD_ARG      # a bad argument before an unsupported size
    nothing = {k: None for k in _EDGE_PTRS + _EDGE_OUTS}
    assert _edge(G=0, **nothing) == OK and _edge(G=0, T=BIG, E=BIG, **nothing) == OK          # no graphs: nothing touched
    assert _edge(E=0, src=None, dst=None, **{k: None for k in _EDGE_OUTS}) == OK              # no edges: nothing launched


def test_graph_homophily_ragged_argument_checks_without_a_device():
    for kw in (dict(G=-1), dict(T=-1), dict(E=-1), dict(C=0)):
        assert _homophily(**kw) == BAD_ARG, kw
    for k in _HOMO_PTRS + _HOMO_OUTS:
        assert _homophily(**{k: None}) == BAD_ARG, k
    assert _homophily(C=65) == UNSUPPORTED and _homophily(T=BIG) == UNSUPPORTED and _homophily(E=BIG) == UNSUPPORTED
    assert _homophily(C=65, bad=None) == BAD_ARG and _homophily(C=65, E=-1) == BAD_ARG
    assert _homophily(G=0, C=65, **{k: None for k in _HOMO_PTRS + _HOMO_OUTS}) == OK


def test_edge_values_compact_ragged_argument_checks_without_a_device():
    for kw in (dict(G=-1), dict(M=-1), dict(E=-1)):
        assert _compact(**kw) == BAD_ARG, kw
    for k in _COMPACT_PTRS + ("out",):
        assert _compact(**{k: None}) == BAD_ARG, k
    assert _compact(E=BIG) == UNSUPPORTED and _compact(E=BIG, out=None) == BAD_ARG
    assert _compact(G=0, E=BIG, **{k: None for k in _COMPACT_PTRS + ("out",)}) == OK
    assert _compact(M=0, values=None, out=None) == OK and _compact(E=0, values=None, src=None, dst=None, out=None) == OK


def test_lambda2_ragged_argument_checks_without_a_device():
    for kw in (dict(G=-1), dict(E=-1), dict(max_nodes=-1)):
        assert _lambda2(**kw) == BAD_ARG, kw
    for k in _LAM_PTRS + ("lambda2",):
        assert _lambda2(**{k: None}) == BAD_ARG, k
    assert _lambda2(max_nodes=197) == UNSUPPORTED and _lambda2(E=BIG) == UNSUPPORTED
    assert _lambda2(max_nodes=197, lambda2=None) == BAD_ARG and _lambda2(max_nodes=197, G=-1) == BAD_ARG
    assert _lambda2(G=0, max_nodes=197, E=BIG, **{k: None for k in _LAM_PTRS + ("lambda2",)}) == OK
