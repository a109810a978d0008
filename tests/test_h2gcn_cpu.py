"""H2GCN without a device: the four C entries declared where they belong with argument checks that answer before any device
work, the self-checks of the restatement (tests/h2gcn_ref.py) and the construction of ``GraphMIL(gnn_type='h2gcn')``.

The tests of the entries, of ``from_parts``, of the model and of the driver fail without the feature.  The self-checks of the
restatement (path, star, complete graph, symmetry and invariance, the CSR restatement, the bound) and
``test_other_types_keep_their_state_dict_keys`` exercise only tests/h2gcn_ref.py resp. the other types: they need no library
code of this feature and pass with or without it -- they pin the definition that the GPU tests compare the kernels with."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import h2gcn_ref as R  # noqa: E402
from isic_hip import lib  # noqa: E402

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
P = 0x10000                      # a dummy, 16-byte aligned, non-NULL pointer: never dereferenced (errors come first)
NAMES = ("isic_two_hop_count", "isic_two_hop_write", "isic_h2_prop_f32", "isic_h2_prop_bwd_f32")
HEADER = "isic_hip_h2.h"


def test_entries_are_declared_in_the_new_header_exported_and_parsed():
    inc = os.path.dirname(lib.header_path())
    assert f'#include "{HEADER}"' in open(os.path.join(inc, "isic_hip.h")).read()
    raw = open(os.path.join(inc, HEADER)).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    assert os.path.join(inc, HEADER) in [os.path.normpath(p) for p in lib.extension_header_paths()]
    protos = lib.parse_header(os.path.join(inc, HEADER))
    assert set(protos) == set(NAMES)
    assert [a[1] for a in protos[NAMES[0]][1]] == ["rowptr", "col", "nnz", "node_offsets", "G", "max_nodes", "N", "deg1", "deg2",
                                                  "bad", "stream"]
    assert [a[1] for a in protos[NAMES[1]][1]] == ["rowptr", "col", "nnz", "node_offsets", "G", "max_nodes", "N", "rowptr1",
                                                  "rowptr2", "nnz1", "nnz2", "col1", "val1", "perm1", "col2", "val2", "perm2",
                                                  "bad", "stream"]
    assert [a[1] for a in protos[NAMES[2]][1]] == ["rowptr1", "col1", "val1", "nnz1", "rowptr2", "col2", "val2", "nnz2",
                                                  "node_offsets", "G", "max_nodes", "N", "H", "ldh", "F", "Z", "ldz", "bad", "stream"]
    assert [a[1] for a in protos[NAMES[3]][1]] == ["rowptr1", "col1", "val1", "nnz1", "rowptr2", "col2", "val2", "nnz2",
                                                  "node_offsets", "G", "max_nodes", "N", "dZ", "ldz", "F", "dH", "ldh", "bad", "stream"]
    L = lib.lib()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert protos[name][0] is ctypes.c_int
        assert name in L.extension and name not in L.public and name in L.fn and hasattr(cdll, name), name
    for macro, v in (("ISIC_H2_MAX_NODES", 256), ("ISIC_H2_SLAB", 32)):
        assert f"#define {macro} {v}\n" in raw
    from isic_hip import build, graph
    assert (graph.H2_MAX_NODES, graph.H2_SLAB) == (256, 32) and HEADER in map(os.path.basename, build.header_deps())


def _count(rowptr=P, col=P, nnz=40, off=P, G=2, max_nodes=5, N=9, deg1=P, deg2=P, bad=P):
    return lib.lib().fn[NAMES[0]](rowptr, col, nnz, off, G, max_nodes, N, deg1, deg2, bad, None)


def _write(rowptr=P, col=P, nnz=40, off=P, G=2, max_nodes=5, N=9, rp1=P, rp2=P, nnz1=7, nnz2=9, col1=P, val1=P, perm1=P, col2=P,
           val2=P, perm2=P, bad=P):
    return lib.lib().fn[NAMES[1]](rowptr, col, nnz, off, G, max_nodes, N, rp1, rp2, nnz1, nnz2, col1, val1, perm1, col2, val2,
                                  perm2, bad, None)


def _prop(which=2, rp1=P, col1=P, val1=P, nnz1=7, rp2=P, col2=P, val2=P, nnz2=9, off=P, G=2, max_nodes=5, N=9, X=P, ldx=None, F=7,
          out=P, ldo=None, bad=P):
    # forward: X = H (ldh), out = Z (ldz); backward: X = dZ (ldz), out = dH (ldh)
    ldh, ldz = F, 2 * F
    if which == 2:
        ldx, ldo = (ldh if ldx is None else ldx), (ldz if ldo is None else ldo)
    else:
        ldx, ldo = (ldz if ldx is None else ldx), (ldh if ldo is None else ldo)
    return lib.lib().fn[NAMES[which]](rp1, col1, val1, nnz1, rp2, col2, val2, nnz2, off, G, max_nodes, N, X, ldx, F, out, ldo, bad,
                                      None)


def test_builder_argument_checks_answer_without_a_device():
    for kw in (dict(rowptr=None), dict(col=None), dict(off=None), dict(deg1=None), dict(deg2=None), dict(bad=None), dict(G=-1),
               dict(N=-1), dict(nnz=-1), dict(max_nodes=-1), dict(off=P + 4), dict(deg1=P + 2), dict(bad=P + 2)):
        assert _count(**kw) == BAD_ARG, kw
    assert _count(max_nodes=257) == UNSUPPORTED and _count(N=1 << 31) == UNSUPPORTED and _count(G=1 << 31) == UNSUPPORTED
    assert _count(G=0) == OK and _count(G=0, rowptr=None, col=None, off=None, deg1=None, deg2=None, bad=None) == OK
    assert _count(G=0, max_nodes=256) == OK and _count(G=0, max_nodes=257) == UNSUPPORTED
    for kw in (dict(rowptr=None), dict(col=None), dict(off=None), dict(rp1=None), dict(rp2=None), dict(col1=None), dict(val2=None),
               dict(perm1=None), dict(bad=None), dict(nnz1=-1), dict(nnz2=-1), dict(off=P + 4), dict(val1=P + 2), dict(perm2=P + 1)):
        assert _write(**kw) == BAD_ARG, kw
    assert _write(max_nodes=257) == UNSUPPORTED and _write(nnz2=1 << 31) == UNSUPPORTED
    assert _write(G=0) == OK and _write(nnz1=0, col1=None, val1=None, perm1=None, G=0) == OK


@pytest.mark.parametrize("which", (2, 3))
def test_propagation_argument_checks_answer_without_a_device(which):
    for kw in (dict(rp1=None), dict(col1=None), dict(val2=None), dict(rp2=None), dict(off=None), dict(X=None), dict(out=None),
               dict(bad=None), dict(F=0), dict(G=-1), dict(N=-1), dict(nnz1=-1), dict(nnz2=-1), dict(max_nodes=-1), dict(off=P + 4),
               dict(out=P + 2), dict(X=P + 2), dict(bad=P + 2), dict(val1=P + 1)):
        assert _prop(which, **kw) == BAD_ARG, kw
    # the row strides: ldh >= F and ldz >= 2 F
    small_x, small_o = (6, 13) if which == 2 else (13, 6)
    assert _prop(which, ldx=small_x) == BAD_ARG and _prop(which, ldo=small_o) == BAD_ARG
    assert _prop(which, max_nodes=257) == UNSUPPORTED
    assert _prop(which, G=1 << 31) == UNSUPPORTED and _prop(which, G=1 << 28, F=768) == UNSUPPORTED    # a grid that would not fit
    assert _prop(which, G=0) == OK and _prop(which, G=0, max_nodes=257) == UNSUPPORTED and _prop(which, G=0, F=0) == BAD_ARG
    assert _prop(which, G=0, ldx=1 << 20, ldo=1 << 20) == OK


# ---------------------------------------------------------------------------------------------- the restatement
def _pairs(A):
    return {(int(i), int(j)) for i, j in zip(*np.nonzero(A))}


def test_path_gives_the_distance_2_pairs():
    n = 9
    A1, A2 = R.two_hop_dense(R.path_edges(n), n)
    assert _pairs(A1) == {(i, j) for i in range(n) for j in range(n) if abs(i - j) == 1}
    assert _pairs(A2) == {(i, j) for i in range(n) for j in range(n) if abs(i - j) == 2}


def test_star_gives_the_clique_of_the_leaves():
    n = 7
    A1, A2 = R.two_hop_dense(R.star_edges(n), n)
    assert _pairs(A1) == {(0, j) for j in range(1, n)} | {(j, 0) for j in range(1, n)}
    assert _pairs(A2) == {(i, j) for i in range(1, n) for j in range(1, n) if i != j}
    assert not A2[0].any()


def test_complete_graph_has_no_2_hop_pair():
    A1, A2 = R.two_hop_dense(R.complete_edges(6), 6)
    assert int(A1.sum()) == 30 and not A2.any()


@pytest.mark.parametrize("n", (1, 2, 3, 23, 65))
def test_a2_is_symmetric_disjoint_and_invariant(n):
    """symmetric, disjoint from A1 and from the diagonal, equal to the thresholded square of A1, and unchanged when the edges
    are reversed, repeated or joined by self loops"""
    rng = np.random.default_rng(n)
    ei = R.knn_like_edges(n, 3, rng)
    A1, A2 = R.two_hop_dense(ei, n)
    assert (A1 == A1.T).all() and (A2 == A2.T).all()
    assert not (A1 & A2).any() and not np.diag(A1).any() and not np.diag(A2).any()
    sq = (A1.astype(np.int64) @ A1.astype(np.int64)) > 0
    assert (A2 == (sq & ~A1 & ~np.eye(n, dtype=bool))).all()
    loops = np.stack([np.arange(n), np.arange(n)])
    for other in (ei[::-1], np.concatenate([ei, ei], axis=1), np.concatenate([loops, ei, loops], axis=1),
                  ei[:, rng.permutation(ei.shape[1])]):
        B1, B2 = R.two_hop_dense(other, n)
        assert (B1 == A1).all() and (B2 == A2).all()


def test_the_csr_restatement_is_canonical_and_its_perm_an_involution():
    n = 40
    ei = R.knn_like_edges(n, 4, np.random.default_rng(1))
    for A in R.two_hop_dense(ei, n):
        deg, rowptr, col, val, perm = R.csr_of(A)
        row = np.repeat(np.arange(n), deg)
        assert rowptr[-1] == A.sum() == col.size and (np.diff(rowptr) == deg).all()
        assert all((np.diff(col[rowptr[i]:rowptr[i + 1]]) > 0).all() for i in range(n))
        assert (perm[perm] == np.arange(col.size)).all() and (col[perm] == row).all() and (row[perm] == col).all()
        assert val.dtype == np.float32 and (val == val[perm]).all()
        An = R.normalise(A).numpy()
        np.testing.assert_allclose(val, An[row, col], rtol=3 * 2.0 ** -24)
    # a node without any edge: a zero row, no division by zero
    deg, rowptr, col, val, perm = R.csr_of(np.zeros((3, 3), dtype=bool))
    assert deg.tolist() == [0, 0, 0] and col.size == 0 and not R.normalise(np.zeros((3, 3))).any()


def test_bound_holds_for_honest_fp32_and_not_for_a_dropped_entry():
    """the dot-product bound of tests/test_h2gcn_gpu.py on its own batch: an fp32 run of the restatement stays inside it and
    uses a visible part of it, and Z with ONE 2-hop entry left out leaves it"""
    sizes, offsets, eis = R.kernel_batch()
    gen = torch.Generator().manual_seed(3)
    worst, wrong = 0.0, float("inf")
    for n, ei in zip(sizes, eis):
        if n < 2:
            continue
        A1, A2 = R.two_hop_dense(ei, n)
        h = torch.randn(n, 33, generator=gen)
        for A in (A1, A2):
            An = R.normalise(A, torch.float32).double()
            m = int(A.sum(axis=1).max()) + 2
            bound = R.dot_bound(An, h.double(), m)
            z, z32 = An @ h.double(), (An.float() @ h).double()
            worst = max(worst, float(((z32 - z).abs() / bound.clamp_min(1e-300)).max()))
            if A is A2 and A.any():
                i, j = (int(v[0]) for v in np.nonzero(A))
                Ad = An.clone()
                Ad[i, j] = 0.0
                wrong = min(wrong, float((((Ad @ h.double()) - z).abs() / bound.clamp_min(1e-300)).max()))
    print(f"fp32 restatement, worst error / bound {worst:.4f}; a dropped entry {wrong:.1f}")
    assert 1e-3 < worst <= 1.0 and wrong > 100.0


# ---------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("layers", (1, 2, 3))
def test_graphmil_constructs_with_the_documented_widths_and_keys(layers):
    from gnn_models import GNN_TYPES, GraphMIL, _GRAPH_MODE
    assert "h2gcn" in GNN_TYPES and _GRAPH_MODE["h2gcn"] == "h2"
    cfg = dict(gnn_type="h2gcn", gnn_hidden=64, gnn_layers=layers, att_dim=16, classifier_dim=24)
    m = GraphMIL(32, "h2gcn", 64, layers, att_dim=16, classifier_dim=24, classifier_light=True)
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(R.graphmil_shapes(32, cfg).items())
    assert not any(k.startswith("gnn_layers") for k in sd)
    assert len(m.gnn_layers) == layers
    for i, layer in enumerate(m.gnn_layers):
        assert not list(layer.parameters()) and not list(layer.buffers()) and not layer.state_dict()
        assert m.layer_norms[i].normalized_shape == (2 ** (i + 1) * 64,)
    assert m.final_gnn_dim == (2 ** (layers + 1) - 1) * 64 and m.graph_mode == "h2"
    assert m.attention_layers[0][0].in_features == m.final_gnn_dim and m.classifier[0].in_features == m.final_gnn_dim
    # input_proj: whenever input_dim != gnn_hidden, with or without the residual (as fagcn and gcnii)
    assert m.input_proj is not None and GraphMIL(32, "h2gcn", 64, 1, use_residual=False).input_proj is not None
    assert GraphMIL(64, "h2gcn", 64, 1).input_proj is None
    assert GraphMIL(32, "h2gcn", 64, 2, use_layer_norm=False).layer_norms is None


def test_graphmil_raises_above_4096_columns():
    from gnn_models import GraphMIL
    GraphMIL(32, "h2gcn", 64, 5)                                   # 63 x 64 = 4032
    assert GraphMIL(32, "h2gcn", 585, 2).final_gnn_dim == 4095
    for hidden, layers in ((64, 6), (586, 2), (1366, 1), (1024, 2)):
        with pytest.raises(ValueError, match="4096"):
            GraphMIL(32, "h2gcn", hidden, layers)
    GraphMIL(32, "gcn", 2049, 1)                                   # the limit is h2gcn's alone


def test_other_types_keep_their_state_dict_keys():
    """the new type changes no other type's parameters: same keys and shapes as before it existed (gprgnn: tests/gpr_ref.py)"""
    import gpr_ref
    from gnn_models import GraphMIL
    cfg = dict(gnn_type="gprgnn", gnn_hidden=64, gnn_layers=2, att_dim=16, classifier_dim=24, gpr_k=4)
    m = GraphMIL(32, "gprgnn", 64, 2, att_dim=16, classifier_dim=24, classifier_light=True, gpr_k=4)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == list(gpr_ref.graphmil_shapes(32, cfg).items())
    assert GraphMIL(64, "gcn", 64, 2, use_residual=False).input_proj is None
    assert GraphMIL(32, "gcn", 64, 2, use_residual=False).input_proj is None


def test_from_parts_takes_sym_and_no_build_does():
    from isic_hip import graph as G
    assert G.SYM_MODE == "sym" and "sym" not in G.GraphBatch.MODES and G.TwoHopGraph.mode == "h2"
    with pytest.raises(ValueError):
        G.GraphBatch.from_parts(3, 0, "nonsense", {})
    assert G.H2_RESIDENT_DEFAULT in (True, False) and G.h2_last_path() in (None, "resident", "composed")


def test_driver_accepts_the_new_type():
    import importlib
    drv = importlib.import_module("05_train_gnns")
    assert "h2gcn" in drv.GNN_TYPES
    assert drv.parse_args(["--gnn", "h2gcn"]).gnn == ["h2gcn"]
