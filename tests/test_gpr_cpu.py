"""GPR-GNN / APPNP without a device: the three C entries declared where they belong with argument checks that answer before
any device work, the self-checks of the restatement (tests/gpr_ref.py) and the construction of the two GraphMIL types."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gpr_ref as R  # noqa: E402
from isic_hip import lib  # noqa: E402
from oracle import gnn  # noqa: E402

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
P = 0x10000                      # a dummy, 16-byte aligned, non-NULL pointer: never dereferenced (errors come first)
NAMES = ("isic_gpr_prop_f32", "isic_gpr_prop_bwd_workspace_bytes", "isic_gpr_prop_bwd_f32")
HEADER = "isic_hip_gpr.h"


def test_entries_are_declared_in_the_new_header_exported_and_parsed():
    inc = os.path.dirname(lib.header_path())
    assert f'#include "{HEADER}"' in open(os.path.join(inc, "isic_hip.h")).read()
    raw = open(os.path.join(inc, HEADER)).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    assert os.path.join(inc, HEADER) in [os.path.normpath(p) for p in lib.extension_header_paths()]
    protos = lib.parse_header(os.path.join(inc, HEADER))
    assert set(protos) == set(NAMES)
    assert [a[1] for a in protos[NAMES[0]][1]] == ["rowptr", "col", "val", "nnz", "node_offsets", "G", "max_nodes", "N", "H", "gamma",
                                                  "K", "F", "bias", "Z", "bad", "stream"]
    assert [a[1] for a in protos[NAMES[2]][1]] == ["rowptr_t", "col_t", "val_t", "nnz", "node_offsets", "G", "max_nodes", "N", "dZ",
                                                  "H", "gamma", "K", "F", "dH", "dgamma", "beta_gamma", "workspace",
                                                  "workspace_bytes", "bad", "stream"]
    assert protos[NAMES[0]][0] is ctypes.c_int and protos[NAMES[2]][0] is ctypes.c_int and protos[NAMES[1]][0] is ctypes.c_size_t
    L = lib.lib()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name not in L.public and name in L.fn and hasattr(cdll, name), name
    for macro, v in (("ISIC_GPR_MAX_NODES", 256), ("ISIC_GPR_MAX_K", 16), ("ISIC_GPR_SLAB", 32)):
        assert f"#define {macro} {v}\n" in raw
    from isic_hip import build, graph
    assert (graph.GPR_MAX_NODES, graph.GPR_MAX_K, graph.GPR_SLAB) == (256, 16, 32) and HEADER in map(os.path.basename, build.header_deps())


def _fwd(rowptr=P, col=P, val=P, nnz=40, off=P, G=2, max_nodes=5, N=9, H=P, gamma=P, K=3, F=7, bias=None, Z=P, bad=P):
    return lib.lib().fn[NAMES[0]](rowptr, col, val, nnz, off, G, max_nodes, N, H, gamma, K, F, bias, Z, bad, None)


def _bwd(rowptr=P, col=P, val=P, nnz=40, off=P, G=2, max_nodes=5, N=9, dZ=P, H=P, gamma=P, K=3, F=7, dH=P, dgamma=P, beta=0.0,
         ws=P, ws_bytes=1 << 20, bad=P):
    return lib.lib().fn[NAMES[2]](rowptr, col, val, nnz, off, G, max_nodes, N, dZ, H, gamma, K, F, dH, dgamma, beta, ws, ws_bytes,
                                  bad, None)


def test_forward_argument_checks_answer_without_a_device():
    for kw in (dict(rowptr=None), dict(col=None), dict(val=None), dict(off=None), dict(H=None), dict(gamma=None), dict(Z=None),
               dict(bad=None), dict(K=17), dict(K=-1), dict(F=0), dict(G=-1), dict(N=-1), dict(nnz=-1), dict(max_nodes=-1),
               dict(off=P + 4), dict(Z=P + 2), dict(bad=P + 2), dict(bias=P + 1)):
        assert _fwd(**kw) == BAD_ARG, kw
    assert _fwd(max_nodes=257) == UNSUPPORTED
    assert _fwd(G=1 << 31) == UNSUPPORTED and _fwd(G=1 << 28, F=768) == UNSUPPORTED       # a grid that would not fit
    assert _fwd(G=0) == OK and _fwd(G=0, rowptr=None, col=None, val=None, off=None, H=None, gamma=None, Z=None, bad=None) == OK
    assert _fwd(G=0, max_nodes=256, K=16) == OK and _fwd(G=0, max_nodes=257) == UNSUPPORTED and _fwd(G=0, K=17) == BAD_ARG


def test_backward_argument_checks_answer_without_a_device():
    for kw in (dict(rowptr=None), dict(col=None), dict(val=None), dict(off=None), dict(dZ=None), dict(gamma=None), dict(bad=None),
               dict(K=17), dict(F=0), dict(G=-1), dict(N=-1), dict(nnz=-1), dict(beta=0.5), dict(H=None), dict(dH=P + 2),
               dict(dgamma=P + 2), dict(off=P + 4)):
        assert _bwd(**kw) == BAD_ARG, kw
    assert _bwd(max_nodes=257) == UNSUPPORTED
    assert _bwd(G=1 << 31) == UNSUPPORTED
    need = lib.lib().fn[NAMES[1]](2, 3, 7)
    assert need == 2 * 1 * 4 * 4 and lib.lib().fn[NAMES[1]](668, 10, 128) == 668 * 4 * 11 * 4
    assert lib.lib().fn[NAMES[1]](5, 3, 33) == 5 * 2 * 4 * 4 and lib.lib().fn[NAMES[1]](0, 3, 7) == 0
    assert _bwd(ws=None) == WORKSPACE and _bwd(ws_bytes=need - 1) == WORKSPACE and _bwd(ws=P + 2) == WORKSPACE
    assert _bwd(dgamma=None, H=None, ws=None, ws_bytes=0, dH=None) == OK          # nothing asked for: no launch
    assert _bwd(G=0, dgamma=None, ws=None, ws_bytes=0) == OK


# ---------------------------------------------------------------------------------------------- the restatement


def _directed_graph(n=23, seed=3, weighted=False):
    gen = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (5 * n,), generator=gen)
    dst = torch.randint(0, n - 1, (5 * n,), generator=gen)            # node n - 1 has no in-edge beyond its self loop
    ei = torch.stack([src, dst])
    ei = torch.cat([ei, ei[:, :3], torch.tensor([[4], [4]])], dim=1)   # duplicates and one explicit self loop
    ew = torch.rand(ei.shape[1], generator=gen, dtype=torch.float64) + 0.5 if weighted else None
    return ei, ew


@pytest.mark.parametrize("weighted", (False, True))
def test_dense_adjacency_is_gcn_norm(weighted):
    """the per-edge loop against oracle/gnn.py's ``gcn_norm`` scattered into a dense matrix, on a directed multigraph"""
    n = 23
    ei, ew = _directed_graph(n, weighted=weighted)
    A = R.dense_adj(ei, n, ew)
    e2, w2 = gnn.gcn_norm(ei, ew, n, dtype=torch.float64)
    B = torch.zeros((n, n), dtype=torch.float64).index_put_((e2[1], e2[0]), w2, accumulate=True)
    assert A.dtype == torch.float64 and not torch.equal(A, A.t())
    assert float((A - B).abs().max()) <= 4 * 2.0 ** -53 * float(B.abs().max())
    x = torch.randn(n, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert float((A @ x - gnn.propagate(x, e2, w2)).abs().max()) < 1e-14
    assert A[n - 1].count_nonzero() == 1 and A[n - 1, n - 1] > 0
    keep = ei[0] != ei[1]
    cin, cout = torch.bincount(ei[1][keep], minlength=n) + 1, torch.bincount(ei[0][keep], minlength=n) + 1
    assert R.max_row_entries(ei, n) == (int(cin.max()), int(cout.max()))


@pytest.mark.parametrize("K,alpha", [(0, 0.1), (1, 0.3), (4, 0.1), (10, 0.1), (16, 0.5), (10, 0.0), (10, 1.0)])
def test_closed_form_is_the_appnp_recurrence(K, alpha):
    n = 23
    ei, ew = _directed_graph(n, weighted=True)
    A = R.dense_adj(ei, n, ew)
    h = torch.randn(n, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    g = R.ppr_gamma(K, alpha)
    assert g.shape == (K + 1,) and abs(float(g.sum()) - 1.0) < 1e-15
    z, x = R.gpr_propagate(h, A, g), R.appnp_recurrence(h, A, K, alpha)
    assert float((z - x).abs().max()) <= 64 * 2.0 ** -53 * float(x.abs().max())
    from isic_hip.graph import gpr_gamma
    assert torch.equal(gpr_gamma(K, alpha), g.float())


def test_k0_is_a_scaled_copy_plus_bias():
    n = 9
    ei, _ = _directed_graph(n)
    A = R.dense_adj(ei, n)
    gen = torch.Generator().manual_seed(5)
    x, W = torch.randn(n, 4, dtype=torch.float64, generator=gen), torch.randn(3, 4, dtype=torch.float64, generator=gen)
    b, g = torch.randn(3, dtype=torch.float64, generator=gen), torch.tensor([-0.7], dtype=torch.float64)
    assert torch.equal(R.gpr_layer(x, A, W, b, g), g[0] * (x @ W.t()) + b)


def test_bound_holds_for_honest_fp32_and_not_for_a_dropped_edge():
    """the dot-product bound on the very batch tests/test_gpr_gpu.py runs (A^ rounded to fp32, as the device holds it): an
    fp32 run of the restatement stays inside it and uses a visible part of it -- forward, dH and dgamma -- and a hop with one
    edge left out leaves it"""
    sizes, offsets, eis, ews = R.kernel_batch()
    gen = torch.Generator().manual_seed(9)
    worst = {"z": 0.0, "dh": 0.0, "dg": 0.0, "wrong": float("inf")}
    for K in (10, 16):
        gamma, Fw = R.mixed_sign_gamma(K).double(), 36
        d = max(R.max_row_entries(ei, n)[0] for n, ei in zip(sizes, eis))
        d_t = max(R.max_row_entries(ei, n)[1] for n, ei in zip(sizes, eis))
        dg32, dg64, dgb = torch.zeros(K + 1), torch.zeros(K + 1, dtype=torch.float64), torch.zeros(K + 1, dtype=torch.float64)
        for n, ei, ew in zip(sizes, eis, ews):
            if n == 0:
                continue
            A = R.dense_adj(ei, n, ew).float().double()
            h, dz = torch.randn(n, Fw, generator=gen).double(), torch.randn(n, Fw, generator=gen).double()
            bias = torch.randn(Fw, generator=gen).double()
            z, (bound, _) = R.gpr_propagate(h, A, gamma, bias), R.propagate_bound(h, A, gamma, d, bias)
            z32 = R.gpr_propagate(h.float(), A.float(), gamma.float(), bias.float()).double()
            worst["z"] = max(worst["z"], float(((z32 - z).abs() / bound).max()))
            dh, (bh, _) = R.gpr_propagate(dz, A.t(), gamma), R.propagate_bound(dz, A.t(), gamma, d_t)
            dh32 = R.gpr_propagate(dz.float(), A.float().t(), gamma.float()).double()
            worst["dh"] = max(worst["dh"], float(((dh32 - dh).abs() / bh).max()))
            ref, b = R.dgamma_ref_and_bound(dz, A, h, K, d_t, dot_len=offsets[-1] * Fw)
            dg64, dgb = dg64 + ref, dgb + b
            dg32 = dg32 + R.dgamma_ref_and_bound(dz.float(), A.float(), h.float(), K, d_t)[0]
            if n >= 63:                          # one edge left out of every hop
                e_drop = int((ei[0] != ei[1]).nonzero()[5])
                wrong = R.gpr_propagate(h, R.dense_adj(ei, n, ew, drop_edge=e_drop).float().double(), gamma, bias)
                worst["wrong"] = min(worst["wrong"], float(((wrong - z).abs() / bound).max()))
        worst["dg"] = max(worst["dg"], float(((dg32.double() - dg64).abs() / dgb).max()))
    print(f"fp32 restatement, worst error / bound: {worst}")
    # (the dgamma bound carries the worst case of a dot product of N F = 25 000 terms and is loose by construction:
    # rounding errors of random signs use a millionth of it)
    assert 1e-3 < worst["z"] <= 1.0 and 1e-3 < worst["dh"] <= 1.0 and 0.0 < worst["dg"] <= 1.0, worst
    assert worst["wrong"] > 100.0, worst


# ---------------------------------------------------------------------------------------------- the model


@pytest.mark.parametrize("gtype", ("gprgnn", "appnp"))
def test_graphmil_constructs_with_the_documented_keys(gtype):
    from gnn_models import GNN_TYPES, GraphMIL
    assert gtype in GNN_TYPES and "sgc" not in GNN_TYPES
    cfg = dict(gnn_type=gtype, gnn_hidden=64, gnn_layers=2, att_dim=16, classifier_dim=24, gpr_k=4)
    m = GraphMIL(32, gtype, 64, 2, att_dim=16, classifier_dim=24, classifier_light=True, gpr_k=4, gpr_alpha=0.2)
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == list(R.graphmil_shapes(32, cfg).items())
    for i in range(2):
        for key in (f"gnn_layers.{i}.lin.weight", f"gnn_layers.{i}.bias", f"gnn_layers.{i}.gamma"):
            assert key in sd
        assert torch.equal(sd[f"gnn_layers.{i}.gamma"], R.ppr_gamma(4, 0.2).float())
        assert float(sd[f"gnn_layers.{i}.bias"].abs().max()) == 0.0
    params, bufs = dict(m.named_parameters()), dict(m.named_buffers())
    assert ("gnn_layers.0.gamma" in params) == (gtype == "gprgnn")
    assert ("gnn_layers.0.gamma" in bufs) == (gtype == "appnp")
    assert m.graph_mode == "gcn" and m.input_proj is not None
    assert GraphMIL(64, gtype, 64, 2).input_proj is None and GraphMIL(32, gtype, 64, 2, use_residual=False).input_proj is None
    assert GraphMIL(64, gtype, 64, 1).gnn_layers[0].gamma.shape == (11,)                    # gpr_k = 10 by default
    assert GraphMIL(64, gtype, 64, 1, gpr_k=0).gnn_layers[0].gamma.tolist() == [1.0]


@pytest.mark.parametrize("kw", [dict(gpr_k=-1), dict(gpr_k=17), dict(gpr_k=2.5), dict(gpr_alpha=-0.01), dict(gpr_alpha=1.01),
                                dict(gpr_alpha=float("nan"))])
def test_graphmil_rejects_k_and_alpha_outside_their_ranges(kw):
    from gnn_models import GraphMIL
    for gtype in ("gprgnn", "appnp", "gcn"):
        with pytest.raises(ValueError):
            GraphMIL(32, gtype, 64, 2, **kw)
    GraphMIL(32, "gprgnn", 64, 1, gpr_k=16, gpr_alpha=1.0)
    GraphMIL(32, "appnp", 64, 1, gpr_k=0, gpr_alpha=0.0)


def test_driver_accepts_the_new_types_and_flags():
    import importlib
    drv = importlib.import_module("05_train_gnns")
    src = open(drv.__file__).read()
    assert '"--gpr-k"' in src and '"--gpr-alpha"' in src and "gpr_k=" in src and "gpr_alpha=" in src
    assert "gprgnn" in drv.GNN_TYPES and "appnp" in drv.GNN_TYPES
