"""CPU-only checks of the k-NN graphs among patch sets of unequal size (include/isic_hip_knn_ragged.h, tests/knn_ragged_ref.py):
the analytic edge offsets against the restatement, the restatement against the reference-generated golden k-NN vectors, the
two entry points declared, exported and known to the header parser, and their argument checks, which answer before any
device work."""
import ctypes
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

import knn_ragged_ref as KR  # noqa: E402
from helpers import load_golden  # noqa: E402
from isic_hip import lib  # noqa: E402
from oracle import formula  # noqa: E402

NAMES = ("isic_knn_graph_ragged", "isic_knn_edges_ragged")
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call
SIZES = (0, 1, 2, 3, 17, 40, 196)
KS = (1, 3, 8, 16)


def test_knn_edge_offsets_equal_the_restatement():
    from isic_hip.graph import knn_edge_counts, knn_edge_offsets
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    x = torch.randn(int(offs[-1]), 6, generator=torch.Generator().manual_seed(0))
    got = knn_edge_offsets(SIZES, KS)
    assert list(got) == list(KS)
    for q, k in enumerate(KS):
        ei, eo = KR.knn_edges_ragged(x, offs, k)
        assert got[k].dtype == np.int64 and got[k].tolist() == eo.tolist() and ei.shape == (2, eo[-1]), k
        kk = [0 if n < 2 else max(1, min(k, n - 1)) for n in SIZES]                     # 03_build_graphs.py:42-45
        assert np.diff(got[k]).tolist() == [n * c for n, c in zip(SIZES, kk)]
        assert knn_edge_counts(SIZES, KS)[q].tolist() == np.diff(got[k]).tolist()
    assert knn_edge_offsets([], KS)[8].tolist() == [0]


def test_restatement_equals_the_reference_generated_golden_lists():
    g = load_golden("graphs.npz")
    for tag, n, dd in (("a", 196, 768), ("b", 64, 512), ("c", 17, 8)):
        xg = formula.gapped_points(n, dd, seed=n)
        for k in KS:
            ei, eo = KR.knn_edges_ragged(xg, [0, n], k)
            assert eo.tolist() == [0, n * min(k, n - 1)] and np.array_equal(ei.numpy(), g[f"knn.{tag}.{k}"]), (tag, k)
    # the clamp, and a batch: every graph's slice is its own list, global ids add the graph's first row
    x5 = formula.gapped_points(5, 4, seed=5)
    assert np.array_equal(KR.knn_edges_ragged(x5, [0, 5], 99)[0].numpy(), g["knn.clampk"])
    xb = torch.cat([x5, torch.zeros(1, 4), x5])
    ei, eo = KR.knn_edges_ragged(xb, [0, 5, 5, 6, 11], 99)
    eg, _ = KR.knn_edges_ragged(xb, [0, 5, 5, 6, 11], 99, global_ids=True)
    assert eo.tolist() == [0, 20, 20, 20, 40]
    assert np.array_equal(ei[:, :20].numpy(), g["knn.clampk"]) and np.array_equal(ei[:, 20:].numpy(), g["knn.clampk"])
    assert np.array_equal(eg[:, 20:].numpy(), g["knn.clampk"] + 6) and np.array_equal(eg[:, :20].numpy(), g["knn.clampk"])


def test_entry_points_are_declared_exported_and_parsed():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_knn_ragged.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(inc, "isic_hip_knn_ragged.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    assert os.path.join(inc, "isic_hip_knn_ragged.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    protos = lib.parse_header(os.path.join(inc, "isic_hip_knn_ragged.h"))
    assert set(protos) == set(NAMES) and [len(protos[n][1]) for n in NAMES] == [10, 14]
    for n in NAMES:
        assert protos[n][0] is ctypes.c_int and protos[n][1][-1][1] == "stream", n
    knn = {a[1]: a for a in protos[NAMES[0]][1]}
    assert knn["total_nodes"][0] is ctypes.c_int64 and knn["nn_dist"][2] and knn["max_nodes"][0] is ctypes.c_int
    edges = {a[1]: a for a in protos[NAMES[1]][1]}
    assert edges["total_edges"][0] is ctypes.c_int64 and edges["k_values"][2] and edges["bad"][2] and edges["edge_base"][2]
    L = lib.lib()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name not in L.public and name in L.fn and hasattr(cdll, name), name


def _knn(G=3, D=64, k=8, max_nodes=100, total_nodes=50, **kw):
    a = dict(x=P, offsets=P, nn_idx=P, nn_dist=P)
    a.update(kw)
    return lib.lib().fn[NAMES[0]](a["x"], a["offsets"], G, D, k, max_nodes, total_nodes, a["nn_idx"], a["nn_dist"], None)


def test_knn_graph_ragged_argument_checks():
    for kw in (dict(D=48), dict(D=16), dict(k=17), dict(max_nodes=209), dict(G=2 ** 22 + 1)):
        assert _knn(**kw) == UNSUPPORTED, kw
    for kw in (dict(G=-1), dict(D=0), dict(k=0), dict(max_nodes=-1), dict(total_nodes=-1), dict(x=None), dict(offsets=None),
               dict(nn_idx=None)):
        assert _knn(**kw) == BAD_ARG, kw
    for kw in (dict(G=0), dict(total_nodes=0), dict(G=0, x=None, offsets=None, nn_idx=None), dict(max_nodes=0)):
        assert _knn(**kw) == OK, kw                                                   # no-ops: nothing is launched


def _edges(kmax=8, G=3, total_nodes=50, ks=(1, 3), K=None, total_edges=100, **kw):
    a = dict(nn_idx=P, offsets=P, edge_base=P, src_out=P, dst_out=P, bad=P)
    a.update(kw)
    kv = (ctypes.c_int32 * max(len(ks), 1))(*ks)
    kptr = kw.get("k_values", ctypes.addressof(kv))
    return lib.lib().fn[NAMES[1]](a["nn_idx"], kmax, a["offsets"], G, total_nodes, kptr, len(ks) if K is None else K,
                                  a["edge_base"], total_edges, 0, a["src_out"], a["dst_out"], a["bad"], None)


def test_knn_edges_ragged_argument_checks():
    for kw in (dict(kmax=0), dict(G=-1), dict(total_nodes=-1), dict(total_edges=-1), dict(K=0), dict(ks=tuple(range(1, 18))),
               dict(ks=(3, 0)), dict(k_values=None), dict(offsets=None), dict(edge_base=None), dict(src_out=None),
               dict(dst_out=None), dict(bad=None), dict(nn_idx=None)):
        assert _edges(**kw) == BAD_ARG, kw
    for kw in (dict(total_nodes=2 ** 31), dict(kmax=65537), dict(G=2 ** 22 + 1)):
        assert _edges(**kw) == UNSUPPORTED, kw
    for kw in (dict(G=0), dict(total_edges=0), dict(G=0, offsets=None, edge_base=None, src_out=None, dst_out=None, bad=None)):
        assert _edges(**kw) == OK, kw


def test_python_surface_rejects_before_any_launch():
    from isic_hip.graph import knn_ragged_supported
    assert knn_ragged_supported(768, 16, 208) and knn_ragged_supported(32, 1, 0)
    assert not any(knn_ragged_supported(*a) for a in ((48, 8, 100), (16, 8, 100), (64, 17, 100), (64, 8, 209), (64, 0, 10)))
    from isic_hip import train as T
    with pytest.raises(ValueError, match="lesion_only"):
        T.GraphStore([], "cpu", True, lesion_knn=8)
