"""CPU-only checks of the random patch graphs over graphs of unequal size (include/isic_hip_randgraph_ragged.h,
tests/rand_graph_ragged_ref.py): the restatement against the reference-generated golden graphs at lesion-size node counts and
against ``build_graphs._random_edge_index`` per graph, the two entry points declared, exported and known to the header
parser, their argument checks (which answer before any device work), the analytic edge bound, and the Python surface's
rejections and seeds."""
import ctypes
import os
import pickle
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rand_graph_ragged_ref as RGR  # noqa: E402
import rand_graph_ref as RR  # noqa: E402
from helpers import load_golden  # noqa: E402
from isic_hip import lib  # noqa: E402

NAMES = ("isic_random_graph_ragged_count", "isic_random_graph_ragged_write")
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
P = 0x10000                                         # a non-NULL, 8-byte aligned pointer value: never dereferenced, because every
#                                                     call below is either rejected or has G == 0 (nothing is launched)


def test_restatement_equals_the_reference_generated_golden_graphs():
    g = load_golden("random_ragged.npz")
    assert sorted(g.files) == sorted(RGR.golden_key(*c) for c in RGR.GOLDEN_CASES) and len(g.files) == 36
    for n, r, s in RGR.GOLDEN_CASES:
        want = g[RGR.golden_key(n, r, s)]
        assert want.dtype == np.int16
        assert np.array_equal(RR.random_edge_index(n, r, s), want.astype(np.int64)), (n, r, s)
    # as a batch: own n, own clamp, own seed, flat layout and offsets
    sizes = [c[0] for c in RGR.GOLDEN_CASES if c[1] == 16]
    seeds = [c[2] for c in RGR.GOLDEN_CASES if c[1] == 16]
    for global_ids in (False, True):
        ei, eo = RGR.random_graphs_ragged(seeds, sizes, (16,), global_ids)[16]
        first = np.concatenate([[0], np.cumsum(sizes)])
        for i, (n, s) in enumerate(zip(sizes, seeds)):
            want = g[RGR.golden_key(n, 16, s)].astype(np.int64) + (first[i] if global_ids else 0)
            assert np.array_equal(ei[:, eo[i]:eo[i + 1]], want), (n, s, global_ids)
        assert eo[-1] == ei.shape[1]
    assert g[RGR.golden_key(5, 16, 42)].shape == (2, 20) and g[RGR.golden_key(2, 4, 42)].tolist() == [[0, 1], [1, 0]]


def test_restatement_equals_the_host_builder_per_graph():
    import build_graphs as bg
    sizes = [0, 1, 2, 3, 4, 5, 17, 26, 27, 33, 64, 65, 129]
    seeds = [42 if i % 2 else 2 ** 32 + 7 for i in range(len(sizes))]
    rs = (1, 4, 16, 300)
    got = RGR.random_graphs_ragged(seeds, sizes, rs)
    for r in rs:
        ei, eo = got[r]
        assert eo[0] == 0 and eo[-1] == ei.shape[1]
        for i, (n, s) in enumerate(zip(sizes, seeds)):
            want = bg._random_edge_index(n, r=r, seed=s).numpy()
            assert np.array_equal(ei[:, eo[i]:eo[i + 1]], want), (n, r, s)
    assert got[300][1][3] - got[300][1][2] == 2 and got[16][1][6] - got[16][1][5] == 20      # the per-graph clamp: n = 2, n = 5


def test_entry_points_are_declared_exported_and_parsed():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_randgraph_ragged.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(inc, "isic_hip_randgraph_ragged.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    assert os.path.join(inc, "isic_hip_randgraph_ragged.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    protos = lib.parse_header(os.path.join(inc, "isic_hip_randgraph_ragged.h"))
    assert set(protos) == set(NAMES) and [len(protos[n][1]) for n in NAMES] == [9, 13]
    for n in NAMES:
        assert protos[n][0] is ctypes.c_int and protos[n][1][-1][1] == "stream", n
        assert [a[1] for a in protos[n][1][:6]] == ["seeds", "node_offsets", "G", "max_nodes", "r_values", "n_r"]
    wr = {a[1]: a for a in protos[NAMES[1]][1]}
    assert wr["total"][0] is ctypes.c_int64 and wr["global_ids"][0] is ctypes.c_int and wr["edge_off"][2] and wr["bad"][2]
    L = lib.lib()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name not in L.public and name in L.fn and hasattr(cdll, name), name
    from isic_hip import graph
    assert (graph.RANDOM_RAGGED_MAX_NODES, graph.RANDOM_RAGGED_MAX_R_VALUES, graph.RANDOM_RAGGED_PACK_NODES) == tuple(
        int(re.search(rf"#define {m} (\d+)", open(os.path.join(inc, "isic_hip_randgraph_ragged.h")).read()).group(1))
        for m in ("ISIC_RANDGRAPH_RAGGED_MAX_NODES", "ISIC_RANDGRAPH_RAGGED_MAX_R_VALUES", "ISIC_RANDGRAPH_RAGGED_PACK_NODES"))


def _call(which, G=3, max_nodes=100, rs=(1, 4), n_r=None, total=50, **kw):
    a = dict(seeds=P, node_offsets=P, counts=P, bad=P, edge_off=P, src=P, dst=P)
    a.update(kw)
    rv = (ctypes.c_int * max(len(rs), 1))(*rs)
    rptr = kw.get("r_values", ctypes.addressof(rv))
    n_r = len(rs) if n_r is None else n_r
    f = lib.lib().fn[NAMES[which]]
    if which == 0:
        return f(a["seeds"], a["node_offsets"], G, max_nodes, rptr, n_r, a["counts"], a["bad"], None)
    return f(a["seeds"], a["node_offsets"], G, max_nodes, rptr, n_r, a["edge_off"], total, 0, a["src"], a["dst"], a["bad"], None)


@pytest.mark.parametrize("which", [0, 1], ids=["count", "write"])
def test_argument_checks_answer_without_a_device(which):
    own = ("counts",) if which == 0 else ("edge_off", "src", "dst")
    for name in ("seeds", "node_offsets", "bad", "r_values") + own:
        assert _call(which, **{name: None}) == BAD_ARG, name
    for kw in (dict(G=-1), dict(max_nodes=-1)) + ((dict(total=-1),) if which else ()):
        assert _call(which, **kw) == BAD_ARG, kw
    for name in ("seeds", "node_offsets") + own:                                     # int64 arrays: 8-byte aligned
        assert _call(which, **{name: P + 4}) == BAD_ARG, name
    assert _call(which, bad=P + 2) == BAD_ARG                                        # uint32: 4-byte aligned
    for kw in (dict(n_r=0), dict(rs=tuple(range(1, 18))), dict(max_nodes=257)):
        assert _call(which, **kw) == UNSUPPORTED, kw
    for kw in (dict(G=0), dict(G=0, seeds=None, node_offsets=None, counts=None, bad=None, edge_off=None, src=None, dst=None),
               dict(G=0, max_nodes=256, rs=tuple(range(1, 17)))):
        assert _call(which, **kw) == OK, kw                                          # nothing is launched
    assert _call(which, G=0, r_values=None) == BAD_ARG and _call(which, G=0, n_r=17) == UNSUPPORTED


def test_random_edge_caps_match_a_brute_force_evaluation():
    from isic_hip.graph import random_edge_caps
    sizes = [0, 1, 2, 3, 4, 5, 17, 30, 64, 65, 196, 256]
    rs = (1, 2, 4, 8, 12, 16, 300)
    caps = random_edge_caps(sizes, rs)
    assert caps.dtype == np.int64 and caps.shape == (len(rs), len(sizes))
    assert np.array_equal(caps, RGR.random_edge_caps(sizes, rs))
    assert caps[:, :2].sum() == 0 and caps[-1].tolist() == [n * (n - 1) if n >= 2 else 0 for n in sizes]
    # it IS a bound, and tight where the clamp makes the graph complete
    for j, r in enumerate(rs):
        for i, n in enumerate(sizes[:9]):
            e = RR.graph(n, r, 42).shape[1] if n >= 2 else 0
            assert e <= caps[j][i] and (e == caps[j][i] or r < n - 1), (n, r)
    assert random_edge_caps([], rs).shape == (len(rs), 0)


def _load_script(name, alias):
    import importlib.util
    spec = importlib.util.spec_from_file_location(alias, os.path.join(ROOT, "multimodal-isic_amd", name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_python_surface_rejects_before_any_launch():
    from isic_hip import train as T
    with pytest.raises(ValueError, match="lesion_only"):
        T.GraphStore([], "cpu", True, lesion_random=4)
    with pytest.raises(ValueError, match="exclude"):
        T.GraphStore([], "cpu", True, lesion_only=True, lesion_knn=8, lesion_random=4)
    with pytest.raises(ValueError, match=">= 1"):
        T.GraphStore([], "cpu", True, lesion_only=True, lesion_random=0)
    m05 = _load_script("05_train_gnns.py", "train_gnns_05_random_cpu")
    common = ["--gnn", "gcn", "--variants", "random4"]
    with pytest.raises(SystemExit):
        m05.parse_args(common + ["--lesion-random"])                                # needs --lesion-flags
    args = m05.parse_args(common + ["--lesion-flags", "flags.pkl", "--lesion-random"])
    assert args.lesion_random and args.graph_seed == 42
    assert m05.lesion_random_r(args, "random4") == 4 and m05.lesion_random_r(args, "knn8") is None
    assert m05.lesion_random_r(args, "grid8") is None and m05.lesion_knn_k(args, "random4") is None
    assert m05.lesion_random_r(m05.parse_args(common + ["--lesion-flags", "flags.pkl"]), "random4") is None
    assert m05.parse_args(common + ["--graph-seed", "7"]).graph_seed == 7


def test_load_fold_records_attaches_the_seeds_of_03(tmp_path):
    """`03_build_graphs.py:135-136`: graph_seed = seed + fold * 10000 + row_idx, row_idx the image's index LABEL in the
    patch-statistics frame of its (fold, split) -- here a frame whose labels are neither 0..n-1 nor in the graph frame's order."""
    import pandas as pd
    m05 = _load_script("05_train_gnns.py", "train_gnns_05_random_seeds")
    fold, ids, labels = 3, ["a", "b", "c", "d"], [7, 2, 11, 5]
    gdir, sdir = tmp_path / "graph_outputs" / "m", tmp_path / "patch_stats" / "m"
    gdir.mkdir(parents=True), sdir.mkdir(parents=True)
    ei = np.asarray([[0, 1], [1, 0]], dtype=np.int64)
    rows = [{"model_name": "m", "fold": fold, "split": "val", "image_id": i, "grid4_edge_index": ei, "grid8_edge_index": ei,
             "knn_edge_indices": {}, "random_edge_indices": {4: ei}} for i in reversed(ids)]
    pickle.dump(pd.DataFrame(rows), open(gdir / "graph_dataset.pkl", "wb"))
    stats = pd.DataFrame([{"image_id": i, "label": 0, "patch_embeddings": np.zeros((3, 2), np.float32)} for i in ids], index=labels)
    pickle.dump(stats, open(sdir / f"patch_stats_fold_{fold}_val.pkl", "wb"))
    recs = m05.load_fold_records(tmp_path, "m", fold, "val", "random4")
    assert [r["image_id"] for r in recs] == list(reversed(ids))
    assert {r["image_id"]: r["graph_seed"] for r in recs} == {i: 42 + fold * 10_000 + lab for i, lab in zip(ids, labels)}
    assert all(isinstance(r["graph_seed"], int) and "keep" not in r for r in recs)
    recs = m05.load_fold_records(tmp_path, "m", fold, "val", "random4", graph_seed=1000)
    assert sorted(r["graph_seed"] for r in recs) == sorted(1000 + fold * 10_000 + lab for lab in labels)
