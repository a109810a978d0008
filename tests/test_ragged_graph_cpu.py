"""CPU-only checks of the ragged patch graphs (include/isic_hip_ragged.h, tests/ragged_graph_ref.py): the numpy restatement
of the induced subgraph against a per-edge loop, the three entry points declared, exported and known to the header parser,
and their argument checks -- BAD_ARG, UNSUPPORTED and the no-op cases -- which all answer before any device work."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ragged_graph_ref as R  # noqa: E402
from isic_hip import lib  # noqa: E402

NAMES = ("isic_induced_subgraph_count", "isic_induced_subgraph_write", "isic_csr_batch_assemble_ragged")
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call
BIG = 2 ** 31


# ------------------------------------------------------------------ the restatement against a per-edge loop
def _brute(src, dst, keep, weight=None):
    n = len(keep)
    kept = [bool(k) for k in keep]
    if not any(kept):
        kept = [True] * n
    new, rows = {}, []
    for i in range(n):
        if kept[i]:
            new[i] = len(rows)
            rows.append(i)
    s2, d2, w2 = [], [], []
    for e, (s, d) in enumerate(zip(src, dst)):
        if kept[s] and kept[d]:
            s2.append(new[s]); d2.append(new[d])
            if weight is not None:
                w2.append(weight[e])
    return s2, d2, rows, w2


@pytest.mark.parametrize("n, E, pattern", [(1, 3, "all"), (2, 5, "none"), (37, 300, "random"), (37, 300, "one"),
                                           (64, 0, "random"), (50, 257, "alternate")])
def test_restatement_equals_a_per_edge_loop(n, E, pattern):
    rng = np.random.default_rng(n * 1000 + E)
    src, dst = rng.integers(0, n, E), rng.integers(0, n, E)
    if E > 4:
        src[1], dst[1] = src[0], dst[0]                                  # a duplicated edge
        dst[2] = src[2]                                                  # a self loop
    keep = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "random": rng.random(n) < 0.5,
            "one": np.arange(n) == n // 2, "alternate": np.arange(n) % 2 == 0}[pattern]
    w = rng.random(E).astype(np.float32)
    s2, d2, rows, w2 = R.induced_subgraph(src, dst, keep, w)
    bs, bd, brows, bw = _brute(src.tolist(), dst.tolist(), keep.tolist(), w.tolist())
    assert s2.tolist() == bs and d2.tolist() == bd and rows.tolist() == brows
    assert w2.tolist() == [np.float32(v) for v in bw]
    if pattern in ("all", "none"):                                       # no flag set keeps everything, like every flag set
        assert s2.tolist() == src.tolist() and rows.tolist() == list(range(n))


def test_restatement_over_a_record_set_concatenates_the_graphs():
    rng = np.random.default_rng(7)
    ns, es = [3, 1, 40, 0, 17], [10, 2, 257, 0, 60]
    noff, eoff = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(es)])
    src = np.concatenate([rng.integers(0, max(n, 1), e) for n, e in zip(ns, es)])
    dst = np.concatenate([rng.integers(0, max(n, 1), e) for n, e in zip(ns, es)])
    keep = rng.random(noff[-1]) < 0.6
    ei, eo, no, rows = R.induced_subgraphs(src, dst, eoff, noff, keep)
    assert eo[0] == 0 and no[0] == 0 and ei.shape == (2, eo[-1]) and rows.shape == (no[-1],)
    for g in range(len(ns)):
        s2, d2, r2 = R.induced_subgraph(src[eoff[g]:eoff[g + 1]], dst[eoff[g]:eoff[g + 1]], keep[noff[g]:noff[g + 1]])
        assert ei[0, eo[g]:eo[g + 1]].tolist() == s2.tolist() and ei[1, eo[g]:eo[g + 1]].tolist() == d2.tolist()
        assert rows[no[g]:no[g + 1]].tolist() == r2.tolist()


# ------------------------------------------------------------------ the ABI without a device
def test_ragged_entry_points_are_declared_exported_and_parsed():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_ragged.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(inc, "isic_hip_ragged.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    assert os.path.join(inc, "isic_hip_ragged.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    protos = lib.parse_header(os.path.join(inc, "isic_hip_ragged.h"))
    assert set(protos) == set(NAMES)
    assert [len(protos[n][1]) for n in NAMES] == [13, 18, 25]
    for n in NAMES:
        assert protos[n][0] is ctypes.c_int and protos[n][1][-1][1] == "stream", n
    count = {a[1]: a for a in protos[NAMES[0]][1]}
    assert count["keep"][2] and count["bad"][2] and count["T"][0] is ctypes.c_int64 and count["G"][0] is ctypes.c_int
    asm = {a[1]: a for a in protos[NAMES[2]][1]}
    assert asm["total_nnz"][0] is ctypes.c_int64 and asm["row_index_out"][2] and asm["sel"][2]
    L = lib.lib()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name not in L.public and name in L.fn and hasattr(cdll, name), name


def _count(G=3, T=10, E=20, **kw):
    a = dict(node_offsets=P, edge_offsets=P, src=P, dst=P, keep=P, new_id=P, kept_nodes=P, kept_edges=P, bad=P)
    a.update(kw)
    return lib.lib().fn[NAMES[0]](a["node_offsets"], a["edge_offsets"], a["src"], a["dst"], a["keep"], G, T, E, a["new_id"],
                                  a["kept_nodes"], a["kept_edges"], a["bad"], None)


def _write(G=3, T=10, E=20, T_out=5, E_out=7, **kw):
    a = dict(node_offsets=P, edge_offsets=P, src=P, dst=P, edge_weight=None, new_id=P, node_out_offsets=P, edge_out_offsets=P,
             src_out=P, dst_out=P, edge_weight_out=None, rows_out=P)
    a.update(kw)
    return lib.lib().fn[NAMES[1]](a["node_offsets"], a["edge_offsets"], a["src"], a["dst"], a["edge_weight"], a["new_id"], G, T, E,
                                  a["node_out_offsets"], a["edge_out_offsets"], T_out, E_out, a["src_out"], a["dst_out"],
                                  a["edge_weight_out"], a["rows_out"], None)


_ASM_PTRS = ("sel", "node_base", "nnz_base", "store_node_off", "store_nnz_off", "rowptr", "rowptr_t", "col", "col_t", "val",
             "val_t", "perm_t", "rowptr_out", "rowptr_t_out", "col_out", "col_t_out", "val_out", "val_t_out", "perm_t_out",
             "row_index_out")


def _assemble(B=2, G=4, total_nodes=10, total_nnz=30, **kw):
    a = {k: P for k in _ASM_PTRS}
    a.update(kw)
    return lib.lib().fn[NAMES[2]](a["sel"], a["node_base"], a["nnz_base"], B, G, total_nodes, total_nnz, a["store_node_off"],
                                  a["store_nnz_off"], *[a[k] for k in _ASM_PTRS[5:]], None)


def test_induced_count_argument_checks_without_a_device():
    for kw in (dict(G=-1), dict(T=-1), dict(E=-1)):
        assert _count(**kw) == BAD_ARG, kw
    for k in ("node_offsets", "edge_offsets", "src", "dst", "keep", "new_id", "kept_nodes", "kept_edges", "bad"):
        assert _count(**{k: None}) == BAD_ARG, k
    assert _count(T=BIG) == UNSUPPORTED and _count(E=BIG) == UNSUPPORTED
    assert _count(T=-1, E=BIG) == BAD_ARG                                # a bad argument is reported before an unsupported size
    nothing = dict(node_offsets=None, edge_offsets=None, src=None, dst=None, keep=None, new_id=None, kept_nodes=None,
                   kept_edges=None, bad=None)
    assert _count(G=0, **nothing) == OK and _count(G=0, T=BIG, E=BIG, **nothing) == OK      # no graphs: nothing touched


def test_induced_write_argument_checks_without_a_device():
    for kw in (dict(G=-1), dict(T=-1), dict(E=-1), dict(T_out=-1), dict(E_out=-1)):
        assert _write(**kw) == BAD_ARG, kw
    for k in ("node_offsets", "edge_offsets", "src", "dst", "new_id", "node_out_offsets", "edge_out_offsets", "src_out",
              "dst_out", "rows_out"):
        assert _write(**{k: None}) == BAD_ARG, k
    assert _write(edge_weight=P) == BAD_ARG and _write(edge_weight_out=P) == BAD_ARG        # the weights: both or neither
    for kw in (dict(T=BIG), dict(E=BIG), dict(T_out=BIG), dict(E_out=BIG)):
        assert _write(**kw) == UNSUPPORTED, kw
    nothing = {k: None for k in ("node_offsets", "edge_offsets", "src", "dst", "new_id", "node_out_offsets", "edge_out_offsets",
                                 "src_out", "dst_out", "rows_out")}
    assert _write(G=0, **nothing) == OK


def test_ragged_assemble_argument_checks_without_a_device():
    for kw in (dict(B=-1), dict(G=-1), dict(total_nodes=-1), dict(total_nnz=-1), dict(G=0)):
        assert _assemble(**kw) == BAD_ARG, kw
    for k in _ASM_PTRS[:-1]:
        assert _assemble(**{k: None}) == BAD_ARG, k
    for kw in (dict(total_nodes=BIG - 1), dict(total_nnz=BIG - 1), dict(total_nodes=BIG), dict(total_nnz=2 ** 40)):
        assert _assemble(**kw) == UNSUPPORTED, kw
    assert _assemble(B=0, G=0, **{k: None for k in _ASM_PTRS}) == OK     # an empty batch: nothing touched
    assert _assemble(B=0, total_nodes=BIG, total_nnz=BIG, **{k: None for k in _ASM_PTRS}) == OK
