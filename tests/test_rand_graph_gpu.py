"""``isic_random_graph_i64`` (csrc/rand_graph.hip) through the C ABI, and the ``device_random`` switch above it, on the
MI355X: every integer the device writes equals the restatement of tests/rand_graph_ref.py, which
tests/test_rand_graph_ref_cpu.py holds to torch's CPU stream, to numpy's MT19937 and to the reference's own arrays (and
shows that each wrong variant kept there changes such an integer).  Equality, never a tolerance.

The outputs of the C entry are prefilled with a sentinel and sit between guard areas: entries at or beyond a graph's edge
count, and both guards, must still hold the sentinel afterwards."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rand_graph_ref as R  # noqa: E402
from helpers import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = -7777
BAD_ARG, UNSUPPORTED = -1, -2
SEEDS5 = [0, 42, 2 ** 32 + 42, 2 ** 63 - 1, 42]                  # a repeat, and seeds with a high half
DEFAULT_R = list(range(1, 9)) + [12, 16]


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further GPU work: {e}", returncode=3)


def layout(G, n, rs):
    """-> [(first element, cap)] per r in the caller's order, total elements (include/isic_hip_randgraph.h)"""
    blocks, at = [], 0
    for r in rs:
        rc = R.clamp_r(n, r)
        cap = min(2 * n * rc, n * (n - 1))
        blocks.append((at, cap))
        at += 2 * G * cap
    return blocks, at


class Out:
    """guard | edges | guard  and  guard | counts | guard, sentinel everywhere"""

    def __init__(self, G, n, rs):
        self.G, self.n, self.rs = G, n, list(rs)
        self.blocks, self.total = layout(G, n, rs) if n >= 2 else ([(0, 0)] * len(rs), 0)
        self.edges = torch.full((self.total + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.int64)
        self.counts = torch.full((max(len(rs), 1) * G + 2 * GUARD,), SENTINEL, device=DEV, dtype=torch.int32)

    @property
    def edges_ptr(self):
        return self.edges.data_ptr() + 8 * GUARD

    @property
    def counts_ptr(self):
        return self.counts.data_ptr() + 4 * GUARD

    def read(self):
        """-> (edges [total], counts [n_r, G]) on the host, after checking the guards"""
        e, c = self.edges.cpu().numpy(), self.counts.cpu().numpy()
        k = len(self.rs) * self.G
        assert (e[:GUARD] == SENTINEL).all() and (e[GUARD + self.total:] == SENTINEL).all(), "edge guard overwritten"
        assert (c[:GUARD] == SENTINEL).all() and (c[GUARD + k:] == SENTINEL).all(), "count guard overwritten"
        return e[GUARD:GUARD + self.total], c[GUARD:GUARD + k].reshape(len(self.rs), self.G)

    def untouched(self):
        return bool((self.edges == SENTINEL).all()) and bool((self.counts == SENTINEL).all())


def entry(seeds, n, rs, out=None, G=None, n_r=None, seeds_ptr="own", edges_ptr="own", counts_ptr="own", r_ptr="own"):
    """one call of the C entry -> (return code, Out); every pointer can be replaced (None -> NULL)"""
    from isic_hip.lib import IsicHipError, call
    G = len(seeds) if G is None else G
    out = out or Out(max(G, 0), n, rs)
    sd = torch.tensor([s if s < 2 ** 63 else s - 2 ** 64 for s in seeds] or [0], dtype=torch.int64).to(DEV)
    ra = (ctypes.c_int * max(len(rs), 1))(*[int(r) for r in rs])
    args = [sd.data_ptr() if seeds_ptr == "own" else seeds_ptr, G, n, ctypes.addressof(ra) if r_ptr == "own" else r_ptr,
            len(rs) if n_r is None else n_r, out.edges_ptr if edges_ptr == "own" else edges_ptr,
            out.counts_ptr if counts_ptr == "own" else counts_ptr]
    try:
        call("isic_random_graph_i64", *args)
    except IsicHipError as e:
        return e.code, out
    torch.cuda.synchronize()
    return 0, out


def check(out, seeds):
    """counts and the first counts columns equal the restatement; everything beyond them still holds the sentinel"""
    edges, counts = out.read()
    G, n = out.G, out.n
    for j, (r, (at, cap)) in enumerate(zip(out.rs, out.blocks)):
        block = edges[at:at + 2 * G * cap].reshape(G, 2, cap)
        for g, seed in enumerate(seeds):
            want = R.graph(n, r, seed)
            e = int(counts[j, g])
            assert e == want.shape[1], ("count", n, r, seed, e, want.shape[1])
            assert np.array_equal(block[g, :, :e], want), ("edges", n, r, seed)
            assert (block[g, :, e:] == SENTINEL).all(), ("beyond the count", n, r, seed)


@pytest.mark.parametrize("n", R.SIZES)
def test_edges_equal_the_restatement_over_the_case_list(n):
    rs = R.r_list(n)[::-1]                          # the full r list of the size in one call, DEscending: the entry orders it
    assert {(n, r, s) for r in rs for s in SEEDS5} == {c for c in R.CASES if c[0] == n}
    rc, out = entry(SEEDS5, n, rs)
    assert rc == 0
    check(out, SEEDS5)


def test_goldens_are_reproduced_from_the_device():
    g = load_golden("graphs.npz")
    big = [c for c in R.GOLDEN if c[1] == 196]
    seeds, rs = [c[3] for c in big], [c[2] for c in big]
    rc, out = entry(seeds, 196, rs)
    assert rc == 0
    edges, counts = out.read()
    for j, (name, n, r, seed) in enumerate(big):
        at, cap = out.blocks[j]
        e = int(counts[j, j])
        assert np.array_equal(edges[at:at + 2 * 3 * cap].reshape(3, 2, cap)[j, :, :e], g[name]), name
    name, n, r, seed = [c for c in R.GOLDEN if c[1] != 196][0]
    rc, out = entry([seed], n, [r])
    edges, counts = out.read()
    assert rc == 0 and np.array_equal(edges.reshape(1, 2, -1)[0, :, :int(counts[0, 0])], g[name]), name


@pytest.mark.parametrize("G", [1, 3, 257])
def test_batch_sizes_with_the_default_r_values(G):
    seeds = [20_000 + (g % 7) for g in range(G)]                 # (seven distinct streams: the restatement is cached)
    rc, out = entry(seeds, 196, DEFAULT_R)
    assert rc == 0
    check(out, seeds)


def test_a_second_call_gives_identical_bits():
    rs = [16, 1, 3, 3, 200]                                      # unordered, a repeat, one to clamp
    rc, a = entry(SEEDS5, 91, rs)
    rc2, b = entry(SEEDS5, 91, rs)
    assert rc == 0 and rc2 == 0
    assert torch.equal(a.edges, b.edges) and torch.equal(a.counts, b.counts)
    check(a, SEEDS5)
    rc, c = entry(SEEDS5, 91, rs, out=a)                         # and onto its own output
    assert rc == 0 and torch.equal(a.edges, b.edges) and torch.equal(a.counts, b.counts)


def test_argument_errors_leave_the_outputs_untouched():
    seeds, rs = [1, 2, 3], [1, 4]
    for n in (0, 1):                                             # fewer than two nodes: no edges, every count 0
        rc, out = entry(seeds, n, rs)
        edges, counts = out.read()
        assert rc == 0 and (counts == 0).all() and bool((out.edges == SENTINEL).all())
    for kw, code in ((dict(n=257), UNSUPPORTED), (dict(n_r=17), UNSUPPORTED), (dict(n_r=0), UNSUPPORTED),
                     (dict(n_r=-1), UNSUPPORTED), (dict(G=-1), BAD_ARG), (dict(n=-1), BAD_ARG),
                     (dict(seeds_ptr=None), BAD_ARG), (dict(edges_ptr=None), BAD_ARG), (dict(counts_ptr=None), BAD_ARG),
                     (dict(r_ptr=None), BAD_ARG)):
        n = kw.pop("n", 17)
        out = Out(3, 17, rs)
        rc, out = entry(seeds, n, rs if kw.get("n_r", 0) != 17 else list(range(1, 18)), out=out, **kw)
        assert rc == code, (kw, n, rc)
        assert out.untouched(), (kw, n)
    out = Out(3, 17, rs)
    for kw in (dict(edges_ptr=out.edges_ptr + 4), dict(counts_ptr=out.counts_ptr + 2), dict(seeds_ptr=out.edges_ptr + 4)):
        rc, _ = entry(seeds, 17, rs, out=out, **kw)
        assert rc == BAD_ARG and out.untouched(), kw
    rc, _ = entry(seeds, 17, rs, out=out, G=0)                   # no graphs: nothing is launched
    assert rc == 0 and out.untouched()
    rc, _ = entry(seeds, 17, rs, out=out, G=0, seeds_ptr=None, edges_ptr=None, counts_ptr=None)
    assert rc == 0 and out.untouched()
    rc, _ = entry(seeds, 17, rs, out=out)                        # and the same buffers do take a valid call
    assert rc == 0
    check(out, seeds)


# ----------------------------------------------------------------------------- the switch above the entry
def same_container(got, want):
    """values, dtype, device and container type (a stacked tensor or a list of tensors)"""
    assert type(got) is type(want), (type(got), type(want))
    if isinstance(want, torch.Tensor):
        got, want = [got], [want]
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.device == b.device and a.shape == b.shape and torch.equal(a, b)


def teacher_outputs(G, N, D=32, C=7, seed=3):
    from pipeline import DeviceTeacherOutputs
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(G, N, D, generator=gen).to(DEV)
    pp = torch.softmax(torch.randn(G, N, C, generator=gen), dim=2).to(DEV)
    return DeviceTeacherOutputs(x, pp, torch.rand(G, N, generator=gen).to(DEV), (torch.arange(G) % C).to(DEV),
                                [f"img{i}" for i in range(G)])


@pytest.mark.parametrize("N,variant,stacked", [(196, "random4", False), (9, "random16", True)])
def test_edge_index_and_graph_records_match_the_host_build(N, variant, stacked):
    outs = teacher_outputs(6, N)
    want = outs.edge_index(variant, fold=1, seed=42)
    assert isinstance(want, torch.Tensor) == stacked              # the ragged list and the stacked tensor are both covered
    same_container(outs.edge_index(variant, fold=1, seed=42, device_random=True), want)
    same_container(outs.edge_index(variant, fold=1, seed=42, device_random=False), want)
    recs, base = outs.graph_records(variant, fold=1, seed=42, device_random=True), outs.graph_records(variant, fold=1, seed=42)
    assert len(recs) == len(base) == 6
    for a, b in zip(recs, base):
        assert a.keys() == b.keys() and a["y"] == b["y"] and a["image_id"] == b["image_id"] and a["x"] is not None
        assert torch.equal(a["x"], b["x"])
        same_container(a["edge_index"], b["edge_index"])


def test_outputs_object_carries_the_switch():
    outs = teacher_outputs(3, 9)
    want = outs.edge_index("random2", fold=2, seed=7)
    outs.device_random = True                                     # what collect_teacher_outputs_device(device_random=True) sets
    same_container(outs.edge_index("random2", fold=2, seed=7), want)
    same_container(outs.edge_index("knn3"), teacher_outputs(3, 9).edge_index("knn3"))


def frames_equal(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for (_, ra), (_, rb) in zip(a.iterrows(), b.iterrows()):
        for col in a.columns:
            va, vb = ra[col], rb[col]
            if isinstance(vb, dict):
                assert list(va.keys()) == list(vb.keys()), col
                for k in vb:
                    assert isinstance(va[k], np.ndarray) and va[k].dtype == vb[k].dtype and np.array_equal(va[k], vb[k]), (col, k)
            elif isinstance(vb, np.ndarray):
                assert va.dtype == vb.dtype and np.array_equal(va, vb), col
            else:
                assert va == vb, col


def test_graph_frame_matches_the_host_build():
    outs = teacher_outputs(6, 196)
    kw = dict(k_values=(1, 4), r_values=(1, 2, 16), seed=42, row_offset=5)
    frames_equal(outs.graph_frame("m", 2, "val", device_random=True, **kw), outs.graph_frame("m", 2, "val", **kw))


def test_build_graph_records_match_the_host_build():
    import pandas as pd
    import build_graphs as bg
    rng = np.random.default_rng(8)
    frame = pd.DataFrame({"image_id": [f"img{i}" for i in range(8)],
                          "patch_embeddings": [rng.standard_normal((196, 8)).astype(np.float32) for _ in range(8)]},
                         index=[3, 4, 5, 6, 10, 11, 12, 40])     # (the seed of a row follows its index label)
    args = (frame, "m", 1, "train", [2, 8], list(bg.DEFAULT_R_VALUES), 42)
    frames_equal(pd.DataFrame(bg.build_graph_records(*args, device_random=True)), pd.DataFrame(bg.build_graph_records(*args)))
    by_name = bg.random_edge_index_batched(196, [4, 400], [42, 43], device=DEV)
    assert sorted(by_name) == [4, 400] and all(isinstance(v, list) and len(v) == 2 for v in by_name.values())
    assert all(e.is_cuda and e.dtype == torch.int64 for v in by_name.values() for e in v)
    assert np.array_equal(by_name[4][1].cpu().numpy(), R.graph(196, 4, 43))
