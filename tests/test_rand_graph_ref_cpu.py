"""tests/rand_graph_ref.py -- the restatement the device build of the random patch graphs is held to -- against its three
witnesses on the CPU: numpy's MT19937 for the written-out generator, the reference's own arrays in
tests/golden/graphs.npz, and ``build_graphs._random_edge_index`` (torch's CPU stream) over the case list the GPU test
reuses.  Equality everywhere; and each deliberately wrong variant kept in the restatement changes an integer somewhere.

Sizes 80 and 91: a node consumes n - 2 = 78 resp. 89 words, and 8 * 78 = 624, 7 * 89 = 623 -- node 8 of the first starts
exactly on a state-block boundary, node 7 of the second has its first used word as the last of block 0 and its second as
the first of block 1.  r = n - 1 at n = 64 and n = 196 uses every word across all block boundaries."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rand_graph_ref as R  # noqa: E402
from helpers import load_golden  # noqa: E402


@pytest.mark.parametrize("seed", [0, 5, 42, 2 ** 32 - 1])
def test_written_out_generator_equals_numpy_mt19937(seed):
    want = np.random.RandomState(seed)._bit_generator.random_raw(2000).astype(np.uint32)
    assert np.array_equal(R.mt_words(seed, 2000), want)
    assert np.array_equal(R.mt_words(seed, 700), want[:700])            # the cached stream is a prefix of itself


def test_restatement_equals_the_goldens():
    g = load_golden("graphs.npz")
    assert sorted(k for k in g.files if k.startswith("random.")) == sorted(name for name, *_ in R.GOLDEN)
    for name, n, r, seed in R.GOLDEN:
        got = R.random_edge_index(n, r, seed)
        assert got.dtype == g[name].dtype and np.array_equal(got, g[name]), name


@pytest.mark.parametrize("n", R.SIZES)
def test_restatement_equals_the_host_builder(n):
    import build_graphs as bg
    cases = [c for c in R.CASES if c[0] == n]
    assert len(cases) == len(R.r_list(n)) * len(R.SEEDS)
    for _, r, seed in cases:
        want = bg._random_edge_index(n, r, seed).numpy()
        got = R.random_edge_index(n, r, seed)
        assert got.dtype == want.dtype and np.array_equal(got, want), (n, r, seed)


def test_case_list_covers_the_block_boundaries():
    assert [R.clamp_r(n, r) for n in (2, 7) for r in R.r_list(n)] == [1, 1, 3, 6]
    assert R.r_list(196) == [1, 3, 16, 201] and R.r_list(3) == [1, 8] and R.r_list(17) == [1, 3, 22]
    assert 8 * (80 - 2) == R.N_STATE and 7 * (91 - 2) == R.N_STATE - 1
    assert all(R.clamp_r(n, R.r_list(n)[-1]) == n - 1 for n in R.SIZES)                # r = n - 1 at every size
    assert R.random_edge_index(1, 4, 0).shape == (2, 0) and R.random_edge_index(0, 4, 0).shape == (2, 0)


@pytest.mark.parametrize("n,seed", [(17, 42), (196, 2 ** 32 + 42), (256, 0)])
def test_targets_of_a_smaller_r_are_a_prefix(n, seed):
    t16 = R.targets(n, 16, seed)
    assert t16.shape == (n, 16)
    assert np.array_equal(R.targets(n, 3, seed), t16[:, :3])
    assert np.array_equal(R.targets(n, 16, seed), R.targets(n, n - 1, seed)[:, :16])


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_each_wrong_variant_changes_an_integer(variant):
    changed = []
    for n, r, seed in R.CASES:
        if n > 91:                                                      # (the small sizes are enough, and quick)
            continue
        a, b = R.random_edge_index(n, r, seed), R.random_edge_index(n, r, seed, variant)
        if a.shape != b.shape or not np.array_equal(a, b):
            changed.append((n, r, seed))
    assert changed, variant
    if variant == "fold_seed":                                          # only a seed with a high half can tell
        assert all(s >= 2 ** 32 for _, _, s in changed)


def test_generator_variants_change_the_stream():
    base = R.mt_words(42, 1300)
    assert not np.array_equal(R.mt_words(42, 1300, old_state0=True), base)
    assert np.array_equal(R.mt_words(42, 623, old_state0=True), base[:623])     # the last word of a block is the first to differ
    assert not np.array_equal(R.mt_words(42, 1300, temper_drop=True), base)


def test_entry_point_is_declared_and_exported():
    from isic_hip import lib
    L = lib.lib()
    inc = os.path.dirname(lib.header_path())
    assert '#include "isic_hip_randgraph.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    assert os.path.join(inc, "isic_hip_randgraph.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    assert "isic_random_graph_i64" in L.extension and "isic_random_graph_i64" in L.fn
    text = open(os.path.join(inc, "isic_hip_randgraph.h")).read()
    assert "#define ISIC_RANDGRAPH_MAX_NODES 256\n" in text and "#define ISIC_RANDGRAPH_MAX_R_VALUES 16\n" in text
    assert "03_build_graphs.py:57-78" in text


def test_argument_checks_without_a_device():
    """the codes that are decided before any device work (the rest, and that outputs stay untouched: the GPU test)"""
    import ctypes
    from isic_hip import lib
    f = lib.lib().fn["isic_random_graph_i64"]
    P = 1 << 20                                                         # a plausible aligned address that is never read
    rs = (ctypes.c_int * 17)(*range(1, 18))
    ra = ctypes.addressof(rs)
    BAD_ARG, UNSUPPORTED = -1, -2
    assert f(P, 4, 257, ra, 2, P, P, None) == UNSUPPORTED
    assert f(P, 4, 196, ra, 17, P, P, None) == UNSUPPORTED
    assert f(P, 4, 196, ra, 0, P, P, None) == UNSUPPORTED
    assert f(P, -1, 196, ra, 2, P, P, None) == BAD_ARG
    assert f(P, 4, -1, ra, 2, P, P, None) == BAD_ARG
    assert f(P, 4, 196, None, 2, P, P, None) == BAD_ARG
    assert f(None, 4, 196, ra, 2, P, P, None) == BAD_ARG
    assert f(P, 4, 196, ra, 2, None, P, None) == BAD_ARG
    assert f(P, 4, 196, ra, 2, P, None, None) == BAD_ARG
    assert f(P + 4, 4, 196, ra, 2, P, P, None) == BAD_ARG
    assert f(P, 4, 196, ra, 2, P + 4, P, None) == BAD_ARG
    assert f(P, 4, 196, ra, 2, P, P + 2, None) == BAD_ARG
    assert f(P, 0, 196, ra, 2, P, P, None) == 0 and f(None, 0, 196, ra, 16, None, None, None) == 0      # no graphs: nothing launched


def test_edges_layout_of_the_python_binding():
    from isic_hip.graph import random_graph_layout
    blocks, total = random_graph_layout(5, 196, [16, 1, 400])
    assert blocks == [(0, 2 * 196 * 16), (5 * 2 * 2 * 196 * 16, 2 * 196), (5 * 2 * 2 * 196 * 17, 196 * 195)]
    assert total == 5 * 2 * (2 * 196 * 17 + 196 * 195)
    assert random_graph_layout(3, 1, [4]) == ([(0, 0)], 0)
