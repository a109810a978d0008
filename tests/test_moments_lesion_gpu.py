"""The token statistics over a subset of each image's tokens on the MI355X: ``isic_token_moments_masked_f32`` and
``isic_token_moments_ragged_f32`` through the ABI and the Python surface.

The yardstick of every row with n >= 1 kept tokens (n >= 2 when unbiased) is ``isic_token_moments_f32`` -- the dense entry,
pinned by tests/test_moments_gpu.py -- on B = 1, T = n over a contiguous copy of the kept tokens: the rows must have its BITS.
The same rows are held to the derived bounds of tests/moments_ref.py against the fp64 restatement (max and median exactly),
the masked and the ragged form must agree bit for bit, and the rows with n == 0 and unbiased n == 1 must carry NaN exactly
where include/isic_hip_moments_ragged.h says."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moments_lesion_ref as LR  # noqa: E402
import moments_ref as R  # noqa: E402
from isic_hip.lib import IsicHipError, call, lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DENSE, MASKED, RAGGED = "isic_token_moments_f32", "isic_token_moments_masked_f32", "isic_token_moments_ragged_f32"
SENTINEL = -777.25
OK, BAD_ARG, UNSUPPORTED = 0, -1, -2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def upload_rows(rows, ldx=None, misalign=False):
    """rows [R, D] fp32 numpy -> (device store, pointer, ldx): rows ``ldx`` floats apart, the padding filled with a large value
    that must not be read into any statistic; ``misalign``: the first row starts 4 bytes past a 16-byte boundary"""
    n, D = rows.shape
    ldx = ldx or D
    store = torch.full((n * ldx + 1,), 1e30, dtype=torch.float32)
    off = 1 if misalign else 0
    if n:
        store[off:off + n * ldx].view(n, ldx)[:, :D] = torch.from_numpy(np.ascontiguousarray(rows))
    store = store.to(DEV)
    assert store.data_ptr() % 16 == 0
    return store, store.data_ptr() + 4 * off, ldx


def run_dense(rows, eps=R.EPS, unbiased=False):
    """the yardstick: rows [n, D] (contiguous copy of the kept tokens) -> [6 D] from the dense entry with B = 1, T = n"""
    n, D = rows.shape
    store, ptr, ldx = upload_rows(rows)
    out = torch.full((1, 6 * D), SENTINEL, device=DEV, dtype=torch.float32)
    call(DENSE, ptr, 1, n, D, ldx, float(eps), int(unbiased), out, 6 * D)
    return out.cpu().numpy()[0]


def run_masked(x, keep, eps=R.EPS, unbiased=False, ldx=None, ldo=None, misalign=False, want_counts=True):
    """x [B, T, D] fp32 numpy, keep [B, T] -> (out [B, 6 D], the padding of out or None, counts [B] or None)"""
    B, T, D = x.shape
    ldo = ldo or 6 * D
    store, ptr, ldx = upload_rows(x.reshape(B * T, D), ldx, misalign)
    flags = torch.from_numpy(np.ascontiguousarray(keep).astype(np.uint8)).to(DEV)
    out = torch.full((B, ldo), SENTINEL, device=DEV, dtype=torch.float32)
    counts = torch.full((B,), -5, device=DEV, dtype=torch.int32) if want_counts else None
    call(MASKED, ptr, flags, B, T, D, ldx, float(eps), int(unbiased), out, ldo, counts)
    o = out.cpu().numpy()
    return o[:, :6 * D], (o[:, 6 * D:] if ldo > 6 * D else None), (counts.cpu().numpy() if want_counts else None)


def run_ragged(rows, offsets, max_nodes, eps=R.EPS, unbiased=False, ldx=None, ldo=None, misalign=False, want_counts=True,
               total=None):
    """rows [total, D], offsets int64 [G + 1] -> (out [G, 6 D], padding or None, counts [G] or None, bad)"""
    D = rows.shape[1]
    G = len(offsets) - 1
    ldo = ldo or 6 * D
    store, ptr, ldx = upload_rows(rows, ldx, misalign)
    off = torch.from_numpy(np.asarray(offsets, dtype=np.int64)).to(DEV)
    out = torch.full((G, ldo), SENTINEL, device=DEV, dtype=torch.float32)
    counts = torch.full((G,), -5, device=DEV, dtype=torch.int32) if want_counts else None
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    call(RAGGED, ptr, off, G, int(max_nodes), len(rows) if total is None else total, D, ldx, float(eps), int(unbiased), out, ldo,
         counts, bad)
    o = out.cpu().numpy()
    return o[:, :6 * D], (o[:, 6 * D:] if ldo > 6 * D else None), (counts.cpu().numpy() if want_counts else None), int(bad.item())


def check_rows(x, keep, got, counts, unbiased, tag, eps=R.EPS):
    """checks 1, 2 and 4 of one masked (or equivalent ragged) result"""
    B, T, D = x.shape
    n = keep.sum(axis=1)
    if counts is not None:
        assert counts.dtype == np.int32 and np.array_equal(counts, n), tag
    assert np.array_equal(np.isnan(got), LR.expected_nan(keep, D, unbiased)), tag        # NaN there and nowhere else
    ref, bound = LR.reference_masked(x, keep, eps, unbiased), LR.bounds_masked(x, keep, eps, unbiased)
    for b in range(B):
        if LR.defined(int(n[b]), unbiased):
            want = run_dense(np.ascontiguousarray(x[b, keep[b]]), eps, unbiased)
            assert same_bits(got[b], want), (tag, b, int(n[b]))                          # 1: the dense entry's bits
            per = R.worst_per_stat(got[b:b + 1], ref[b:b + 1], bound[b:b + 1])           # 2: the CPU restatement
            assert R.selections_equal(got[b:b + 1], ref[b:b + 1]), (tag, b)
            assert max(per.values()) <= 1.0, (tag, b, per)
        elif n[b] == 1:                                                                  # unbiased, one token: the element
            lone = x[b, keep[b]][0]
            for s in (0, 1, 3):
                assert same_bits(got[b, s * D:(s + 1) * D], lone), (tag, b, s)


def check_case(x, keep, unbiased, tag):
    """masked through the ABI, then the ragged form on the compacted rows with the induced offsets: checks 1 to 4"""
    got, _, counts = run_masked(x, keep, R.EPS, unbiased)
    check_rows(x, keep, got, counts, unbiased, tag)
    rows, offsets = LR.compact(x, keep)
    rg, _, rcounts, bad = run_ragged(rows, offsets, max(int(keep.sum(axis=1).max()), 0), R.EPS, unbiased)
    assert bad == 0 and np.array_equal(rcounts, counts), tag
    assert same_bits(rg, got), tag                                                       # 3: masked == ragged, NaN rows included
    return got


@pytest.mark.parametrize("T,D", list(itertools.product(LR.DEVICE_T, LR.DEVICE_D)))
def test_every_keep_pattern_alone_and_in_batches(T, D):
    """B = 1: every pattern alone; B = 3: the patterns three at a time and one batch that mixes them.  `unbiased` alternates."""
    x3 = R.make_input("mixed", 3, T, D)
    unbiased = (T + D) % 2 == 1
    for i, name in enumerate(LR.PATTERNS):
        keep = LR.keep_batch((name,), T, seed=i)
        check_case(x3[i % 3:i % 3 + 1], keep, unbiased, f"T {T} D {D} B 1 {name} unbiased {unbiased}")
    groups = [LR.PATTERNS[0:3], LR.PATTERNS[3:6], LR.PATTERNS[6:8] + ("bernoulli",), tuple(LR.mixed_names(3))]
    for j, names in enumerate(groups):
        keep = LR.keep_batch(names, T, seed=j)
        check_case(x3, keep, not unbiased if j % 2 else unbiased, f"T {T} D {D} B 3 {names}")


def test_width_768_once():
    x = R.make_input("mixed", 3, 196, 768)
    keep = LR.keep_batch(("bernoulli", "none", "prefix"), 196)
    check_case(x, keep, True, "T 196 D 768")


@pytest.mark.parametrize("unbiased", (False, True))
@pytest.mark.parametrize("D", (64, 65))
def test_ragged_sizes_in_one_call(D, unbiased):
    sizes = LR.RAGGED_SIZES
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = R.make_input("mixed", 1, int(offsets[-1]), D)[0]
    got, _, counts, bad = run_ragged(rows, offsets, 256, R.EPS, unbiased)
    assert bad == 0 and counts.tolist() == list(sizes)
    for g, n in enumerate(sizes):
        seg = rows[offsets[g]:offsets[g + 1]][None]                            # [1, n, D]
        check_rows(seg, np.ones((1, n), dtype=bool), got[g:g + 1], counts[g:g + 1], unbiased, f"ragged n {n} D {D}")
    # ties and a constant channel through the ragged form, still the dense entry's bits
    ties = R.make_input("ties", 1, int(offsets[-1]), D)[0]
    got, _, _, bad = run_ragged(ties, offsets, 256, R.EPS, unbiased)
    for g, n in enumerate(sizes):
        if LR.defined(n, unbiased):
            assert same_bits(got[g], run_dense(ties[offsets[g]:offsets[g + 1]], R.EPS, unbiased)), (g, n)


def test_counts_may_be_null():
    x = R.make_input("mixed", 3, 65, 7)
    keep = LR.keep_batch(LR.mixed_names(3), 65)
    with_counts, _, counts = run_masked(x, keep)
    without, _, none = run_masked(x, keep, want_counts=False)
    assert none is None and same_bits(with_counts, without) and counts.tolist() == keep.sum(axis=1).tolist()
    rows, offsets = LR.compact(x, keep)
    a, _, _, _ = run_ragged(rows, offsets, 65)
    b, _, none, bad = run_ragged(rows, offsets, 65, want_counts=False)
    assert none is None and bad == 0 and same_bits(a, b) and same_bits(a, with_counts)


def test_a_row_depends_on_nothing_but_its_own_kept_tokens():
    T, D = 196, 130
    x = R.make_input("mixed", 3, T, D, seed=3)
    keep = LR.keep_batch(("bernoulli", "alternating", "suffix"), T)
    for unbiased in (False, True):
        full, _, _ = run_masked(x, keep, R.EPS, unbiased)
        again, _, _ = run_masked(x, keep, R.EPS, unbiased)
        assert same_bits(full, again)                                           # two identical calls
        for b in range(3):                                                      # B, and the other images' flags
            alone, _, _ = run_masked(x[b:b + 1], keep[b:b + 1], R.EPS, unbiased)
            assert same_bits(alone[0], full[b]), b
            others = LR.keep_batch(("none", "all", "first"), T)
            others[b] = keep[b]
            moved, _, _ = run_masked(x, others, R.EPS, unbiased)
            assert same_bits(moved[b], full[b]), b
        # the tokens that are not kept do not matter
        y = x.copy()
        y[~keep] = 1e30
        masked_out, _, _ = run_masked(y, keep, R.EPS, unbiased)
        assert same_bits(masked_out, full)
        rows, offsets = LR.compact(x, keep)
        largest = int(keep.sum(axis=1).max())
        first, _, _, _ = run_ragged(rows, offsets, largest, R.EPS, unbiased)
        assert same_bits(first, full)
        for max_nodes in (largest + 1, 200, 256):                               # max_nodes only sizes LDS
            other, _, _, bad = run_ragged(rows, offsets, max_nodes, R.EPS, unbiased)
            assert bad == 0 and same_bits(other, first), max_nodes
        other, _, _, _ = run_ragged(rows, offsets, largest, R.EPS, unbiased)
        assert same_bits(other, first)
        for g in range(3):                                                      # a graph alone
            alone, _, _, _ = run_ragged(rows[offsets[g]:offsets[g + 1]], np.array([0, offsets[g + 1] - offsets[g]]), 256, R.EPS,
                                        unbiased)
            assert same_bits(alone[0], first[g]), g


@pytest.mark.parametrize("unbiased", (False, True))
@pytest.mark.parametrize("T,D,ldx,ldo,misalign", (
    (196, 65, 68, 6 * 65 + 5, False),       # a channel slice, 16-byte path with a partial vector at the slab tail
    (5, 7, 9, 50, False),                   # element path (ldx % 4 != 0), padded
    (196, 64, 64, 384, True),               # ldx % 4 == 0 but X not 16-byte aligned: element path
    (65, 130, 132, 6 * 130 + 3, True),
))
def test_padded_and_misaligned_layouts(T, D, ldx, ldo, misalign, unbiased):
    x = R.make_input("mixed", 3, T, D)
    keep = LR.keep_batch(("bernoulli", "none", "suffix"), T)
    plain, _, counts = run_masked(x, keep, R.EPS, unbiased)
    check_rows(x, keep, plain, counts, unbiased, f"layout T {T} D {D}")
    got, pad, _ = run_masked(x, keep, R.EPS, unbiased, ldx, ldo, misalign)
    assert same_bits(got, plain)                                                # the layout and the load path change no bit
    assert pad is None or bool((pad == SENTINEL).all())                         # the padding of out is left untouched
    rows, offsets = LR.compact(x, keep)
    rg, rpad, _, bad = run_ragged(rows, offsets, T, R.EPS, unbiased, ldx, ldo, misalign)
    assert bad == 0 and same_bits(rg, plain)
    assert rpad is None or bool((rpad == SENTINEL).all())


def test_bad_graphs_write_nothing_and_leave_their_neighbours_alone():
    D, total, max_nodes = 65, 40, 12
    rows = R.make_input("mixed", 1, total + 8, D)[0]                            # 8 rows beyond `total`: never read
    # graph g owns [offsets[g], offsets[g + 1]):
    #   (-2, 0) starts below 0 | (0, 6) good | (6, 4) decreases | (4, 10) good | (10, 25) spans 15 > max_nodes | (25, 30) good |
    #   (30, 41) ends beyond total
    offsets = np.array([-2, 0, 6, 4, 10, 25, 30, 41], dtype=np.int64)
    good, wrong = (1, 3, 5), (0, 2, 4, 6)
    got, _, counts, bad = run_ragged(rows, offsets, max_nodes, total=total)
    assert bad == len(wrong)
    assert counts.tolist() == [0, 6, 0, 6, 0, 5, 0]
    for g in wrong:
        assert (got[g] == SENTINEL).all(), g                                    # the bad rows keep their sentinel
    for g in good:
        want = run_dense(rows[offsets[g]:offsets[g + 1]])
        assert same_bits(got[g], want), g                                       # the neighbours are what they are alone
    _, _, none, bad = run_ragged(rows, offsets, max_nodes, total=total, want_counts=False)
    assert none is None and bad == len(wrong)
    from isic_hip.moments import token_moments_ragged
    xd = torch.from_numpy(rows[:total]).to(DEV)
    with pytest.raises(IsicHipError, match="4 graph"):
        token_moments_ragged(xd, torch.from_numpy(offsets).to(DEV), max_nodes=max_nodes)
    with pytest.raises(IsicHipError, match="1 graph"):                          # a span above max_nodes alone
        token_moments_ragged(xd, [0, 6, 19, 25], max_nodes=12)
    with pytest.raises(IsicHipError, match="graph"):                            # max_nodes from decreasing host offsets
        token_moments_ragged(xd, [0, 6, 4, 10])


def test_error_codes_come_without_a_launch():
    x = R.make_input("mixed", 2, 5, 7)
    store, ptr, _ = upload_rows(x.reshape(10, 7))
    keep = torch.ones((2, 5), device=DEV, dtype=torch.uint8)
    off = torch.tensor([0, 5, 10], device=DEV, dtype=torch.int64)
    out = torch.full((2, 42), SENTINEL, device=DEV, dtype=torch.float32)
    counts = torch.full((2,), -5, device=DEV, dtype=torch.int32)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    fm, fr = lib().fn[MASKED], lib().fn[RAGGED]
    st = torch.cuda.current_stream().cuda_stream
    k, o, c, f, bd = keep.data_ptr(), out.data_ptr(), counts.data_ptr(), off.data_ptr(), bad.data_ptr()
    big = torch.zeros((2, 257), device=DEV, dtype=torch.uint8)
    assert fm(ptr, big.data_ptr(), 2, 257, 7, 7, 1e-6, 0, o, 42, c, st) == UNSUPPORTED
    assert fr(ptr, f, 2, 257, 10, 7, 7, 1e-6, 0, o, 42, c, bd, st) == UNSUPPORTED
    for args in ((None, k, 2, 5, 7, 7, 1e-6, 0, o, 42, c), (ptr, None, 2, 5, 7, 7, 1e-6, 0, o, 42, c),
                 (ptr, k, 2, 5, 7, 7, 1e-6, 0, None, 42, c), (ptr, k, -1, 5, 7, 7, 1e-6, 0, o, 42, c),
                 (ptr, k, 2, -5, 7, 7, 1e-6, 0, o, 42, c), (ptr, k, 2, 5, -7, 7, 1e-6, 0, o, 42, c),
                 (ptr, k, 2, 5, 7, 6, 1e-6, 0, o, 42, c), (ptr, k, 2, 5, 7, 7, 1e-6, 0, o, 41, c),
                 (ptr, k, 2, 5, 7, 7, -1.0, 0, o, 42, c), (ptr, k, 2, 5, 7, 7, 1e-6, 3, o, 42, c)):
        assert fm(*args, st) == BAD_ARG, args
    for args in ((None, f, 2, 5, 10, 7, 7, 1e-6, 0, o, 42, c, bd), (ptr, None, 2, 5, 10, 7, 7, 1e-6, 0, o, 42, c, bd),
                 (ptr, f, 2, 5, 10, 7, 7, 1e-6, 0, None, 42, c, bd), (ptr, f, 2, 5, 10, 7, 7, 1e-6, 0, o, 42, c, None),
                 (ptr, f, -2, 5, 10, 7, 7, 1e-6, 0, o, 42, c, bd), (ptr, f, 2, -5, 10, 7, 7, 1e-6, 0, o, 42, c, bd),
                 (ptr, f, 2, 5, -10, 7, 7, 1e-6, 0, o, 42, c, bd), (ptr, f, 2, 5, 10, -7, 7, 1e-6, 0, o, 42, c, bd),
                 (ptr, f, 2, 5, 10, 7, 7, float("nan"), 0, o, 42, c, bd)):
        assert fr(*args, st) == BAD_ARG, args
    assert fm(ptr, k, 0, 5, 7, 7, 1e-6, 0, o, 42, c, st) == OK and fr(ptr, f, 0, 5, 10, 7, 7, 1e-6, 0, o, 42, c, bd, st) == OK
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and counts.tolist() == [-5, -5] and int(bad.item()) == 0    # nothing was launched
    # and the same buffers through a good call
    assert fm(ptr, k, 2, 5, 7, 7, 1e-6, 0, o, 42, c, st) == OK
    torch.cuda.synchronize()
    assert counts.tolist() == [5, 5] and same_bits(out.cpu().numpy()[0], run_dense(x[0]))
    assert store.numel() == 71


def test_python_surface():
    import utils
    from isic_hip.moments import token_moments, token_moments_ragged
    x = R.make_input("mixed", 3, 196, 96, seed=2)
    keep = LR.keep_batch(LR.mixed_names(3), 196)                               # bernoulli, none, first
    xd = torch.from_numpy(x).to(DEV)
    for unbiased in (False, True):
        want, _, wcounts = run_masked(x, keep, 1e-3, unbiased)
        for dtype, scale in ((torch.bool, 1), (torch.uint8, 3), (torch.int64, -7), (torch.float32, 0.25), (torch.float16, -0.5)):
            kd = (torch.from_numpy(keep).to(DEV).to(torch.float32) * scale).to(dtype)      # any non-zero value keeps
            for fn in (token_moments, utils.concat_patch_moments):
                got = fn(xd, eps=1e-3, unbiased=unbiased, keep=kd)
                assert got.shape == (3, 6 * 96) and got.dtype == torch.float32 and got.device == xd.device
                assert same_bits(got.cpu().numpy(), want), (unbiased, dtype)
        got, counts = token_moments(xd, eps=1e-3, unbiased=unbiased, keep=torch.from_numpy(keep).to(DEV), return_counts=True)
        assert counts.dtype == torch.int32 and counts.device == xd.device and np.array_equal(counts.cpu().numpy(), wcounts)
        assert same_bits(got.cpu().numpy(), want)
        # the compacted store: host offsets, device offsets, an explicit bound
        rows, offsets = LR.compact(x, keep)
        rd = torch.from_numpy(rows).to(DEV)
        for off, mn in ((offsets.tolist(), None), (torch.from_numpy(offsets), None), (torch.from_numpy(offsets).to(DEV), None),
                        (torch.from_numpy(offsets).to(DEV), 256)):
            got, counts = token_moments_ragged(rd, off, eps=1e-3, unbiased=unbiased, max_nodes=mn, return_counts=True)
            assert got.shape == (3, 6 * 96) and same_bits(got.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), wcounts)
        assert same_bits(token_moments_ragged(rd, offsets.tolist(), eps=1e-3, unbiased=unbiased).cpu().numpy(), want)
    # a channel slice of a wider grid is read in place; a transposed view is made contiguous
    kd = torch.from_numpy(keep).to(DEV)
    lo, _, _ = run_masked(np.ascontiguousarray(x[:, :, :40]), keep)
    assert same_bits(token_moments(xd[:, :, :40], keep=kd).cpu().numpy(), lo)
    xt = np.ascontiguousarray(x.transpose(0, 2, 1))                             # [3, 96, 196]
    kt = LR.keep_batch(("alternating", "last", "none"), 96)
    tr, _, _ = run_masked(xt, kt)
    assert same_bits(token_moments(xd.transpose(1, 2), keep=torch.from_numpy(kt).to(DEV)).cpu().numpy(), tr)
    rows, offsets = LR.compact(x[:, :, :40], keep)
    wide = torch.from_numpy(np.ascontiguousarray(x[keep])).to(DEV)             # [total, 96]
    assert same_bits(token_moments_ragged(wide[:, :40], offsets.tolist()).cpu().numpy(), lo)
    # without keep: today's call and its counts; empty batches
    dense, dcounts = token_moments(xd, return_counts=True)
    assert torch.equal(dense, token_moments(xd)) and dcounts.tolist() == [196] * 3
    allk, _, _ = run_masked(x, np.ones((3, 196), dtype=bool))
    assert same_bits(dense.cpu().numpy(), allk)                                 # every flag set: the dense entry's bits
    assert token_moments(xd[:0], keep=kd[:0]).shape == (0, 6 * 96)
    out, counts = token_moments_ragged(wide, [0], return_counts=True)
    assert out.shape == (0, 6 * 96) and counts.shape == (0,)
    empty = token_moments_ragged(wide[:0], [0, 0, 0])
    assert empty.shape == (2, 6 * 96) and bool(torch.isnan(empty).all())
    g = xd.clone().requires_grad_(True)
    with pytest.raises(RuntimeError):
        token_moments(g, keep=kd)
    with torch.no_grad():
        assert same_bits(token_moments(g, keep=kd).cpu().numpy(), token_moments(xd, keep=kd).cpu().numpy())
    with pytest.raises(ValueError, match="is on"):
        token_moments(xd, keep=torch.from_numpy(keep))                          # keep on the host, latent on the device


def test_extract_latents_lesion_moments(tmp_path, monkeypatch):
    import save_latent as sl
    from isic_hip.moments import token_moments
    monkeypatch.chdir(tmp_path)                                                 # extract_latents writes dataframes_latents/ here
    cfg = {"device": DEV, "seed": 42, "pca": False}
    data = (sl.SyntheticDermImages(n=5), sl.SyntheticDermImages(n=5, seed=5))   # image 4 of each has no mask
    base = sl.extract_latents(cfg, "missing.pth", datasets=data, batch_size=4)
    les = sl.extract_latents(dict(cfg, lesion_moments=True), "missing.pth", datasets=data, batch_size=4)
    today = ["image_path", "segmentation_path", "target", "latent_pooled_max", "latent_pooled_mean", "ids_restore", "ids_keep"]
    for k in (2, 3):                                                            # the pooled frames
        assert list(base[k].columns) == today                                   # without the key: today's columns
        assert list(les[k].columns) == today + ["latent_lesion_moments", "lesion_patch_count"] and len(les[k]) == 5
        for col in ("image_path", "segmentation_path", "target"):
            assert list(base[k][col]) == list(les[k][col])
        for i in range(5):
            assert np.array_equal(base[k]["latent_pooled_max"].iloc[i], les[k]["latent_pooled_max"].iloc[i])
            assert np.array_equal(base[k]["latent_pooled_mean"].iloc[i], les[k]["latent_pooled_mean"].iloc[i])
        raw = les[k + 2]                                                        # the raw frame of the same split
        latent = np.stack(raw["latent"].values).astype(np.float32)              # [5, 196, D]
        flags = np.stack([np.asarray(m).ravel() for m in raw["lesion_mask_patches"].values]).astype(bool)
        want = token_moments(torch.from_numpy(latent).to(DEV), keep=torch.from_numpy(flags).to(DEV)).cpu().numpy()
        got = np.stack(les[k]["latent_lesion_moments"].values)
        assert got.dtype == np.float32 and got.shape == (5, 6 * latent.shape[2]) and same_bits(got, want)
        count = les[k]["lesion_patch_count"].to_numpy()
        assert count.tolist() == flags.sum(axis=1).tolist() and count[4] == 0 and (count[:4] > 0).all()
        assert np.isnan(got[4]).all() and np.isfinite(got[:4]).all()
    for k in (0, 1, 4, 5):                                                      # the patch and raw frames do not depend on the key
        assert len(base[k]) == len(les[k]) and list(base[k].columns) == list(les[k].columns)
