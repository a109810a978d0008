"""The token statistics over a subset of each image's tokens, checked without a device: the restatement
(tests/moments_lesion_ref.py) against the reference's recorded outputs on the kept tokens, the NaN conventions, the two C
entries declared where they belong with argument checks that answer before any device work, and every rejection of the Python
surface."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moments_lesion_ref as LR  # noqa: E402
import moments_ref as R  # noqa: E402
from isic_hip import lib  # noqa: E402

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
P = 0x10000                      # a dummy, 16-byte aligned, non-NULL pointer: never dereferenced (errors come first)
NAMES = ("isic_token_moments_masked_f32", "isic_token_moments_ragged_f32")
HEADER = "isic_hip_moments_ragged.h"


@pytest.fixture(scope="module")
def golden():
    with np.load(LR.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_golden_file_holds_exactly_the_defined_rows(golden):
    keys = [k for k, _, _, _ in LR.golden_keys()]
    assert sorted(golden) == sorted(keys) and len(keys) == 11      # 3 + 3 of "grid"; 3 + 2 of "small" (n = 6, 1, 0, 12)
    assert os.path.getsize(LR.GOLDEN) < 16384
    _, keep = LR.golden_input("small")
    assert keep.sum(axis=1).tolist() == [6, 1, 0, 12]


@pytest.mark.parametrize("key,name,unbiased,b", LR.golden_keys())
def test_restatement_agrees_with_the_recorded_reference(golden, key, name, unbiased, b):
    x, keep = LR.golden_input(name)
    D = x.shape[2]
    ref = LR.reference_masked(x, keep, R.EPS, unbiased)[b:b + 1]
    bound = LR.bounds_masked(x, keep, R.EPS, unbiased)[b:b + 1]
    rec = golden[key][None]
    assert rec.dtype == np.float32 and rec.shape == (1, 6 * D) and np.isfinite(bound).all() and np.isfinite(ref).all()
    print(f"{key}: worst error / bound {R.worst_per_stat(rec, ref, bound)}")
    assert R.selections_equal(rec, ref)                                     # max and median: element for element
    assert R.worst(rec, ref, bound) <= 1.0
    kept = x[b, keep[b]]
    assert np.array_equal(rec[0, D:2 * D], kept.max(axis=0))
    assert np.array_equal(rec[0, 3 * D:4 * D], np.sort(kept, axis=0)[(len(kept) - 1) // 2])


@pytest.mark.parametrize("unbiased", (False, True))
def test_nan_rows_are_exactly_where_the_definition_puts_them(unbiased):
    for name in LR.GOLDEN_CASES:
        x, keep = LR.golden_input(name)
        D = x.shape[2]
        ref = LR.reference_masked(x, keep, R.EPS, unbiased)
        assert np.array_equal(np.isnan(ref), LR.expected_nan(keep, D, unbiased)), name
    x, keep = LR.golden_input("small")                                          # n = 6, 1, 0, 12
    D = x.shape[2]
    ref = LR.reference_masked(x, keep, R.EPS, unbiased)
    assert np.isnan(ref[2]).all() and np.isfinite(ref[0]).all() and np.isfinite(ref[3]).all()
    lone = x[1, 0].astype(np.float64)
    for s in (0, 1, 3):                                                         # mean, max, median: the element
        assert np.array_equal(ref[1, s * D:(s + 1) * D], lone)
    for s in LR.NAN_STATS_LONE:
        assert bool(np.isnan(ref[1, s * D:(s + 1) * D]).all()) == unbiased
    if not unbiased:                                                            # one token: std 0, sigma = eps, 0 / eps^k
        assert (ref[1, 2 * D:3 * D] == 0).all() and (ref[1, 4 * D:5 * D] == 0).all() and (ref[1, 5 * D:] == -3).all()


@pytest.mark.filterwarnings("ignore:std")
def test_torch_gives_the_lone_token_convention():
    """std of one value is NaN under `unbiased`, and clamp(min=eps) keeps a NaN: the convention is torch's own"""
    one = torch.tensor([[[1.5], ]])
    out = R.torch_composition(one, R.EPS, True)[0]
    assert out[0] == 1.5 and out[1] == 1.5 and out[3] == 1.5
    assert torch.isnan(out[2]) and torch.isnan(out[4]) and torch.isnan(out[5])


def test_restatement_is_the_dense_one_on_the_kept_tokens_and_ragged_agrees():
    x = R.make_input("mixed", 3, 65, 7)
    keep = LR.keep_batch(("bernoulli", "alternating", "all"), 65)
    ref = LR.reference_masked(x, keep)
    for b in range(3):
        assert np.array_equal(ref[b], R.reference(np.ascontiguousarray(x[b:b + 1, keep[b]]))[0])
    assert np.array_equal(ref[2], R.reference(x[2:3])[0])
    rows, offsets = LR.compact(x, keep)
    assert offsets[-1] == len(rows) == keep.sum() and np.array_equal(LR.reference_ragged(rows, offsets), ref)
    for name in LR.PATTERNS:                                                    # the patterns are what their names say
        k = LR.keep_pattern(name, 65)
        assert k.dtype == bool and k.shape == (65,)
    assert LR.keep_pattern("none", 5).sum() == 0 and LR.keep_pattern("all", 5).sum() == 5
    assert LR.keep_pattern("first", 5).tolist() == [True, False, False, False, False]
    assert LR.keep_pattern("last", 5).tolist() == [False, False, False, False, True]
    assert LR.keep_pattern("prefix", 5).tolist() == [True, True, False, False, False]
    assert LR.keep_pattern("suffix", 5).tolist() == [False, False, True, True, True]
    assert LR.keep_pattern("alternating", 5).tolist() == [True, False, True, False, True]
    assert 30 < LR.keep_pattern("bernoulli", 196).sum() < 90


def test_entries_are_declared_in_the_new_header_only_and_exported():
    inc = os.path.dirname(lib.header_path())
    assert f'#include "{HEADER}"' in open(os.path.join(inc, "isic_hip.h")).read()
    raw = open(os.path.join(inc, HEADER)).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    assert os.path.join(inc, HEADER) in [os.path.normpath(p) for p in lib.extension_header_paths()]
    protos = lib.parse_header(os.path.join(inc, HEADER))
    assert set(protos) == set(NAMES) and [len(protos[n][1]) for n in NAMES] == [12, 14]
    for n in NAMES:
        assert protos[n][0] is ctypes.c_int and protos[n][1][-1][1] == "stream", n
    assert [a[1] for a in protos[NAMES[0]][1]] == ["X", "keep", "B", "T", "D", "ldx", "eps", "unbiased", "out", "ldo", "counts",
                                                  "stream"]
    assert [a[1] for a in protos[NAMES[1]][1]] == ["X", "node_offsets", "G", "max_nodes", "total", "D", "ldx", "eps", "unbiased",
                                                  "out", "ldo", "counts", "bad", "stream"]
    rg = {a[1]: a for a in protos[NAMES[1]][1]}
    assert rg["G"][0] is ctypes.c_int64 and rg["total"][0] is ctypes.c_int64 and rg["ldx"][0] is ctypes.c_int64
    L = lib.lib()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name not in L.public and name in L.fn and hasattr(cdll, name), name
    assert len(L.public) == 96
    assert f"#define ISIC_MOMENTS_RAGGED_MAX_NODES {LR.MAX_NODES}\n" in raw and "quiet NaN" in raw
    from isic_hip import build, moments
    assert moments.MAX_NODES == LR.MAX_NODES and HEADER in map(os.path.basename, build.header_deps())


def _masked(X=P, keep=P, B=2, T=5, D=7, ldx=7, eps=1e-6, unbiased=0, out=P, ldo=42, counts=P):
    return lib.lib().fn[NAMES[0]](X, keep, B, T, D, ldx, eps, unbiased, out, ldo, counts, None)


def _ragged(X=P, off=P, G=2, max_nodes=5, total=9, D=7, ldx=7, eps=1e-6, unbiased=0, out=P, ldo=42, counts=P, bad=P):
    return lib.lib().fn[NAMES[1]](X, off, G, max_nodes, total, D, ldx, eps, unbiased, out, ldo, counts, bad, None)


def test_masked_argument_checks_answer_without_a_device():
    nan = float("nan")
    for kw in (dict(X=None), dict(keep=None), dict(out=None), dict(B=-1), dict(T=0), dict(T=-3), dict(D=0), dict(ldx=6), dict(ldo=41),
               dict(eps=-1e-6), dict(eps=nan), dict(unbiased=2), dict(unbiased=-1), dict(counts=P + 2)):
        assert _masked(**kw) == BAD_ARG, kw
    assert _masked(T=LR.MAX_NODES + 1) == UNSUPPORTED
    assert _masked(B=1 << 31, T=1) == UNSUPPORTED                               # a grid that would not fit
    assert _masked(B=1 << 28, D=768, ldx=768, ldo=4608) == UNSUPPORTED          # 2^28 images x 12 slabs
    assert _masked(B=0) == OK and _masked(B=0, X=None, keep=None, out=None, counts=None) == OK
    assert _masked(B=0, T=1, unbiased=1) == OK                                  # unbiased with T = 1 is a device fact here
    assert _masked(B=0, T=LR.MAX_NODES) == OK and _masked(B=0, T=LR.MAX_NODES + 1) == UNSUPPORTED


def test_ragged_argument_checks_answer_without_a_device():
    nan = float("nan")
    for kw in (dict(X=None), dict(off=None), dict(out=None), dict(bad=None), dict(G=-1), dict(max_nodes=-1), dict(total=-1),
               dict(D=0), dict(ldx=6), dict(ldo=41), dict(eps=-1e-6), dict(eps=nan), dict(unbiased=2), dict(unbiased=-1),
               dict(off=P + 4), dict(counts=P + 2), dict(bad=P + 2)):
        assert _ragged(**kw) == BAD_ARG, kw
    assert _ragged(max_nodes=LR.MAX_NODES + 1) == UNSUPPORTED
    assert _ragged(G=1 << 31) == UNSUPPORTED and _ragged(G=1 << 28, D=768, ldx=768, ldo=4608) == UNSUPPORTED
    assert _ragged(G=0) == OK and _ragged(G=0, X=None, off=None, out=None, counts=None, bad=None) == OK
    assert _ragged(G=0, max_nodes=LR.MAX_NODES, unbiased=1) == OK and _ragged(G=0, max_nodes=LR.MAX_NODES + 1) == UNSUPPORTED


def _import_utils():
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(lib.__file__)))
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import utils
    return utils


def test_token_moments_keep_raises_before_the_device_is_touched():
    from isic_hip.moments import token_moments
    utils = _import_utils()
    x = torch.zeros(2, 4, 8)
    keep = torch.ones(2, 4, dtype=torch.bool)
    for fn in (token_moments, utils.concat_patch_moments):
        for bad_keep in (torch.ones(2, 5), torch.ones(4, 2), torch.ones(2, 4, 1), torch.ones(8), np.ones((2, 4), dtype=bool),
                         [[1] * 4] * 2, torch.ones(2, 4, dtype=torch.complex64)):
            with pytest.raises(ValueError, match="keep"):
                fn(x, keep=bad_keep)
        with pytest.raises(ValueError, match="masked entry"):
            fn(torch.zeros(1, LR.MAX_NODES + 1, 2), keep=torch.ones(1, LR.MAX_NODES + 1))
        with pytest.raises(ValueError, match="eps"):
            fn(x, eps=-1.0, keep=keep)
        with pytest.raises(ValueError, match="eps"):
            fn(x, eps=float("nan"), keep=keep)
        with pytest.raises(ValueError):
            fn(torch.zeros(4, 8), keep=keep)                                    # latent not 3-D
        with pytest.raises(ValueError):
            fn(x.half(), keep=keep)                                             # latent not fp32
        with pytest.raises(ValueError, match="is on"):
            fn(x, keep=keep.to("meta"))                                         # keep on another device than latent
        for dtype in (torch.bool, torch.uint8, torch.int64, torch.float32, torch.float16):
            with pytest.raises(lib.IsicHipError, match="CPU tensor"):           # every dtype passes the checks: the CPU tensor stops it
                fn(x, keep=keep.to(dtype))
        # the host-side `unbiased` check on T == 1 does not apply with keep (n is a device fact) ...
        with pytest.raises(lib.IsicHipError, match="CPU tensor"):
            fn(torch.zeros(2, 1, 8), unbiased=True, keep=torch.ones(2, 1))
        with pytest.raises(ValueError, match="two tokens"):                     # ... and is kept without it
            fn(torch.zeros(2, 1, 8), unbiased=True)
        with pytest.raises(RuntimeError, match="no backward"):
            fn(torch.zeros(2, 4, 8, requires_grad=True), keep=keep)


def test_token_moments_ragged_raises_before_the_device_is_touched():
    from isic_hip.moments import token_moments_ragged as tmr
    x = torch.zeros(9, 8)
    off = torch.tensor([0, 4, 9])
    for args in ((torch.zeros(2, 4, 8), off), (torch.zeros(9), off), ([[0.0] * 8] * 9, off)):
        with pytest.raises(ValueError, match="2-D"):
            tmr(*args)
    with pytest.raises(ValueError, match="fp32"):
        tmr(x.double(), off)
    with pytest.raises(ValueError, match="D must"):
        tmr(torch.zeros(9, 0), off)
    for bad_off in (off.to(torch.int32), off.double(), off.reshape(1, 3), torch.zeros(0, dtype=torch.int64), [0.0, 4.0, 9.0]):
        with pytest.raises(ValueError, match="offsets"):
            tmr(x, bad_off)
    with pytest.raises(ValueError, match="max_nodes"):
        tmr(x, off, max_nodes=-1)
    with pytest.raises(ValueError, match="exceeds 256"):
        tmr(x, off, max_nodes=LR.MAX_NODES + 1)
    with pytest.raises(ValueError, match="exceeds 256"):                        # taken from the offsets
        tmr(torch.zeros(300, 8), torch.tensor([0, 257, 300]))
    with pytest.raises(ValueError, match="eps"):
        tmr(x, off, eps=-1.0)
    with pytest.raises(RuntimeError, match="no backward"):
        tmr(torch.zeros(9, 8, requires_grad=True), off)
    for offsets in (off, [0, 4, 9], np.array([0, 4, 9], dtype=np.int64)):       # host offsets in any of these forms pass
        with pytest.raises(lib.IsicHipError, match="CPU tensor"):
            tmr(x, offsets)
    with pytest.raises(lib.IsicHipError, match="CPU tensor"):
        tmr(x, off, unbiased=True, max_nodes=256, return_counts=True)


def test_keep_none_reaches_the_old_call(monkeypatch):
    """without `keep` the dense entry is called with today's arguments, and nothing else"""
    from isic_hip import moments
    utils = _import_utils()
    calls = []
    monkeypatch.setattr(moments, "call", lambda name, *a: calls.append((name, a)))

    class OnDevice(torch.Tensor):                                               # a CPU tensor that says it is a device tensor
        is_cuda = True

    class NoDevice:
        def __init__(self, device):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(torch.cuda, "device", NoDevice)
    x = torch.zeros(3, 5, 8).as_subclass(OnDevice)
    for fn in (moments.token_moments, utils.concat_patch_moments):
        del calls[:]
        out = fn(x, eps=1e-3, unbiased=True)
        assert isinstance(out, torch.Tensor) and out.shape == (3, 48)
        assert len(calls) == 1 and calls[0][0] == "isic_token_moments_f32"
        a = calls[0][1]
        assert a[0] == x.data_ptr() and a[1:7] == (3, 5, 8, 8, 1e-3, 1) and a[7] is out and a[8] == 48 and len(a) == 9
        del calls[:]
        fn(x, keep=torch.ones(3, 5).as_subclass(OnDevice))
        assert [c[0] for c in calls] == ["isic_token_moments_masked_f32"]
        a = calls[0][1]
        assert a[0] == x.data_ptr() and a[1].dtype == torch.uint8 and a[1].shape == (3, 5) and a[2:8] == (3, 5, 8, 8, 1e-6, 0)
        assert a[9] == 48 and a[10] is None and len(a) == 11


def test_lesion_moments_key_is_documented_and_defaults_to_off():
    _import_utils()
    import inspect
    import save_latent as sl
    assert "lesion_moments" in sl.__doc__
    src = inspect.getsource(sl.extract_latents)
    assert 'config.get("lesion_moments", False)' in src
    assert inspect.signature(sl._extract_from_loader).parameters["lesion_moments"].default is False
