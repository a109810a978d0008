"""Inputs, keep patterns and the CPU restatement for the token statistics over a SUBSET of each image's tokens
(include/isic_hip_moments_ragged.h, csrc/token_moments_ragged.hip, ``isic_hip.moments.token_moments(keep=...)`` and
``token_moments_ragged``).  Plain numpy; shared by tests/test_moments_lesion_cpu.py, tests/test_moments_lesion_gpu.py and
tests/gen_moments_lesion_golden.py.

Everything numeric is tests/moments_ref.py applied to an image's kept tokens (imported, not restated): ``reference_masked``
is ``moments_ref.reference`` on ``x[b:b+1, keep[b]]`` and ``bounds_masked`` is ``moments_ref.bounds`` of the same tokens.
The two conventions of the header are filled in here:
    n == 0                 all six statistics NaN
    n == 1 with unbiased   mean, max, median the element; std, skewness, kurtosis NaN (torch: std is NaN, clamp keeps it)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moments_ref as R  # noqa: E402

MAX_NODES = 256                  # ISIC_MOMENTS_RAGGED_MAX_NODES
NAN_STATS_LONE = (2, 4, 5)       # std, skewness, kurtosis: NaN for one kept token with `unbiased`
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_moments_lesion.npz")

PATTERNS = ("all", "none", "first", "last", "alternating", "prefix", "suffix", "bernoulli")


def keep_pattern(name, T, seed=0):
    """bool [T]"""
    k = np.zeros(T, dtype=bool)
    if name == "all":
        k[:] = True
    elif name == "none":
        pass
    elif name == "first":
        k[0] = True
    elif name == "last":
        k[-1] = True
    elif name == "alternating":
        k[::2] = True
    elif name == "prefix":
        k[:(T + 2) // 3] = True
    elif name == "suffix":
        k[T - (T + 1) // 2:] = True
    elif name == "bernoulli":
        k = np.random.default_rng(4242 + 131 * seed + T).random(T) < 0.3
    else:
        raise KeyError(name)
    return k


def keep_batch(names, T, seed=0):
    """bool [len(names), T]: image b follows pattern names[b]"""
    return np.stack([keep_pattern(n, T, seed + 17 * b) for b, n in enumerate(names)])


def mixed_names(B):
    """one batch that mixes the patterns, starting with those that differ most"""
    order = ("bernoulli", "none", "first", "all", "alternating", "last", "prefix", "suffix")
    return [order[b % len(order)] for b in range(B)]


def defined(n, unbiased):
    """True where the dense entry is defined for T = n (the bit-equality rule applies)"""
    return n >= (2 if unbiased else 1)


def compact(x, keep):
    """x [B, T, D], keep bool [B, T] -> (rows [total, D] in image-major, token order; offsets int64 [B + 1])"""
    keep = np.asarray(keep, dtype=bool)
    counts = keep.sum(axis=1).astype(np.int64)
    return np.ascontiguousarray(x[keep]), np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _fill(x, keep, eps, unbiased, fn):
    x = np.asarray(x)
    keep = np.asarray(keep, dtype=bool)
    B, T, D = x.shape
    out = np.full((B, 6 * D), np.nan, dtype=np.float64)
    for b in range(B):
        n = int(keep[b].sum())
        if n == 0:
            continue
        rows = x[b:b + 1, keep[b]]
        if defined(n, unbiased):
            out[b] = fn(rows, eps, unbiased)[0]
        else:                                                   # n == 1, unbiased
            out[b] = fn(rows, eps, False)[0]
            for s in NAN_STATS_LONE:
                out[b, s * D:(s + 1) * D] = np.nan
    return out


def reference_masked(x, keep, eps=R.EPS, unbiased=False):
    """-> [B, 6 D] float64: ``moments_ref.reference`` of each image's kept tokens, with the two NaN conventions"""
    return _fill(x, keep, eps, unbiased, R.reference)


def bounds_masked(x, keep, eps=R.EPS, unbiased=False):
    """-> [B, 6 D] float64: ``moments_ref.bounds`` of each image's kept tokens; NaN where the reference is NaN"""
    return _fill(x, keep, eps, unbiased, R.bounds)


def reference_ragged(rows, offsets, eps=R.EPS, unbiased=False, fn=R.reference):
    """rows [total, D], offsets [G + 1] -> [G, 6 D] float64 (the same conventions, per graph)"""
    rows = np.asarray(rows)
    G, D = len(offsets) - 1, rows.shape[1]
    out = np.full((G, 6 * D), np.nan, dtype=np.float64)
    for g in range(G):
        seg = rows[offsets[g]:offsets[g + 1]][None]
        out[g] = _fill(seg, np.ones((1, seg.shape[1]), dtype=bool), eps, unbiased, fn)[0]
    return out


def expected_nan(keep, D, unbiased):
    """bool [B, 6 D]: exactly where the definition puts a NaN (finite inputs, eps > 0)"""
    counts = np.asarray(keep, dtype=bool).sum(axis=1)
    m = np.zeros((len(counts), 6, D), dtype=bool)
    m[counts == 0] = True
    if unbiased:
        for s in NAN_STATS_LONE:
            m[counts == 1, s] = True
    return m.reshape(len(counts), 6 * D)


# name -> (kind, B, T, D, keep patterns per image): the cases recorded from the reference in tests/golden/patch_moments_lesion.npz
GOLDEN_CASES = {
    "grid": ("mixed", 3, 196, 8, ("bernoulli", "prefix", "alternating")),
    "small": ("mixed", 4, 12, 4, ("suffix", "first", "none", "all")),
}


def golden_input(name):
    kind, B, T, D, names = GOLDEN_CASES[name]
    return R.make_input(kind, B, T, D), keep_batch(names, T)


def golden_keys():
    """(key in the npz, case name, unbiased, image) for every image the reference is defined on"""
    out = []
    for name in GOLDEN_CASES:
        _, keep = golden_input(name)
        for unbiased in (False, True):
            for b, n in enumerate(keep.sum(axis=1)):
                if defined(int(n), unbiased):
                    out.append((f"{name}_u{int(unbiased)}_b{b}", name, unbiased, b))
    return out


# the device shapes
DEVICE_T = (1, 2, 5, 64, 65, 196, 256)
DEVICE_D = (1, 7, 64, 65, 130)
DEVICE_B = (1, 3)
RAGGED_SIZES = (0, 1, 2, 63, 64, 65, 196, 256)
