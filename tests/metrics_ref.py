"""Numpy restatement of the device metric counts (csrc/metrics.hip, include/isic_hip_metrics.h) and of the float formulas of
isic_hip/metrics.py, the case lists both test modules walk, and deliberately wrong variants.  Plain numpy on the CPU; shared
by tests/test_metrics_ref_cpu.py (the restatement's floats equal sklearn's, every wrong variant changes an integer on some
case) and tests/test_metrics_gpu.py (the device's integers equal the restatement's bit for bit on the same cases).

Counts, for scores [n, C] fp32 and labels [n] int64; a sample is counted when its label lies in [0, C) and its C scores are
finite:
    confusion[t][p] = #{counted i : labels[i] == t, argmax_i == p}     argmax = the LOWEST index holding the row maximum
    pair2[c]        = sum over counted i with labels[i] == c, counted j with labels[j] != c of 2 [s_ic > s_jc] + [s_ic == s_jc]
    flags           = (#non-finite score elements, #labels outside [0, C))
as a literal O(n^2) broadcast of fp32 compares (numpy compares subnormals by value; -0.0 == 0.0).
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "include", "isic_hip_metrics.h")).read()
BLOCK = int(re.search(r"#define\s+ISIC_METRICS_BLOCK\s+(\d+)", _HDR).group(1))
TILE = int(re.search(r"#define\s+ISIC_METRICS_TILE\s+(\d+)", _HDR).group(1))

SEED = 20240
SIZES = (1, 2, 5, BLOCK - 1, BLOCK, BLOCK + 1, TILE + 1, 2 * TILE + 3)
CLASSES = (2, 3, 7, 16)
FAMILIES = ("softmax", "quant1", "quant2", "quant4", "equal", "absent1", "absent2", "one_label", "subnormal", "neg_zero",
            "tied_max")
CASES = tuple((f, n, C) for f in FAMILIES for n in SIZES for C in CLASSES)
VARIANTS = ("ties0", "ties2", "ge_one_side", "argmax_last", "flush_subnormals", "pair_int32", "pair_uint32")
FLT_MIN = np.float32(2.0 ** -126)

# The smallest case at which a 32-bit pair total goes wrong: n = 98304, C = 2, labels alternate 0, 1 (balanced).  The
# expectations are closed-form, so no n^2 restatement is needed.
BIG_N = 98304
BIG_HALF2 = (BIG_N // 2) ** 2                     # 2 415 919 104 > 2^31


def big_case(kind):
    """-> scores [BIG_N, 2] fp32, labels, expected confusion [2, 2], expected pair2 [2]"""
    labels = (np.arange(BIG_N) % 2).astype(np.int64)
    h = BIG_N // 2
    if kind == "equal":                           # every pair ties: (n/2)^2 per class; argmax 0 everywhere
        scores = np.full((BIG_N, 2), 0.5, dtype=np.float32)
        return scores, labels, np.array([[h, 0], [h, 0]], dtype=np.int64), np.array([BIG_HALF2, BIG_HALF2], dtype=np.int64)
    if kind == "separated":                       # column 1: every positive above every negative -> 2 (n/2)^2 > 2^32;
        scores = np.empty((BIG_N, 2), dtype=np.float32)      # column 0 constant -> ties -> (n/2)^2
        scores[:, 0] = 0.5
        scores[:, 1] = np.where(labels == 1, 0.75, 0.25) + (np.arange(BIG_N) % 1024).astype(np.float32) * np.float32(2.0 ** -14)
        return scores, labels, np.array([[h, 0], [0, h]], dtype=np.int64), np.array([BIG_HALF2, 2 * BIG_HALF2], dtype=np.int64)
    raise KeyError(kind)


BIG_KINDS = ("equal", "separated")


# ---------------------------------------------------------------------------------------------------- input families
def _softmax32(logits):
    z = logits.astype(np.float32)
    z = z - z.max(axis=1, keepdims=True)
    e = np.exp(z, dtype=np.float32)
    return (e / e.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)


def make_case(family, n, C):
    """-> (scores [n, C] fp32, labels [n] int64), a pure function of its arguments"""
    rng = np.random.default_rng(SEED + 1009 * FAMILIES.index(family) + 31 * n + C)
    labels = rng.integers(0, C, size=n).astype(np.int64)
    logits = 2.0 * rng.standard_normal((n, C)) + 1.5 * np.eye(C)[labels]
    scores = _softmax32(logits)
    if family == "softmax":
        pass
    elif family.startswith("quant"):              # logits on a grid of 1, 2 or 4 levels per unit, clipped: heavy ties
        q = float(family[5:])
        scores = _softmax32(np.clip(np.round(logits * 0.5 * q) / q, -1.0, 1.0))
    elif family == "equal":
        scores = np.full((n, C), 1.0 / C, dtype=np.float32)
    elif family in ("absent1", "absent2"):        # one or two classes never occur as a label (at least one class stays)
        k = min(int(family[-1]), C - 1)
        gone = rng.choice(C, size=k, replace=False)
        keep = np.setdiff1d(np.arange(C), gone)
        labels = keep[rng.integers(0, len(keep), size=n)].astype(np.int64)
    elif family == "one_label":
        labels = np.full(n, C // 2, dtype=np.int64)
    elif family == "subnormal":                   # column 0: multiples of 1e-40 below 2^-126, with ties
        scores[:, 0] = (rng.integers(0, 100, size=n).astype(np.float64) * 1e-40).astype(np.float32)
        assert (np.abs(scores[:, 0]) < FLT_MIN).all()
    elif family == "neg_zero":                    # column 0 of -0.0 / 0.0 / a few positives; some rows all zeros of both signs
        scores[:, 0] = rng.choice(np.array([-0.0, 0.0, 1e-3], dtype=np.float32), size=n)
        rows = rng.random(n) < 0.25
        scores[rows] = rng.choice(np.array([-0.0, 0.0], dtype=np.float32), size=(int(rows.sum()), C))
    elif family == "tied_max":                    # the row maximum sits in two columns
        a = rng.integers(0, C - 1, size=n)
        b = a + 1 + rng.integers(0, C - 1 - a)
        top = scores.max(axis=1)
        scores[np.arange(n), a] = top
        scores[np.arange(n), b] = top
    else:
        raise KeyError(family)
    return np.ascontiguousarray(scores, dtype=np.float32), labels


def make_loss(n, seed=0):
    rng = np.random.default_rng(SEED + 77 + n + seed)
    return (-np.log(rng.random(n) * 0.999 + 1e-3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the counts
def counted(scores, labels, C):
    return (labels >= 0) & (labels < C) & np.isfinite(scores).all(axis=1)


def counts(scores, labels, C, variant=None):
    """-> confusion [C, C] int64, pair2 [C] int64, flags [2] int64; `variant` one of VARIANTS for a wrong restatement"""
    scores = np.asarray(scores, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    flags = np.array([np.count_nonzero(~np.isfinite(scores)), np.count_nonzero((labels < 0) | (labels >= C))], dtype=np.int64)
    keep = counted(scores, labels, C)
    s, y = scores[keep], labels[keep]
    if variant == "flush_subnormals":
        s = np.where(np.abs(s) < FLT_MIN, np.float32(0.0), s)
    if len(s):
        pred = (C - 1 - np.argmax(s[:, ::-1], axis=1)) if variant == "argmax_last" else np.argmax(s, axis=1)
    else:
        pred = np.zeros(0, dtype=np.int64)
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (y, pred), 1)
    pair2 = np.zeros(C, dtype=np.int64)
    for c in range(C):
        pos, neg = s[y == c, c][:, None], s[y != c, c][None, :]
        gt, eq = np.count_nonzero(pos > neg), np.count_nonzero(pos == neg)
        if variant == "ties0":
            pair2[c] = 2 * gt
        elif variant == "ties2":
            pair2[c] = 2 * gt + 2 * eq
        elif variant == "ge_one_side":            # the tie term written as >=
            pair2[c] = 2 * gt + np.count_nonzero(pos >= neg)
        else:
            pair2[c] = 2 * gt + eq
    return conf, wrap(pair2, variant), flags


def wrap(pair2, variant):
    """the total as a 32-bit accumulator would hold it"""
    if variant == "pair_int32":
        return pair2.astype(np.int32).astype(np.int64)
    if variant == "pair_uint32":
        return pair2.astype(np.uint32).astype(np.int64)
    return pair2


# ---------------------------------------------------------------------------------------------------- the floats
def floats(conf, pair2):
    """The formulas of isic_hip/metrics.py restated: -> dict of fp64 values (per_class_auc an array)."""
    conf = np.asarray(conf, dtype=np.int64)
    C = conf.shape[0]
    n = int(conf.sum())
    nan = float("nan")
    support, predicted = conf.sum(axis=1), conf.sum(axis=0)
    rec, prec, f1, auc = np.zeros(C), np.zeros(C), np.zeros(C), np.full(C, np.nan)
    for c in range(C):
        tp = float(conf[c, c])
        rec[c] = tp / support[c] if support[c] else 0.0
        prec[c] = tp / predicted[c] if predicted[c] else 0.0
        f1[c] = 2.0 * prec[c] * rec[c] / (prec[c] + rec[c]) if prec[c] + rec[c] > 0 else 0.0
        if support[c] and n - support[c]:
            auc[c] = float(pair2[c]) / (2.0 * float(support[c]) * float(n - support[c]))
    has, present = support > 0, (support + predicted) > 0
    out = {"accuracy": float(np.trace(conf)) / n if n else nan,
           "bacc": float(rec[has].mean()) if has.any() else nan,
           "auc": float(auc.mean()), "per_class_auc": auc}
    for name, v in (("precision", prec), ("recall", rec), ("f1", f1)):
        out["macro_" + name] = float(v[present].mean()) if present.any() else nan
        out["weighted_" + name] = float((v * support).sum() / n) if n else nan
    return out


FLOAT_KEYS = ("accuracy", "bacc", "auc", "macro_precision", "macro_recall", "macro_f1", "weighted_precision",
              "weighted_recall", "weighted_f1")
