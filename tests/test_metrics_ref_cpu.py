"""The restatement of tests/metrics_ref.py on the CPU: its floats (and those ``isic_hip.metrics.ClassMetrics`` forms from the
same integers) equal scikit-learn's on every case, the golden fixture is reproduced from fp32 scores, and every wrong
variant kept there changes at least one integer on at least one case -- so the bit-exact comparison of
tests/test_metrics_gpu.py can tell each of them from the right answer.

Tolerance against sklearn: 1e-12 absolute.  Both sides evaluate the same rational numbers in fp64; the only difference is
the order of at most n additions of terms <= 1 in sklearn's trapezoid sum, about n 2^-53 = 1e-13 at n = 1027 (observed:
2e-16).  NaN must meet NaN."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import metrics_ref as R  # noqa: E402

TOL = 1e-12
_CACHE = {}


def case_counts(case):
    """the restatement of a case, computed once and shared (read-only)"""
    if case not in _CACHE:
        s, y = R.make_case(*case)
        conf, pair2, flags = R.counts(s, y, case[2])
        for a in (s, y, conf, pair2, flags):
            a.setflags(write=False)
        _CACHE[case] = (s, y, conf, pair2, flags)
    return _CACHE[case]


def same(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= TOL


def sklearn_floats(scores, labels, C):
    from sklearn.metrics import accuracy_score, balanced_accuracy_score, precision_recall_fscore_support, roc_auc_score
    pred = scores.argmax(axis=1)
    per = np.full(C, np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for c in range(C):
            try:
                per[c] = roc_auc_score(labels == c, scores[:, c])
            except ValueError:                    # one class only
                pass
        out = {"accuracy": accuracy_score(labels, pred), "bacc": balanced_accuracy_score(labels, pred),
               "auc": float(per.mean()), "per_class_auc": per}
        for avg in ("macro", "weighted"):
            p, r, f, _ = precision_recall_fscore_support(labels, pred, average=avg, zero_division=0)
            out[avg + "_precision"], out[avg + "_recall"], out[avg + "_f1"] = float(p), float(r), float(f)
        # the call the loops make (train.gnn_metrics), where sklearn accepts the input: more than two columns, rows summing to 1
        if C > 2 and np.allclose(1.0, scores.sum(axis=1)):
            try:
                out["ovr"] = float(roc_auc_score(labels, scores, multi_class="ovr", labels=np.arange(C)))
            except ValueError:
                out["ovr"] = float("nan")
    return out


@pytest.mark.parametrize("n,C", [(n, C) for n in R.SIZES for C in R.CLASSES])
def test_floats_agree_with_sklearn(n, C):
    from isic_hip.metrics import ClassMetrics
    for family in R.FAMILIES:
        s, y, conf, pair2, flags = case_counts((family, n, C))
        assert flags.tolist() == [0, 0]
        ref, mine, cm = sklearn_floats(s, y, C), R.floats(conf, pair2), ClassMetrics(conf, pair2)
        for k in R.FLOAT_KEYS:
            assert same(mine[k], ref[k]), (family, k, mine[k], ref[k])
            assert same(getattr(cm, k), ref[k]), (family, "ClassMetrics", k, getattr(cm, k), ref[k])
        for c in range(C):
            assert same(mine["per_class_auc"][c], ref["per_class_auc"][c]), (family, c)
            assert same(cm.per_class_auc[c], ref["per_class_auc"][c]), (family, c)
        if "ovr" in ref:
            assert same(mine["auc"], ref["ovr"]), (family, mine["auc"], ref["ovr"])
        assert np.array_equal(cm.confusion, conf) and cm.n == n
        assert set(cm.as_dict()) == {"loss", "accuracy", "bacc", "auc", "macro_f1"}


def test_golden_fixture_from_fp32_scores(golden_dir):
    from isic_hip.metrics import ClassMetrics
    g = np.load(os.path.join(golden_dir, "metrics.npz"))
    s, y = g["scores"].astype(np.float32), g["y"].astype(np.int64)
    conf, pair2, flags = R.counts(s, y, s.shape[1])
    assert flags.tolist() == [0, 0]
    f, cm = R.floats(conf, pair2), ClassMetrics(conf, pair2)
    for got in (f["auc"], cm.auc):
        assert abs(got - float(g["auc"])) <= TOL
    for got in (f["bacc"], cm.bacc):
        assert abs(got - float(g["bacc"])) <= TOL


def test_big_case_closed_forms_match_a_scaled_down_restatement():
    """the closed forms of the 64-bit case, checked where the n^2 restatement is affordable: the same construction cut to
    its first 2048 rows must give (m/2)^2 and 2 (m/2)^2"""
    m = 2048
    for kind in R.BIG_KINDS:
        s, y, conf_big, pair_big = R.big_case(kind)
        conf, pair2, flags = R.counts(s[:m], y[:m], 2)
        scale = (R.BIG_N // m)
        assert np.array_equal(conf * scale, conf_big) and np.array_equal(pair2 * scale * scale, pair_big)
    assert R.BIG_HALF2 > 2 ** 31 and 2 * R.BIG_HALF2 > 2 ** 32


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_changes_an_integer(variant):
    hit = []
    if variant in ("pair_int32", "pair_uint32"):                      # only a total beyond 32 bits can show these
        for kind in R.BIG_KINDS:
            _, _, _, pair2 = R.big_case(kind)
            if not np.array_equal(R.wrap(pair2, variant), pair2):
                hit.append(kind)
    else:
        for case in R.CASES:
            if case[1] > R.BLOCK + 1:                                 # the small sizes already tell the variants apart
                continue
            s, y, conf, pair2, flags = case_counts(case)
            conf_w, pair_w, _ = R.counts(s, y, case[2], variant=variant)
            if not (np.array_equal(conf_w, conf) and np.array_equal(pair_w, pair2)):
                hit.append(case)
    print(variant, "changes an integer on", len(hit), "case(s)")
    assert hit, f"no case tells the variant {variant} from the restatement"


def test_restatement_flags_and_exclusion():
    s, y = R.make_case("softmax", 40, 7)
    s, y = s.copy(), y.copy()
    s[3, 2], s[9, 0], y[17] = np.nan, np.inf, 7
    conf, pair2, flags = R.counts(s, y, 7)
    assert flags.tolist() == [2, 1]
    keep = np.ones(40, dtype=bool)
    keep[[3, 9, 17]] = False
    conf2, pair22, flags2 = R.counts(s[keep], y[keep], 7)
    assert flags2.tolist() == [0, 0] and np.array_equal(conf, conf2) and np.array_equal(pair2, pair22) and conf.sum() == 37
