"""The device PCA's restatement and bounds (tests/pca_ref.py) checked without a device: the restatement equals sklearn on
float64 input, the input families meet their gap / margin conditions, the bounds admit a plain fp32 evaluation and reject
every wrong variant, and the C entries check their arguments before any device work."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pca_ref as R  # noqa: E402
from isic_hip import lib  # noqa: E402

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x1000                       # a dummy, 16-byte aligned, non-NULL pointer: never dereferenced (errors come first)

case = R.fit_case


@pytest.mark.parametrize("M,D", R.FIT_SHAPES + ((2, 8),))
def test_restatement_equals_sklearn_on_float64(M, D):
    from sklearn.decomposition import PCA
    x = R.family(M, D).astype(np.float64)
    ref = R.fit_eval(x)
    sk = PCA(n_components=0.90).fit(x)
    assert ref["k"] == sk.n_components_
    scale = ref["eigenvalues"][0]
    assert np.abs(ref["explained_variance"] - sk.explained_variance_).max() <= 1e-9 * scale
    assert np.abs(ref["components"] - sk.components_).max() <= 1e-9
    assert np.abs(ref["mean"] - sk.mean_).max() <= 1e-9 * np.abs(sk.mean_).max()
    t = R.transform_eval(x, ref["components"], ref["mean"])
    assert np.abs(t - sk.transform(x)).max() <= 1e-9 * np.sqrt(scale) * 10
    if M <= 3:
        return
    ri = R.fit_eval(x, n_components=3)
    assert ri["k"] == 3 and np.abs(ri["components"] - PCA(n_components=3).fit(x).components_).max() <= 1e-9


@pytest.mark.parametrize("with_rows", (False, True))
@pytest.mark.parametrize("M,D", R.FIT_SHAPES)
def test_families_meet_their_conditions_and_no_component_is_left_out(M, D, with_rows):
    x, rows, ref = case(M, D, with_rows)
    gap, margin = R.conditions(ref)
    print(f"family ({M}, {D}, rows={with_rows}): k {ref['k']}, min gap {gap:.2e} lambda_1, margin {margin:.2e}")
    assert gap >= 1e-3 and margin >= 1e-4
    b = R.fit_bounds(x, rows, ref)
    assert b["checked"].all(), b["components"]


@pytest.mark.parametrize("with_rows", (False, True))
@pytest.mark.parametrize("M,D", R.DEVICE_FIT_SHAPES)
def test_bounds_admit_a_plain_fp32_fit_and_transform(M, D, with_rows):
    x, rows, ref = case(M, D, with_rows)
    got = R.fit_eval(x, rows, dtype=np.float32)
    r = R.fit_ratios(got, ref, R.fit_bounds(x, rows, ref))
    print(f"fp32 numpy fit ({M}, {D}, rows={with_rows}): error / bound {r}")
    assert R.worst(r) <= 1.0
    c32, m32 = ref["components"].astype(np.float32), ref["mean"].astype(np.float32)
    t = R.transform_eval(x, c32, m32, rows, dtype=np.float32)
    assert R.ratio(t, R.transform_eval(x, c32, m32, rows), R.transform_bound(x, c32, m32, rows)) <= 1.0


GRAM_CASES = [(M, D) for D in R.GRAM_D for M in R.GRAM_M] + [(M, 64) for M in R.GRAM_RUN_M]


@pytest.mark.parametrize("M,D", GRAM_CASES)
def test_bounds_admit_a_plain_fp32_gram(M, D):
    x = R.family(M, D)
    shift = x[: max(1, M // 2)].astype(np.float64).mean(axis=0).astype(np.float32)
    G, cs = R.gram_eval(x, None, shift)
    G32, cs32 = R.gram_eval(x, None, shift, dtype=np.float32)
    EG, Ec = R.gram_bound(x, None, shift)
    assert R.ratio(G32, G, EG) <= 1.0 and R.ratio(cs32, cs, Ec) <= 1.0


def test_gram_bounds_reject_the_wrong_variants():
    M, D = 2 * R.RUN + 3, 64
    x, rows = R.family(M, D), R.rows_for(2 * R.RUN + 3)
    shift = x.astype(np.float64).mean(axis=0).astype(np.float32)
    for bug in ("uncentred", "rows_ignored", "last_run_dropped", "not_mirrored"):
        use = rows if bug == "rows_ignored" else None
        G, cs = R.gram_eval(x, use, shift)
        Gb, csb = R.gram_eval(x, use, shift, bug=bug)
        EG, Ec = R.gram_bound(x, use, shift)
        assert R.ratio(Gb, G, EG) > 1.0, bug
        if bug != "not_mirrored":
            assert R.ratio(csb, cs, Ec) > 1.0, bug


@pytest.mark.parametrize("bug", ("uncentred", "rows_ignored", "last_run_dropped", "not_mirrored", "divisor_m", "sign_first"))
def test_fit_bounds_reject_the_wrong_variants(bug):
    """on the small shapes (a divisor M instead of M - 1 is a relative 1 / M: inside the bounds at M = 5000, far outside
    at M = 40 and 65), with a row index (so that ignoring it matters)"""
    for M, D in ((40, 64), (65, 64)):
        x, rows, ref = case(M, D, True)
        got = R.fit_eval(x, rows, bug=bug)
        assert R.worst(R.fit_ratios(got, ref, R.fit_bounds(x, rows, ref))) > 1.0, (bug, M, D)


def test_side_left_changes_the_component_count_where_the_ratio_is_met_exactly():
    """side="left" and side="right" differ only where the cumulative ratio EQUALS n_components: asked for exactly the
    ratio the first j components explain, sklearn's rule keeps j + 1"""
    x, _, ref = case(300, 64, False)
    cum = np.cumsum(ref["eigenvalues"] / ref["eigenvalues"].sum())
    j = 4
    right = R.fit_eval(x, n_components=float(cum[j]))
    left = R.fit_eval(x, n_components=float(cum[j]), bug="side_left")
    assert right["k"] == j + 2 and left["k"] == j + 1
    assert R.fit_ratios(left, right, R.fit_bounds(x, None, right))["k"] > 1.0


def test_gap_independent_checks_admit_fp32_and_reject_wrong_outputs():
    """R.output_checks (what the end-to-end device test asserts on an encoder's latents): a family member fitted and
    transformed in plain fp32 around the first batch's mean is admitted, with further rows that were only transformed;
    rejected are a fit that dropped its last run, an output scaled by 0.1 %, and outputs whose rows are permuted (fitted
    rows: the reconstruction residual; transformed-only rows: the recovered map)"""
    x, _, _ = case(300, 64, False)
    xt = R.family(120, 64, seed=9)
    first = np.arange(300) < 100
    shift = x[first].astype(np.float64).mean(axis=0).astype(np.float32)
    fit = R.fit_eval(x, dtype=np.float32, shift=shift)
    c32, m32 = fit["components"].astype(np.float32), fit["mean"].astype(np.float32)
    t = R.transform_eval(x, c32, m32, dtype=np.float32)
    tt = R.transform_eval(xt, c32, m32, dtype=np.float32)
    k_ok, ra, rb, rc = R.output_checks(x, t, first, xt, tt)
    print(f"fp32 numpy output checks: covariance {ra:.3e} residual {rb:.3e} transformed-only rows {rc:.3e}")
    assert k_ok and ra <= 1.0 and rb <= 1.0 and rc <= 1.0
    perm = np.random.default_rng(3).permutation(300)
    _, ra, rb, _ = R.output_checks(x, t[perm], first)
    assert ra <= 1.0 and rb > 1.0                             # the covariance cannot see the order of the rows, the residual does
    _, _, _, rc = R.output_checks(x, t, first, xt, tt[np.random.default_rng(4).permutation(120)])
    assert rc > 1.0
    _, ra, _, _ = R.output_checks(x, t[:, ::-1] * 1.001, first)                     # columns scaled by 0.1 %
    assert ra > 1.0
    xl = np.concatenate([x] * 8)                              # 2400 rows: two runs, the second one dropped from the fit
    fl = np.arange(2400) < 100
    tl = {}
    for bug in (None, "last_run_dropped"):
        f = R.fit_eval(xl, dtype=np.float32, shift=shift, bug=bug)
        tl[bug] = R.transform_eval(xl, f["components"].astype(np.float32), f["mean"].astype(np.float32), dtype=np.float32)
    k_ok, ra, rb, _ = R.output_checks(xl, tl[None], fl)
    assert k_ok and ra <= 1.0 and rb <= 1.0
    k_ok, ra, rb, _ = R.output_checks(xl, tl["last_run_dropped"], fl)
    assert not (k_ok and ra <= 1.0 and rb <= 1.0)


def test_entry_points_are_declared_and_exported():
    L = lib.lib()
    inc = os.path.dirname(lib.header_path())
    assert '#include "isic_hip_pca.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    assert os.path.join(inc, "isic_hip_pca.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    for name in ("isic_gram_shifted_f32_workspace_bytes", "isic_gram_shifted_f32"):
        assert name in L.extension and name in L.fn, name
    assert L.fn["isic_abi_version"]() == 1
    assert f"#define ISIC_GRAM_RUN {R.RUN}\n" in open(os.path.join(inc, "isic_hip_pca.h")).read()


def test_argument_checks_without_a_device():
    L = lib.lib().fn
    q, g = L["isic_gram_shifted_f32_workspace_bytes"], L["isic_gram_shifted_f32"]
    big = 1 << 40
    assert q(100, 1028) == 0 and q(100, 6) == 0 and q(-1, 64) == 0 and q(0, 64) == 0
    need = q(5000, 64)
    assert need >= 3 * (128 * 128 + 128) * 4                                   # three runs of one tile pair
    assert q(1 << 22, 768) == q(1 << 23, 768) > 0                              # bounded: stops growing with M
    assert g(P, 100, 1028, 1028, None, None, P, P, 0.0, P, big, None) == UNSUPPORTED      # D > 1024
    assert g(P, 100, 6, 8, None, None, P, P, 0.0, P, big, None) == UNSUPPORTED            # D % 4
    assert g(P, 100, 0, 8, None, None, P, P, 0.0, P, big, None) == BAD_ARG                # D <= 0
    assert g(P, 100, 64, 60, None, None, P, P, 0.0, P, big, None) == UNSUPPORTED          # ldx < D
    assert g(P, 100, 64, 66, None, None, P, P, 0.0, P, big, None) == UNSUPPORTED          # ldx % 4
    assert g(P + 4, 100, 64, 64, None, None, P, P, 0.0, P, big, None) == UNSUPPORTED      # X not 16-byte aligned
    assert g(P, 100, 64, 64, None, P + 4, P, P, 0.0, P, big, None) == UNSUPPORTED         # shift not 16-byte aligned
    assert g(P, 5000, 64, 64, None, None, P, P, 0.0, P, need - 1, None) == WORKSPACE      # short workspace
    assert g(P, 5000, 64, 64, None, None, P, P, 0.0, None, 0, None) == WORKSPACE
    assert g(P, 100, 64, 64, None, None, P, P, 0.5, P, big, None) == BAD_ARG              # beta not in {0, 1}
    assert g(P, 100, 64, 64, None, None, None, P, 0.0, P, big, None) == BAD_ARG           # no G
    assert g(P, 100, 64, 64, None, None, P, None, 0.0, P, big, None) == BAD_ARG           # no colsum
    assert g(None, 100, 64, 64, None, None, P, P, 0.0, P, big, None) == BAD_ARG           # no X with M > 0
    assert g(P, -1, 64, 64, None, None, P, P, 0.0, P, big, None) == BAD_ARG               # negative M
    assert g(None, 0, 64, 64, None, None, P, P, 1.0, None, 0, None) == 0                  # M == 0, beta == 1: nothing to do


def test_device_pca_rejects_cpu_tensors_and_bad_options():
    import torch
    from isic_hip.lib import IsicHipError
    from isic_hip.pca import DevicePCA
    with pytest.raises(IsicHipError):
        DevicePCA().partial_fit(torch.zeros(8, 4))
    with pytest.raises(IsicHipError):
        DevicePCA().transform(torch.zeros(8, 4))
    for bad in (0.0, 1.0, 1.5, 0, -2, "mle"):
        with pytest.raises(ValueError):
            DevicePCA(bad)
    with pytest.raises(ValueError):
        DevicePCA().finalize()                                                 # no samples: M < 2
