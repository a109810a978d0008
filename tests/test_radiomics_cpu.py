"""Radiomic features without a device: the names, the entry's declaration and its argument checks (which answer before any
device work), and the self-checks of the restatement (tests/radiomics_ref.py) that the GPU tests compare the kernel with.

The tests of the names, of the header and of the argument checks fail without the feature.  The self-checks of the
restatement (the 3 x 3 image worked by hand, the percentile rule against ``numpy.percentile``, the counting identities)
exercise only tests/radiomics_ref.py: they pin the definition, not the kernel."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import radiomics_ref as R  # noqa: E402
from isic_hip import lib  # noqa: E402

OK, BAD_ARG = 0, -1
P = 0x10000                      # a dummy non-NULL pointer: never dereferenced (errors come first)
NAME = "isic_radiomics_u8"
HEADER = "isic_hip_radiomics.h"


# ---------------------------------------------------------------------------------------------- names and the ABI
def test_feature_names():
    from isic_hip import radiomics as M
    names = M.feature_names()
    assert len(names) == 224 == len(set(names))
    for c, ch in enumerate(("gs", "red", "green", "blue")):
        block = names[56 * c:56 * (c + 1)]
        assert all(n.startswith("original_") and n.endswith("_" + ch) for n in block)
        classes = [n.split("_")[1] for n in block]
        assert classes == ["firstorder"] * 18 + ["glcm"] * 24 + ["gldm"] * 14
        for cls, lo, hi in (("firstorder", 0, 18), ("glcm", 18, 42), ("gldm", 42, 56)):
            feats = [n[len(f"original_{cls}_"):-len("_" + ch)] for n in block[lo:hi]]
            # PyRadiomics lists a class's features in the sorted order of its get<Name>FeatureValue methods
            assert feats == sorted(feats, key=lambda f: f"get{f}FeatureValue"), cls
    assert names[0] == "original_firstorder_10Percentile_gs" and names[-1].endswith("SmallDependenceLowGrayLevelEmphasis_blue")
    assert M.feature_names(("red",)) == names[56:112]
    with pytest.raises(ValueError):
        M.feature_names(("grey",))
    assert (M.FIRSTORDER, M.GLCM, M.GLDM) == (R.FIRSTORDER, R.GLCM, R.GLDM) and M.ANGLES == R.ANGLES


def test_entry_is_declared_in_the_new_header_exported_and_parsed():
    from isic_hip import build, radiomics as M
    inc = os.path.dirname(lib.header_path())
    assert f'#include "{HEADER}"' in open(os.path.join(inc, "isic_hip.h")).read()
    raw = open(os.path.join(inc, HEADER)).read()
    text = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == {NAME}
    assert os.path.join(inc, HEADER) in [os.path.normpath(p) for p in lib.extension_header_paths()]
    protos = lib.parse_header(os.path.join(inc, HEADER))
    assert [a[1] for a in protos[NAME][1]] == ["pixels", "masks", "offsets", "hw", "n_pool", "index", "B", "bin_width", "label",
                                              "out", "counts", "n_empty", "stream"]
    L = lib.lib()
    assert protos[NAME][0] is ctypes.c_int and NAME in L.extension and NAME not in L.public and NAME in L.fn
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), NAME)
    macros = dict(re.findall(r"#define (ISIC_RADIOMICS_\w+)\s+(\d+)", raw))
    assert {k: int(v) for k, v in macros.items()} == {
        "ISIC_RADIOMICS_MAX_LEVELS": M.MAX_LEVELS, "ISIC_RADIOMICS_FEATURES": M.FEATURES, "ISIC_RADIOMICS_COUNTS": M.COUNTS,
        "ISIC_RADIOMICS_TILE_H": M.TILE_H, "ISIC_RADIOMICS_TILE_W": M.TILE_W}
    assert (M.MAX_LEVELS, M.FEATURES, M.COUNTS) == (R.LEVELS, R.N_FEATURES, R.N_COUNTS) == (32, 56, 4640)
    assert HEADER in map(os.path.basename, build.header_deps())
    assert os.path.join(build.CSRC, "radiomics.hip") in build.sources()


def _entry(pixels=P, masks=P, offsets=P, hw=P, n_pool=3, index=P, B=2, bin_width=10, label=255, out=P, counts=None, n_empty=P):
    return lib.lib().fn[NAME](pixels, masks, offsets, hw, n_pool, index, B, bin_width, label, out, counts, n_empty, None)


def test_argument_checks_answer_without_a_device():
    for kw in (dict(pixels=None), dict(masks=None), dict(offsets=None), dict(hw=None), dict(index=None), dict(out=None),
               dict(n_empty=None), dict(n_pool=0), dict(n_pool=-1), dict(B=-1), dict(bin_width=7), dict(bin_width=0),
               dict(bin_width=-10), dict(bin_width=256), dict(label=0), dict(label=256), dict(label=-1)):
        assert _entry(**kw) == BAD_ARG, kw
    # B == 0 returns 0 without a launch, whatever the pointers; the scalar domains still hold
    assert _entry(B=0) == OK
    assert _entry(B=0, pixels=None, masks=None, offsets=None, hw=None, index=None, out=None, n_empty=None, n_pool=0) == OK
    assert _entry(B=0, bin_width=7) == BAD_ARG and _entry(B=0, label=0) == BAD_ARG
    assert _entry(B=0, bin_width=8) == OK and _entry(B=0, bin_width=255, label=1) == OK


def test_bin_of_a_byte_by_multiplication():
    """csrc/radiomics.hip forms v / bin_width as (v * m) >> 16 with m = 65536 / bin_width + 1: exact on the whole domain"""
    v = np.arange(256, dtype=np.int64)
    for bw in range(8, 256):
        assert np.array_equal((v * (65536 // bw + 1)) >> 16, v // bw), bw


# ---------------------------------------------------------------------------------------------- the restatement
HAND = np.array([[10, 11, 20],
                 [12, 21, 22],
                 [13, 14, 25]], dtype=np.uint8)          # bin width 10: levels 1 1 2 / 1 2 2 / 1 1 2


def _gray_image(v):
    return np.repeat(np.asarray(v, dtype=np.uint8)[:, :, None], 3, axis=2)


def test_gray_of_equal_channels_is_the_value_and_matches_the_fixed_point_weights():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    ch = R.channels_of(_gray_image(v))
    assert all(np.array_equal(ch[c], v) for c in range(4))
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (9, 7, 3), dtype=np.uint8)
    want = np.floor((0.299 * img[..., 0] + 0.587 * img[..., 1] + 0.114 * img[..., 2]) + 0.5)
    assert np.abs(R.channels_of(img)[0] - want).max() <= 1 and (R.channels_of(img)[1:] == img.transpose(2, 0, 1)).all()


def test_hand_worked_3x3_counts():
    counts = R.count_image(_gray_image(HAND), np.full((3, 3), 255, np.uint8), bin_width=10)
    assert all(np.array_equal(counts[0], counts[c]) for c in range(1, 4))
    hist, glcm, gldm = R.split(counts[0])
    assert hist.sum() == 9 and all(hist[v] == 1 for v in HAND.reshape(-1))
    want = {0: [[4, 3], [3, 2]], 1: [[2, 2], [2, 2]], 2: [[4, 2], [2, 4]], 3: [[2, 2], [2, 2]]}   # over bins 1, 2
    for k in range(4):
        assert glcm[k][1:3, 1:3].tolist() == want[k] and glcm[k].sum() == np.sum(want[k])
    dep = np.zeros((32, 9), np.int64)
    dep[1, 2], dep[1, 4], dep[2, 2], dep[2, 3] = 4, 1, 2, 2     # level 1: j = 3 four times, j = 5 once; level 2: 3, 3, 4, 4
    assert np.array_equal(gldm, dep)


@pytest.mark.parametrize("T", (np.float64, np.longdouble))
def test_hand_worked_3x3_features(T):
    f = R.features_image(_gray_image(HAND), np.full((3, 3), 255, np.uint8), bin_width=10, T=T)
    assert f.shape == (4, 56) and f.dtype == T and all(np.array_equal(f[0], f[c]) for c in range(1, 4))
    lit = {("glcm", "Contrast"): 11 / 24, ("glcm", "JointEnergy"): 25 / 96, ("glcm", "Idm"): 37 / 48,
           ("gldm", "SmallDependenceEmphasis"): 499 / 5400, ("firstorder", "Median"): 14.0,
           ("firstorder", "10Percentile"): 10.8, ("firstorder", "Minimum"): 10.0, ("firstorder", "Maximum"): 25.0,
           ("firstorder", "Energy"): float((HAND.astype(np.int64) ** 2).sum()), ("glcm", "JointAverage"): (17 / 12 + 1.5 * 3) / 4,
           ("gldm", "GrayLevelNonUniformity"): (25 + 16) / 9, ("gldm", "DependenceNonUniformity"): (36 + 4 + 1) / 9}
    for (cls, name), want in lit.items():
        got = float(f[0, R.column(cls, name)])
        assert abs(got - want) <= 1e-14 * abs(want), (cls, name, got, want)


def test_percentile_rule_is_numpys():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 9, 10, 11, 100, 101, 1000, 4097):
        x = np.sort(rng.integers(0, 256, n))
        for q in (0.1, 0.25, 0.5, 0.75, 0.9):
            assert R.percentile_linear(x, q) == np.percentile(x, 100 * q), (n, q)
    # and inside the first-order features, from the histogram
    x = rng.integers(3, 200, 777)
    f = R.firstorder_features(np.bincount(x, minlength=256), 10)
    assert f[R.FIRSTORDER.index("10Percentile")] == np.percentile(x, 10)
    assert f[R.FIRSTORDER.index("90Percentile")] == np.percentile(x, 90)
    assert f[R.FIRSTORDER.index("Median")] == np.median(x)
    assert f[R.FIRSTORDER.index("InterquartileRange")] == np.percentile(x, 75) - np.percentile(x, 25)
    np.testing.assert_allclose(f[R.FIRSTORDER.index("Variance")], np.var(x), rtol=1e-13)


def test_counting_identities_on_a_random_roi():
    """every angle's matrix is symmetric and sums to twice its pairs; the GLDM and the histogram hold every ROI pixel once;
    a mask byte other than the label is background"""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (23, 31, 3), dtype=np.uint8)
    mask = np.where(rng.random((23, 31)) < 0.6, 255, 0).astype(np.uint8)
    mask[rng.random((23, 31)) < 0.1] = 128
    counts = R.count_image(img, mask, bin_width=25)
    roi = mask == 255
    for c in range(4):
        hist, glcm, gldm = R.split(counts[c])
        assert hist.sum() == gldm.sum() == roi.sum()
        for k, (dy, dx) in enumerate(R.ANGLES):
            assert np.array_equal(glcm[k], glcm[k].T)
            pairs = sum(roi[y, x] and roi[y + dy, x + dx] for y in range(23 - dy) for x in range(max(0, -dx), 31 - max(0, dx)))
            assert glcm[k].sum() == 2 * pairs
        assert np.array_equal(gldm.sum(axis=1)[:11], np.bincount(np.arange(256) // 25, weights=hist).astype(np.int64))
    assert np.array_equal(R.count_image(img, np.where(mask == 128, 1, mask), 25), counts)


def test_special_values_of_the_restatement():
    full = lambda s: np.full(s, 255, np.uint8)
    # a constant image: one level
    f = R.features_image(_gray_image(np.full((5, 4), 77)), full((5, 4)))[0]
    g = lambda cls, name: float(f[R.column(cls, name)])
    assert g("glcm", "MCC") == 1.0 and g("glcm", "Correlation") == 1.0 and abs(g("glcm", "JointEntropy")) < 1e-15
    assert abs(g("firstorder", "Entropy")) < 1e-15 and g("firstorder", "Variance") == 0.0 and g("firstorder", "Kurtosis") == 0.0
    assert g("gldm", "DependenceNonUniformityNormalized") > 0
    # a checkerboard of two values: M has the eigenvalue -1
    yy, xx = np.mgrid[0:6, 0:6]
    f = R.features_image(_gray_image(np.where((yy + xx) % 2 == 0, 30, 90)), full((6, 6)))[0]
    assert abs(f[R.column("glcm", "MCC")] - 1.0) < 1e-14
    # one pixel: no pair in any angle
    f = R.features_image(_gray_image([[200]]), full((1, 1)))[0]
    assert np.isnan(f[18:42]).all() and not np.isnan(f[:18]).any() and not np.isnan(f[42:]).any()
    assert np.isnan(R.features_image(_gray_image([[200]]), np.zeros((1, 1), np.uint8))).all()


# ---------------------------------------------------------------------------------------------- the script's host side
def test_dermdataset_hands_out_the_whole_image_on_request(tmp_path):
    import pandas as pd
    from PIL import Image
    from dataset import DermDataset
    from isic_hip.augment import uint8_transform
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (12, 20, 3), dtype=np.uint8)
    mask = np.zeros((12, 20), np.uint8)
    mask[2:7, 11:19] = 255
    ip, sp = str(tmp_path / "img.png"), str(tmp_path / "seg.png")
    Image.fromarray(img).save(ip)
    Image.fromarray(mask).save(sp)
    df = pd.DataFrame([{"image_path": ip, "segmentation_path": sp, "dx": 1}])
    whole = DermDataset(df, None, transform=uint8_transform, crop=False)[0]
    assert np.array_equal(whole["image"].numpy(), img) and np.array_equal(whole["mask"].numpy(), mask)
    cropped = DermDataset(df, None, transform=uint8_transform)[0]                # today's behaviour: the square crop
    assert cropped["image"].shape == (12, 12, 3) and cropped["mask"].shape == (12, 12)
    assert whole["radiomics"].shape == (102,)


def test_extraction_script_arguments():
    import extract_radiomics as X
    a = X.parse_args([])
    assert (a.config_path, a.max_bytes, a.bin_width, a.label, a.synthetic, a.out) == ("config.yml", 1 << 30, 10, 255, 0, None)
    a = X.parse_args(["--synthetic", "7", "--max-bytes", "4096", "--out", "x.pkl", "--unknown-flag"])
    assert (a.synthetic, a.max_bytes, a.out) == (7, 4096, "x.pkl")
