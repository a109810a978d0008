"""Radiomic features on the MI355X: ``isic_radiomics_u8`` through the ABI and ``isic_hip.radiomics``.

Every case is held to two yardsticks.  The integer matrices (``counts``) must equal numpy's integer counting
(tests/radiomics_ref.py: ``count_image``) bit for bit.  The features must lie within ``radiomics_ref.tolerance`` of the fp64
restatement: 1e-11 |ref| plus 32 times the gap between the restatement in fp64 and in ``numpy.longdouble`` on that input;
NaN exactly where the restatement has NaN.  All cases live in ONE ragged pool that is uploaded, counted and restated once per
bin width; the tests read from that.

Largest error / tolerance seen on the MI355X: 0.065 (bin width 10, the 130 x 257 image), 0.013 at width 8, 0.024 at width 25
(the test prints it; DESIGN.md, "Radiomic features")."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import radiomics_ref as R  # noqa: E402
from isic_hip import radiomics as M  # noqa: E402
from isic_hip.augment import ImagePool  # noqa: E402
from isic_hip.lib import IsicHipError, call  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAD_ARG = -1
SENTINEL = -777.25


# ---------------------------------------------------------------------------------------------- the cases
def _gray(v):
    return np.repeat(np.asarray(v, dtype=np.uint8)[:, :, None], 3, axis=2)


def _full(h, w):
    return np.full((h, w), 255, np.uint8)


def _derm_like(h, w, seed):
    """the recipe of SyntheticDermPixels at a chosen size: a smooth tinted gradient plus noise under an elliptic lesion"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(yy * 255) // max(h - 1, 1), (xx * 255) // max(w - 1, 1), np.full((h, w), 40 * (seed % 7))], axis=2)
    img = np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)
    cy, cx = rng.random(2) * 0.2 + 0.4
    mask = ((((yy - cy * h) / (0.45 * h)) ** 2 + ((xx - cx * w) / (0.45 * w)) ** 2) <= 1.0).astype(np.uint8) * 255
    return img, mask


def _cases():
    rng = np.random.default_rng(2024)
    rnd = lambda h, w, lo=0, hi=256: rng.integers(lo, hi, (h, w, 3)).astype(np.uint8)
    c = {}
    c["one_pixel"] = (rnd(1, 1), _full(1, 1))
    c["two_pixels"] = (_gray([[50, 51]]), _full(1, 2))           # no value inside [P10, P90] = [50.1, 50.9]
    c["row_1x7"] = (rnd(1, 7), _full(1, 7))
    c["column_9x1"] = (rnd(9, 1), _full(9, 1))
    c["full_3x3"] = (rnd(3, 3), _full(3, 3))
    c["constant"] = (_gray(np.full((12, 9), 77)), _full(12, 9))
    yy, xx = np.mgrid[0:6, 0:6]
    c["checkerboard"] = (_gray(np.where((yy + xx) % 2 == 0, 30, 90)), _full(6, 6))
    c["only_0_and_255"] = ((rng.integers(0, 2, (10, 13, 3)) * 255).astype(np.uint8), _full(10, 13))
    img = rnd(11, 14, 37, 200)
    img[4, 5] = 37                                               # the minimum of every channel, gray included
    c["minimum_37"] = (img, _full(11, 14))
    mask = np.where(rng.random((15, 12)) < 0.5, 255, 0).astype(np.uint8)
    mask[rng.random((15, 12)) < 0.2] = 128
    mask[rng.random((15, 12)) < 0.2] = 1
    mask[7, 6] = 255
    c["other_mask_bytes"] = (rnd(15, 12), mask)
    yy, xx = np.mgrid[0:40, 0:70]
    ell = ((((yy - 19.5) / 20.0) ** 2 + ((xx - 34.5) / 35.0) ** 2) <= 1.0)
    assert ell[0].any() and ell[-1].any() and ell[:, 0].any() and ell[:, -1].any() and not ell.all()
    c["ellipse_on_borders"] = (_derm_like(40, 70, 3)[0], ell.astype(np.uint8) * 255)
    c["empty_mask"] = (rnd(8, 8), np.zeros((8, 8), np.uint8))
    for k, (h, w) in enumerate(((17, 33), (67, 131), (300, 5), (130, 257))):
        c[f"derm_{h}x{w}"] = _derm_like(h, w, 10 + k)
    return c


CASES = _cases()
NAMES = list(CASES)
RAGGED = [n for n in NAMES if n.startswith("derm_")]
BIN_WIDTHS = {10: NAMES, 8: RAGGED + ["only_0_and_255", "minimum_37"], 25: RAGGED + ["other_mask_bytes", "full_3x3"]}


class _State:
    pass


@pytest.fixture(scope="module")
def S():
    """the pool, one launch per bin width over the images that width is checked on, and the restatement of each, once"""
    s = _State()
    s.pool = ImagePool.from_arrays([CASES[n] for n in NAMES], DEV)
    s.feats, s.counts, s.n_empty, s.ref_counts, s.ref64, s.refld = {}, {}, {}, {}, {}, {}
    for bw, names in BIN_WIDTHS.items():
        idx = [NAMES.index(n) for n in names]
        f, c, e = M.radiomic_features(s.pool, idx, bin_width=bw, return_counts=True)
        s.feats[bw], s.counts[bw], s.n_empty[bw] = f.cpu().numpy(), c.cpu().numpy(), e
        for n in names:
            rc = R.count_image(*CASES[n], bin_width=bw)
            s.ref_counts[bw, n] = rc
            s.ref64[bw, n] = np.stack([R.features_from_counts(x, bw, np.float64) for x in rc])
            s.refld[bw, n] = np.stack([R.features_from_counts(x, bw, np.longdouble) for x in rc])
    return s


def _row(s, bw, name):
    b = BIN_WIDTHS[bw].index(name)
    return s.feats[bw][b].reshape(4, 56), s.counts[bw][b]


def _check(got, ref64, refld, what):
    """-> the largest error / tolerance of the finite features"""
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN pattern")
    tol = R.tolerance(ref64, refld)
    err = np.abs(got - ref64)
    ok = nan | (err <= tol)
    if not ok.all():
        ch, f = (int(v[0]) for v in np.nonzero(~ok))
        names = M.feature_names()
        pytest.fail(f"{what}: {names[56 * ch + f]}: got {got[ch, f]!r}, restatement {ref64[ch, f]!r}, error {err[ch, f]:.3e} "
                    f"above {tol[ch, f]:.3e}; {int((~ok).sum())} feature(s) outside")
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(nan | (err == 0), 0.0, err / tol)
    return float(ratio.max())


def _f(row, cls, name, ch=0):
    return float(row[ch, R.column(cls, name)])


# ---------------------------------------------------------------------------------------------- counts and features
@pytest.mark.parametrize("bw", sorted(BIN_WIDTHS))
def test_counts_are_numpys_bit_for_bit(S, bw):
    for n in BIN_WIDTHS[bw]:
        _, counts = _row(S, bw, n)
        assert counts.dtype == np.int32 and counts.shape == (4, M.COUNTS)
        ref = S.ref_counts[bw, n]
        if not np.array_equal(counts, ref):
            ch, i = (int(v[0]) for v in np.nonzero(counts != ref))
            pytest.fail(f"{n}, bin width {bw}: channel {ch} counter {i}: {counts[ch, i]} != {ref[ch, i]}; "
                        f"{int((counts != ref).sum())} counter(s) differ")


@pytest.mark.parametrize("bw", sorted(BIN_WIDTHS))
def test_features_within_the_tolerance_of_the_restatement(S, bw):
    worst = {}
    for n in BIN_WIDTHS[bw]:
        row, _ = _row(S, bw, n)
        worst[n] = _check(row, S.ref64[bw, n], S.refld[bw, n], f"{n}, bin width {bw}")
    print(f"bin width {bw}: largest error / tolerance {max(worst.values()):.4f} ({max(worst, key=worst.get)})")
    assert S.n_empty[bw] == sum(n == "empty_mask" for n in BIN_WIDTHS[bw])


def test_tile_seams_are_crossed():
    sizes = [CASES[n][0].shape[:2] for n in RAGGED]
    assert sizes == [(17, 33), (67, 131), (300, 5), (130, 257)]
    assert any(w > M.TILE_W for _, w in sizes) and any(h > M.TILE_H for h, _ in sizes)
    assert any(w > 2 * M.TILE_W and h > 2 * M.TILE_H for h, w in sizes)          # a tile with neighbours on every side
    assert any(w < M.TILE_W and h % M.TILE_H for h, w in sizes)


def test_one_pixel(S):
    row, counts = _row(S, 10, "one_pixel")
    assert np.isnan(row[:, 18:42]).all() and not np.isnan(row[:, :18]).any() and not np.isnan(row[:, 42:]).any()
    img = CASES["one_pixel"][0]
    for ch, v in enumerate(R.channels_of(img)[:, 0, 0]):
        hist, glcm, gldm = R.split(counts[ch])
        assert hist[v] == 1 and hist.sum() == 1 and not glcm.any()
        assert gldm[v // 10, 0] == 1 and gldm.sum() == 1                        # level 1, dependence 1
        assert _f(row, "firstorder", "Mean", ch) == v == _f(row, "firstorder", "Median", ch)
        assert _f(row, "firstorder", "Variance", ch) == 0.0 and _f(row, "gldm", "SmallDependenceEmphasis", ch) == 1.0


def test_two_pixels_have_no_value_between_their_percentiles(S):
    """the documented NaN of the robust deviation, and of nothing else"""
    row, _ = _row(S, 10, "two_pixels")
    k = R.column("firstorder", "RobustMeanAbsoluteDeviation")
    assert np.isnan(row[:, k]).all() and np.isnan(row).sum() == 4
    assert _f(row, "firstorder", "10Percentile") == 50.1 and _f(row, "firstorder", "90Percentile") == 50.9


def test_constant_image(S):
    row, _ = _row(S, 10, "constant")
    for ch in range(4):
        assert _f(row, "glcm", "MCC", ch) == 1.0 and _f(row, "glcm", "Correlation", ch) == 1.0
        for cls, name in (("firstorder", "Entropy"), ("glcm", "JointEntropy"), ("glcm", "SumEntropy"),
                          ("glcm", "DifferenceEntropy")):
            assert abs(_f(row, cls, name, ch)) < 1e-15, name
        assert _f(row, "firstorder", "Variance", ch) == 0.0 and _f(row, "firstorder", "Uniformity", ch) == 1.0
        assert _f(row, "glcm", "JointAverage", ch) == 1.0                        # Ng = 1: the one level is 1


def test_checkerboard_mcc_is_one(S):
    row, _ = _row(S, 10, "checkerboard")
    assert all(abs(_f(row, "glcm", "MCC", ch) - 1.0) < 1e-14 for ch in range(4))


def test_two_levels_out_of_26_and_the_level_offset(S):
    row, counts = _row(S, 10, "only_0_and_255")
    for ch in range(1, 4):                                                      # the colour channels hold 0 and 255 only
        hist, _, gldm = R.split(counts[ch])
        assert set(np.nonzero(hist)[0]) == {0, 255} and set(np.nonzero(gldm.sum(axis=1))[0]) == {0, 25}
        assert _f(row, "firstorder", "Range", ch) == 255.0
        assert 2.0 < _f(row, "glcm", "SumAverage", ch) < 52.0                    # i, j in {1, 26}
    row, counts = _row(S, 10, "minimum_37")
    for ch in range(4):
        assert _f(row, "firstorder", "Minimum", ch) == 37.0
        assert np.nonzero(R.split(counts[ch])[2].sum(axis=1))[0].min() == 3      # absolute bin 3 is level 1
        assert 1.0 <= _f(row, "glcm", "JointAverage", ch) <= 17.0


def test_other_mask_bytes_are_background(S):
    img, mask = CASES["other_mask_bytes"]
    assert (mask == 128).any() and (mask == 1).any()
    _, counts = _row(S, 10, "other_mask_bytes")
    assert R.split(counts[0])[0].sum() == (mask == 255).sum()
    pool = ImagePool.from_arrays([(img, np.where(mask == 255, 255, 0).astype(np.uint8))], DEV)
    f, c, _ = M.radiomic_features(pool, return_counts=True)
    b = NAMES.index("other_mask_bytes")
    assert np.array_equal(c.cpu().numpy()[0], S.counts[10][b])
    assert np.array_equal(f.cpu().numpy().view(np.uint64)[0], S.feats[10][b].view(np.uint64))
    # another label: the pixels of byte 128 are the ROI now
    f128, c128, e = M.radiomic_features(S.pool, [b], label=128, return_counts=True)
    assert e == 0 and np.array_equal(c128.cpu().numpy()[0], R.count_image(img, mask, 10, label=128))


def test_empty_mask_gives_a_nan_row_and_touches_nothing_else(S):
    b = NAMES.index("empty_mask")
    assert np.isnan(S.feats[10][b]).all() and not S.counts[10][b].any() and S.n_empty[10] == 1
    for nb in (b - 1, b + 1):
        assert not np.isnan(S.feats[10][nb][:18]).any()
    # through the ABI: one row in the middle of a buffer, the counter is added to
    pool = S.pool
    out = torch.full((3, 224), SENTINEL, device=DEV, dtype=torch.float64)
    n_empty = torch.full((1,), 5, device=DEV, dtype=torch.int64)
    call("isic_radiomics_u8", pool.pixels, pool.masks, pool.offsets, pool.hw, len(pool),
         torch.tensor([b], device=DEV), 1, 10, 255, out[1:2], None, n_empty)
    out = out.cpu().numpy()
    assert (out[0] == SENTINEL).all() and (out[2] == SENTINEL).all() and np.isnan(out[1]).all() and int(n_empty) == 6
    call("isic_radiomics_u8", pool.pixels, pool.masks, pool.offsets, pool.hw, len(pool),
         torch.tensor([b, 0, b], device=DEV), 3, 10, 255, torch.empty((3, 224), device=DEV, dtype=torch.float64), None, n_empty)
    assert int(n_empty) == 8


def test_index_subset_permuted_and_repeated(S):
    pick = [NAMES.index(n) for n in ("derm_67x131", "full_3x3", "derm_67x131", "ellipse_on_borders", "one_pixel", "empty_mask")]
    f, c, e = M.radiomic_features(S.pool, pick, return_counts=True)
    f, c = f.cpu().numpy(), c.cpu().numpy()
    assert e == 1 and f.shape == (6, 224)
    for row, b in enumerate(pick):
        f1, c1, _ = M.radiomic_features(S.pool, [b], return_counts=True)
        assert np.array_equal(f[row].view(np.uint64), f1.cpu().numpy()[0].view(np.uint64)), NAMES[b]
        assert np.array_equal(c[row], c1.cpu().numpy()[0])
        assert np.array_equal(f[row].view(np.uint64), S.feats[10][b].view(np.uint64))
    none = M.radiomic_features(S.pool, [])
    assert none.shape == (0, 224) and none.dtype == torch.float64


def test_two_identical_calls_give_identical_bits(S):
    a = M.radiomic_features(S.pool).cpu().numpy()
    b = M.radiomic_features(S.pool).cpu().numpy()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert np.array_equal(a.view(np.uint64), S.feats[10].view(np.uint64))


def test_bad_arguments(S):
    pool = S.pool
    out = torch.empty((2, 224), device=DEV, dtype=torch.float64)
    n_empty = torch.zeros(1, device=DEV, dtype=torch.int64)
    idx = torch.tensor([0, 1], device=DEV)
    good = dict(pixels=pool.pixels, masks=pool.masks, offsets=pool.offsets, hw=pool.hw, n_pool=len(pool), index=idx, B=2,
                bin_width=10, label=255, out=out, counts=None, n_empty=n_empty)
    call("isic_radiomics_u8", *good.values())
    for kw in (dict(pixels=None), dict(masks=None), dict(offsets=None), dict(hw=None), dict(index=None), dict(out=None),
               dict(n_empty=None), dict(n_pool=0), dict(B=-1), dict(bin_width=7), dict(bin_width=256), dict(label=0),
               dict(label=256)):
        with pytest.raises(IsicHipError) as ei:
            call("isic_radiomics_u8", *{**good, **kw}.values())
        assert ei.value.code == BAD_ARG, kw
    for bad in ([len(pool)], [-1], [0, 99]):
        with pytest.raises(ValueError):
            M.radiomic_features(pool, bad)
    for kw in (dict(bin_width=7), dict(bin_width=256), dict(label=0), dict(label=256)):
        with pytest.raises(ValueError):
            M.radiomic_features(pool, [0], **kw)


# ---------------------------------------------------------------------------------------------- the frame
def test_frame_columns_and_dermdataset(S, tmp_path):
    import pandas as pd
    from PIL import Image
    from dataset import DermDataset
    pick = [NAMES.index("derm_17x33"), NAMES.index("full_3x3")]
    frame = M.radiomics_frame(S.pool, pick)
    assert list(frame.columns) == M.feature_names() and frame.shape == (2, 224)
    assert np.array_equal(np.ascontiguousarray(frame.to_numpy()).view(np.uint64), S.feats[10][pick].view(np.uint64))
    assert list(M.radiomics_frame(S.pool, pick, channels=("green", "gs")).columns) == M.feature_names(("green", "gs"))
    rows = []
    for k, b in enumerate(pick):
        img, mask = CASES[NAMES[b]]
        ip, sp = str(tmp_path / f"img_{k}.png"), str(tmp_path / f"seg_{k}.png")
        Image.fromarray(img).save(ip)
        Image.fromarray(mask).save(sp)
        rows.append({"image_path": ip, "segmentation_path": sp, "dx": k})
    ds = DermDataset(pd.DataFrame(rows), frame)
    for k in range(2):
        rad = ds[k]["radiomics"]
        assert rad.shape == (224,) and rad.dtype == torch.float32
        assert torch.equal(rad, torch.from_numpy(frame.values[k].astype(np.float32)))


def test_extraction_script_on_synthetic_images(tmp_path):
    """``extract_radiomics.py --synthetic``: the frame of a chunked extraction equals the one-pool frame, row for row"""
    import pandas as pd
    import extract_radiomics as X
    from isic_hip.augment import SyntheticDermPixels
    ds = SyntheticDermPixels(5, size=(24, 40))
    out = str(tmp_path / "rad.pkl")
    frame = X.main(["--synthetic", "5", "--out", out])
    assert frame.shape == (5, 224) and list(frame.columns) == M.feature_names()
    assert frame.iloc[4].isna().all() and not frame.iloc[:4].isna().any().any()          # every fifth image has no mask
    assert pd.read_pickle(out).equals(frame)
    whole = X.extract(ds, DEV)
    chunked = X.extract(ds, DEV, max_bytes=2 * 4 * 24 * 40)                               # two images per pool
    assert whole.shape == (5, 224) and chunked.equals(whole)
    with pytest.raises(ValueError):
        X.extract(ds, DEV, max_bytes=4 * 24 * 40 - 1)
    args = X.parse_args(["--config_path", "other.yml", "--max-bytes", "1000"])
    assert (args.config_path, args.max_bytes, args.bin_width, args.label, args.synthetic) == ("other.yml", 1000, 10, 255, 0)
