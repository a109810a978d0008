"""Radiomic features of the lesions of a resident image pool: the vector that ``radiomics_mlp``, the fusion branches and
``with_radiomic_node_features`` take, made on the device.

The reference extracts them with PyRadiomics (``RadiomicExtractor.py``, ``extract_radiomics.py``, ``params.yml``: label 255,
bin width 10, 2-D, symmetrical GLCM) from the gray, red, green and blue channel of every image inside its lesion mask.  Of
``params.yml``'s classes this module has the three that reduce, on uint8 images with a fixed bin width, to small integer
matrices counted in one pass over the pixels: ``firstorder`` (18 features), ``glcm`` (24) and ``gldm`` (14), on the original
image type -- 56 per channel, 224 per lesion.  ``shape2D``, ``glrlm``, ``glszm``, ``ngtdm`` and the filtered image types
(wavelet, LoG, square, ...) are not built; the names below leave room for them.

``isic_radiomics_u8`` (include/isic_hip_radiomics.h, csrc/radiomics.hip) does the work in one launch on an ``ImagePool``.
There is no CPU fallback.  PyRadiomics is not among this project's dependencies: parity is with a restatement of its
published definitions (tests/radiomics_ref.py), not with its output.
"""
from __future__ import annotations

import torch

from .lib import call

MAX_LEVELS = 32                     # ISIC_RADIOMICS_MAX_LEVELS: bin_width >= 8 on uint8
FEATURES = 56                       # ISIC_RADIOMICS_FEATURES, per channel
COUNTS = 4640                       # ISIC_RADIOMICS_COUNTS, per channel: hist[256], glcm[4][32][32], gldm[32][9]
TILE_H, TILE_W = 30, 62             # ISIC_RADIOMICS_TILE_H / _W: the kernel's LDS tile, for tests that must cross its seams
CHANNELS = ("gs", "red", "green", "blue")       # the suffixes of extract_radiomics.py:70, in the kernel's channel order
ANGLES = ((0, 1), (1, -1), (1, 0), (1, 1))      # (dy, dx) of glcm[k]

# PyRadiomics's order inside a class: that of its get<Name>FeatureValue methods, sorted
FIRSTORDER = ("10Percentile", "90Percentile", "Energy", "Entropy", "InterquartileRange", "Kurtosis", "Maximum",
              "MeanAbsoluteDeviation", "Mean", "Median", "Minimum", "Range", "RobustMeanAbsoluteDeviation", "RootMeanSquared",
              "Skewness", "TotalEnergy", "Uniformity", "Variance")
GLCM = ("Autocorrelation", "ClusterProminence", "ClusterShade", "ClusterTendency", "Contrast", "Correlation",
        "DifferenceAverage", "DifferenceEntropy", "DifferenceVariance", "Id", "Idm", "Idmn", "Idn", "Imc1", "Imc2",
        "InverseVariance", "JointAverage", "JointEnergy", "JointEntropy", "MCC", "MaximumProbability", "SumAverage",
        "SumEntropy", "SumSquares")
GLDM = ("DependenceEntropy", "DependenceNonUniformity", "DependenceNonUniformityNormalized", "DependenceVariance",
        "GrayLevelNonUniformity", "GrayLevelVariance", "HighGrayLevelEmphasis", "LargeDependenceEmphasis",
        "LargeDependenceHighGrayLevelEmphasis", "LargeDependenceLowGrayLevelEmphasis", "LowGrayLevelEmphasis",
        "SmallDependenceEmphasis", "SmallDependenceHighGrayLevelEmphasis", "SmallDependenceLowGrayLevelEmphasis")
CLASSES = (("firstorder", FIRSTORDER), ("glcm", GLCM), ("gldm", GLDM))


def feature_names(channels=CHANNELS):
    """``original_<class>_<Feature>_<channel>``: PyRadiomics's names with the suffix of ``extract_radiomics.py:70``,
    channel-major as the reference's ``pd.concat`` -- 56 per channel."""
    for ch in channels:
        if ch not in CHANNELS:
            raise ValueError(f"channel {ch!r}: one of {CHANNELS}")
    return [f"original_{cls}_{name}_{ch}" for ch in channels for cls, names in CLASSES for name in names]


def radiomic_features(pool, index=None, bin_width=10, label=255, return_counts=False):
    """-> fp64 ``[B, 224]`` on the pool's device, row ``b`` for pool image ``index[b]`` (all of them in order when ``index``
    is None), columns as ``feature_names()``.  An image without a pixel of ``mask == label`` gets a row of NaN.

    ``return_counts=True``: ``(features, counts int32 [B, 4, 4640], n_empty)`` -- the integer matrices behind the features
    in the layout of include/isic_hip_radiomics.h, and the number of rows without an ROI (a Python int: one synchronisation).
    ``ValueError`` for an index outside the pool, ``bin_width`` outside 8..255 or ``label`` outside 1..255."""
    if index is None:
        index = torch.arange(len(pool), dtype=torch.int64)
    index = torch.as_tensor(index, dtype=torch.int64).reshape(-1).cpu()
    B = index.numel()
    if B and (int(index.min()) < 0 or int(index.max()) >= len(pool)):
        raise ValueError(f"index outside the pool of {len(pool)} images")
    if not 8 <= int(bin_width) <= 255:
        raise ValueError(f"bin_width: 8..255 (at most {MAX_LEVELS} bins on uint8), got {bin_width}")
    if not 1 <= int(label) <= 255:
        raise ValueError(f"label: 1..255, got {label}")
    dev = pool.device
    out = torch.empty((B, len(CHANNELS) * FEATURES), device=dev, dtype=torch.float64)
    counts = torch.empty((B, len(CHANNELS), COUNTS), device=dev, dtype=torch.int32) if return_counts else None
    n_empty = torch.zeros(1, device=dev, dtype=torch.int64)
    call("isic_radiomics_u8", pool.pixels, pool.masks, pool.offsets, pool.hw, len(pool), index.to(dev), B, int(bin_width),
         int(label), out, counts, n_empty)
    if return_counts:
        return out, counts, int(n_empty.item())
    return out


def radiomics_frame(pool, index=None, bin_width=10, label=255, channels=CHANNELS):
    """A pandas frame of the features with ``feature_names(channels)`` as its columns, one row per chosen image: what
    ``DermDataset(df, radiomics)`` takes and what ``extract_radiomics.py`` pickles."""
    import pandas as pd
    names = feature_names(channels)
    feats = radiomic_features(pool, index, bin_width, label).cpu().numpy()
    frame = pd.DataFrame(feats, columns=feature_names())
    return frame[names] if tuple(channels) != CHANNELS else frame

