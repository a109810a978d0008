"""A numpy restatement of the radiomic definitions that include/isic_hip_radiomics.h documents: test infrastructure for
csrc/radiomics.hip and ``isic_hip.radiomics``, written from the published PyRadiomics definitions (first-order, GLCM and
GLDM of the original image type, symmetrical GLCM at distance 1, GLDM alpha 0, fixed bin width, 2-D) and not from the kernel.

Two halves.  ``count_image`` counts the three integer matrices of every channel with array slices (int64, no tiles, no
atomics) in the header's layout.  ``features_from_counts`` turns them into the 56 features per channel in a floating type of
the caller's choice: ``numpy.float64`` is the reference, ``numpy.longdouble`` the same expressions with 11 more mantissa
bits, and the gap between the two measures what cancellation costs on that input (tests/test_radiomics_gpu.py).

MCC in ``longdouble``: numpy has no eigen-solver in that type.  The fp64 eigenvectors V of M (``numpy.linalg.eigh``) are
accurate to O(n eps); the Rayleigh quotient v' M v / v' v of a vector that is delta away from an eigenvector is delta^2 away
from its eigenvalue, so the quotients formed in ``longdouble`` from the ``longdouble`` M are its eigenvalues to about 1e-30."""
import numpy as np

EPS = 2.0 ** -52
LEVELS = 32
N_HIST, N_GLCM, N_GLDM = 256, 4 * LEVELS * LEVELS, LEVELS * 9
N_COUNTS = N_HIST + N_GLCM + N_GLDM
ANGLES = ((0, 1), (1, -1), (1, 0), (1, 1))
NEIGHBOURS = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))

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
N_FEATURES = len(FIRSTORDER) + len(GLCM) + len(GLDM)


def column(cls, name):
    """the column of a feature inside one channel's 56"""
    base = 0
    for c, names in CLASSES:
        if c == cls:
            return base + names.index(name)
        base += len(names)
    raise KeyError(cls)


# ---------------------------------------------------------------------------------------------- counting
def channels_of(image):
    """HWC uint8 RGB -> [4, H, W] int64: gray (OpenCV's 8-bit BGR2GRAY in integers), red, green, blue"""
    rgb = np.asarray(image).astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return np.stack([(4899 * r + 9617 * g + 1868 * b + 8192) >> 14, r, g, b])


def _shifted(h, w, dy, dx):
    """slices of the pixels p and of q = p + (dy, dx) for every p that has q inside the image"""
    ys, xs = slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx))
    yq, xq = slice(max(0, dy), h - max(0, -dy)), slice(max(0, dx), w - max(0, -dx))
    return (ys, xs), (yq, xq)


def count_channel(v, roi, bin_width):
    """one channel -> int64 [N_COUNTS]: hist[256], glcm[4][32][32], gldm[32][9]"""
    h, w = v.shape
    hist = np.bincount(v[roi], minlength=256)
    a = v // bin_width
    glcm = np.zeros((4, LEVELS, LEVELS), np.int64)
    for k, (dy, dx) in enumerate(ANGLES):
        P, Q = _shifted(h, w, dy, dx)
        both = roi[P] & roi[Q]
        ap, aq = a[P][both], a[Q][both]
        one_way = np.bincount(ap * LEVELS + aq, minlength=LEVELS * LEVELS).reshape(LEVELS, LEVELS)
        glcm[k] = one_way + one_way.T
    dep = np.zeros((h, w), np.int64)
    for dy, dx in NEIGHBOURS:
        P, Q = _shifted(h, w, dy, dx)
        dep[P] += roi[P] & roi[Q] & (a[P] == a[Q])
    gldm = np.bincount(a[roi] * 9 + dep[roi], minlength=LEVELS * 9)
    return np.concatenate([hist, glcm.reshape(-1), gldm])


def count_image(image, mask, bin_width=10, label=255):
    """-> int64 [4, N_COUNTS]"""
    roi = np.asarray(mask) == label
    return np.stack([count_channel(v, roi, bin_width) for v in channels_of(image)])


def split(counts):
    counts = np.asarray(counts)
    return (counts[:N_HIST], counts[N_HIST:N_HIST + N_GLCM].reshape(4, LEVELS, LEVELS),
            counts[N_HIST + N_GLCM:].reshape(LEVELS, 9))


# ---------------------------------------------------------------------------------------------- features
def percentile_linear(x_sorted, q, T=np.float64):
    """numpy.percentile(x, 100 q) by its 'linear' rule, spelled out: the virtual index (n - 1) q, its floor and
    fraction, and numpy's two-sided interpolation between the two order statistics"""
    n = len(x_sorted)
    q = T(q)
    vi = T(n - 1) * q
    lo = min(max(int(np.floor(vi)), 0), n - 1)
    hi = min(lo + 1, n - 1)
    g = vi - T(np.floor(vi))
    a, b = T(x_sorted[lo]), T(x_sorted[hi])
    d = b - a
    return b - d * (T(1) - g) if g >= T(0.5) else a + d * g


def _entropy(p, T):
    return -(p * np.log2(p + T(EPS))).sum()


def firstorder_features(hist, bin_width, T=np.float64):
    x = np.repeat(np.arange(256), hist)                            # the ROI values, ascending
    n = T(len(x))
    xv = x.astype(T)
    mean = xv.sum() / n
    c = xv - mean
    m2, m3, m4 = (c ** 2).sum() / n, (c ** 3).sum() / n, (c ** 4).sum() / n
    p10, p25, p50, p75, p90 = (percentile_linear(x, q, T) for q in (0.1, 0.25, 0.5, 0.75, 0.9))
    inner = xv[(xv >= p10) & (xv <= p90)]
    with np.errstate(invalid="ignore", divide="ignore"):         # no value inside [P10, P90]: 0 / 0 = NaN, as documented
        rmad = np.abs(inner - inner.sum() / T(len(inner))).sum() / T(len(inner))
    energy = (xv * xv).sum()
    binned = np.bincount(x // bin_width)
    p = binned[binned > 0].astype(T) / n
    zero = T(0)
    return np.array([p10, p90, energy, _entropy(p, T), p75 - p25, m4 / (m2 * m2) if m2 != 0 else zero, xv.max(),
                     np.abs(c).sum() / n, mean, p50, xv.min(), xv.max() - xv.min(),
                     rmad, np.sqrt(energy / n),
                     m3 / m2 ** T(1.5) if m2 != 0 else zero, energy, (p * p).sum(), m2], dtype=T)


def _second_largest_abs_eigenvalue(M, T):
    w, V = np.linalg.eigh(M.astype(np.float64))
    if T is not np.float64:
        V = V.astype(T)
        w = np.array([(V[:, k] @ (M @ V[:, k])) / (V[:, k] @ V[:, k]) for k in range(len(w))], dtype=T)
    return np.sort(np.abs(w))[-2]


def glcm_features(glcm, levels, Ng, T=np.float64):
    """``levels``: {absolute bin: gray level i} of the bins present in the ROI.  The mean over the angles that have a pair."""
    bins = np.array(sorted(levels))
    lev = np.array([levels[a] for a in bins]).astype(T)
    i, j = lev[:, None], lev[None, :]
    rows = []
    for k in range(4):
        C = glcm[k][np.ix_(bins, bins)].astype(T)
        S = C.sum()
        if S == 0:
            continue
        p = C / S
        px = p.sum(axis=1)
        ux = (i * p).sum()
        var = ((lev - ux) ** 2 * px).sum()
        sig = np.sqrt(var)
        kd = np.abs(i - j)
        pd = np.array([p[kd == d].sum() for d in range(Ng)], dtype=T)
        ks = np.arange(2, 2 * Ng + 1)
        ps = np.array([p[(i + j) == s].sum() for s in ks], dtype=T)
        kdv, ksv = np.arange(Ng).astype(T), ks.astype(T)
        pxy = px[:, None] * px[None, :]
        hx, hxy = _entropy(px, T), _entropy(p, T)
        hxy1 = -(p * np.log2(pxy + T(EPS))).sum()
        hxy2 = _entropy(pxy, T)
        da = (kdv * pd).sum()
        if len(bins) < 2:
            mcc = T(1)
        else:
            r = C.sum(axis=1)
            ok = r > 0
            M = np.zeros_like(C)
            M[np.ix_(ok, ok)] = C[np.ix_(ok, ok)] / np.sqrt(np.outer(r[ok], r[ok]))
            mcc = _second_largest_abs_eigenvalue(M, T)
        e = i + j - 2 * ux
        rows.append([
            (p * i * j).sum(), (e ** 4 * p).sum(), (e ** 3 * p).sum(), (e ** 2 * p).sum(), ((i - j) ** 2 * p).sum(),
            (p * (i - ux) * (j - ux)).sum() / (sig * sig) if var != 0 else T(1),
            da, _entropy(pd, T), ((kdv - da) ** 2 * pd).sum(),
            (pd / (1 + kdv)).sum(), (pd / (1 + kdv ** 2)).sum(), (pd / (1 + kdv ** 2 / T(Ng) ** 2)).sum(),
            (pd / (1 + kdv / T(Ng))).sum(),
            (hxy - hxy1) / hx if hx != 0 else T(0),
            np.sqrt(1 - np.exp(-2 * (hxy2 - hxy))) if hxy2 >= hxy else T(0),
            (pd[1:] / kdv[1:] ** 2).sum(),
            ux, (p * p).sum(), hxy, mcc, p.max(), (ksv * ps).sum(), _entropy(ps, T), var])
    if not rows:
        return np.full(len(GLCM), np.nan, dtype=T)
    return np.array(rows, dtype=T).sum(axis=0) / T(len(rows))


def gldm_features(gldm, levels, T=np.float64):
    bins = np.array(sorted(levels))
    P = gldm[bins].astype(T)
    Nz = P.sum()
    p = P / Nz
    i = np.array([levels[a] for a in bins]).astype(T)[:, None]
    j = np.arange(1, 10).astype(T)[None, :]
    mu_i, mu_j = (p * i).sum(), (p * j).sum()
    return np.array([
        _entropy(p, T), (P.sum(axis=0) ** 2).sum() / Nz, (P.sum(axis=0) ** 2).sum() / Nz ** 2, (p * (j - mu_j) ** 2).sum(),
        (P.sum(axis=1) ** 2).sum() / Nz, (p * (i - mu_i) ** 2).sum(), (P * i ** 2).sum() / Nz, (P * j ** 2).sum() / Nz,
        (P * i ** 2 * j ** 2).sum() / Nz, (P * j ** 2 / i ** 2).sum() / Nz, (P / i ** 2).sum() / Nz, (P / j ** 2).sum() / Nz,
        (P * i ** 2 / j ** 2).sum() / Nz, (P / (i ** 2 * j ** 2)).sum() / Nz], dtype=T)


def features_from_counts(counts, bin_width=10, T=np.float64):
    """int [N_COUNTS] of one channel -> [56] in ``T``; NaN without an ROI pixel"""
    hist, glcm, gldm = split(counts)
    if hist.sum() == 0:
        return np.full(N_FEATURES, np.nan, dtype=T)
    values = np.nonzero(hist)[0]
    lo = int(values.min()) // bin_width
    Ng = int(values.max()) // bin_width - lo + 1
    levels = {int(a): int(a) - lo + 1 for a in np.unique(values // bin_width)}
    return np.concatenate([firstorder_features(hist, bin_width, T), glcm_features(glcm, levels, Ng, T),
                           gldm_features(gldm, levels, T)])


def features_image(image, mask, bin_width=10, label=255, T=np.float64):
    """-> [4, 56] in ``T``"""
    return np.stack([features_from_counts(c, bin_width, T) for c in count_image(image, mask, bin_width, label)])


def tolerance(ref64, ref_ld):
    """what the device may differ from the fp64 restatement by, per feature: 1e-11 |ref| for a 1024-term fp64 sum (about
    1e-13) with margin for chained sums, logarithms and the Jacobi sweeps, plus 32 times the gap between the restatement in
    fp64 and in longdouble, which is what cancellation costs on this input"""
    gap = np.abs(ref64.astype(np.longdouble) - ref_ld).astype(np.float64)
    return 1e-11 * np.abs(ref64) + 32.0 * gap
