/* libisic_hip.so -- radiomic features of the lesions of a resident uint8 image pool: the first-order, GLCM and GLDM classes
 * of the reference's params.yml (RadiomicExtractor.py, extract_radiomics.py) on the original image type, for the gray,
 * red, green and blue channel of every chosen image in one launch (isic_hip/radiomics.py).  Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h and isic_hip_moments.h: device pointers, return 0 or a negative ISIC_ERR_* code, arguments
 * are checked before any device work, no allocation, no synchronisation, `stream` last.
 *
 * pixels, masks, offsets, hw, n_pool: the arrays of isic_hip.augment.ImagePool, as isic_augment_u8 takes them -- image n is
 * HWC uint8 (R is byte 0) at byte 3 offsets[n] of `pixels`, its mask HW uint8 at byte offsets[n] of `masks`, hw[2 n] rows
 * and hw[2 n + 1] columns.  Row b of the result belongs to pool image index[b] (the caller checks 0 <= index[b] < n_pool
 * on the host, where the list is made; the kernel clamps).  An image has fewer than 2^30 pixels (the counts are 32-bit).
 *
 * Channels, in this order: gray, red, green, blue; gray = (4899 R + 9617 G + 1868 B + 8192) >> 14, the 8-bit BGR2GRAY of
 * OpenCV in integers.  The region of interest (ROI) is mask == label; every other mask byte is background.
 *
 * The kernel counts, per image and channel, three integer matrices in one pass over the pixels; `counts`, when not NULL,
 * receives them as int32 [B][4][ISIC_RADIOMICS_COUNTS] in this layout:
 *   [0, 256)        hist[v]         ROI pixels of value v
 *   [256, 4352)     glcm[k][a][b]   k = 0..3 for the offsets (dy, dx) = (0, 1), (1, -1), (1, 0), (1, 1), distance 1; over
 *                                   ABSOLUTE bins a = v / bin_width (integer division), 32 x 32 per angle.  For an ROI pixel
 *                                   p and the ROI pixel q = p + offset inside the image glcm[k][a(p)][a(q)] and
 *                                   glcm[k][a(q)][a(p)] each grow by one (symmetric; the diagonal grows by two).
 *   [4352, 4640)    gldm[a][j]      ROI pixels of bin a with exactly j of their 8 neighbours inside the image, in the ROI
 *                                   and of the same bin (alpha = 0), 32 x 9.
 *
 * The features are fp64 functions of these integers, formed by the same workgroup in a fixed order of additions: two
 * identical calls give identical bits, and a row depends on its own image only.  PyRadiomics's gray level of a bin is
 * i = a - min_ROI / bin_width + 1 and Ng = max_ROI / bin_width - min_ROI / bin_width + 1 (integer divisions); levels
 * without an ROI pixel are skipped, as PyRadiomics deletes their empty rows and columns.  eps = 2^-52 inside every
 * log2(p + eps).  out is fp64 [B][4][ISIC_RADIOMICS_FEATURES]; per channel, in the order of PyRadiomics's feature names:
 *   firstorder [0, 18):  10Percentile 90Percentile Energy Entropy InterquartileRange Kurtosis Maximum MeanAbsoluteDeviation
 *                        Mean Median Minimum Range RobustMeanAbsoluteDeviation RootMeanSquared Skewness TotalEnergy
 *                        Uniformity Variance
 *       on the raw ROI values; percentiles by numpy.percentile's linear rule (virtual index (n - 1) q); Entropy and
 *       Uniformity on the discretised histogram; Kurtosis m4 / m2^2 and Skewness m3 / m2^1.5, 0 when m2 = 0; the robust
 *       deviation over the values in [P10, P90] about their own mean; TotalEnergy = Energy (unit spacing); population variance.
 *       When no ROI value lies in [P10, P90] (two pixels of different value, say) the robust deviation is 0 / 0 = NaN, as
 *       numpy gives for the mean of an empty selection; every other first-order feature stays defined.
 *   glcm [18, 42):       Autocorrelation ClusterProminence ClusterShade ClusterTendency Contrast Correlation DifferenceAverage
 *                        DifferenceEntropy DifferenceVariance Id Idm Idmn Idn Imc1 Imc2 InverseVariance JointAverage
 *                        JointEnergy JointEntropy MCC MaximumProbability SumAverage SumEntropy SumSquares
 *       every angle normalised to sum 1, every feature per angle, then the mean over the angles that have a pair; NaN if no
 *       angle has one.  Correlation is 1 when sigma = 0, Imc1 0 when max(HX, HY) = 0, Imc2 0 when HXY2 < HXY.  MCC is the
 *       second largest |lambda| of M = D^-1/2 P D^-1/2 over the levels of the ROI (cyclic Jacobi, fp64; a level without a
 *       pair in that angle has a zero row), 1 when the ROI has fewer than two levels.
 *   gldm [42, 56):       DependenceEntropy DependenceNonUniformity DependenceNonUniformityNormalized DependenceVariance
 *                        GrayLevelNonUniformity GrayLevelVariance HighGrayLevelEmphasis LargeDependenceEmphasis
 *                        LargeDependenceHighGrayLevelEmphasis LargeDependenceLowGrayLevelEmphasis LowGrayLevelEmphasis
 *                        SmallDependenceEmphasis SmallDependenceHighGrayLevelEmphasis SmallDependenceLowGrayLevelEmphasis
 *
 * An image without an ROI pixel gets a row of quiet NaNs (its counts are zero) and adds 1 to *n_empty, which the caller
 * zeroes; no other row changes.
 *
 * One launch, one workgroup per row b.  The image is walked in tiles of ISIC_RADIOMICS_TILE_H x ISIC_RADIOMICS_TILE_W pixels
 * that are staged in LDS with a halo of one pixel as the four bins of each pixel in one word; all four channels are counted
 * from that word with integer LDS atomics.
 *
 * ISIC_ERR_BAD_ARG: B < 0, n_pool < 0, bin_width outside 8..255 (more than ISIC_RADIOMICS_MAX_LEVELS bins otherwise), label
 * outside 1..255; with B > 0: pixels, masks, offsets, hw, index, out or n_empty NULL, or n_pool < 1.  B == 0 returns 0
 * without a launch. */
#ifndef ISIC_HIP_RADIOMICS_H
#define ISIC_HIP_RADIOMICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISIC_RADIOMICS_MAX_LEVELS 32      /* bin_width >= 8 on uint8 */
#define ISIC_RADIOMICS_FEATURES   56      /* 18 + 24 + 14 per channel */
#define ISIC_RADIOMICS_COUNTS     4640    /* 256 + 4 * 32 * 32 + 32 * 9 per channel */
#define ISIC_RADIOMICS_TILE_H     30      /* with the halo: 32 x 64 words */
#define ISIC_RADIOMICS_TILE_W     62
int isic_radiomics_u8(const uint8_t* pixels, const uint8_t* masks, const int64_t* offsets, const int32_t* hw,
                      int64_t n_pool, const int64_t* index, int64_t B, int bin_width, int label,
                      double* out /* [B][4][56] */, int32_t* counts /* optional, may be NULL */,
                      int64_t* n_empty /* one counter, added to */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_RADIOMICS_H */
