/* libisic_hip.so -- per-image statistics of a token grid over its token axis: the reference's concat_patch_moments
 * (utils.py:16-31; isic_hip/moments.py: token_moments, utils.py: concat_patch_moments).  Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h: row-major device tensors, return 0 or a negative ISIC_ERR_* code, arguments are
 * checked before any device work, no allocation, no synchronisation, `stream` last.
 */
#ifndef ISIC_HIP_MOMENTS_H
#define ISIC_HIP_MOMENTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* X is fp32: token t of image b, channel d, is X[(b T + t) ldx + d].  out is fp32: out[b ldo + s D + d] with
 * s = 0..5 for mean, max, std, median, skewness, excess kurtosis of the T values of (b, d) -- the reference's
 * concatenation order.  With c_t = x_t - mean:
 *   mean     = (sum_t x_t) / T
 *   max      = max_t x_t                                         (an input element: no rounding)
 *   std      = sqrt(sum_t c_t^2 / (T - unbiased))
 *   median   = the element of ascending rank (T - 1) / 2 (integer division: the lower middle element of an even T,
 *              as torch.median)                                  (an input element: no rounding)
 *   sigma    = max(std, eps)
 *   skew     = (sum_t c_t^3 / T) / sigma^3
 *   kurtosis = (sum_t c_t^4 / T) / sigma^4 - 3
 *
 * One launch.  A block of 256 threads takes one image and one slab of W channels, stages X[b, 0:T, slab] into LDS once
 * (16-byte loads along D when ldx % 4 == 0 and X is 16-byte aligned, element loads otherwise) and works from LDS only: X
 * is read once and nothing but `out` is written; the ldo - 6 D floats of padding of an out row are not touched.
 * The slab width follows T so that the [T][W] tile fits in 64 KiB:
 *   T <= 256: W = 64        256 < T <= 512: W = 32        512 < T <= 1024: W = 16
 * The 256 / W threads of a channel each walk every (256 / W)-th token in ascending order (fp32), their partial sums meet in
 * LDS in ascending thread order; sum and max first, then with the mean known sum c^2, sum c^3, sum c^4.  The median is a
 * radix selection on order-preserving integer keys (four bits per pass from the sign down: the candidates are counted
 * into 16 bins in LDS, the digit is the bin in which the running count passes the rank; it stops once one candidate is
 * left in every channel of the slab), exact with any number of equal values; -0.0 orders below +0.0.  No floating-point
 * atomics (the bins are integer counts, which no order of additions can change): two identical calls give identical
 * bits, and the row of image b does not depend on B or on the other images.
 *
 * ISIC_ERR_BAD_ARG: X or out NULL with B > 0, B < 0, T < 1, D < 1, ldx < D, ldo < 6 D, eps negative or NaN, unbiased not
 * 0 or 1, unbiased with T < 2.  ISIC_ERR_UNSUPPORTED: T > ISIC_MOMENTS_MAX_T, or B ceil(D / W) blocks beyond 2^31 - 1.
 * B == 0 returns 0 without a launch.  Inputs are finite: NaN or Inf inputs are outside the domain (their outputs are
 * unspecified).  eps == 0 with a constant channel divides 0 by 0, as the reference does. */
#define ISIC_MOMENTS_MAX_T 1024
int isic_token_moments_f32(const float* X, int64_t B, int T, int D, int64_t ldx, float eps, int unbiased, float* out,
                           int64_t ldo, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_MOMENTS_H */
