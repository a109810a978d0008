/* libisic_hip.so -- the batch transform of the MAE fine-tune: crop, resize, flips, rot90 and normalisation of uint8 images
 * that stay resident on the device (included by isic_hip.h).
 *
 * multimodal-isic_amd/isic_hip/augment.py holds the pool and draws the parameters on the host; this entry produces one batch
 * per launch.  Conventions as in isic_hip_mae.h: return 0 or a negative ISIC_ERR_* code, arguments are checked before any
 * device work, no allocation, device pointers, `stream` last.
 *
 * Pool: n_pool images of ragged sizes.  Image n is hw[n] = (h, w) (int32 [n_pool][2]), stored HWC uint8 at byte
 * 3 * offsets[n] of `pixels`; its lesion mask is HW uint8 at byte offsets[n] of `masks`.  offsets (int64 [n_pool + 1]) count
 * pixels, and every address is 64-bit: a pool may exceed 2^31 bytes.
 *
 * Output b of B: the source image is index[b]; box[b] = (y0, x0, ch, cw) (int32 [B][4]) is the crop inside it; op[b] holds
 * the horizontal flip in bit 0, the vertical flip in bit 1 and k of np.rot90(., k) in bits 2-3, applied to the S x S resize
 * of the crop in the order hflip, vflip, rot90 (the reference's Compose order).  Per output pixel the kernel undoes the
 * rotation and then the flips to find pixel (r, c) of the resized crop, and resamples with exact rational coordinates:
 * along an axis of crop length n,
 *     num = max((2 r + 1) n - S, 0),   i0 = min(num / (2 S), n - 1),   i1 = min(i0 + 1, n - 1),   weight = (num mod 2 S) / (2 S)
 * -- the half-pixel centres of cv2.INTER_LINEAR / torch align_corners=False without antialiasing, clamped to the crop (not
 * to the image).  The image value is the bilinear blend of the four uint8 taps in fp32, then (v / 255 - mean[c]) / std[c];
 * nothing is rounded to uint8 in between, as in this project's CPU transform.  Parity with albumentations' fixed-point
 * uint8 resize is unpinned: that library is on none of the machines this was developed on.
 * The mask is nearest neighbour, i = min(floor(r n / S), n - 1) in integers, and its byte value is written as a float,
 * unscaled.
 *
 * image_out fp32 [B][3][S][S] and mask_out fp32 [B][1][S][S], contiguous; mask_out may be NULL (masks may then be NULL too).
 * The kernel cannot report a bad parameter: it clamps index[b] into [0, n_pool), the box into its image (sides at least 1
 * and at most 2^20) and every tap into the box, so no parameter value reads outside the pool; an image of no pixels gives
 * zeros.  The caller validates boxes and indices where it makes them.
 */
#ifndef ISIC_HIP_AUGMENT_H
#define ISIC_HIP_AUGMENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* B >= 0, 1 <= S <= 1024, std* != 0, else BAD_ARG; B == 0 is a no-op.  With B > 0: n_pool >= 1 and every pointer but masks /
 * mask_out non-NULL; masks == NULL with mask_out != NULL is BAD_ARG. */
int isic_augment_u8(const uint8_t* pixels, const uint8_t* masks, const int64_t* offsets, const int32_t* hw, int64_t n_pool,
                    const int64_t* index, const int32_t* box, const int32_t* op, float mean0, float mean1, float mean2,
                    float std0, float std1, float std2, float* image_out, float* mask_out, int64_t B, int S, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_AUGMENT_H */
