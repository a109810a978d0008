/* libisic_hip.so -- the 64 -> 64 weight gradient of the ResNet-18 patch encoder with the BatchNorm-backward apply pass
 * folded in (included by isic_hip.h).
 *
 * Conventions as in isic_hip.h: NHWC bf16 activations as 16-bit patterns, fp32 accumulation, return 0 or a negative
 * ISIC_ERR_* code, arguments are checked before any device work, no allocation, device pointers, `stream` last.
 */
#ifndef ISIC_HIP_WGRAD_BNBWD_H
#define ISIC_HIP_WGRAD_BNBWD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Weight gradient of a 64 -> 64 3x3 / stride 1 / pad 1 layer whose output gradient does not exist yet: the layer's output
 * c went through BatchNorm (+ReLU) and dz is the gradient of THAT output.  The kernel forms
 *   dc = BatchNorm backward of dz = what isic_bn_bwd_apply_mask_bf16(dz, c, relu_mask, ...) writes when relu_mask is given,
 *        what isic_bn_bwd_apply_bf16(dz, c, NULL, ..., relu = 1, scale, shift) writes when it is NULL
 * on its way into LDS, stores it to dc (bit-identical to those passes) and accumulates dw += conv_wgrad(x, dc) exactly as
 * isic_conv2d_wgrad_bf16(x, dc) does -- one pass over (dz, c) and one kernel less.  sum_dz / sum_dzx[64]: the reduced
 * sums (dbeta / dgamma of isic_bn_bwd_reduce*_bf16); dgamma_f32 / dbeta_f32 (optional) get += them.  No residual
 * gradient is written.  workspace: isic_conv2d_wgrad_workspace_bytes(N, 64, H, W, 64, 3, 3).  ..._supported() says
 * whether the shape is served; another ReLU form (relu_mask and scale both NULL) is ISIC_ERR_UNSUPPORTED. */
size_t isic_conv2d_wgrad_bnbwd_supported(int N, int H, int W, int Cin, int Cout, int Kh, int Kw, int stride, int pad,
                                         int has_mask);
int isic_conv2d_wgrad_bnbwd_bf16(const uint16_t* x, const uint16_t* dz, const uint16_t* c, const uint8_t* relu_mask,
                                 const float* mean, const float* rstd, const float* gamma, const double* sum_dz,
                                 const double* sum_dzx, const float* scale, const float* shift, uint16_t* dc, float* dw,
                                 float* dgamma_f32, float* dbeta_f32, int N, int H, int W, void* workspace,
                                 size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_WGRAD_BNBWD_H */
