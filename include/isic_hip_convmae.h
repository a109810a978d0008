/* libisic_hip.so -- the convolutional front of the ConvMAE-Base patch encoder (included by isic_hip.h).
 *
 * ConvMAEBaseEncoder (multimodal-isic_amd/isic_hip/convmae.py) composes these with isic_gemm_f16 / _ln / _stats and
 * isic_attention_f16.  Conventions as in isic_hip.h: return 0 or a negative ISIC_ERR_* code, arguments are checked before
 * any device work, device pointers, `stream` last, no allocation.  fp16 tensors travel as uint16_t bit patterns; every
 * sum is in fp32.  Activations are NHWC: pixel-major rows of C channels.
 */
#ifndef ISIC_HIP_CONVMAE_H
#define ISIC_HIP_CONVMAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Depthwise 5x5 convolution, stride 1, zero padding 2 (Conv2d(C, C, 5, padding=2, groups=C)):
 *   y[n][h][w][c] = bias[c] + sum_{kh,kw} w_taps[kh*5+kw][c] x[n][h+kh-2][w+kw-2][c]
 * x, y: NHWC fp16 [N][H][W][C]; w_taps: fp32 [25][C] (the OIHW weight [C][1][5][5] transposed); bias fp32 [C] or NULL.
 * C % 64 == 0, else UNSUPPORTED; any H, W >= 1. */
int isic_dwconv5x5_f16(const uint16_t* x, const float* w_taps, const float* bias, uint16_t* y, int N, int H, int W, int C,
                       void* stream);
/* Rows of a P x P / stride P convolution over NHWC fp16 x[N][H][W][C] (space-to-depth):
 *   rows[(n*(H/P) + py)*(W/P) + px][(kh*P + kw)*C + c] = x[n][py*P+kh][px*P+kw][c]
 * (the OIHW weight permuted to [O][kh][kw][I] is then the Linear weight).  P in {2, 4}, C % 8 == 0, H % P == W % P == 0,
 * else UNSUPPORTED. */
int isic_patch_rows_nhwc_f16(const uint16_t* x, uint16_t* rows, int N, int H, int W, int C, int P, void* stream);
/* The same rows from an NCHW fp32 image[N][C][H][W], rounded to fp16, zero-padded from C*P*P to K_out columns (the stem:
 * C = 3, P = 4, K_out = 64 so that isic_gemm_f16 takes it).  K_out % 8 == 0, K_out >= C*P*P, H % P == W % P == 0, else
 * UNSUPPORTED. */
int isic_patch_rows_nchw_f32(const float* images, uint16_t* rows, int N, int C, int H, int W, int P, int K_out,
                             void* stream);
/* y = act(LayerNorm(x + a + b)) over rows of N fp16 values (a, b: optional fp16 addends of x's shape, NULL = 0; the sum
 * (x + a) + b is taken in fp32 and not rounded), two-pass mean / variance in fp32, act: 0 none, 1 erf-GELU after the affine.
 * Writes y (fp16) and / or y_f32.  N % 64 == 0 and N <= 1024, else UNSUPPORTED. */
int isic_layernorm_add_f16(const uint16_t* x, const uint16_t* a, const uint16_t* b, const float* gamma, const float* beta,
                           uint16_t* y, float* y_f32, int64_t M, int N, int act, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_CONVMAE_H */
