/* libisic_hip.so -- MXFP8 outputs on the convolutional front of the ConvMAE-Base patch encoder (included by isic_hip.h).
 *
 * The opt-in inference format of the frozen encoder (multimodal-isic_amd/isic_hip/convmae.py, precision="mxfp8"): these
 * write the operands isic_gemm_mxfp8 reads.  The format and the quantisation rule are exactly those of isic_hip_mxfp8.h
 * (OCP MX, e4m3fn elements q, one E8M0 scale s per 32 consecutive elements of a row); every output is quantised from the
 * fp32 value, with no fp16 rounding between.  Conventions as in isic_hip_mxfp8.h: return 0 or a negative ISIC_ERR_* code,
 * arguments are checked before any device work, device pointers, `stream` last, no allocation, nothing to do (M or N
 * images == 0) returns 0.  fp16 tensors travel as uint16_t bit patterns; activations are NHWC.
 */
#ifndef ISIC_HIP_CONVMAE_MXFP8_H
#define ISIC_HIP_CONVMAE_MXFP8_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* act(LayerNorm(x)) over rows of N fp16 values (act: 0 none, 1 erf-GELU after the affine) -> q[M][N], s[M][N/32]:
 * bitwise the quantisation of the y_f32 that isic_layernorm_add_f16 writes for the same x, gamma, beta, act and eps
 * without addends (the same kernel with another epilogue).  N % 64 == 0 and N <= 1024, else UNSUPPORTED. */
int isic_layernorm_act_mxfp8_f16(const uint16_t* x, const float* gamma, const float* beta, uint8_t* q, uint8_t* s, int64_t M,
                                 int N, int act, float eps, void* stream);
/* The depthwise 5x5 of isic_dwconv5x5_f16 -- x NHWC fp16 [N][H][W][C], w_taps fp32 [25][C], bias fp32 [C] or NULL, zero
 * padding 2 -- whose fp32 sums are quantised per pixel in blocks of 32 channels -> q[N*H*W][C], s[N*H*W][C/32].  C % 64 == 0, else UNSUPPORTED;
 * any H, W >= 1. */
int isic_dwconv5x5_mxfp8_f16(const uint16_t* x, const float* w_taps, const float* bias, uint8_t* q, uint8_t* s, int N, int H,
                             int W, int C, void* stream);
/* The rows of isic_patch_rows_nhwc_f16, in the same [kh][kw][c] column order, as MXFP8: q[rows][P*P*C], s[rows][P*P*C/32],
 * rows = N (H/P) (W/P).  A block is 32 consecutive channels of one pixel of x.  P in {2, 4}, C % 32 == 0,
 * H % P == W % P == 0, else UNSUPPORTED. */
int isic_patch_rows_mxfp8_nhwc_f16(const uint16_t* x, uint8_t* q, uint8_t* s, int N, int H, int W, int C, int P,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_CONVMAE_MXFP8_H */
