/* libisic_hip.so -- training entry points of the ConvMAE-Base patch encoder (included by isic_hip.h).
 *
 * The backward pass of ConvMAEBaseEncoder(trainable=True) (multimodal-isic_amd/isic_hip/convmae.py) composes these with
 * the ViT-S backward of isic_hip_vit_train.h (weight-gradient GEMM, column sums, attention backward, dGELU epilogue) and
 * the forward kernels of isic_hip_convmae.h.  Conventions as in isic_hip_vit_train.h: return 0 or a negative ISIC_ERR_*
 * code, arguments are checked before any device work, device pointers, `stream` last.  fp16 tensors travel as uint16_t
 * bit patterns; gradients are fp32; activations are NHWC (pixel-major rows of C channels).
 *
 * `scale` (= 1/S, the inverse of the caller's power-of-two loss scale) multiplies every reduction that lands in a
 * parameter gradient, in fp32.  accumulate == 1: out += scale * sum, 0: out = scale * sum.  Every reduction is split over
 * blocks into fp32 slabs added in a fixed order (no float atomics): bit-reproducible.  A workspace of
 * ..._workspace_bytes(...) bytes holds the slabs (ISIC_ERR_WORKSPACE when it is smaller).
 */
#ifndef ISIC_HIP_CONVMAE_TRAIN_H
#define ISIC_HIP_CONVMAE_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Weight and bias gradient of the depthwise 5x5 convolution of isic_dwconv5x5_f16, stride 1, zero padding 2:
 *   dw_taps[kh*5+kw][c] (+)= scale * sum_{n,h,w} dy[n][h][w][c] x[n][h+kh-2][w+kw-2][c]   (x zero outside the image)
 *   db[c]               (+)= scale * sum_{n,h,w} dy[n][h][w][c]                           (when db is not NULL)
 * x: the convolution's input, dy: the gradient of its output, NHWC fp16 [N][H][W][C]; dw_taps fp32 [25][C] (the layout
 * of isic_dwconv5x5_f16's w_taps).  C % 64 == 0, else UNSUPPORTED; any H, W >= 1.  (The data gradient is
 * isic_dwconv5x5_f16 itself with the taps reversed, t -> 24 - t, and no bias.) */
size_t isic_dwconv5x5_wgrad_f16_workspace_bytes(int N, int H, int W, int C);
int isic_dwconv5x5_wgrad_f16(const uint16_t* x, const uint16_t* dy, float* dw_taps, float* db, int N, int H, int W, int C,
                             float scale, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of isic_layernorm_add_f16 over rows of N (N % 64 == 0, N <= 1024, else UNSUPPORTED).  The row statistics of
 * v = (x + a) + b (a, b: optional fp16 addends, NULL = 0; the sum in fp32, unrounded) are recomputed with the forward's
 * own two-pass fp32 arithmetic, so only the forward's inputs are needed.  dy[M][N] is fp16 (dy_is_f32 == 0) or fp32 (1),
 * multiplied by dy_mul on load.  With x^ = (v - mean) rstd and t = x^ gamma + beta, act == 1 first multiplies dy by the
 * erf-GELU derivative at t (act == 0: the identity); then with g^ = dy gamma:
 *   g_out = g_in + rstd (g^ - mean(g^) - x^ mean(g^ x^))   -- the gradient of v, hence of x, a and b alike
 * (fp32; g_in NULL = 0; g_out may alias g_in) and / or its fp16 copy g_out16 (either may be NULL, not both);
 * dgamma[N] (+)= scale * sum dy x^, dbeta[N] (+)= scale * sum dy (dy after the GELU derivative). */
size_t isic_layernorm_add_bwd_f16_workspace_bytes(int64_t M, int N);
int isic_layernorm_add_bwd_f16(const void* dy, int dy_is_f32, float dy_mul, const uint16_t* x, const uint16_t* a,
                               const uint16_t* b, const float* gamma, const float* beta, int act, float eps,
                               const float* g_in, float* g_out, uint16_t* g_out16, float* dgamma, float* dbeta, int64_t M,
                               int N, float scale, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* Depth-to-space, the adjoint of isic_patch_rows_nhwc_f16: from drows[(n*(H/P) + py)*(W/P) + px][(kh*P + kw)*C + c]
 * (fp16)
 *   dx[n][py*P+kh][px*P+kw][c] (+)= drows[...]        (fp32 NHWC [N][H][W][C]; accumulate == 1 adds to dx, 0 writes it)
 * and, when dx16 is not NULL, the fp16 copy of the result.  Every element of dx is written exactly once.  P in {2, 4},
 * C % 8 == 0, H % P == W % P == 0, else UNSUPPORTED. */
int isic_patch_rows_bwd_f16(const uint16_t* drows, float* dx, uint16_t* dx16, int N, int H, int W, int C, int P,
                            int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_CONVMAE_TRAIN_H */
