/* libisic_hip.so -- training entry points of the ViT-S/16 patch encoder (included by isic_hip.h).
 *
 * The backward pass of a stack of pre-norm transformer blocks (multimodal-isic_amd/isic_hip/transformer.py: the ViT-S/16
 * encoder, blocks3 of ConvMAE-Base and the MAE decoder); its LayerNorm backward is isic_layernorm_add_bwd_f16
 * (isic_hip_convmae_train.h).  Conventions as in isic_hip.h: return 0 or a negative ISIC_ERR_* code, arguments are
 * checked before any device work, device pointers, `stream` last.  fp16 tensors travel as uint16_t bit patterns;
 * gradients are fp32.  They sit in a header of their own so that isic_hip.h keeps listing the drop-in surface of the
 * reference.
 *
 * The backward runs on loss-scaled gradients (a power of two S chosen by the caller); `scale` (= 1/S) multiplies every
 * reduction that lands in a parameter gradient, in fp32.  accumulate == 1: out += scale * sum, 0: out = scale * sum.
 * Every reduction is split over blocks into fp32 slabs added in a fixed order (no float atomics): bit-reproducible.
 * A workspace of ..._workspace_bytes(...) bytes holds the slabs (ISIC_ERR_WORKSPACE when it is smaller).
 */
#ifndef ISIC_HIP_VIT_TRAIN_H
#define ISIC_HIP_VIT_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Weight gradient of C = A . W^T: dW[N][K] (+)= scale * sum_m dY[m][n] X[m][k] over the rows of dY[M][N] and X[M][K]
 * (fp16), on v_mfma_f32_16x16x32_f16; db[N] (+)= scale * sum_m dY[m][n] when db is not NULL.  N and K multiples of 128
 * in [128, 4096], else UNSUPPORTED; M arbitrary (M == 0: an empty sum). */
size_t isic_gemm_f16_wgrad_workspace_bytes(int64_t M, int N, int K);
int isic_gemm_f16_wgrad(const uint16_t* dY, const uint16_t* X, float* dW, float* db, int64_t M, int N, int K, float scale,
                        int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* out[cols] (+)= scale * sum_r x[r][cols] (fp16 rows): bias gradients, and the position-embedding gradient with x viewed
 * as [images][tokens * dim].  cols % 8 == 0, else UNSUPPORTED. */
size_t isic_colsum_f16_workspace_bytes(int64_t rows, int cols);
int isic_colsum_f16(const uint16_t* x, float* out, int64_t rows, int cols, float scale, int accumulate, void* workspace,
                    size_t workspace_bytes, void* stream);
/* Backward of isic_attention_f16 per (image, head): from qkv[M][3 D], its output out[M][D] and dout[M][D] (fp16,
 * D = heads * 64) -> dqkv[M][3 D] (fp16, same layout as qkv).  S and P are recomputed from q and k (softmax scale 1/8).
 * head_dim 64 and tokens <= 208, else UNSUPPORTED. */
int isic_attention_bwd_f16(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, uint16_t* dqkv, int n_images,
                           int tokens, int heads, int head_dim, void* stream);
/* C = (A . W^T) * gelu'(aux) elementwise (erf-GELU derivative; aux[M][N] fp16, the saved fc1 pre-activation): the data
 * gradient of fc1's output.  isic_gemm_f16's shape rules (K % 64 == 0, N % 128 == 0, else UNSUPPORTED). */
int isic_gemm_f16_dgelu(const uint16_t* A, const uint16_t* W, const uint16_t* aux, uint16_t* C, int M, int N, int K,
                        void* stream);
/* isic_gemm_f16 with act 1 (no residual) that also writes the pre-activation A . W^T + bias rounded to fp16 -> pre[M][N].
 * C is bitwise what isic_gemm_f16 writes. */
int isic_gemm_f16_gelu_pre(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* C, uint16_t* pre, int M, int N,
                           int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_VIT_TRAIN_H */
