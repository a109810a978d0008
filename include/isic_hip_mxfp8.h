/* libisic_hip.so -- MXFP8 entry points of the ViT-S/16 patch encoder (included by isic_hip.h).
 *
 * The opt-in inference format of the frozen encoder (multimodal-isic_amd/isic_hip/vit.py, precision="mxfp8"; the
 * reference runs its frozen encoder under no_grad, save_latent.py:42-60).  Conventions as in isic_hip.h: return 0 or a
 * negative ISIC_ERR_* code, arguments are checked before any device work, device pointers, `stream` last.
 * They sit in a header of their own so that isic_hip.h keeps listing the drop-in surface of the reference.
 *
 * Format: OCP MX with FP8 E4M3 (e4m3fn) elements.  An operand of R rows and K columns is q[R][K] e4m3 bytes plus
 * s[R][K/32] E8M0 bytes, one per 32 consecutive elements along K: value = float(q) * 2^(s - 127).  A block quantises as:
 * amax = max |v| (fp32); amax == 0 -> scale byte 0 and every element +0; otherwise e = the smallest integer with
 * amax <= 448 * 2^e (clamped to [-127, 127]), scale byte e + 127, element = round-to-nearest-even e4m3fn of v * 2^-e
 * (never saturates).  Inputs must be finite.
 */
#ifndef ISIC_HIP_MXFP8_H
#define ISIC_HIP_MXFP8_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Rows x[M][K] (fp16 bit patterns if x_is_f32 == 0, fp32 if 1) -> (q, s): the weights (from the fp32 masters, once per
 * weight version) and the attention output before attn.proj.  K % 32 == 0, else UNSUPPORTED. */
int isic_mxfp8_quantize(const void* x, int x_is_f32, uint8_t* q, uint8_t* s, int64_t M, int K, void* stream);
/* LayerNorm over the N = 384 fp16 values of a row (affine, eps) quantised to MXFP8 straight from the fp32 normalised
 * values (no fp16 rounding between): isic_layernorm_f16's kernel with another way out (csrc/ln_rows.inc: one source text,
 * the same sums in the same order, mean = sum * (1 / N)).  The compiler contracts multiply-adds per kernel, so the fp32
 * values quantised here may differ in the last bit from the ones isic_layernorm_f16 writes;
 * tests/test_ln_rows_gpu.py pins the bits of each.  N != 384: UNSUPPORTED. */
int isic_layernorm_mxfp8_f16(const uint16_t* x, const float* gamma, const float* beta, uint8_t* q, uint8_t* s, int64_t M,
                             int N, float eps, void* stream);
/* C = act((A_q . A_s)[M,K] (W_q . W_s)[N,K]^T + bias) (+ residual), fp32 accumulation on the block-scaled MFMA.  bias,
 * act (0 none, 1 erf-GELU), residual / residual_rows as isic_gemm_f16.  The output is EITHER fp16 C[M][N] (C_q = C_s =
 * NULL) OR MXFP8 (C_q[M][N], C_s[M][N/32]; C = NULL), quantised from the fp32 epilogue value; both or neither: BAD_ARG.
 * K % 128 == 0 and N % 128 == 0, else UNSUPPORTED; M arbitrary. */
int isic_gemm_mxfp8(const uint8_t* A_q, const uint8_t* A_s, const uint8_t* W_q, const uint8_t* W_s, const float* bias,
                    const uint16_t* residual, uint16_t* C, uint8_t* C_q, uint8_t* C_s, int M, int N, int K, int act,
                    int residual_rows, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_MXFP8_H */
