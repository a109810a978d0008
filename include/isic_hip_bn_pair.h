/* libisic_hip.so -- BatchNorm backward of the two norms that meet at a ResNet-18 downsample block's output, bn2 and the
 * shortcut's downsample.1, in one reduce and one apply pass (included by isic_hip.h).
 *
 * Conventions as in isic_hip.h: NHWC bf16 activations as 16-bit patterns, fp32 accumulation, return 0 or a negative
 * ISIC_ERR_* code, arguments are checked before any device work, no allocation, device pointers, `stream` last.
 */
#ifndef ISIC_HIP_BN_PAIR_H
#define ISIC_HIP_BN_PAIR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out = relu(bn(x) + bn2(x2)): both norms receive dz = dy where the ReLU was active (bit j of relu_mask[i]: element j of
 * 8-channel vector i, as isic_bn_apply_mask_bf16 writes it) and 0 elsewhere.  x, x2, dy: [rows, C]; C as for
 * isic_bn_bwd_reduce_bf16 (C % 8 == 0, C / 8 divides 256), else ISIC_ERR_UNSUPPORTED.
 *
 * reduce: one walk over the rows; sum_dzx[C] += sum dz * xhat and sum_dz[C] += sum dz are the sums of
 *   isic_bn_bwd_reduce_mask_bf16(dy, x, relu_mask, mean, rstd), sum_dzx2[C] += sum dz * xhat2 is the first sum of
 *   isic_bn_bwd_reduce_bf16(dz, x2, relu = 0, mean2, rstd2) (its second is sum_dz again).  fp64, zeroed by the caller.
 * apply: one flat walk; dx is what isic_bn_bwd_apply_mask_bf16(dy, x, relu_mask, ...) writes to dx, dx2 what
 *   isic_bn_bwd_apply_bf16(dz, x2, relu = 0, ...) writes with (sum_dzx2, sum_dz).  dgamma_f32 / dbeta_f32 and
 *   dgamma2_f32 / dbeta2_f32 (each pair optional) get += the sums.  dz itself is not written.
 * Both give the bits of the launches they replace, by construction: the pair is the same kernel template as those
 * launches, instantiated for two norms (same launch geometry and thread mapping), and every value -- the gate, the
 * accumulation step, the constants, dx -- comes from the same functions of csrc/bn_bwd_math.inc, whose source text spells
 * out every rounding (contraction off, each fused multiply-add a __builtin_fmaf), so nothing is left to the compiler's
 * contraction choices.  tests/test_bn_pair_gpu.py compares the two exactly; tests/test_bn_bwd_math_gpu.py compares both
 * with a numpy emulation of the include. */
int isic_bn_bwd_reduce_pair_bf16(const uint16_t* dy, const uint16_t* x, const uint8_t* relu_mask, const float* mean,
                                 const float* rstd, const uint16_t* x2, const float* mean2, const float* rstd2, int64_t rows,
                                 int C, double* sum_dzx, double* sum_dz, double* sum_dzx2, void* stream);
int isic_bn_bwd_apply_pair_bf16(const uint16_t* dy, const uint16_t* x, const uint8_t* relu_mask, const float* mean,
                                const float* rstd, const float* gamma, const double* sum_dzx, const double* sum_dz,
                                const uint16_t* x2, const float* mean2, const float* rstd2, const float* gamma2,
                                const double* sum_dzx2, int64_t rows, int C, uint16_t* dx, uint16_t* dx2, float* dgamma_f32,
                                float* dbeta_f32, float* dgamma2_f32, float* dbeta2_f32, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_BN_PAIR_H */
