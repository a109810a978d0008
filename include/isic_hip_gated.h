/* libisic_hip.so -- the gate of gated attention pooling (Ilse et al. 2018): t = tanh(h V^T + b_V) * sigmoid(h U^T + b_U)
 * in front of the attention-pool kernels, which take t as an input and stay as they are (isic_attn_pool_fwd / _bwd,
 * isic_attn_pool_wide_fwd / _bwd).  Opt-in: the reference has no gate.  Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h: row-major fp32 device tensors, return 0 or a negative ISIC_ERR_* code, arguments are
 * checked before any device work, no allocation, no synchronisation, `stream` last.
 *
 * Layout.  nA = heads * A.  The pre-activation matrix p [T, 2 nA] (one GEMM over the stacked operand [V ; U]) holds the
 * tanh-branch columns of all heads in [0, nA) and the gate columns in [nA, 2 nA); head k owns columns k A .. k A + A - 1 of
 * each half.  ISIC_ERR_BAD_ARG: T < 0, heads < 1, A < 1, heads * A > ISIC_GATE_MAX_NA, a NULL tensor with T > 0, a beta
 * other than 0 or 1.  Element indices are 64-bit: T * 2 nA may exceed 2^31.  T == 0 returns 0 and touches nothing.
 */
#ifndef ISIC_HIP_GATED_H
#define ISIC_HIP_GATED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISIC_GATE_MAX_NA (1 << 20)

/* p [T, 2 nA] is OVERWRITTEN with tv | sg (tv = isic tanh of the first half, the function of the GEMM epilogue;
 * sg = 1 / (1 + exp(-x)) of the second half: exactly 1 for large x, exactly 0 for large -x, no NaN at +-inf) and
 * t [T, nA] = tv * sg is written.  One streaming pass: 2 reads and 3 writes per element pair.  16-byte accesses where
 * nA % 4 == 0 and p, t are 16-byte aligned; single floats otherwise. */
int isic_gate_fwd_f32(float* p, int T, int heads, int A, float* t, void* stream);

/* Backward of the gate from the saved a [T, 2 nA] = tv | sg, the score gradient d_s [T, heads] of the pool backward and
 * w3 [heads, A]:  d_t[n, kA+j] = d_s[n,k] w3[k,j];   d_p [T, 2 nA] = d_v | d_g  with  d_v = d_t sg (1 - tv^2)  (before the
 * tanh),  d_g = d_t tv sg (1 - sg)  (before the sigmoid).  The same pass takes the column sums
 *   d_bias [2 nA] = sum_n d_v | sum_n d_g,   d_w3 [heads, A] = sum_n d_s[n,k] tv sg,   d_b3 [heads] = sum_n d_s[n,k],
 * each as  out = beta * out + sum  (beta 0 or 1; 0 never reads out).  Rows n = c, c + chunks, c + 2 chunks, ... form row
 * chunk c, chunks = min(ceil(T / 16), 2048): a function of T alone.  Every chunk parks its sums as slab c of the workspace,
 * [chunks][3 nA + heads], and the slabs are added in the fixed order of the shared slab reducer (16 lanes per element):
 * no float atomics, two calls give the same bits.  The workspace has to hold isic_gate_bwd_f32_workspace_bytes(T, heads, A)
 * bytes (0 outside the domain), 16-byte aligned: ISIC_ERR_WORKSPACE otherwise, before any device work.  d_p may not alias a. */
size_t isic_gate_bwd_f32_workspace_bytes(int T, int heads, int A);
int isic_gate_bwd_f32(const float* d_s, const float* w3, const float* a, int T, int heads, int A, float* d_p,
                      float* d_bias, float* d_w3, float* d_b3, float beta, void* workspace, size_t workspace_bytes,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_GATED_H */
