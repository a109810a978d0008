/* libisic_hip.so -- the integer counts every validation metric of the reference is a function of: the confusion matrix and,
 * per class, the number of (positive, negative) pairs the class score orders correctly (ties count half).  The device half
 * of the scoring the reference does on the CPU with scikit-learn: 01_train_mil_teacher.py:111-113,266-272 (roc_auc_score,
 * balanced_accuracy_score), 05_train_gnns.py:284-302 (accuracy, balanced accuracy, macro one-vs-rest AUROC, macro
 * precision / recall / F1), utils_g_mil.py:245-251,806-812.  isic_hip/metrics.py (class_counts, ClassMetrics) forms the floats
 * from the counts in fp64 on the host.  Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h: row-major device tensors, return 0 or a negative ISIC_ERR_* code, arguments are
 * checked before any device work, no allocation, no synchronisation, `stream` last.
 */
#ifndef ISIC_HIP_METRICS_H
#define ISIC_HIP_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Inputs: scores [n, C] fp32 (dense), labels [n] int64 (as isic_cross_entropy takes them), loss [n] fp32 or NULL.
 *
 * A sample is COUNTED when its label lies in [0, C) and all C of its scores are finite.  Outputs, all written on every
 * call (the caller never zeroes anything):
 *   confusion[C * C] int64   [t][p] = counted samples with label t and prediction p; the prediction is the LOWEST index
 *                            that holds the row maximum (numpy's argmax rule).
 *   pair2[C]         int64   for class c: the sum over counted i with labels[i] == c and counted j with labels[j] != c of
 *                            2 [s_ic > s_jc] + [s_ic == s_jc].  The order is that of the IEEE fp32 compare of the stored
 *                            values: -0.0 == 0.0, subnormals compare by value and are never flushed (the softmax outputs
 *                            of a confident model are subnormal).  AUROC_c = pair2[c] / (2 support_c (n - support_c)).
 *   flags[2]         int64   [0] the number of non-finite score ELEMENTS, [1] the number of labels outside [0, C).  A sample
 *                            that adds to either flag is not counted: it contributes to no other output.
 *   loss_sum[1]      fp64    the sum of loss[i] over counted samples.  loss == NULL: 0.0 is written when loss_sum is given,
 *                            and loss_sum may be NULL.
 *
 * Accumulation.  A block owns ISIC_METRICS_BLOCK = 256 samples i (one thread each; a thread is a positive of exactly one
 * class) and walks tiles of ISIC_METRICS_TILE = 512 samples j staged in LDS; a thread's count inside one tile is 32-bit
 * (at most 2 * 512), everything across tiles and blocks is 64-bit.  Block partials are parked in the workspace and a
 * finishing kernel on the same stream adds them: the integers exactly, the fp64 loss partials (a fixed tree inside a
 * block) in ascending block order.  No floating-point atomics, no fences: two identical calls give identical bits, and a
 * captured launch replays correctly.  The cost is n^2 comparisons (4 M at n = 2048, 10^10 at n = 10^5).
 *
 * Domain: 2 <= C <= 16 and 0 <= n < 2^31, otherwise ISIC_ERR_UNSUPPORTED.  confusion, pair2 or flags NULL, loss_sum NULL
 * with loss given, scores or labels NULL with n > 0, n < 0: ISIC_ERR_BAD_ARG.  A workspace smaller than the query (or not
 * 16-byte aligned): ISIC_ERR_WORKSPACE.  n == 0 writes zeros.  The workspace query returns 0 outside the domain. */
#define ISIC_METRICS_BLOCK 256
#define ISIC_METRICS_TILE 512
size_t isic_class_metrics_f32_workspace_bytes(int64_t n, int C);
int isic_class_metrics_f32(const float* scores, const int64_t* labels, const float* loss, int64_t n, int C,
                           int64_t* confusion, int64_t* pair2, int64_t* flags, double* loss_sum, void* workspace,
                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_METRICS_H */
