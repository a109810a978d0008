/* libisic_hip.so -- the shifted Gram matrix of resident latents: the device half of the latent PCA of
 * save_latent.py:163-185 (isic_hip/pca.py: DevicePCA).  Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h: row-major device tensors, return 0 or a negative ISIC_ERR_* code, arguments are
 * checked before any device work, no allocation, no synchronisation, `stream` last.
 */
#ifndef ISIC_HIP_PCA_H
#define ISIC_HIP_PCA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* With z_m = X[r_m, 0:D] - shift (one fp32 subtraction per element, made while the row tile is staged: no centred copy
 * is written) and r_m = rows[m] (rows != NULL) or m:
 *   G[D, D]   = beta * G      + sum_{m < M} z_m z_m^T          (fp64, row-major, leading dimension D)
 *   colsum[D] = beta * colsum + sum_{m < M} z_m                (fp64)
 * X is fp32 with rows ldx floats apart, rows int32 (read entry by entry below M; a caller that follows the groups-of-8
 * convention of isic_gemm_f32_rows_ws is served as well), shift [D] fp32 or NULL (zeros), beta 0 or 1 (1: a fit accumulated
 * over encoder batches; beta == 0 never reads the outputs).
 *
 * Accumulation.  The M rows are cut into runs of ISIC_GRAM_RUN = 2048 rows.  Inside a run the products are accumulated in
 * fp32 in the accumulators of v_mfma_f32_16x16x4_f32 (one 128 x 128 tile of G per block, only the tile pairs with column
 * tile J >= row tile I); the run's fp32 partial is parked in the workspace and a finishing kernel adds the partials of the
 * runs in ascending run order in fp64, applies beta and writes G[i,j] and G[j,i] from the same value: G is bit-symmetric.
 * The column sums take the same road (fp32 inside a run, fp64 across runs).  No atomics: two identical calls give
 * identical bits.  The workspace holds at most 2048 tiles at a time; a longer M is walked in several launches that
 * accumulate into G, so its size stops growing with M.
 *
 * Domain: 4 <= D <= 1024, D % 4 == 0, ldx >= D, ldx % 4 == 0, X (and shift) 16-byte aligned; otherwise ISIC_ERR_UNSUPPORTED.
 * G or colsum NULL, X NULL with M > 0, M < 0, beta not 0 or 1: ISIC_ERR_BAD_ARG.  A workspace smaller than the query
 * (or not 16-byte aligned): ISIC_ERR_WORKSPACE.  M == 0 is legal: beta == 0 writes zeros, beta == 1 leaves the outputs
 * alone.  Every row index must lie inside X; they are not checked. */
#define ISIC_GRAM_RUN 2048
size_t isic_gram_shifted_f32_workspace_bytes(int64_t M, int D);
int isic_gram_shifted_f32(const float* X, int64_t M, int D, int64_t ldx, const int32_t* rows, const float* shift,
                          double* G, double* colsum, double beta, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_PCA_H */
