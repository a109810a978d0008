/* libisic_hip.so -- the wide rows of GraphMIL: attention pooling over more than 1024 feature columns and / or more than
 * four pooling heads, and the LayerNorm backward over more than 1024 columns (gnn_concat=True with hidden x heads up to
 * 4096, att_heads = 8: the corner of the reference's search space, tune_mil.py:170-200, that isic_attn_pool_fwd / _bwd
 * and isic_layernorm_bwd* refuse).  Included by isic_hip.h.
 *
 * Conventions as in isic_hip.h: row-major fp32 device tensors, return 0 or a negative ISIC_ERR_* code, arguments are
 * checked before any device work, no allocation, no synchronisation, `stream` last.  The entries of isic_hip.h keep
 * their domains and their refusals; the caller chooses (isic_hip/ops.py: _pool_wide() is the one place that picks the
 * pool entry, forward and backward, for the autograd Function and for torch.ops.isic_hip.attn_pool alike; the wide
 * LayerNorm backward for N > 1024).
 */
#ifndef ISIC_HIP_WIDE_H
#define ISIC_HIP_WIDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Domain of the two pool entries: 1 <= H <= ISIC_WIDE_MAX_H, 1 <= A <= ISIC_WIDE_MAX_A, 1 <= heads <=
 * ISIC_WIDE_MAX_HEADS, 0 <= max_bag <= ISIC_WIDE_MAX_BAG (a bag's scores, heads floats per row, and its head-mean
 * weights stay in LDS: 2048 x 8 x 4 B = 64 KiB next to the 16 KiB of w3).  ISIC_ERR_UNSUPPORTED outside, before any
 * device work: no output is touched.  ISIC_ERR_BAD_ARG: a NULL tensor with B > 0, B < 0, a size below 1, max_bag < 0.
 * B == 0 returns 0 without a launch.  max_bag >= the longest bag is the caller's promise, as in isic_attn_pool_fwd. */
#define ISIC_WIDE_MAX_H 4096
#define ISIC_WIDE_MAX_A 512
#define ISIC_WIDE_MAX_HEADS 8
#define ISIC_WIDE_MAX_BAG 2048

/* GraphMIL form of isic_attn_pool_fwd (no class-space branch): h [T,H], t [T,heads*A] (= tanh(h W2^T + b2)),
 * w3 [heads,A], b3 [heads], offsets [B+1] (int64) -> att [T,heads] (softmax over each bag per head),
 * z [B,H] = mean_k sum_n att[n,k] h[n,:] = sum_n abar[n] h[n,:] with abar[n] = mean_k att[n,k]: ONE weighted column
 * sum over h whatever the head count.  Two launches: a block per bag (scores, a wave per row; softmax per head in LDS;
 * att), then a block per (bag, 64 columns): abar from att, four row groups, joined in group order.  t and h are read once.
 * An empty bag reads no row and writes no row of att; its z row is zero.  No atomics: two calls give the same bits. */
int isic_attn_pool_wide_fwd(const float* h, const float* t, const float* w3, const float* b3, const int64_t* offsets,
                            int B, int H, int A, int heads, int max_bag, float* att, float* z, void* stream);

/* Backward of the above from the saved att: d_z [B,H] -> d_s [T,heads] (gradient of the scores), d_u [T,heads*A]
 * (gradient BEFORE the tanh: d_s w3 (1 - t^2)), d_h [T,H] = abar[n] d_z[b,:] (accumulate_dh: +=), which EXCLUDES the
 * d_u W2 term (the caller's GEMM), as isic_attn_pool_bwd.  dL/da[n,k] = d_z[b] . h[n] / heads =: g[n] is the same for every
 * head: one H-long dot per row, then d_s[n,k] = att[n,k] (g[n] - sum_m att[m,k] g[m]) per head in LDS.  Two launches: a
 * block per bag (g, d_s, d_u), then a block per (bag, 256 columns, rows n = r mod 8) for d_h.  h and t are read once.  An empty
 * bag reads and writes no row.  No atomics and a fixed summation order: two calls give the same bits. */
int isic_attn_pool_wide_bwd(const float* h, const float* t, const float* att, const float* w3, const int64_t* offsets,
                            int B, int H, int A, int heads, int max_bag, const float* d_z, float* d_h,
                            int accumulate_dh, float* d_u, float* d_s, void* stream);

/* isic_layernorm_bwd_ws for 1 <= N <= ISIC_WIDE_MAX_N (ISIC_ERR_UNSUPPORTED beyond, no output touched): the same
 * arguments, the same arithmetic per element, the same dropout words and ReLU mask (element index row * N + col, seed,
 * stream_id + clock[0] * 1024) as the forward isic_layernorm_fwd_clk used.  A block of 256 threads per row, rows
 * block, block + grid, ...; grid = min(ceil(M / 2), ISIC_WIDE_LN_MAX_BLOCKS); the two row sums go through LDS; a thread
 * keeps the dgamma / dbeta partials of its columns over the block's rows.  With N % 4 == 0 and 16-byte aligned x, dy, dx,
 * gamma, beta a thread owns four neighbouring columns (16-byte accesses, one Philox block per four elements); otherwise
 * single columns.  dx is written; dgamma / dbeta are ACCUMULATED (+=).  With a workspace of
 * isic_layernorm_bwd_wide_workspace_bytes(N) bytes (16-byte aligned) every block stores its [2][N] partial row and the
 * partial rows are added in block order (bit-reproducible, the reducer of isic_layernorm_bwd_ws); with workspace NULL or
 * too small they meet through fp32 atomics, one per column and block. */
#define ISIC_WIDE_MAX_N 4096
#define ISIC_WIDE_LN_MAX_BLOCKS 512
size_t isic_layernorm_bwd_wide_workspace_bytes(int N);      /* 0 outside 1 <= N <= ISIC_WIDE_MAX_N */
int isic_layernorm_bwd_wide_ws(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                               const float* rstd, float* dx, float* dgamma, float* dbeta, int M, int N, int relu,
                               uint32_t drop_threshold, float drop_scale, uint64_t seed, uint64_t stream_id,
                               const uint64_t* clock, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_WIDE_H */
