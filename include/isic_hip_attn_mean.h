/* libisic_hip.so -- head-averaged attention (PyG concat=False) for GATConv, GATv2Conv and TransformerConv: the four
 * attention entries of isic_hip.h with the mean over heads formed inside the kernels (included by isic_hip.h).
 *
 * Conventions as in isic_hip.h: fp32 row-major device tensors, return 0 or a negative ISIC_ERR_* code, arguments are
 * checked before any device work, no allocation, no synchronisation, `stream` last.
 */
#ifndef ISIC_HIP_ATTN_MEAN_H
#define ISIC_HIP_ATTN_MEAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* With o[i,h,:] the per-head aggregate isic_gat_fwd / isic_edge_attn_fwd compute without a bias:
 *   out[i,f] = (1/H) sum_h o[i,h,f] + bias[f]          out [N,F], bias [F] or NULL.
 * Inputs ([N,H,F]), scores, softmax, the CSR modes, alpha[nnz,H] (pre-dropout) and the dropout element slot*H + h are
 * those of the concat entries.  Any H and F: the wave that owns a destination row keeps the row's ceil(F/64) partial sums
 * over the heads in registers while F <= 256 and adds head by head into its own out row beyond that; nothing of width H*F
 * is written.  A mode-1 node without incoming edges gets out = bias.
 *
 * The backward entries take dout [N,F] and return what the concat entries return for dout_concat[i,h,f] = dout[i,f] / H,
 * in the same arrays with the same shapes (gat: de, dar, dal, dxp; edge_attn: de, dqd, dks, dv, datt += as there, so
 * datt stays the one output that is not bit-reproducible).  The destination sweep holds row i of dout in registers for
 * all heads (F <= 256), the source sweep gathers dout[dst,:] with row stride F.  d bias is the caller's colsum(dout).
 * Rows of more than 512 stored entries park their per-edge values in alpha / de as in the concat entries. */
int isic_gat_fwd_mean(const float* xp, const float* al, const float* ar, const int32_t* rowptr, const int32_t* col,
                      const float* bias, float* out, float* alpha, int64_t N, int H, int F, float negative_slope,
                      uint32_t drop_threshold, float drop_scale, uint64_t seed, uint64_t stream_id, void* stream);
int isic_gat_bwd_mean(const float* dout, const float* xp, const float* alpha, const float* al, const float* ar,
                      const float* att_src, const float* att_dst, const int32_t* rowptr, const int32_t* col,
                      const int32_t* rowptr_t, const int32_t* col_t, const int32_t* perm_t, float* de, float* dar, float* dal,
                      float* dxp, int64_t N, int H, int F, float negative_slope, uint32_t drop_threshold, float drop_scale,
                      uint64_t seed, uint64_t stream_id, void* stream);
int isic_edge_attn_fwd_mean(int mode, const float* ks, const float* qd, const float* v, const float* att,
                            const int32_t* rowptr, const int32_t* col, const float* bias, float* out, float* alpha, int64_t N,
                            int H, int F, float negative_slope, float scale, uint32_t drop_threshold, float drop_scale,
                            uint64_t seed, uint64_t stream_id, void* stream);
int isic_edge_attn_bwd_mean(int mode, const float* dout, const float* ks, const float* qd, const float* v, const float* att,
                            const float* alpha, const int32_t* rowptr, const int32_t* col, const int32_t* rowptr_t,
                            const int32_t* col_t, const int32_t* perm_t, float* de, float* dqd, float* dks, float* dv,
                            float* datt, int64_t N, int H, int F, float negative_slope, float scale, uint32_t drop_threshold,
                            float drop_scale, uint64_t seed, uint64_t stream_id, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_ATTN_MEAN_H */
