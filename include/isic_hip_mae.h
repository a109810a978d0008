/* libisic_hip.so -- entry points of the ConvMAE-Base masked-autoencoder objective (included by isic_hip.h).
 *
 * ConvMAEBase (multimodal-isic_amd/isic_hip/convmae_mae.py) composes these with the encoder's forward and backward kernels
 * (isic_hip_convmae.h, isic_hip_convmae_train.h, isic_hip_vit_train.h).  Conventions as in isic_hip_convmae_train.h: return 0 or a
 * negative ISIC_ERR_* code, arguments are checked before any device work, no allocation, device pointers, `stream` last;
 * fp16 tensors travel as uint16_t bit patterns; token rows are [N][T][C] with T tokens per image in raster order.
 *
 * Masking: every image keeps L of its T tokens.  ids_keep[N][L] (int64) lists the kept tokens (the first L entries of
 * ids_shuffle[N][T], a permutation of 0..T-1 per image); ids_restore[N][T] is its inverse: token t is kept iff
 * ids_restore[n][t] < L, and is then row ids_restore[n][t] of the kept rows.  An index outside its range reads as a zero row.
 * keep[N][T] (uint8) is 1 for a kept token, 0 for a removed one.
 */
#ifndef ISIC_HIP_MAE_H
#define ISIC_HIP_MAE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The masked depthwise 5x5 of a CBlock: y = isic_dwconv5x5_f16(keep (.) x), where pixel (h, w) lies in token
 * (h / P) * (W / P) + w / P (P = pixels per token side: 4 at 56 x 56, 2 at 28 x 28).  xm (may be NULL) receives keep (.) x,
 * the input the weight gradient (isic_dwconv5x5_wgrad_f16) takes.  C % 64 == 0, H % P == W % P == 0, else UNSUPPORTED. */
int isic_dwconv5x5_masked_f16(const uint16_t* x, const uint8_t* keep, int P, const float* w_taps, const float* bias,
                              uint16_t* xm, uint16_t* y, int N, int H, int W, int C, void* stream);
/* Its data gradient: dx = keep (.) isic_dwconv5x5_f16(dy) with the reversed taps w_taps_rev (t -> 24 - t) and no bias. */
int isic_dwconv5x5_masked_dgrad_f16(const uint16_t* dy, const uint8_t* keep, int P, const float* w_taps_rev, uint16_t* dx,
                                    int N, int H, int W, int C, void* stream);
/* isic_attention_f16 and isic_attention_bwd_f16 (isic_hip_vit_train.h) with heads 32 wide: softmax scale 1 / sqrt(32),
 * tokens <= 208, else UNSUPPORTED; n_images == 0 is a no-op.  qkv[n_images*tokens][3*heads*32], out / dout
 * [n_images*tokens][heads*32]. */
int isic_attention_d32_f16(const uint16_t* qkv, uint16_t* out, int n_images, int tokens, int heads, void* stream);
int isic_attention_d32_bwd_f16(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, uint16_t* dqkv, int n_images,
                               int tokens, int heads, void* stream);
/* Row gather y[n][j] = x[n][ids_keep[n][j]] (x: [N][T][C], y: [N][L][C]) and its adjoint, the scatter
 * x[n][t] = ids_restore[n][t] < L ? y[n][ids_restore[n][t]] : 0 (every row of x written once; a negative rank is a zero
 * row too).  C % 8 == 0. */
int isic_gather_rows_f16(const uint16_t* x, const int64_t* ids_keep, uint16_t* y, int N, int T, int L, int C, void* stream);
int isic_scatter_rows_f16(const uint16_t* y, const int64_t* ids_restore, uint16_t* x, int N, int T, int L, int C,
                          void* stream);
/* The decoder's unshuffle: out[n][t] = fp16((ids_restore[n][t] < L ? y[n][ids_restore[n][t]] : mask_token) + pos[t]), the
 * sum in fp32 (y fp16 [N][L][C], mask_token fp32 [C], pos fp32 [T][C], out fp16 [N][T][C]).  A rank outside [0, L), a
 * negative one included, takes the mask token.  C % 8 == 0. */
int isic_mae_unshuffle_f16(const uint16_t* y, const int64_t* ids_restore, const float* mask_token, const float* pos,
                           uint16_t* out, int N, int T, int L, int C, void* stream);
/* Its adjoint, split by ids_shuffle[N][T]: dy_keep[n][j] = dout[n][ids_shuffle[n][j]] for j < L (the kept rows in ids_keep
 * order) and d_removed[n][j - L] = the same for j >= L ([N][T - L][C]; NULL only when L == T), whose column sum
 * (isic_colsum_f16) is the gradient of mask_token.  pos gets no gradient. */
int isic_mae_unshuffle_bwd_f16(const uint16_t* dout, const int64_t* ids_shuffle, uint16_t* dy_keep, uint16_t* d_removed, int N,
                               int T, int L, int C, void* stream);
/* Fused pixel-reconstruction loss over T = (H / P) (W / P) patches of K = P P C values per image.  The target of patch
 * (n, t) is patchify(images) in (row, column, channel) order, read from the NCHW fp32 images; with norm_pix == 1 it is
 * (target - mean) / sqrt(var + 1e-6) per patch, var unbiased.  pred fp16 [N][T][K], mask fp32 [N][T] (1 = removed):
 *   loss[0] = sum_{n,t} mask l_{n,t} / mask_sum,  l = mean_k (pred - target)^2            (fp32, on the device)
 *   dpred   = fp16(loss_scale * mask * 2 (pred - target) / (K mask_sum))                  (d loss / d pred, scaled)
 * mask_sum is the caller's sum of mask (> 0).  Both sums run in a fixed order (bit-reproducible); the workspace holds
 * N T per-patch terms.  2 <= K <= 1024 (the unbiased variance needs two values), H % P == W % P == 0, else UNSUPPORTED. */
size_t isic_mae_loss_f16_workspace_bytes(int N, int H, int W, int P);
int isic_mae_loss_f16(const uint16_t* pred, const float* images, const float* mask, int norm_pix, float mask_sum,
                      float loss_scale, uint16_t* dpred, float* loss, int N, int C, int H, int W, int P, void* workspace,
                      size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_MAE_H */
