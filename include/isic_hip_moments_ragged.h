/* libisic_hip.so -- the token statistics of isic_hip_moments.h (the reference's concat_patch_moments, utils.py:16-31) over
 * an arbitrary SUBSET of each image's tokens -- the lesion patches -- in two forms: flags on the dense grid, and offsets into
 * a compacted store.  Opt-in: isic_token_moments_f32 and its bits are untouched.  isic_hip/moments.py (token_moments with
 * `keep`, token_moments_ragged) calls them.  Included by isic_hip.h.
 *
 * Conventions as in isic_hip_moments.h and isic_hip_ragged.h: return 0 or a negative ISIC_ERR_* code, every argument is
 * checked before any device work, no allocation, no synchronisation, no read-back, `stream` last.  Every offset is 64-bit.
 * A value read from device memory (a node offset) is compared with the sizes passed by value before it is used as an index:
 * no argument VALUE makes a kernel read or write outside the arrays as their sizes are stated here.
 *
 * out is fp32: out[b ldo + s D + d] with s = 0..5 for mean, max, std, median, skewness, excess kurtosis (the reference's
 * order) of the n kept tokens of image (graph) b, channel d; the ldo - 6 D floats of padding of a row are not touched.
 * counts, int32 [B] or [G], may be NULL; otherwise counts[b] = n_b.  By the number n of kept tokens:
 *   n >= 1 (n >= 2 when unbiased)  the row is BIT FOR BIT what isic_token_moments_f32 returns for B = 1, T = n on a
 *                                   contiguous copy of the kept tokens in their order (ascending t; ascending row), wherever
 *                                   that entry is defined (finite inputs).
 *   n == 0                          all six statistics of every channel are quiet NaN and the count is 0.  (The reference
 *                                   raises on an empty token axis -- its max has no identity; NaN plus a count is this
 *                                   library's convention, so that one image without a lesion does not stop a batch.)
 *   n == 1 with unbiased            mean, max and median are the element; std, skewness and kurtosis are NaN -- what torch
 *                                   gives (std of one value is NaN, and clamp(min=eps) keeps a NaN).  The dense entry rejects
 *                                   this case by value; here n is a device fact.
 *
 * One launch per call.  A block of 256 threads takes one image (graph) and one slab of 64 channels, stages the kept tokens
 * into LDS as [n][64] floats (16-byte loads along D when ldx % 4 == 0 and X is 16-byte aligned, element loads otherwise) and
 * then runs the source text of the dense kernel (csrc/token_moments.inc) with the token count n.  T and max_nodes are at most
 * ISIC_MOMENTS_RAGGED_MAX_NODES = 256: up to 256 tokens the dense kernel always takes its 64-channel slab with four threads
 * per channel, so the summation order of an image depends on its own n alone -- not on T, max_nodes, B or the other
 * images.  (T and max_nodes only size the dynamic LDS, at most 64 KiB.)  The masked form finds n and the ascending list of
 * kept token ids with one thread per token: a ballot, a prefix popcount inside each wave and the four wave totals through
 * LDS -- a stable compaction, so the sums follow the compacted positions.  No floating-point atomics: two identical calls
 * give identical bits.
 *
 * ISIC_ERR_BAD_ARG: B / G, T / max_nodes or total negative, T < 1, D < 1, ldx < D, ldo < 6 D, eps negative or NaN, unbiased
 * not 0 or 1; with B or G > 0 a NULL X (ragged: unless total == 0), out, keep / node_offsets / bad; node_offsets not 8-byte
 * aligned, counts or bad not 4-byte aligned.  ISIC_ERR_UNSUPPORTED: T or max_nodes > ISIC_MOMENTS_RAGGED_MAX_NODES, or
 * B ceil(D / 64) blocks beyond 2^31 - 1.  B == 0 or G == 0 returns 0 without a launch. */
#ifndef ISIC_HIP_MOMENTS_RAGGED_H
#define ISIC_HIP_MOMENTS_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISIC_MOMENTS_RAGGED_MAX_NODES 256

/* Flags on the dense grid.  X as in isic_token_moments_f32: token t of image b, channel d, is X[(b T + t) ldx + d].
 * keep is uint8 [B][T], contiguous: non-zero keeps the token.  Image b has n_b kept tokens, in ascending t. */
int isic_token_moments_masked_f32(const float* X, const uint8_t* keep, int64_t B, int T, int D, int64_t ldx,
                                  float eps, int unbiased, float* out, int64_t ldo, int32_t* counts, void* stream);

/* Offsets into a compacted store.  Row i of the store is X[i ldx + d], `total` rows.  node_offsets is device int64 [G+1]:
 * graph g owns rows [node_offsets[g], node_offsets[g+1]).  max_nodes is the caller's bound on n_g; a result does not depend
 * on it.  bad is device uint32 [1], zeroed by the caller; the kernel only adds to it.  A graph is BAD if its offsets
 * decrease, leave [0, total] or span more than max_nodes: it writes nothing to out, sets counts[g] = 0 when counts is given,
 * adds 1 to bad[0] and does not disturb its neighbours. */
int isic_token_moments_ragged_f32(const float* X, const int64_t* node_offsets, int64_t G, int max_nodes,
                                  int64_t total, int D, int64_t ldx, float eps, int unbiased,
                                  float* out, int64_t ldo, int32_t* counts, uint32_t* bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ISIC_HIP_MOMENTS_RAGGED_H */
