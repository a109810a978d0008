// The batch transform of the MAE fine-tune (include/isic_hip_augment.h): crop + bilinear resize + flips + rot90 + normalise
// from a ragged uint8 pool, one launch per batch.
//
// Memory-bound: 16 output bytes per pixel (three image channels and the mask, fp32) against at most 4 source bytes.  A
// workgroup of 256 threads owns a 32 x 32 tile of one output image; thread (ty, tx) writes pixels (ty, 4 tx .. 4 tx + 3) of
// each plane with one 16-byte store, so every store instruction of a wave covers 8 rows x 128 B.  A 2-D tile keeps the
// source footprint compact when k is odd and consecutive output columns walk source rows: 32 x 32 outputs read one patch
// of about (32 ch / S) x (32 cw / S) source pixels whatever the rotation, not 32 whole source rows.
//
// The coordinates are separable.  Output pixel (i, j) maps to pixel (r, c) of the resized crop with r a function of i alone
// and c of j alone when k is even, and r of j and c of i when k is odd.  The first 64 threads work out the taps and weights
// of the tile's 32 rows and 32 columns once (the only integer divisions of the kernel) and leave them in LDS.
#include "common.h"

namespace {

constexpr int AUG_TILE = 32;                 // output tile side; 8 threads x 4 pixels across, 32 threads down
constexpr int AUG_MAX_SIDE = 1 << 20;        // crop sides are clamped to this: (2 r + 1) n stays below 2^31 for r < 1024

struct AxisTap {
  int i0, i1, nn;                            // bilinear taps and the nearest-neighbour index, relative to the crop
  float w;                                   // weight of i1
};

// index r of the resized axis (length S) over a crop axis of length n
__device__ __forceinline__ AxisTap axis_tap(int r, int n, int S) {
  const unsigned twoS = 2u * (unsigned)S;
  const unsigned full = (2u * (unsigned)r + 1u) * (unsigned)n;
  const unsigned num = full > (unsigned)S ? full - (unsigned)S : 0u;
  const unsigned q = num / twoS;
  AxisTap t;
  t.i0 = min((int)q, n - 1);
  t.i1 = min(t.i0 + 1, n - 1);
  t.w = (float)(num - q * twoS) / (float)twoS;
  t.nn = min((int)(((unsigned long long)r * (unsigned)n) / (unsigned)S), n - 1);
  return t;
}

struct AugNorm {
  float scale[3], bias[3];                   // (v / 255 - mean) / std = v * scale + bias
};

__global__ __launch_bounds__(256) void augment_u8_kernel(const uint8_t* __restrict__ pixels, const uint8_t* __restrict__ masks,
                                                         const int64_t* __restrict__ offsets, const int32_t* __restrict__ hw,
                                                         int64_t n_pool, const int64_t* __restrict__ index,
                                                         const int32_t* __restrict__ box, const int32_t* __restrict__ op,
                                                         AugNorm norm, float* __restrict__ image_out,
                                                         float* __restrict__ mask_out, int S, int tiles_x, int tiles) {
  __shared__ AxisTap tap_row[AUG_TILE], tap_col[AUG_TILE];      // of output rows i / output columns j of this tile
  const int64_t b = blockIdx.x / tiles;
  const int t = (int)(blockIdx.x - b * tiles);
  const int ti = (t / tiles_x) * AUG_TILE, tj = (t % tiles_x) * AUG_TILE;

  int64_t n = index[b];
  n = n < 0 ? 0 : (n >= n_pool ? n_pool - 1 : n);
  const int h = hw[2 * n], w = hw[2 * n + 1];
  const bool empty = h <= 0 || w <= 0;
  const int y0 = empty ? 0 : min(max(box[4 * b], 0), h - 1);
  const int x0 = empty ? 0 : min(max(box[4 * b + 1], 0), w - 1);
  const int ch = empty ? 1 : min(min(max(box[4 * b + 2], 1), h - y0), AUG_MAX_SIDE);
  const int cw = empty ? 1 : min(min(max(box[4 * b + 3], 1), w - x0), AUG_MAX_SIDE);
  const int code = op[b];
  const bool hflip = code & 1, vflip = code & 2;
  const int k = (code >> 2) & 3;
  const bool odd = k & 1;

  // Undo rot90(k), then vflip / hflip.  V = vflip(hflip(R)); out = rot90(V, k):
  //   k = 0: out[i][j] = V[i][j]          k = 1: V[j][S-1-i]          k = 2: V[S-1-i][S-1-j]          k = 3: V[S-1-j][i]
  // so the row of V comes from i (k even) or j (k odd), mirrored for k = 2, 3, and its column from the other index,
  // mirrored for k = 1, 2.  Thread u < 32 serves output row ti + u, thread 32 + u output column tj + u.
  if (threadIdx.x < 2 * AUG_TILE) {
    const bool is_col = threadIdx.x >= AUG_TILE;                 // an output column index j
    const int u = threadIdx.x & (AUG_TILE - 1);
    const int o = min((is_col ? tj : ti) + u, S - 1);
    const bool to_row = is_col == odd;                           // this output index selects a row of V
    const bool mirror = to_row ? (k >= 2) : (k == 1 || k == 2);
    int v = mirror ? S - 1 - o : o;
    if (to_row ? vflip : hflip) v = S - 1 - v;
    const AxisTap a = axis_tap(v, to_row ? ch : cw, S);
    (is_col ? tap_col : tap_row)[u] = a;
  }
  __syncthreads();

  const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
  const int i = ti + ty, j = tj + 4 * tx;
  if (i >= S || j >= S) return;
  const int64_t plane = (int64_t)S * S;
  float* img = image_out + (b * 3 * plane + (int64_t)i * S + j);
  float* msk = mask_out ? mask_out + (b * plane + (int64_t)i * S + j) : nullptr;
  const bool vec = (S & 3) == 0;                                 // then j + 3 < S and every row start is 16-byte aligned

  float out[4][4];                                               // [channel or mask][pixel]
  if (empty) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int p = 0; p < 4; ++p) out[c][p] = 0.f;
  } else {
    const int64_t base = offsets[n] + (int64_t)y0 * w + x0;      // pixel index of the crop's corner
    const AxisTap ri = tap_row[ty];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const AxisTap cj = tap_col[min(4 * tx + p, AUG_TILE - 1)];
      const AxisTap& ry = odd ? cj : ri;                         // source rows
      const AxisTap& cx = odd ? ri : cj;                         // source columns
      const int64_t r0 = base + (int64_t)ry.i0 * w, r1 = base + (int64_t)ry.i1 * w;
      const uint8_t* p00 = pixels + 3 * (r0 + cx.i0);
      const uint8_t* p01 = pixels + 3 * (r0 + cx.i1);
      const uint8_t* p10 = pixels + 3 * (r1 + cx.i0);
      const uint8_t* p11 = pixels + 3 * (r1 + cx.i1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float a00 = (float)p00[c], a01 = (float)p01[c], a10 = (float)p10[c], a11 = (float)p11[c];
        const float top = a00 + cx.w * (a01 - a00);
        const float bot = a10 + cx.w * (a11 - a10);
        const float v = top + ry.w * (bot - top);
        out[c][p] = v * norm.scale[c] + norm.bias[c];
      }
      out[3][p] = msk ? (float)masks[base + (int64_t)ry.nn * w + cx.nn] : 0.f;
    }
  }

  if (vec) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const f32x4 v = {out[c][0], out[c][1], out[c][2], out[c][3]};
      *reinterpret_cast<f32x4*>(img + c * plane) = v;
    }
    if (msk) {
      const f32x4 v = {out[3][0], out[3][1], out[3][2], out[3][3]};
      *reinterpret_cast<f32x4*>(msk) = v;
    }
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (j + p >= S) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) img[c * plane + p] = out[c][p];
      if (msk) msk[p] = out[3][p];
    }
  }
}

}  // namespace

extern "C" int isic_augment_u8(const uint8_t* pixels, const uint8_t* masks, const int64_t* offsets, const int32_t* hw,
                               int64_t n_pool, const int64_t* index, const int32_t* box, const int32_t* op, float mean0,
                               float mean1, float mean2, float std0, float std1, float std2, float* image_out, float* mask_out,
                               int64_t B, int S, void* stream) {
  ISIC_CHECK_ARG(B >= 0 && S >= 1 && S <= 1024);
  ISIC_CHECK_ARG(std0 != 0.f && std1 != 0.f && std2 != 0.f);
  ISIC_CHECK_ARG(!(mask_out && !masks));
  if (B == 0) return ISIC_OK;
  ISIC_CHECK_ARG(n_pool >= 1 && pixels && offsets && hw && index && box && op && image_out);
  const int tiles_x = ceil_div(S, AUG_TILE), tiles = tiles_x * tiles_x;
  ISIC_CHECK_ARG(B <= (int64_t)0x7fffffff / tiles);
  const float mean[3] = {mean0, mean1, mean2}, stdv[3] = {std0, std1, std2};
  AugNorm norm;
  for (int c = 0; c < 3; ++c) {
    norm.scale[c] = (float)(1.0 / (255.0 * (double)stdv[c]));
    norm.bias[c] = (float)(-(double)mean[c] / (double)stdv[c]);
  }
  hipLaunchKernelGGL(augment_u8_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, as_stream(stream), pixels, masks, offsets, hw,
                     n_pool, index, box, op, norm, image_out, mask_out, S, tiles_x, tiles);
  return isic_launch_status();
}
