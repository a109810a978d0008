// Kernel templates of the ConvMAE-Base convolutional front that csrc/convmae.hip (fp16 outputs) and csrc/convmae_mxfp8.hip
// (MXFP8 outputs, include/isic_hip_convmae_mxfp8.h) instantiate: the depthwise 5x5 and the row LayerNorm.  An MXFP8
// instantiation runs the arithmetic of the fp16 one and differs in its epilogue only.
// (An .inc, like mx_quant.inc: included by convmae.hip, convmae_mxfp8.hip and mxfp8.hip only, not one of the csrc/*.h that
// every kernel may see and that bench.py therefore stamps its PMC traffic profile with.)
#pragma once
#include "common.h"
#include "ln_rows.inc"       // ln_row_center; brings mx_quant.inc

namespace {

__device__ __forceinline__ float cm_gelu(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

// ---------------------------------------------------------------- depthwise 5x5
// One block = one image, a tile of DW_TH x DW_TW output pixels and 64 channels.  The input tile with its 2-pixel halo,
// (DW_TH + 4) x (DW_TW + 4) pixels x 128 bytes (45 KB), is staged once in LDS with 16-byte loads (zero outside the image);
// a thread then owns one output column and 8 channels and slides down the DW_TH rows: per kernel column kw it holds the
// five taps w[0..4][kw] and reads each of the DW_TH + 4 input pixels of its column once (16 bytes, ds_read_b128; a wave
// reads 1 KB contiguous), adding it into every output row it touches.  That is 5 (DW_TH + 4) LDS reads per DW_TH outputs
// instead of 25.  Tiles of 7 x 28 divide the 56 x 56 and 28 x 28 maps of ConvMAE-Base; other sizes take guarded edges.
constexpr int DW_TH = 7, DW_TW = 28, DW_CC = 64;
constexpr int DW_LR = DW_TH + 4, DW_LC = DW_TW + 4;                 // staged rows / columns
constexpr int DW_CHUNKS = DW_LR * DW_LC * (DW_CC / 8);             // 16-byte pieces in the tile
constexpr int DW_PER_T = (DW_CHUNKS + 255) / 256;

// MASK (the MAE's masked CBlock, include/isic_hip_mae.h): keep[n][(h / P) * (W / P) + w / P] flags the token a pixel lies
// in.  DW_MASK_IN zeroes the removed pixels of x as they are staged (and writes that masked input to xm for the weight
// gradient: every pixel is inside exactly one tile); DW_MASK_OUT zeroes the removed pixels of y (the data gradient).
// DW_PLAIN is isic_dwconv5x5_f16, instruction for instruction.
// DW_MX (include/isic_hip_convmae_mxfp8.h) is DW_PLAIN whose fp32 accumulators leave as MXFP8: the four lanes g = 4 b ..
// 4 b + 3 of an output column hold the 32-channel block b of each of its pixels; they pass the early return together (it
// depends on the column only) and the row guard is uniform over them, so the two shuffles of the block maximum stay
// outside it.  A lane writes its 8 element bytes to mq[pixel][C], the first of the four the scale to ms[pixel][C / 32].
enum { DW_PLAIN = 0, DW_MASK_IN = 1, DW_MASK_OUT = 2, DW_MX = 3 };

template <int MASK>
__global__ __launch_bounds__(256) void dwconv5x5_f16_kernel(const unsigned short* __restrict__ x,
                                                             const float* __restrict__ wt, const float* __restrict__ bias,
                                                             unsigned short* __restrict__ y, int H, int W, int C,
                                                             int tiles_w, int tiles_hw, const unsigned char* __restrict__ keep,
                                                             int P, unsigned short* __restrict__ xm,
                                                             unsigned char* __restrict__ mq, unsigned char* __restrict__ ms) {
  __shared__ __attribute__((aligned(16))) u32x4 tile[DW_LR * DW_LC * (DW_CC / 8)];
  const int tid = threadIdx.x;
  const int64_t bid = blockIdx.x;
  const int cchunks = C / DW_CC;
  const int t = (int)(bid % tiles_hw);
  const int cq = (int)((bid / tiles_hw) % cchunks);
  const int64_t n = bid / ((int64_t)tiles_hw * cchunks);
  const int h0 = (t / tiles_w) * DW_TH, w0 = (t % tiles_w) * DW_TW, c0 = cq * DW_CC;
  const unsigned short* xn = x + (size_t)n * H * W * C + c0;

  u32x4 v[DW_PER_T];
#pragma unroll
  for (int i = 0; i < DW_PER_T; ++i) {
    const int e = tid + 256 * i;
    const int pix = e >> 3, q = e & 7;
    const int h = h0 - 2 + pix / DW_LC, w = w0 - 2 + pix % DW_LC;
    v[i] = (u32x4){0u, 0u, 0u, 0u};
    if (e < DW_CHUNKS && h >= 0 && h < H && w >= 0 && w < W) {
      if (MASK != DW_MASK_IN || keep[n * (int64_t)((H / P) * (W / P)) + (h / P) * (W / P) + w / P])
        v[i] = *reinterpret_cast<const u32x4*>(xn + ((size_t)h * W + w) * C + q * 8);
      if (MASK == DW_MASK_IN && xm && pix / DW_LC >= 2 && pix / DW_LC < DW_TH + 2 && pix % DW_LC >= 2 && pix % DW_LC < DW_TW + 2)
        *reinterpret_cast<u32x4*>(xm + (size_t)n * H * W * C + c0 + ((size_t)h * W + w) * C + q * 8) = v[i];
    }
  }
#pragma unroll
  for (int i = 0; i < DW_PER_T; ++i) {
    const int e = tid + 256 * i;
    if (e < DW_CHUNKS) tile[e] = v[i];
  }
  __syncthreads();

  const int g = tid & 7, col = tid >> 3;                              // 8 channel groups x 32 columns (28 used)
  const int ow = w0 + col;
  if (col >= DW_TW || ow >= W) return;                                // no barrier after this point
  const int cb = c0 + g * 8;
  float acc[DW_TH][8];
  {
    float b0[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b0[j] = bias ? bias[cb + j] : 0.f;
#pragma unroll
    for (int r = 0; r < DW_TH; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[r][j] = b0[j];
  }
#pragma unroll 1
  for (int kw = 0; kw < 5; ++kw) {                                     // rolled: 56 accumulators + 40 taps stay in registers
    float wk[5][8];
#pragma unroll
    for (int kh = 0; kh < 5; ++kh) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(wt + (size_t)(kh * 5 + kw) * C + cb);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(wt + (size_t)(kh * 5 + kw) * C + cb + 4);
      wk[kh][0] = lo[0]; wk[kh][1] = lo[1]; wk[kh][2] = lo[2]; wk[kh][3] = lo[3];
      wk[kh][4] = hi[0]; wk[kh][5] = hi[1]; wk[kh][6] = hi[2]; wk[kh][7] = hi[3];
    }
#pragma unroll
    for (int r = 0; r < DW_LR; ++r) {
      float f[8];
      f16_unpack8(tile[(r * DW_LC + col + kw) * 8 + g], f);
#pragma unroll
      for (int kh = 0; kh < 5; ++kh) {
        const int oh = r - kh;                                         // compile-time after unrolling
        if (oh < 0 || oh >= DW_TH) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[oh][j] = fmaf(wk[kh][j], f[j], acc[oh][j]);
      }
    }
  }
  if (MASK == DW_MX) {
    const size_t pix0 = (size_t)n * H * W + (size_t)h0 * W + ow;
#pragma unroll
    for (int r = 0; r < DW_TH; ++r) {
      unsigned char scale;
      const u32x2 o = mx_block8(acc[r], scale);
      if (h0 + r < H) {
        const size_t pix = pix0 + (size_t)r * W;
        *reinterpret_cast<u32x2*>(mq + pix * C + cb) = o;
        if ((g & 3) == 0) ms[pix * (C >> 5) + (cb >> 5)] = scale;
      }
    }
    return;
  }
  unsigned short* yp = y + ((size_t)n * H * W + (size_t)h0 * W + ow) * C + cb;
#pragma unroll
  for (int r = 0; r < DW_TH; ++r)
    if (h0 + r < H) {
      if (MASK == DW_MASK_OUT && !keep[n * (int64_t)((H / P) * (W / P)) + ((h0 + r) / P) * (W / P) + ow / P])
        *reinterpret_cast<u32x4*>(yp + (size_t)r * W * C) = (u32x4){0u, 0u, 0u, 0u};
      else
        *reinterpret_cast<u32x4*>(yp + (size_t)r * W * C) = f16_pack8(acc[r]);
    }
}

// ---------------------------------------------------------------- LayerNorm of (x + a + b), optional GELU
// One wave per row, CPL 16-byte pieces per lane (N / 8 <= 64 CPL); four rows per block.  Two-pass statistics in fp32 on
// the values held in registers: ln_row_center (csrc/ln_rows.inc), the text the ViT-width layernorm_f16_kernel runs too, here
// with the mean as a true division (LN_MEAN_DIV, explained there).
// MX (include/isic_hip_convmae_mxfp8.h): no addends, and the fp32 values y32 would receive are quantised to MXFP8 instead
// -- lanes 4 k .. 4 k + 3 hold the 32-element block lane / 4 + 16 i of the row, and N % 64 == 0 switches those four lanes
// on or off together; mq[M][N] takes the element bytes, ms[M][N / 32] the scales.
template <int CPL, bool MX = false>
__global__ __launch_bounds__(256) void layernorm_add_f16_kernel(const unsigned short* __restrict__ x,
                                                                 const unsigned short* __restrict__ a,
                                                                 const unsigned short* __restrict__ b,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta,
                                                                 unsigned short* __restrict__ y, float* __restrict__ y32,
                                                                 int64_t M, int N, int act, float eps,
                                                                 unsigned char* __restrict__ mq = nullptr,
                                                                 unsigned char* __restrict__ ms = nullptr) {
  const int lane = threadIdx.x & 63;
  const int pieces = N >> 3;
  const float invn = 1.f / (float)N;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * 4) {
    float f[CPL][8], mean, rstd;
    ln_row_center<64, CPL, LN_MEAN_DIV>(x, a, b, (size_t)row * N, lane, pieces, N, invn, eps, f, mean, rstd);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int q = lane + 64 * i;
      if (!MX && q >= pieces) continue;
      const int col = (q < pieces ? q : 0) * 8;
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + col), g1 = *reinterpret_cast<const f32x4*>(gamma + col + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + col), b1 = *reinterpret_cast<const f32x4*>(beta + col + 4);
      const float gg[8] = {g0[0], g0[1], g0[2], g0[3], g1[0], g1[1], g1[2], g1[3]};
      const float bb[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
      float o8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float t = f[i][j] * rstd * gg[j] + bb[j];
        o8[j] = act ? cm_gelu(t) : t;
      }
      const size_t off = (size_t)row * N + col;
      if (MX) {                                                        // every lane reaches the shuffles
        unsigned char scale;
        const u32x2 o = mx_block8(o8, scale);
        if (q < pieces) {
          *reinterpret_cast<u32x2*>(mq + off) = o;
          if ((lane & 3) == 0) ms[(size_t)row * (N >> 5) + (q >> 2)] = scale;
        }
        continue;
      }
      if (y) *reinterpret_cast<u32x4*>(y + off) = f16_pack8(o8);
      if (y32) {
        *reinterpret_cast<f32x4*>(y32 + off) = (f32x4){o8[0], o8[1], o8[2], o8[3]};
        *reinterpret_cast<f32x4*>(y32 + off + 4) = (f32x4){o8[4], o8[5], o8[6], o8[7]};
      }
    }
  }
}

static inline int64_t cm_grid(int64_t work, int64_t per_block, int64_t cap) {
  int64_t g = (work + per_block - 1) / per_block;
  return g < 1 ? 1 : (g > cap ? cap : g);
}

}  // namespace
