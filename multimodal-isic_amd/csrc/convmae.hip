// The convolutional front of the ConvMAE-Base patch encoder (gfx950, fp16 activations, fp32 arithmetic inside): the
// depthwise 5x5 token mixer of a CBlock, the rows of the non-overlapping P x P patch convolutions (space-to-depth), and a
// LayerNorm over rows of up to 1024 channels with an optional erf-GELU and up to two fp16 addends.  Everything else of the
// encoder (1x1 convs, patch / decode convs, the ViT-B stage) is isic_gemm_f16* and isic_attention_f16.
// include/isic_hip_convmae.h declares the entry points; isic_hip/convmae.py composes them.

#include "common.h"

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
enum { DW_PLAIN = 0, DW_MASK_IN = 1, DW_MASK_OUT = 2 };

template <int MASK>
__global__ __launch_bounds__(256) void dwconv5x5_f16_kernel(const unsigned short* __restrict__ x,
                                                             const float* __restrict__ wt, const float* __restrict__ bias,
                                                             unsigned short* __restrict__ y, int H, int W, int C,
                                                             int tiles_w, int tiles_hw, const unsigned char* __restrict__ keep,
                                                             int P, unsigned short* __restrict__ xm) {
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

// ---------------------------------------------------------------- patch rows
// NHWC fp16 -> rows[(n, py, px)][kh][kw][c]: for a fixed kh the P*C values of a row are contiguous in x, so every 16-byte
// piece of a row is one 16-byte piece of x.
__global__ __launch_bounds__(256) void patch_rows_nhwc_kernel(const unsigned short* __restrict__ x,
                                                               unsigned short* __restrict__ rows, int H, int W, int C, int P,
                                                               int64_t nvec) {
  const int gh = H / P, gw = W / P, seg = P * C, kv = P * seg / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % kv) * 8;
    const int64_t row = i / kv;
    const int px = (int)(row % gw), py = (int)((row / gw) % gh);
    const int64_t n = row / ((int64_t)gw * gh);
    const int kh = k / seg, rem = k - kh * seg;
    const unsigned short* src = x + (((size_t)n * H + (size_t)(py * P + kh)) * W + (size_t)px * P) * C + rem;
    *reinterpret_cast<u32x4*>(rows + i * 8) = *reinterpret_cast<const u32x4*>(src);
  }
}

// NCHW fp32 -> the same rows, fp16, zero-padded to Kout columns; one thread gathers 8 values of a row
__global__ __launch_bounds__(256) void patch_rows_nchw_kernel(const float* __restrict__ img, unsigned short* __restrict__ rows,
                                                               int C, int H, int W, int P, int Kout, int64_t nvec) {
  const int gh = H / P, gw = W / P, K = C * P * P, kv = Kout / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
    const int k0 = (int)(i % kv) * 8;
    const int64_t row = i / kv;
    const int px = (int)(row % gw), py = (int)((row / gw) % gh);
    const int64_t n = row / ((int64_t)gw * gh);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      f[j] = 0.f;
      if (k < K) {
        const int c = k % C, kk = k / C, kh = kk / P, kw = kk - kh * P;
        f[j] = img[(((size_t)n * C + c) * H + (size_t)(py * P + kh)) * W + (size_t)px * P + kw];
      }
    }
    *reinterpret_cast<u32x4*>(rows + i * 8) = f16_pack8(f);
  }
}

// ---------------------------------------------------------------- LayerNorm of (x + a + b), optional GELU
// One wave per row, CPL 16-byte pieces per lane (N / 8 <= 64 CPL); four rows per block.  Two-pass statistics in fp32 on
// the values held in registers (the arithmetic of layernorm_f16_kernel).
template <int CPL>
__global__ __launch_bounds__(256) void layernorm_add_f16_kernel(const unsigned short* __restrict__ x,
                                                                 const unsigned short* __restrict__ a,
                                                                 const unsigned short* __restrict__ b,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta,
                                                                 unsigned short* __restrict__ y, float* __restrict__ y32,
                                                                 int64_t M, int N, int act, float eps) {
  const int lane = threadIdx.x & 63;
  const int pieces = N >> 3;
  const float invn = 1.f / (float)N;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < M; row += (int64_t)gridDim.x * 4) {
    float f[CPL][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int q = lane + 64 * i;
      const bool on = q < pieces;
      const size_t off = (size_t)row * N + (size_t)(on ? q : 0) * 8;
      f16_unpack8(*reinterpret_cast<const u32x4*>(x + off), f[i]);
      if (a) {
        float t[8];
        f16_unpack8(*reinterpret_cast<const u32x4*>(a + off), t);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[i][j] += t[j];
      }
      if (b) {
        float t[8];
        f16_unpack8(*reinterpret_cast<const u32x4*>(b + off), t);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[i][j] += t[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s += on ? f[i][j] : 0.f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    // a true division, not s * invn: the compiler fuses "f - s * invn" into one FMA with the product unrounded, and where
    // 1 / N is inexact (N = 768: 2 * 768 * fl(1 / 768) = 2 + 2^-24) a constant row no longer cancels to 0 -- times
    // rstd = 1 / sqrt(eps) that is 6e-5 in x^.  N c / N is exact for every row of equal values c.
    const float mean = s / (float)N;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const bool on = lane + 64 * i < pieces;
#pragma unroll
      for (int j = 0; j < 8; ++j) { f[i][j] -= mean; v += on ? f[i][j] * f[i][j] : 0.f; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const float rstd = rsqrtf(v * invn + eps);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int q = lane + 64 * i;
      if (q >= pieces) continue;
      const int col = q * 8;
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
      if (y) *reinterpret_cast<u32x4*>(y + off) = f16_pack8(o8);
      if (y32) {
        *reinterpret_cast<f32x4*>(y32 + off) = (f32x4){o8[0], o8[1], o8[2], o8[3]};
        *reinterpret_cast<f32x4*>(y32 + off + 4) = (f32x4){o8[4], o8[5], o8[6], o8[7]};
      }
    }
  }
}

int64_t cm_grid(int64_t work, int64_t per_block, int64_t cap) {
  int64_t g = (work + per_block - 1) / per_block;
  return g < 1 ? 1 : (g > cap ? cap : g);
}

}  // namespace

extern "C" {

int isic_dwconv5x5_f16(const uint16_t* x, const float* w_taps, const float* bias, uint16_t* y, int N, int H, int W, int C,
                       void* stream) {
  ISIC_CHECK_ARG(N >= 0 && H > 0 && W > 0 && C > 0);
  if (C % DW_CC != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && w_taps && y);
  const int tiles_w = (W + DW_TW - 1) / DW_TW, tiles_h = (H + DW_TH - 1) / DW_TH;
  const int64_t blocks = (int64_t)N * (C / DW_CC) * tiles_w * tiles_h;
  if (blocks > (int64_t)INT32_MAX) return ISIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(dwconv5x5_f16_kernel<DW_PLAIN>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, w_taps, bias, y,
                     H, W, C, tiles_w, tiles_w * tiles_h, nullptr, 1, nullptr);
  return isic_launch_status();
}

int isic_patch_rows_nhwc_f16(const uint16_t* x, uint16_t* rows, int N, int H, int W, int C, int P, void* stream) {
  ISIC_CHECK_ARG(N >= 0 && H > 0 && W > 0 && C > 0 && P > 0);
  if ((P != 2 && P != 4) || C % 8 != 0 || H % P != 0 || W % P != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && rows);
  const int64_t nvec = (int64_t)N * H * W * C / 8;
  hipLaunchKernelGGL(patch_rows_nhwc_kernel, dim3((unsigned)cm_grid(nvec, 256, 16384)), dim3(256), 0, as_stream(stream), x,
                     rows, H, W, C, P, nvec);
  return isic_launch_status();
}

int isic_patch_rows_nchw_f32(const float* images, uint16_t* rows, int N, int C, int H, int W, int P, int K_out,
                             void* stream) {
  ISIC_CHECK_ARG(N >= 0 && C > 0 && H > 0 && W > 0 && P > 0 && K_out > 0);
  if (K_out % 8 != 0 || K_out < C * P * P || H % P != 0 || W % P != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(images && rows);
  const int64_t nvec = (int64_t)N * (H / P) * (W / P) * (K_out / 8);
  hipLaunchKernelGGL(patch_rows_nchw_kernel, dim3((unsigned)cm_grid(nvec, 256, 16384)), dim3(256), 0, as_stream(stream),
                     images, rows, C, H, W, P, K_out, nvec);
  return isic_launch_status();
}

int isic_layernorm_add_f16(const uint16_t* x, const uint16_t* a, const uint16_t* b, const float* gamma, const float* beta,
                           uint16_t* y, float* y_f32, int64_t M, int N, int act, float eps, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && N > 0 && (act == 0 || act == 1) && eps >= 0.f);
  if (N % 64 != 0 || N > 1024) return ISIC_ERR_UNSUPPORTED;
  if (M == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && gamma && beta && (y || y_f32));
  const dim3 grid((unsigned)cm_grid(M, 4 * 4, 8192));
  if (N <= 512)
    hipLaunchKernelGGL(layernorm_add_f16_kernel<1>, grid, dim3(256), 0, as_stream(stream), x, a, b, gamma, beta, y, y_f32, M,
                       N, act, eps);
  else
    hipLaunchKernelGGL(layernorm_add_f16_kernel<2>, grid, dim3(256), 0, as_stream(stream), x, a, b, gamma, beta, y, y_f32, M,
                       N, act, eps);
  return isic_launch_status();
}

// include/isic_hip_mae.h
static int dwconv5x5_masked(int mode, const uint16_t* x, const uint8_t* keep, int P, const float* w_taps, const float* bias,
                            uint16_t* xm, uint16_t* y, int N, int H, int W, int C, void* stream) {
  ISIC_CHECK_ARG(N >= 0 && H > 0 && W > 0 && C > 0 && P > 0);
  if (C % DW_CC != 0 || H % P != 0 || W % P != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && keep && w_taps && y);
  const int tiles_w = (W + DW_TW - 1) / DW_TW, tiles_h = (H + DW_TH - 1) / DW_TH;
  const int64_t blocks = (int64_t)N * (C / DW_CC) * tiles_w * tiles_h;
  if (blocks > (int64_t)INT32_MAX) return ISIC_ERR_UNSUPPORTED;
  const unsigned char* k = reinterpret_cast<const unsigned char*>(keep);
  if (mode == DW_MASK_IN)
    hipLaunchKernelGGL(dwconv5x5_f16_kernel<DW_MASK_IN>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, w_taps, bias,
                       y, H, W, C, tiles_w, tiles_w * tiles_h, k, P, xm);
  else
    hipLaunchKernelGGL(dwconv5x5_f16_kernel<DW_MASK_OUT>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, w_taps,
                       bias, y, H, W, C, tiles_w, tiles_w * tiles_h, k, P, nullptr);
  return isic_launch_status();
}

int isic_dwconv5x5_masked_f16(const uint16_t* x, const uint8_t* keep, int P, const float* w_taps, const float* bias,
                              uint16_t* xm, uint16_t* y, int N, int H, int W, int C, void* stream) {
  return dwconv5x5_masked(DW_MASK_IN, x, keep, P, w_taps, bias, xm, y, N, H, W, C, stream);
}

int isic_dwconv5x5_masked_dgrad_f16(const uint16_t* dy, const uint8_t* keep, int P, const float* w_taps_rev, uint16_t* dx,
                                    int N, int H, int W, int C, void* stream) {
  return dwconv5x5_masked(DW_MASK_OUT, dy, keep, P, w_taps_rev, nullptr, nullptr, dx, N, H, W, C, stream);
}

}  // extern "C"
