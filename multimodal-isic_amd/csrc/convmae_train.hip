// Backward of the convolutional front of the ConvMAE-Base patch encoder (gfx950, fp16 activations, fp32 arithmetic and
// gradients): the depthwise 5x5 weight / bias gradient, the backward of the LayerNorm of (x + a + b) with its optional
// GELU, and depth-to-space (the adjoint of the patch rows).  Everything else of the backward is the transformer-block
// backward (vit_train.hip) and gemm_f16; that one in turn takes its LayerNorm backward from here, for all three trainable
// encoders (isic_hip/transformer.py).  Entry points: include/isic_hip_convmae_train.h; the Python side is
// isic_hip/convmae.py (trainable=True).
//
// Every reduction that lands in a parameter gradient goes into fp32 slabs, one per block, that a second pass adds in a
// fixed order and multiplies by `scale`: no float atomics, so the backward is bit-reproducible.

#include "common.h"
#include "ln_rows.inc"
#include "slab_sum.inc"

namespace {

// d/dt of 0.5 t (1 + erf(t / sqrt 2)) = Phi(t) + t phi(t)
__device__ __forceinline__ float ct_dgelu(float t) {
  return 0.5f * (1.f + erff(t * 0.70710678118654752f)) + t * 0.39894228040143268f * __expf(-0.5f * t * t);
}

int64_t ct_grid(int64_t work, int64_t per_block, int64_t cap) {
  int64_t g = (work + per_block - 1) / per_block;
  return g < 1 ? 1 : (g > cap ? cap : g);
}

// ---------------------------------------------------------------- slab reducer
// slab[S][n]: i < n_split -> out_a[i], else out_b[i - n_split] (skipped when out_b is NULL); (+)= scale * sum over the S
// slabs, in the fixed order B of slab_sum.inc on scalars with four accumulators: a block covers 16 outputs with 16 threads
// each, 16 x 4 loads in flight per output instead of a chain of S dependent ones (512 slabs of the LayerNorm backward took
// 112 us per call that way).

__global__ __launch_bounds__(256) void ct_slab_reduce_kernel(const float* __restrict__ slab, int S, int64_t n,
                                                             int64_t n_split, float* out_a, float* out_b, float scale,
                                                             int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const float s = isic_slab_sum_lds16<4>(slab, (size_t)i, S, (size_t)n, i < n);
  if (threadIdx.x >= 16 || i >= n) return;
  float* out = i < n_split ? out_a + i : (out_b ? out_b + (i - n_split) : nullptr);
  if (out) *out = accumulate ? fmaf(scale, s, *out) : scale * s;
}

int ct_slab_reduce(const float* slab, int S, int64_t n, int64_t n_split, float* a, float* b, float scale, int accumulate,
                   hipStream_t st) {
  hipLaunchKernelGGL(ct_slab_reduce_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st,
                     slab, S, n, n_split, a, b, scale, accumulate);
  return isic_launch_status();
}

// ---------------------------------------------------------------- depthwise 5x5 weight / bias gradient
// Block (z, cq): 64 channels cq*64.. over the output tiles z, z + S, z + 2S, ... (tiles of DG_TH x DG_TW pixels of one
// image).  Per tile the input with its 2-pixel halo, (DG_TH + 4) x (DG_TW + 4) pixels x 128 bytes (18 KB), is staged
// once in LDS with 16-byte loads (zeros outside the image), as in the forward.  A thread owns one output column and 4
// channels: it loads dy of its DG_TH pixels (8 bytes each) into registers, then reads each of the (DG_TH + 4) x 5 input
// pixels its taps touch once from LDS (ds_read_b64; a wave reads 4 neighbouring pixels = 512 contiguous bytes) and adds
// dy x into every tap that pairs them.  The 25 x 4 tap sums (and 4 bias sums) stay in registers across all the block's
// tiles; at the end the 14 column threads are added (shuffles inside a wave, then the four waves in LDS, in index order)
// and the block writes one slab [26][C] (25 taps, then the bias).  Tiles of 4 x 14 divide the 56 x 56 and 28 x 28 maps of
// ConvMAE-Base; other sizes take guarded edges (dy = 0 outside the image).  Taller tiles stage less halo but hold more dy
// rows in registers: 7 rows already took 256 VGPRs + 46 AGPRs (one wave per SIMD), 4 rows take 228 (two).
constexpr int DG_TH = 4, DG_TW = 14, DG_CC = 64;
constexpr int DG_LR = DG_TH + 4, DG_LC = DG_TW + 4;                  // staged rows / columns
constexpr int DG_CHUNKS = DG_LR * DG_LC * (DG_CC / 8);              // 16-byte pieces in the tile
constexpr int DG_PER_T = (DG_CHUNKS + 255) / 256;
constexpr int DG_TAPS = 26;                                          // 25 taps + the bias
constexpr int DG_TARGET_BLOCKS = 1024;
constexpr int DG_RED = 4 * DG_TAPS * DG_CC / 4;                     // the wave sums [4][26][64] fp32, in 16-byte units
constexpr int DG_LDS = DG_CHUNKS > DG_RED ? DG_CHUNKS : DG_RED;

struct DgPlan { int S; int tiles_w; int tiles_hw; int64_t tiles; };
DgPlan dg_plan(int N, int H, int W, int C) {
  DgPlan p;
  p.tiles_w = (W + DG_TW - 1) / DG_TW;
  p.tiles_hw = p.tiles_w * ((H + DG_TH - 1) / DG_TH);
  p.tiles = (int64_t)N * p.tiles_hw;
  const int chunks = C / DG_CC;
  int64_t S = (DG_TARGET_BLOCKS + chunks - 1) / chunks;
  if (S > p.tiles) S = p.tiles;
  if (S < 1) S = 1;
  p.S = (int)S;
  return p;
}

__global__ __launch_bounds__(256) void dwconv5x5_wgrad_f16_kernel(const unsigned short* __restrict__ x,
                                                                   const unsigned short* __restrict__ dy,
                                                                   float* __restrict__ slab, int H, int W, int C,
                                                                   int tiles_w, int tiles_hw, int64_t tiles, int S) {
  __shared__ __attribute__((aligned(16))) u32x4 tile[DG_LDS];
  const int tid = threadIdx.x;
  const int z = blockIdx.x, cq = blockIdx.y, c0 = cq * DG_CC;
  const int g = tid & 15, col = tid >> 4;                              // 16 channel groups of 4 x 16 columns (14 used)
  const int colr = col < DG_TW ? col : DG_TW - 1;                      // idle columns read inside the tile (their dy is 0)
  float acc[25][4], accb[4];
#pragma unroll
  for (int t = 0; t < 25; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) accb[j] = 0.f;

  for (int64_t t = z; t < tiles; t += S) {
    const int64_t n = t / tiles_hw;
    const int tt = (int)(t - n * tiles_hw);
    const int h0 = (tt / tiles_w) * DG_TH, w0 = (tt % tiles_w) * DG_TW;
    const unsigned short* xn = x + (size_t)n * H * W * C + c0;
    const unsigned short* dyn = dy + (size_t)n * H * W * C + c0;
    __syncthreads();                                                   // the previous tile's LDS reads are done
#pragma unroll
    for (int i = 0; i < DG_PER_T; ++i) {
      const int e = tid + 256 * i;
      const int pix = e >> 3, q = e & 7;
      const int h = h0 - 2 + pix / DG_LC, w = w0 - 2 + pix % DG_LC;
      u32x4 v = (u32x4){0u, 0u, 0u, 0u};
      if (e < DG_CHUNKS && h >= 0 && h < H && w >= 0 && w < W)
        v = *reinterpret_cast<const u32x4*>(xn + ((size_t)h * W + w) * C + q * 8);
      if (e < DG_CHUNKS) tile[e] = v;
    }
    float d[DG_TH][4];
    const int ow = w0 + col;
#pragma unroll
    for (int r = 0; r < DG_TH; ++r) {
      u32x2 u = (u32x2){0u, 0u};
      if (col < DG_TW && ow < W && h0 + r < H)
        u = *reinterpret_cast<const u32x2*>(dyn + ((size_t)(h0 + r) * W + ow) * C + g * 4);
      f16_unpack2(u[0], d[r][0], d[r][1]);
      f16_unpack2(u[1], d[r][2], d[r][3]);
    }
    __syncthreads();
    const unsigned short* ts = reinterpret_cast<const unsigned short*>(tile);
#pragma unroll
    for (int r = 0; r < DG_LR; ++r) {
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) {
        const u32x2 u = *reinterpret_cast<const u32x2*>(ts + (size_t)(r * DG_LC + colr + kw) * DG_CC + g * 4);
        float f[4];
        f16_unpack2(u[0], f[0], f[1]);
        f16_unpack2(u[1], f[2], f[3]);
#pragma unroll
        for (int kh = 0; kh < 5; ++kh) {
          const int oh = r - kh;                                       // compile-time after unrolling
          if (oh < 0 || oh >= DG_TH) continue;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[kh * 5 + kw][j] = fmaf(d[oh][j], f[j], acc[kh * 5 + kw][j]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);                               // keep the LDS reads row by row (registers)
    }
#pragma unroll
    for (int r = 0; r < DG_TH; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) accb[j] += d[r][j];
  }
  // the 4 columns of a wave (lane = 16 * column + channel group), then the 4 waves
#pragma unroll
  for (int o = 16; o < 64; o <<= 1) {
#pragma unroll
    for (int t = 0; t < 25; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t][j] += __shfl_xor(acc[t][j], o);
#pragma unroll
    for (int j = 0; j < 4; ++j) accb[j] += __shfl_xor(accb[j], o);
  }
  __syncthreads();                                                     // the tile's LDS is reused for the wave sums
  float* red = reinterpret_cast<float*>(tile);                         // [4 waves][26][64]
  const int lane = tid & 63, wave = tid >> 6;
  if (lane < 16) {
#pragma unroll
    for (int t = 0; t < 25; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[(wave * DG_TAPS + t) * DG_CC + g * 4 + j] = acc[t][j];
#pragma unroll
    for (int j = 0; j < 4; ++j) red[(wave * DG_TAPS + 25) * DG_CC + g * 4 + j] = accb[j];
  }
  __syncthreads();
  for (int i = tid; i < DG_TAPS * DG_CC; i += 256) {
    const int tap = i / DG_CC, ch = i - tap * DG_CC;
    const float s = ((red[i] + red[DG_TAPS * DG_CC + i]) + red[2 * DG_TAPS * DG_CC + i]) + red[3 * DG_TAPS * DG_CC + i];
    slab[((int64_t)z * DG_TAPS + tap) * C + c0 + ch] = s;
  }
}

// ---------------------------------------------------------------- LayerNorm of (x + a + b) (+ GELU): backward
// One wave per row with the forward's layout (lane l holds the 16-byte pieces l + 64 i, i < CPL) and the forward's text
// for the statistics (ln_row_center, csrc/ln_rows.inc: the same sums in the same order, the mean a true division).  The
// compiler contracts multiply-adds per kernel, so the recomputed (mean, rstd) may differ from the forward's in the last
// bit; tests/test_ln_rows_gpu.py pins both.  Rows are split over a fixed grid of blocks in contiguous chunks; a lane
// keeps its columns' partial (sum dy x^, sum dy) over its wave's rows, the four waves are added in LDS in index order and
// each block writes one slab [2][N].
constexpr int LA_BLOCKS = 512;

struct LaPlan { int G; int64_t chunk; };
LaPlan la_plan(int64_t M) {
  int64_t G = (M + 63) / 64;
  if (G > LA_BLOCKS) G = LA_BLOCKS;
  if (G < 1) G = 1;
  const int64_t chunk = (M + G - 1) / G;
  return {(int)((M + chunk - 1) / chunk), chunk};
}

template <int CPL>
__global__ __launch_bounds__(256) void layernorm_add_bwd_f16_kernel(const void* __restrict__ dy_, int dy_f32, float dy_mul,
                                                                     const unsigned short* __restrict__ x,
                                                                     const unsigned short* __restrict__ a,
                                                                     const unsigned short* __restrict__ b,
                                                                     const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, int act, float eps,
                                                                     const float* g_in, float* g_out,
                                                                     unsigned short* g_out16, int64_t M, int N,
                                                                     int64_t chunk, float* __restrict__ slab) {
  __shared__ float red[4][2][64 * 8 * CPL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pieces = N >> 3;
  const float invn = 1.f / (float)N;
  float gam[CPL][8], bet[CPL][8], pg[CPL][8], pb[CPL][8];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int q = lane + 64 * i;
    const int col = (q < pieces ? q : 0) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      gam[i][j] = gamma[col + j];
      bet[i][j] = beta[col + j];
      pg[i][j] = 0.f;
      pb[i][j] = 0.f;
    }
  }
  const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = min(M, r0 + chunk);
  for (int64_t row = r0 + wave; row < r1; row += 4) {
    // ---- the forward's statistics: the same text and mean rule as layernorm_add_f16_kernel (ln_row_center)
    float f[CPL][8], mean, rstd;
    ln_row_center<64, CPL, LN_MEAN_DIV>(x, a, b, (size_t)row * N, lane, pieces, N, invn, eps, f, mean, rstd);
    // ---- backward: f becomes x^, d the (GELU-differentiated) incoming gradient
    float d[CPL][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int q = lane + 64 * i;
      const bool on = q < pieces;
      const size_t off = (size_t)row * N + (size_t)(on ? q : 0) * 8;
      if (dy_f32) {
        const float* p = reinterpret_cast<const float*>(dy_) + off;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
        d[i][0] = lo[0]; d[i][1] = lo[1]; d[i][2] = lo[2]; d[i][3] = lo[3];
        d[i][4] = hi[0]; d[i][5] = hi[1]; d[i][6] = hi[2]; d[i][7] = hi[3];
      } else {
        f16_unpack8(*reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned short*>(dy_) + off), d[i]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = f[i][j] * rstd;
        f[i][j] = xh;
        float dd = on ? d[i][j] * dy_mul : 0.f;
        if (act) dd *= ct_dgelu(xh * gam[i][j] + bet[i][j]);
        d[i][j] = dd;
        pg[i][j] = fmaf(dd, xh, pg[i][j]);
        pb[i][j] += dd;
        const float gh = dd * gam[i][j];
        s1 += gh;
        s2 = fmaf(gh, xh, s2);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o); s2 += __shfl_xor(s2, o); }
    const float m1 = s1 * invn, m2 = s2 * invn;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int q = lane + 64 * i;
      if (q >= pieces) continue;
      const size_t off = (size_t)row * N + (size_t)q * 8;
      float o8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o8[j] = rstd * (d[i][j] * gam[i][j] - m1 - f[i][j] * m2);
      if (g_in) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(g_in + off), hi = *reinterpret_cast<const f32x4*>(g_in + off + 4);
        o8[0] += lo[0]; o8[1] += lo[1]; o8[2] += lo[2]; o8[3] += lo[3];
        o8[4] += hi[0]; o8[5] += hi[1]; o8[6] += hi[2]; o8[7] += hi[3];
      }
      if (g_out) {
        *reinterpret_cast<f32x4*>(g_out + off) = (f32x4){o8[0], o8[1], o8[2], o8[3]};
        *reinterpret_cast<f32x4*>(g_out + off + 4) = (f32x4){o8[4], o8[5], o8[6], o8[7]};
      }
      if (g_out16) *reinterpret_cast<u32x4*>(g_out16 + off) = f16_pack8(o8);
    }
  }
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int q = lane + 64 * i;
    if (q >= pieces) continue;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[wave][0][q * 8 + j] = pg[i][j];
      red[wave][1][q * 8 + j] = pb[i][j];
    }
  }
  __syncthreads();
  for (int i = tid; i < 2 * N; i += 256) {
    const int which = i / N, col = i - which * N;
    const float t = ((red[0][which][col] + red[1][which][col]) + red[2][which][col]) + red[3][which][col];
    slab[((int64_t)blockIdx.x * 2 + which) * N + col] = t;
  }
}

// ---------------------------------------------------------------- depth-to-space
// One thread per 16-byte piece of drows (8 channels of one (kh, kw) of one patch row); for a fixed kh the P*C values of a
// row are contiguous in dx, as in patch_rows_nhwc_kernel.
__global__ __launch_bounds__(256) void patch_rows_bwd_kernel(const unsigned short* __restrict__ drows, float* __restrict__ dx,
                                                              unsigned short* __restrict__ dx16, int H, int W, int C, int P,
                                                              int accumulate, int64_t nvec) {
  const int gh = H / P, gw = W / P, seg = P * C, kv = P * seg / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % kv) * 8;
    const int64_t row = i / kv;
    const int px = (int)(row % gw), py = (int)((row / gw) % gh);
    const int64_t n = row / ((int64_t)gw * gh);
    const int kh = k / seg, rem = k - kh * seg;
    const size_t off = (((size_t)n * H + (size_t)(py * P + kh)) * W + (size_t)px * P) * C + rem;
    float f[8];
    f16_unpack8(*reinterpret_cast<const u32x4*>(drows + i * 8), f);
    if (accumulate) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(dx + off), hi = *reinterpret_cast<const f32x4*>(dx + off + 4);
      f[0] += lo[0]; f[1] += lo[1]; f[2] += lo[2]; f[3] += lo[3];
      f[4] += hi[0]; f[5] += hi[1]; f[6] += hi[2]; f[7] += hi[3];
    }
    *reinterpret_cast<f32x4*>(dx + off) = (f32x4){f[0], f[1], f[2], f[3]};
    *reinterpret_cast<f32x4*>(dx + off + 4) = (f32x4){f[4], f[5], f[6], f[7]};
    if (dx16) *reinterpret_cast<u32x4*>(dx16 + off) = f16_pack8(f);
  }
}

}  // namespace

extern "C" {

size_t isic_dwconv5x5_wgrad_f16_workspace_bytes(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % DG_CC != 0) return 0;
  return (size_t)dg_plan(N, H, W, C).S * DG_TAPS * C * sizeof(float);
}

int isic_dwconv5x5_wgrad_f16(const uint16_t* x, const uint16_t* dy, float* dw_taps, float* db, int N, int H, int W, int C,
                             float scale, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(N >= 0 && H > 0 && W > 0 && C > 0 && (accumulate == 0 || accumulate == 1));
  if (C % DG_CC != 0) return ISIC_ERR_UNSUPPORTED;
  ISIC_CHECK_ARG(dw_taps && (N == 0 || (x && dy)));
  hipStream_t st = as_stream(stream);
  if (N == 0) {                                        // an empty sum: zero, or nothing to add
    if (accumulate) return ISIC_OK;
    if (hipMemsetAsync(dw_taps, 0, (size_t)25 * C * sizeof(float), st) != hipSuccess) return ISIC_ERR_LAUNCH;
    if (db && hipMemsetAsync(db, 0, (size_t)C * sizeof(float), st) != hipSuccess) return ISIC_ERR_LAUNCH;
    return ISIC_OK;
  }
  if (!workspace || workspace_bytes < isic_dwconv5x5_wgrad_f16_workspace_bytes(N, H, W, C)) return ISIC_ERR_WORKSPACE;
  const DgPlan p = dg_plan(N, H, W, C);
  float* slab = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(dwconv5x5_wgrad_f16_kernel, dim3((unsigned)p.S, (unsigned)(C / DG_CC)), dim3(256), 0, st, x, dy, slab,
                     H, W, C, p.tiles_w, p.tiles_hw, p.tiles, p.S);
  if (isic_launch_status() != ISIC_OK) return ISIC_ERR_LAUNCH;
  return ct_slab_reduce(slab, p.S, (int64_t)DG_TAPS * C, (int64_t)25 * C, dw_taps, db, scale, accumulate, st);
}

size_t isic_layernorm_add_bwd_f16_workspace_bytes(int64_t M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return (size_t)la_plan(M).G * 2 * N * sizeof(float);
}

int isic_layernorm_add_bwd_f16(const void* dy, int dy_is_f32, float dy_mul, const uint16_t* x, const uint16_t* a,
                               const uint16_t* b, const float* gamma, const float* beta, int act, float eps,
                               const float* g_in, float* g_out, uint16_t* g_out16, float* dgamma, float* dbeta, int64_t M,
                               int N, float scale, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && N > 0 && (dy_is_f32 == 0 || dy_is_f32 == 1) && (act == 0 || act == 1) && eps >= 0.f &&
                 (accumulate == 0 || accumulate == 1));
  if (N % 64 != 0 || N > 1024) return ISIC_ERR_UNSUPPORTED;
  ISIC_CHECK_ARG(gamma && beta && dgamma && dbeta);
  ISIC_CHECK_ARG(M == 0 || (dy && x && (g_out || g_out16)));
  hipStream_t st = as_stream(stream);
  if (M == 0) {
    if (accumulate) return ISIC_OK;
    if (hipMemsetAsync(dgamma, 0, (size_t)N * sizeof(float), st) != hipSuccess) return ISIC_ERR_LAUNCH;
    return hipMemsetAsync(dbeta, 0, (size_t)N * sizeof(float), st) == hipSuccess ? ISIC_OK : ISIC_ERR_LAUNCH;
  }
  if (!workspace || workspace_bytes < isic_layernorm_add_bwd_f16_workspace_bytes(M, N)) return ISIC_ERR_WORKSPACE;
  const LaPlan p = la_plan(M);
  float* slab = reinterpret_cast<float*>(workspace);
  if (N <= 512)
    hipLaunchKernelGGL(layernorm_add_bwd_f16_kernel<1>, dim3(p.G), dim3(256), 0, st, dy, dy_is_f32, dy_mul, x, a, b, gamma,
                       beta, act, eps, g_in, g_out, g_out16, M, N, p.chunk, slab);
  else
    hipLaunchKernelGGL(layernorm_add_bwd_f16_kernel<2>, dim3(p.G), dim3(256), 0, st, dy, dy_is_f32, dy_mul, x, a, b, gamma,
                       beta, act, eps, g_in, g_out, g_out16, M, N, p.chunk, slab);
  if (isic_launch_status() != ISIC_OK) return ISIC_ERR_LAUNCH;
  return ct_slab_reduce(slab, p.G, (int64_t)2 * N, N, dgamma, dbeta, scale, accumulate, st);
}

int isic_patch_rows_bwd_f16(const uint16_t* drows, float* dx, uint16_t* dx16, int N, int H, int W, int C, int P,
                            int accumulate, void* stream) {
  ISIC_CHECK_ARG(N >= 0 && H > 0 && W > 0 && C > 0 && P > 0 && (accumulate == 0 || accumulate == 1));
  if ((P != 2 && P != 4) || C % 8 != 0 || H % P != 0 || W % P != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(drows && dx);
  const int64_t nvec = (int64_t)N * H * W * C / 8;
  hipLaunchKernelGGL(patch_rows_bwd_kernel, dim3((unsigned)ct_grid(nvec, 256, 16384)), dim3(256), 0, as_stream(stream),
                     drows, dx, dx16, H, W, C, P, accumulate, nvec);
  return isic_launch_status();
}

}  // extern "C"
