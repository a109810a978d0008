// The masked-autoencoder objective of ConvMAE-Base (isic_hip/convmae_mae.py): the token gather / scatter between the
// full 196-token grid and the kept tokens, the decoder's unshuffle (mask tokens + position embedding) and its adjoint, and
// the fused pixel-reconstruction loss.  The masked depthwise 5x5 lives with its unmasked form in convmae.hip, the
// head-width-32 attention with the head-width-64 kernels in vit_ops.hip / vit_train.hip.
// include/isic_hip_mae.h declares the entry points.

#include "common.h"

namespace {

// ---------------------------------------------------------------- row movement
// One thread per 16-byte piece (8 fp16 channels) of an output row: every output element is written exactly once, no atomics.
// An index outside [0, T) yields a zero row (never an out-of-bounds read).
__global__ __launch_bounds__(256) void gather_rows_kernel(const unsigned short* __restrict__ x, const int64_t* __restrict__ ids,
                                                          unsigned short* __restrict__ y, int64_t rows_out, int T, int L,
                                                          int C) {
  const int cv = C / 8;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < rows_out * cv; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / cv;
    const int c = (int)(e - r * cv);
    const int64_t n = r / L, id = ids[r];
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (id >= 0 && id < T) v = *reinterpret_cast<const u32x4*>(x + ((n * T + id) * C) + 8 * c);
    *reinterpret_cast<u32x4*>(y + r * C + 8 * c) = v;
  }
}

// x[n][t] = rank < L ? y[n][rank] : 0, rank = ids_restore[n][t]
__global__ __launch_bounds__(256) void scatter_rows_kernel(const unsigned short* __restrict__ y,
                                                           const int64_t* __restrict__ ids_restore,
                                                           unsigned short* __restrict__ x, int64_t rows_out, int T, int L,
                                                           int C) {
  const int cv = C / 8;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < rows_out * cv; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / cv;
    const int c = (int)(e - r * cv);
    const int64_t n = r / T, rank = ids_restore[r];
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (rank >= 0 && rank < L) v = *reinterpret_cast<const u32x4*>(y + ((n * L + rank) * C) + 8 * c);
    *reinterpret_cast<u32x4*>(x + r * C + 8 * c) = v;
  }
}

// out[n][t] = fp16((rank < L ? y[n][rank] : mask_token) + pos[t]), the sum in fp32
__global__ __launch_bounds__(256) void unshuffle_kernel(const unsigned short* __restrict__ y, const int64_t* __restrict__ ids_restore,
                                                        const float* __restrict__ mask_token, const float* __restrict__ pos,
                                                        unsigned short* __restrict__ out, int64_t rows_out, int T, int L,
                                                        int C) {
  const int cv = C / 8;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < rows_out * cv; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / cv;
    const int c = (int)(e - r * cv);
    const int64_t n = r / T, t = r - n * T, rank = ids_restore[r];
    float f[8];
    if (rank >= 0 && rank < L) {
      f16_unpack8(*reinterpret_cast<const u32x4*>(y + ((n * L + rank) * C) + 8 * c), f);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = mask_token[8 * c + i];
    }
    const float* pr = pos + t * C + 8 * c;
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = f16_pack2(f[2 * i] + pr[2 * i], f[2 * i + 1] + pr[2 * i + 1]);
    *reinterpret_cast<u32x4*>(out + r * C + 8 * c) = o;
  }
}

// dy_keep[n][j] = dout[n][ids_shuffle[n][j]] (j < L); d_removed[n][j - L] = dout[n][ids_shuffle[n][j]] (j >= L)
__global__ __launch_bounds__(256) void unshuffle_bwd_kernel(const unsigned short* __restrict__ dout,
                                                            const int64_t* __restrict__ ids_shuffle,
                                                            unsigned short* __restrict__ dy_keep,
                                                            unsigned short* __restrict__ d_removed, int64_t rows, int T,
                                                            int L, int C) {
  const int cv = C / 8;
  for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < rows * cv; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / cv;
    const int c = (int)(e - r * cv);
    const int64_t n = r / T, j = r - n * T, id = ids_shuffle[r];
    u32x4 v = (u32x4){0u, 0u, 0u, 0u};
    if (id >= 0 && id < T) v = *reinterpret_cast<const u32x4*>(dout + ((n * T + id) * C) + 8 * c);
    if (j < L) *reinterpret_cast<u32x4*>(dy_keep + (n * L + j) * C + 8 * c) = v;
    else if (d_removed) *reinterpret_cast<u32x4*>(d_removed + (n * (T - L) + (j - L)) * C + 8 * c) = v;
  }
}

// ---------------------------------------------------------------- reconstruction loss
// One block per patch (n, t): the K = P * P * Cimg target values in (row, column, channel) order come straight from the
// NCHW fp32 images; mean and the unbiased variance (norm_pix) and the squared error are block sums in a fixed order
// (wave shuffles, then the four waves in order): bit-reproducible.  part[n * T + t] = mask * mean_k (pred - target)^2;
// dpred = mask * 2 (pred - target) / (K * mask_sum) * loss_scale, fp16.
constexpr int LS_THREADS = 256, LS_EPT = 4, LS_KMAX = LS_THREADS * LS_EPT;

__device__ __forceinline__ float block_sum_fixed(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                                                   // red is reused: the previous sum's readers are done
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(LS_THREADS) void mae_loss_kernel(const unsigned short* __restrict__ pred,
                                                              const float* __restrict__ img, const float* __restrict__ mask,
                                                              int norm_pix, float dscale, unsigned short* __restrict__ dpred,
                                                              float* __restrict__ part, int T, int Cimg, int H, int W,
                                                              int P) {
  __shared__ float red[4];
  const int64_t patch = blockIdx.x;
  const int64_t n = patch / T;
  const int t = (int)(patch - n * T);
  const int gw = W / P, ph = t / gw, pw = t - ph * gw;
  const int K = P * P * Cimg;
  float tv[LS_EPT], pv[LS_EPT];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LS_EPT; ++i) {
    const int k = threadIdx.x + LS_THREADS * i;
    tv[i] = 0.f;
    pv[i] = 0.f;
    if (k < K) {
      const int c = k % Cimg, pq = k / Cimg, p = pq / P, q = pq - p * P;
      tv[i] = img[((n * Cimg + c) * H + (ph * P + p)) * (int64_t)W + pw * P + q];
      pv[i] = (float)__builtin_bit_cast(_Float16, pred[patch * K + k]);
      s += tv[i];
    }
  }
  if (norm_pix) {
    const float mean = block_sum_fixed(s, red) / (float)K;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < LS_EPT; ++i)
      if (threadIdx.x + LS_THREADS * i < K) v += (tv[i] - mean) * (tv[i] - mean);
    const float var = block_sum_fixed(v, red) / (float)(K - 1);
    const float rs = 1.f / sqrtf(var + 1e-6f);
#pragma unroll
    for (int i = 0; i < LS_EPT; ++i) tv[i] = (tv[i] - mean) * rs;
  }
  const float m = mask[patch];
  float e = 0.f;
#pragma unroll
  for (int i = 0; i < LS_EPT; ++i) {
    const int k = threadIdx.x + LS_THREADS * i;
    if (k < K) {
      const float d = pv[i] - tv[i];
      e += d * d;
      const float g = m == 0.f ? 0.f : m * 2.f * d * dscale;
      dpred[patch * K + k] = __builtin_bit_cast(unsigned short, (_Float16)g);
    }
  }
  e = block_sum_fixed(e, red);
  if (threadIdx.x == 0) part[patch] = m * (e / (float)K);
}

// loss = (sum of part in a fixed order) / mask_sum: one block
__global__ __launch_bounds__(LS_THREADS) void mae_loss_reduce_kernel(const float* __restrict__ part, int64_t n, float inv_sum,
                                                                     float* __restrict__ loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += LS_THREADS) s += part[i];
  s = block_sum_fixed(s, red);
  if (threadIdx.x == 0) loss[0] = s * inv_sum;
}

int64_t grid_for(int64_t work) {
  int64_t g = (work + 255) / 256;
  return g < 1 ? 1 : (g > 16384 ? 16384 : g);
}

}  // namespace

extern "C" {

int isic_gather_rows_f16(const uint16_t* x, const int64_t* ids_keep, uint16_t* y, int N, int T, int L, int C, void* stream) {
  ISIC_CHECK_ARG(N >= 0 && T > 0 && L > 0 && L <= T && C > 0);
  if (C % 8 != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && ids_keep && y);
  const int64_t rows = (int64_t)N * L;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)grid_for(rows * (C / 8))), dim3(256), 0, as_stream(stream), x, ids_keep, y,
                     rows, T, L, C);
  return isic_launch_status();
}

int isic_scatter_rows_f16(const uint16_t* y, const int64_t* ids_restore, uint16_t* x, int N, int T, int L, int C,
                          void* stream) {
  ISIC_CHECK_ARG(N >= 0 && T > 0 && L > 0 && L <= T && C > 0);
  if (C % 8 != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(y && ids_restore && x);
  const int64_t rows = (int64_t)N * T;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)grid_for(rows * (C / 8))), dim3(256), 0, as_stream(stream), y, ids_restore,
                     x, rows, T, L, C);
  return isic_launch_status();
}

int isic_mae_unshuffle_f16(const uint16_t* y, const int64_t* ids_restore, const float* mask_token, const float* pos,
                           uint16_t* out, int N, int T, int L, int C, void* stream) {
  ISIC_CHECK_ARG(N >= 0 && T > 0 && L > 0 && L <= T && C > 0);
  if (C % 8 != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(y && ids_restore && mask_token && pos && out);
  const int64_t rows = (int64_t)N * T;
  hipLaunchKernelGGL(unshuffle_kernel, dim3((unsigned)grid_for(rows * (C / 8))), dim3(256), 0, as_stream(stream), y, ids_restore,
                     mask_token, pos, out, rows, T, L, C);
  return isic_launch_status();
}

int isic_mae_unshuffle_bwd_f16(const uint16_t* dout, const int64_t* ids_shuffle, uint16_t* dy_keep, uint16_t* d_removed, int N,
                               int T, int L, int C, void* stream) {
  ISIC_CHECK_ARG(N >= 0 && T > 0 && L > 0 && L <= T && C > 0);
  if (C % 8 != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(dout && ids_shuffle && dy_keep && (d_removed || L == T));
  const int64_t rows = (int64_t)N * T;
  hipLaunchKernelGGL(unshuffle_bwd_kernel, dim3((unsigned)grid_for(rows * (C / 8))), dim3(256), 0, as_stream(stream), dout,
                     ids_shuffle, dy_keep, d_removed, rows, T, L, C);
  return isic_launch_status();
}

size_t isic_mae_loss_f16_workspace_bytes(int N, int H, int W, int P) {
  if (N <= 0 || P <= 0 || H % P != 0 || W % P != 0) return 0;
  return (size_t)N * (H / P) * (W / P) * sizeof(float);
}

int isic_mae_loss_f16(const uint16_t* pred, const float* images, const float* mask, int norm_pix, float mask_sum,
                      float loss_scale, uint16_t* dpred, float* loss, int N, int C, int H, int W, int P, void* workspace,
                      size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && P > 0 && (norm_pix == 0 || norm_pix == 1));
  ISIC_CHECK_ARG(mask_sum > 0.f && loss_scale > 0.f);
  if (H % P != 0 || W % P != 0 || P * P * C > LS_KMAX || P * P * C < 2) return ISIC_ERR_UNSUPPORTED;
  ISIC_CHECK_ARG(pred && images && mask && dpred && loss);
  if (!workspace || workspace_bytes < isic_mae_loss_f16_workspace_bytes(N, H, W, P)) return ISIC_ERR_WORKSPACE;
  const int T = (H / P) * (W / P);
  const int64_t patches = (int64_t)N * T;
  if (patches > (int64_t)INT32_MAX) return ISIC_ERR_UNSUPPORTED;
  const int K = P * P * C;
  float* part = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(mae_loss_kernel, dim3((unsigned)patches), dim3(LS_THREADS), 0, as_stream(stream), pred, images, mask, norm_pix,
                     loss_scale / ((float)K * mask_sum), dpred, part, T, C, H, W, P);
  hipLaunchKernelGGL(mae_loss_reduce_kernel, dim3(1), dim3(LS_THREADS), 0, as_stream(stream), part, patches, 1.f / mask_sum, loss);
  return isic_launch_status();
}

}  // extern "C"
