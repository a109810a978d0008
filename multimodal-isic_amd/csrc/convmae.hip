// The convolutional front of the ConvMAE-Base patch encoder (gfx950, fp16 activations, fp32 arithmetic inside): the
// depthwise 5x5 token mixer of a CBlock, the rows of the non-overlapping P x P patch convolutions (space-to-depth), and a
// LayerNorm over rows of up to 1024 channels with an optional erf-GELU and up to two fp16 addends.  Everything else of the
// encoder (1x1 convs, patch / decode convs, the ViT-B stage) is isic_gemm_f16* and isic_attention_f16.
// include/isic_hip_convmae.h declares the entry points; isic_hip/convmae.py composes them.

#include "convmae_kernels.inc"

namespace {

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
                     H, W, C, tiles_w, tiles_w * tiles_h, nullptr, 1, nullptr, nullptr, nullptr);
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
                       y, H, W, C, tiles_w, tiles_w * tiles_h, k, P, xm, nullptr, nullptr);
  else
    hipLaunchKernelGGL(dwconv5x5_f16_kernel<DW_MASK_OUT>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, w_taps,
                       bias, y, H, W, C, tiles_w, tiles_w * tiles_h, k, P, nullptr, nullptr, nullptr);
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
