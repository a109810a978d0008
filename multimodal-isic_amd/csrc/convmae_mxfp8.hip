// MXFP8 outputs on the convolutional front of the ConvMAE-Base patch encoder (isic_hip/convmae.py precision="mxfp8"):
// what feeds isic_gemm_mxfp8 there -- a row LayerNorm (optional erf-GELU) at the widths of isic_layernorm_add_f16, the
// depthwise 5x5 and the space-to-depth patch rows, each quantised from its fp32 values by the rule of csrc/mxfp8.hip
// (csrc/mx_quant.inc).  The LayerNorm and the depthwise 5x5 are instantiations of the fp16 kernels' templates
// (csrc/convmae_kernels.inc).  include/isic_hip_convmae_mxfp8.h declares the entry points.

#include "convmae_kernels.inc"

namespace {

// ---------------------------------------------------------------- patch rows -> MXFP8
// The rows of patch_rows_nhwc_kernel ([kh][kw][c] columns), one 4-lane group per 32-element block: C % 32 == 0, so a
// block of a row is 32 consecutive channels of one pixel of x.  A lane reads 16 bytes of x and writes 8 element bytes.
__global__ __launch_bounds__(256) void patch_rows_mx_kernel(const unsigned short* __restrict__ x, unsigned char* __restrict__ q,
                                                            unsigned char* __restrict__ s, int H, int W, int C, int P,
                                                            int64_t nvec) {
  const int gh = H / P, gw = W / P, seg = P * C, kv = P * seg / 8;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;       // 8-element piece of the rows; nvec % 4 == 0
  const bool live = gid < nvec;
  const int64_t i = live ? gid : 0;
  const int k = (int)(i % kv) * 8;
  const int64_t row = i / kv;
  const int px = (int)(row % gw), py = (int)((row / gw) % gh);
  const int64_t n = row / ((int64_t)gw * gh);
  const int kh = k / seg, rem = k - kh * seg;
  const unsigned short* src = x + (((size_t)n * H + (size_t)(py * P + kh)) * W + (size_t)px * P) * C + rem;
  float f[8];
  f16_unpack8(*reinterpret_cast<const u32x4*>(src), f);
  unsigned char scale;
  const u32x2 o = mx_block8(f, scale);
  if (live) {
    *reinterpret_cast<u32x2*>(q + i * 8) = o;
    if ((gid & 3) == 0) s[i >> 2] = scale;
  }
}

}  // namespace

extern "C" {

int isic_layernorm_act_mxfp8_f16(const uint16_t* x, const float* gamma, const float* beta, uint8_t* q, uint8_t* s, int64_t M,
                                 int N, int act, float eps, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && N > 0 && (act == 0 || act == 1) && eps >= 0.f);
  if (N % 64 != 0 || N > 1024) return ISIC_ERR_UNSUPPORTED;
  if (M == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && gamma && beta && q && s);
  const dim3 grid((unsigned)cm_grid(M, 4 * 4, 8192));
  if (N <= 512)
    hipLaunchKernelGGL((layernorm_add_f16_kernel<1, true>), grid, dim3(256), 0, as_stream(stream), x, nullptr, nullptr, gamma,
                       beta, nullptr, nullptr, M, N, act, eps, q, s);
  else
    hipLaunchKernelGGL((layernorm_add_f16_kernel<2, true>), grid, dim3(256), 0, as_stream(stream), x, nullptr, nullptr, gamma,
                       beta, nullptr, nullptr, M, N, act, eps, q, s);
  return isic_launch_status();
}

int isic_dwconv5x5_mxfp8_f16(const uint16_t* x, const float* w_taps, const float* bias, uint8_t* q, uint8_t* s, int N, int H,
                             int W, int C, void* stream) {
  ISIC_CHECK_ARG(N >= 0 && H > 0 && W > 0 && C > 0);
  if (C % DW_CC != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && w_taps && q && s);
  const int tiles_w = (W + DW_TW - 1) / DW_TW, tiles_h = (H + DW_TH - 1) / DW_TH;
  const int64_t blocks = (int64_t)N * (C / DW_CC) * tiles_w * tiles_h;
  if (blocks > (int64_t)INT32_MAX) return ISIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(dwconv5x5_f16_kernel<DW_MX>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, w_taps, bias,
                     nullptr, H, W, C, tiles_w, tiles_w * tiles_h, nullptr, 1, nullptr, q, s);
  return isic_launch_status();
}

int isic_patch_rows_mxfp8_nhwc_f16(const uint16_t* x, uint8_t* q, uint8_t* s, int N, int H, int W, int C, int P,
                                   void* stream) {
  ISIC_CHECK_ARG(N >= 0 && H > 0 && W > 0 && C > 0 && P > 0);
  if ((P != 2 && P != 4) || C % 32 != 0 || H % P != 0 || W % P != 0) return ISIC_ERR_UNSUPPORTED;
  if (N == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && q && s);
  const int64_t nvec = (int64_t)N * H * W * C / 8;
  const int64_t grid = (nvec + 255) / 256;
  if (grid > (int64_t)INT32_MAX) return ISIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(patch_rows_mx_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), x, q, s, H, W, C, P, nvec);
  return isic_launch_status();
}

}  // extern "C"
