// The fp16 row LayerNorm, written once: two-pass fp32 statistics over the values a row's lanes hold in registers, and the
// kernel of the ViT-width entry points over it.  Included by csrc/vit_ops.hip and csrc/mxfp8.hip (layernorm_f16_kernel)
// and, through csrc/convmae_kernels.inc, by csrc/convmae.hip, csrc/convmae_mxfp8.hip and csrc/convmae_train.hip
// (layernorm_add_f16_kernel and its backward keep their kernels and call ln_row_center).
//
// One text, the same sums in the same order, two mean rules -- and NOT one rounding: the compiler contracts
// multiply-adds per kernel after inlining, so the sum of squares is all v_fmac in one kernel, all v_pk_mul + v_add in
// another and mixed in a third (DESIGN.md section 4, "The row LayerNorm"), and two kernels' statistics for the same
// row may differ in the last bit.  tests/test_ln_rows_gpu.py pins the bits of each.
#pragma once
#include "common.h"
#include "mx_quant.inc"

// How the mean is taken from the row sum s.
//   LN_MEAN_RCP: s * (1 / N), the ViT-width kernels' (N is a template constant there).  1 / 384 is inexact, and where the
//                compiler fuses "f - s * invn" into one FMA with the product unrounded (it does in the statistics-only
//                and MXFP8 kernels, not in the fp16 one) a row of equal values need not centre to exactly 0.
//   LN_MEAN_DIV: s / N, a true division, the ConvMAE kernels': N c / N is exact for every row of equal values c, which
//                times rstd = 1 / sqrt(eps) would otherwise be 6e-5 in x^ at N = 768.
enum LnMean { LN_MEAN_RCP, LN_MEAN_DIV };

// Row statistics of v = (x + a) + b (a, b: optional fp16 addends, null = absent; the sum in fp32, unrounded) for the
// row that starts at element row0.  LPR lanes share the row (a power of two, for the shuffles); lane `lane` of them
// holds the 16-byte pieces lane + LPR i, i < CPL, of which the first `pieces` exist (a lane whose piece does not exist
// reads piece 0 and contributes 0 to both sums).  n = 8 pieces, invn = 1 / n as the caller has it (a constant or a run
// time quotient).  Leaves f = v - mean, and (mean, rstd).
template <int LPR, int CPL, LnMean MEAN>
__device__ __forceinline__ void ln_row_center(const unsigned short* __restrict__ x, const unsigned short* __restrict__ a,
                                              const unsigned short* __restrict__ b, size_t row0, int lane, int pieces, int n,
                                              float invn, float eps, float (&f)[CPL][8], float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int q = lane + LPR * i;
    const bool on = q < pieces;
    const size_t off = row0 + (size_t)(on ? q : 0) * 8;
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
  for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, LPR);
  mean = MEAN == LN_MEAN_DIV ? s / (float)n : s * invn;
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const bool on = lane + LPR * i < pieces;
#pragma unroll
    for (int j = 0; j < 8; ++j) { f[i][j] -= mean; v += on ? f[i][j] * f[i][j] : 0.f; }
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, LPR);
  rstd = rsqrtf(v * invn + eps);
}

namespace {

// ---------------------------------------------------------------- LayerNorm, rows of N = 8 * ACT halves
// LPR lanes per row, the first ACT of them active (N = 384: 48 of 64), one 16-byte piece per lane.  Three ways out:
//   LN_OUT_Y     o0 = y fp16 and / or o1 = y32 fp32 (the encoder's final norm hands fp32 tokens to the MIL head);
//   LN_OUT_STATS o1 = stats[M][2] = (mean, rstd), for a LayerNorm folded into the product that consumes it
//                (isic_gemm_f16_ln): reads x once, writes 8 bytes per row; gamma and beta are not read;
//   LN_OUT_MX    o0 = q[M][N] e4m3 bytes, o1 = s[M][N / 32] scale bytes, quantised from the fp32 normalised values:
//                lanes 4 b .. 4 b + 3 hold block b of the row (ACT % 4 == 0).
enum LnOut { LN_OUT_Y, LN_OUT_STATS, LN_OUT_MX };

template <int LPR, int ACT, LnOut OUT>
__global__ __launch_bounds__(256) void layernorm_f16_kernel(const unsigned short* __restrict__ x,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, void* __restrict__ o0,
                                                             void* __restrict__ o1, int64_t M, float eps) {
  constexpr int N = 8 * ACT;
  const int lane = threadIdx.x % LPR, rl = threadIdx.x / LPR, rls = 256 / LPR;
  const bool act = lane < ACT;
  const int col = (act ? lane : 0) * 8;
  float g[8], b[8];
  if (OUT != LN_OUT_STATS) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { g[j] = gamma[col + j]; b[j] = beta[col + j]; }
  }
  for (int64_t row = (int64_t)blockIdx.x * rls + rl; row < M; row += (int64_t)gridDim.x * rls) {
    float f[1][8], mean, rstd;
    ln_row_center<LPR, 1, LN_MEAN_RCP>(x, nullptr, nullptr, (size_t)(row * N), lane, ACT, N, 1.f / N, eps, f, mean, rstd);
    if (OUT == LN_OUT_STATS) {
      float* stats = static_cast<float*>(o1);
      if (lane == 0) {
        stats[row * 2] = mean;
        stats[row * 2 + 1] = rstd;
      }
      continue;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) f[0][j] = f[0][j] * rstd * g[j] + b[j];
    if (OUT == LN_OUT_MX) {
      unsigned char scale;
      const u32x2 o = mx_block8(f[0], scale);                         // every lane reaches the shuffles
      if (act) {
        *reinterpret_cast<u32x2*>(static_cast<unsigned char*>(o0) + row * N + col) = o;
        if ((lane & 3) == 0) static_cast<unsigned char*>(o1)[row * (N / 32) + (lane >> 2)] = scale;
      }
    } else {
      unsigned short* y = static_cast<unsigned short*>(o0);
      float* y32 = static_cast<float*>(o1);
      if (act && y) *reinterpret_cast<u32x4*>(y + row * N + col) = f16_pack8(f[0]);
      if (act && y32) {
        *reinterpret_cast<f32x4*>(y32 + row * N + col) = (f32x4){f[0][0], f[0][1], f[0][2], f[0][3]};
        *reinterpret_cast<f32x4*>(y32 + row * N + col + 4) = (f32x4){f[0][4], f[0][5], f[0][6], f[0][7]};
      }
    }
  }
}

}  // namespace
