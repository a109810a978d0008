// The arithmetic of BatchNorm(+ReLU) backward, written once.  A kernel that forms BatchNorm-backward values -- the gated
// gradient dz, the sums of dz and dz * xhat, the per-channel constants, dx -- takes them from here: encoder_ops.hip
// (bn_bwd_reduce_kernel, bn_bwd_apply_kernel, the two stem kernels), conv_wgrad_c64.hip (wgrad_c64_kernel<2>, <3>) and
// conv_stem.hip (conv_stem_wgrad_bn_kernel).  These kernels promise each other's bits (tests/test_bn_pair_gpu.py,
// test_wgrad_bnbwd_gpu.py, test_encoder_gpu.py compare with torch.equal) and keep the promise by running the same functions.
//
// Every body is under `#pragma clang fp contract(off)` and every fused multiply-add is a __builtin_fmaf: the source text
// IS the rounding sequence, whatever -ffp-contract the file is built with.  tests/bn_bwd_ref.py emulates these functions
// step by step in numpy; tests/test_bn_bwd_math_gpu.py compares the device with it exactly.
//
//   dz  = the ReLU was active ? dy : 0
//   dx  = k1 * (dz - k2 - xhat * k3),  xhat = (x - mean) * rstd,  k1 = gamma * rstd,  k2 = sum dz / rows,
//         k3 = sum dz * xhat / rows
//       = kA * dz + (kB * x + kD): three constants per channel and two fused multiply-adds per element
#pragma once

namespace isic_bn_bwd {

// MODE: where the ReLU mask comes from -- 0 no ReLU, 1 the stored output `y`, 2 recomputed from the BatchNorm input as
// x * scale + shift (one fused multiply-add, as the forward pass's compiler made of it), 3 bit j of the mask byte m.
// The arguments a mode does not name are ignored.  !(v > 0) ? 0 : g -- a NaN output gates to 0, and so do +0 and -0.
template <int MODE>
__device__ __forceinline__ float gate(float g, float x, float y, float scale, float shift, unsigned m, int j) {
#pragma clang fp contract(off)
  static_assert(MODE >= 0 && MODE <= 3, "0 no ReLU, 1 from y, 2 from x, 3 mask bits");
  if constexpr (MODE == 0) return g;
  else if constexpr (MODE == 3) return ((m >> j) & 1u) ? g : 0.f;
  else {
    const float v = MODE == 2 ? __builtin_fmaf(x, scale, shift) : y;
    return !(v > 0.f) ? 0.f : g;
  }
}

// One element of the reduce pass: sum dz * xhat (xhat rounded by itself: a subtraction and a product) and sum dz.
// The second form serves a further norm that receives the same dz (its sum of dz is the first one's).
__device__ __forceinline__ void accumulate(float dz, float x, float mean, float rstd, float& acc_dzx) {
#pragma clang fp contract(off)
  acc_dzx = __builtin_fmaf(dz, (x - mean) * rstd, acc_dzx);
}
__device__ __forceinline__ void accumulate(float dz, float x, float mean, float rstd, float& acc_dzx, float& acc_dz) {
#pragma clang fp contract(off)
  accumulate(dz, x, mean, rstd, acc_dzx);
  acc_dz += dz;
}

// A reduce block sums a CONTIGUOUS range of rows (not a grid-strided set): DRAM pages are walked in order
// (5.8 -> 6.2 TB/s for the backward sums).  Row lane rl of `rls` takes begin + rl, begin + rl + rls, ... < end.
struct RowRange { int64_t begin, end; };
__device__ __forceinline__ RowRange block_rows(int64_t rows, int rls) {
  const int64_t per_block = ((rows + gridDim.x - 1) / gridDim.x + rls - 1) / rls * rls;
  const int64_t begin = (int64_t)blockIdx.x * per_block, end = begin + per_block;
  return {begin, end < rows ? end : rows};
}

__device__ __forceinline__ float inv_count(int64_t rows) { return 1.f / (float)rows; }

// The constants of one channel.  sum_dzx, sum_dz: the reduced fp64 sums, cast to float by the caller, `(float)sum[c]`
// (taken as doubles and cast here, the flat apply kernels come out 4 VGPRs larger and lose a wave per SIMD:
// profiles/bn_bwd_math_isa.txt); inv_rows = inv_count(rows).
__device__ __forceinline__ void constants(float mean, float rstd, float gamma, float sum_dzx, float sum_dz, float inv_rows,
                                          float& kA, float& kB, float& kD) {
#pragma clang fp contract(off)
  const float k1 = gamma * rstd, k2 = sum_dz * inv_rows, k3 = sum_dzx * inv_rows;
  kA = k1;
  kB = (-k1 * k3) * rstd;
  kD = k1 * __builtin_fmaf(k3 * rstd, mean, -k2);
}

// dx with one rounding per multiply-add: what every kernel but the fused stem weight gradient writes.
__device__ __forceinline__ float dx(float kA, float kB, float kD, float x, float dz) {
#pragma clang fp contract(off)
  return __builtin_fmaf(kA, dz, __builtin_fmaf(kB, x, kD));
}

// dx = (kD + kB * x) + kA * dz with each product and each sum rounded by itself: two roundings where dx() has one.
// ONLY conv_stem_wgrad_bn_kernel (the fused stem weight gradient) uses this: the operand of its MFMAs differs from what
// isic_bn_bwd_apply_pooled_bf16 writes by one rounding per multiply-add of every element (DESIGN.md, "bn_bwd_math.inc").
__device__ __forceinline__ float dx_unfused(float kA, float kB, float kD, float x, float dz) {
#pragma clang fp contract(off)
  const float t = kD + kB * x;
  return t + kA * dz;
}

// Channel c of the fp32 parameter gradients gets += the fp64 sums, each cast to float first: block 0 of every apply
// kernel, each channel by one thread.
__device__ __forceinline__ void fold(int c, const double* __restrict__ sum_dzx, const double* __restrict__ sum_dz,
                                     float* __restrict__ dgamma_f32, float* __restrict__ dbeta_f32) {
  dgamma_f32[c] += (float)sum_dzx[c];
  dbeta_f32[c] += (float)sum_dz[c];
}

}  // namespace isic_bn_bwd
