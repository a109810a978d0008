// The MXFP8 quantisation rule as device helpers, shared by csrc/mxfp8.hip and csrc/convmae_mxfp8.hip (the format and the
// rule are stated at the top of csrc/mxfp8.hip and in include/isic_hip_mxfp8.h).
#pragma once
#include "common.h"

// ---------------------------------------------------------------- the quantisation rule
__device__ __forceinline__ int mx_exponent(float amax) {          // amax > 0, finite
  const unsigned b = __float_as_uint(amax);
  const int eb = (int)(b >> 23);                                 // biased exponent (sign bit is 0)
  if (eb == 0) return -127;                                      // subnormal amax: far below the clamp
  // amax = m 2^E with m in [1, 2): E = eb - 127; amax <= 448 2^e  <=>  m 2^(E - e) <= 1.75 2^8
  //   -> e = E - 8 if m <= 1.75 else E - 7   (m <= 1.75  <=>  mantissa bits <= 0x600000)
  int e = eb - 127 - 8 + ((b & 0x7FFFFF) > 0x600000 ? 1 : 0);
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}
// 2^-e as an exact fp32 (e in [-127, 120] for finite amax: 2^-e is a normal number)
__device__ __forceinline__ float mx_inv_scale(int e) { return __uint_as_float((unsigned)(127 - e) << 23); }

// round-to-nearest-even e4m3fn of v, |v| <= 448
__device__ __forceinline__ unsigned f32_to_e4m3(float v) {
  const unsigned u = __float_as_uint(v);
  const unsigned sign = (u >> 24) & 0x80u;
  const unsigned a = u & 0x7FFFFFFFu;
  unsigned r;
  if (a >= 0x3C800000u) {                                         // >= 2^-6: e4m3 normal range
    r = (a + 0x7FFFFu + ((a >> 20) & 1u)) >> 20;                 // RNE to 3 mantissa bits (a carry bumps the exponent)
    r -= (127u - 7u) << 3;
  } else {                                                       // subnormal: multiples of 2^-9, 8 -> 0x08 = 2^-6
    r = (unsigned)rintf(__uint_as_float(a) * 512.f);
  }
  return sign | r;
}

// quantise 8 values of one block with its inverse scale (zero block: inv = 0 -> every element +0)
__device__ __forceinline__ u32x2 mx_pack8(const float (&f)[8], float inv, bool zero) {
  u32x2 o;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) w |= f32_to_e4m3(f[4 * h + j] * inv) << (8 * j);
    o[h] = zero ? 0u : w;
  }
  return o;
}

// One lane's 8 values of a 32-element block that four consecutive lanes hold (lanes 4 k .. 4 k + 3; all four must reach
// the shuffles): amax over the block, its exponent, the lane's element bytes and the block's scale byte.
__device__ __forceinline__ u32x2 mx_block8(const float (&f)[8], unsigned char& scale) {
  float am = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(f[j]));
  am = fmaxf(am, __shfl_xor(am, 1));
  am = fmaxf(am, __shfl_xor(am, 2));
  const bool zero = !(am > 0.f);
  const int e = zero ? 0 : mx_exponent(am);
  scale = (unsigned char)(zero ? 0 : e + 127);
  return mx_pack8(f, zero ? 0.f : mx_inv_scale(e), zero);
}

// the same 8 conversions on v_cvt_pk_fp8_f32 (gfx950: OCP e4m3fn, round to nearest even in the normal range; |v * inv|
// <= 448, so its saturation behaviour never matters) with the e4m3 subnormal range (|t| < 2^-6) redone by the rule's
// integer form: the converter's handling of that range has not been checked bit for bit against the rule.  The GELU +
// MXFP8 epilogue of fc1 is VALU-bound: 0.84 ms per launch at 2048 images with the integer form throughout, 0.76 with this.
__device__ __forceinline__ u32x2 mx_pack8_hw(const float (&f)[8], float inv, bool zero) {
  u32x2 o;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = f[4 * h + j] * inv;
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], w, true);
    unsigned u = (unsigned)w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = fabsf(t[j]);
      const unsigned sub = ((__float_as_uint(t[j]) >> 24) & 0x80u) | (unsigned)rintf(a * 512.f);
      u = a < 0.015625f ? (u & ~(0xFFu << (8 * j))) | (sub << (8 * j)) : u;
    }
    o[h] = zero ? 0u : u;
  }
  return o;
}
