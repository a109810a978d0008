// Device primitives shared by the LDS-DMA / MFMA tile kernels (gfx950): the asm memory primitives, the packed-bf16
// conversions, the DPP row sum and the register-only epilogue fragments.  A primitive that two kernel files use lives
// here; a new kernel calls it and does not bring a copy of its own ("Shared tile primitives").
// Every function is a __forceinline__ leaf: moving one here leaves the kernels' ISA unchanged (profiles/tile_primitives_isa.txt).
// (The zero / sink pages -- g_*_zero_page, g_*_zeros, g_c64_sink, g_c64_ones -- stay one per kernel file: a shared device
//  global would need relocatable device code across translation units, which the build does not use.)
#pragma once
#include "common.h"

// ---------------------------------------------------------------- asm memory primitives
// One LDS-DMA instruction from inline asm: 64 lanes x 16 B from per-lane global addresses to the wave-uniform LDS
// byte address `lds_dst` (+ lane*16).  Issued from asm so that hipcc neither counts it in vmcnt nor fences the
// following ds_read_tr with a vmcnt(0) drain (it does for the builtin form in conv_wgrad.hip); completion is
// tracked by the caller's own counted s_waitcnt.  M0 (the DMA's LDS base) is saved and restored inside the statement.
__device__ __forceinline__ void isic_glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// LDS-DMA / store with a wave-uniform 64-bit base (SGPR pair) and a 32-bit per-lane byte offset
__device__ __forceinline__ void isic_glds16_s(const void* sbase, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// (the s_nop covers the hazard "VMEM store of more than 64 bits followed by a write of its data VGPRs", which the
//  compiler cannot see through the asm statement)
// Ordinary stores, not non-temporal ones (late round 4).  The two waves of a SIMD write the two 64-byte halves of a pixel
// row half a tile apart; non-temporal, each half goes to memory by itself (64-byte segments stream at 3.2 TB/s against 5.4
// for whole lines, profiles/r03_probe_rw.txt), cached, the L2 joins them: dgrad + addend 1.356 -> 1.295 ms, dgrad 0.951 ->
// 0.939 ms, forward with statistics unchanged (conv_c64.hip, interleaved A/B, 4096 images).
__device__ __forceinline__ void isic_store16_s(void* sbase, unsigned voff, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ void isic_store16_v(void* ptr, u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" ::"v"(ptr), "v"(v) : "memory");
}

// ---------------------------------------------------------------- packed bf16 <-> f32
// two floats -> one word of two bf16: ONE v_cvt_pk_bf16_f32 (round to nearest even, NaN preserved), `lo` in bits 0..15
__device__ __forceinline__ unsigned isic_pack_bf16x2(float lo, float hi) {
  const f32x2 f = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
}
// four accumulators -> two words through the scalar cast of common.h (same rounding; the LDS-staged epilogues use it)
__device__ __forceinline__ u32x2 isic_pack_bf16x4(const f32x4& c) {
  u32x2 v;
  v[0] = (unsigned)f32_to_bf16_bits(c[0]) | ((unsigned)f32_to_bf16_bits(c[1]) << 16);
  v[1] = (unsigned)f32_to_bf16_bits(c[2]) | ((unsigned)f32_to_bf16_bits(c[3]) << 16);
  return v;
}
// the four values of two packed words, exactly (what a consumer of the rounded output will read)
__device__ __forceinline__ void isic_unpack_bf16x4(unsigned lo, unsigned hi, float (&r)[4]) {
  r[0] = __uint_as_float(lo << 16);
  r[1] = __uint_as_float(lo & 0xFFFF0000u);
  r[2] = __uint_as_float(hi << 16);
  r[3] = __uint_as_float(hi & 0xFFFF0000u);
}

// ---------------------------------------------------------------- register-only epilogue fragments
// Each is one fixed sequence of operations: which multiply-adds the compiler fuses, and so the last bit of the
// result, depends on it.  A kernel whose fragment differs keeps its own text instead of a flag here.
//
// c += the bf16x4 addend held in (lo, hi): fp32 add in the accumulator domain, rounded once afterwards
__device__ __forceinline__ void isic_add_bf16x4(f32x4& c, unsigned lo, unsigned hi) {
  c[0] += __uint_as_float(lo << 16);
  c[1] += __uint_as_float(lo & 0xFFFF0000u);
  c[2] += __uint_as_float(hi << 16);
  c[3] += __uint_as_float(hi & 0xFFFF0000u);
}
// ... added only where bit e of `bits` is set (the addend's ReLU mask; 0xF: unmasked)
__device__ __forceinline__ void isic_add_bf16x4_masked(f32x4& c, unsigned lo, unsigned hi, unsigned bits) {
  c[0] += (bits & 1u) ? __uint_as_float(lo << 16) : 0.f;
  c[1] += (bits & 2u) ? __uint_as_float(lo & 0xFFFF0000u) : 0.f;
  c[2] += (bits & 4u) ? __uint_as_float(hi << 16) : 0.f;
  c[3] += (bits & 8u) ? __uint_as_float(hi & 0xFFFF0000u) : 0.f;
}
// s[e] += r[e], q[e] += r[e]^2 for the four ROUNDED values r (BatchNorm sum / sum of squares)
__device__ __forceinline__ void isic_sum_sumsq4(float* s, float* q, const float (&r)[4]) {
  s[0] += r[0]; q[0] += r[0] * r[0];
  s[1] += r[1]; q[1] += r[1] * r[1];
  s[2] += r[2]; q[2] += r[2] * r[2];
  s[3] += r[3]; q[3] += r[3] * r[3];
}

// ---------------------------------------------------------------- DPP row (16 lanes) reductions
// sum over the 16 lanes of a DPP row (after the MFMAs: the lanes of one fg group), result in every lane:
// row_ror 8, 4, 2, 1 (dpp_ctrl 0x128, 0x124, 0x122, 0x121), all rows and banks enabled
__device__ __forceinline__ float isic_row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));
  return v;
}
