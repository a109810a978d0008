// MXFP8 inference path of the frozen ViT-S/16 patch encoder (BASELINE.json configs[4], isic_hip/vit.py precision="mxfp8").
//
// Format (OCP MX, FP8 E4M3 = e4m3fn, not the MI300 fnuz): an operand of R rows and K columns is q[R][K] e4m3 bytes and
// s[R][K / 32] E8M0 bytes, one scale per 32 consecutive elements along K; value = float(q) * 2^(s - 127).
// Quantisation of a block (the one rule, restated on the CPU by tests/mxfp8_ref.py):
//   amax = max |v| (fp32); amax == 0 -> scale byte 0, every element +0;
//   else e = the smallest integer with amax <= 448 * 2^e (frexp exponent + one compare), clamped to [-127, 127]
//   (the clamp only binds below 448 * 2^-127, where it cannot saturate); scale byte e + 127;
//   element = round-to-nearest-even e4m3fn of v * 2^-e (subnormals as torch's x.to(float8_e4m3fn); |v * 2^-e| <= 448 by
//   the choice of e, so nothing saturates).
// The conversion is done in integer arithmetic here rather than with v_cvt_pk_fp8_f32, so that the rule above -- not a
// rounding / saturation mode of the converter -- is what the bytes follow.
//
// isic_gemm_mxfp8 runs on v_mfma_scale_f32_16x16x128_f8f6f4 (format code 0 = E4M3 for both operands).  Lane map of the
// scaled 16x16x128 form with e4m3 operands, measured on the MI355X with one-hot operands (a value code per byte, a
// distinct scale per lane) and pinned by tests/test_mxfp8_gpu.py (exact integer data, asymmetric W): lane l = 16 g + r
// holds row r of the first operand / column r of the second, bytes 0-15 of its 8 VGPRs at k = 16 g + j and bytes 16-31 at
// k = 64 + 16 g + (j - 16) -- NOT 32 consecutive k -- while its scale VGPR (byte 0, opsel 0) is the E8M0 scale of the MX
// block k / 32 = g of that row / column, whose elements sit in other lanes' bytes.  So a lane loads the 16-byte chunks g
// and g + 4 of the 128-byte K-step and the scale byte of block g.  The C/D layout is the one of every 16x16 MFMA:
// col = lane & 15, row = 4 (lane >> 4) + reg.

#include "common.h"
#include "mx_quant.inc"
#include "ln_rows.inc"       // layernorm_f16_kernel<64, 48, LN_OUT_MX>: the row LayerNorm of isic_layernorm_mxfp8_f16

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------- quantise rows
// One 4-lane group per 32-element block: a lane converts 8 elements and writes 8 bytes.
template <bool F32>
__global__ __launch_bounds__(256) void mx_quantize_kernel(const void* __restrict__ x, unsigned char* __restrict__ q,
                                                          unsigned char* __restrict__ s, int64_t nblocks, int K) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;   // 8-element piece
  const int64_t blk = gid >> 2;
  const bool live = blk < nblocks;
  const int64_t piece = live ? gid : 0;
  float f[8];
  if (F32) {
    const f32x4* p = reinterpret_cast<const f32x4*>(static_cast<const float*>(x) + piece * 8);
    const f32x4 a = p[0], b = p[1];
    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
  } else {
    const u32x4 v = *reinterpret_cast<const u32x4*>(static_cast<const unsigned short*>(x) + piece * 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned w = v[j];
      f[2 * j] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu));
      f[2 * j + 1] = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
    }
  }
  unsigned char scale;
  const u32x2 o = mx_block8(f, scale);
  if (live) {
    *reinterpret_cast<u32x2*>(q + piece * 8) = o;
    if ((gid & 3) == 0) s[blk] = scale;
  }
}

// ---------------------------------------------------------------- GEMM on the scaled MFMA
// C = act((A_q . A_s) (W_q . W_s)^T + bias) (+ residual).  256 threads = 2 x 2 waves of 64 x 64 outputs on a 128 x 128
// tile, K-step 128 (one scaled MFMA deep).  Operands and their scale bytes are staged into LDS with LDS-DMA
// (global_load_lds: 16-byte pieces of the 128-byte operand rows, 4-byte scale words), double-buffered, one barrier per
// K-step.  Operand rows are 128 B; the 16-byte chunk c of row r sits at position c ^ swz(r) (XOR applied on the global
// side: the DMA writes a wave's 1 KB contiguously).
// Operand roles are swapped (W is the MFMA's first operand) and the W rows of a wave's four 16-column tiles are read in
// the order n = 16 (rho >> 2) + 4 j + (rho & 3) (rho = lane & 15 of the reading lane, j = tile): the lane (fr, g) then
// ends with the 16 CONSECUTIVE columns 16 g + 4 j + r of row fr -- two 16-byte fp16 stores, or one 16-byte MX store and
// an MX block (32 columns) on the lane pair g, g ^ 1.
constexpr int MG_M = 128, MG_N = 128, MG_K = 128;
constexpr int MG_A = MG_M * MG_K, MG_W = MG_N * MG_K;             // operand bytes per K-step
constexpr int MG_SA = MG_A + MG_W, MG_SW = MG_SA + MG_M * 4;      // scale words (4 blocks of a row per K-step)
constexpr int MG_STAGE = MG_SW + MG_N * 4;
constexpr int MG_LDS = 2 * MG_STAGE;

struct MxGemmArgs {
  const unsigned char* A;      // [M][K]
  const unsigned char* As;     // [M][K / 32]
  const unsigned char* W;      // [N][K]
  const unsigned char* Ws;     // [N][K / 32]
  const float* bias;           // [N] or null
  const unsigned short* res;   // fp16 [M][N] (res_rows == 0) or [res_rows][N], or null
  unsigned short* C;           // fp16 [M][N], or null
  unsigned char* Cq;           // [M][N], or null
  unsigned char* Cs;           // [M][N / 32]
  int M, N, K, res_rows, mtiles, ntiles, ntiles_total;
};

__device__ __forceinline__ unsigned swz_a(int r) { return (unsigned)(r & 7); }
__device__ __forceinline__ unsigned swz_w(int r) { return (unsigned)(((r >> 4) & 3) | (((r >> 1) & 1) << 2)); }
__device__ __forceinline__ float gelu_erf_mx(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

template <int GELU, bool RES, bool MXOUT>
__global__ __launch_bounds__(256, 2) void gemm_mxfp8_kernel(MxGemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // blocks of one XCD (workgroup id % 8) take consecutive tiles; a tile's N-slices are adjacent (A re-read from L2)
  const int nb = a.ntiles_total, per = (nb + 7) / 8;
  const int bid = blockIdx.x;
  const int tile = (bid & 7) * per + (bid >> 3);
  if (tile >= nb) return;
  const int mt = tile / a.ntiles, nt = tile - mt * a.ntiles;
  const int m0 = mt * MG_M, n0 = nt * MG_N;
  const int K = a.K, KS = K >> 5, KT = K / MG_K;

  // ---- staging addresses: wave w moves operand rows 8 (4 q + w) + (lane >> 3), q = 0..3, for A and for W
  const int r8 = lane >> 3, p8 = lane & 7;
  const unsigned char* ga[4];
  const unsigned char* gw[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = 8 * (4 * q + wave) + r8;
    const int m = min(m0 + r, a.M - 1);                           // ragged tail: a valid row, its results are not stored
    ga[q] = a.A + (size_t)m * K + ((p8 ^ swz_a(r)) << 4);
    gw[q] = a.W + (size_t)(n0 + r) * K + ((p8 ^ swz_w(r)) << 4);
  }
  // scale words: waves 0, 1 -> A rows 64 w + lane; waves 2, 3 -> W rows 64 (w - 2) + lane
  const unsigned char* gs;
  {
    const int r = 64 * (wave & 1) + lane;
    gs = wave < 2 ? a.As + (size_t)min(m0 + r, a.M - 1) * KS : a.Ws + (size_t)(n0 + r) * KS;
  }
  auto issue = [&](int kt, int buf) {
    unsigned char* st = smem + buf * MG_STAGE;
    const int ko = kt * MG_K;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      __builtin_amdgcn_global_load_lds(ga[q] + ko, (lds_ptr)(st + (4 * q + wave) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(gw[q] + ko, (lds_ptr)(st + MG_A + (4 * q + wave) * 1024), 16, 0, 0);
    }
    __builtin_amdgcn_global_load_lds(gs + kt * 4, (lds_ptr)(st + (wave < 2 ? MG_SA : MG_SW) + 256 * (wave & 1)), 4, 0, 0);
  };

  const int fr = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  int ra[4], rw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = wm * 64 + 16 * i + fr;
    rw[i] = wn * 64 + 16 * (fr >> 2) + 4 * i + (fr & 3);
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  issue(0, 0);
#pragma unroll 1
  for (int kt = 0; kt < KT; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // this wave's pieces of K-step kt have landed
    __syncthreads();                                                // ... and everyone's; buffer kt + 1 is free
    if (kt + 1 < KT) issue(kt + 1, (kt + 1) & 1);
    const unsigned char* st = smem + (kt & 1) * MG_STAGE;
    i32x8 af[4], wf[4];
    int as[4], ws[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned char* pa = st + ra[i] * 128;
      const u32x4 a0 = *reinterpret_cast<const u32x4*>(pa + (((unsigned)g ^ swz_a(ra[i])) << 4));          // k 16 g ..
      const u32x4 a1 = *reinterpret_cast<const u32x4*>(pa + (((unsigned)(g + 4) ^ swz_a(ra[i])) << 4));    // k 64 + 16 g ..
      af[i] = (i32x8){(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
      const unsigned char* pw = st + MG_A + rw[i] * 128;
      const u32x4 w0 = *reinterpret_cast<const u32x4*>(pw + (((unsigned)g ^ swz_w(rw[i])) << 4));
      const u32x4 w1 = *reinterpret_cast<const u32x4*>(pw + (((unsigned)(g + 4) ^ swz_w(rw[i])) << 4));
      wf[i] = (i32x8){(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], (int)w1[0], (int)w1[1], (int)w1[2], (int)w1[3]};
      as[i] = st[MG_SA + ra[i] * 4 + g];
      ws[i] = st[MG_SW + rw[i] * 4 + g];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], af[i], acc[i][j], 0, 0, 0, ws[j], 0, as[i]);
  }

  // ---- register-only epilogue: lane (fr, g) holds columns n0 + wn 64 + 16 g + {0..15} of row m0 + wm 64 + 16 i + fr
  const int cb = n0 + wn * 64 + 16 * g;
  float bv[16];
#pragma unroll
  for (int e = 0; e < 16; e += 4) {
    const f32x4 b4 = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + cb + e) : (f32x4){0.f, 0.f, 0.f, 0.f};
    bv[e] = b4[0]; bv[e + 1] = b4[1]; bv[e + 2] = b4[2]; bv[e + 3] = b4[3];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + 16 * i + fr;
    const bool valid = m < a.M;
    const int mc = valid ? m : 0;
    float c[16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) c[4 * j + r] = acc[i][j][r] + bv[4 * j + r];
    if (GELU) {
#pragma unroll
      for (int e = 0; e < 16; ++e) c[e] = gelu_erf_mx(c[e]);
    }
    if (RES) {
      const size_t roff = (size_t)(a.res_rows > 0 ? mc % a.res_rows : mc) * a.N + cb;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const u32x4 rv = *reinterpret_cast<const u32x4*>(a.res + roff + 8 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned w = rv[e];
          c[8 * h + 2 * e] += (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu));
          c[8 * h + 2 * e + 1] += (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
        }
      }
    }
    if (MXOUT) {
      float am = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) am = fmaxf(am, fabsf(c[e]));
      am = fmaxf(am, __shfl_xor(am, 16));                          // lanes g, g ^ 1: the 32 columns of one block
      const bool zero = !(am > 0.f);
      const int ex = zero ? 0 : mx_exponent(am);
      const float inv = zero ? 0.f : mx_inv_scale(ex);
      float lo[8], hi[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { lo[e] = c[e]; hi[e] = c[8 + e]; }
      const u32x2 p0 = mx_pack8_hw(lo, inv, zero), p1 = mx_pack8_hw(hi, inv, zero);
      if (valid) {
        __builtin_nontemporal_store((u32x4){p0[0], p0[1], p1[0], p1[1]},
                                    reinterpret_cast<u32x4*>(a.Cq + (size_t)m * a.N + cb));
        if ((g & 1) == 0) a.Cs[(size_t)m * (a.N >> 5) + (cb >> 5)] = (unsigned char)(zero ? 0 : ex + 127);
      }
    } else {
      u32x4 o[2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const _Float16 x0 = (_Float16)c[8 * h + 2 * e], x1 = (_Float16)c[8 * h + 2 * e + 1];   // round to nearest even
          o[h][e] = (unsigned)__builtin_bit_cast(unsigned short, x0) | ((unsigned)__builtin_bit_cast(unsigned short, x1) << 16);
        }
      if (valid) {
        __builtin_nontemporal_store(o[0], reinterpret_cast<u32x4*>(a.C + (size_t)m * a.N + cb));
        __builtin_nontemporal_store(o[1], reinterpret_cast<u32x4*>(a.C + (size_t)m * a.N + cb + 8));
      }
    }
  }
}

template <int GELU, bool RES, bool MXOUT>
int launch_mx(const MxGemmArgs& a, hipStream_t stream) {
  const int grid = (a.ntiles_total + 7) / 8 * 8;
  return isic_launch_lds<gemm_mxfp8_kernel<GELU, RES, MXOUT>, MG_LDS>(dim3(grid), dim3(256), MG_LDS, stream, a);
}

template <int GELU, bool RES>
int launch_mx_out(const MxGemmArgs& a, bool mx, hipStream_t s) {
  return mx ? launch_mx<GELU, RES, true>(a, s) : launch_mx<GELU, RES, false>(a, s);
}

}  // namespace

extern "C" {

int isic_mxfp8_quantize(const void* x, int x_is_f32, uint8_t* q, uint8_t* s, int64_t M, int K, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && K > 0 && (x_is_f32 == 0 || x_is_f32 == 1));
  if (K % 32 != 0) return ISIC_ERR_UNSUPPORTED;
  if (M == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && q && s);
  const int64_t nblocks = M * (K / 32);
  const int64_t grid = (nblocks * 4 + 255) / 256;
  if (grid > 0x7FFFFFFF) return ISIC_ERR_UNSUPPORTED;
  if (x_is_f32)
    hipLaunchKernelGGL((mx_quantize_kernel<true>), dim3((unsigned)grid), dim3(256), 0, as_stream(stream), x, q, s, nblocks, K);
  else
    hipLaunchKernelGGL((mx_quantize_kernel<false>), dim3((unsigned)grid), dim3(256), 0, as_stream(stream), x, q, s, nblocks, K);
  return isic_launch_status();
}

int isic_layernorm_mxfp8_f16(const uint16_t* x, const float* gamma, const float* beta, uint8_t* q, uint8_t* s, int64_t M,
                             int N, float eps, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && N > 0 && eps >= 0.f);
  if (N != 384) return ISIC_ERR_UNSUPPORTED;
  if (M == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && gamma && beta && q && s);
  int64_t g = (M + 16 - 1) / 16;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL((layernorm_f16_kernel<64, 48, LN_OUT_MX>), dim3((int)g), dim3(256), 0, as_stream(stream), x, gamma, beta,
                     q, s, M, eps);
  return isic_launch_status();
}

int isic_gemm_mxfp8(const uint8_t* A_q, const uint8_t* A_s, const uint8_t* W_q, const uint8_t* W_s, const float* bias,
                    const uint16_t* residual, uint16_t* C, uint8_t* C_q, uint8_t* C_s, int M, int N, int K, int act,
                    int residual_rows, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && N > 0 && K > 0 && (act == 0 || act == 1) && residual_rows >= 0);
  ISIC_CHECK_ARG((C != nullptr) != (C_q != nullptr));                 // exactly one output form
  ISIC_CHECK_ARG(C_q == nullptr || C_s != nullptr);
  ISIC_CHECK_ARG(residual || residual_rows == 0);
  if (N % MG_N != 0 || K % MG_K != 0) return ISIC_ERR_UNSUPPORTED;
  if (M == 0) return ISIC_OK;
  ISIC_CHECK_ARG(A_q && A_s && W_q && W_s);
  MxGemmArgs a;
  a.A = A_q; a.As = A_s; a.W = W_q; a.Ws = W_s; a.bias = bias; a.res = residual; a.C = C; a.Cq = C_q; a.Cs = C_s;
  a.M = M; a.N = N; a.K = K; a.res_rows = residual_rows;
  a.mtiles = (M + MG_M - 1) / MG_M;
  a.ntiles = N / MG_N;
  const int64_t total = (int64_t)a.mtiles * a.ntiles;
  if (total > 0x7FFFFFF0) return ISIC_ERR_UNSUPPORTED;
  a.ntiles_total = (int)total;
  hipStream_t s = as_stream(stream);
  const bool mx = C_q != nullptr;
  if (act == 1) return residual ? launch_mx_out<1, true>(a, mx, s) : launch_mx_out<1, false>(a, mx, s);
  return residual ? launch_mx_out<0, true>(a, mx, s) : launch_mx_out<0, false>(a, mx, s);
}

}  // extern "C"
