// ViT-S/16 companions of gemm_f16.hip (gfx950, fp16 activations, fp32 arithmetic inside): patch extraction, LayerNorm
// over 384-wide token rows, and multi-head self-attention over the 196 tokens of one image on MFMA.
//
// The reference's encoder is an un-vendored ConvMAE conv-ViT run frozen (save_latent.py:42-60); these implement the
// ViT-S/16 named by BASELINE.json configs[4] with timm semantics (pre-norm blocks, LayerNorm eps 1e-6, scaled dot
// product attention without a class token or masking: save_latent.py passes mask_ratio = 0).  oracle/vit.py is the fp32
// CPU restatement.

#include "common.h"
#include "ln_rows.inc"       // layernorm_f16_kernel: the row LayerNorm of isic_layernorm_f16 and isic_row_stats_f16

namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- patches
// images NCHW (fp32 or bf16/fp16 bits are not mixed here: fp32 in) -> rows [n*gh*gw + py*gw + px][c*P*P + ky*P + kx]
// fp16: the im2col of a PxP / stride P convolution (Conv2d weight [D][C][P][P] flattened is then a Linear weight).
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ img, unsigned short* __restrict__ out,
                                                        int N, int C, int H, int W, int P) {
  const int gh = H / P, gw = W / P, K = C * P * P, kv = K >> 3;
  const int64_t nvec = (int64_t)N * gh * gw * kv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
    const int k0 = (int)(i % kv) * 8;
    const int64_t row = i / kv;
    const int px = (int)(row % gw), py = (int)((row / gw) % gh), n = (int)(row / ((int64_t)gw * gh));
    const int c = k0 / (P * P), r = k0 - c * P * P, ky = r / P, kx = r - ky * P;      // P % 8 == 0: 8 values share (c, ky)
    const float* src = img + (((size_t)n * C + c) * H + (py * P + ky)) * W + px * P + kx;
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
    const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    *reinterpret_cast<u32x4*>(out + i * 8) = f16_pack8(f);
  }
}

// ---------------------------------------------------------------- attention
// One block (8 waves) per (image, head): T <= 208 tokens, head width 64.  K and V row-major in LDS ([token][64] = 128-byte
// rows; 16-byte chunks XOR-swizzled by token & 7 for K, by (token >> 1) & 7 for V); Q is never staged: a wave reads the two
// 16-byte fragments of its 16 queries straight from global memory.  54 KB of LDS: two blocks per CU (register-limited), so
// one block's loads overlap the other's arithmetic.  A wave owns query tiles of 16: S^T = K.Q^T on
// v_mfma_f32_16x16x32_f16 (13 key tiles x 2 k-steps; a lane then holds, for ITS query l % 16, the scores of keys
// 16t + 4(l/16) + r), softmax over keys = in-lane over the 52 values + two xor shuffles; the probabilities are already
// in operand position of P.V up to a permutation of the contraction index (k-slot 8(l/16) + e <-> key
// 32u + 16(e/4) + 4(l/16) + e%4), which the V fragments follow.
// Round 3: O^T = V^T.P^T instead of O = P.V.  The V^T fragment (head dimension x keys) comes out of the row-major V with
// ds_read_b64_tr_b16 -- a 16-lane group addresses 4 keys x 16 head dimensions and each lane receives ONE dimension's four
// keys -- so V is staged with 16-byte writes like K (it was 32 ds_write_b16 per thread into a transposed copy); the head
// dimensions a group addresses are chosen so that a lane ends with EIGHT CONSECUTIVE dimensions of its own query
// (d = 32 (jd >> 1) + 8 (l / 16) + 4 (jd & 1) + r): the result is normalised with the lane's own 1 / sum and leaves in two
// 16-byte stores, no LDS transpose, no shuffles.
// Templated on the head width HD in {32, 64} (the MAE decoder's heads are 32 wide): a K / V row is HD * 2 bytes = HD / 8
// chunks of 16 bytes, swizzled by the same token bits masked to HD / 8 - 1; S^T takes HD / 32 k-steps and O^T HD / 16
// head-dimension tiles.  HD = 64 is the kernel described above, instruction for instruction.
constexpr int AT_TMAX = 208, AT_KPAD = 224;                          // tokens padded to 13 x 16 (scores) / 7 x 32 (P.V)
constexpr int AT_WAVES = 8;
template <int HD> constexpr int at_lds() { return (AT_TMAX + AT_KPAD) * HD * 2; }

template <int HD>
__global__ __launch_bounds__(AT_WAVES * 64, 2) void attention_f16_kernel(const unsigned short* __restrict__ qkv,
                                                                          unsigned short* __restrict__ out, int T,
                                                                          int heads, float scale_log2e) {
  static_assert(HD == 32 || HD == 64, "head width 32 or 64");
  constexpr int RB = HD * 2, CH = HD / 8, SW = CH - 1, KS = HD / 32, JD = HD / 16;   // row bytes, chunks, swizzle mask
  constexpr int AT_K = AT_TMAX * RB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* Ks = smem;
  unsigned char* Vs = smem + AT_K;
  typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
  const unsigned vs0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)Vs;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x / heads, head = blockIdx.x - img * heads;
  const int D = heads * HD, ld = 3 * D;                               // qkv row: [q heads*HD | k heads*HD | v heads*HD]
  const unsigned short* base = qkv + (size_t)img * T * ld + head * HD;
  const int fr = lane & 15, fg = lane >> 4;
  const int qtiles = (T + 15) >> 4;

  // ---- this wave's first query fragments (global -> registers), in flight while K and V are staged
  auto load_q = [&](int qt, f16x8 (&qf)[KS]) {
    const int q = min(qt * 16 + fr, T - 1);                           // rows >= T: any valid row, never stored
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      qf[ks] = *reinterpret_cast<const f16x8*>(base + (size_t)q * ld + (ks * 4 + fg) * 8);
  };
  f16x8 qf[KS];
  if (wave < qtiles) load_q(wave, qf);

  // ---- stage K (swizzled rows of 128 B) and V^T; rows >= T are zero.  All of a thread's loads first, then the stores.
  constexpr int KV_PER = (AT_KPAD * CH + AT_WAVES * 64 - 1) / (AT_WAVES * 64);     // 4 (HD 64) / 2 (HD 32) vectors per thread
  u32x4 kr[KV_PER], vr[KV_PER];
#pragma unroll
  for (int u = 0; u < KV_PER; ++u) {
    const int idx = tid + u * AT_WAVES * 64, t = idx / CH, ch = idx % CH;
    kr[u] = (u32x4){0u, 0u, 0u, 0u};
    vr[u] = kr[u];
    if (t < T) {
      kr[u] = *reinterpret_cast<const u32x4*>(base + (size_t)t * ld + D + ch * 8);
      vr[u] = *reinterpret_cast<const u32x4*>(base + (size_t)t * ld + 2 * D + ch * 8);
    }
  }
#pragma unroll
  for (int u = 0; u < KV_PER; ++u) {
    const int idx = tid + u * AT_WAVES * 64, t = idx / CH, ch = idx % CH;
    if (t < AT_TMAX) *reinterpret_cast<u32x4*>(Ks + t * RB + ((ch ^ (t & SW)) << 4)) = kr[u];
    if (t < AT_KPAD) *reinterpret_cast<u32x4*>(Vs + t * RB + ((ch ^ ((t >> 1) & SW)) << 4)) = vr[u];
  }
  __syncthreads();

  // V^T fragment addresses: lane (fg, fq, fp) of a 16-lane group reads key 4fg + fq (+ 32u, + 16 for the upper half), the four
  // head dimensions 32 (jd >> 1) + 8 fp + 4 (jd & 1) + {0..3}: chunk (jd >> 1) * 4 + fp, swizzled by (key >> 1) & 7 (the
  // same for every u and both halves), byte (jd & 1) * 8 inside it.  16 keys x 4 x 8 bytes per instruction spread over half
  // of the banks evenly: the b64 rate.
  unsigned voff[JD];
  {
    const int fq = fr >> 2, fp = fr & 3, key = 4 * fg + fq, hsw = (key >> 1) & SW;
#pragma unroll
    for (int jd = 0; jd < JD; ++jd)
      voff[jd] = vs0 + (unsigned)(key * RB + ((((jd >> 1) * 4 + fp) ^ hsw) << 4) + (jd & 1) * 8);
  }
  for (int qt = wave; qt < qtiles; qt += AT_WAVES) {
    // ---- S^T tile row: keys x this tile's 16 queries
    f32x4 s[13];
#pragma unroll
    for (int kt = 0; kt < 13; ++kt) {
      const int krow = kt * 16 + fr;
      s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f16x8 kf = *reinterpret_cast<const f16x8*>(Ks + krow * RB + (((ks * 4 + fg) ^ (krow & SW)) << 4));
        s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[ks], s[kt], 0, 0, 0);   // D[key 4fg+r][query fr]
      }
    }
    if (qt + AT_WAVES < qtiles) load_q(qt + AT_WAVES, qf);            // next tile's queries under the softmax
    // ---- softmax over the keys of query fr (base-2 exponent, scale folded in); keys >= T masked out
    // The softmax is what this kernel spends its issue slots on (52 values per lane and tile against 54 MFMAs): the maximum is
    // taken over the RAW scores (the scale is positive), scale and shift are one FMA, the exponential is the bare v_exp_f32
    // (results below 2^-126 flush to zero: they are rounded to fp16 next), and only a key tile that crosses T is masked.
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 13; ++kt) {
      if (kt * 16 + 16 > T) {                                         // wave-uniform: at most the last tiles
        asm volatile("" ::: "memory");                                // a real branch: if-converted, it costs 2 selects per value
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kt][r] = kt * 16 + fg * 4 + r < T ? s[kt][r] : -INFINITY;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float shift = -mx * scale_log2e;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 13; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kt][r] = __builtin_amdgcn_exp2f(fmaf(s[kt][r], scale_log2e, shift));
        sum += s[kt][r];
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;                                      // of query fr

    // ---- O^T = V^T.P^T: 7 key blocks of 32 (tiles 2u, 2u+1; tile 13 does not exist: zeros), 4 head-dimension tiles of 16
    f32x4 o[JD];
#pragma unroll
    for (int jd = 0; jd < JD; ++jd) o[jd] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 7; ++u) {
      f16x8 pf;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pf[r] = (_Float16)s[2 * u][r];
        pf[4 + r] = (2 * u + 1 < 13) ? (_Float16)s[2 * u + 1 < 13 ? 2 * u + 1 : 12][r] : (_Float16)0.f;
      }
#pragma unroll
      for (int jd = 0; jd < JD; ++jd) {
        s16x8_t t;
        t.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)(voff[jd] + (unsigned)(u * 32 * RB)));
        t.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)(voff[jd] + (unsigned)(u * 32 * RB + 16 * RB)));
        o[jd] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, t), pf, o[jd], 0, 0, 0);   // D[d-slot 4fg+r][query fr]
      }
    }
    // ---- normalise with the lane's own 1 / sum; dimensions 32t' + 8fg + {0..7} of query fr: two 16-byte stores
    const int q = qt * 16 + fr;
#pragma unroll
    for (int tp = 0; tp < HD / 32; ++tp) {
      u32x4 v;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 c = o[2 * tp + h] * inv;
        const f16x2 p0 = {(_Float16)c[0], (_Float16)c[1]}, p1 = {(_Float16)c[2], (_Float16)c[3]};
        v[2 * h] = __builtin_bit_cast(unsigned, p0);
        v[2 * h + 1] = __builtin_bit_cast(unsigned, p1);
      }
      if (q < T) *reinterpret_cast<u32x4*>(out + ((size_t)img * T + q) * D + head * HD + 32 * tp + 8 * fg) = v;
    }
  }
}

// One dispatch for the two entry points over layernorm_f16_kernel (o0, o1: the mode's outputs, csrc/ln_rows.inc): a block
// takes 256 / LPR rows per pass, the grid four passes' worth of blocks up to 8192.
template <LnOut OUT>
int ln16_launch(const uint16_t* x, const float* gamma, const float* beta, void* o0, void* o1, int64_t M, int N, float eps,
                       void* stream) {
  int64_t g;
#define LAUNCH_LN16(LPR, ACT)                                                                                    \
  g = (M + (256 / LPR) * 4 - 1) / ((256 / LPR) * 4);                                                             \
  if (g > 8192) g = 8192;                                                                                        \
  hipLaunchKernelGGL((layernorm_f16_kernel<LPR, ACT, OUT>), dim3((int)g), dim3(256), 0, as_stream(stream), x, gamma, beta, \
                     o0, o1, M, eps)
  if (N == 128) { LAUNCH_LN16(16, 16); }
  else if (N == 256) { LAUNCH_LN16(32, 32); }
  else if (N == 384) { LAUNCH_LN16(64, 48); }
  else if (N == 512) { LAUNCH_LN16(64, 64); }
  else return ISIC_ERR_UNSUPPORTED;
#undef LAUNCH_LN16
  return isic_launch_status();
}

}  // namespace

extern "C" {

int isic_vit_patchify_f16(const float* images_nchw, uint16_t* rows, int N, int C, int H, int W, int P, void* stream) {
  ISIC_CHECK_ARG(images_nchw && rows && N > 0 && C > 0 && H > 0 && W > 0 && P > 0);
  if (P % 8 != 0 || H % P != 0 || W % P != 0 || W % 4 != 0) return ISIC_ERR_UNSUPPORTED;
  const int64_t nvec = (int64_t)N * (H / P) * (W / P) * (C * P * P / 8);
  int64_t g = (nvec + 255) / 256;
  if (g > 16384) g = 16384;
  hipLaunchKernelGGL(patchify_kernel, dim3((int)g), dim3(256), 0, as_stream(stream), images_nchw, rows, N, C, H, W, P);
  return isic_launch_status();
}

int isic_layernorm_f16(const uint16_t* x, const float* gamma, const float* beta, uint16_t* y, float* y_f32, int64_t M,
                       int N, float eps, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && N > 0);
  if (M == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && gamma && beta && (y || y_f32));
  return ln16_launch<LN_OUT_Y>(x, gamma, beta, y, y_f32, M, N, eps, stream);
}

int isic_row_stats_f16(const uint16_t* x, float* stats, int64_t M, int N, float eps, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && N > 0);
  if (M == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && stats);
  return ln16_launch<LN_OUT_STATS>(x, nullptr, nullptr, nullptr, stats, M, N, eps, stream);
}

int isic_attention_f16(const uint16_t* qkv, uint16_t* out, int n_images, int tokens, int heads, int head_dim,
                       void* stream) {
  ISIC_CHECK_ARG(n_images >= 0 && tokens > 0 && heads > 0);
  if (head_dim != 64 || tokens > AT_TMAX) return ISIC_ERR_UNSUPPORTED;
  if (n_images == 0) return ISIC_OK;
  ISIC_CHECK_ARG(qkv && out);
  const float scale_log2e = 0.125f * 1.4426950408889634f;            // 1 / sqrt(64), base-2 exponent
  return isic_launch_lds<attention_f16_kernel<64>, at_lds<64>()>(dim3(n_images * heads), dim3(AT_WAVES * 64), at_lds<64>(),
                                                                 as_stream(stream), qkv, out, tokens, heads, scale_log2e);
}

// include/isic_hip_mae.h: the MAE decoder's heads, 32 wide
int isic_attention_d32_f16(const uint16_t* qkv, uint16_t* out, int n_images, int tokens, int heads, void* stream) {
  ISIC_CHECK_ARG(n_images >= 0 && tokens > 0 && heads > 0);
  if (tokens > AT_TMAX) return ISIC_ERR_UNSUPPORTED;
  if (n_images == 0) return ISIC_OK;
  ISIC_CHECK_ARG(qkv && out);
  const float scale_log2e = 0.17677669529663688f * 1.4426950408889634f;   // 1 / sqrt(32), base-2 exponent
  return isic_launch_lds<attention_f16_kernel<32>, at_lds<32>()>(dim3(n_images * heads), dim3(AT_WAVES * 64), at_lds<32>(),
                                                                 as_stream(stream), qkv, out, tokens, heads, scale_log2e);
}

}  // extern "C"
