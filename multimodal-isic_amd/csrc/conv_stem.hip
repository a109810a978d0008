// ResNet stem convolution 7x7 / stride 2 / pad 3, 3 -> 64 channels, on bf16 MFMA (gfx950).
//
// Cin = 3 is too thin for the generic implicit GEMM (K-tiles of 64 channels), so the stem gets its
// own direct kernels.  The input is NHWC with C padded to 4 (8 bytes per pixel); a block stages the
// (21 x 40)-pixel input patch of an 8 x 16 output tile in LDS once and every MFMA A-fragment is a
// single ds_read_b128 out of it: for output pixel (oy,ox) and kernel row kh the 8 taps kw = 0..7
// (the 8th is a zero-weight pad) x 4 channels are 32 CONTIGUOUS bf16 of patch row 2*oy+kh starting
// at column 2*ox, so K = 7 steps of 32.  Weights are packed [64][7][8][4] (kw, c zero padded).
//
// The weight gradient uses the same patch: K = pixels, the dY tile is staged [pixel][co] and both
// operands are fetched with the transposing LDS read ds_read_b64_tr_b16 (for the input operand each
// lane addresses its own pixel's 4 taps x 4 channels = 8 contiguous bytes).
//
// No counterpart in the reference (encoder un-vendored, save_latent.py:42-60); ResNet-18 layer
// table: SURVEY.md 8d (conv1: 118 MMAC per 224x224 image).
#include <type_traits>

#include "common.h"
#include "slab_sum.inc"
#include "mfma_tile.h"
#include "pool_grad.h"
#include "bn_bwd_math.inc"

namespace {

constexpr int TH = 8, TW = 16;             // output tile
constexpr int PR = 2 * TH + 5, PC = 40;    // patch rows (21) / cols (38 used, 40 allocated)
constexpr int PROW = PC * 8;               // bytes per patch row (4 bf16 per pixel)
constexpr int WROW = 7 * 64 + 16;          // bytes per co row of the LDS weight image (padded: conflict-free)
constexpr int YROW = 128 + 32;             // bytes per pixel row of the staged dY tile
constexpr int STEM_DW_ELEMS = 64 * 7 * 7 * 3;   // the weight gradient, [co][kh][kw][c]
constexpr int STEM_WGRAD_BLOCKS = 512;
constexpr int STEM_FWD_BLOCKS = 768;       // persistent blocks of the forward kernel: three per CU (LDS, registers)     // persistent blocks of the weight-gradient kernels (one partial each)

struct StemArgs {
  const unsigned short* in;   // [N,Hin,Win,4]
  const unsigned short* w;    // [64][7][8][4]
  unsigned short* out;        // [N,Hout,Wout,64]
  const unsigned short* dy;   // wgrad: [N,Hout,Wout,64]
  float* dw;                  // wgrad: [64][7][7][3] fp32
  double* stat_sum;           // fwd, optional: [slots][64] BatchNorm sum / sum of squares of the rounded outputs
  double* stat_sumsq;
  int stat_slots;
  int N, Hin, Win, Hout, Wout, tiles_h, tiles_w, total_tiles;
};

// The input patch of a tile, staged in two halves -- global loads into registers, registers into LDS -- so that the
// loads of the NEXT tile are in flight while the current tile is multiplied (PR * PC = 840 pixels: at most 4 per thread).
// patch pixel (pr, pc) = input pixel (2*oy0 - 3 + pr, 2*ox0 - 3 + pc); 8 bytes each
constexpr int PATCH_PER_THREAD = (PR * PC + 255) / 256;
__device__ __forceinline__ void fetch_patch(u32x2 (&r)[PATCH_PER_THREAD], const StemArgs& a, int tile, int tid) {
  const int n = tile / (a.tiles_h * a.tiles_w);
  const int t2 = tile - n * (a.tiles_h * a.tiles_w);
  const int oy0 = (t2 / a.tiles_w) * TH, ox0 = (t2 % a.tiles_w) * TW;
#pragma unroll
  for (int u = 0; u < PATCH_PER_THREAD; ++u) {
    const int idx = tid + 256 * u;
    const int pr = idx / PC, pc = idx - pr * PC;
    const int hi = 2 * oy0 - 3 + pr, wi = 2 * ox0 - 3 + pc;
    u32x2 v = {0u, 0u};
    if (tile < a.total_tiles && idx < PR * PC && hi >= 0 && hi < a.Hin && wi >= 0 && wi < a.Win)
      v = *reinterpret_cast<const u32x2*>(a.in + (((size_t)n * a.Hin + hi) * a.Win + wi) * 4);
    r[u] = v;
  }
}
__device__ __forceinline__ void commit_patch(unsigned char* Ps, const u32x2 (&r)[PATCH_PER_THREAD], int tid) {
#pragma unroll
  for (int u = 0; u < PATCH_PER_THREAD; ++u) {
    const int idx = tid + 256 * u;
    if (idx < PR * PC) {
      const int pr = idx / PC, pc = idx - pr * PC;
      *reinterpret_cast<u32x2*>(Ps + pr * PROW + pc * 8) = r[u];
    }
  }
}

// Forward: register-only epilogue.  The block's LDS weight image holds the 64 packed rows PERMUTED -- MFMA tile j, row m
// is output channel 32 (j >> 1) + 8 (m >> 2) + 4 (j & 1) + (m & 3) -- so that after the MFMAs (operand roles swapped,
// D[co][pixel]) lane (fg, fi) holds, of pixel column fi, channels 8 fg .. 8 fg + 7 in tiles 0, 1 and 32 + 8 fg .. + 7 in
// tiles 2, 3: the 16 bytes at column group fg of both 64-byte halves of the pixel's 128-byte row, which is what
// isic_pair_rows (common.h) wants.  No C tile in LDS and no barrier after the MFMAs (two per tile, 36 KB of LDS); the
// packed [64][7][8][4] weights in memory are unchanged.  What the epilogue's round trip through LDS cost was small
// (2.32 -> 2.23 ms at 4096 images); the larger part of this kernel's time beside its memory traffic was vector-ALU work
// per tile, so, as in the fused weight gradient, the tile loop keeps only what forms a value of the result (-> 1.91 ms):
// scalar tile coordinates advanced by carries, per-thread patch coordinates and offsets computed once, a block-uniform
// path without validity selects and store guards for tiles whose outputs all exist, two values per v_cvt_pk_bf16_f32,
// the statistics a template parameter instead of a branch per MFMA tile.
// Measured and left out: a second patch buffer for one barrier per tile (2.233 vs 2.231 ms), two cached
// 64-byte stores per lane instead of the half-row swap (2.31 vs 2.23 ms), weight fragments held in registers (does not
// fit 168 VGPRs without scratch).  The persistent grid stays 768 blocks: a block's fp32 partial sums, and with them the
// last bits of the statistics, depend on which tiles it owns.
__device__ __forceinline__ int stem_fwd_lds_row(int co) {
  return (2 * (co >> 5) + ((co >> 2) & 1)) * 16 + 4 * ((co >> 3) & 3) + (co & 3);
}
__device__ __forceinline__ int stem_fwd_channel(int j, int fg, int r) { return 32 * (j >> 1) + 8 * fg + 4 * (j & 1) + r; }

// s[e] += r[e], q[e] += r[e] * r[e] for the four rounded values in (lo, hi), the product rounded by itself: the
// multiply and the add stay separate instructions, as hipcc has always compiled these sums (it prefers packed adds to
// fused multiply-adds here), so that the statistics do not depend on that choice
__device__ __forceinline__ void stem_stat4(float* s, float* q, unsigned lo, unsigned hi) {
#pragma clang fp contract(off)
  const float r0 = __uint_as_float(lo << 16), r1 = __uint_as_float(lo & 0xFFFF0000u);
  const float r2 = __uint_as_float(hi << 16), r3 = __uint_as_float(hi & 0xFFFF0000u);
  s[0] += r0; q[0] += r0 * r0;
  s[1] += r1; q[1] += r1 * r1;
  s[2] += r2; q[2] += r2 * r2;
  s[3] += r3; q[3] += r3 * r3;
}

struct StemTile { int n, oy0, ox0; };           // block-uniform tile coordinates, advanced without divisions

// STATS: with the fused BatchNorm sums (a.stat_sum / a.stat_sumsq); three blocks per CU (<= 168 VGPRs)
template <bool STATS>
__global__ __launch_bounds__(256, 3) void conv_stem_fwd_kernel(StemArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[64 * WROW + PR * PROW];
  unsigned char* Ws = smem;
  unsigned char* Ps = smem + 64 * WROW;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fi = lane & 15, fg = lane >> 4;

  // weights -> LDS once per block: 64 rows x 448 bytes (28 chunks of 16 B), row co at its permuted place
  for (int idx = tid; idx < 64 * 28; idx += 256) {
    const int co = idx / 28, ch = idx - co * 28;
    *reinterpret_cast<u32x4*>(Ws + stem_fwd_lds_row(co) * WROW + ch * 16) =
        *reinterpret_cast<const u32x4*>(a.w + co * 224 + ch * 8);
  }

  // ---- tile cursor: tile += gridDim.x as (n, oy0, ox0) += (step_n, step_y, step_x) with carries, in scalar registers
  const int tiles_img = a.tiles_h * a.tiles_w;
  const int step_n = (int)gridDim.x / tiles_img, step_r = (int)gridDim.x - step_n * tiles_img;
  const int step_y = (step_r / a.tiles_w) * TH, step_x = (step_r % a.tiles_w) * TW;
  const int span_y = a.tiles_h * TH, span_x = a.tiles_w * TW;
  auto advance = [&](StemTile& t) {
    t.ox0 += step_x;
    if (t.ox0 >= span_x) { t.ox0 -= span_x; t.oy0 += TH; }
    t.oy0 += step_y;
    if (t.oy0 >= span_y) { t.oy0 -= span_y; t.n += 1; }
    t.n += step_n;
  };
  // ---- this thread's patch pixels (idx = tid + 256 u): patch coordinates and in-image byte offset, the same for every tile
  int ppr[PATCH_PER_THREAD], ppc[PATCH_PER_THREAD];
  unsigned poff[PATCH_PER_THREAD];
#pragma unroll
  for (int u = 0; u < PATCH_PER_THREAD; ++u) {
    const int idx = tid + 256 * u;
    const bool have = idx < PR * PC;
    ppr[u] = have ? idx / PC : -(1 << 24);                               // padding: never inside the image
    ppc[u] = idx % PC;
    poff[u] = have ? (unsigned)((ppr[u] * a.Win + ppc[u]) * 8) : 0u;
  }
  u32x2 pre[PATCH_PER_THREAD];
  auto fetch = [&](const StemTile& t, bool live) {
    const int hi0 = 2 * t.oy0 - 3, wi0 = 2 * t.ox0 - 3;
    const unsigned char* org = reinterpret_cast<const unsigned char*>(a.in) + (((int64_t)t.n * a.Hin + hi0) * a.Win + wi0) * 8;
#pragma unroll
    for (int u = 0; u < PATCH_PER_THREAD; ++u) {
      u32x2 v = {0u, 0u};
      if (live && (unsigned)(hi0 + ppr[u]) < (unsigned)a.Hin && (unsigned)(wi0 + ppc[u]) < (unsigned)a.Win)
        v = *reinterpret_cast<const u32x2*>(org + poff[u]);
      pre[u] = v;
    }
  };

  StemTile cur;
  {
    const int bid = blockIdx.x, t2 = bid % tiles_img;
    cur.n = bid / tiles_img; cur.oy0 = (t2 / a.tiles_w) * TH; cur.ox0 = (t2 % a.tiles_w) * TW;
  }
  fetch(cur, true);
  // fused BatchNorm statistics of the ROUNDED outputs, in registers over all tiles of the block: lane (fg, fi) owns
  // channels stem_fwd_channel(j, fg, r) of pixel column fi -- 16 sums + 16 sums of squares (fp32; ~800 values each),
  // reduced over the 16 lanes of a DPP row and the four waves once, at the end.  A channel's values are added in the
  // order they always were (tiles of the block, rows i, then columns by the butterfly, then waves): only the lane and
  // slot that hold a channel depend on the permutation.
  float st_s[4][4], st_q[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) { st_s[j][r] = 0.f; st_q[j][r] = 0.f; }
  const unsigned frag_p = (unsigned)(4 * wave * PROW + (2 * fi + 2 * fg) * 8);
  const unsigned frag_w = (unsigned)(fi * WROW + fg * 16);
  const unsigned lane_o = (unsigned)(((fi & ~1) * 64 + 8 * fg + ((fi & 1) ? 32 : 0)) * 2);   // bytes from the tile row's first pixel

  for (int tile = blockIdx.x; tile < a.total_tiles; tile += gridDim.x) {
    StemTile nxt = cur;
    advance(nxt);
    lds_barrier();                                       // previous tile's patch fully consumed / weights visible
#pragma unroll
    for (int u = 0; u < PATCH_PER_THREAD; ++u)
      if (tid + 256 * u < PR * PC) *reinterpret_cast<u32x2*>(Ps + (tid + 256 * u) * 8) = pre[u];       // PROW = 8 PC
    lds_barrier();                                       // (NOT __syncthreads(): that drains vmcnt, i.e. waits for the previous
                                                         //  tile's output stores to complete their round trip to memory)
    fetch(nxt, tile + (int)gridDim.x < a.total_tiles);   // next tile's loads fly under this tile's MFMAs and stores

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < 7; ++kh) {
      bf16x8 af[2], bfr[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const bf16x8*>(Ps + frag_p + (2 * i + kh) * PROW);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = *reinterpret_cast<const bf16x8*>(Ws + frag_w + j * 16 * WROW + kh * 64);
      // swapped operand roles, D[co][pixel]: lane (fg, fi) ends with LDS rows 16j + 4fg + {0..3} of pixel fi
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
    }
    // epilogue from registers: pixel (oy, ox0 + fi), 16 bytes at column group fg of each 64-byte half; adjacent lanes
    // (pixels fi, fi ^ 1) swap one half, so that a store instruction writes whole 128-byte pixel rows.  A tile whose
    // outputs all exist (block-uniform, the usual case) takes the path without validity selects and store guards.
    const bool full = cur.oy0 + TH <= a.Hout && cur.ox0 + TW <= a.Wout;
    unsigned char* otile = reinterpret_cast<unsigned char*>(a.out) +
                           (((int64_t)cur.n * a.Hout + cur.oy0) * a.Wout + cur.ox0) * 128;
    auto epilogue = [&](auto full_c) {
      constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int oyl = wave * 2 + i;
        const bool in = FULL || ((cur.oy0 + oyl < a.Hout) && (cur.ox0 + fi < a.Wout));
        u32x4 vv[2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned w0 = isic_pack_bf16x2(acc[i][j][0], acc[i][j][1]), w1 = isic_pack_bf16x2(acc[i][j][2], acc[i][j][3]);
          vv[j >> 1][2 * (j & 1)] = w0;
          vv[j >> 1][2 * (j & 1) + 1] = w1;
          if (STATS) stem_stat4(st_s[j], st_q[j], in ? w0 : 0u, in ? w1 : 0u);
        }
        u32x4 da, db;
        isic_pair_rows(vv[0], vv[1], fi & 1, da, db);
        unsigned char* o = otile + (int64_t)oyl * a.Wout * 128 + lane_o;
        const bool row = FULL || cur.oy0 + oyl < a.Hout;
        if (row && (FULL || cur.ox0 + (fi & ~1) < a.Wout)) __builtin_nontemporal_store(da, reinterpret_cast<u32x4*>(o));
        if (row && (FULL || cur.ox0 + (fi | 1) < a.Wout)) __builtin_nontemporal_store(db, reinterpret_cast<u32x4*>(o + 128));
      }
    };
    if (full) epilogue(std::true_type{});
    else epilogue(std::false_type{});
    cur = nxt;
  }
  if (STATS) {
    // DPP row sums over the 16 pixel columns, then the four waves meet in LDS
    __shared__ float stat_red[2][4][64];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sv = st_s[j][r], qv = st_q[j][r];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { sv += __shfl_xor(sv, o, 16); qv += __shfl_xor(qv, o, 16); }
        const int c = stem_fwd_channel(j, fg, r);
        if (fi == 0) { stat_red[0][wave][c] = sv; stat_red[1][wave][c] = qv; }
      }
    lds_barrier();
    if (tid < 128) {
      const int c = tid & 63, w = tid >> 6;
      const float t = (stat_red[w][0][c] + stat_red[w][1][c]) + (stat_red[w][2][c] + stat_red[w][3][c]);
      const size_t slot = (size_t)(blockIdx.x % a.stat_slots) * 64 + c;
      atomicAdd((w == 0 ? a.stat_sum : a.stat_sumsq) + slot, (double)t);
    }
  }
}

__global__ __launch_bounds__(256) void conv_stem_wgrad_kernel(StemArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[PR * PROW + TH * TW * YROW];
  unsigned char* Ps = smem;
  unsigned char* Ys = smem + PR * PROW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fg = lane >> 4, fi = lane & 15, fq = fi >> 2, fp = fi & 3;
  typedef __attribute__((address_space(3))) s16x4* lds_s16x4;

  // n-tiles: nt = kh*2 + half (14 of them); wave w owns nt = w, w+4, w+8, w+12
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // operands of the next tile are fetched into registers while the current one is multiplied
  u32x2 pre[PATCH_PER_THREAD];
  u32x4 prey[4];
  auto fetch_dy = [&](int tile) {
    const int n = tile / (a.tiles_h * a.tiles_w);
    const int t2 = tile - n * (a.tiles_h * a.tiles_w);
    const int oy0 = (t2 / a.tiles_w) * TH, ox0 = (t2 % a.tiles_w) * TW;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = tid + 256 * u;
      const int p = idx >> 3, ch = idx & 7;
      const int oy = oy0 + (p >> 4), ox = ox0 + (p & 15);
      u32x4 v = {0u, 0u, 0u, 0u};
      if (tile < a.total_tiles && oy < a.Hout && ox < a.Wout)
        v = *reinterpret_cast<const u32x4*>(a.dy + (((size_t)n * a.Hout + oy) * a.Wout + ox) * 64 + ch * 8);
      prey[u] = v;
    }
  };
  fetch_patch(pre, a, blockIdx.x, tid);
  fetch_dy(blockIdx.x);
  for (int tile = blockIdx.x; tile < a.total_tiles; tile += gridDim.x) {
    lds_barrier();                                       // previous tile's operands fully consumed
    commit_patch(Ps, pre, tid);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int idx = tid + 256 * u;
      *reinterpret_cast<u32x4*>(Ys + (idx >> 3) * YROW + (idx & 7) * 16) = prey[u];
    }
    lds_barrier();
    fetch_patch(pre, a, tile + gridDim.x, tid);
    fetch_dy(tile + gridDim.x);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k1 = ks * 32 + 8 * fg + fq, k2 = k1 + 4;   // the two pixel rows this lane addresses
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(Ys + k1 * YROW + (i * 16 + 4 * fp) * 2));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(Ys + k2 * YROW + (i * 16 + 4 * fp) * 2));
        s16x8_t t; t.lo = lo; t.hi = hi;
        af[i] = __builtin_bit_cast(bf16x8, t);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int nt = wave + 4 * j;
        const int kh = nt >> 1, half = nt & 1;
        // nt >= 14 would address past the taps: clamp the address (result discarded at the end)
        const int khc = kh > 6 ? 6 : kh;
        const unsigned char* p1 = Ps + (2 * (k1 >> 4) + khc) * PROW + (2 * (k1 & 15) + half * 4 + fp) * 8;
        const unsigned char* p2 = Ps + (2 * (k2 >> 4) + khc) * PROW + (2 * (k2 & 15) + half * 4 + fp) * 8;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)p1);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)p2);
        s16x8_t t; t.lo = lo; t.hi = hi;
        bfr[j] = __builtin_bit_cast(bf16x8, t);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  }
  // dw[co][kh][kw][c], c < 3, kw < 7
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nt = wave + 4 * j;
      if (nt >= 14) continue;
      const int kh = nt >> 1, kw = (nt & 1) * 4 + (fi >> 2), c = fi & 3;
      if (kw >= 7 || c >= 3) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = i * 16 + fg * 4 + r;
        // the block's OWN partial (workspace [grid][64*7*7*3]); isic_slab_reduce_launch adds them in a fixed order:
        // deterministic, where fp32 atomics added the blocks in arrival order
        a.dw[(size_t)blockIdx.x * STEM_DW_ELEMS + ((co * 7 + kh) * 7 + kw) * 3 + c] = acc[i][j][r];
      }
    }
}

// ---------------------------------------------------------------- weight gradient fed by the POOLED gradient
// Same tiles and MFMA schedule as conv_stem_wgrad_kernel, but the dY tile is never read from memory: it is the
// BatchNorm(+ReLU) backward of the 3x3/2 max-pool backward of the pooled gradient, formed in registers from the stem
// activation y0 (read once, here), the pooled gradient and the argmax codes -- what stem_bn_bwd_apply_kernel would have
// written (3.3 GB at 2048 images) and this kernel read back.  A thread owns the 2x2 pixels (2a+dy, 2b+dx) of one
// 8-channel group (pool_grad.h): 8 x 16 tile = 4 x 8 such blocks x 8 groups = 256 threads.  The raw loads of the NEXT
// tile stay in registers while the current one is multiplied; the arithmetic happens when they are committed to LDS.
//
// What a tile costs is vector-ALU issue, so the tile loop carries only what forms a value of the result.  Static counts
// (hipcc -O3, gfx950; profiles/stem_wgrad_valu_bench.txt): 559 vector instructions per thread and tile on the path of a
// tile whose outputs all exist, against about 1,000 in the loop of the kernel this replaces (1,795 in that whole
// kernel); 208 VGPRs, two waves per SIMD, no scratch.  Measured at 4096 images: 4.27 -> 3.36 ms per launch, still 1.9x
// the byte floor (1.75 ms for 10.7 GB), outputs equal element for element.  What is left in the loop is the dY
// arithmetic: the max-pool routing of 32 values (72 byte compares + 72 selects + 28 packed adds), their bf16 rounding,
// the ReLU mask (16 packed FMAs, 32 compares, 32 selects), dY = (D + B*y0) + A*dz (32 packed multiplies, 32 packed
// adds) and its packing.  Removed:
//   * the patch goes by LDS-DMA into two buffers (no fetch_patch / commit_patch: their division by 40, bounds tests,
//     64-bit addresses and 8 staging registers);
//   * tile coordinates are scalar and advance by carries (no division per tile), address bases are scalar, per-thread
//     offsets are 32-bit and computed once;
//   * a tile whose outputs all exist takes a path without clamps and `live` / `in` selects;
//   * the MFMA fragment addresses are two per-tile bases + immediates.
// The per-thread argmax / gradient loads (each pooling window is fetched by up to four threads) stay as they are.
// Measured and rejected earlier: a producer / consumer split (4 waves load + form dY with two tiles of operands in
// flight, 4 waves multiply: 2.7 ms vs 2.15 ms at 2048 images -- one VALU wave per SIMD issues worse than two) and
// wave-uniform base + per-thread constant offsets with an incremental tile cursor (2.11 ms vs 2.15 ms: the address
// arithmetic was not the bulk of it).  That variant touched the addressing alone, and with the block-index test still
// inside the divergent prologue branch its cursor and bases were vector values all the same (see the end of the
// kernel); the present form also drops the patch staging, the clamps and the validity selects.
struct StemBnArgs {
  StemArgs s;                       // s.dy unused
  const unsigned short* y0;         // [N,Hout,Wout,64] stem convolution output
  const unsigned char* argmax;      // [N,Hp,Wp,64]
  const unsigned short* gp;         // [N,Hp,Wp,64] gradient of the pooled activation
  const float* mean; const float* rstd; const float* gamma; const float* scale; const float* shift;
  const double* dgamma; const double* dbeta;
  float* dgamma_f32; float* dbeta_f32;
  int Hp, Wp;
};

// The input patch by LDS-DMA: origin (2*oy0 - 3, 2*ox0 - 4) -- one pixel left of the patch the register path stages, so
// that with an even Win every 16-byte piece (two pixels) is aligned and lies wholly inside or wholly outside the image.
// A patch row is 20 pieces, the patch 420, lane-linear in LDS: seven wave-instructions of 64 pieces (the last one
// carries 28 padding pieces into the buffer's tail), two per wave.  Out-of-image pieces read the zero page.
constexpr int PPIECES = PR * (PROW / 16);
constexpr int PDMA = (PPIECES + 63) / 64;
constexpr int PBUF = PDMA * 1024;
__device__ __attribute__((aligned(256))) unsigned char g_stem_zero_page[256];


// max-pool routing of channels 4*HALF .. +3: windows_to_grad4 (pool_grad.h) without its `live` tests -- the caller has
// set the codes of a missing window to 0xFF, which selects nothing.  Same contributions, same order (window rows, then
// columns), same bf16 rounding
template <int HALF>
__device__ __forceinline__ void stem_route4_interior(const isic_pool::Windows& w, float (&out)[4][4]) {
  float acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[p][j] = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jw = 0; jw < 2; ++jw) {
      const unsigned lo = w.g[i * 2 + jw][2 * HALF], hi = w.g[i * 2 + jw][2 * HALF + 1];
      const float g[4] = {__uint_as_float(lo << 16), __uint_as_float(lo & 0xFFFF0000u), __uint_as_float(hi << 16),
                          __uint_as_float(hi & 0xFFFF0000u)};
      const unsigned am = w.am[i * 2 + jw][HALF];
#pragma unroll
      for (int dy = i; dy < 2; ++dy)
#pragma unroll
        for (int dx = jw; dx < 2; ++dx) {
          const unsigned code = (unsigned)((dy + 1 - 2 * i) * 3 + (dx + 1 - 2 * jw));
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (((am >> (j * 8)) & 0xFFu) == code) acc[dy * 2 + dx][j] += g[j];
        }
    }
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[p][j] = bf16_bits_to_f32(f32_to_bf16_bits(acc[p][j]));
}

// DMA = true needs an even Win and a 16-byte aligned input; DMA = false stages the patch through registers
// (fetch_patch / commit_patch) and serves every other shape.
template <bool DMA>
__global__ __launch_bounds__(256, 2) void conv_stem_wgrad_bn_kernel(StemBnArgs b) {
  const StemArgs& a = b.s;
  constexpr int PSZ = DMA ? 2 * PBUF : PR * PROW;        // DMA: two patch buffers, tile t+1 lands while tile t is multiplied
  constexpr int PSH = DMA ? 8 : 0;                       // DMA: the patch starts one pixel further left
  __shared__ __attribute__((aligned(16))) unsigned char smem[PSZ + TH * TW * YROW];
  __shared__ __attribute__((aligned(16))) float cst[5][64];     // A, B, D of dY = A*dz + B*y0 + D; sc, sh of the ReLU mask
  unsigned char* Ys = smem + PSZ;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fg = lane >> 4, fi = lane & 15, fq = fi >> 2, fp = fi & 3;
  typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
  // this lane's part of the MFMA fragment addresses (see the tile loop)
  const unsigned frag_y = (unsigned)((8 * fg + fq) * YROW + 8 * fp);
  const unsigned frag_p = (unsigned)(2 * (fg >> 1) * PROW + (16 * (fg & 1) + 2 * fq + fp) * 8 + PSH);
  const isic_pool::PoolGeom geom{a.Hout, a.Wout, 64, b.Hp, b.Wp};

  const int bid = blockIdx.x;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- tile cursor: tile += gridDim.x as (n, oy0, ox0) += (step_n, step_y, step_x) with carries, in scalar registers
  const int tiles_img = a.tiles_h * a.tiles_w;
  const int step_n = (int)gridDim.x / tiles_img, step_r = (int)gridDim.x - step_n * tiles_img;
  const int step_y = (step_r / a.tiles_w) * TH, step_x = (step_r % a.tiles_w) * TW;
  const int span_y = a.tiles_h * TH, span_x = a.tiles_w * TW;
  auto advance = [&](StemTile& t) {
    t.ox0 += step_x;
    if (t.ox0 >= span_x) { t.ox0 -= span_x; t.oy0 += TH; }
    t.oy0 += step_y;
    if (t.oy0 >= span_y) { t.oy0 -= span_y; t.n += 1; }
    t.n += step_n;
  };
  // a tile whose outputs all exist (block-uniform, the usual case) is formed without clamps and validity selects, from
  // a per-image scalar base and 32-bit per-thread offsets; of its pooling windows only those of the last row / column
  // can be missing: such a window is loaded from its neighbour's address and its argmax codes are overwritten by 0xFF
  const bool fits32 = (int64_t)a.Hout * a.Wout < (1 << 24);             // in-image byte offsets (128 B per pixel) fit 31 bits
  auto interior = [&](const StemTile& t) { return fits32 && t.oy0 + TH <= a.Hout && t.ox0 + TW <= a.Wout; };

  // this thread's 2x2 pixel block inside the tile and its channel group
  const int cg = tid & 7, bl = tid >> 3, al = bl >> 3, bw = bl & 7;
  const unsigned yoff = (unsigned)((2 * al * a.Wout + 2 * bw) * 128 + cg * 16);   // pixel (2al, 2bw) from the tile origin
  const unsigned goff = (unsigned)((al * b.Wp + bw) * 128 + cg * 16);             // window (al, bw) from the tile's first
  u32x2 pre[DMA ? 1 : PATCH_PER_THREAD];
  u32x4 xr[4];
  isic_pool::Windows win;
  auto fetch_dy = [&](const StemTile& t, auto INT) {
    if constexpr (decltype(INT)::value) {
      const unsigned char* yb = reinterpret_cast<const unsigned char*>(b.y0) +
                                (((int64_t)t.n * a.Hout + t.oy0) * a.Wout + t.ox0) * 128;
      const int64_t w0 = ((int64_t)t.n * b.Hp + (t.oy0 >> 1)) * b.Wp + (t.ox0 >> 1);
      const unsigned char* gb = reinterpret_cast<const unsigned char*>(b.gp) + w0 * 128;
      const unsigned char* ab = b.argmax + w0 * 64;
#pragma unroll
      for (int p = 0; p < 4; ++p)
        xr[p] = *reinterpret_cast<const u32x4*>(yb + (size_t)(p >> 1) * a.Wout * 128 + yoff + (p & 1) * 128);
      const unsigned drow = ((t.oy0 >> 1) + al + 1 < b.Hp) ? (unsigned)b.Wp * 128u : 0u;
      const unsigned dcol = ((t.ox0 >> 1) + bw + 1 < b.Wp) ? 128u : 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned o = goff + ((k >> 1) ? drow : 0u) + ((k & 1) ? dcol : 0u);
        win.am[k] = *reinterpret_cast<const u32x2*>(ab + (o >> 1));
        win.g[k] = *reinterpret_cast<const u32x4*>(gb + o);
      }
    } else {
      const int ga = (t.oy0 >> 1) + al, gb = (t.ox0 >> 1) + bw;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int hi = min(2 * ga + (p >> 1), a.Hout - 1), wi = min(2 * gb + (p & 1), a.Wout - 1);
        xr[p] = *reinterpret_cast<const u32x4*>(b.y0 + (((size_t)t.n * a.Hout + hi) * a.Wout + wi) * 64 + cg * 8);
      }
      isic_pool::load_windows(win, b.argmax, b.gp, geom, t.n, min(ga, b.Hp - 1), min(gb, b.Wp - 1), cg);
    }
  };
  // raw loads -> dY values of the 2x2 pixels -> LDS rows [pixel][co]
  auto commit_dy = [&](const StemTile& t, auto INT) {
    constexpr bool I_ = decltype(INT)::value;
    const int ga = (t.oy0 >> 1) + al, gb = (t.ox0 >> 1) + bw;
    const bool inside = I_ || ((t.oy0 + TH <= a.Hout) && (t.ox0 + TW <= a.Wout));
    if constexpr (I_) {
      const bool row1 = ga + 1 < b.Hp, col1 = gb + 1 < b.Wp;
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const bool live = ((k >> 1) == 0 || row1) && ((k & 1) == 0 || col1);
        win.am[k][0] = live ? win.am[k][0] : 0xFFFFFFFFu;
        win.am[k][1] = live ? win.am[k][1] : 0xFFFFFFFFu;
      }
    }
    auto half = [&](auto HC) {
      constexpr int H_ = decltype(HC)::value;
      float g[4][4];
      if constexpr (I_) stem_route4_interior<H_>(win, g);      // (missing windows: codes already 0xFF)
      else isic_pool::windows_to_grad4<H_>(win, geom, ga, gb, g);
      const int c0 = cg * 8 + H_ * 4;
      const f32x4 kA = *reinterpret_cast<const f32x4*>(&cst[0][c0]), kB = *reinterpret_cast<const f32x4*>(&cst[1][c0]);
      const f32x4 kD = *reinterpret_cast<const f32x4*>(&cst[2][c0]), sc = *reinterpret_cast<const f32x4*>(&cst[3][c0]);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(&cst[4][c0]);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int oyl = 2 * al + (p >> 1), oxl = 2 * bw + (p & 1);
        const bool in = inside || ((t.oy0 + oyl < a.Hout) && (t.ox0 + oxl < a.Wout));
        const unsigned lo = xr[p][2 * H_], hi = xr[p][2 * H_ + 1];
        float xv[4];
        isic_unpack_bf16x4(lo, hi, xv);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // the mask and dz are the two-kernel path's (isic_bn_bwd_apply_pooled_bf16); dY is NOT: dx_unfused rounds each
          // product and each sum of (D + B*y0) + A*dz by itself, stem_bn_bwd_apply_kernel makes two fused multiply-adds
          const float dz = isic_bn_bwd::gate<2>(g[p][j], xv[j], 0.f, sc[j], sh[j], 0u, 0);
          o[j] = isic_bn_bwd::dx_unfused(kA[j], kB[j], kD[j], xv[j], dz);
          if (!inside) o[j] = in ? o[j] : 0.f;
        }
        *reinterpret_cast<u32x2*>(Ys + (oyl * TW + oxl) * YROW + cg * 16 + H_ * 8) = isic_pack_bf16x4(o);
      }
    };
    half(std::integral_constant<int, 0>{});
    __builtin_amdgcn_sched_barrier(0);                   // keep the two halves' temporaries from overlapping
    half(std::integral_constant<int, 1>{});
  };

  // ---- patch DMA: this wave's instructions d = wave, wave + 4; piece q = 64 d + lane = patch row q / 20, pixels 2 (q % 20) ..+1
  int ppr[2], ppc[2];
  unsigned poff[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = (wave + 4 * u) * 64 + lane;
    ppr[u] = q < PPIECES ? q / (PROW / 16) : -100000;                    // padding piece: never inside the image
    ppc[u] = 2 * (q % (PROW / 16));
    poff[u] = q < PPIECES ? (unsigned)((ppr[u] * a.Win + ppc[u]) * 8) : 0u;
  }
  const unsigned char* zp = g_stem_zero_page + (lane & 7) * 16;
  auto issue_patch = [&](const StemTile& t, int buf) {
    const int hi0 = 2 * t.oy0 - 3, wi0 = 2 * t.ox0 - 4;
    const unsigned char* org = reinterpret_cast<const unsigned char*>(a.in) +
                               (((int64_t)t.n * a.Hin + hi0) * a.Win + wi0) * 8;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int d = wave + 4 * u;
      if (d < PDMA) {                                                    // wave-uniform
        const bool ok = (unsigned)(hi0 + ppr[u]) < (unsigned)a.Hin && (unsigned)(wi0 + ppc[u]) < (unsigned)a.Win;
        isic_glds16(ok ? org + poff[u] : zp, __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(buf * PBUF + d * 1024)));
      }
    }
  };

  StemTile cur;
  {
    const int t0 = bid;                                   // < total_tiles: the grid is never larger
    const int n = t0 / tiles_img, t2 = t0 - n * tiles_img;
    cur.n = n; cur.oy0 = (t2 / a.tiles_w) * TH; cur.ox0 = (t2 % a.tiles_w) * TW;
  }
  int buf = 0;
  // (after the scalar set-up above: what is first computed inside this divergent branch and used again behind it
  //  comes out of the branch's join as a vector value, tile coordinates and address bases included)
  if (tid < 64) {
    // dY = k1*(dz - k2 - xh*k3), xh = (y0 - mu)*rs  ==  A*dz + B*y0 + D: the three constants of the two-kernel path
    const float inv_rows = isic_bn_bwd::inv_count((int64_t)a.N * a.Hout * a.Wout);
    isic_bn_bwd::constants(b.mean[tid], b.rstd[tid], b.gamma[tid], (float)b.dgamma[tid], (float)b.dbeta[tid], inv_rows,
                           cst[0][tid], cst[1][tid], cst[2][tid]);
    cst[3][tid] = b.scale[tid]; cst[4][tid] = b.shift[tid];
  }
  __syncthreads();                                       // constants visible
  if constexpr (DMA) issue_patch(cur, 0);
  else fetch_patch(pre, a, bid, tid);
  if (interior(cur)) fetch_dy(cur, std::true_type{});
  else fetch_dy(cur, std::false_type{});
  for (int tile = bid; tile < a.total_tiles; tile += gridDim.x) {
    unsigned char* Ps = smem + (DMA ? buf * PBUF : 0);
    lds_barrier();                                       // previous tile's operands fully consumed
    if constexpr (!DMA) commit_patch(Ps, pre, tid);
    if (interior(cur)) commit_dy(cur, std::true_type{});
    else commit_dy(cur, std::false_type{});
    if constexpr (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the patch have landed
    lds_barrier();
    const bool more = tile + (int)gridDim.x < a.total_tiles;
    if constexpr (!DMA) fetch_patch(pre, a, tile + gridDim.x, tid);
    if (more) {                                          // block-uniform
      advance(cur);
      if constexpr (DMA) issue_patch(cur, buf ^ 1);      // the other buffer: last read before the two barriers above
      if (interior(cur)) fetch_dy(cur, std::true_type{});
      else fetch_dy(cur, std::false_type{});
    }
    buf ^= 1;
    // fragment addresses = one per-tile base + compile-time offsets.  Pixel row k1 = 32 ks + 8 fg + fq (k2 = k1 + 4) and
    // n-tile nt = wave + 4 j (kernel row kh = (wave >> 1) + 2 j, half = wave & 1): the patch address
    // (2 (k >> 4) + kh) PROW + (2 (k & 15) + 4 half + fp) 8 splits into the lane's part, the wave's part and
    // (4 ks + 2 j) PROW (+ 64 for k2).  nt >= 14 (j = 3 of waves 2, 3: kh = 7) would address past the taps: those two
    // waves read row kh = 6 instead (result discarded at the end)
    const unsigned char* yb = Ys + frag_y;
    const unsigned char* pb = Ps + frag_p + ((wave >> 1) * PROW + (wave & 1) * 32);
    const unsigned char* pb3 = pb - (wave >= 2 ? PROW : 0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(yb + ks * 32 * YROW + i * 32));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(yb + (ks * 32 + 4) * YROW + i * 32));
        s16x8_t t; t.lo = lo; t.hi = hi;
        af[i] = __builtin_bit_cast(bf16x8, t);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned char* p1 = (j < 3 ? pb : pb3) + (4 * ks + 2 * j) * PROW;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)p1);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(p1 + 64));
        s16x8_t t; t.lo = lo; t.hi = hi;
        bfr[j] = __builtin_bit_cast(bf16x8, t);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nt = wave + 4 * j;
      if (nt >= 14) continue;
      const int kh = nt >> 1, kw = (nt & 1) * 4 + (fi >> 2), c = fi & 3;
      if (kw >= 7 || c >= 3) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = i * 16 + fg * 4 + r;
        // the block's OWN partial (workspace [grid][64*7*7*3]); isic_slab_reduce_launch adds them in a fixed order:
        // deterministic, where fp32 atomics added the blocks in arrival order
        a.dw[(size_t)bid * STEM_DW_ELEMS + ((co * 7 + kh) * 7 + kw) * 3 + c] = acc[i][j][r];
      }
    }
  // the fp32 copies of dgamma / dbeta, by block 0.  At the END: a test of the block index inside the divergent branch
  // at the top lets the compiler merge "block index == 0" with the register at that branch's join, which turns the
  // block index -- and with it every tile coordinate and address base of the loop -- into vector values
  if (bid == 0 && tid < 64 && b.dgamma_f32) isic_bn_bwd::fold(tid, b.dgamma, b.dbeta, b.dgamma_f32, b.dbeta_f32);
}

// fp32 [64][7][7][3] (channels_last memory of the OIHW parameter) -> bf16 [64][7][8][4], zero padded
__global__ void stem_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ ws) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 64 * 7 * 8 * 4) return;
  const int c = idx & 3, kw = (idx >> 2) & 7, kh = (idx >> 5) % 7, co = idx / 224;
  float v = 0.f;
  if (c < 3 && kw < 7) v = w[((co * 7 + kh) * 7 + kw) * 3 + c];
  ws[idx] = f32_to_bf16_bits(v);
}

int stem_args(StemArgs& a, int N, int Hin, int Win, int Hout, int Wout) {
  if (Hout != (Hin + 6 - 7) / 2 + 1 || Wout != (Win + 6 - 7) / 2 + 1) return ISIC_ERR_BAD_ARG;
  a.N = N; a.Hin = Hin; a.Win = Win; a.Hout = Hout; a.Wout = Wout;
  a.tiles_h = ceil_div(Hout, TH); a.tiles_w = ceil_div(Wout, TW);
  const int64_t tt = (int64_t)N * a.tiles_h * a.tiles_w;
  if (tt > 0x7FFFFFFFLL) return ISIC_ERR_UNSUPPORTED;
  a.total_tiles = (int)tt;
  return ISIC_OK;
}

}  // namespace

extern "C" {

int isic_conv_stem_fwd_bf16(const uint16_t* in_nhwc4, const uint16_t* w_stem, uint16_t* out, int N, int Hin, int Win,
                            int Hout, int Wout, void* stream) {
  return isic_conv_stem_fwd_stats_bf16(in_nhwc4, w_stem, out, N, Hin, Win, Hout, Wout, nullptr, nullptr, 0, stream);
}

int isic_conv_stem_fwd_stats_bf16(const uint16_t* in_nhwc4, const uint16_t* w_stem, uint16_t* out, int N, int Hin,
                                  int Win, int Hout, int Wout, double* stat_sum, double* stat_sumsq, int stat_slots,
                                  void* stream) {
  ISIC_CHECK_ARG(in_nhwc4 && w_stem && out && N > 0 && Hin > 0 && Win > 0);
  ISIC_CHECK_ARG((stat_sum == nullptr) == (stat_sumsq == nullptr));
  ISIC_CHECK_ARG(!stat_sum || stat_slots > 0);
  StemArgs a;
  a.stat_sum = stat_sum; a.stat_sumsq = stat_sumsq; a.stat_slots = stat_slots > 0 ? stat_slots : 1;
  a.in = in_nhwc4; a.w = w_stem; a.out = out; a.dy = nullptr; a.dw = nullptr;
  int rc = stem_args(a, N, Hin, Win, Hout, Wout);
  if (rc != ISIC_OK) return rc;
  const int grid = a.total_tiles < STEM_FWD_BLOCKS ? a.total_tiles : STEM_FWD_BLOCKS;
  if (stat_sum) hipLaunchKernelGGL(conv_stem_fwd_kernel<true>, dim3(grid), dim3(256), 0, as_stream(stream), a);
  else hipLaunchKernelGGL(conv_stem_fwd_kernel<false>, dim3(grid), dim3(256), 0, as_stream(stream), a);
  return isic_launch_status();
}

size_t isic_conv_stem_wgrad_workspace_bytes(void) { return (size_t)STEM_WGRAD_BLOCKS * STEM_DW_ELEMS * sizeof(float); }

int isic_conv_stem_wgrad_bf16(const uint16_t* in_nhwc4, const uint16_t* dy, float* dw, int N, int Hin, int Win,
                              int Hout, int Wout, void* workspace, size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(in_nhwc4 && dy && dw && workspace && N > 0 && Hin > 0 && Win > 0);
  if (workspace_bytes < isic_conv_stem_wgrad_workspace_bytes()) return ISIC_ERR_WORKSPACE;
  StemArgs a;
  a.stat_sum = nullptr; a.stat_sumsq = nullptr; a.stat_slots = 1;
  a.in = in_nhwc4; a.w = nullptr; a.out = nullptr; a.dy = dy; a.dw = reinterpret_cast<float*>(workspace);
  int rc = stem_args(a, N, Hin, Win, Hout, Wout);
  if (rc != ISIC_OK) return rc;
  const int grid = a.total_tiles < STEM_WGRAD_BLOCKS ? a.total_tiles : STEM_WGRAD_BLOCKS;
  hipLaunchKernelGGL(conv_stem_wgrad_kernel, dim3(grid), dim3(256), 0, as_stream(stream), a);
  isic_slab_reduce_launch(ISIC_SLAB_XOR16, reinterpret_cast<const float*>(workspace), grid, STEM_DW_ELEMS, dw, 1.f,
                          as_stream(stream));                       // dw += the blocks' partials (slab_sum.inc, order A)
  return isic_launch_status();
}

int isic_conv_stem_wgrad_bn_pooled_bf16(const uint16_t* in_nhwc4, const uint16_t* y0, const uint8_t* argmax,
                                        const uint16_t* dy_pooled, const float* mean, const float* rstd,
                                        const float* gamma, const float* scale, const float* shift, const double* dgamma,
                                        const double* dbeta, float* dw, float* dgamma_f32, float* dbeta_f32, int N,
                                        int Hin, int Win, int Hout, int Wout, int Hp, int Wp, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(in_nhwc4 && y0 && argmax && dy_pooled && mean && rstd && gamma && scale && shift && dgamma && dbeta && dw);
  ISIC_CHECK_ARG(workspace != nullptr);
  if (workspace_bytes < isic_conv_stem_wgrad_workspace_bytes()) return ISIC_ERR_WORKSPACE;
  ISIC_CHECK_ARG(N > 0 && Hin > 0 && Win > 0 && (dgamma_f32 == nullptr) == (dbeta_f32 == nullptr));
  ISIC_CHECK_ARG(Hp == (Hout + 2 - 3) / 2 + 1 && Wp == (Wout + 2 - 3) / 2 + 1);
  StemBnArgs b;
  StemArgs& a = b.s;
  a.stat_sum = nullptr; a.stat_sumsq = nullptr; a.stat_slots = 1;
  a.in = in_nhwc4; a.w = nullptr; a.out = nullptr; a.dy = nullptr; a.dw = reinterpret_cast<float*>(workspace);
  int rc = stem_args(a, N, Hin, Win, Hout, Wout);
  if (rc != ISIC_OK) return rc;
  b.y0 = y0; b.argmax = argmax; b.gp = dy_pooled; b.mean = mean; b.rstd = rstd; b.gamma = gamma; b.scale = scale;
  b.shift = shift; b.dgamma = dgamma; b.dbeta = dbeta; b.dgamma_f32 = dgamma_f32; b.dbeta_f32 = dbeta_f32;
  b.Hp = Hp; b.Wp = Wp;
  const int grid = a.total_tiles < STEM_WGRAD_BLOCKS ? a.total_tiles : STEM_WGRAD_BLOCKS;
  // the patch goes by LDS-DMA where its 16-byte pieces are aligned and never straddle the right border
  if (Win % 2 == 0 && (reinterpret_cast<uintptr_t>(in_nhwc4) & 15) == 0)
    hipLaunchKernelGGL(conv_stem_wgrad_bn_kernel<true>, dim3(grid), dim3(256), 0, as_stream(stream), b);
  else
    hipLaunchKernelGGL(conv_stem_wgrad_bn_kernel<false>, dim3(grid), dim3(256), 0, as_stream(stream), b);
  isic_slab_reduce_launch(ISIC_SLAB_XOR16, reinterpret_cast<const float*>(workspace), grid, STEM_DW_ELEMS, dw, 1.f,
                          as_stream(stream));                       // dw += the blocks' partials (slab_sum.inc, order A)
  return isic_launch_status();
}

int isic_conv_stem_pack_bf16(const float* w_krsc, uint16_t* w_stem, void* stream) {
  ISIC_CHECK_ARG(w_krsc && w_stem);
  hipLaunchKernelGGL(stem_pack_kernel, dim3(ceil_div(64 * 224, 256)), dim3(256), 0, as_stream(stream), w_krsc, w_stem);
  return isic_launch_status();
}

}  // extern "C"
