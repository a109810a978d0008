// Weight gradient of the 64 -> 64 channel 3x3 / stride 1 / pad 1 layers (ResNet-18 layer1) with ALL NINE TAPS PER
// BLOCK and the whole 64 x 9 x 64 gradient resident in registers (gfx950, bf16 MFMA, fp32 accumulate).
//
//   dW[co][kh][kw][ci] = sum over pixels p of  dY[p][co] * X[p + (kh-1, kw-1)][ci]
//
// is a GEMM whose K dimension is the pixel index (1.6 M pixels at N = 512) and whose output is tiny.  The generic
// kernel (conv_wgrad.hip) gives every block one tap and re-reads dY and X from L2 nine times.  Here one persistent
// 768-thread block per CU walks a contiguous range of 4 x 32 pixel tiles; per tile four STAGING WAVES bring dY
// (16 KB) and the (4+2) x (32+2) pixel halo patch of X (26 KB used) into LDS ONCE by LDS-DMA, three stages deep, and
// MFMA wave (c, h) accumulates D[ci in 16c..16c+16][co in 32h..32h+32] for all nine taps: 18 MFMA tiles = 72
// accumulator VGPRs that never leave the register file until the block is done (two MFMA waves per SIMD: one wave
// alone cannot keep the matrix core busy between its own address arithmetic and LDS waits).  Every X fragment (patch row, tap column) is read from LDS once per tile
// and used for up to three tap rows; the operands are read with transposing LDS reads (ds_read_b64_tr_b16), since
// the K axis (pixels) is the row axis of the NHWC images in LDS.
// The partial gradients of the blocks go to the workspace with plain stores and are summed by a second kernel in
// a fixed order: the result does not depend on the scheduling (no atomics).
//
// wgrad_c64_kernel<2> / <3> are the same kernel with the BatchNorm-backward apply pass folded into its staging waves: dY
// does not exist yet, the staging waves form it from the incoming gradient and the convolution output (see BNBWD below).

#include "common.h"
#include "slab_sum.inc"
#include "mfma_tile.h"
#include "pool_grad.h"
#include "bn_bwd_math.inc"

namespace {

constexpr int WT_H = 4, WT_W = 32;                  // pixel tile
constexpr int XP = 48;                              // pitch of the X patch in LDS (pixels; multiple of 16: swizzle key)
constexpr int X_ROWS = WT_H + 2;
constexpr int X_BYTES = X_ROWS * XP * 128;          // 36,864
constexpr int DY_BYTES = WT_H * WT_W * 128;         // 16,384
constexpr int STAGE = X_BYTES + DY_BYTES;           // 53,248
constexpr int NSTAGE = 3;
constexpr int SCRATCH = NSTAGE * STAGE;             // 1 KB landing zone of the padding DMAs
constexpr int LDS_TOTAL = SCRATCH + 1024;           // 160,768 B
constexpr int NDMA = 12;                            // DMA groups (8 pixels) per staging wave and tile: 6 + 4 + 2
constexpr int DW_ELEMS = 64 * 9 * 64;

struct WC64Args {
  const unsigned short* x;
  const unsigned short* dy;
  float* partial;       // [gridDim][64][9][64]
  int N, H, W, tiles_y, tiles_x, total_tiles, tiles_per_block;
};

// BNBWD: dY = kA * dz + (kB * c + kD) per channel, dz = relu_mask ? g : 0: the functions of bn_bwd_math.inc, as in
// isic_bn_bwd_apply*_bf16 (encoder_ops.hip)
struct WC64BnArgs : WC64Args {        // dy = g, the gradient of the BatchNorm(+ReLU) output
  const unsigned short* c;            // the BatchNorm input (this layer's raw convolution output)
  const unsigned char* mask;          // MODE 3: one bit per element
  const float *mean, *rstd, *gamma, *scale, *shift;   // scale, shift: MODE 2 (mask recomputed from c)
  const double *dgamma, *dbeta;       // the reduced sums
  unsigned short* dc;                 // dY is also written out (the data gradient reads it next)
  float *dgamma_f32, *dbeta_f32;
};

__device__ __attribute__((aligned(256))) unsigned char g_wc64_zeros[2048];

// Register loads the compiler must not count: its waits would drain the LDS-DMAs in flight beside them.  The data is
// there after the counted wait of wc64_landed*, which names every destination.
__device__ __forceinline__ u32x4 wc64_load16(const void* gsrc) {
  u32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(gsrc) : "memory");
  return v;
}
__device__ __forceinline__ unsigned wc64_load1(const void* gsrc) {
  unsigned v;
  asm volatile("global_load_ubyte %0, %1, off" : "=v"(v) : "v"(gsrc) : "memory");
  return v;
}
template <int N>
__device__ __forceinline__ void wc64_landed(u32x4 (&g)[4], u32x4 (&c)[4]) {
  asm volatile("s_waitcnt vmcnt(%8)"
               : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]), "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3])
               : "n"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wc64_landed(u32x4 (&g)[4], u32x4 (&c)[4], unsigned (&m)[4]) {
  asm volatile("s_waitcnt vmcnt(%12)"
               : "+v"(g[0]), "+v"(g[1]), "+v"(g[2]), "+v"(g[3]), "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]),
                 "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3])
               : "n"(N) : "memory");
}
template <int V> struct WC64Int { static constexpr int value = V; };
template <int MODE> struct WC64Mode { typedef WC64BnArgs Args; };
template <> struct WC64Mode<0> { typedef WC64Args Args; };

#ifdef WC64_STAMPS   // tests/probes: per tile clock before the wait, after the barrier, after the MFMAs (wave 0, 256 blocks x 64 tiles)
__device__ unsigned long long g_wc64_stamps[256 * 64 * 4];
#define WC64_STAMP(kk, k) do { if (threadIdx.x == 512 && blockIdx.x < 256 && (kk) < 64) g_wc64_stamps[(blockIdx.x * 64 + (kk)) * 4 + (k)] = clock64(); } while (0)
#else
#define WC64_STAMP(kk, k) do { } while (0)
#endif

// MODE 0: dY is read (WC64Args).  MODE 2 / 3: dY is formed by the staging waves (WC64BnArgs), ReLU mask recomputed from
// c * scale + shift / read from the 1-bit mask -- the modes of bn_bwd_apply_kernel.
template <int MODE>
__global__ __launch_bounds__(768) void wgrad_c64_kernel(typename WC64Mode<MODE>::Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave12 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int t_begin = blockIdx.x * a.tiles_per_block;
  const int ntl = min(a.total_tiles - t_begin, a.tiles_per_block);       // >= 1 by construction of the grid

  if (wave12 >= 8) {
    // =================================================================== staging waves (one per SIMD)
    // An LDS-DMA instruction with per-lane addresses holds its wave at issue for the order of 100 cycles: issued by
    // the MFMA waves themselves, the twelve DMAs per SIMD and tile cost a quarter of the tile time.  These four waves
    // do nothing else, so the stall is theirs alone.
    // Wave p stages the 8-column block p of the X patch (6 rows) and of dY (4 rows), and rows 2p, 2p+1 of the X
    // patch's fifth block (columns 32..39; rows 6, 7 do not exist: padding): 12 DMA groups of 8 pixels per tile.
    // Lane -> pixel column offset lane/8, 16-byte slot lane%8.  The 32-byte granule G of the pixel in LDS column px
    // holds channel block G ^ key(px), key = bit1(px) | bit3(px) << 1: conflict-free transposing reads for every
    // tap shift (the 8 pixel rows a half-wave addresses are b..b+3 and b+8..b+11: bits 0, 1, 3 tell them apart).
    const int p = wave12 - 8;
    const int tiles_img = a.tiles_y * a.tiles_x;
    struct Tile { int n, y0, x0; };                    // wave-uniform tile coordinates, advanced incrementally
    auto advance = [&](Tile& tl) {
      tl.x0 += WT_W;
      if (tl.x0 >= a.W) {
        tl.x0 = 0; tl.y0 += WT_H;
        if (tl.y0 >= a.H) { tl.y0 = 0; tl.n += 1; }
      }
    };
    Tile ahead;
    {
      const int n = t_begin / tiles_img, rem = t_begin - n * tiles_img;
      const int ty = rem / a.tiles_x;
      ahead.n = n; ahead.y0 = ty * WT_H; ahead.x0 = (rem - ty * a.tiles_x) * WT_W;
    }
    const int r8 = lane >> 3, slot = lane & 7;
    const unsigned lane_e = (unsigned)(r8 * 128 + ((((slot >> 1) ^ ((r8 >> 1) & 1)) << 5) | ((slot & 1) << 4)));   // even blocks
    const unsigned lane_p = lane_e ^ (unsigned)((p & 1) << 6);                                                      // block p
    const long long W128 = (long long)a.W * 128;
    const unsigned long long zeros = (unsigned long long)g_wc64_zeros;
    auto issue_tile = [&](const Tile& tl, int stage, bool live) {
      const long long org = ((long long)tl.n * a.H + tl.y0) * a.W + tl.x0;               // pixel index of the tile origin
      const unsigned long long xrow = (unsigned long long)a.x + (unsigned long long)((org - a.W - 1 + 8 * p) * 128);   // patch (0, 8p)
      const unsigned long long yrow = (unsigned long long)a.dy + (unsigned long long)((org + 8 * p) * 128);            // tile (0, 8p)
      const unsigned long long erow = (unsigned long long)a.x + (unsigned long long)((org + (long long)(2 * p - 1) * a.W + 31) * 128);   // patch (2p, 32)
      const bool okx = (unsigned)(tl.x0 - 1 + 8 * p + r8) < (unsigned)a.W;
      const bool oky = (unsigned)(tl.x0 + 8 * p + r8) < (unsigned)a.W;
      const bool oke = (unsigned)(tl.x0 + 31 + r8) < (unsigned)a.W;
      const unsigned sbase = lds0 + (unsigned)stage * STAGE;
#pragma unroll
      for (int j = 0; j < NDMA; ++j) {
        unsigned long long rowaddr;
        bool okc, row_ok, real = live;
        unsigned lanev, dst;
        if (j < 6) {                                   // X patch row j, block p
          rowaddr = xrow + (unsigned long long)(j * W128);
          row_ok = (unsigned)(tl.y0 - 1 + j) < (unsigned)a.H; okc = okx; lanev = lane_p;
          dst = (unsigned)((j * XP + 8 * p) * 128);
        } else if (j < 10) {                           // dY row j - 6, block p
          if constexpr (MODE != 0) continue;           // formed in registers instead: commit_dy below
          rowaddr = yrow + (unsigned long long)((j - 6) * W128);
          row_ok = (unsigned)(tl.y0 + j - 6) < (unsigned)a.H; okc = oky; lanev = lane_p;
          dst = (unsigned)(X_BYTES + ((j - 6) * 4 + p) * 1024);
        } else {                                       // X patch row 2p + (j - 10), block 4
          const int pr = 2 * p + (j - 10);
          rowaddr = erow + (unsigned long long)((j - 10) * W128);
          row_ok = (unsigned)(tl.y0 - 1 + pr) < (unsigned)a.H; okc = oke; lanev = lane_e;
          real = real && pr < X_ROWS;
          dst = (unsigned)((pr * XP + 32) * 128);
        }
        const bool ok = okc && row_ok && real;
        // per-lane select of two wave-uniform addresses, half by half (out-of-image lanes read a zero page)
        const unsigned lo = ok ? (unsigned)rowaddr : (unsigned)zeros, hi = ok ? (unsigned)(rowaddr >> 32) : (unsigned)(zeros >> 32);
        const unsigned long long src = (((unsigned long long)hi << 32) | lo) + lanev;
        isic_glds16(reinterpret_cast<const void*>(src), real ? sbase + dst : lds0 + SCRATCH);   // padding: zeros -> scratch
      }
    };
    if constexpr (MODE != 0) {
      // ------------------------------------------------------------- BNBWD: the four dY groups go through registers
      // Each lane loads the 16 bytes of g and c (and its mask byte) the DMA would have copied, forms its 8 values of dY,
      // writes them to the LDS slot the DMA filled and to global memory.  The lane's 8 channels never change.
      // Order on the wave's memory queue (loads, stores and DMAs retire in issue order):
      //   prologue  D(0) L(0) D(1) L(1) | wait L(0), commit 0 -> S(0)
      //   step kk   barrier | D(kk+2) L(kk+2) | wait L(kk+1), commit kk+1 -> S(kk+1)
      // D = the 8 X-patch DMAs, L = the NLD register loads, S = up to 4 dY stores.  When step kk waits, L(kk+1) is
      // followed by S(kk), D(kk+2), L(kk+2): "at most 8 + NLD outstanding" retires L(kk+1) whether or not S(kk) was
      // issued (a wave whose lanes are all outside the image skips it), and with it the older D(kk+1).  Tile kk+1 is
      // then complete in LDS once its ds_writes are (lgkmcnt(0) before the barrier).  L(kk+2) stays in flight while
      // tile kk+1 is committed; its registers are the set tile kk used.
      constexpr int NLD = MODE == 3 ? 12 : 8;
      const int cg = (int)((lane_p & 127u) >> 4);
      float kA[8], kB[8], kD[8], sc[8], sh[8];
      {
        const float inv_rows = isic_bn_bwd::inv_count((int64_t)a.N * a.H * a.W);
        if (blockIdx.x == 0 && p == 0 && a.dgamma_f32) isic_bn_bwd::fold(lane, a.dgamma, a.dbeta, a.dgamma_f32, a.dbeta_f32);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = cg * 8 + j;
          isic_bn_bwd::constants(a.mean[c], a.rstd[c], a.gamma[c], (float)a.dgamma[c], (float)a.dbeta[c], inv_rows, kA[j],
                                 kB[j], kD[j]);
          sc[j] = MODE == 2 ? a.scale[c] : 0.f; sh[j] = MODE == 2 ? a.shift[c] : 0.f;
        }
        // the constants are in registers before the first DMA: the compiler's own wait for their loads (it counts only
        // those) would otherwise fall into the pipeline and drain it
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(kA[j]), "+v"(kB[j]), "+v"(kD[j]), "+v"(sc[j]), "+v"(sh[j]));
      }
      u32x4 rg[2][4], rc[2][4];
      unsigned rm[2][4];
      // byte offset of the lane's 16 bytes of row j of the tile (the source the DMA used), validity of the pixel
      auto dy_off = [&](const Tile& tl, int j, bool& ok) -> long long {
        ok = (unsigned)(tl.x0 + 8 * p + r8) < (unsigned)a.W && (unsigned)(tl.y0 + j) < (unsigned)a.H;
        return ((((long long)tl.n * a.H + tl.y0 + j) * a.W + tl.x0 + 8 * p) << 7) + (long long)lane_p;
      };
      auto load_dy = [&](const Tile& tl, bool live, auto SET) {
        constexpr int S = decltype(SET)::value;
#pragma unroll
        for (int j = 0; j < WT_H; ++j) {
          bool ok;
          const long long off = dy_off(tl, j, ok);
          ok = ok && live;                             // out-of-image lanes read the zero page: the count stays fixed
          const unsigned char* zp = g_wc64_zeros + lane_p;
          rg[S][j] = wc64_load16(ok ? reinterpret_cast<const unsigned char*>(a.dy) + off : zp);
          rc[S][j] = wc64_load16(ok ? reinterpret_cast<const unsigned char*>(a.c) + off : zp);
          if constexpr (MODE == 3) rm[S][j] = wc64_load1(ok ? a.mask + (off >> 4) : zp);
        }
      };
      auto commit_dy = [&](const Tile& tl, int stage, auto SET) {
        constexpr int S = decltype(SET)::value;
        if constexpr (MODE == 3) wc64_landed<8 + NLD>(rg[S], rc[S], rm[S]);
        else wc64_landed<8 + NLD>(rg[S], rc[S]);
        const unsigned sdy = lds0 + (unsigned)stage * STAGE + (unsigned)(X_BYTES + p * 1024 + lane * 16);
#pragma unroll
        for (int j = 0; j < WT_H; ++j) {
          bool ok;
          const long long off = dy_off(tl, j, ok);
          float g[8], xv[8], o[8];
          isic_pool::unpack8(rg[S][j], g);
          isic_pool::unpack8(rc[S][j], xv);
          const unsigned m = MODE == 3 ? rm[S][j] : 0u;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float dz = isic_bn_bwd::gate<MODE>(g[e], xv[e], 0.f, sc[e], sh[e], m, e);
            o[e] = isic_bn_bwd::dx(kA[e], kB[e], kD[e], xv[e], dz);
          }
          u32x4 v = isic_pool::pack8(o);
          if (!ok) v = (u32x4){0u, 0u, 0u, 0u};       // padding pixels are zeros in LDS, as the DMA left them
          *(__attribute__((address_space(3))) u32x4*)(size_t)(sdy + (unsigned)(j * 4 * 1024)) = v;
          if (ok) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(reinterpret_cast<unsigned char*>(a.dc) + off));
        }
      };
      Tile next = ahead;                               // the tile committed next
      issue_tile(ahead, 0, true);
      load_dy(ahead, true, WC64Int<0>());
      advance(ahead);
      issue_tile(ahead, 1, ntl > 1);
      load_dy(ahead, ntl > 1, WC64Int<1>());
      advance(ahead);
      commit_dy(next, 0, WC64Int<0>());
      advance(next);
      auto step = [&](int kk, auto SET) {             // SET: register set of tile kk (free), the other holds tile kk+1
        constexpr int S = decltype(SET)::value;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's part of tile kk is in LDS
        __builtin_amdgcn_s_barrier();                 // the MFMA waves are done with stage (kk+2)%3 = (kk-1)%3
        issue_tile(ahead, (kk + 2) % NSTAGE, kk + 2 < ntl);
        load_dy(ahead, kk + 2 < ntl, WC64Int<S>());
        advance(ahead);
        if (kk + 1 < ntl) {
          commit_dy(next, (kk + 1) % NSTAGE, WC64Int<S ^ 1>());
          advance(next);
        }
      };
      for (int kk = 0; kk < ntl; kk += 2) {
        step(kk, WC64Int<0>());
        if (kk + 1 >= ntl) break;
        step(kk + 1, WC64Int<1>());
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // nothing of this wave is in flight when it ends
      return;
    }
    issue_tile(ahead, 0, true);
    advance(ahead);
    issue_tile(ahead, 1, ntl > 1);
    advance(ahead);
    for (int kk = 0; kk < ntl; ++kk) {
      WC64_STAMP(kk, 0);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");   // tile kk landed: only tile kk+1's groups in flight
      WC64_STAMP(kk, 3);
      __builtin_amdgcn_s_barrier();                   // the MFMA waves are done with stage (kk+2)%3 = (kk-1)%3
      WC64_STAMP(kk, 1);
      issue_tile(ahead, (kk + 2) % NSTAGE, kk + 2 < ntl);
      advance(ahead);
      WC64_STAMP(kk, 2);
    }
    return;
  }

  // ======================================================================= MFMA waves
  const int wave = wave12 & 3, half = wave12 >> 2;     // ci block / co half; waves (c, 0) and (c, 1) share a SIMD
  const int fg = lane >> 4, fi = lane & 15, fq = fi >> 2, fp = fi & 3;
  // ---- fragment addresses (bytes inside a stage).  A transposing read: lane (fg, fq, fp) addresses pixel row
  //      8fg + fq (+4 for the second half), 8 bytes at channel 4fp of a 16-channel block; lane fi then holds channel fi
  //      of pixels 8fg .. 8fg+3 (+4): the 8 consecutive K values of the 16x16x32 MFMA operands.
  //      X (ci block c), tap column kw: patch pixel column 8fg + fq + kw (+4)
  unsigned xaddr[3][2];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int px = 8 * fg + fq + kw + 4 * h;
      const int key = ((px >> 1) & 1) | (((px >> 3) & 1) << 1);
      xaddr[kw][h] = (unsigned)(px * 128 + ((wave ^ key) << 5) + fp * 8);
    }
  //      dY (co block 2h + c2): tile column 8fg + fq (+4): the key is the same for both halves
  unsigned yaddr[2];
  {
    const int key = ((fq >> 1) & 1) | ((fg & 1) << 1);
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) yaddr[c2] = (unsigned)(X_BYTES + (8 * fg + fq) * 128 + (((2 * half + c2) ^ key) << 5) + fp * 8);
  }

  f32x4 acc[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < 2; ++c) acc[t][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int kk = 0; kk < ntl; ++kk) {
    __builtin_amdgcn_s_barrier();              // the staging waves saw tile kk land
    // LDS byte addresses of this tile's fragments
    const unsigned st = lds0 + (unsigned)(kk % NSTAGE) * STAGE;
    unsigned xb[3][2], yb[2];
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) { xb[kw][0] = st + xaddr[kw][0]; xb[kw][1] = st + xaddr[kw][1]; }
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) yb[c2] = st + yaddr[c2];
    auto read_frag = [&](unsigned base_lo, unsigned base_hi, int off) -> bf16x8 {
      s16x8_t t;
      t.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)(base_lo + (unsigned)off));
      t.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)(base_hi + (unsigned)off));
      return __builtin_bit_cast(bf16x8, t);
    };
    bf16x8 yf[4][2];                            // dY fragments of the four 32-pixel rows (k-steps) x this wave's two co blocks
    bf16x8 xf[X_ROWS][3];                       // X fragments of patch row pr, tap column kw
    auto read_row = [&](int pr) {
      if (pr < WT_H) {
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) yf[pr][c2] = read_frag(yb[c2], yb[c2] + 4 * 128, pr * 32 * 128);
      }
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) xf[pr][kw] = read_frag(xb[kw][0], xb[kw][1], pr * XP * 128);
    };
    read_row(0);
#pragma unroll
    for (int pr = 0; pr < X_ROWS; ++pr) {       // patch row pr serves k-step s = pr - kh of tap row kh
      if (pr + 1 < X_ROWS) read_row(pr + 1);    // one row ahead of the MFMAs
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int s = pr - kh;
        if (s < 0 || s >= WT_H) continue;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
          for (int c2 = 0; c2 < 2; ++c2)
            acc[kh * 3 + kw][c2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[pr][kw], yf[s][c2], acc[kh * 3 + kw][c2], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);        // keeps the prefetch distance: reads of row pr+1 stay above the MFMAs of row pr
    }
  }

  // ---- this block's partial gradient: lane (fg, fi) holds D[ci = 16c + 4fg + r][co = 32h + 16 c2 + fi]
  float* part = a.partial + (size_t)blockIdx.x * DW_ELEMS;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
      *reinterpret_cast<f32x4*>(part + ((size_t)(half * 32 + c2 * 16 + fi) * 9 + t) * 64 + wave * 16 + fg * 4) = acc[t][c2];
}

int wc64_blocks(int N, int H, int W, int* tiles_per_block) {
  const int cus = isic_cu_count();
  const int64_t total = (int64_t)N * ceil_div(H, WT_H) * ceil_div(W, WT_W);
  const int tpb = (int)ceil_div64(total, cus);
  if (tiles_per_block) *tiles_per_block = tpb;
  return (int)ceil_div64(total, tpb);
}

}  // namespace

// bytes of workspace the 64 -> 64 kernel needs for N images of H x W (0: shape not handled)
size_t isic_wgrad_c64_workspace_bytes(int N, int H, int W) {
  if ((int64_t)N * ceil_div(H, WT_H) * ceil_div(W, WT_W) > 0x7FFFFFFFLL) return 0;
  return (size_t)wc64_blocks(N, H, W, nullptr) * DW_ELEMS * sizeof(float);
}

// called by isic_conv2d_wgrad_bf16 for Cin = Cout = 64, 3x3, stride 1, pad 1
int isic_wgrad_c64_launch(const uint16_t* x, const uint16_t* dy, float* dw, int N, int H, int W, void* workspace,
                          hipStream_t stream) {
  WC64Args a;
  a.x = x; a.dy = dy; a.partial = reinterpret_cast<float*>(workspace);
  a.N = N; a.H = H; a.W = W;
  a.tiles_y = ceil_div(H, WT_H); a.tiles_x = ceil_div(W, WT_W);
  a.total_tiles = N * a.tiles_y * a.tiles_x;
  const int grid = wc64_blocks(N, H, W, &a.tiles_per_block);
  const int rc = isic_launch_lds<wgrad_c64_kernel<0>, LDS_TOTAL>(dim3(grid), dim3(768), LDS_TOTAL, stream, a);
  if (rc != ISIC_OK) return rc;
  isic_slab_reduce_launch(ISIC_SLAB_LDS16_V2, a.partial, grid, DW_ELEMS, dw, 1.f, stream);   // dw += (slab_sum.inc, order B)
  return isic_launch_status();
}

// called by isic_conv2d_wgrad_bnbwd_bf16: the same launch with dY = BatchNorm backward of (g, c) formed on the way
// (relu_mask given: its bits are the ReLU mask; otherwise it is recomputed from c * scale + shift); dY is also left in dc
int isic_wgrad_c64_bnbwd_launch(const uint16_t* x, const uint16_t* g, const uint16_t* c, const uint8_t* relu_mask,
                                const float* mean, const float* rstd, const float* gamma, const double* dgamma,
                                const double* dbeta, const float* scale, const float* shift, uint16_t* dc, float* dw,
                                float* dgamma_f32, float* dbeta_f32, int N, int H, int W, void* workspace,
                                hipStream_t stream) {
  WC64BnArgs a;
  a.x = x; a.dy = g; a.partial = reinterpret_cast<float*>(workspace);
  a.N = N; a.H = H; a.W = W;
  a.tiles_y = ceil_div(H, WT_H); a.tiles_x = ceil_div(W, WT_W);
  a.total_tiles = N * a.tiles_y * a.tiles_x;
  a.c = c; a.mask = relu_mask; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.scale = scale; a.shift = shift;
  a.dgamma = dgamma; a.dbeta = dbeta; a.dc = dc; a.dgamma_f32 = dgamma_f32; a.dbeta_f32 = dbeta_f32;
  const int grid = wc64_blocks(N, H, W, &a.tiles_per_block);
  const int rc = relu_mask ? isic_launch_lds<wgrad_c64_kernel<3>, LDS_TOTAL>(dim3(grid), dim3(768), LDS_TOTAL, stream, a)
                           : isic_launch_lds<wgrad_c64_kernel<2>, LDS_TOTAL>(dim3(grid), dim3(768), LDS_TOTAL, stream, a);
  if (rc != ISIC_OK) return rc;
  isic_slab_reduce_launch(ISIC_SLAB_LDS16_V2, a.partial, grid, DW_ELEMS, dw, 1.f, stream);   // dw += (slab_sum.inc, order B)
  return isic_launch_status();
}
