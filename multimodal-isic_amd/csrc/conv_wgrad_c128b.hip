// Weight gradient of the 3x3 / stride 1 / pad 1 layers with Cin % 128 == 0 and Cout % 64 == 0 (ResNet-18 layer2..4), all
// nine taps per block, SIXTY-FOUR output channels per block (round 4; it replaced a 32-output-channel all-taps kernel,
// DESIGN.md):
//
//   dW[co][kh][kw][ci] = sum over pixels p of  dY[p][co] * X[p + (kh-1, kw-1)][ci]
//
// What the 32-channel kernel waits for (round 4, compiled-out parts at 2048 images of 28 x 28 x 128, ms per launch): whole
// kernel 0.587 -- without MFMAs 0.587 -- without fragment reads 0.594 -- without LDS-DMA 0.322 -- DMA only 0.539.  It is the
// staging stream and nothing else: 63.5 KB per 4 x 32-pixel tile and block, 3.6 GB per launch at 6.7 TB/s, because the
// 55 KB halo patch of X is fetched again by every 32-output-channel block of a pixel range (Cout / 32 = 4 / 8 / 16 times).
// Putting those blocks on one XCD so that they share its L2 changed nothing (0.594 / 0.609 / 0.543 against 0.587 / 0.629 /
// 0.562 ms for 128 / 256 / 512 channels).  So the block is made to USE a staged patch twice as often instead:
//
//   * block = (128 input channels, 64 output channels, pixel range): 9 x 128 x 64 fp32 = 144 accumulator VGPRs per wave at
//     eight waves -- the whole register file of the CU (512 threads x 256), so there are no staging waves: every wave
//     multiplies AND issues nine of the tile's LDS-DMA groups between its MFMA groups.  The slot decides the kind: slots
//     j = 0..6 bring X group wave + 8 j (54 real, two padding DMAs into a sink), slots 7, 8 dY group wave + 8 (j - 7) --
//     no branch on the kind in the unrolled loop, and nine DMAs per wave and tile, which is all the tile top's vmcnt(0)
//     relies on.  An address is (valid ? operand + wave-uniform tile part : zero page) + lane part: the lane part (pixel
//     in group x pixel pitch + swizzled slot; per slot for packed images) is formed ONCE before the tile loop, the tile
//     part is scalar arithmetic, validity is a wave-uniform row test and one column compare (packed: one bit of a lane
//     mask, with a second mask for the batch's last, partly empty pack).  No vector multiply or division is left in the
//     loop.  wgrad_dma_addr.inc holds this arithmetic for device and host, next to the per-DMA form it replaced;
//     tests/wgrad_dma_addr_check.cpp compares the two on the host ("Weight-gradient DMA addresses");
//   * two instances: <false> for W >= 16, <true> for packed images, so each carries only the lane registers it needs;
//   * per tile 55 KB of X + 16 KB of dY for 144 MFMAs per wave instead of 63.5 KB for 72: 1.8x fewer staged bytes per MAC;
//   * LDS images as before -- X: 256-byte pixel rows, 32-byte granules XOR-swizzled by (P & 3) | ((row + (col >> 3)) & 1) << 2;
//     dY: now 128-byte pixel rows, granule G of tile pixel P holds channel block G ^ (((P >> 1) & 1) | ((P >> 3) & 1) << 1):
//     the eight pixels b..b+3, b+8..b+11 a half-wave's transposing read touches land in eight different 32-byte bank groups;
//   * two stages of 77,824 B; one barrier per tile; per-block partials + a fixed-order reduction: deterministic, no atomics;
//   * small images (W <= 15 / W <= 7) packed two / four to a 32-column tile row, at least one empty column between them.
#include "common.h"
#include "slab_sum.inc"
#include "mfma_tile.h"
#include "wgrad_dma_addr.inc"

namespace {

using namespace wga::c128;                          // tile, LDS image and DMA-slot constants: wgrad_dma_addr.inc
constexpr int LDS_ALL = SINK + 1024;                // 156,672 B: two stages of 77,824 B + the sink of padding / dead DMAs
constexpr int SLICE_ELEMS = 64 * 9 * 128;           // one block's partial gradient
static_assert(XB == 61440 && YB == 16384 && STG == 77824 && 8 * XSLOTS >= XGROUPS && 8 * (NDMA - XSLOTS) == YGROUPS, "");

struct WC128BArgs {
  const unsigned short* x;      // [N][H][W][Cx]
  const unsigned short* dy;     // [N][H][W][Cy]
  float* partial;               // [pairs][blocks_per_pair][64][9][128], pair = ci_slice * (Cy / 64) + co_slice
  int N, H, W, tiles_y, tiles_x, total_tiles, tiles_per_block, blocks_per_pair;
  int Cx, Cy, co_slices;
  int pack, slot_shift, Wv;
};

__device__ __attribute__((aligned(256))) unsigned char g_wc128b_zeros[2048];

// PACKED: two / four small images per tile row (per-slot lane offsets and a validity mask instead of column compares)
template <bool PACKED>
__global__ __launch_bounds__(512) void wgrad_c128b_kernel(WC128BArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pair = blockIdx.x / a.blocks_per_pair, bs = blockIdx.x - pair * a.blocks_per_pair;
  const int ci_slice = pair / a.co_slices, slice = pair - ci_slice * a.co_slices;      // slice: 64 output channels
  const int t_begin = bs * a.tiles_per_block;
  const int ntl = min(a.total_tiles - t_begin, a.tiles_per_block);       // >= 1 by construction of the grid

  // ---------------------------------------------------------------- staging (every wave: nine slots, wgrad_dma_addr.inc)
  const int tiles_img = a.tiles_y * a.tiles_x;
  wga::Tile ahead;
  {
    const int n = t_begin / tiles_img, rem = t_begin - n * tiles_img;
    const int ty = rem / a.tiles_x;
    ahead.n = n; ahead.y0 = ty * T_H; ahead.x0 = (rem - ty * a.tiles_x) * T_W;
  }
  // the lane parts of the addresses once; the tile origin and (packed) the validity mask of the tile ahead once per tile
  const Geom geo = {a.N, a.H, a.W, a.Cx, a.Cy, a.pack, a.slot_shift};
  const Lane<PACKED> ln = lane_init<PACKED>(geo, wave, lane);
  const unsigned long long zeros = (unsigned long long)g_wc128b_zeros;
  const unsigned long long xbase = (unsigned long long)a.x + (unsigned long long)ci_slice * 256;
  const unsigned long long ybase = (unsigned long long)a.dy + (unsigned long long)slice * 128;
  wga::TileOrg org = tile_org(geo, ahead);
  unsigned vmask = tile_mask<PACKED>(geo, ln, ahead);
  // slot j of tile `ahead` into stage `stage`: j = 0..6 X group wave + 8 j (two of the 56 are padding), j = 7, 8 dY group
  // wave + 8 (j - 7); a dead prefetch (!live) and the padding read the zero page into the sink behind the stages
  auto dma_one = [&](int j, int stage, bool live) {
    const wga::Dma r = dma<PACKED>(geo, ln, org, vmask, ahead, wave, j, stage, live);
    const unsigned long long base = r.ok ? (r.op ? ybase : xbase) + (unsigned long long)r.soff : zeros;
    isic_glds16(reinterpret_cast<const void*>(base + r.loff), lds0 + r.dst);
  };
  auto next_tile = [&] {
    ahead.x0 += T_W;
    if (ahead.x0 >= a.Wv) {
      ahead.x0 = 0; ahead.y0 += T_H;
      if (ahead.y0 >= a.H) { ahead.y0 = 0; ahead.n += 1; }
    }
    org = tile_org(geo, ahead);
    vmask = tile_mask<PACKED>(geo, ln, ahead);
  };

  // ---------------------------------------------------------------- fragments: wave c = input channels 16c .. 16c+16
  const int fg = lane >> 4, fi = lane & 15, fq = fi >> 2, fp = fi & 3;
  unsigned xaddr[3][2][2];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int par = 0; par < 2; ++par) {
        const int px = 8 * fg + fq + kw + 4 * h;
        const int key = (px & 3) | (((par + (px >> 3)) & 1) << 2);
        xaddr[kw][h][par] = (unsigned)(px * 256 + ((wave ^ key) << 5) + fp * 8);
      }
  // dY, 16-channel block c2 of the 64: tile pixel 32 s + 8 fg + fq (+ 4): key = ((fq >> 1) & 1) | (fg & 1) << 1
  unsigned yaddr[4];
  {
    const int key = ((fq >> 1) & 1) | ((fg & 1) << 1);
#pragma unroll
    for (int c2 = 0; c2 < 4; ++c2) yaddr[c2] = (unsigned)(XB + (8 * fg + fq) * 128 + ((c2 ^ key) << 5) + fp * 8);
  }

  f32x4 acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int j = 0; j < NDMA; ++j) dma_one(j, 0, true);
  next_tile();

  for (int kk = 0; kk < ntl; ++kk) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // tile kk landed (this wave's groups)
    __builtin_amdgcn_s_barrier();                       // ... every group; everyone is done with stage (kk + 1) & 1
    const unsigned st = lds0 + (unsigned)(kk & 1) * STG;
    const bool more = kk + 1 < ntl;
    const int nstage = (kk + 1) & 1;
    auto read_frag = [&](unsigned base_lo, unsigned base_hi, int off) -> bf16x8 {
      s16x8_t t;
      t.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)(base_lo + (unsigned)off));
      t.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(size_t)(base_hi + (unsigned)off));
      return __builtin_bit_cast(bf16x8, t);
    };
    bf16x8 xf[XROWS][3];                        // X fragments of patch row pr, tap column kw (three rows live at a time)
    bf16x8 yf[4];                               // dY fragments of k-step s (one 32-pixel tile row), four co blocks
    auto read_xrow = [&](int pr) {
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
        xf[pr][kw] = read_frag(st + xaddr[kw][0][pr & 1], st + xaddr[kw][1][pr & 1], pr * XPITCH * 256);
    };
    read_xrow(0);
    read_xrow(1);
#pragma unroll
    for (int s = 0; s < T_H; ++s) {             // k-step s = tile row s of dY against patch rows s, s+1, s+2 (tap rows 0, 1, 2)
#pragma unroll
      for (int c2 = 0; c2 < 4; ++c2) yf[c2] = read_frag(st + yaddr[c2], st + yaddr[c2] + 4 * 128, s * 32 * 128);
      read_xrow(s + 2);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        // the tile's nine DMA groups of the NEXT tile go out between the MFMA groups: 12 slots per tile, 9 used
        const int slot = s * 3 + kh;
        // (two per group in groups 0-4, or all nine in front of the first group: 0 .. +3 % slower -- when they go out is not it)
        if (slot < NDMA) dma_one(slot, nstage, more);
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
          for (int c2 = 0; c2 < 4; ++c2)
            acc[kh * 3 + kw][c2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[s + kh][kw], yf[c2], acc[kh * 3 + kw][c2], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);      // a DMA's address arithmetic and the fragment reads stay in their own slot
      }
    }
    next_tile();
  }

  // this block's partial: lane (fg, fi) holds D[ci = 16c + 4fg + r][co = 64 slice + 16 c2 + fi]
  float* part = a.partial + (size_t)blockIdx.x * SLICE_ELEMS;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c2 = 0; c2 < 4; ++c2)
      *reinterpret_cast<f32x4*>(part + ((size_t)(c2 * 16 + fi) * 9 + t) * 128 + wave * 16 + fg * 4) = acc[t][c2];
}

struct WC128BPlan { int pack, slot_shift, Wv, tiles_y, tiles_x, total_tiles, tiles_per_block, blocks_per_pair, pairs; };

bool wc128b_plan(int N, int H, int W, int Cin, int Cout, WC128BPlan& p) {
  const int cus = isic_cu_count();
  if (Cin % 128 != 0 || Cout % 64 != 0 || N <= 0 || H <= 0 || W <= 0) return false;
  p.pack = W <= 7 ? 4 : (W <= 15 ? 2 : 1);                        // >= 1 empty column between packed images
  p.slot_shift = p.pack == 4 ? 3 : (p.pack == 2 ? 4 : 5);
  p.Wv = p.pack == 1 ? W : T_W;
  p.tiles_y = ceil_div(H, T_H);
  p.tiles_x = ceil_div(p.Wv, T_W);
  const int64_t total = (int64_t)ceil_div(N, p.pack) * p.tiles_y * p.tiles_x;
  if (total > 0x7FFFFFFFLL || (int64_t)N * H * W * (Cin > Cout ? Cin : Cout) > 0x7FFFFFFFFFLL) return false;
  // packed: a lane's byte offset from the first image of its pack is held in 32 bits (wgrad_dma_addr.inc)
  if (p.pack > 1 && (int64_t)(p.pack + 1) * H * W * (Cin > Cout ? Cin : Cout) * 2 > 0x7FFFFFFFLL) return false;
  p.total_tiles = (int)total;
  p.pairs = (Cin / 128) * (Cout / 64);
  const int per_pair = cus >= p.pairs ? cus / p.pairs : 1;
  p.tiles_per_block = (int)ceil_div64(total, per_pair);
  p.blocks_per_pair = (int)ceil_div64(total, p.tiles_per_block);
  return true;
}

}  // namespace

// bytes of workspace the 64-output-channel all-taps kernel needs (0: shape not handled)
size_t isic_wgrad_c128b_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
  WC128BPlan p;
  if (!wc128b_plan(N, H, W, Cin, Cout, p)) return 0;
  return (size_t)p.pairs * p.blocks_per_pair * SLICE_ELEMS * sizeof(float);
}

// called by isic_conv2d_wgrad_bf16 for 3x3, stride 1, pad 1, Cin % 128 == 0, Cout % 64 == 0
int isic_wgrad_c128b_launch(const uint16_t* x, const uint16_t* dy, float* dw, int N, int H, int W, int Cin, int Cout,
                            void* workspace, hipStream_t stream) {
  WC128BPlan p;
  if (!wc128b_plan(N, H, W, Cin, Cout, p)) return ISIC_ERR_UNSUPPORTED;
  WC128BArgs a;
  a.x = x; a.dy = dy; a.partial = reinterpret_cast<float*>(workspace);
  a.N = N; a.H = H; a.W = W;
  a.tiles_y = p.tiles_y; a.tiles_x = p.tiles_x; a.total_tiles = p.total_tiles;
  a.tiles_per_block = p.tiles_per_block; a.blocks_per_pair = p.blocks_per_pair;
  a.Cx = Cin; a.Cy = Cout; a.co_slices = Cout / 64; a.pack = p.pack; a.slot_shift = p.slot_shift; a.Wv = p.Wv;
  const dim3 grid(p.pairs * p.blocks_per_pair);
  const int rc = p.pack > 1 ? isic_launch_lds<wgrad_c128b_kernel<true>, LDS_ALL>(grid, dim3(512), LDS_ALL, stream, a)
                            : isic_launch_lds<wgrad_c128b_kernel<false>, LDS_ALL>(grid, dim3(512), LDS_ALL, stream, a);
  if (rc != ISIC_OK) return rc;
  hipLaunchKernelGGL((wgrad_pair_reduce_kernel<64, 128>), dim3(p.pairs * (SLICE_ELEMS / 64)), dim3(256), 0, stream, a.partial, dw,
                     p.blocks_per_pair, a.co_slices, Cin);
  return isic_launch_status();
}
