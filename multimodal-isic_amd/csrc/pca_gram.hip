// Shifted Gram matrix of resident latents (include/isic_hip_pca.h):  G = beta G + sum_m z_m z_m^T,  colsum = beta colsum +
// sum_m z_m  with  z_m = X[r_m, 0:D] - shift,  fp64 outputs.  The device half of the latent PCA of save_latent.py:163-185
// (sklearn's covariance_eigh solver is this Gram matrix plus a D x D eigenproblem).  Exact fp32 products on
// v_mfma_f32_16x16x4_f32 (gfx950); the reduction dimension is the ROW dimension M.
//
//   * G is cut into 128 x 128 tiles; only the pairs (I, J) with J >= I are computed.  A block owns one pair and one RUN of
//     ISIC_GRAM_RUN = 2048 rows: 4 waves, a 64 x 64 tile each (16 accumulators); on a diagonal pair the wave below the
//     diagonal sits out.
//   * Both operands have the output index contiguous, so the MFMA operands are read as in gemm_f32t.hip: lane l reads ONE
//     float4 Z[k0 + (l >> 4)][c0 + 4 (l & 15) ..+3]; component r is the operand of the 16 x 16 tile whose rows are
//     c0 + 4 i + r.  The rows are staged through LDS 32 at a time (double-buffered, one barrier per stage), the shift is
//     subtracted on the way into LDS, rows past the run and columns past D are staged as zeros.  On a diagonal pair ONE
//     staged panel serves as both operands.
//   * 64-bit row offsets (M ldx exceeds 2^31 at the workload's size); rows[] is read entry by entry, below M only.
//   * The run's fp32 partial tile goes to the workspace; gram_finish_kernel adds the runs' tiles in ascending run order in
//     fp64, applies beta and writes G[i,j] and G[j,i] from one value.  The column sums are formed by the diagonal blocks
//     while they stage (fp32 inside the run: 256 rows per thread, then the 8 row groups in group order) and finished the
//     same way.  No atomics anywhere: the bits do not depend on timing.
//   * Blocks b and b + 8 share an XCD (observed placement, used for speed only): the pairs of one run are dealt to one
//     XCD so that the run's rows are read from HBM once and from that L2 afterwards.
// Error of an element of G: at most gamma(ISIC_GRAM_RUN + 1) sum_m |z_mi| |z_mj| plus the rounding of x - shift
// (tests/pca_ref.py derives the bound the tests use).
#include "common.h"
#include "../../include/isic_hip_pca.h"

namespace {

constexpr int PW = 128;                  // panel (tile) width
constexpr int KT = 32;                   // rows per stage
constexpr int RUN = ISIC_GRAM_RUN;       // rows per fp32 run
constexpr int MAX_TILES = 2048;          // partial tiles parked at a time (~4 rounds of 2 blocks per CU)
constexpr size_t TILE_FLOATS = (size_t)PW * PW;

struct GramArgs {
  const float* X;
  const int32_t* rows;
  const float* shift;
  float* part;                           // [runs][pairs][128][128]
  float* csum;                           // [runs][panels * 128]
  int64_t m_begin, M, ldx;               // first row of this launch; end of the rows
  int D, panels, pairs, runs;            // runs of this launch
};

__device__ __forceinline__ void pair_to_tiles(int pair, int panels, int& I, int& J) {
  int i = 0, p = pair;
  while (p >= panels - i) { p -= panels - i; ++i; }
  I = i; J = i + p;
}

__global__ __launch_bounds__(256) void gram_run_kernel(GramArgs a) {
  __shared__ float4 tile[2][2][KT][PW / 4];          // [buffer][operand][row][column quad]: 64 KB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  // blocks b, b + 8, ... share an XCD: they get the pairs of the same runs
  const int xcd = blockIdx.x & 7, k = blockIdx.x >> 3;
  const int run = (k / a.pairs) * 8 + xcd, pair = k - (k / a.pairs) * a.pairs;
  if (run >= a.runs) return;                         // block-uniform
  int I, J;
  pair_to_tiles(pair, a.panels, I, J);
  const bool diag = I == J;
  const int bsel = diag ? 0 : 1;                     // the B operand's panel in LDS
  const bool works = !(diag && wm == 1 && wn == 0);  // wave-uniform: the tile below the diagonal is never read
  const int64_t m0 = a.m_begin + (int64_t)run * RUN;
  const int64_t m_end = m0 + RUN < a.M ? m0 + RUN : a.M;
  const int stages = (int)((m_end - m0 + KT - 1) / KT);

  // staging: thread (rr, q) moves column quad q of rows rr, rr + 8, rr + 16, rr + 24 of a stage
  const int q = tid & 31, rr = tid >> 5;
  const int cI = I * PW + 4 * q, cJ = J * PW + 4 * q;
  const bool okI = cI < a.D, okJ = !diag && cJ < a.D;
  float4 shI = make_float4(0.f, 0.f, 0.f, 0.f), shJ = shI;
  if (a.shift) {
    if (okI) shI = *reinterpret_cast<const float4*>(a.shift + cI);
    if (okJ) shJ = *reinterpret_cast<const float4*>(a.shift + cJ);
  }
  float4 ra[KT / 8], rb[KT / 8];
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);       // this thread's column sums (diagonal blocks)

  // the row indices are requested one stage ahead of the rows they address, so that no stage waits for an index
  int ridx[KT / 8];
  auto fetch_index = [&](int s) {
#pragma unroll
    for (int p = 0; p < KT / 8; ++p) {
      const int64_t m = m0 + (int64_t)s * KT + rr + 8 * p;
      ridx[p] = (a.rows && m < m_end) ? a.rows[m] : 0;
    }
  };
  auto fetch = [&](int s) {
#pragma unroll
    for (int p = 0; p < KT / 8; ++p) {
      const int64_t m = m0 + (int64_t)s * KT + rr + 8 * p;
      ra[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      rb[p] = ra[p];
      if (m < m_end) {
        const int64_t r = a.rows ? (int64_t)ridx[p] : m;
        const float* row = a.X + r * a.ldx;
        if (okI) ra[p] = *reinterpret_cast<const float4*>(row + cI);
        if (okJ) rb[p] = *reinterpret_cast<const float4*>(row + cJ);
      }
    }
    fetch_index(s + 1);
  };
  auto commit = [&](int s, int buf) {
#pragma unroll
    for (int p = 0; p < KT / 8; ++p) {
      const bool in = m0 + (int64_t)s * KT + rr + 8 * p < m_end;
      float4 za = make_float4(0.f, 0.f, 0.f, 0.f), zb = za;
      if (in && okI) za = make_float4(ra[p].x - shI.x, ra[p].y - shI.y, ra[p].z - shI.z, ra[p].w - shI.w);
      if (in && okJ) zb = make_float4(rb[p].x - shJ.x, rb[p].y - shJ.y, rb[p].z - shJ.z, rb[p].w - shJ.w);
      tile[buf][0][rr + 8 * p][q] = za;
      if (!diag) tile[buf][1][rr + 8 * p][q] = zb;
      if (diag) { cs.x += za.x; cs.y += za.y; cs.z += za.z; cs.w += za.w; }
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  fetch_index(0);
  fetch(0);
  commit(0, 0);
  __syncthreads();
  const int kr = lane >> 4, lq = lane & 15;
  for (int s = 0; s < stages; ++s) {
    const int buf = s & 1;
    const bool more = s + 1 < stages;                // block-uniform
    if (more) fetch(s + 1);
    if (works) {
#pragma unroll
      for (int kk = 0; kk < KT / 4; ++kk) {
        const float4 va = tile[buf][0][4 * kk + kr][wm * 16 + lq];
        const float4 vb = tile[buf][bsel][4 * kk + kr][wn * 16 + lq];
        const float fa[4] = {va.x, va.y, va.z, va.w}, fb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[r], fb[c], acc[r][c], 0, 0, 0);
      }
    }
    if (more) commit(s + 1, buf ^ 1);
    __syncthreads();
  }

  // acc[r][c][v] of lane l = tile[wm 64 + 16 (l >> 4) + 4 v + r][wn 64 + 4 (l & 15) + c]
  if (works) {
    float* out = a.part + ((size_t)run * a.pairs + pair) * TILE_FLOATS + (size_t)(wm * 64 + 16 * kr) * PW + wn * 64 + 4 * lq;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int v = 0; v < 4; ++v)
        *reinterpret_cast<f32x4*>(out + (size_t)(4 * v + r) * PW) = (f32x4){acc[r][0][v], acc[r][1][v], acc[r][2][v], acc[r][3][v]};
  }
  if (diag) {                                        // block-uniform; every wave is past the loop's last barrier
    tile[0][0][rr][q] = cs;
    __syncthreads();
    if (rr == 0) {
      float4 t = tile[0][0][0][q];
#pragma unroll
      for (int g = 1; g < 8; ++g) {
        const float4 u = tile[0][0][g][q];
        t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
      }
      *reinterpret_cast<float4*>(a.csum + (size_t)run * a.panels * PW + cI) = t;
    }
  }
}

// G[i,j] = G[j,i] = beta G[i,j] + sum over the runs (ascending) of the fp32 partials, in fp64; colsum likewise.
// Blocks [0, pairs * 64): 256 elements of a tile each; the blocks after them: 256 columns of colsum each.
__global__ __launch_bounds__(256) void gram_finish_kernel(const float* __restrict__ part, const float* __restrict__ csum,
                                                          double* __restrict__ G, double* __restrict__ colsum, int D,
                                                          int panels, int pairs, int runs, int beta) {
  const int tile_blocks = pairs * (int)(TILE_FLOATS / 256);
  if ((int)blockIdx.x >= tile_blocks) {
    const int d = ((int)blockIdx.x - tile_blocks) * 256 + threadIdx.x;
    if (d >= D) return;
    double s = 0.0;
    for (int z = 0; z < runs; ++z) s += (double)csum[(size_t)z * panels * PW + d];
    colsum[d] = beta ? colsum[d] + s : s;
    return;
  }
  const int pair = blockIdx.x / (int)(TILE_FLOATS / 256);
  const int e = (blockIdx.x - pair * (int)(TILE_FLOATS / 256)) * 256 + threadIdx.x;
  int I, J;
  pair_to_tiles(pair, panels, I, J);
  const int gi = I * PW + e / PW, gj = J * PW + e % PW;
  if (gi >= D || gj >= D || gj < gi) return;
  const float* p = part + (size_t)pair * TILE_FLOATS + e;
  const size_t stride = (size_t)pairs * TILE_FLOATS;
  double s = 0.0;
#pragma unroll 8
  for (int z = 0; z < runs; ++z) s += (double)p[(size_t)z * stride];
  const size_t up = (size_t)gi * D + gj, lo = (size_t)gj * D + gi;
  const double g = beta ? G[up] + s : s;
  G[up] = g;
  G[lo] = g;
}

struct GramPlan { int panels, pairs, slots; int64_t runs; };

bool gram_plan(int64_t M, int D, GramPlan& p) {
  if (M < 0 || D < 4 || D > 1024 || (D & 3)) return false;
  p.panels = ceil_div(D, PW);
  p.pairs = p.panels * (p.panels + 1) / 2;
  p.runs = ceil_div64(M, RUN);
  int slots = (MAX_TILES / p.pairs) & ~7;            // whole groups of 8 runs: one run per XCD label
  if (slots < 8) slots = 8;
  p.slots = (int)(p.runs < slots ? p.runs : slots);
  return true;
}

}  // namespace

extern "C" {

size_t isic_gram_shifted_f32_workspace_bytes(int64_t M, int D) {
  GramPlan p;
  if (!gram_plan(M, D, p)) return 0;
  return (size_t)p.slots * ((size_t)p.pairs * TILE_FLOATS + (size_t)p.panels * PW) * sizeof(float);
}

int isic_gram_shifted_f32(const float* X, int64_t M, int D, int64_t ldx, const int32_t* rows, const float* shift,
                          double* G, double* colsum, double beta, void* workspace, size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && D > 0 && ldx >= 0 && G && colsum && (X || M == 0));
  ISIC_CHECK_ARG(beta == 0.0 || beta == 1.0);
  GramPlan p;
  if (!gram_plan(M, D, p) || ldx < D || (ldx & 3) || (reinterpret_cast<uintptr_t>(X) & 15) ||
      (shift && (reinterpret_cast<uintptr_t>(shift) & 15)))
    return ISIC_ERR_UNSUPPORTED;
  const size_t need = isic_gram_shifted_f32_workspace_bytes(M, D);
  if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))) return ISIC_ERR_WORKSPACE;
  if (M == 0 && beta == 1.0) return ISIC_OK;
  hipStream_t st = as_stream(stream);
  GramArgs a;
  a.X = X; a.rows = rows; a.shift = shift;
  a.part = reinterpret_cast<float*>(workspace);
  a.csum = a.part + (size_t)p.slots * p.pairs * TILE_FLOATS;
  a.M = M; a.ldx = ldx; a.D = D; a.panels = p.panels; a.pairs = p.pairs;
  const int finish_blocks = p.pairs * (int)(TILE_FLOATS / 256) + ceil_div(D, 256);
  int64_t done = 0;
  do {                                               // (once with zero runs when M == 0, beta == 0: the outputs are zeroed)
    const int runs = (int)(p.runs - done < p.slots ? p.runs - done : p.slots);
    if (runs > 0) {
      a.m_begin = done * RUN; a.runs = runs;
      hipLaunchKernelGGL(gram_run_kernel, dim3(ceil_div(runs, 8) * 8 * p.pairs), dim3(256), 0, st, a);
    }
    hipLaunchKernelGGL(gram_finish_kernel, dim3(finish_blocks), dim3(256), 0, st, a.part, a.csum, G, colsum, D, p.panels,
                       p.pairs, runs, (beta == 1.0 || done > 0) ? 1 : 0);
    done += runs;
  } while (done < p.runs);
  return isic_launch_status();
}

}  // extern "C"
