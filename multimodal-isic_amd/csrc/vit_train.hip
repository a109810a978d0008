// Backward pass of a stack of pre-norm transformer blocks (gfx950, fp16 operands, fp32 arithmetic and gradients): the
// weight-gradient GEMM, the attention backward and a column-sum reducer (bias and position-embedding gradients).  The
// data-gradient products and the GELU-derivative epilogue are modes of gemm_f16.hip; the LayerNorm backward is
// isic_layernorm_add_bwd_f16 (convmae_train.hip), which recomputes the forward's statistics.  Entry points:
// include/isic_hip_vit_train.h; the Python side is isic_hip/transformer.py, shared by the three trainable encoders.
//
// The backward runs on gradients multiplied by a power-of-two loss scale S (picked per call); every reduction that
// lands in a parameter gradient multiplies by `scale` = 1/S in fp32.  Every reduction is split over blocks into fp32 slabs
// that one more pass adds in a fixed order: no float atomics, so the step is bit-reproducible.

#include "common.h"

namespace {

// ------------------------------------------------------------------ slab reducer
// out[i] = (accumulate ? out[i] : 0) + scale * sum_{z < S} ws[z][i], z in index order: one thread per element, i.e. order
// A of slab_sum.inc with G = 1 and no tree.  It keeps its own text: it issues four loads ahead of four dependent adds, a
// different instruction stream from the one-load-per-add walk of isic_slab_sum_xor, and the adds are the same either way.
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ ws, int S, int64_t n, float* out,
                                                          float scale, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  int z = 0;
  for (; z + 4 <= S; z += 4) {
    const float a0 = ws[(int64_t)z * n + i], a1 = ws[(int64_t)(z + 1) * n + i];
    const float a2 = ws[(int64_t)(z + 2) * n + i], a3 = ws[(int64_t)(z + 3) * n + i];
    s += a0; s += a1; s += a2; s += a3;
  }
  for (; z < S; ++z) s += ws[(int64_t)z * n + i];
  out[i] = accumulate ? fmaf(scale, s, out[i]) : scale * s;
}

int slab_reduce(const float* ws, int S, int64_t n, float* out, float scale, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, S, n, out, scale,
                     accumulate);
  return isic_launch_status();
}

// ------------------------------------------------------------------ column sums of fp16 rows
// x[R][C] (C % 8 == 0): block (cb, z) sums the 64 columns cb*64.. over rows [z*chunk, (z+1)*chunk): 8 lanes per 8-column
// chunk, 32 row lanes; the row lanes are added in LDS in index order.  S == 1: straight into out with scale / accumulate.
constexpr int CS_ROWS_PER_SLAB = 4096;

struct ColsumPlan { int S; int64_t chunk; };
ColsumPlan colsum_plan(int64_t R) {
  int64_t S = (R + CS_ROWS_PER_SLAB - 1) / CS_ROWS_PER_SLAB;
  if (S > 256) S = 256;
  if (S < 1) S = 1;
  return {(int)S, (R + S - 1) / S};
}

__global__ __launch_bounds__(256) void colsum_f16_kernel(const unsigned short* __restrict__ x, int64_t R, int C,
                                                         int64_t chunk, float* dst, float scale, int direct, int accumulate) {
  __shared__ float part[32][65];
  const int tid = threadIdx.x, cq = tid & 7, rl = tid >> 3;
  const int c0 = blockIdx.x * 64 + cq * 8;
  const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = min(R, r0 + chunk);
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c0 < C) {
    for (int64_t r = r0 + rl; r < r1; r += 32) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(x + r * C + c0);
      const unsigned w0 = v[0], w1 = v[1], w2 = v[2], w3 = v[3];
      s[0] += f16_lo(w0); s[1] += f16_hi(w0); s[2] += f16_lo(w1); s[3] += f16_hi(w1);
      s[4] += f16_lo(w2); s[5] += f16_hi(w2); s[6] += f16_lo(w3); s[7] += f16_hi(w3);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) part[rl][cq * 8 + e] = s[e];
  __syncthreads();
  if (tid < 64) {
    const int c = blockIdx.x * 64 + tid;
    float t = 0.f;
    for (int q = 0; q < 32; ++q) t += part[q][tid];
    if (c < C) {
      if (direct) dst[c] = accumulate ? fmaf(scale, t, dst[c]) : scale * t;
      else dst[(int64_t)blockIdx.y * C + c] = t;
    }
  }
}

int colsum(const unsigned short* x, int64_t R, int C, float* out, float scale, int accumulate, float* ws, hipStream_t st) {
  const ColsumPlan p = colsum_plan(R);
  const dim3 grid((unsigned)((C + 63) / 64), (unsigned)p.S);
  hipLaunchKernelGGL(colsum_f16_kernel, grid, dim3(256), 0, st, x, R, C, p.chunk, p.S == 1 ? out : ws, scale,
                     (int)(p.S == 1), accumulate);
  if (p.S == 1) return isic_launch_status();
  if (isic_launch_status() != ISIC_OK) return ISIC_ERR_LAUNCH;
  return slab_reduce(ws, p.S, C, out, scale, accumulate, st);
}

// ------------------------------------------------------------------ weight gradient  dW[N][K] = sum_m dY[m][n] X[m][k]
// Block: a 128 (n) x 128 (k) output tile over a slab of rows; 4 waves in 2 x 2, each 64 x 64 = 4 x 4 tiles of
// v_mfma_f32_16x16x32_f16 with the contraction over m.  Per step of 32 rows, threads 0-127 stage dY and 128-255 stage X:
// a thread loads 4 rows x 8 columns (four 16-byte loads) and writes them transposed, 4 consecutive m per 8-byte LDS write,
// into [column][m] tiles (row pitch 40 halves = 80 B, 16-byte aligned), so that an MFMA fragment (8 consecutive m of one
// column) is one 16-byte LDS read.  The operands' m order inside a fragment is the same for both, so the MFMA's internal
// k assignment does not matter.  Next step's global loads are in flight during this step's MFMAs.
constexpr int WG_T = 128, WG_MS = 32, WG_PITCH = 40;   // halves
constexpr int WG_TARGET_BLOCKS = 512;

struct WgradPlan { int S; int64_t chunk; };
WgradPlan wgrad_plan(int64_t M, int N, int K) {
  const int tiles = (N / WG_T) * (K / WG_T);
  int64_t S = (WG_TARGET_BLOCKS + tiles - 1) / tiles;
  const int64_t max_s = (M + 4 * WG_MS - 1) / (4 * WG_MS);             // a slab has at least 128 rows
  if (S > max_s) S = max_s;
  if (S < 1) S = 1;
  int64_t chunk = (M + S - 1) / S;
  chunk = (chunk + WG_MS - 1) / WG_MS * WG_MS;
  S = (M + chunk - 1) / chunk;
  if (S < 1) S = 1;
  return {(int)S, chunk};
}

__global__ __launch_bounds__(256) void wgrad_f16_kernel(const unsigned short* __restrict__ dY,
                                                        const unsigned short* __restrict__ X, int64_t M, int N, int K,
                                                        int64_t chunk, float* dst, float scale, int direct, int accumulate) {
  __shared__ __attribute__((aligned(16))) unsigned short sY[2][WG_T * WG_PITCH];
  __shared__ __attribute__((aligned(16))) unsigned short sX[2][WG_T * WG_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * WG_T, k0 = blockIdx.y * WG_T;
  const int64_t mb = (int64_t)blockIdx.z * chunk, me = min(M, mb + chunk);
  // staging role
  const bool isX = tid >= 128;
  const int st = tid & 127, rg = st >> 4, cg = st & 15;      // rows 4rg..4rg+3 of the step, columns 8cg..8cg+7 of the tile
  const unsigned short* src = isX ? X : dY;
  const int ld = isX ? K : N;
  const int col0 = (isX ? k0 : n0) + cg * 8;
  u32x4 buf[4];
  auto load = [&](int64_t m0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t m = m0 + 4 * rg + r;
      buf[r] = m < me ? *reinterpret_cast<const u32x4*>(src + m * ld + col0) : (u32x4){0u, 0u, 0u, 0u};
    }
  };
  auto stash = [&](int b) {
    unsigned short* t = isX ? sX[b] : sY[b];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int w = e >> 1, sh = (e & 1) * 16;
      const unsigned h0 = (buf[0][w] >> sh) & 0xffffu, h1 = (buf[1][w] >> sh) & 0xffffu;
      const unsigned h2 = (buf[2][w] >> sh) & 0xffffu, h3 = (buf[3][w] >> sh) & 0xffffu;
      *reinterpret_cast<u32x2*>(t + (cg * 8 + e) * WG_PITCH + 4 * rg) = (u32x2){h0 | (h1 << 16), h2 | (h3 << 16)};
    }
  };
  // MFMA role: wave (wn, wk) owns n wn*64.., k wk*64..; the first operand is X (its row index = k: a lane ends with four
  // consecutive k of one n -> one 16-byte store)
  const int wn = wave >> 1, wk = wave & 1;
  const int fr = lane & 15, fg = lane >> 4;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  int b = 0;
  if (mb < me) {
    load(mb);
    stash(0);
  }
  __syncthreads();
  for (int64_t m0 = mb; m0 < me; m0 += WG_MS) {
    const bool more = m0 + WG_MS < me;
    if (more) load(m0 + WG_MS);
    f16x8 xa[4], yb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xa[i] = *reinterpret_cast<const f16x8*>(sX[b] + (wk * 64 + i * 16 + fr) * WG_PITCH + fg * 8);
      yb[i] = *reinterpret_cast<const f16x8*>(sY[b] + (wn * 64 + i * 16 + fr) * WG_PITCH + fg * 8);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa[j], yb[i], acc[i][j], 0, 0, 0);
    if (more) stash(b ^ 1);
    __syncthreads();
    b ^= 1;
  }
  // acc[i][j]: n = n0 + wn*64 + i*16 + fr, k = k0 + wk*64 + j*16 + 4*fg + {0..3}
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = n0 + wn * 64 + i * 16 + fr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + wk * 64 + j * 16 + 4 * fg;
      if (direct) {
        f32x4* p = reinterpret_cast<f32x4*>(dst + (int64_t)n * K + k);
        *p = accumulate ? (*p + scale * acc[i][j]) : scale * acc[i][j];
      } else {
        *reinterpret_cast<f32x4*>(dst + ((int64_t)blockIdx.z * N + n) * K + k) = acc[i][j];
      }
    }
  }
}

bool wgrad_dim_ok(int d) { return d >= WG_T && d <= 4096 && d % WG_T == 0; }

size_t wgrad_ws_bytes(int64_t M, int N, int K, bool with_bias) {
  const WgradPlan p = wgrad_plan(M, N, K);
  size_t b = p.S > 1 ? (size_t)p.S * N * K * sizeof(float) : 0;
  if (with_bias) {
    const ColsumPlan c = colsum_plan(M);
    const size_t cb = c.S > 1 ? (size_t)c.S * N * sizeof(float) : 0;
    if (cb > b) b = cb;
  }
  return b;
}

// ------------------------------------------------------------------ attention backward, one block per (image, head)
// Scalar fp32 on VALU (fp16 pair dot products on v_dot2): S and P are recomputed from Q and K.
//   pass 1 (thread = query i): row max m_i and sum l_i of exp(s_ij - m_i), Delta_i = dO_i . O_i
//   pass 2 (thread = query i): dQ_i = scale * sum_j dS_ij K_j,  dS_ij = P_ij (dO_i . V_j - Delta_i)
//   pass 3 (thread = key j):   dV_j = sum_i P_ij dO_i,  dK_j = scale * sum_i dS_ij Q_i
// Every sum runs in index order inside one thread: deterministic without atomics.  Q, K, V, dO of the (image, head) sit in
// LDS as fp16 (4 x T x 128 B, 106.5 KB at T = 208); reads of a row by all lanes are broadcasts.
// Templated on the head width HD in {32, 64} (the MAE decoder's heads are 32 wide); HD = 64 is the kernel as described.
constexpr int AB_MAXT = 208, AB_THREADS = 256;
template <int HD> constexpr int ab_lds() { return 4 * AB_MAXT * HD * 2 + 3 * AB_MAXT * 4; }

template <int HD>
__device__ __forceinline__ float dot_hd(const f16x2 (&a)[HD / 2], const unsigned short* row) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < HD / 8; ++c) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(row + 8 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_fdot2(a[4 * c + e], __builtin_bit_cast(f16x2, (unsigned)v[e]), s, false);
  }
  return s;
}
template <int HD>
__device__ __forceinline__ void axpy_hd(float (&acc)[HD], float w, const unsigned short* row) {
#pragma unroll
  for (int c = 0; c < HD / 8; ++c) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(row + 8 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned u = v[e];
      acc[8 * c + 2 * e] = fmaf(w, f16_lo(u), acc[8 * c + 2 * e]);
      acc[8 * c + 2 * e + 1] = fmaf(w, f16_hi(u), acc[8 * c + 2 * e + 1]);
    }
  }
}
template <int HD>
__device__ __forceinline__ void load_row(f16x2 (&r)[HD / 2], const unsigned short* p) {
#pragma unroll
  for (int c = 0; c < HD / 8; ++c) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(p + 8 * c);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[4 * c + e] = __builtin_bit_cast(f16x2, (unsigned)v[e]);
  }
}
template <int HD>
__device__ __forceinline__ void store_row(unsigned short* p, const float (&a)[HD], float mul) {
#pragma unroll
  for (int c = 0; c < HD / 8; ++c) {
    u32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = f16_pack2(a[8 * c + 2 * e] * mul, a[8 * c + 2 * e + 1] * mul);
    *reinterpret_cast<u32x4*>(p + 8 * c) = v;
  }
}

template <int HD>
__global__ __launch_bounds__(AB_THREADS) void attention_bwd_f16_kernel(const unsigned short* __restrict__ qkv,
                                                                       const unsigned short* __restrict__ out,
                                                                       const unsigned short* __restrict__ dout,
                                                                       unsigned short* __restrict__ dqkv, int T, int H) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned short* sQ = reinterpret_cast<unsigned short*>(smem);
  unsigned short* sK = sQ + AB_MAXT * HD;
  unsigned short* sV = sK + AB_MAXT * HD;
  unsigned short* sO = sV + AB_MAXT * HD;                   // dO
  float* sM = reinterpret_cast<float*>(sO + AB_MAXT * HD);
  float* sL = sM + AB_MAXT;                                  // 1 / l_i
  float* sD = sL + AB_MAXT;                                  // Delta_i
  const int img = blockIdx.x / H, h = blockIdx.x - img * H;
  const int D = H * HD, ld = 3 * D;
  const int64_t row0 = (int64_t)img * T;
  const float sc = HD == 64 ? 0.125f : 0.17677669529663688f;       // 1 / sqrt(HD)
  const int tid = threadIdx.x;
  for (int i = tid; i < T * (HD / 8); i += AB_THREADS) {
    const int t = i / (HD / 8), c = (i % (HD / 8)) * 8;
    const unsigned short* base = qkv + (row0 + t) * ld + h * HD + c;
    *reinterpret_cast<u32x4*>(sQ + t * HD + c) = *reinterpret_cast<const u32x4*>(base);
    *reinterpret_cast<u32x4*>(sK + t * HD + c) = *reinterpret_cast<const u32x4*>(base + D);
    *reinterpret_cast<u32x4*>(sV + t * HD + c) = *reinterpret_cast<const u32x4*>(base + 2 * D);
    *reinterpret_cast<u32x4*>(sO + t * HD + c) = *reinterpret_cast<const u32x4*>(dout + (row0 + t) * D + h * HD + c);
  }
  __syncthreads();
  const int i = tid;
  f16x2 a[HD / 2], b[HD / 2];
  if (i < T) {
    // pass 1
    load_row<HD>(a, sQ + i * HD);
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < T; ++j) {
      const float s = dot_hd<HD>(a, sK + j * HD) * sc;
      if (s > m) { l = l * __expf(m - s) + 1.f; m = s; }
      else l += __expf(s - m);
    }
    load_row<HD>(b, sO + i * HD);
    const unsigned short* orow = out + (row0 + i) * D + h * HD;
    float dl = 0.f;
#pragma unroll
    for (int c = 0; c < HD / 8; ++c) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(orow + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) dl = __builtin_amdgcn_fdot2(b[4 * c + e], __builtin_bit_cast(f16x2, (unsigned)v[e]), dl, false);
    }
    sM[i] = m; sL[i] = 1.f / l; sD[i] = dl;
    // pass 2
    float dq[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) dq[d] = 0.f;
    const float rl = 1.f / l;
    for (int j = 0; j < T; ++j) {
      const float p = __expf(dot_hd<HD>(a, sK + j * HD) * sc - m) * rl;
      const float ds = p * (dot_hd<HD>(b, sV + j * HD) - dl);
      axpy_hd<HD>(dq, ds, sK + j * HD);
    }
    store_row<HD>(dqkv + (row0 + i) * ld + h * HD, dq, sc);
  }
  __syncthreads();
  if (i < T) {
    // pass 3 (thread = key j = i)
    load_row<HD>(a, sK + i * HD);
    load_row<HD>(b, sV + i * HD);
    float dk[HD], dv[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
    for (int q = 0; q < T; ++q) {
      const float p = __expf(dot_hd<HD>(a, sQ + q * HD) * sc - sM[q]) * sL[q];
      const float ds = p * (dot_hd<HD>(b, sO + q * HD) - sD[q]);
      axpy_hd<HD>(dv, p, sO + q * HD);
      axpy_hd<HD>(dk, ds, sQ + q * HD);
    }
    store_row<HD>(dqkv + (row0 + i) * ld + D + h * HD, dk, sc);
    store_row<HD>(dqkv + (row0 + i) * ld + 2 * D + h * HD, dv, 1.f);
  }
}

}  // namespace

extern "C" {

size_t isic_gemm_f16_wgrad_workspace_bytes(int64_t M, int N, int K) {
  if (M <= 0 || !wgrad_dim_ok(N) || !wgrad_dim_ok(K)) return 0;
  return wgrad_ws_bytes(M, N, K, true);
}

int isic_gemm_f16_wgrad(const uint16_t* dY, const uint16_t* X, float* dW, float* db, int64_t M, int N, int K, float scale,
                        int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && N > 0 && K > 0 && (accumulate == 0 || accumulate == 1));
  if (!wgrad_dim_ok(N) || !wgrad_dim_ok(K)) return ISIC_ERR_UNSUPPORTED;
  ISIC_CHECK_ARG(dW && (M == 0 || (dY && X)));
  hipStream_t st = as_stream(stream);
  if (M == 0) {                                        // an empty sum: zero, or nothing to add
    if (accumulate) return ISIC_OK;
    if (hipMemsetAsync(dW, 0, (size_t)N * K * sizeof(float), st) != hipSuccess) return ISIC_ERR_LAUNCH;
    if (db && hipMemsetAsync(db, 0, (size_t)N * sizeof(float), st) != hipSuccess) return ISIC_ERR_LAUNCH;
    return ISIC_OK;
  }
  if (workspace_bytes < wgrad_ws_bytes(M, N, K, db != nullptr) || (workspace_bytes > 0 && !workspace))
    return ISIC_ERR_WORKSPACE;
  float* ws = reinterpret_cast<float*>(workspace);
  const WgradPlan p = wgrad_plan(M, N, K);
  const dim3 grid(N / WG_T, K / WG_T, p.S);
  hipLaunchKernelGGL(wgrad_f16_kernel, grid, dim3(256), 0, st, dY, X, M, N, K, p.chunk, p.S == 1 ? dW : ws, scale,
                     (int)(p.S == 1), accumulate);
  if (isic_launch_status() != ISIC_OK) return ISIC_ERR_LAUNCH;
  if (p.S > 1) {
    const int rc = slab_reduce(ws, p.S, (int64_t)N * K, dW, scale, accumulate, st);
    if (rc != ISIC_OK) return rc;
  }
  return db ? colsum(dY, M, N, db, scale, accumulate, ws, st) : ISIC_OK;
}

size_t isic_colsum_f16_workspace_bytes(int64_t rows, int cols) {
  if (rows <= 0 || cols <= 0) return 0;
  const ColsumPlan p = colsum_plan(rows);
  return p.S > 1 ? (size_t)p.S * cols * sizeof(float) : 0;
}

int isic_colsum_f16(const uint16_t* x, float* out, int64_t rows, int cols, float scale, int accumulate, void* workspace,
                    size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(rows >= 0 && cols > 0 && (accumulate == 0 || accumulate == 1));
  if (cols % 8 != 0) return ISIC_ERR_UNSUPPORTED;
  ISIC_CHECK_ARG(out && (rows == 0 || x));
  hipStream_t st = as_stream(stream);
  if (rows == 0) {
    if (accumulate) return ISIC_OK;
    return hipMemsetAsync(out, 0, (size_t)cols * sizeof(float), st) == hipSuccess ? ISIC_OK : ISIC_ERR_LAUNCH;
  }
  if (workspace_bytes < isic_colsum_f16_workspace_bytes(rows, cols) || (workspace_bytes > 0 && !workspace))
    return ISIC_ERR_WORKSPACE;
  return colsum(x, rows, cols, out, scale, accumulate, reinterpret_cast<float*>(workspace), st);
}

int isic_attention_bwd_f16(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, uint16_t* dqkv, int n_images,
                           int tokens, int heads, int head_dim, void* stream) {
  ISIC_CHECK_ARG(n_images >= 0 && tokens > 0 && heads > 0 && head_dim > 0);
  if (head_dim != 64 || tokens > AB_MAXT) return ISIC_ERR_UNSUPPORTED;
  if (n_images == 0) return ISIC_OK;
  ISIC_CHECK_ARG(qkv && out && dout && dqkv);
  return isic_launch_lds<attention_bwd_f16_kernel<64>, ab_lds<64>()>(dim3(n_images * heads), dim3(AB_THREADS), ab_lds<64>(),
                                                                     as_stream(stream), qkv, out, dout, dqkv, tokens, heads);
}

// include/isic_hip_mae.h: the MAE decoder's heads, 32 wide
int isic_attention_d32_bwd_f16(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, uint16_t* dqkv, int n_images,
                               int tokens, int heads, void* stream) {
  ISIC_CHECK_ARG(n_images >= 0 && tokens > 0 && heads > 0);
  if (tokens > AB_MAXT) return ISIC_ERR_UNSUPPORTED;
  if (n_images == 0) return ISIC_OK;
  ISIC_CHECK_ARG(qkv && out && dout && dqkv);
  return isic_launch_lds<attention_bwd_f16_kernel<32>, ab_lds<32>()>(dim3(n_images * heads), dim3(AB_THREADS), ab_lds<32>(),
                                                                     as_stream(stream), qkv, out, dout, dqkv, tokens, heads);
}

}  // extern "C"
