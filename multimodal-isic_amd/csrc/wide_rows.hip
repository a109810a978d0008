// The wide rows of GraphMIL (gfx950): attention pooling over up to 4096 feature columns and up to eight pooling heads, and
// the LayerNorm backward over up to 4096 columns (include/isic_hip_wide.h).
//
// Replaces 05_train_gnns.py:205-213 (multi-head pool, mean over heads) and the backward of 05_train_gnns.py:187-199
// (LayerNorm -> ReLU -> Dropout -> residual) where gnn_concat=True makes the width hidden x heads > 1024 or att_heads = 8
// (tune_mil.py:170-200).  The kernels of attn_pool.hip keep zacc[heads][H / 64] in registers, which is what stops them at
// four heads and 1024 columns.  Nothing here works per head over H:
//   forward   z = (1/K) sum_k sum_n a[n,k] h[n] = sum_n abar[n] h[n],  abar[n] = mean_k a[n,k]
//   backward  dL/da[n,k] = dz . h[n] / K =: g[n] for every head k;  ds[n,k] = a[n,k] (g[n] - sum_m a[m,k] g[m])
// so the H-wide work is one weighted column sum (forward), one dot per row and one scaled copy of dz per row (backward),
// and the per-head work is the softmax over the bag on heads floats per row in LDS.  No atomics in the pool kernels: every
// sum has a fixed order.
#include "common.h"
#include "slab_sum.inc"

namespace {

constexpr int SC_NWAVE = 8, SC_NTHR = SC_NWAVE * 64;        // scores / softmax: a block per bag (a wave per head in the softmax)
constexpr int BW_NWAVE = 16, BW_NTHR = BW_NWAVE * 64;       // backward rows: a block per bag
constexpr int ZS_COLS = 64, ZS_GROUPS = 4;                  // column sum: 64 columns x 4 row groups per block
constexpr int DH_COLS = 256, DH_SPLIT = 8;                  // d_h: 256 columns per block, rows blockIdx.z (mod 8)

__host__ __device__ inline int pad4(int n) { return (n + 3) & ~3; }        // every LDS carve a multiple of 16 bytes

// sum over the A columns of head k of row . w (a wave; VEC: A % 4 == 0 and 16-byte aligned rows)
template <bool VEC>
__device__ __forceinline__ float head_dot(const float* __restrict__ row, const float* __restrict__ w, int n, int lane) {
  float p = 0.f;
  if (VEC) {
    const f32x4* r4 = reinterpret_cast<const f32x4*>(row);
    const f32x4* w4 = reinterpret_cast<const f32x4*>(w);
    for (int i = lane; i < (n >> 2); i += 64) {
      const f32x4 a = r4[i], b = w4[i];
      p += (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
    }
  } else {
    for (int j = lane; j < n; j += 64) p += row[j] * w[j];
  }
  return wave_sum(p);
}

// ---- forward, launch 1: scores (a wave per row), softmax over the bag per head (wave k owns head k), att.
// LDS (floats): w3s[pad4(NH*A)] | sc[pad4(max_bag*NH)] | Ms[8] | Ls[8]
template <bool VEC>
__global__ __launch_bounds__(SC_NTHR) void pool_wide_att_kernel(const float* __restrict__ t, const float* __restrict__ w3,
                                                                 const float* __restrict__ b3,
                                                                 const int64_t* __restrict__ offsets, int A, int NH,
                                                                 int max_bag, float* __restrict__ att) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* w3s = smem;
  float* sc = w3s + pad4(NH * A);
  float* Ms = sc + pad4(max_bag * NH);
  float* Ls = Ms + 8;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int64_t lo = offsets[b];
  const int nb = (int)(offsets[b + 1] - lo);
  if (nb <= 0) return;                                       // block-uniform: an empty bag writes nothing here
  const int At = NH * A;
  for (int i = tid; i < At; i += SC_NTHR) w3s[i] = w3[i];
  __syncthreads();
  for (int n = wave; n < nb; n += SC_NWAVE) {
    const float* trow = t + (size_t)(lo + n) * At;
    for (int k = 0; k < NH; ++k) {
      const float s = head_dot<VEC>(trow + k * A, w3s + k * A, A, lane) + b3[k];
      if (lane == 0) sc[n * NH + k] = s;
    }
  }
  __syncthreads();
  if (wave < NH) {                                           // fixed lane-strided order, then a fixed reduction tree
    const int k = wave;
    float mx = -INFINITY;
    for (int n = lane; n < nb; n += 64) mx = fmaxf(mx, sc[n * NH + k]);
    mx = wave_max(mx);
    float se = 0.f;
    for (int n = lane; n < nb; n += 64) se += expf(sc[n * NH + k] - mx);
    se = wave_sum(se);
    if (lane == 0) { Ms[k] = mx; Ls[k] = se; }
  }
  __syncthreads();
  for (int i = tid; i < nb * NH; i += SC_NTHR) {
    const int k = i % NH;
    att[(size_t)lo * NH + i] = expf(sc[i] - Ms[k]) / Ls[k];
  }
}

// abar[n] = mean_k att[n,k] of the bag's rows into LDS (heads adds in head order, one division)
__device__ __forceinline__ void head_mean_to_lds(const float* __restrict__ att, int64_t lo, int nb, int NH, float* ab,
                                                 int tid, int nthr) {
  for (int n = tid; n < nb; n += nthr) {
    const float* ar = att + (size_t)(lo + n) * NH;
    float s = ar[0];
    for (int k = 1; k < NH; ++k) s += ar[k];
    ab[n] = s / (float)NH;
  }
}

// ---- forward, launch 2: z[b, col] = sum_n abar[n] h[n, col].  Block (column chunk, bag): 64 columns x 4 row groups; group
// g walks the rows n = g (mod 4), four of them in flight; the four partial sums meet in LDS in group order.
// LDS (floats): ab[pad4(max_bag)] | zp[4][64]
__global__ __launch_bounds__(ZS_COLS * ZS_GROUPS) void pool_wide_sum_kernel(const float* __restrict__ h,
                                                                              const float* __restrict__ att,
                                                                              const int64_t* __restrict__ offsets, int H,
                                                                              int NH, int max_bag, float* __restrict__ z) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ab = smem;
  float* zp = ab + pad4(max_bag);
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int b = blockIdx.y;
  const int64_t lo = offsets[b];
  const int nb = (int)(offsets[b + 1] - lo);
  head_mean_to_lds(att, lo, nb, NH, ab, tid, ZS_COLS * ZS_GROUPS);
  __syncthreads();
  const int col = blockIdx.x * ZS_COLS + lane;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (col < H) {
    const float* hp = h + (size_t)lo * H + col;
    int n = g;
    for (; n + 3 * ZS_GROUPS < nb; n += 4 * ZS_GROUPS) {
      const float h0 = hp[(size_t)n * H], h1 = hp[(size_t)(n + ZS_GROUPS) * H], h2 = hp[(size_t)(n + 2 * ZS_GROUPS) * H],
                  h3 = hp[(size_t)(n + 3 * ZS_GROUPS) * H];
      s0 += ab[n] * h0; s1 += ab[n + ZS_GROUPS] * h1; s2 += ab[n + 2 * ZS_GROUPS] * h2; s3 += ab[n + 3 * ZS_GROUPS] * h3;
    }
    for (; n < nb; n += ZS_GROUPS) s0 += ab[n] * hp[(size_t)n * H];
  }
  zp[g * ZS_COLS + lane] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && col < H)
    z[(size_t)b * H + col] = (zp[lane] + zp[ZS_COLS + lane]) + (zp[2 * ZS_COLS + lane] + zp[3 * ZS_COLS + lane]);
}

// ---- backward, launch 1 (a block per bag): g[n] = dz . h[n] / heads (a wave per row), dot[k] = sum_n att[n,k] g[n] (wave k,
// fixed order), ds[n,k] = att[n,k] (g[n] - dot[k]), d_u[n, kA + j] = ds[n,k] w3[k,j] (1 - t^2).
// LDS (floats): w3s[pad4(NH*A)] | dzs[pad4(H)] | gs[pad4(max_bag)] | dots[8]
template <bool VECH, bool VECA>
__global__ __launch_bounds__(BW_NTHR) void pool_wide_bwd_rows_kernel(const float* __restrict__ h, const float* __restrict__ t,
                                                                      const float* __restrict__ att,
                                                                      const float* __restrict__ w3,
                                                                      const int64_t* __restrict__ offsets, int H, int A,
                                                                      int NH, int max_bag, const float* __restrict__ d_z,
                                                                      float* __restrict__ d_u, float* __restrict__ d_s) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* w3s = smem;
  float* dzs = w3s + pad4(NH * A);
  float* gs = dzs + pad4(H);
  float* dots = gs + pad4(max_bag);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int64_t lo = offsets[b];
  const int nb = (int)(offsets[b + 1] - lo);
  if (nb <= 0) return;                                       // block-uniform
  const int At = NH * A;
  for (int i = tid; i < At; i += BW_NTHR) w3s[i] = w3[i];
  for (int i = tid; i < H; i += BW_NTHR) dzs[i] = d_z[(size_t)b * H + i];
  __syncthreads();
  for (int n = wave; n < nb; n += BW_NWAVE) {
    const float p = head_dot<VECH>(h + (size_t)(lo + n) * H, dzs, H, lane);
    if (lane == 0) gs[n] = p / (float)NH;
  }
  __syncthreads();
  if (wave < NH) {
    float d = 0.f;
    for (int n = lane; n < nb; n += 64) d += att[(size_t)(lo + n) * NH + wave] * gs[n];
    d = wave_sum(d);
    if (lane == 0) dots[wave] = d;
  }
  __syncthreads();
  for (int n = wave; n < nb; n += BW_NWAVE) {
    const float gn = gs[n];
    const float* trow = t + (size_t)(lo + n) * At;
    float* urow = d_u + (size_t)(lo + n) * At;
    for (int k = 0; k < NH; ++k) {
      const float ds = att[(size_t)(lo + n) * NH + k] * (gn - dots[k]);
      if (lane == 0) d_s[(size_t)(lo + n) * NH + k] = ds;
      if (VECA) {
        const f32x4* t4 = reinterpret_cast<const f32x4*>(trow + k * A);
        const f32x4* w4 = reinterpret_cast<const f32x4*>(w3s + k * A);
        f32x4* u4 = reinterpret_cast<f32x4*>(urow + k * A);
        for (int i = lane; i < (A >> 2); i += 64) {
          const f32x4 tv = t4[i], wv = w4[i];
          f32x4 uv;
#pragma unroll
          for (int e = 0; e < 4; ++e) uv[e] = ds * wv[e] * (1.f - tv[e] * tv[e]);
          u4[i] = uv;
        }
      } else {
        for (int j = lane; j < A; j += 64) {
          const float tv = trow[k * A + j];
          urow[k * A + j] = ds * w3s[k * A + j] * (1.f - tv * tv);
        }
      }
    }
  }
}

// ---- backward, launch 2: d_h[n, col] (+)= abar[n] dz[b, col].  Block (column chunk, bag, row slot): a thread per column
// keeps its dz value; rows n = blockIdx.z (mod DH_SPLIT).  abar[n] is block-uniform (heads loads of att per row).
__global__ __launch_bounds__(DH_COLS) void pool_wide_dh_kernel(const float* __restrict__ att, const int64_t* __restrict__ offsets,
                                                               int H, int NH, const float* __restrict__ d_z,
                                                               float* __restrict__ d_h, int accumulate) {
  const int b = blockIdx.y;
  const int64_t lo = offsets[b];
  const int nb = (int)(offsets[b + 1] - lo);
  const int col = blockIdx.x * DH_COLS + threadIdx.x;
  if (col >= H) return;
  const float dzv = d_z[(size_t)b * H + col];
  for (int n = blockIdx.z; n < nb; n += DH_SPLIT) {
    const float* ar = att + (size_t)(lo + n) * NH;
    float s = ar[0];
    for (int k = 1; k < NH; ++k) s += ar[k];
    const float v = (s / (float)NH) * dzv;
    float* p = d_h + (size_t)(lo + n) * H + col;
    *p = accumulate ? *p + v : v;
  }
}

__device__ __forceinline__ bool keep_elem(unsigned long long idx, unsigned int thr, unsigned long long seed,
                                          unsigned long long stream_id) {
  return thr == 0 || philox_word(idx, seed, stream_id) >= thr;
}

// ---- LayerNorm backward, N <= 256 JN (any N, any alignment): a block of 256 threads per row (rows blockIdx.x, + gridDim.x, ...), thread tid owns
// the columns tid + 256 j.  The arithmetic per element, the ReLU mask and the dropout words are layernorm_bwd_kernel's
// (rowwise.hip); only the two row sums differ in shape: wave shuffles, then the four waves through LDS (two buffers, so one
// barrier per row).  A column belongs to one thread of the block: its dgamma / dbeta partials over the block's rows never
// leave registers until the end.
template <int JN>
__global__ __launch_bounds__(256) void layernorm_bwd_wide_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta, int M, int N, int relu,
    unsigned int thr, float scale, unsigned long long seed, unsigned long long stream_id,
    const unsigned long long* __restrict__ clock, float* __restrict__ partial) {
  if (clock) stream_id += clock[0] * 1024ULL;        // device step clock (captured graphs): stream = base + step * 1024
  extern __shared__ __attribute__((aligned(16))) float smem[];      // red[2 buffers][2 sums][4 waves]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float pg[JN], pb[JN], gam[JN], bet[JN];
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const int col = tid + 256 * j;
    pg[j] = 0.f; pb[j] = 0.f;
    gam[j] = col < N ? gamma[col] : 0.f;
    bet[j] = col < N ? beta[col] : 0.f;
  }
  int buf = 0;
  for (int row = blockIdx.x; row < M; row += gridDim.x, buf ^= 1) {          // block-uniform trip count
    const float mean = mean_in[row], rstd = rstd_in[row];
    float g[JN], xh[JN];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      const int col = tid + 256 * j;
      g[j] = 0.f; xh[j] = 0.f;
      if (col < N) {
        const size_t idx = (size_t)row * N + col;
        xh[j] = (x[idx] - mean) * rstd;
        float gg = dy[idx];
        if (thr) gg = keep_elem((unsigned long long)idx, thr, seed, stream_id) ? gg * scale : 0.f;
        if (relu && !(xh[j] * gam[j] + bet[j] > 0.f)) gg = 0.f;
        pg[j] += gg * xh[j];
        pb[j] += gg;
        g[j] = gg * gam[j];
        s1 += g[j];
        s2 += g[j] * xh[j];
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    float* red = smem + buf * 8;
    if (lane == 0) { red[wave] = s1; red[4 + wave] = s2; }
    __syncthreads();
    s1 = ((red[0] + red[1]) + (red[2] + red[3])) / (float)N;
    s2 = ((red[4] + red[5]) + (red[6] + red[7])) / (float)N;
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      const int col = tid + 256 * j;
      if (col < N) dx[(size_t)row * N + col] = rstd * (g[j] - s1 - xh[j] * s2);
    }
  }
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const int col = tid + 256 * j;
    if (col < N) {
      if (partial) {                                 // deterministic: the block's own row, ln_bwd_reduce_kernel adds in order
        partial[(size_t)blockIdx.x * 2 * N + col] = pg[j];
        partial[(size_t)blockIdx.x * 2 * N + N + col] = pb[j];
      } else {                                       // 256 contiguous bytes per wave instruction
        atomicAdd(&dgamma[col], pg[j]);
        atomicAdd(&dbeta[col], pb[j]);
      }
    }
  }
}

// ---- ... for N % 4 == 0 and 16-byte aligned rows: thread tid owns the FOUR columns 4 (tid + 256 j) .. + 3 -- 16-byte
// accesses and one Philox block per four elements (the scalar form evaluates the block once per element), the same words:
// element row N + col is word (col & 3) of block (row N + col) >> 2.  JV = ceil(N / 1024) vectors per thread.
template <int JV>
__global__ __launch_bounds__(256) void layernorm_bwd_wide_vec_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta, int M, int N, int relu,
    unsigned int thr, float scale, unsigned long long seed, unsigned long long stream_id,
    const unsigned long long* __restrict__ clock, float* __restrict__ partial) {
  if (clock) stream_id += clock[0] * 1024ULL;        // device step clock (captured graphs): stream = base + step * 1024
  extern __shared__ __attribute__((aligned(16))) float smem[];      // red[2 buffers][2 sums][4 waves]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 pg[JV], pb[JV], gam[JV], bet[JV];
#pragma unroll
  for (int j = 0; j < JV; ++j) {
    const int col = 4 * (tid + 256 * j);
    pg[j] = zero; pb[j] = zero;
    gam[j] = col < N ? *reinterpret_cast<const f32x4*>(gamma + col) : zero;
    bet[j] = col < N ? *reinterpret_cast<const f32x4*>(beta + col) : zero;
  }
  int buf = 0;
  for (int row = blockIdx.x; row < M; row += gridDim.x, buf ^= 1) {          // block-uniform trip count
    const float mean = mean_in[row], rstd = rstd_in[row];
    f32x4 g[JV], xh[JV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < JV; ++j) {
      const int col = 4 * (tid + 256 * j);
      g[j] = zero; xh[j] = zero;
      if (col < N) {
        const size_t idx = (size_t)row * N + col;
        xh[j] = (*reinterpret_cast<const f32x4*>(x + idx) - mean) * rstd;
        f32x4 gg = *reinterpret_cast<const f32x4*>(dy + idx);
        if (thr) {
          const Philox4 r = philox_block((unsigned long long)idx >> 2, seed, stream_id);
          gg[0] = r.x >= thr ? gg[0] * scale : 0.f; gg[1] = r.y >= thr ? gg[1] * scale : 0.f;
          gg[2] = r.z >= thr ? gg[2] * scale : 0.f; gg[3] = r.w >= thr ? gg[3] * scale : 0.f;
        }
        if (relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (!(xh[j][e] * gam[j][e] + bet[j][e] > 0.f)) gg[e] = 0.f;
        }
        pg[j] += gg * xh[j];
        pb[j] += gg;
        g[j] = gg * gam[j];
        const f32x4 gx = g[j] * xh[j];
        s1 += (g[j][0] + g[j][1]) + (g[j][2] + g[j][3]);
        s2 += (gx[0] + gx[1]) + (gx[2] + gx[3]);
      }
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    float* red = smem + buf * 8;
    if (lane == 0) { red[wave] = s1; red[4 + wave] = s2; }
    __syncthreads();
    s1 = ((red[0] + red[1]) + (red[2] + red[3])) / (float)N;
    s2 = ((red[4] + red[5]) + (red[6] + red[7])) / (float)N;
#pragma unroll
    for (int j = 0; j < JV; ++j) {
      const int col = 4 * (tid + 256 * j);
      if (col < N) *reinterpret_cast<f32x4*>(dx + (size_t)row * N + col) = (g[j] - s1 - xh[j] * s2) * rstd;
    }
  }
#pragma unroll
  for (int j = 0; j < JV; ++j) {
    const int col = 4 * (tid + 256 * j);
    if (col < N) {
      if (partial) {                                 // deterministic: the block's own row, ln_bwd_reduce_kernel adds in order
        *reinterpret_cast<f32x4*>(partial + (size_t)blockIdx.x * 2 * N + col) = pg[j];
        *reinterpret_cast<f32x4*>(partial + (size_t)blockIdx.x * 2 * N + N + col) = pb[j];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          atomicAdd(&dgamma[col + e], pg[j][e]);
          atomicAdd(&dbeta[col + e], pb[j][e]);
        }
      }
    }
  }
}

// the row kernels size their LDS by the call's shape: up to a workgroup's 160 KB runs, more is ISIC_ERR_UNSUPPORTED
constexpr int WIDE_MAX_LDS = 160 * 1024;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int pool_wide_domain(int H, int A, int heads, int max_bag) {
  return (H > ISIC_WIDE_MAX_H || A > ISIC_WIDE_MAX_A || heads > ISIC_WIDE_MAX_HEADS || max_bag > ISIC_WIDE_MAX_BAG)
             ? ISIC_ERR_UNSUPPORTED : ISIC_OK;
}

}  // namespace

extern "C" {

int isic_attn_pool_wide_fwd(const float* h, const float* t, const float* w3, const float* b3, const int64_t* offsets,
                            int B, int H, int A, int heads, int max_bag, float* att, float* z, void* stream) {
  ISIC_CHECK_ARG(B >= 0 && H > 0 && A > 0 && heads > 0 && max_bag >= 0);
  if (B == 0) return ISIC_OK;
  ISIC_CHECK_ARG(h && t && w3 && b3 && offsets && att && z);
  int rc = pool_wide_domain(H, A, heads, max_bag);
  if (rc != ISIC_OK) return rc;
  const size_t lds1 = sizeof(float) * ((size_t)pad4(heads * A) + pad4(max_bag * heads) + 16);
  const bool vec = A % 4 == 0 && aligned16(t);
  rc = vec ? isic_launch_lds<pool_wide_att_kernel<true>, WIDE_MAX_LDS>(dim3(B), dim3(SC_NTHR), lds1, as_stream(stream), t, w3, b3,
                                                                       offsets, A, heads, max_bag, att)
           : isic_launch_lds<pool_wide_att_kernel<false>, WIDE_MAX_LDS>(dim3(B), dim3(SC_NTHR), lds1, as_stream(stream), t, w3, b3,
                                                                        offsets, A, heads, max_bag, att);
  if (rc != ISIC_OK) return rc;
  const size_t lds2 = sizeof(float) * ((size_t)pad4(max_bag) + ZS_GROUPS * ZS_COLS);
  hipLaunchKernelGGL(pool_wide_sum_kernel, dim3(ceil_div(H, ZS_COLS), B), dim3(ZS_COLS * ZS_GROUPS), lds2, as_stream(stream),
                     h, att, offsets, H, heads, max_bag, z);
  return isic_launch_status();
}

int isic_attn_pool_wide_bwd(const float* h, const float* t, const float* att, const float* w3, const int64_t* offsets,
                            int B, int H, int A, int heads, int max_bag, const float* d_z, float* d_h,
                            int accumulate_dh, float* d_u, float* d_s, void* stream) {
  ISIC_CHECK_ARG(B >= 0 && H > 0 && A > 0 && heads > 0 && max_bag >= 0);
  if (B == 0) return ISIC_OK;
  ISIC_CHECK_ARG(h && t && att && w3 && offsets && d_z && d_h && d_u && d_s);
  int rc = pool_wide_domain(H, A, heads, max_bag);
  if (rc != ISIC_OK) return rc;
  const size_t lds = sizeof(float) * ((size_t)pad4(heads * A) + pad4(H) + pad4(max_bag) + 8);
  const bool vech = H % 4 == 0 && aligned16(h), veca = A % 4 == 0 && aligned16(t) && aligned16(d_u);
#define LAUNCH_WIDE_BWD(VH, VA)                                                                                            \
  rc = isic_launch_lds<pool_wide_bwd_rows_kernel<VH, VA>, WIDE_MAX_LDS>(dim3(B), dim3(BW_NTHR), lds, as_stream(stream), h, \
                                                                        t, att, w3, offsets, H, A, heads, max_bag, d_z, d_u, d_s)
  if (vech && veca) { LAUNCH_WIDE_BWD(true, true); }
  else if (vech) { LAUNCH_WIDE_BWD(true, false); }
  else if (veca) { LAUNCH_WIDE_BWD(false, true); }
  else { LAUNCH_WIDE_BWD(false, false); }
#undef LAUNCH_WIDE_BWD
  if (rc != ISIC_OK) return rc;
  hipLaunchKernelGGL(pool_wide_dh_kernel, dim3(ceil_div(H, DH_COLS), B, DH_SPLIT), dim3(DH_COLS), 0, as_stream(stream), att,
                     offsets, H, heads, d_z, d_h, accumulate_dh);
  return isic_launch_status();
}

size_t isic_layernorm_bwd_wide_workspace_bytes(int N) {
  return N > 0 && N <= ISIC_WIDE_MAX_N ? (size_t)ISIC_WIDE_LN_MAX_BLOCKS * 2 * N * sizeof(float) : 0;
}

int isic_layernorm_bwd_wide_ws(const float* dy, const float* x, const float* gamma, const float* beta, const float* mean,
                               const float* rstd, float* dx, float* dgamma, float* dbeta, int M, int N, int relu,
                               uint32_t drop_threshold, float drop_scale, uint64_t seed, uint64_t stream_id,
                               const uint64_t* clock, void* workspace, size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(M >= 0 && N > 0);
  if (M == 0) return ISIC_OK;
  ISIC_CHECK_ARG(dy && x && gamma && beta && mean && rstd && dx && dgamma && dbeta);
  if (N > ISIC_WIDE_MAX_N) return ISIC_ERR_UNSUPPORTED;
  float* partial = (workspace && workspace_bytes >= isic_layernorm_bwd_wide_workspace_bytes(N) && aligned16(workspace))
                       ? reinterpret_cast<float*>(workspace) : nullptr;
  int grid = ceil_div(M, 2);                                       // two rows per block halve the partial rows of a short batch
  if (grid > ISIC_WIDE_LN_MAX_BLOCKS) grid = ISIC_WIDE_LN_MAX_BLOCKS;
#define LAUNCH_LN_WIDE(KERNEL)                                                                                       \
  hipLaunchKernelGGL(KERNEL, dim3(grid), dim3(256), 16 * sizeof(float), as_stream(stream), dy, x, gamma, beta, mean,  \
                     rstd, dx, dgamma, dbeta, M, N, relu, drop_threshold, drop_scale, (unsigned long long)seed,       \
                     (unsigned long long)stream_id, (const unsigned long long*)clock, partial)
  if (N % 4 == 0 && aligned16(x) && aligned16(dy) && aligned16(dx) && aligned16(gamma) && aligned16(beta)) {
    if (N <= 1024) LAUNCH_LN_WIDE(layernorm_bwd_wide_vec_kernel<1>);
    else if (N <= 2048) LAUNCH_LN_WIDE(layernorm_bwd_wide_vec_kernel<2>);
    else LAUNCH_LN_WIDE(layernorm_bwd_wide_vec_kernel<4>);
  } else {
    if (N <= 1024) LAUNCH_LN_WIDE(layernorm_bwd_wide_kernel<4>);
    else if (N <= 2048) LAUNCH_LN_WIDE(layernorm_bwd_wide_kernel<8>);
    else LAUNCH_LN_WIDE(layernorm_bwd_wide_kernel<16>);
  }
#undef LAUNCH_LN_WIDE
  if (partial) isic_ln_bwd_reduce_launch(partial, grid, N, dgamma, dbeta, as_stream(stream));
  return isic_launch_status();
}

}  // extern "C"
