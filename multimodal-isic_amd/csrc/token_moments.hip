// Per-image statistics of a token grid over its token axis (include/isic_hip_moments.h): mean, max, std, median, skewness
// and excess kurtosis of X[b, 0:T, d] for every (b, d), in one launch.  Replaces the eight or so torch passes (one of them a
// full sort per column) of the reference's concat_patch_moments (utils.py:16-31).
//
//   * Tile.  Block (b, slab) stages X[b, 0:T, slab] into LDS as [T][W] floats, W = 64 / 32 / 16 by T so that the tile is
//     at most 64 KiB.  Thread (g, c) = (tid / W, tid % W) owns channel c of the slab and the tokens g, g + G, ... with
//     G = 256 / W.  A wave reads 64 consecutive floats of the tile per instruction (one row at W = 64, two at 32, four at
//     16): no bank conflict.  Channels past D are staged as zeros and never written out.
//   * Moments.  Every thread adds its tokens in ascending order; the G partials of a channel are parked in LDS and EVERY
//     thread of the channel adds them in ascending g, so all of them hold the same bits without a broadcast.  Sum and max
//     first; with the mean known, sum c^2, sum c^3, sum c^4 in a second walk over the tile.
//   * Median.  Each thread turns its own tile elements into KEYS in place (unsigned order == IEEE order of finite fp32: a
//     negative pattern is complemented, a positive one gets its sign bit set).  The key of rank k = (T - 1) / 2 is found four
//     bits per pass from the top: the threads of a channel add their candidates (keys that agree with the decided prefix)
//     into the channel's 16 bins by the next digit (integer LDS adds, two 16-bit bins per word: the order cannot change a
//     count); every thread of the channel then walks the bins upwards, the digit is the bin in which the running count
//     passes k, and k drops by the count below it.  Equal keys stay candidates together, so any number of ties is exact.
//     The walk stops once every channel of the block has a single candidate (or after the last digit); the candidates' key
//     is then the median.  The bins live in the words the moment partials used.
#include "common.h"
#include "../../include/isic_hip_moments.h"

#include <limits.h>

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_TILE_BYTES = 65536;

struct MomentsArgs {
  const float* X;
  float* out;
  int64_t ldx, ldo;
  int T, D, slabs, vec;
  float eps;
  int unbiased;
};

__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

template <int W>
__global__ __launch_bounds__(BLOCK) void token_moments_kernel(MomentsArgs a) {
  constexpr int G = BLOCK / W;                 // threads per channel
  constexpr int W4 = W / 4;
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [T][W]
  __shared__ float part[3][BLOCK];             // [.][g * W + c]
  __shared__ unsigned med[W];
  const int tid = threadIdx.x, c = tid % W, g = tid / W;
  const int T = a.T, D = a.D;
  const int64_t b = blockIdx.x / a.slabs;
  const int d0 = (int)(blockIdx.x % a.slabs) * W;
  const float* xb = a.X + b * T * a.ldx + d0;

  // ---- stage the slab: X is read here and nowhere else
  if (a.vec) {
#pragma unroll 4
    for (int e = tid; e < T * W4; e += BLOCK) {
      const int t = e / W4, q = (e % W4) * 4;
      const float* src = xb + (int64_t)t * a.ldx + q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (d0 + q + 3 < D) {
        v = *reinterpret_cast<const f32x4*>(src);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (d0 + q + i < D) v[i] = src[i];
      }
      *reinterpret_cast<f32x4*>(&tile[t * W + q]) = v;
    }
  } else {
#pragma unroll 4
    for (int e = tid; e < T * W; e += BLOCK) {
      const int t = e / W, q = e % W;
      tile[e] = (d0 + q < D) ? xb[(int64_t)t * a.ldx + q] : 0.f;
    }
  }
  __syncthreads();

  float* col = tile + c;
  // ---- sum and max
  float s = 0.f, mx = -INFINITY;
#pragma unroll 8
  for (int t = g; t < T; t += G) {
    const float v = col[t * W];
    s += v;
    mx = fmaxf(mx, v);
  }
  part[0][tid] = s;
  part[1][tid] = mx;
  __syncthreads();
  s = part[0][c];
  mx = part[1][c];
#pragma unroll
  for (int j = 1; j < G; ++j) {
    s += part[0][j * W + c];
    mx = fmaxf(mx, part[1][j * W + c]);
  }
  const float mean = s / (float)T;
  __syncthreads();                             // part[] is written again below

  // ---- central power sums; the thread's elements become keys on the way
  float s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll 8
  for (int t = g; t < T; t += G) {
    const float v = col[t * W];
    const float cv = v - mean, c2 = cv * cv;
    s2 += c2;
    s3 += c2 * cv;
    s4 += c2 * c2;
    col[t * W] = __uint_as_float(key_of(v));   // only this thread reads or writes the element until the last scan
  }
  part[0][tid] = s2;
  part[1][tid] = s3;
  part[2][tid] = s4;
  __syncthreads();
  s2 = part[0][c];
  s3 = part[1][c];
  s4 = part[2][c];
#pragma unroll
  for (int j = 1; j < G; ++j) {
    s2 += part[0][j * W + c];
    s3 += part[1][j * W + c];
    s4 += part[2][j * W + c];
  }

  // ---- median: the key of rank k, one 4-bit digit per pass
  unsigned* hist = reinterpret_cast<unsigned*>(&part[0][0]);   // [8][W] words, two 16-bit bins each (a count is <= T <= 1024)
  const unsigned* kcol = reinterpret_cast<const unsigned*>(col);
  unsigned prefix = 0u, mask = 0u;
  int k = (T - 1) / 2, ncand = T;
  for (int shift = 28; shift >= 0; shift -= 4) {
    // (the barrier also separates the reads of part[] above and of hist[] in the previous pass from the zeroing below)
    if (!__syncthreads_or(ncand > 1)) break;
    for (int i = tid; i < 8 * W; i += BLOCK) hist[i] = 0u;
    __syncthreads();
#pragma unroll 8
    for (int t = g; t < T; t += G) {
      const unsigned key = kcol[t * W];
      if ((key & mask) == prefix) {
        const unsigned d = (key >> shift) & 15u;
        atomicAdd(&hist[(d >> 1) * W + c], 1u << ((d & 1u) * 16u));   // integer: the order cannot change the counts
      }
    }
    __syncthreads();
    int below = 0, digit = 0, count = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned w = hist[j * W + c];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int n = (int)((w >> (16 * h)) & 0xFFFFu);
        if (!found) {
          if (k < below + n) {
            found = true;
            digit = 2 * j + h;
            count = n;
          } else {
            below += n;
          }
        }
      }
    }
    k -= below;                                // (k < ncand always holds, so a digit is found)
    ncand = count;
    prefix |= (unsigned)digit << shift;
    mask |= 15u << shift;
  }
  // the candidates all hold one key (a single one is left, or every bit is decided): whoever owns one publishes it
#pragma unroll 8
  for (int t = g; t < T; t += G) {
    const unsigned key = kcol[t * W];
    if ((key & mask) == prefix) med[c] = key;
  }
  __syncthreads();

  if (g == 0 && d0 + c < D) {
    const float var = s2 / (float)(T - a.unbiased);
    const float sd = sqrtf(var);
    const float sigma = fmaxf(sd, a.eps);
    const float sg2 = sigma * sigma;
    const float n = (float)T;
    float* o = a.out + b * a.ldo + d0 + c;
    o[0] = mean;
    o[(int64_t)D] = mx;
    o[(int64_t)2 * D] = sd;
    o[(int64_t)3 * D] = value_of(med[c]);
    o[(int64_t)4 * D] = (s3 / n) / (sg2 * sigma);
    o[(int64_t)5 * D] = (s4 / n) / (sg2 * sg2) - 3.f;
  }
}

int slab_width(int T) { return T <= 256 ? 64 : (T <= 512 ? 32 : 16); }

template <int W>
int launch_moments(const MomentsArgs& a, int64_t blocks, hipStream_t st) {
  static IsicPerDeviceOnce once;              // hipFuncSetAttribute is per device (one flag set per template instance)
  if (isic_once_per_device(once, [] {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(token_moments_kernel<W>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, MAX_TILE_BYTES);
      }) != hipSuccess)
    return ISIC_ERR_LAUNCH;
  const size_t lds = (size_t)a.T * W * sizeof(float);
  hipLaunchKernelGGL(token_moments_kernel<W>, dim3((unsigned)blocks), dim3(BLOCK), lds, st, a);
  return isic_launch_status();
}

}  // namespace

extern "C" {

int isic_token_moments_f32(const float* X, int64_t B, int T, int D, int64_t ldx, float eps, int unbiased, float* out,
                           int64_t ldo, void* stream) {
  ISIC_CHECK_ARG(B >= 0 && T >= 1 && D >= 1 && ldx >= D && ldo >= (int64_t)6 * D);
  ISIC_CHECK_ARG(eps >= 0.f);                  // false for a NaN as well
  ISIC_CHECK_ARG((unbiased == 0 || unbiased == 1) && !(unbiased && T < 2));
  ISIC_CHECK_ARG((X && out) || B == 0);
  if (T > ISIC_MOMENTS_MAX_T) return ISIC_ERR_UNSUPPORTED;
  const int W = slab_width(T);
  const int slabs = ceil_div(D, W);
  if (B > (int64_t)INT_MAX / slabs) return ISIC_ERR_UNSUPPORTED;
  if (B == 0) return ISIC_OK;
  MomentsArgs a;
  a.X = X; a.out = out; a.ldx = ldx; a.ldo = ldo; a.T = T; a.D = D; a.slabs = slabs;
  a.vec = (ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0) ? 1 : 0;
  a.eps = eps; a.unbiased = unbiased;
  const int64_t blocks = B * slabs;
  hipStream_t st = as_stream(stream);
  switch (W) {
    case 64: return launch_moments<64>(a, blocks, st);
    case 32: return launch_moments<32>(a, blocks, st);
    default: return launch_moments<16>(a, blocks, st);
  }
}

}  // extern "C"
