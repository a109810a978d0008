// The fixed-order slab reduction: the one place that says in which order the partial sums of a split reduction meet.
//
// A split reduction (split-K GEMM, weight gradient, column sum, LayerNorm parameter gradient) never joins its blocks
// through float atomics.  Block s parks its partial result as slab s of a workspace laid out [slabs][elements], and a
// second small kernel forms  sum_s slab[s][e]  for every element e with the adds in an order that depends on `slabs`
// alone, never on timing.  That is what makes the training step bit-reproducible, and both orders are written here, once.
// T is float or f32x4 (four neighbouring elements, added component by component); every add is one IEEE fp32 add.
//
// Order A, isic_slab_sum_xor<G, T>: G neighbouring lanes share one element (G = 16, 8 or 4, lane g = threadIdx.x % G).
//   1. lane g:  v_g = 0;  v_g += slab[z]  for z = g, g + G, g + 2G, ...          (ascending z)
//   2. xor tree, for o = G/2, G/4, ..., 1:  v_g = v_g + v_(g ^ o)  in every lane at once.
//   Every lane of the group ends with the sum; lane 0 writes it.
//
// Order B, isic_slab_sum_lds16<ACC, T>: a block of 256 threads is 16 columns x 16 groups (column = threadIdx.x % 16,
//   group = threadIdx.x / 16), a column is one element.  ACC = 1, 2 or 4 accumulators a[0 .. ACC-1] per thread, all 0.
//   1. group g walks z = g, g + 16 ACC, g + 32 ACC, ... while z + 16 (ACC - 1) < slabs:  a[k] += slab[z + 16 k]  for every k.
//      tail:  the slabs z, z + 16, ... that are left (fewer than ACC of them) go to a[0], a[1], ... in turn.
//   2. pairwise join:  p_g = a[0]   |   a[0] + a[1]   |   (a[0] + a[1]) + (a[2] + a[3]).
//   3. the 16 group sums meet through LDS in group order:  t = p_0;  t += p_g  for g = 1 .. 15.
//   The threads of group 0 end with the sum.  (A sum that starts from 0 is never -0, so starting step 3 from p_0 and
//   starting it from 0 give the same bits.)
//
// Both take `live`: a thread whose element lies past the end loads nothing, but still takes part in the shuffles / the
// barrier, so the callers branch on `live` only after the call.  A kernel keeps its own epilogue (where the sum goes, beta,
// scale, bias, ...) and takes only the sum from here; share a reducer only where its adds are these adds in this order.
//
// The kernels for a plain [slabs][n] stack and their launchers live in slab_reduce.hip and are declared at the end.
// tests/slab_reduce_ref.py restates both orders in numpy; tests/test_slab_reduce_gpu.py holds the device to it bit for bit.
#pragma once
#include "common.h"

__device__ __forceinline__ float isic_slab_shfl_xor(float v, int o, int width) { return __shfl_xor(v, o, width); }
__device__ __forceinline__ f32x4 isic_slab_shfl_xor(f32x4 v, int o, int width) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = __shfl_xor(v[e], o, width);
  return r;
}

// order A.  slab0: slab 0 in units of T; i: this thread's element; stride: elements of T per slab
template <int G, typename T>
__device__ __forceinline__ T isic_slab_sum_xor(const T* __restrict__ slab0, size_t i, int slabs, size_t stride, bool live) {
  static_assert(G == 4 || G == 8 || G == 16, "G lanes per element");
  const int g = threadIdx.x % G;
  T v = {};
  if (live)
    for (int z = g; z < slabs; z += G) v += slab0[(size_t)z * stride + i];
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += isic_slab_shfl_xor(v, o, G);
  return v;
}

// order B (256 threads per block; the sum is valid where threadIdx.x < 16 && live)
template <int ACC, typename T>
__device__ __forceinline__ T isic_slab_sum_lds16(const T* __restrict__ slab0, size_t i, int slabs, size_t stride, bool live) {
  static_assert(ACC == 1 || ACC == 2 || ACC == 4, "accumulators per thread");
  __shared__ T red[16][16];
  const int q = threadIdx.x & 15, g = threadIdx.x >> 4;
  T a[ACC] = {};
  if (live) {
    const T* p = slab0 + i;
    int z = g, k = 0;
    for (; z + 16 * (ACC - 1) < slabs; z += 16 * ACC)
#pragma unroll
      for (int j = 0; j < ACC; ++j) a[j] += p[(size_t)(z + 16 * j) * stride];
    if constexpr (ACC > 1)
      for (; z < slabs; z += 16, ++k) a[k] += p[(size_t)z * stride];
  }
  T t = a[0];
  if constexpr (ACC == 2) t = a[0] + a[1];
  if constexpr (ACC == 4) t = (a[0] + a[1]) + (a[2] + a[3]);
  red[g][q] = t;
  __syncthreads();
  if (threadIdx.x < 16 && live) {
    t = red[0][q];
#pragma unroll
    for (int k = 1; k < 16; ++k) t += red[k][q];
  }
  return t;
}

// The all-taps weight gradients of conv_wgrad_c128b.hip (CO = 64, CI = 128) and conv_wgrad_s2.hip (CO = 128, CI = 64):
// dw[CO co_slice + co][tap][CI ci_slice + ci] += sum over the blocks of a (ci_slice, co_slice) pair, order B with one
// accumulator.  partial: [pairs][blocks_per_pair][CO][9][CI]; grid = pairs * CO * 9 * CI / 64 blocks, exactly.
template <int CO, int CI>
__global__ __launch_bounds__(256) void wgrad_pair_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dw,
                                                                 int blocks_per_pair, int co_slices, int Cin) {
  constexpr int SLICE4 = CO * 9 * CI / 4;
  const size_t e4 = (size_t)blockIdx.x * 16 + (threadIdx.x & 15);  // float4 index into [pairs][CO][9][CI]
  const int pair = (int)(e4 / SLICE4);
  const size_t l4 = e4 - (size_t)pair * SLICE4;                    // ... inside the pair: (co * 9 + tap) * (CI / 4) + ci / 4
  const f32x4* base = reinterpret_cast<const f32x4*>(partial) + (size_t)pair * blocks_per_pair * SLICE4;
  const f32x4 t = isic_slab_sum_lds16<1>(base, l4, blocks_per_pair, (size_t)SLICE4, true);
  if (threadIdx.x < 16) {
    const int ci_slice = pair / co_slices, co_slice = pair - ci_slice * co_slices;
    const int row = (int)(l4 / (CI / 4)), ci4 = (int)(l4 % (CI / 4));   // row = co * 9 + tap
    f32x4* out = reinterpret_cast<f32x4*>(dw + ((size_t)co_slice * CO * 9 + row) * Cin + ci_slice * CI) + ci4;
    *out = *out + t;
  }
}

// ---- slab_reduce.hip: out[i] = beta * out[i] + sum over the slabs of partial[slabs][n].  beta == 0 never reads out;
// beta == 1 is the exact `+=` of the weight gradients.
enum IsicSlabForm {
  ISIC_SLAB_XOR16 = 0,     // order A, G = 16, scalar
  ISIC_SLAB_XOR4 = 1,      // order A, G = 4, scalar: few slabs (<= 32), four times the elements per block
  ISIC_SLAB_LDS16_V1 = 2,  // order B on f32x4, one accumulator   (n % 4 == 0, 16-byte aligned pointers)
  ISIC_SLAB_LDS16_V2 = 3,  // order B on f32x4, two accumulators  (likewise)
};
void isic_slab_reduce_launch(IsicSlabForm form, const float* partial, int slabs, int64_t n, float* out, float beta,
                             hipStream_t stream);
// C[M,N] with rows ldc apart = beta * C + sum over the splits of partial[splits][M][N]: ISIC_SLAB_LDS16_V1 where N, ldc and
// the pointers allow 16-byte accesses, ISIC_SLAB_XOR16 otherwise
void isic_gemm_split_reduce_launch(const float* partial, int splits, float* C, int M, int N, int ldc, float beta,
                                   hipStream_t stream);
// ---- rowwise.hip: dgamma[n] += sum over the blocks of partial[nblocks][2][N] (row 0; row 1: dbeta) (ln_bwd_reduce_kernel:
// order A, G = 16), for every LayerNorm backward kernel that parks [2][N] partial rows
void isic_ln_bwd_reduce_launch(const float* partial, int nblocks, int N, float* dgamma, float* dbeta, hipStream_t stream);
