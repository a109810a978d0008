// Workgroup primitives of the one-workgroup-per-graph kernels over ragged record sets (ragged_graph.hip, hetero_ragged.hip):
// 256 threads walk a graph's nodes or edges in chunks of 256.  Needs common.h.
#pragma once

constexpr int RG_BLOCK = 256;                              // threads per workgroup = edges / flags per scan chunk
constexpr int RG_WAVES = RG_BLOCK / ISIC_WAVE;

// Exclusive prefix of a flag over the block's 256 threads in thread order: wave ballot + popcount below the lane, the four
// wave totals through LDS.  Block-uniform call sites only (two barriers).
__device__ __forceinline__ int rg_block_scan(bool flag, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(flag);
  const int below = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __popcll(bal);
  __syncthreads();
  int wbase = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < RG_WAVES; ++w) {
    const int c = wsum[w];
    wbase += w < wave ? c : 0;
    total += c;
  }
  __syncthreads();                                         // wsum is free for the next chunk
  return wbase + below;
}

__device__ __forceinline__ unsigned rg_block_sum(unsigned v, unsigned* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned s = 0;
#pragma unroll
  for (int w = 0; w < RG_WAVES; ++w) s += red[w];
  __syncthreads();
  return s;
}
