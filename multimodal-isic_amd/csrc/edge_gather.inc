// The row gather of one edge by one wave, shared by edge_hetero_kernel (hetero.hip) and edge_hetero_ragged_kernel
// (hetero_ragged.hip) so that both give the same bits: sum_i (xs[i] - xd[i])^2 over D floats (16-byte loads when D % 4 == 0)
// and sum_c ps[c] * log((ps[c] + eps) / (pd[c] + eps)) over C classes, both reduced across the 64 lanes (every lane returns
// the sums).  Wave-uniform call sites only.  Needs common.h.
#pragma once

__device__ __forceinline__ void edge_row_sums(const float* __restrict__ xs, const float* __restrict__ xd,
                                              const float* __restrict__ ps, const float* __restrict__ pd, int D, int C,
                                              float eps, int lane, float& sqdiff, float& kl_out) {
  float acc = 0.f;
  if ((D & 3) == 0) {
    for (int i = lane * 4; i < D; i += 256) {
      const float4 a = *reinterpret_cast<const float4*>(xs + i);
      const float4 b = *reinterpret_cast<const float4*>(xd + i);
      const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
      acc += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  } else {
    for (int i = lane; i < D; i += 64) {
      const float df = xs[i] - xd[i];
      acc += df * df;
    }
  }
  float kl = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float p = ps[c], q = pd[c];
    kl += p * logf((p + eps) / (q + eps));
  }
  sqdiff = wave_sum(acc);
  kl_out = wave_sum(kl);
}

// Euclidean distance of lattice positions a and b on a grid_w-wide lattice (04:124-125,166)
__device__ __forceinline__ float lattice_distance(int a, int b, int grid_w) {
  const float dx = (float)(a % grid_w - b % grid_w), dy = (float)(a / grid_w - b / grid_w);
  return sqrtf(dx * dx + dy * dy);
}
