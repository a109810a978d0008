// Head mean (PyG ``concat=False``) inside the attention kernels of gat.hip and edge_attn.hip.
//
// One wave owns a destination row across all heads, and lane l owns the row's elements f = l + 64 q.  The forward
// therefore sums the heads per lane: the ceil(F / 64) partial sums of a row stay in registers while F <= 64 *
// HEAD_MEAN_MAXQ (= 256: every width the models use), statically indexed so that nothing goes to scratch.  Wider rows
// fall back to a read-modify-write of the out[N,F] row by the lane that owns the element -- the same lane writes and
// re-reads an address, so program order is all the ordering it needs.  Registers first because the fallback costs the
// H - 1 extra round trips to the row that the fusion is there to avoid; a register array sized for any F would not fit.
// The destination sweep of the backward keeps row i of dout[N,F] in registers under the same bound and re-reads it per
// edge (from L1/L2, as the concat kernels do) beyond it.
#pragma once
#include "common.h"

constexpr int HEAD_MEAN_MAXQ = 4;

__device__ __forceinline__ bool head_mean_in_regs(int F) { return F <= 64 * HEAD_MEAN_MAXQ; }

// forward: sum over heads of the row's per-head aggregates, then out[i,f] = sum / H + bias[f]
struct HeadMeanRow {
  float acc[HEAD_MEAN_MAXQ] = {0.f, 0.f, 0.f, 0.f};

  // head h's aggregate `v` of the element *o = out[i, lane + 64 q]
  __device__ __forceinline__ void add(float v, float* o, int q, int h, bool in_regs) {
    if (in_regs) {
#pragma unroll
      for (int t = 0; t < HEAD_MEAN_MAXQ; ++t) acc[t] += (t == q) ? v : 0.f;
    } else {
      *o = h ? *o + v : v;
    }
  }

  __device__ __forceinline__ void finish(float* orow, const float* bias, float inv_h, int F, int lane, bool in_regs) {
    if (in_regs) {
#pragma unroll
      for (int t = 0; t < HEAD_MEAN_MAXQ; ++t) {
        const int f = lane + 64 * t;
        if (f < F) orow[f] = acc[t] * inv_h + (bias ? bias[f] : 0.f);
      }
    } else {
      for (int f = lane; f < F; f += 64) orow[f] = orow[f] * inv_h + (bias ? bias[f] : 0.f);
    }
  }
};

// backward, destination sweep: <drow, xr> per edge and head.  MEAN: drow is dout[i,:] of dout[N,F] for every head and
// the product carries the 1/H of the mean; otherwise the plain lane-strided dot product of the concat kernels.
template <bool MEAN>
struct HeadMeanDout {
  float reg[HEAD_MEAN_MAXQ];
  float inv_h;
  bool in_regs;

  __device__ __forceinline__ HeadMeanDout(const float* drow_mean, int F, int H, int lane)
      : inv_h(1.f / (float)H), in_regs(MEAN && head_mean_in_regs(F)) {
#pragma unroll
    for (int t = 0; t < HEAD_MEAN_MAXQ; ++t) {
      const int f = lane + 64 * t;
      reg[t] = (in_regs && f < F) ? drow_mean[f] : 0.f;
    }
  }

  // every lane returns the same value
  __device__ __forceinline__ float dot(const float* drow, const float* __restrict__ xr, int F, int lane) const {
    float d = 0.f;
    if (in_regs) {
#pragma unroll
      for (int t = 0; t < HEAD_MEAN_MAXQ; ++t) {
        const int f = lane + 64 * t;
        if (f < F) d += reg[t] * xr[f];
      }
    } else {
      for (int f = lane; f < F; f += 64) d += drow[f] * xr[f];
    }
    d = wave_sum(d);
    return MEAN ? d * inv_h : d;
  }
};
