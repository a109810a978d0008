// The gate of gated attention pooling (include/isic_hip_gated.h): t = tanh(h V^T + b_V) * sigmoid(h U^T + b_U), forward and
// backward, as two streaming passes around the attention-pool kernels, which take t as an input and stay as they are.
//
// p [T, 2 nA] = tanh-branch columns | gate columns (one GEMM over the stacked operand).  Both kernels are HBM-bound and hold
// no tile: a thread owns V = 4 neighbouring columns of one half (16-byte accesses; V = 1 where nA % 4 != 0 or a pointer is
// not 16-byte aligned) and reads the same columns of the other half nA floats further on.
//   forward:  2 reads + 3 writes of V floats per thread and row        (20 nA bytes per row)
//   backward: 2 reads + 2 writes of V floats per thread and row, heads floats of d_s (cache hits)  (16 nA bytes per row);
//             the column sums stay in registers over the rows of a chunk and leave as one slab row per chunk.
#include "slab_sum.inc"

#include "../../include/isic_hip_gated.h"

namespace {

// The sibling of isic_tanhf (common.h).  exp(-x) = 0 for large x: 1 / 1 = 1 exactly; exp(-x) = inf for large -x (from
// x < -88.8 on): 1 / inf = 0 exactly; x = +-inf likewise: no NaN.
__device__ __forceinline__ float isic_sigmoidf(float x) { return 1.f / (1.f + __expf(-x)); }

template <int V>
struct GateVec {
  float v[V];
};
template <int V>
__device__ __forceinline__ GateVec<V> gate_load(const float* q) {
  GateVec<V> r;
  if constexpr (V == 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(q);
#pragma unroll
    for (int e = 0; e < 4; ++e) r.v[e] = x[e];
  } else {
    r.v[0] = *q;
  }
  return r;
}
template <int V>
__device__ __forceinline__ void gate_store(float* q, const GateVec<V>& r) {
  if constexpr (V == 4) {
    const f32x4 x = {r.v[0], r.v[1], r.v[2], r.v[3]};
    *reinterpret_cast<f32x4*>(q) = x;
  } else {
    *q = r.v[0];
  }
}

// Element i of [T][nAv] (nAv = nA / V column groups per half): row i / nAv, group i % nAv.  Grid-stride; the (row, group)
// pair is advanced by the stride's own quotient and remainder, so the loop holds no division.
template <int V>
__global__ __launch_bounds__(256) void gate_fwd_kernel(float* __restrict__ p, float* __restrict__ t, int T, int nAv) {
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  const int nA = nAv * V, step_rows = (int)(step / nAv), step_cols = (int)(step % nAv);
  int64_t row = first / nAv;
  int c = (int)(first % nAv);
  for (; row < T; row += step_rows, c += step_cols) {
    if (c >= nAv) {
      c -= nAv;
      if (++row >= T) break;
    }
    float* pv = p + (row * 2 * nA + (int64_t)c * V);
    GateVec<V> x = gate_load<V>(pv), g = gate_load<V>(pv + nA), o;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      x.v[e] = isic_tanhf(x.v[e]);
      g.v[e] = isic_sigmoidf(g.v[e]);
      o.v[e] = x.v[e] * g.v[e];
    }
    gate_store<V>(pv, x);
    gate_store<V>(pv + nA, g);
    gate_store<V>(t + (row * nA + (int64_t)c * V), o);
  }
}

// Thread (chunk s, column group c): rows s, s + S, s + 2 S, ... in ascending order, one accumulator per sum and column.
// Neighbouring threads hold neighbouring column groups and then the next chunk = the next row: every wave reads whole
// runs of a row, and with few columns runs of neighbouring rows.  d_b3[k] is kept by the thread that owns the first
// column of head k.  slab: [S][3 nA + heads] = sum d_v | sum d_g | sum d_s t | sum d_s.
template <int V>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ d_s, const float* __restrict__ w3,
                                                        const float* __restrict__ a, int T, int heads, int A, int nAv, int S,
                                                        float* __restrict__ d_p, float* __restrict__ slab) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)S * nAv) return;
  const int s = (int)(g / nAv), col = (int)(g % nAv) * V, nA = nAv * V;
  int k[V];
  float w[V];
  bool head_first[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    k[e] = (col + e) / A;
    head_first[e] = col + e == k[e] * A;
    w[e] = w3[col + e];                                             // w3 [heads, A] is nA floats in column order
  }
  float sv[V] = {}, sg_[V] = {}, sw[V] = {}, sb[V] = {};
  for (int r = s; r < T; r += S) {
    const float* ar = a + ((int64_t)r * 2 * nA + col);
    const GateVec<V> tv = gate_load<V>(ar), sg = gate_load<V>(ar + nA);
    const float* ds = d_s + (int64_t)r * heads;
    float dsv[V];
    dsv[0] = ds[k[0]];
#pragma unroll
    for (int e = 1; e < V; ++e) dsv[e] = k[e] == k[e - 1] ? dsv[e - 1] : ds[k[e]];
    GateVec<V> dv, dg;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float dt = dsv[e] * w[e];
      dv.v[e] = dt * sg.v[e] * (1.f - tv.v[e] * tv.v[e]);
      dg.v[e] = dt * tv.v[e] * sg.v[e] * (1.f - sg.v[e]);
      sv[e] += dv.v[e];
      sg_[e] += dg.v[e];
      sw[e] += dsv[e] * (tv.v[e] * sg.v[e]);
      sb[e] += head_first[e] ? dsv[e] : 0.f;
    }
    float* dr = d_p + ((int64_t)r * 2 * nA + col);
    gate_store<V>(dr, dv);
    gate_store<V>(dr + nA, dg);
  }
  float* out = slab + (size_t)s * (3 * (size_t)nA + heads);
#pragma unroll
  for (int e = 0; e < V; ++e) {
    out[col + e] = sv[e];
    out[nA + col + e] = sg_[e];
    out[2 * nA + col + e] = sw[e];
    if (head_first[e]) out[3 * (size_t)nA + k[e]] = sb[e];
  }
}

// The slabs meet in order A of slab_sum.inc (16 lanes per element); the epilogue sends element i to its gradient:
// [0, 2 nA) d_bias, [2 nA, 3 nA) d_w3, [3 nA, 3 nA + heads) d_b3, each  out = beta * out + sum.
__global__ __launch_bounds__(256) void gate_bwd_reduce_kernel(const float* __restrict__ slab, int S, int nA, int heads,
                                                               float* __restrict__ d_bias, float* __restrict__ d_w3,
                                                               float* __restrict__ d_b3, float beta) {
  const int n = 3 * nA + heads, i = blockIdx.x * 16 + threadIdx.x / 16;
  const float sum = isic_slab_sum_xor<16>(slab, (size_t)i, S, (size_t)n, i < n);
  if (i < n && threadIdx.x % 16 == 0) {
    float* o = i < 2 * nA ? d_bias + i : i < 3 * nA ? d_w3 + (i - 2 * nA) : d_b3 + (i - 3 * nA);
    *o = beta != 0.f ? beta * (*o) + sum : sum;
  }
}

// row chunks of the backward: a function of T alone
int gate_chunks(int T) { return T <= 16 ? 1 : T >= 16 * 2048 ? 2048 : ceil_div(T, 16); }

bool gate_dims_ok(int T, int heads, int A) {
  return T >= 0 && heads >= 1 && A >= 1 && (int64_t)heads * A <= ISIC_GATE_MAX_NA;
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

}  // namespace

int isic_gate_fwd_f32(float* p, int T, int heads, int A, float* t, void* stream) {
  ISIC_CHECK_ARG(gate_dims_ok(T, heads, A));
  if (T == 0) return ISIC_OK;
  ISIC_CHECK_ARG(p && t);
  const int nA = heads * A;
  const bool vec = nA % 4 == 0 && aligned16(p) && aligned16(t);
  const int nAv = vec ? nA / 4 : nA;
  const int64_t blocks = ceil_div64((int64_t)T * nAv, 256);
  const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));       // 8 blocks per CU, the rest by grid stride
  if (vec) hipLaunchKernelGGL(gate_fwd_kernel<4>, grid, dim3(256), 0, as_stream(stream), p, t, T, nAv);
  else hipLaunchKernelGGL(gate_fwd_kernel<1>, grid, dim3(256), 0, as_stream(stream), p, t, T, nAv);
  return isic_launch_status();
}

size_t isic_gate_bwd_f32_workspace_bytes(int T, int heads, int A) {
  if (!gate_dims_ok(T, heads, A) || T == 0) return 0;
  return (size_t)gate_chunks(T) * (3 * (size_t)heads * A + heads) * sizeof(float);
}

int isic_gate_bwd_f32(const float* d_s, const float* w3, const float* a, int T, int heads, int A, float* d_p,
                      float* d_bias, float* d_w3, float* d_b3, float beta, void* workspace, size_t workspace_bytes,
                      void* stream) {
  ISIC_CHECK_ARG(gate_dims_ok(T, heads, A) && (beta == 0.f || beta == 1.f));
  if (T == 0) return ISIC_OK;
  ISIC_CHECK_ARG(d_s && w3 && a && d_p && d_bias && d_w3 && d_b3 && d_p != a);
  if (!workspace || workspace_bytes < isic_gate_bwd_f32_workspace_bytes(T, heads, A) || !aligned16(workspace))
    return ISIC_ERR_WORKSPACE;
  const int nA = heads * A, S = gate_chunks(T);
  float* slab = reinterpret_cast<float*>(workspace);
  const bool vec = nA % 4 == 0 && aligned16(a) && aligned16(d_p);
  const int nAv = vec ? nA / 4 : nA;
  const dim3 grid((unsigned)ceil_div64((int64_t)S * nAv, 256));
  if (vec)
    hipLaunchKernelGGL(gate_bwd_kernel<4>, grid, dim3(256), 0, as_stream(stream), d_s, w3, a, T, heads, A, nAv, S, d_p, slab);
  else
    hipLaunchKernelGGL(gate_bwd_kernel<1>, grid, dim3(256), 0, as_stream(stream), d_s, w3, a, T, heads, A, nAv, S, d_p, slab);
  hipLaunchKernelGGL(gate_bwd_reduce_kernel, dim3((unsigned)ceil_div(3 * nA + heads, 16)), dim3(256), 0, as_stream(stream),
                     slab, S, nA, heads, d_bias, d_w3, d_b3, beta);
  return isic_launch_status();
}
