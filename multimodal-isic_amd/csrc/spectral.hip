// Spectral and summary statistics of the heterophily stage (04_measure_heterophily.py:149-159, :172-181), gfx950.
//
// isic_laplacian_lambda2_f64: lambda_2 (second-smallest eigenvalue) of L = I - D^-1/2 max(A, A^T) D^-1/2 per graph, one
// workgroup per graph, everything in LDS:
//   1. counts   A is the packed lower triangle of the n x n matrix in fp64 (slot (i, j), i >= j, at i(i+1)/2 + j:
//               196 * 197 / 2 * 8 B = 154 448 B at the patch-grid size).  While edges are counted a slot is two uint32
//               counters, c_ij in the low word and c_ji in the high word (LDS atomics), so duplicated edges count with
//               their multiplicity (scipy's COO -> CSR sums them, :151-152); self loops are skipped (:117-118).  Each
//               slot then becomes (double)max(c_ij, c_ji) in place (:153, element-wise max, not sum, not OR).
//   2. scale    deg_i = row sums, d^-1/2 = 0 for an isolated node (:154-156), slot (i, j) <- -d_i^-1/2 a_ij d_j^-1/2,
//               diagonal <- 1.
//   3. reduce   Householder tridiagonalisation in place, LAPACK's DSYTD2 (lower) one column at a time: v from column k
//               (wave 0), p = tau * A22 v (a wave per row: the row's own slots j <= i and its column below the diagonal,
//               no cross-wave sums), A22 -= v w^T + w v^T with w = p - tau/2 (p.v) v (a wave per row, lanes along it).
//               The diagonal d and subdiagonal e stay in the diagonal / first subdiagonal slots.
//   4. bisect   Sturm counts of the tridiagonal with dstebz's pivmin guard, multisection: each of the 512 threads
//               counts at one shift per round, the interval containing the 2nd eigenvalue shrinks 513-fold per round,
//               ~6 rounds to fp64 resolution on the Gershgorin interval.
// All sums run in a fixed order: the result is bit-identical from run to run.
//
// isic_laplacian_lambda2_ragged_f64 (include/isic_hip_hetero_ragged.h): the same device function per graph, with the node
// count of every graph taken from node_offsets, LOCAL ids and the LDS sized by a host-known max_nodes.
//
// isic_segment_stats_f32: mean / population std / median of values[m][e0:e1) per (measure m, segment g), one workgroup
// per pair: fp64 sums, bitonic sort of the segment in LDS (fp32 keys, padded with +inf to a power of two).
#include <float.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int SP_THREADS = 512;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SEG_THREADS = 512;
constexpr int SEG_WAVES = SEG_THREADS / 64;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ int tri(int i) { return i * (i + 1) / 2; }   // first slot of packed row i

// LDS layout (dynamic, sized by n): [slots: n(n+1)/2 doubles][vec0: n doubles][vec1: n doubles][scal: 8 doubles]
__host__ __device__ constexpr size_t lambda2_lds_bytes(int n) {
  return ((size_t)n * (n + 1) / 2 + 2 * (size_t)n + 8) * sizeof(double);
}
constexpr int SP_MAX_LDS = (int)lambda2_lds_bytes(ISIC_SPECTRAL_MAX_NODES);

// lambda_2 of the graph with n nodes whose edges are src/dst[e0:e1) with node ids id_base .. id_base + n - 1, by the whole
// workgroup, into *out; `sm` is the dynamic LDS (lambda2_lds_bytes(n) at least).  e0 <= e1 are valid positions (the callers
// check the offsets); n <= 1 gives 0.0, an id outside the graph NaN.  Block-uniform call sites only.
__device__ __forceinline__ void laplacian_lambda2_graph(double* sm, const int64_t* __restrict__ src,
                                                        const int64_t* __restrict__ dst, int64_t e0, int64_t e1, int n,
                                                        int64_t id_base, double* __restrict__ out) {
  const int T = n * (n + 1) / 2;
  double* Ap = sm;                       // packed lower triangle
  double* vec0 = sm + T;                 // d^-1/2, then the Householder vector v, then the diagonal d
  double* vec1 = vec0 + n;               // p = tau A v, then e^2
  double* scal = vec1 + n;               // [0..1] tau (by column parity)  [2] lo  [3] hi  [4] pivmin  [5] tnorm  [6] ints
  int* flag = reinterpret_cast<int*>(scal + 6);   // flag[0] bad input, flag[1] multisection winner
  unsigned int* cnt = reinterpret_cast<unsigned int*>(sm);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int s = tid; s < T; s += SP_THREADS) Ap[s] = 0.0;
  if (tid == 0) flag[0] = 0;
  __syncthreads();

  // ---- 1. directed multiplicities
  int bad = 0;
  for (int64_t e = e0 + tid; e < e1; e += SP_THREADS) {
    const int64_t s = src[e] - id_base, t = dst[e] - id_base;
    if (s < 0 || s >= n || t < 0 || t >= n) {
      bad = 1;
      continue;
    }
    if (s == t) continue;
    const int i = (int)(s > t ? s : t), j = (int)(s > t ? t : s);
    atomicAdd(&cnt[2 * (tri(i) + j) + (s > t ? 0 : 1)], 1u);
  }
  if (bad) atomicOr(&flag[0], 1);
  __syncthreads();
  if (flag[0]) {
    if (tid == 0) *out = __builtin_nan("");
    return;
  }
  if (n <= 1) {
    if (tid == 0) *out = 0.0;
    return;
  }
  // counters -> symmetric weight max(c_ij, c_ji) in place (each slot read and written by one lane)
  for (int i = wave; i < n; i += SP_WAVES)
    for (int j = lane; j <= i; j += 64) {
      const int s = tri(i) + j;
      const unsigned int lo = cnt[2 * s], hi = cnt[2 * s + 1];
      Ap[s] = (double)(lo > hi ? lo : hi);
    }
  __syncthreads();

  // ---- 2. degrees (row i = its own slots j < i plus column i below the diagonal) and scaling
  for (int i = wave; i < n; i += SP_WAVES) {
    double acc = 0.0;
    for (int j = lane; j < n; j += 64) acc += j <= i ? Ap[tri(i) + j] : Ap[tri(j) + i];
    acc = wave_sum_f64(acc);
    if (lane == 0) vec0[i] = acc > 0.0 ? 1.0 / sqrt(acc) : 0.0;
  }
  __syncthreads();
  for (int i = wave; i < n; i += SP_WAVES) {
    const double di = vec0[i];
    for (int j = lane; j <= i; j += 64) {
      const int s = tri(i) + j;
      Ap[s] = j == i ? 1.0 : -(di * Ap[s] * vec0[j]);
    }
  }
  __syncthreads();

  // ---- 3. Householder tridiagonalisation (DSYTD2, lower): columns 0 .. n-3
  for (int k = 0; k < n - 2; ++k) {
    const int o = k + 1, m = n - o;
    if (wave == 0) {
      const double alpha = Ap[tri(o) + k];
      double xn2 = 0.0;
      for (int r = 1 + lane; r < m; r += 64) {
        const double x = Ap[tri(o + r) + k];
        xn2 += x * x;
      }
      xn2 = wave_sum_f64(xn2);
      double tau = 0.0;
      if (xn2 > 0.0) {
        const double beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
        tau = (beta - alpha) / beta;
        const double sc = 1.0 / (alpha - beta);
        for (int r = lane; r < m; r += 64) vec0[r] = r == 0 ? 1.0 : Ap[tri(o + r) + k] * sc;
        if (lane == 0) Ap[tri(o) + k] = beta;             // e_k
      }
      if (lane == 0) scal[k & 1] = tau;
    }
    __syncthreads();
    // H = I: column k is already reduced (uniform branch, no closing barrier: the parity slot keeps the next column's
    // tau from overwriting this one before every wave has read it)
    const double tau = scal[k & 1];
    if (tau == 0.0) continue;
    // p_i = tau * sum_j A22[i][j] v_j
    for (int i = wave; i < m; i += SP_WAVES) {
      const int gi = o + i;
      double acc = 0.0;
      for (int j = lane; j < m; j += 64) acc += (j <= i ? Ap[tri(gi) + o + j] : Ap[tri(o + j) + gi]) * vec0[j];
      acc = wave_sum_f64(acc);
      if (lane == 0) vec1[i] = tau * acc;
    }
    __syncthreads();
    // alpha2 = -tau/2 (p.v), computed by every wave in the same order
    double pv = 0.0;
    for (int j = lane; j < m; j += 64) pv += vec1[j] * vec0[j];
    const double a2 = -0.5 * tau * wave_sum_f64(pv);
    for (int i = wave; i < m; i += SP_WAVES) {
      const double vi = vec0[i], wi = vec1[i] + a2 * vi;
      double* row = Ap + tri(o + i) + o;
      for (int j = lane; j <= i; j += 64) {
        const double vj = vec0[j], wj = vec1[j] + a2 * vj;
        row[j] -= vi * wj + wi * vj;
      }
    }
    __syncthreads();
  }

  // ---- 4. tridiagonal (d, e^2), Gershgorin interval, multisection on the Sturm count
  for (int i = tid; i < n; i += SP_THREADS) {
    vec0[i] = Ap[tri(i) + i];
    if (i + 1 < n) {
      const double e = Ap[tri(i + 1) + i];
      vec1[i] = e * e;
    }
  }
  if (wave == 0) {
    double gl = DBL_MAX, gu = -DBL_MAX, e2max = 0.0;
    for (int i = lane; i < n; i += 64) {
      const double el = i > 0 ? fabs(Ap[tri(i) + i - 1]) : 0.0, er = i + 1 < n ? fabs(Ap[tri(i + 1) + i]) : 0.0;
      const double d = Ap[tri(i) + i];
      gl = fmin(gl, d - el - er);
      gu = fmax(gu, d + el + er);
      e2max = fmax(e2max, er * er);
    }
    gl = wave_min_f64(gl);
    gu = wave_max_f64(gu);
    e2max = wave_max_f64(e2max);
    if (lane == 0) {
      const double pivmin = DBL_MIN * fmax(1.0, e2max);
      const double tnorm = fmax(fabs(gl), fabs(gu));
      const double pad = 2.0 * n * DBL_EPSILON * tnorm + 2.0 * pivmin;
      scal[2] = gl - pad;
      scal[3] = gu + pad;
      scal[4] = pivmin;
      scal[5] = tnorm;
    }
  }
  __syncthreads();
  const double pivmin = scal[4], tnorm = scal[5];
  for (int round = 0; round < 32; ++round) {
    const double lo = scal[2], hi = scal[3];
    if (!(hi - lo > 2.0 * DBL_EPSILON * fmax(fabs(lo), fabs(hi)) + DBL_EPSILON * tnorm)) break;
    const double x = lo + (hi - lo) * ((double)(tid + 1) / (double)(SP_THREADS + 1));
    // number of eigenvalues <= x (dstebz / dlaebz recurrence)
    double q = vec0[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int c = q <= 0.0;
    for (int i = 1; i < n; ++i) {
      q = vec0[i] - vec1[i - 1] / q - x;
      if (fabs(q) < pivmin) q = -pivmin;
      c += q <= 0.0;
    }
    if (tid == 0) flag[1] = SP_THREADS;
    __syncthreads();
    if (c >= 2) atomicMin(&flag[1], tid);
    __syncthreads();
    const int best = flag[1];
    if (tid == 0) {
      const double step = hi - lo;
      if (best > 0) scal[2] = lo + step * ((double)best / (double)(SP_THREADS + 1));
      if (best < SP_THREADS) scal[3] = lo + step * ((double)(best + 1) / (double)(SP_THREADS + 1));
    }
    __syncthreads();
  }
  if (tid == 0) *out = 0.5 * (scal[2] + scal[3]);
}

__global__ __launch_bounds__(SP_THREADS) void laplacian_lambda2_kernel(const int64_t* __restrict__ src,
                                                                       const int64_t* __restrict__ dst,
                                                                       const int64_t* __restrict__ edge_offsets, int n,
                                                                       double* __restrict__ lambda2) {
  extern __shared__ double sm[];
  const int64_t g = blockIdx.x;
  const int64_t e0 = edge_offsets[g], e1 = edge_offsets[g + 1];
  if (e0 < 0 || e1 < e0 || (e1 > e0 && !(src && dst))) {   // uniform over the block: no edge is read
    if (threadIdx.x == 0) lambda2[g] = __builtin_nan("");
    return;
  }
  laplacian_lambda2_graph(sm, src, dst, e0, e1, n, g * (int64_t)n, lambda2 + g);
}

// graphs of unequal size with LOCAL ids (isic_hip_hetero_ragged.h): n_g from node_offsets, LDS sized for max_nodes
__global__ __launch_bounds__(SP_THREADS) void laplacian_lambda2_ragged_kernel(const int64_t* __restrict__ src,
                                                                              const int64_t* __restrict__ dst,
                                                                              const int64_t* __restrict__ edge_offsets,
                                                                              const int64_t* __restrict__ node_offsets,
                                                                              int64_t E, int max_nodes,
                                                                              double* __restrict__ lambda2) {
  extern __shared__ double sm[];
  const int64_t g = blockIdx.x;
  const int64_t e0 = edge_offsets[g], e1 = edge_offsets[g + 1], n = node_offsets[g + 1] - node_offsets[g];
  if (e0 < 0 || e1 < e0 || e1 > E || n < 0 || n > max_nodes) {   // uniform over the block: no edge is read
    if (threadIdx.x == 0) lambda2[g] = __builtin_nan("");
    return;
  }
  laplacian_lambda2_graph(sm, src, dst, e0, e1, (int)n, 0, lambda2 + g);
}

// ------------------------------------------------------------------------------------------- segment statistics
__device__ double block_sum_f64(double v, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum_f64(v);
  __syncthreads();                        // red may still be read by the previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < SEG_WAVES; ++w) s += red[w];
  return s;
}

__global__ __launch_bounds__(SEG_THREADS) void segment_stats_kernel(const float* __restrict__ values,
                                                                    const int64_t* __restrict__ edge_offsets,
                                                                    int64_t num_edges, int G, double* __restrict__ mean,
                                                                    double* __restrict__ stdv, double* __restrict__ median) {
  __shared__ float keys[ISIC_SEGMENT_MAX_LEN];
  __shared__ double red[SEG_WAVES];
  const int tid = threadIdx.x;
  const int g = (int)(blockIdx.x % (unsigned)G), mi = (int)(blockIdx.x / (unsigned)G);
  const int64_t out = (int64_t)mi * G + g;
  const int64_t e0 = edge_offsets[g], e1 = edge_offsets[g + 1];
  if (e0 < 0 || e1 <= e0 || e1 > num_edges || e1 - e0 > ISIC_SEGMENT_MAX_LEN) {   // empty (np.mean([])) or invalid
    if (tid == 0) mean[out] = stdv[out] = median[out] = __builtin_nan("");
    return;
  }
  const int len = (int)(e1 - e0);
  int P = 1;
  while (P < len) P <<= 1;
  const float* v = values + (int64_t)mi * num_edges + e0;
  double acc = 0.0;
  for (int i = tid; i < P; i += SEG_THREADS) {
    const float x = i < len ? v[i] : INFINITY;
    keys[i] = x;
    if (i < len) acc += (double)x;
  }
  const double mu = block_sum_f64(acc, red) / len;      // the barrier inside also publishes keys[]
  double sq = 0.0;
  for (int i = tid; i < len; i += SEG_THREADS) {
    const double d = (double)keys[i] - mu;
    sq += d * d;
  }
  const double var = block_sum_f64(sq, red) / len;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += SEG_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const float a = keys[i], b = keys[ixj];
          if ((a > b) == ((i & k) == 0)) {
            keys[i] = b;
            keys[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  if (tid == 0) {
    mean[out] = mu;
    stdv[out] = sqrt(var);
    median[out] = (len & 1) ? (double)keys[len / 2] : 0.5 * ((double)keys[len / 2 - 1] + (double)keys[len / 2]);
  }
}

}  // namespace

extern "C" {

int isic_laplacian_lambda2_f64(const int64_t* src, const int64_t* dst, const int64_t* edge_offsets, int G, int nodes,
                               double* lambda2, void* stream) {
  if (nodes < 1 || nodes > ISIC_SPECTRAL_MAX_NODES) return ISIC_ERR_UNSUPPORTED;
  ISIC_CHECK_ARG(G >= 0);
  if (G == 0) return ISIC_OK;
  ISIC_CHECK_ARG(edge_offsets && lambda2);
  return isic_launch_lds<laplacian_lambda2_kernel, SP_MAX_LDS>(dim3((unsigned)G), dim3(SP_THREADS), lambda2_lds_bytes(nodes),
                                                               as_stream(stream), src, dst, edge_offsets, nodes, lambda2);
}

int isic_laplacian_lambda2_ragged_f64(const int64_t* src, const int64_t* dst, const int64_t* edge_offsets,
                                      const int64_t* node_offsets, int G, int64_t E, int max_nodes, double* lambda2,
                                      void* stream) {
  ISIC_CHECK_ARG(G >= 0 && E >= 0 && max_nodes >= 0);
  if (G == 0) return ISIC_OK;
  ISIC_CHECK_ARG(edge_offsets && node_offsets && lambda2);
  ISIC_CHECK_ARG(E == 0 || (src && dst));
  if (max_nodes > ISIC_SPECTRAL_MAX_NODES || E >= 0x80000000LL) return ISIC_ERR_UNSUPPORTED;
  return isic_launch_lds<laplacian_lambda2_ragged_kernel, SP_MAX_LDS>(dim3((unsigned)G), dim3(SP_THREADS),
                                                                      lambda2_lds_bytes(max_nodes), as_stream(stream), src, dst,
                                                                      edge_offsets, node_offsets, E, max_nodes, lambda2);
}

int isic_segment_stats_f32(const float* values, const int64_t* edge_offsets, int64_t num_edges, int M, int G,
                           int64_t max_segment, double* mean, double* std, double* median, void* stream) {
  ISIC_CHECK_ARG(num_edges >= 0 && M >= 0 && G >= 0 && max_segment >= 0);
  if (max_segment > ISIC_SEGMENT_MAX_LEN) return ISIC_ERR_UNSUPPORTED;
  if ((int64_t)M * G == 0) return ISIC_OK;
  ISIC_CHECK_ARG((int64_t)M * G <= 0x7fffffff);
  ISIC_CHECK_ARG(edge_offsets && mean && std && median && (values || num_edges == 0));
  hipLaunchKernelGGL(segment_stats_kernel, dim3((unsigned)(M * G)), dim3(SEG_THREADS), 0, as_stream(stream), values,
                     edge_offsets, num_edges, G, mean, std, median);
  return isic_launch_status();
}

}  // extern "C"
