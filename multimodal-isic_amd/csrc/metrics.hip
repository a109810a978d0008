// The integer counts behind the validation metrics (include/isic_hip_metrics.h): the confusion matrix, the one-vs-rest
// pair counts of the AUROC, the two rejection flags and the fp64 loss sum of one validation set, in two launches.  Replaces
// the per-chunk read-back and the scikit-learn calls of 01_train_mil_teacher.py:111-113,266-272 and 05_train_gnns.py:284-302.
//
//   * Order.  A score is turned into a 32-bit integer KEY whose signed order is the IEEE order of the finite fp32 values
//     (-0.0 is made +0.0 first; then a negative pattern has its low 31 bits flipped).  Keys are compared with integer
//     compares, so a subnormal compares by value whatever the wave's denormal mode says.  A sample that is not counted (a
//     non-finite score, a label outside [0, C), a row past n) gets the key INT_MAX on the j side and INT_MIN on the i side:
//     [k_i > k_j] + [k_i >= k_j] is then 0 without a branch.
//   * Pair pass.  Block (x, y): thread t is sample i = 256 x + t with c = labels[i]; the block walks the tiles y, y + Y, ...
//     of 512 samples j, whose keys sit in LDS as rows of 16 words (lanes of a wave read one row: no bank conflict, constant
//     offsets in the unrolled loop).  The thread adds [k_ic > k_jc] + [k_ic >= k_jc] = 2 [>] + [==] over ALL counted j, its
//     own class and itself included: inside a class the ordered pairs (i, j), (j, i) give 2 together and (i, i) gives 1, so
//     the class's own pairs add exactly support_c^2, which the finishing kernel takes off again.  That keeps the label of j
//     out of the inner loop.  32-bit inside a tile (<= 1024), 64-bit across tiles; the threads of a class meet in LDS (integer
//     adds: the order cannot change the bits) and the block writes 16 int64 partials.
//   * The blocks with y == 0 also form their 256 samples' confusion counts, flags and loss (a fixed tree in fp64).
//   * metrics_finish_kernel (one block) adds the integer partials, the loss partials in ascending block order, derives the
//     supports from the confusion matrix and writes every output.
#include "common.h"
#include "../../include/isic_hip_metrics.h"

#include <limits.h>

namespace {

constexpr int BLOCK = ISIC_METRICS_BLOCK;
constexpr int TILE = ISIC_METRICS_TILE;
constexpr int ROW = 16;                        // words per staged row (C <= 16)
constexpr int MAX_C = 16;
constexpr int TARGET_BLOCKS = 2048;            // the j tiles are dealt to Y blocks per x until the grid has about this many
static_assert(TILE % BLOCK == 0 && TILE <= 4096, "tile");

struct MetricsArgs {
  const float* scores;
  const int64_t* labels;
  const float* loss;
  int64_t n;
  int C, jtiles;
  long long* pair_part;                        // [x][y][16]
  double* loss_part;                           // [x]
  int* conf_part;                              // [x][C * C]
  int* flag_part;                              // [x][2]
};

__device__ __forceinline__ bool nonfinite_bits(unsigned b) { return (b & 0x7F800000u) == 0x7F800000u; }
// signed-integer order == IEEE order of finite fp32 values, -0.0 == +0.0
__device__ __forceinline__ int order_key(unsigned b) {
  if ((b & 0x7FFFFFFFu) == 0u) b = 0u;
  const int s = (int)b;
  return s ^ ((s >> 31) & 0x7FFFFFFF);
}

__global__ __launch_bounds__(BLOCK) void metrics_pair_kernel(MetricsArgs a) {
  __shared__ int keys[TILE * ROW];             // 32 KB
  __shared__ int bad[TILE];
  __shared__ int conf[MAX_C * MAX_C];
  __shared__ int flg[2];
  __shared__ unsigned long long cls[MAX_C];
  __shared__ double lsum[BLOCK];
  const int t = threadIdx.x, C = a.C;
  const int64_t i = (int64_t)blockIdx.x * BLOCK + t;
  const bool first = blockIdx.y == 0;          // block-uniform

  // ---- this thread's sample
  int c = 0, pred = 0, nf = 0, ki = INT_MIN;
  bool lab_bad = false, ok = false;
  if (i < a.n) {
    const int64_t lab = a.labels[i];
    lab_bad = lab < 0 || lab >= C;
    const float* row = a.scores + i * C;
    int best = INT_MIN, own = INT_MIN;
    for (int k = 0; k < C; ++k) {
      const unsigned b = __float_as_uint(row[k]);
      nf += nonfinite_bits(b) ? 1 : 0;
      const int key = order_key(b);
      if (k == 0 || key > best) { best = key; pred = k; }
      if (!lab_bad && k == (int)lab) own = key;
    }
    ok = !lab_bad && nf == 0;
    if (ok) { c = (int)lab; ki = own; }
  }
  if (t < MAX_C) cls[t] = 0ull;
  if (first) {
    conf[t] = 0;                               // BLOCK == MAX_C * MAX_C
    if (t < 2) flg[t] = 0;
    lsum[t] = (ok && a.loss) ? (double)a.loss[i] : 0.0;
    __syncthreads();
    if (ok) atomicAdd(&conf[c * C + pred], 1);
    if (nf) atomicAdd(&flg[0], nf);
    if (lab_bad) atomicAdd(&flg[1], 1);
#pragma unroll
    for (int s = BLOCK / 2; s > 0; s >>= 1) {  // fixed tree
      __syncthreads();
      if (t < s) lsum[t] += lsum[t + s];
    }
    __syncthreads();
    if (t < C * C) a.conf_part[(size_t)blockIdx.x * (C * C) + t] = conf[t];
    if (t < 2) a.flag_part[(size_t)blockIdx.x * 2 + t] = flg[t];
    if (t == 0) a.loss_part[blockIdx.x] = lsum[0];
  }

  // ---- the tiles of j
  unsigned long long total = 0ull;
  const int* mine = keys + c;
  for (int jt = blockIdx.y; jt < a.jtiles; jt += gridDim.y) {
    const int64_t j0 = (int64_t)jt * TILE;
#pragma unroll
    for (int r = t; r < TILE; r += BLOCK) {
      const int64_t j = j0 + r;
      int b = 1;
      if (j < a.n) {
        const int64_t lab = a.labels[j];
        b = (lab < 0 || lab >= C) ? 1 : 0;
      }
      bad[r] = b;
    }
    __syncthreads();                           // (also: every thread is past the previous tile's compare loop)
    for (int e = t; e < TILE * C; e += BLOCK) {
      const int r = e / C, col = e - r * C;
      const int64_t j = j0 + r;
      if (j < a.n) {
        const unsigned b = __float_as_uint(a.scores[j * C + col]);
        if (nonfinite_bits(b)) bad[r] = 1;     // (several threads may store the same 1)
        else keys[r * ROW + col] = order_key(b);
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = t; r < TILE; r += BLOCK)
      if (bad[r])
        for (int col = 0; col < C; ++col) keys[r * ROW + col] = INT_MAX;
    __syncthreads();
    unsigned cnt = 0u;
#pragma unroll 16
    for (int r = 0; r < TILE; ++r) {
      const int kj = mine[r * ROW];
      cnt += (ki > kj ? 1u : 0u) + (ki >= kj ? 1u : 0u);
    }
    total += cnt;
  }
  if (ok && total) atomicAdd(&cls[c], total);
  __syncthreads();
  if (t < MAX_C) a.pair_part[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * MAX_C + t] = (long long)cls[t];
}

__global__ __launch_bounds__(BLOCK) void metrics_finish_kernel(MetricsArgs a, int xblocks, int yblocks, int64_t* confusion,
                                                               int64_t* pair2, int64_t* flags, double* loss_sum) {
  __shared__ long long sconf[MAX_C * MAX_C];
  __shared__ long long spair[BLOCK];
  const int t = threadIdx.x, C = a.C, CC = C * C;
  if (t < CC) {
    long long s = 0;
    for (int x = 0; x < xblocks; ++x) s += a.conf_part[(size_t)x * CC + t];
    sconf[t] = s;
    confusion[t] = s;
  }
  if (t < 2) {
    long long s = 0;
    for (int x = 0; x < xblocks; ++x) s += a.flag_part[(size_t)x * 2 + t];
    flags[t] = s;
  }
  if (t == BLOCK - 1 && loss_sum) {            // ascending block order
    double s = 0.0;
    if (a.loss)
      for (int x = 0; x < xblocks; ++x) s += a.loss_part[x];
    *loss_sum = s;
  }
  {                                            // 16 threads per class; integer adds, any order
    const int c = t & (MAX_C - 1), l = t >> 4;
    const size_t parts = (size_t)xblocks * yblocks;
    long long s = 0;
    for (size_t k = l; k < parts; k += BLOCK / MAX_C) s += a.pair_part[k * MAX_C + c];
    spair[t] = s;
  }
  __syncthreads();
  if (t < C) {
    long long s = 0, support = 0;
    for (int l = 0; l < BLOCK / MAX_C; ++l) s += spair[l * MAX_C + t];
    for (int p = 0; p < C; ++p) support += sconf[t * C + p];
    pair2[t] = s - support * support;          // the class's own ordered pairs and diagonal: exactly support^2
  }
}

struct MetricsPlan { int64_t xblocks; int jtiles, yblocks; size_t pair_bytes, loss_bytes, conf_bytes, flag_bytes; };

bool metrics_plan(int64_t n, int C, MetricsPlan& p) {
  if (n < 0 || n > (int64_t)INT_MAX || C < 2 || C > MAX_C) return false;
  p.xblocks = ceil_div64(n, BLOCK);
  p.jtiles = (int)ceil_div64(n, TILE);
  int64_t y = p.xblocks ? ceil_div64(TARGET_BLOCKS, p.xblocks) : 1;
  if (y > p.jtiles) y = p.jtiles;
  if (y < 1) y = 1;
  p.yblocks = (int)y;
  const auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  p.pair_bytes = (size_t)p.xblocks * p.yblocks * MAX_C * sizeof(long long);
  p.loss_bytes = up16((size_t)p.xblocks * sizeof(double));
  p.conf_bytes = up16((size_t)p.xblocks * C * C * sizeof(int));
  p.flag_bytes = up16((size_t)p.xblocks * 2 * sizeof(int));
  return true;
}

}  // namespace

extern "C" {

size_t isic_class_metrics_f32_workspace_bytes(int64_t n, int C) {
  MetricsPlan p;
  if (!metrics_plan(n, C, p)) return 0;
  return p.pair_bytes + p.loss_bytes + p.conf_bytes + p.flag_bytes;
}

int isic_class_metrics_f32(const float* scores, const int64_t* labels, const float* loss, int64_t n, int C,
                           int64_t* confusion, int64_t* pair2, int64_t* flags, double* loss_sum, void* workspace,
                           size_t workspace_bytes, void* stream) {
  ISIC_CHECK_ARG(n >= 0 && confusion && pair2 && flags && (loss_sum || !loss) && ((scores && labels) || n == 0));
  MetricsPlan p;
  if (!metrics_plan(n, C, p)) return ISIC_ERR_UNSUPPORTED;
  const size_t need = isic_class_metrics_f32_workspace_bytes(n, C);
  if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15))) return ISIC_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  MetricsArgs a;
  a.scores = scores; a.labels = labels; a.loss = loss; a.n = n; a.C = C; a.jtiles = p.jtiles;
  char* w = reinterpret_cast<char*>(workspace);
  a.pair_part = reinterpret_cast<long long*>(w);
  a.loss_part = reinterpret_cast<double*>(w + p.pair_bytes);
  a.conf_part = reinterpret_cast<int*>(w + p.pair_bytes + p.loss_bytes);
  a.flag_part = reinterpret_cast<int*>(w + p.pair_bytes + p.loss_bytes + p.conf_bytes);
  if (n > 0)
    hipLaunchKernelGGL(metrics_pair_kernel, dim3((unsigned)p.xblocks, (unsigned)p.yblocks), dim3(BLOCK), 0, st, a);
  hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(BLOCK), 0, st, a, (int)p.xblocks, p.yblocks, confusion, pair2,
                     flags, loss_sum);
  return isic_launch_status();
}

}  // extern "C"
