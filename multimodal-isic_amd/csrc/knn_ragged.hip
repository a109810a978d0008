// k-NN graphs among patch sets of unequal size (include/isic_hip_knn_ragged.h; gfx950): the Gram kernel of knn_gram.hip with
// its work sized by the graph, and the edge lists of several k values out of one neighbour table.
//
// knn_ragged_kernel<NW>: NW waves own NW row stripes of 16 nodes against NW column tiles.  Three launches, NW = 4, 8, 13, each
// taking the graphs of its size class (<= 64, 65 .. 128, 129 .. 208 nodes; a class above the batch's max_nodes is not
// launched): the small workgroups share a CU.  For a graph of N nodes, nt = ceil(N / 16):
//   * only the waves < nt stage their 16 rows of a K-chunk (LDS-DMA, the XOR-swizzled layout of knn_gram.hip) and multiply,
//     and only against the column tiles < nt: nt^2 tiles instead of 169.  Every skip is wave-uniform.
//   * the MFMA sequence of one accumulator is knn_gram_kernel's: K-chunks of 32 floats in order, two quarters, the four
//     v_mfma_f32_16x16x4_f32 of a quarter take k = 4 fg + j; the Gram diagonal as |x_i|^2, the distance and the selection
//     are the same code (knn_tile.inc, instantiated for NW tiles here and for 13 there).  Tiles that are not multiplied
//     enter the selection as +inf, which is what knn_gram_kernel makes of them (columns past the graph), so indices and
//     distances are equal bit for bit (tests/test_knn_ragged_gpu.py).  The multiply loop is kt_multiply there and here;
//     this kernel steps over the tiles at or past nt and holds one quarter's fragments at a time.
//   * synchronisation is plain: two stages of KC K-chunks (a round); per round every wave waits for ALL its outstanding
//     memory operations (vmcnt(0)), one s_barrier, then the next round's DMA goes out behind it and overlaps this round's
//     MFMAs.  A stage is overwritten one barrier after its last reader has its data.  A workgroup takes ONE graph (the grid
//     is G), so nothing is shared between graphs: no stage, no norm buffer, no outstanding store; the other workgroups of
//     the CU (4 / 2 / 1 of them) cover a graph's first round.
//   * a graph's offsets are validated before they address anything (0 <= lo <= hi <= total_nodes, hi - lo <= max_nodes);
//     staged rows are clamped into the graph, stores are guarded by q < N.
#include "common.h"
#include "mfma_tile.h"
#include "../../include/isic_hip_knn_ragged.h"

namespace {

#include "knn_tile.inc"

constexpr int KR_STAGES = 2;
constexpr int KR_MAX_GRAPHS = 1 << 22;                     // one workgroup per graph: G x 832 threads stays below 2^32

struct KnnRaggedArgs {
  const float* x;
  const int64_t* offsets;
  int64_t* nn_idx;
  float* nn_dist;
  int64_t total_nodes;
  int G, D, k, max_nodes;
  int above;                                               // this launch takes the graphs of above < N <= 16 NW nodes
};

template <int NW, int KC, bool WITH_DIST>
// at most 128 registers: 4 / 2 / 1 workgroups per CU (the 4-wave one by its 33 KB of LDS, the others by their waves)
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(4)))
void knn_ragged_kernel(KnnRaggedArgs a) {
  constexpr int CHUNK = NW * 16 * 128;                     // one K-chunk of 32 floats for NW * 16 rows
  constexpr int STAGE = KC * CHUNK;                        // a round: KC K-chunks behind one wait and one barrier
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)smem;
  float* sqn = reinterpret_cast<float*>(smem + KR_STAGES * STAGE);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int nchunks = a.D >> 5;
  const int nrounds = (nchunks + KC - 1) / KC;
  // staging: piece h (= 0, 1) of this wave brings rows 16 wave + 8 h + r8, swizzled on the source side (knn_tile.inc)
  const int r8 = lane >> 3;
  const unsigned src_chunk = kt_src_chunk(lane);
  const unsigned foff0 = kt_foff0(fr, fg);               // fragment of tile 0, k-quarter 0; kq = 1: ^ 64

  const int g = (int)blockIdx.x;                         // one workgroup per graph: the grid is G
  const long long lo = a.offsets[g], hi = a.offsets[g + 1];
  const bool span_ok = lo >= 0 && hi >= lo && hi <= (long long)a.total_nodes && hi - lo <= (long long)a.max_nodes;
  const bool mine = span_ok && hi - lo > (long long)a.above && hi - lo <= (long long)(NW * 16);
  const int N = __builtin_amdgcn_readfirstlane(mine ? (int)(hi - lo) : 0);
  if (N <= 0) return;                                    // block-uniform: an empty, refused or other launch's graph touches nothing
  const int nt = (N + 15) >> 4;                          // <= NW: max_nodes <= 16 NW
  const bool active = wave < nt;                         // wave-uniform

  auto issue = [&](int r) {                              // the K-chunks r KC .. r KC + KC - 1 (those that exist) into stage r % 2
    if (!active) return;
#pragma unroll
    for (int s = 0; s < KC; ++s) {
      const int kc = r * KC + s;
      if (kc >= nchunks) break;
      const unsigned dst = lds0 + (unsigned)((r % KR_STAGES) * STAGE + s * CHUNK + wave * 2048);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        int row = wave * 16 + h * 8 + r8;
        row = row < N ? row : N - 1;                     // rows past the graph repeat its last node (masked where they are used)
        const unsigned char* src = reinterpret_cast<const unsigned char*>(a.x + (size_t)(lo + row) * a.D) +
                                   (size_t)kc * 128 + src_chunk;
        isic_glds16(src, dst + h * 1024);
      }
    }
  };

  f32x4 acc[NW];
#pragma unroll
  for (int c = 0; c < NW; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};

  issue(0);
  for (int r = 0; r < nrounds; ++r) {
    // round r has landed once this wave's DMAs are complete (everything it has in flight) and every wave has said so;
    // past the barrier no wave reads stage (r + 1) % 2 any more
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (r + 1 < nrounds) issue(r + 1);
    if (!active) continue;
#pragma unroll 1
    for (int s = 0; s < KC; ++s)                           // the K-chunks in their order: the summation order of knn_gram_kernel
      if (r * KC + s < nchunks) kt_multiply<NW, true>(nt, smem + (r % KR_STAGES) * STAGE + s * CHUNK, foff0, wave, acc);
  }

  // ================================================================ the graph is complete: distances -> top-k
  if (active) kt_store_sqn<NW>(acc, wave, fr, fg, sqn);
  lds_barrier();
  if (active) {
    kt_distances<NW>(acc, sqn, wave, fr, fg, nt, N);
    int res_i[4];
    float res_v[4];
    kt_select<NW>(acc, fr, a.k, res_i, res_v);
    // lane fr holds neighbour #fr of its four rows: one contiguous run of k indices per row
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = wave * 16 + fg * 4 + j;
      if (q < N && fr < a.k) {
        const size_t at = (size_t)(lo + q) * a.k + fr;
        a.nn_idx[at] = (int64_t)res_i[j];
        if (WITH_DIST) a.nn_dist[at] = res_v[j];
      }
    }
  }
}

template <int NW, int KC>
int kr_launch(KnnRaggedArgs a, int above, hipStream_t stream) {
  a.above = above;
  constexpr int LDS = KR_STAGES * KC * NW * 16 * 128 + NW * 16 * 4;
  // one workgroup per graph, handed out by the hardware as workgroups retire (graphs differ in work by up to (16 NW / 16)^2
  // and a launch skips the graphs of the other classes, so a fixed share per workgroup leaves a long tail)
  if (!a.nn_dist) return isic_launch_lds<knn_ragged_kernel<NW, KC, false>, LDS>(dim3(a.G), dim3(NW * 64), LDS, stream, a);
  return isic_launch_lds<knn_ragged_kernel<NW, KC, true>, LDS>(dim3(a.G), dim3(NW * 64), LDS, stream, a);
}

// ---------------------------------------------------------------------------------------------------- edge lists
constexpr int KE_MAX_K = 16;
constexpr int KE_BLOCK = 256;

struct KnnEdgesArgs {
  const int64_t* nn_idx;
  const int64_t* offsets;
  const int64_t* edge_base;
  int64_t* src_out;
  int64_t* dst_out;
  uint32_t* bad;
  int64_t total_nodes, total_edges;
  int G, K, kmax, global_ids;
  int k_values[KE_MAX_K];
};

// one workgroup per graph, list after list: position base + e holds edge (e / kk, e % kk) -- consecutive threads write
// consecutive positions
__global__ __launch_bounds__(KE_BLOCK) void knn_edges_ragged_kernel(KnnEdgesArgs a) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t lo = a.offsets[g], hi = a.offsets[g + 1];
  const bool span_ok = lo >= 0 && hi >= lo && hi <= a.total_nodes;          // block-uniform
  const int64_t n = span_ok ? hi - lo : 0;
  const int64_t shift = a.global_ids ? lo : 0;
  unsigned bad = 0;
  for (int q = 0; q < a.K; ++q) {
    const int64_t kq = a.k_values[q];
    const int64_t kk = n < 2 ? 0 : (kq < n - 1 ? kq : n - 1);               // 03:42-45; kq >= 1 is checked by the entry
    const int64_t e0 = a.edge_base[(size_t)q * (a.G + 1) + g], e1 = a.edge_base[(size_t)q * (a.G + 1) + g + 1];
    const int64_t cnt = kk <= a.kmax ? n * kk : -1;                         // n < 2^31, kmax <= 2^16: no overflow
    const bool seg_ok = span_ok && cnt >= 0 && e0 >= 0 && e1 >= e0 && e1 <= a.total_edges && e1 - e0 == cnt;
    if (!seg_ok) {                                                          // block-uniform
      if (tid == 0) ++bad;
      continue;
    }
    const bool small = cnt < 0x7FFFFFFFLL;
    for (int64_t e = tid; e < cnt; e += KE_BLOCK) {
      const int64_t i = small ? (int64_t)((unsigned)e / (unsigned)kk) : e / kk;
      const int64_t j = e - i * kk;                                         // i < n, j < kk <= kmax
      const int64_t v = a.nn_idx[(size_t)(lo + i) * a.kmax + j];
      const bool ok = (uint64_t)v < (uint64_t)n;
      a.src_out[e0 + e] = i + shift;
      a.dst_out[e0 + e] = ok ? v + shift : -1;
      bad += ok ? 0u : 1u;
    }
  }
  if (bad) atomicAdd(a.bad, bad);
}

}  // namespace

extern "C" {

int isic_knn_graph_ragged(const float* x, const int64_t* offsets, int G, int D, int k, int max_nodes,
                          int64_t total_nodes, int64_t* nn_idx, float* nn_dist, void* stream) {
  ISIC_CHECK_ARG(G >= 0 && D > 0 && k > 0 && max_nodes >= 0 && total_nodes >= 0);
  if (!knn_tile_supported(D, k, max_nodes) || G > KR_MAX_GRAPHS) return ISIC_ERR_UNSUPPORTED;
  if (G == 0 || total_nodes == 0) return ISIC_OK;
  ISIC_CHECK_ARG(x && offsets && nn_idx);
  if (max_nodes == 0) return ISIC_OK;                      // no graph may own a node: nothing to write
  KnnRaggedArgs a;
  a.x = x; a.offsets = offsets; a.nn_idx = nn_idx; a.nn_dist = nn_dist; a.total_nodes = total_nodes;
  a.G = G; a.D = D; a.k = k; a.max_nodes = max_nodes;
  // One launch per size class that max_nodes allows, each taking the graphs of its class: a graph is multiplied by the
  // smallest workgroup that holds it, whatever the largest graph of the batch: the 8-wave kernel holds 2 workgroups per
  // CU and a 54-node graph leaves half of its waves idle (DESIGN.md "k-NN graphs among the lesion patches").
  int rc = kr_launch<4, 2>(a, 0, as_stream(stream));
  if (rc == ISIC_OK && max_nodes > 64) rc = kr_launch<8, 2>(a, 64, as_stream(stream));
  if (rc == ISIC_OK && max_nodes > 128) rc = kr_launch<13, 1>(a, 128, as_stream(stream));
  return rc;
}

int isic_knn_edges_ragged(const int64_t* nn_idx, int kmax, const int64_t* offsets, int G, int64_t total_nodes,
                          const int32_t* k_values, int K, const int64_t* edge_base, int64_t total_edges, int global_ids,
                          int64_t* src_out, int64_t* dst_out, uint32_t* bad, void* stream) {
  ISIC_CHECK_ARG(G >= 0 && total_nodes >= 0 && total_edges >= 0 && kmax >= 1 && K >= 1 && K <= KE_MAX_K && k_values);
  for (int q = 0; q < K; ++q) ISIC_CHECK_ARG(k_values[q] >= 1);
  if (total_nodes >= 0x80000000LL || kmax > 65536 || G > KR_MAX_GRAPHS) return ISIC_ERR_UNSUPPORTED;    // n_g * kk < 2^47
  if (G == 0 || total_edges == 0) return ISIC_OK;
  ISIC_CHECK_ARG(offsets && edge_base && src_out && dst_out && bad);
  ISIC_CHECK_ARG(total_nodes == 0 || nn_idx);
  KnnEdgesArgs a;
  a.nn_idx = nn_idx; a.offsets = offsets; a.edge_base = edge_base; a.src_out = src_out; a.dst_out = dst_out; a.bad = bad;
  a.total_nodes = total_nodes; a.total_edges = total_edges; a.G = G; a.K = K; a.kmax = kmax; a.global_ids = global_ids;
  for (int q = 0; q < KE_MAX_K; ++q) a.k_values[q] = q < K ? k_values[q] : 1;
  hipLaunchKernelGGL(knn_edges_ragged_kernel, dim3((unsigned)G), dim3(KE_BLOCK), 0, as_stream(stream), a);
  return isic_launch_status();
}

}  // extern "C"
