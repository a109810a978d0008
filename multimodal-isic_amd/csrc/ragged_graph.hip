// Patch graphs of unequal size (include/isic_hip_ragged.h): the subgraph induced by a node subset for a whole record set --
// count, then a stable compaction -- and the one-launch assembly of a step's batched CSR out of a store whose graphs differ
// in node and entry count (graph.hip: csr_batch_assemble_kernel is the equal-size case).
//
// Every value read from device memory that becomes an index (graph offsets, edge endpoints, selection indices, prefix sums)
// is compared with the sizes passed by value first; what does not fit is counted (`bad`) or dropped, never dereferenced.
#include "common.h"
#include "../../include/isic_hip_ragged.h"

namespace {

#include "ragged_scan.inc"                                  // RG_BLOCK, rg_block_scan, rg_block_sum

// graph g's node and edge segments; ok = both lie inside [0, T] / [0, E] and are non-decreasing
struct RgSegment {
  int64_t n0, n, e0, ne;
  bool ok;
};
__device__ __forceinline__ RgSegment rg_segment(const int64_t* __restrict__ node_offsets,
                                                const int64_t* __restrict__ edge_offsets, int g, int64_t T, int64_t E) {
  RgSegment s;
  const int64_t n1 = node_offsets[g + 1], e1 = edge_offsets[g + 1];
  s.n0 = node_offsets[g]; s.e0 = edge_offsets[g];
  s.n = n1 - s.n0; s.ne = e1 - s.e0;
  s.ok = s.n0 >= 0 && n1 >= s.n0 && n1 <= T && s.e0 >= 0 && e1 >= s.e0 && e1 <= E;
  return s;
}

// one workgroup per graph: new_id of its nodes, then (the ids are read back by other threads of the block: fence + barrier)
// the number of edges with both endpoints kept
__global__ __launch_bounds__(RG_BLOCK) void induced_count_kernel(
    const int64_t* __restrict__ node_offsets, const int64_t* __restrict__ edge_offsets, const int64_t* __restrict__ src,
    const int64_t* __restrict__ dst, const uint8_t* __restrict__ keep, int64_t T, int64_t E, int32_t* new_id,
    int64_t* __restrict__ kept_nodes, int64_t* __restrict__ kept_edges, uint32_t* __restrict__ bad) {
  __shared__ int wsum[RG_WAVES];
  __shared__ unsigned red[RG_WAVES];
  const int g = blockIdx.x, tid = threadIdx.x;
  const RgSegment sg = rg_segment(node_offsets, edge_offsets, g, T, E);
  if (!sg.ok) {                                            // block-uniform
    if (tid == 0) { kept_nodes[g] = 0; kept_edges[g] = 0; bad[g] = 0xFFFFFFFFu; }
    return;
  }
  int any = 0;
  for (int64_t i = tid; i < sg.n; i += RG_BLOCK) any |= keep[sg.n0 + i] != 0 ? 1 : 0;
  any = __syncthreads_or(any);                             // no flag set: the graph keeps every node
  int base = 0;
  for (int64_t c0 = 0; c0 < sg.n; c0 += RG_BLOCK) {        // block-uniform trip count
    const int64_t i = c0 + tid;
    const bool in = i < sg.n;
    const bool flag = in && (!any || keep[sg.n0 + i] != 0);
    int total;
    const int pre = rg_block_scan(flag, wsum, total);
    if (in) new_id[sg.n0 + i] = flag ? base + pre : -1;
    base += total;
  }
  __threadfence_block();
  __syncthreads();
  unsigned cnt = 0, bd = 0;
  for (int64_t e = tid; e < sg.ne; e += RG_BLOCK) {
    const int64_t s = src[sg.e0 + e], d = dst[sg.e0 + e];
    if ((uint64_t)s >= (uint64_t)sg.n || (uint64_t)d >= (uint64_t)sg.n) ++bd;
    else if (new_id[sg.n0 + s] >= 0 && new_id[sg.n0 + d] >= 0) ++cnt;
  }
  cnt = rg_block_sum(cnt, red);
  bd = rg_block_sum(bd, red);
  if (tid == 0) { kept_nodes[g] = base; kept_edges[g] = cnt; bad[g] = bd; }
}

// one workgroup per graph: rows of the kept nodes, then the kept edges chunk by chunk at base + block scan (stable)
__global__ __launch_bounds__(RG_BLOCK) void induced_write_kernel(
    const int64_t* __restrict__ node_offsets, const int64_t* __restrict__ edge_offsets, const int64_t* __restrict__ src,
    const int64_t* __restrict__ dst, const float* __restrict__ w, const int32_t* __restrict__ new_id, int64_t T, int64_t E,
    const int64_t* __restrict__ node_out_offsets, const int64_t* __restrict__ edge_out_offsets, int64_t T_out, int64_t E_out,
    int64_t* __restrict__ src_out, int64_t* __restrict__ dst_out, float* __restrict__ w_out, int64_t* __restrict__ rows_out) {
  __shared__ int wsum[RG_WAVES];
  const int g = blockIdx.x, tid = threadIdx.x;
  const RgSegment sg = rg_segment(node_offsets, edge_offsets, g, T, E);
  if (!sg.ok) return;
  const int64_t no0 = node_out_offsets[g], eo0 = edge_out_offsets[g];
  const int64_t n_lo = no0 > 0 ? no0 : 0, e_lo = eo0 > 0 ? eo0 : 0;      // the graph's own output segments, inside the arrays
  const int64_t n_hi = node_out_offsets[g + 1] < T_out ? node_out_offsets[g + 1] : T_out;
  const int64_t e_hi = edge_out_offsets[g + 1] < E_out ? edge_out_offsets[g + 1] : E_out;
  for (int64_t i = tid; i < sg.n; i += RG_BLOCK) {
    const int id = new_id[sg.n0 + i];
    const int64_t p = no0 + id;
    if (id >= 0 && p >= n_lo && p < n_hi) rows_out[p] = i;
  }
  int64_t base = eo0;
  for (int64_t c0 = 0; c0 < sg.ne; c0 += RG_BLOCK) {       // block-uniform trip count
    const int64_t e = c0 + tid;
    int ns = -1, nd = -1;
    if (e < sg.ne) {
      const int64_t s = src[sg.e0 + e], d = dst[sg.e0 + e];
      if ((uint64_t)s < (uint64_t)sg.n && (uint64_t)d < (uint64_t)sg.n) { ns = new_id[sg.n0 + s]; nd = new_id[sg.n0 + d]; }
    }
    const bool flag = ns >= 0 && nd >= 0;
    int total;
    const int64_t p = base + rg_block_scan(flag, wsum, total);
    if (flag && p >= e_lo && p < e_hi) {
      src_out[p] = ns;
      dst_out[p] = nd;
      if (w_out) w_out[p] = w[sg.e0 + e];
    }
    base += total;
  }
}

// the last position b in [0, B) with base[b] <= i: zero-length segments before it share its base and are stepped over
__device__ __forceinline__ int rg_position(const int64_t* __restrict__ base, int B, int64_t i) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (base[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void csr_batch_assemble_ragged_kernel(
    const int64_t* __restrict__ sel, const int64_t* __restrict__ node_base, const int64_t* __restrict__ nnz_base, int B, int G,
    int64_t total_nodes, int64_t total_nnz, const int64_t* __restrict__ store_node_off,
    const int64_t* __restrict__ store_nnz_off, const int* __restrict__ rowptr, const int* __restrict__ rowptr_t,
    const int* __restrict__ col, const int* __restrict__ col_t, const float* __restrict__ val, const float* __restrict__ val_t,
    const int* __restrict__ perm_t, int* __restrict__ rowptr_o, int* __restrict__ rowptr_t_o, int* __restrict__ col_o,
    int* __restrict__ col_t_o, float* __restrict__ val_o, float* __restrict__ val_t_o, int* __restrict__ perm_t_o,
    int* __restrict__ rowidx_o) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total_nnz) {
    const int b = rg_position(nnz_base, B, i);
    const int64_t g = sel[b], off = i - nnz_base[b];
    if ((uint64_t)g < (uint64_t)G && off >= 0 && i < nnz_base[b + 1]) {
      const int64_t s0 = store_nnz_off[g], s = s0 + off;
      if (s0 >= 0 && s < store_nnz_off[g + 1]) {
        const int64_t dn = node_base[b] - store_node_off[g], de = nnz_base[b] - s0;
        col_o[i] = (int)(col[s] + dn);
        col_t_o[i] = (int)(col_t[s] + dn);
        val_o[i] = val[s];
        val_t_o[i] = val_t[s];
        perm_t_o[i] = (int)(perm_t[s] + de);
      }
    }
  }
  if (i < total_nodes) {
    const int b = rg_position(node_base, B, i);
    const int64_t g = sel[b], off = i - node_base[b];
    if ((uint64_t)g < (uint64_t)G && off >= 0 && i < node_base[b + 1]) {
      const int64_t q0 = store_node_off[g], q = q0 + off;
      if (q0 >= 0 && q < store_node_off[g + 1]) {
        const int64_t de = nnz_base[b] - store_nnz_off[g];
        rowptr_o[i] = (int)(rowptr[q] + de);
        rowptr_t_o[i] = (int)(rowptr_t[q] + de);
        if (rowidx_o) rowidx_o[i] = (int)q;
      }
    }
  } else if (i == total_nodes) {
    rowptr_o[i] = (int)total_nnz;
    rowptr_t_o[i] = (int)total_nnz;
  }
}

}  // namespace

extern "C" {

int isic_induced_subgraph_count(const int64_t* node_offsets, const int64_t* edge_offsets, const int64_t* src,
                                const int64_t* dst, const uint8_t* keep, int G, int64_t T, int64_t E, int32_t* new_id,
                                int64_t* kept_nodes, int64_t* kept_edges, uint32_t* bad, void* stream) {
  ISIC_CHECK_ARG(G >= 0 && T >= 0 && E >= 0);
  if (G == 0) return ISIC_OK;
  ISIC_CHECK_ARG(node_offsets && edge_offsets && kept_nodes && kept_edges && bad);
  ISIC_CHECK_ARG(E == 0 || (src && dst));
  ISIC_CHECK_ARG(T == 0 || (keep && new_id));
  if (T >= 0x80000000LL || E >= 0x80000000LL) return ISIC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(induced_count_kernel, dim3((unsigned)G), dim3(RG_BLOCK), 0, as_stream(stream), node_offsets, edge_offsets,
                     src, dst, keep, T, E, new_id, kept_nodes, kept_edges, bad);
  return isic_launch_status();
}

int isic_induced_subgraph_write(const int64_t* node_offsets, const int64_t* edge_offsets, const int64_t* src,
                                const int64_t* dst, const float* edge_weight, const int32_t* new_id, int G, int64_t T,
                                int64_t E, const int64_t* node_out_offsets, const int64_t* edge_out_offsets, int64_t T_out,
                                int64_t E_out, int64_t* src_out, int64_t* dst_out, float* edge_weight_out,
                                int64_t* rows_out, void* stream) {
  ISIC_CHECK_ARG(G >= 0 && T >= 0 && E >= 0 && T_out >= 0 && E_out >= 0);
  if (G == 0) return ISIC_OK;
  ISIC_CHECK_ARG(node_offsets && edge_offsets && node_out_offsets && edge_out_offsets);
  ISIC_CHECK_ARG(E == 0 || (src && dst));
  ISIC_CHECK_ARG(T == 0 || new_id);
  ISIC_CHECK_ARG(T_out == 0 || rows_out);
  ISIC_CHECK_ARG(E_out == 0 || (src_out && dst_out));
  ISIC_CHECK_ARG((edge_weight == nullptr) == (edge_weight_out == nullptr) || E_out == 0 || E == 0);
  if (T >= 0x80000000LL || E >= 0x80000000LL || T_out >= 0x80000000LL || E_out >= 0x80000000LL) return ISIC_ERR_UNSUPPORTED;
  const bool weights = edge_weight && edge_weight_out;
  hipLaunchKernelGGL(induced_write_kernel, dim3((unsigned)G), dim3(RG_BLOCK), 0, as_stream(stream), node_offsets, edge_offsets,
                     src, dst, weights ? edge_weight : nullptr, new_id, T, E, node_out_offsets, edge_out_offsets, T_out, E_out,
                     src_out, dst_out, weights ? edge_weight_out : nullptr, rows_out);
  return isic_launch_status();
}

int isic_csr_batch_assemble_ragged(const int64_t* sel, const int64_t* node_base, const int64_t* nnz_base, int B, int G,
                                   int64_t total_nodes, int64_t total_nnz, const int64_t* store_node_off,
                                   const int64_t* store_nnz_off, const int32_t* rowptr, const int32_t* rowptr_t,
                                   const int32_t* col, const int32_t* col_t, const float* val, const float* val_t,
                                   const int32_t* perm_t, int32_t* rowptr_out, int32_t* rowptr_t_out, int32_t* col_out,
                                   int32_t* col_t_out, float* val_out, float* val_t_out, int32_t* perm_t_out,
                                   int32_t* row_index_out, void* stream) {
  ISIC_CHECK_ARG(B >= 0 && G >= 0 && total_nodes >= 0 && total_nnz >= 0);
  if (B == 0) return ISIC_OK;
  ISIC_CHECK_ARG(G > 0);
  ISIC_CHECK_ARG(sel && node_base && nnz_base && store_node_off && store_nnz_off && rowptr && rowptr_t && rowptr_out &&
                 rowptr_t_out);
  ISIC_CHECK_ARG(total_nnz == 0 || (col && col_t && val && val_t && perm_t && col_out && col_t_out && val_out && val_t_out &&
                                    perm_t_out));
  if (total_nodes >= 0x7FFFFFFFLL || total_nnz >= 0x7FFFFFFFLL) return ISIC_ERR_UNSUPPORTED;
  const int64_t nr = total_nodes + 1;
  const int64_t work = total_nnz > nr ? total_nnz : nr;
  hipLaunchKernelGGL(csr_batch_assemble_ragged_kernel, dim3((unsigned)ceil_div64(work, 256)), dim3(256), 0, as_stream(stream),
                     sel, node_base, nnz_base, B, G, total_nodes, total_nnz, store_node_off, store_nnz_off, rowptr, rowptr_t,
                     col, col_t, val, val_t, perm_t, rowptr_out, rowptr_t_out, col_out, col_t_out, val_out, val_t_out,
                     perm_t_out, row_index_out);
  return isic_launch_status();
}

}  // extern "C"
