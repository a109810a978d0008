// The device text of the Gram k-NN tile (03_build_graphs.py:37-54), shared by csrc/knn_gram.hip (13 waves, persistent over
// graphs) and csrc/knn_ragged.hip (4 / 8 / 13 waves, one graph per workgroup): bit-equality of the two kernels is a property
// of this text, not of two copies.  Included inside the anonymous namespace of a translation unit, after common.h; knn_dist
// is also the distance of the row-tile knn_kernel of csrc/graph.hip.
//
// Layout that every function here assumes: NT waves, wave r owns the row stripe 16 r .. 16 r + 15 against NT column tiles of
// 16 nodes, acc[c] is the 16 x 16 MFMA accumulator (v_mfma_f32_16x16x4_f32) of stripe `wave` against column tile c.  With
// fr = lane & 15, fg = lane >> 4, acc[c][j] is row 16 wave + 4 fg + j x column 16 c + fr: the 16 NT values of a row live
// in the 16 lanes of one DPP row.
//
// The accumulators are taken by reference and only ever indexed by unrolled constants.  A wave-uniform choice among them
// goes through a named copy (`const f32x4 t = acc[c]`): selecting between acc[c] and another value directly lets the
// compiler form a load at a selected address, which puts the whole array into scratch memory.
#ifndef ISIC_KNN_TILE_INC
#define ISIC_KNN_TILE_INC

// ---- the domain: one workgroup holds a whole graph, a row's k neighbours are one per lane of its DPP row
constexpr int KT_MAX_TILES = 13;
constexpr int KT_MAX_NODES = KT_MAX_TILES * 16;          // 208 (ResNet / ViT patch grids: 196)
constexpr int KT_MAX_K = 16;
constexpr int KT_CHUNK_ROW = 128;                        // a K-chunk: 32 floats of every row; D is a whole number of them

inline bool knn_tile_supported(int D, int k, int max_nodes) {
  return D % 32 == 0 && D >= 32 && k >= 1 && k <= KT_MAX_K && max_nodes <= KT_MAX_NODES;
}

// 03_build_graphs.py:47-48: d = (|x_i|^2 + |x_j|^2) - 2 x_i . x_j, clamp(min = 0)
__device__ __forceinline__ float knn_dist(float si, float sj, float dot) { return fmaxf((si + sj) - 2.0f * dot, 0.f); }

template <int CTRL>
__device__ __forceinline__ float kt_dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ int kt_dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }

// ---- staging: a stage holds [16 NT rows][128 B] per K-chunk, the 16-byte chunks XOR-swizzled on the source side so that the
//      ds_read_b128 fragment reads are conflict-free.  Piece h (= 0, 1) of a wave brings rows 16 wave + 8 h + r8, r8 = lane >> 3;
//      the lane fetches global 16-byte chunk p ^ r8 of its row (row & 7 == r8), so that LDS position p = lane & 7 of a row
//      holds chunk p ^ (row & 7).  -> byte offset of the lane's chunk inside the K-chunk of its row
__device__ __forceinline__ unsigned kt_src_chunk(int lane) { return (unsigned)(((lane & 7) ^ (lane >> 3)) << 4); }

// ---- fragment addresses inside a stage: row 16 c + fr, k-quarter kq (16 floats): chunk (4 kq + fg) ^ (fr & 7).
//      -> byte offset for c = 0, kq = 0; tile c adds c * 2048, kq = 1 is ^ 64
__device__ __forceinline__ unsigned kt_foff0(int fr, int fg) { return (unsigned)(fr * KT_CHUNK_ROW + ((fg ^ (fr & 7)) << 4)); }

// ---- one K-chunk of a row stripe against the nt column tiles of its graph (wave-uniform, 1 <= nt <= NT; nt = NT: the tests
//      fold away): two k-quarters, the four MFMAs of a quarter take k = 4 fg + j -- the summation order of a dot product.
//      Four column tiles at a time, so that a tile's accumulator is touched every fourth MFMA (a dependent MFMA issues ~6
//      slots late); tiles at or past nt are stepped over.  QUARTER_FENCE: one quarter's fragments in registers at a time
//      (where the caller wants the registers more than the earlier reads).
template <int NT, bool QUARTER_FENCE>
__device__ __forceinline__ void kt_multiply(int nt, const unsigned char* st, unsigned foff0, int wave, f32x4 (&acc)[NT]) {
#pragma unroll
  for (int kq = 0; kq < 2; ++kq) {
    if (QUARTER_FENCE) __builtin_amdgcn_sched_barrier(0);
    const unsigned char* q = st + (foff0 ^ (unsigned)(kq << 6));
    const f32x4 av = *reinterpret_cast<const f32x4*>(q + wave * 2048);
#pragma unroll
    for (int c0 = 0; c0 < NT; c0 += 4) {
      if (c0 >= nt) break;
      f32x4 bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c0 + i < NT) bv[i] = *reinterpret_cast<const f32x4*>(q + (c0 + i < nt ? c0 + i : c0) * 2048);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (c0 + i < NT) {
            if (c0 + i < nt) acc[c0 + i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[i][j], acc[c0 + i], 0, 0, 0);
          }
    }
  }
}

// ---- |x_i|^2 = G[i][i]: tile (wave, wave), row 4 fg + j == column fr -- the same MFMA summation order as the dot
//      products, so d[i][i] is exactly 0 before it is set to +inf and d is symmetric bit for bit.  `wave` is wave-uniform.
template <int NT>
__device__ __forceinline__ void kt_store_sqn(const f32x4 (&acc)[NT], int wave, int fr, int fg, float* sqn) {
  f32x4 dg = acc[0];
#pragma unroll
  for (int c = 1; c < NT; ++c) {
    const f32x4 t = acc[c];
    dg = wave == c ? t : dg;
  }
  const float dv = (fr & 3) == 0 ? dg[0] : (fr & 3) == 1 ? dg[1] : (fr & 3) == 2 ? dg[2] : dg[3];
  if ((fr >> 2) == fg) sqn[wave * 16 + fr] = dv;
}

// ---- dot products -> distances, in place.  Only the column tiles < nt were multiplied and have a norm (nt = NT: the test
//      folds away); the others, the columns past the graph's N nodes and the diagonal become +inf.
template <int NT>
__device__ __forceinline__ void kt_distances(f32x4 (&acc)[NT], const float* sqn, int wave, int fr, int fg, int nt, int N) {
  float sr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sr[j] = sqn[wave * 16 + fg * 4 + j];
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    const int col = c * 16 + fr;
    const float sc = c < nt ? sqn[col] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = wave * 16 + fg * 4 + j;
      const float dv = knn_dist(sr[j], sc, acc[c][j]);
      acc[c][j] = (col < N && col != q) ? dv : INFINITY;   // 03:49 diagonal; columns past the graph
    }
  }
}

// ---- the k smallest of every row, ascending, ties -> lower index (03:50 topk(largest = False)): k rounds of a local scan
//      and a 4-step DPP row rotation, no LDS, no shuffles.  Lane fr ends with neighbour #fr of its four rows 4 fg + j:
//      res_i = -1 / res_v = +inf where the row has fewer candidates (or fr >= k).  Consumes acc.
template <int NT>
__device__ __forceinline__ void kt_select(f32x4 (&acc)[NT], int fr, int k, int (&res_i)[4], float (&res_v)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { res_i[j] = -1; res_v[j] = INFINITY; }
  for (int round = 0; round < k; ++round) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float bv = acc[0][j];
      int bc = 0;
#pragma unroll
      for (int c = 1; c < NT; ++c) {                       // strict <: the lowest column of this lane wins a tie
        const bool lt = acc[c][j] < bv;
        bv = lt ? acc[c][j] : bv;
        bc = lt ? c : bc;
      }
      int bi = bc * 16 + fr;
      // minimum of (value, index) over the 16 lanes of the DPP row: rotations by 8, 4, 2, 1
#define KT_STEP(CTRL)                                                    \
      {                                                                  \
        const float ov = kt_dpp_f<CTRL>(bv);                             \
        const int oi = kt_dpp_i<CTRL>(bi);                               \
        const bool take = ov < bv || (ov == bv && oi < bi);              \
        bv = take ? ov : bv;                                             \
        bi = take ? oi : bi;                                             \
      }
      KT_STEP(0x128) KT_STEP(0x124) KT_STEP(0x122) KT_STEP(0x121)
#undef KT_STEP
      const bool found = bv < INFINITY;
      if (fr == round) { res_i[j] = found ? bi : -1; res_v[j] = bv; }
      // the owner of the winner retires it
      const bool own = (bi & 15) == fr;
      const int cs = bi >> 4;
#pragma unroll
      for (int c = 0; c < NT; ++c) acc[c][j] = (own && cs == c) ? INFINITY : acc[c][j];
    }
  }
}

#endif  // ISIC_KNN_TILE_INC
