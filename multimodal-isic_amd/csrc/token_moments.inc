// The token statistics of ONE staged slab: what isic_token_moments_f32 (token_moments.hip) and the masked and ragged entries
// (token_moments_ragged.hip) run once the tokens of an image lie in LDS as [n][W] floats.  One source text for the three
// kernels, so that a row over n tokens has the same bits whichever of them staged it: the summation order depends on n and
// W alone.  Included inside an anonymous namespace, after common.h; the includer defines MOMENTS_BLOCK threads per block.
//
//   * stage_rows.  Tile row i is row `row_of(i)` of the source (the identity for a dense image or a ragged segment, the
//     list of kept token ids for a masked one), 16-byte loads along D when `vec`, element loads otherwise.  Channels past D
//     are staged as zeros and never written out.
//   * moments_of_tile.  Thread (g, c) = (tid / W, tid % W) owns channel c of the slab and the rows g, g + G, ... with
//     G = 256 / W.  Every thread adds its rows in ascending order; the G partials of a channel are parked in LDS and EVERY
//     thread of the channel adds them in ascending g, so all of them hold the same bits without a broadcast.  Sum and max
//     first; with the mean known, sum c^2, sum c^3, sum c^4 in a second walk over the tile.
//   * Median.  Each thread turns its own tile elements into KEYS in place (unsigned order == IEEE order of finite fp32: a
//     negative pattern is complemented, a positive one gets its sign bit set).  The key of rank k = (n - 1) / 2 is found four
//     bits per pass from the top: the threads of a channel add their candidates (keys that agree with the decided prefix)
//     into the channel's 16 bins by the next digit (integer LDS adds, two 16-bit bins per word: the order cannot change a
//     count); every thread of the channel then walks the bins upwards, the digit is the bin in which the running count
//     passes k, and k drops by the count below it.  Equal keys stay candidates together, so any number of ties is exact.
//     The walk stops once every channel of the block has a single candidate (or after the last digit); the candidates' key
//     is then the median.  The bins live in the words the moment partials used.
//   * n == 1 with `unbiased` (which only the masked and ragged entries can meet: the dense one rejects it by value): the
//     variance is 0 / 0, and fmaxf(NaN, eps) would turn the NaN into eps, so std, skewness and kurtosis are set to NaN
//     explicitly -- what torch gives (std is NaN and clamp(min=eps) keeps a NaN).

__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// xs: channel d0 of source row 0.  The whole block calls it; the caller places the barrier after it.
template <int W, class RowOf>
__device__ __forceinline__ void stage_rows(const float* xs, int64_t ldx, int n, int D, int d0, int vec, float* tile,
                                           RowOf row_of) {
  constexpr int W4 = W / 4;
  const int tid = threadIdx.x;
  if (vec) {
    // four vectors per thread and step, in three phases: the source rows first (a masked image reads them from its list in
    // LDS, and a read of the list cannot be moved above a store to the tile), then the four loads, then the four stores, so
    // that the loads are in flight together
    constexpr int STEP = 4;
    const int q = (tid % W4) * 4;                // MOMENTS_BLOCK % W4 == 0: the same channels in every step
    const int total = n * W4;
    for (int e0 = tid; e0 < total; e0 += STEP * MOMENTS_BLOCK) {
      const float* src[STEP];
      f32x4 v[STEP];
#pragma unroll
      for (int i = 0; i < STEP; ++i) {
        const int e = e0 + i * MOMENTS_BLOCK;
        src[i] = xs + (int64_t)row_of(e < total ? e / W4 : 0) * ldx + q;
      }
#pragma unroll
      for (int i = 0; i < STEP; ++i) {
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e0 + i * MOMENTS_BLOCK < total) {
          if (d0 + q + 3 < D) {
            v[i] = *reinterpret_cast<const f32x4*>(src[i]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (d0 + q + j < D) v[i][j] = src[i][j];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < STEP; ++i) {
        const int e = e0 + i * MOMENTS_BLOCK;
        if (e < total) *reinterpret_cast<f32x4*>(&tile[(e / W4) * W + q]) = v[i];
      }
    }
  } else {
#pragma unroll 4
    for (int e = tid; e < n * W; e += MOMENTS_BLOCK) {
      const int t = e / W, q = e % W;
      tile[e] = (d0 + q < D) ? xs[(int64_t)row_of(t) * ldx + q] : 0.f;
    }
  }
}

// tile: [n][W] staged and visible to the block (a barrier lies between the staging and this call), n >= 1.  orow: the
// output row of the image, orow[s D + d].  The whole block calls it with the same n.
template <int W>
__device__ __forceinline__ void moments_of_tile(float* tile, int n_tok, int D, int d0, float eps, int unbiased,
                                                float* orow) {
  constexpr int BLOCK = MOMENTS_BLOCK;
  constexpr int G = BLOCK / W;                 // threads per channel
  __shared__ float part[3][BLOCK];             // [.][g * W + c]
  __shared__ unsigned med[W];
  const int tid = threadIdx.x, c = tid % W, g = tid / W;
  const int T = n_tok;

  float* col = tile + c;
  // ---- sum and max
  float s = 0.f, mx = -INFINITY;
#pragma unroll 8
  for (int t = g; t < T; t += G) {
    const float v = col[t * W];
    s += v;
    mx = fmaxf(mx, v);
  }
  part[0][tid] = s;
  part[1][tid] = mx;
  __syncthreads();
  s = part[0][c];
  mx = part[1][c];
#pragma unroll
  for (int j = 1; j < G; ++j) {
    s += part[0][j * W + c];
    mx = fmaxf(mx, part[1][j * W + c]);
  }
  const float mean = s / (float)T;
  __syncthreads();                             // part[] is written again below

  // ---- central power sums; the thread's elements become keys on the way
  float s2 = 0.f, s3 = 0.f, s4 = 0.f;
#pragma unroll 8
  for (int t = g; t < T; t += G) {
    const float v = col[t * W];
    const float cv = v - mean, c2 = cv * cv;
    s2 += c2;
    s3 += c2 * cv;
    s4 += c2 * c2;
    col[t * W] = __uint_as_float(key_of(v));   // only this thread reads or writes the element until the last scan
  }
  part[0][tid] = s2;
  part[1][tid] = s3;
  part[2][tid] = s4;
  __syncthreads();
  s2 = part[0][c];
  s3 = part[1][c];
  s4 = part[2][c];
#pragma unroll
  for (int j = 1; j < G; ++j) {
    s2 += part[0][j * W + c];
    s3 += part[1][j * W + c];
    s4 += part[2][j * W + c];
  }

  // ---- median: the key of rank k, one 4-bit digit per pass
  unsigned* hist = reinterpret_cast<unsigned*>(&part[0][0]);   // [8][W] words, two 16-bit bins each (a count is <= T <= 1024)
  const unsigned* kcol = reinterpret_cast<const unsigned*>(col);
  unsigned prefix = 0u, mask = 0u;
  int k = (T - 1) / 2, ncand = T;
  for (int shift = 28; shift >= 0; shift -= 4) {
    // (the barrier also separates the reads of part[] above and of hist[] in the previous pass from the zeroing below)
    if (!__syncthreads_or(ncand > 1)) break;
    for (int i = tid; i < 8 * W; i += BLOCK) hist[i] = 0u;
    __syncthreads();
#pragma unroll 8
    for (int t = g; t < T; t += G) {
      const unsigned key = kcol[t * W];
      if ((key & mask) == prefix) {
        const unsigned d = (key >> shift) & 15u;
        atomicAdd(&hist[(d >> 1) * W + c], 1u << ((d & 1u) * 16u));   // integer: the order cannot change the counts
      }
    }
    __syncthreads();
    int below = 0, digit = 0, count = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned w = hist[j * W + c];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int n = (int)((w >> (16 * h)) & 0xFFFFu);
        if (!found) {
          if (k < below + n) {
            found = true;
            digit = 2 * j + h;
            count = n;
          } else {
            below += n;
          }
        }
      }
    }
    k -= below;                                // (k < ncand always holds, so a digit is found)
    ncand = count;
    prefix |= (unsigned)digit << shift;
    mask |= 15u << shift;
  }
  // the candidates all hold one key (a single one is left, or every bit is decided): whoever owns one publishes it
#pragma unroll 8
  for (int t = g; t < T; t += G) {
    const unsigned key = kcol[t * W];
    if ((key & mask) == prefix) med[c] = key;
  }
  __syncthreads();

  if (g == 0 && d0 + c < D) {
    const float var = s2 / (float)(T - unbiased);
    const float sd = sqrtf(var);
    const float sigma = fmaxf(sd, eps);
    const float sg2 = sigma * sigma;
    const float n = (float)T;
    const bool lone = unbiased && T == 1;      // 0 / 0 above: fmaxf would hide the NaN behind eps
    const float qnan = __uint_as_float(0x7FC00000u);
    float* o = orow + d0 + c;
    o[0] = mean;
    o[(int64_t)D] = mx;
    o[(int64_t)2 * D] = lone ? qnan : sd;
    o[(int64_t)3 * D] = value_of(med[c]);
    o[(int64_t)4 * D] = lone ? qnan : (s3 / n) / (sg2 * sigma);
    o[(int64_t)5 * D] = lone ? qnan : (s4 / n) / (sg2 * sg2) - 3.f;
  }
}
