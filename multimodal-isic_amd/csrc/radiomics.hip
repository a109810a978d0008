// Radiomic features of the lesions of a resident uint8 pool (include/isic_hip_radiomics.h): first-order, GLCM and GLDM of
// the gray, red, green and blue channel, one workgroup of 512 threads per image, one launch.
//
// Counting.  The image is walked in tiles of TH x TW pixels.  A tile is staged with a halo of one pixel: a thread reads the
// mask byte and, inside the ROI, the three colour bytes of a pixel, forms the gray value and leaves ONE word in LDS -- the
// absolute bins v / bin_width of the four channels, a byte each, or NONE outside the ROI or the image (the loads of a tile are
// all issued before the first is used, colour bytes whatever the mask says; the padded tile is 32 x 64 words, four cells a
// thread).  Interior pixels add
// their raw values to the four histograms on the way.  Then every interior ROI pixel looks at its eight neighbours in LDS:
// the four forward ones (0,1), (1,-1), (1,0), (1,1) give the GLCM pairs, all eight the GLDM dependence count.  A pair is met
// once, from its first pixel, and goes into a TRIANGULAR matrix (cell (max, min)): the symmetric matrix of the header is
// tri + tri^T, so the diagonal doubles.  16 triangles of 528 counters are 33 KiB where 16 full matrices would be 64.  All
// counters are integers in LDS (ds_add_u32): no order of additions can change them.  v / bin_width is (v * m) >> 16 with
// m = 65536 / bin_width + 1, exact for v < 256 and bin_width >= 8 (the error of m, below 1 / 65536 per unit of v, stays
// below the 1 / bin_width that separates v / bin_width from the next integer).
//
// Features.  Wave w takes GLCM angle w & 3 of two channels, 2 (w >> 2) and the next; waves 0..3 then take first-order and
// GLDM of channel w.  Inside a wave lane a stands for bin a (or for a difference / sum index, or for four histogram values),
// marginals are exact integer sums, the fp64 sums over lanes are butterflies of a fixed shape.  MCC: the wave builds M of
// both its channels over the levels of the ROI as packed lower triangles of doubles in LDS and runs cyclic Jacobi on the
// two side by side, one in each half-wave, lane k of a half updating elements (k, p) and (k, q) of a rotation: the 16
// matrices of an image are worked on at once.  After one barrier 96 threads average the angles.  111 KiB of static LDS:
// gfx950 gives a workgroup up to the 160 KiB of its compute unit, and the registers allow one workgroup a CU anyway.
#include "common.h"
#include "../../include/isic_hip_radiomics.h"

#include <limits.h>

namespace {

constexpr int BLOCK = 512;
constexpr int TH = ISIC_RADIOMICS_TILE_H, TW = ISIC_RADIOMICS_TILE_W, PH = TH + 2, PW = TW + 2;
constexpr int L = ISIC_RADIOMICS_MAX_LEVELS, TRI = L * (L + 1) / 2;
constexpr int NFO = 18, NGLCM = 24, NGLDM = 14, NF = ISIC_RADIOMICS_FEATURES;
constexpr int NCOUNT = ISIC_RADIOMICS_COUNTS;
constexpr unsigned NONE = 0xFFFFFFFFu;          // bins are below 32: no byte of a real word is 0xFF
constexpr int JACOBI_SWEEPS = 40;
constexpr int CELLS = PH * PW / BLOCK;           // tile cells, halo included, per thread
static_assert(PH * PW == CELLS * BLOCK && PW == 64, "a tile with its halo is 32 x 64 words: four cells a thread, no remainder");
static_assert(NF == NFO + NGLCM + NGLDM && NCOUNT == 256 + 4 * L * L + L * 9 && L == 32, "the header's layout");
static_assert(BLOCK == 8 * ISIC_WAVE, "wave w: GLCM angle w & 3 of channels 2 (w >> 2) and 2 (w >> 2) + 1");

struct Shared {
  int tri[4][4][TRI];                           // [channel][angle][(max, min)]
  int hist[4][256];
  int gldm[4][L][9];
  union {
    unsigned tile[PH * PW];                     // counting
    double jac[16][TRI];                        // features: one packed matrix per half-wave, all 16 at once
  } u;
  double glcm_f[4][4][NGLCM];                   // [channel][angle][feature]
  int angle_ok[4][4];
};
static_assert(sizeof(Shared) <= 163840, "static LDS: gfx950 gives a workgroup up to the 160 KiB of its compute unit");

__device__ __forceinline__ int tri_at(int hi, int lo) { return hi * (hi + 1) / 2 + lo; }

// a compiler and LDS fence inside one wave: what other lanes wrote before it is visible after it
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

__device__ __forceinline__ double wsum(double v) { return wave_sum_f64(v); }
__device__ __forceinline__ double wmax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ long long wsum_i(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wmin_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wmax_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

constexpr double EPS = 2.220446049250313e-16;   // 2^-52
__device__ __forceinline__ double plog(double p) { return p * log2(p + EPS); }
__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7FF8000000000000ll); }

// What every feature wave needs of its channel: the ROI size, the bin totals, the levels present and the level offset.
struct ChannelInfo {
  long long N;
  int vmin, vmax, lo, Ng;
  unsigned present;                             // bit a: bin a has an ROI pixel
  long long nb;                                 // lane a < 32: pixels of bin a
};

__device__ __forceinline__ ChannelInfo channel_info(const Shared& s, int c, int bw, int lane) {
  ChannelInfo ci;
  int vmin = 256, vmax = -1;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int v = lane + 64 * r;
    if (s.hist[c][v] > 0) {
      vmin = min(vmin, v);
      vmax = max(vmax, v);
    }
  }
  ci.vmin = wmin_i(vmin);
  ci.vmax = wmax_i(vmax);
  long long nb = 0;
  if (lane < L)
#pragma unroll
    for (int j = 0; j < 9; ++j) nb += s.gldm[c][lane][j];
  ci.nb = nb;
  ci.N = wsum_i(nb);
  ci.present = (unsigned)(__ballot(lane < L && nb > 0) & 0xFFFFFFFFull);
  ci.lo = ci.vmin / bw;
  ci.Ng = ci.vmax / bw - ci.lo + 1;
  return ci;
}

// ------------------------------------------------------------------------------------------------ first-order
// the order statistics of 0-based ranks lo <= hi in one walk: the smallest v whose cumulative count exceeds the rank
__device__ __forceinline__ void values_at_ranks(const int* hist, long long lo, long long hi, int& vlo, int& vhi) {
  long long cum = 0;
  vlo = vhi = 255;
  bool have_lo = false;
  for (int v = 0; v < 256; ++v) {
    cum += hist[v];
    if (!have_lo && cum > lo) {
      vlo = v;
      have_lo = true;
    }
    if (cum > hi) {
      vhi = v;
      return;
    }
  }
}

// numpy.percentile(x, 100 q), method 'linear': virtual index (n - 1) q, then numpy's two-sided lerp.  The products
// and sums are written with the rounding intrinsics so that no fma is contracted into them: the bits are the ones numpy forms.
__device__ __forceinline__ double percentile(const int* hist, long long n, double q) {
  const double vi = __dmul_rn((double)(n - 1), q);
  double fl = floor(vi);
  if (fl < 0.0) fl = 0.0;
  long long lo = (long long)fl;
  if (lo > n - 1) lo = n - 1;
  const long long hi = lo + 1 > n - 1 ? n - 1 : lo + 1;
  const double g = __dadd_rn(vi, -fl);
  int vlo, vhi;
  values_at_ranks(hist, lo, hi, vlo, vhi);
  const double a = (double)vlo, b = (double)vhi;
  const double d = b - a;
  return g >= 0.5 ? __dadd_rn(b, -__dmul_rn(d, __dadd_rn(1.0, -g))) : __dadd_rn(a, __dmul_rn(d, g));
}

__device__ void first_order(const Shared& s, int c, const ChannelInfo& ci, int lane, double* out) {
  const int* hist = s.hist[c];
  const double N = (double)ci.N;
  long long s1 = 0, s2 = 0;
  int hv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int v = lane + 64 * r;
    hv[r] = hist[v];
    s1 += (long long)hv[r] * v;
    s2 += (long long)hv[r] * v * v;
  }
  s1 = wsum_i(s1);
  s2 = wsum_i(s2);
  const double mean = (double)s1 / N, energy = (double)s2;
  double m2 = 0, m3 = 0, m4 = 0, mad = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double h = (double)hv[r], d = (double)(lane + 64 * r) - mean, d2 = d * d;
    m2 += h * d2;
    m3 += h * d2 * d;
    m4 += h * d2 * d2;
    mad += h * fabs(d);
  }
  m2 = wsum(m2) / N;
  m3 = wsum(m3) / N;
  m4 = wsum(m4) / N;
  mad = wsum(mad) / N;
  // lanes 0..4: the 10th, 25th, 50th, 75th and 90th percentile
  const double qs[5] = {0.1, 0.25, 0.5, 0.75, 0.9};
  double pc = 0.0;
  if (lane < 5) pc = percentile(hist, ci.N, qs[lane]);
  const double p10 = __shfl(pc, 0, 64), p25 = __shfl(pc, 1, 64), p50 = __shfl(pc, 2, 64), p75 = __shfl(pc, 3, 64),
               p90 = __shfl(pc, 4, 64);
  // the values inside [P10, P90], about their own mean
  long long rn = 0, rs = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int v = lane + 64 * r;
    if ((double)v >= p10 && (double)v <= p90) {
      rn += hv[r];
      rs += (long long)hv[r] * v;
    }
  }
  rn = wsum_i(rn);
  rs = wsum_i(rs);
  const double rmean = (double)rs / (double)rn;
  double rmad = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int v = lane + 64 * r;
    if ((double)v >= p10 && (double)v <= p90) rmad += (double)hv[r] * fabs((double)v - rmean);
  }
  rmad = wsum(rmad) / (double)rn;
  // the discretised histogram
  const double pb = lane < L ? (double)ci.nb / N : 0.0;
  const double entropy = -wsum(plog(pb)), uniformity = wsum(pb * pb);
  if (lane == 0) {
    out[0] = p10;
    out[1] = p90;
    out[2] = energy;
    out[3] = entropy;
    out[4] = p75 - p25;
    out[5] = m2 == 0.0 ? 0.0 : m4 / (m2 * m2);
    out[6] = (double)ci.vmax;
    out[7] = mad;
    out[8] = mean;
    out[9] = p50;
    out[10] = (double)ci.vmin;
    out[11] = (double)(ci.vmax - ci.vmin);
    out[12] = rmad;
    out[13] = sqrt(energy / N);
    out[14] = m2 == 0.0 ? 0.0 : m3 / (m2 * sqrt(m2));
    out[15] = energy;
    out[16] = uniformity;
    out[17] = m2;
  }
}

// ------------------------------------------------------------------------------------------------ GLDM
__device__ void gldm_features(const Shared& s, int c, const ChannelInfo& ci, int lane, double* out) {
  const double Nz = (double)ci.N;
  const bool row = lane < L && ci.nb > 0;         // a level of the ROI: i >= 1
  const double i = (double)(lane - ci.lo + 1), i2 = i * i;
  double P[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) P[j] = row ? (double)s.gldm[c][lane][j] : 0.0;
  long long col = 0;                              // lane j < 9: pixels with dependence j + 1
  if (lane < 9)
    for (int a = 0; a < L; ++a) col += s.gldm[c][a][lane];
  const double cj = (double)col, nb = row ? (double)ci.nb : 0.0;
  const double dn = wsum(cj * cj), gln = wsum(nb * nb);
  const double mu_j = wsum(cj * (double)(lane + 1)) / Nz, mu_i = wsum(nb * i) / Nz;
  double de = 0, dv = 0, glv = 0, hgle = 0, lde = 0, ldhgle = 0, ldlgle = 0, lgle = 0, sde = 0, sdhgle = 0, sdlgle = 0;
  if (row) {
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const double p = P[j] / Nz, jj = (double)(j + 1), j2 = jj * jj;
      de -= plog(p);
      dv += p * (jj - mu_j) * (jj - mu_j);
      glv += p * (i - mu_i) * (i - mu_i);
      hgle += P[j] * i2;
      lde += P[j] * j2;
      ldhgle += P[j] * i2 * j2;
      ldlgle += P[j] * j2 / i2;
      lgle += P[j] / i2;
      sde += P[j] / j2;
      sdhgle += P[j] * i2 / j2;
      sdlgle += P[j] / (i2 * j2);
    }
  }
  de = wsum(de); dv = wsum(dv); glv = wsum(glv); hgle = wsum(hgle); lde = wsum(lde); ldhgle = wsum(ldhgle);
  ldlgle = wsum(ldlgle); lgle = wsum(lgle); sde = wsum(sde); sdhgle = wsum(sdhgle); sdlgle = wsum(sdlgle);
  if (lane == 0) {
    out[0] = de;
    out[1] = dn / Nz;
    out[2] = dn / (Nz * Nz);
    out[3] = dv;
    out[4] = gln / Nz;
    out[5] = glv;
    out[6] = hgle / Nz;
    out[7] = lde / Nz;
    out[8] = ldhgle / Nz;
    out[9] = ldlgle / Nz;
    out[10] = lgle / Nz;
    out[11] = sde / Nz;
    out[12] = sdhgle / Nz;
    out[13] = sdlgle / Nz;
  }
}

// ------------------------------------------------------------------------------------------------ GLCM, one angle
// The second largest |eigenvalue| of M = D^-1/2 P D^-1/2 over the n levels of the ROI, for TWO matrices at once: lanes 0..31
// of the wave work on one (tri, present, r, m), lanes 32..63 on another; hl = lane & 31.  r: lane hl's row sum of the symmetric
// counts.  M lies packed in `m` ((u, v) with v <= u at u (u + 1) / 2 + v).  Every loop bound and every branch that holds a
// cross-lane operation is uniform over the wave (the longer of the two matrices sets the trip counts, __all / __any decide);
// what differs between the halves is predicated.  A matrix of fewer than two levels is done at once and answers 1.
__device__ __forceinline__ double hsum(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double hmax(double v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ double mcc_pair(const int* tri, unsigned present, long long r, int lane, double* m) {
  const int hl = lane & 31;
  const int n = __popc(present);
  const bool mine = (present >> hl) & 1u;
  const int u = __popc(present & ((1u << hl) - 1u));
  const double rd = (double)r;
  for (int b = 0; b < L; ++b) {
    const double rb = __shfl(rd, b, 32);          // of this half
    const int v = __popc(present & ((1u << b) - 1u));
    if (mine && ((present >> b) & 1u) && b <= hl) {
      const int cnt = tri[tri_at(hl, b)] * (b == hl ? 2 : 1);
      m[tri_at(u, v)] = (rd > 0.0 && rb > 0.0) ? (double)cnt / sqrt(rd * rb) : 0.0;
    }
  }
  wave_lds_sync();
  const int nmax = max(n, __shfl_xor(n, 32, 64));
  bool done = n < 2;
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    double off = 0.0;
    if (!done && hl < n)
      for (int v = 0; v < hl; ++v) off += m[tri_at(hl, v)] * m[tri_at(hl, v)];
    off = hsum(off);
    done = done || off < 1e-30;                   // |entries| <= 1: the diagonal is the spectrum to 1e-15 at the worst
    if (__all(done)) break;
    for (int p = 0; p < nmax - 1; ++p)
      for (int q = p + 1; q < nmax; ++q) {
        const bool in = !done && q < n;
        const double apq = in ? m[tri_at(q, p)] : 0.0;
        const bool rot = in && apq != 0.0;        // the same in every lane of a half
        if (!__any(rot)) continue;
        if (rot) {
          const double app = m[tri_at(p, p)], aqq = m[tri_at(q, q)];
          const double theta = (aqq - app) / (2.0 * apq);
          const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
          if (hl < n && hl != p && hl != q) {
            const int ip = hl > p ? tri_at(hl, p) : tri_at(p, hl), iq = hl > q ? tri_at(hl, q) : tri_at(q, hl);
            const double akp = m[ip], akq = m[iq];
            m[ip] = cs * akp - sn * akq;
            m[iq] = sn * akp + cs * akq;
          }
          if (hl == 0) {
            m[tri_at(p, p)] = app - t * apq;
            m[tri_at(q, q)] = aqq + t * apq;
            m[tri_at(q, p)] = 0.0;
          }
        }
        wave_lds_sync();
      }
  }
  const double e = (n >= 2 && hl < n) ? fabs(m[tri_at(hl, hl)]) : -1.0;
  const double e1 = hmax(e);
  const unsigned top = (unsigned)((__ballot(e == e1) >> (lane & 32)) & 0xFFFFFFFFull);
  const int first = __ffs((int)top) - 1;
  const double e2 = hmax(hl == first ? -1.0 : e);
  return n < 2 ? 1.0 : e2;
}

// Everything of one angle of one channel but MCC; -> lane a's row sum of the symmetric counts (0 everywhere without a pair).
__device__ long long glcm_angle(Shared& s, int c, int k, const ChannelInfo& ci, int lane) {
  const int* tri = s.tri[c][k];
  double* out = s.glcm_f[c][k];
  const bool act = lane < L;
  const int a = lane & 31;
  auto sym = [&](int x, int y) { return x == y ? 2 * tri[tri_at(x, x)] : tri[tri_at(max(x, y), min(x, y))]; };
  long long r = 0;                                // row sum of bin a
  if (act)
    for (int b = 0; b < L; ++b) r += sym(a, b);
  const long long Sn = wsum_i(r);
  if (Sn == 0) {                                  // no pair in this angle
    if (lane == 0) s.angle_ok[c][k] = 0;
    return 0;
  }
  const double S = (double)Sn, Ng = (double)ci.Ng;
  const double i = (double)(a - ci.lo + 1), px = act ? (double)r / S : 0.0;
  const double ux = wsum(i * px);
  const double var = wsum((i - ux) * (i - ux) * px);
  const double hx = -wsum(plog(px));
  double ac = 0, cp = 0, csh = 0, ct = 0, corm = 0, je = 0, hxy = 0, hxy1 = 0, hxy2 = 0, mp = 0;
  for (int b = 0; b < L; ++b) {
    const double pxb = __shfl(px, b, 64);
    if (!act) continue;
    const double p = (double)sym(a, b) / S, j = (double)(b - ci.lo + 1);
    const double e = i + j - 2.0 * ux, e2 = e * e, pp = px * pxb;
    ac += p * i * j;
    cp += e2 * e2 * p;
    csh += e2 * e * p;
    ct += e2 * p;
    corm += p * (i - ux) * (j - ux);
    je += p * p;
    hxy -= plog(p);
    hxy1 -= p * log2(pp + EPS);
    hxy2 -= plog(pp);
    mp = fmax(mp, p);
  }
  ac = wsum(ac); cp = wsum(cp); csh = wsum(csh); ct = wsum(ct); corm = wsum(corm); je = wsum(je); hxy = wsum(hxy);
  hxy1 = wsum(hxy1); hxy2 = wsum(hxy2); mp = wmax(mp);
  // p_{x-y}(kd), kd = lane < 32
  long long dcount = 0;
  if (act)
    for (int x = 0; x + a < L; ++x) dcount += (long long)sym(x, x + a) * (a ? 2 : 1);
  const double kd = (double)a, pd = act ? (double)dcount / S : 0.0;
  const double contrast = wsum(kd * kd * pd), da = wsum(kd * pd), dent = -wsum(plog(pd));
  const double dvar = wsum((kd - da) * (kd - da) * pd);
  const double id = wsum(pd / (1.0 + kd)), idm = wsum(pd / (1.0 + kd * kd));
  const double idmn = wsum(pd / (1.0 + kd * kd / (Ng * Ng))), idn = wsum(pd / (1.0 + kd / Ng));
  const double iv = wsum(act && a >= 1 ? pd / (kd * kd) : 0.0);
  // p_{x+y}(ks), bins x + y = lane < 63
  long long scount = 0;
  if (lane < 2 * L - 1)
    for (int x = max(0, lane - (L - 1)); x <= min(L - 1, lane); ++x) scount += sym(x, lane - x);
  const double ks = (double)(lane - 2 * ci.lo + 2), ps = (double)scount / S;
  const double sa = wsum(ks * ps), se = -wsum(plog(ps));
  if (lane == 0) {
    out[0] = ac;
    out[1] = cp;
    out[2] = csh;
    out[3] = ct;
    out[4] = contrast;
    out[5] = var == 0.0 ? 1.0 : corm / var;       // sigma_x = sigma_y: the matrix is symmetric
    out[6] = da;
    out[7] = dent;
    out[8] = dvar;
    out[9] = id;
    out[10] = idm;
    out[11] = idmn;
    out[12] = idn;
    out[13] = hx == 0.0 ? 0.0 : (hxy - hxy1) / hx;
    out[14] = hxy2 < hxy ? 0.0 : sqrt(1.0 - exp(-2.0 * (hxy2 - hxy)));
    out[15] = iv;
    out[16] = ux;
    out[17] = je;
    out[18] = hxy;
    out[20] = mp;
    out[21] = sa;
    out[22] = se;
    out[23] = var;
    s.angle_ok[c][k] = 1;
  }
  return r;
}

// ------------------------------------------------------------------------------------------------ the kernel
__global__ __launch_bounds__(BLOCK) void radiomics_u8_kernel(const uint8_t* __restrict__ pixels, const uint8_t* __restrict__ masks,
                                                             const int64_t* __restrict__ offsets, const int32_t* __restrict__ hw,
                                                             int64_t n_pool, const int64_t* __restrict__ index, int bw, int label,
                                                             double* __restrict__ out, int32_t* __restrict__ counts,
                                                             unsigned long long* __restrict__ n_empty) {
  __shared__ Shared s;
  const int tid = threadIdx.x, lane = tid % ISIC_WAVE, wave = tid / ISIC_WAVE;
  const int64_t b = blockIdx.x;
  int64_t n = index[b];
  n = n < 0 ? 0 : (n >= n_pool ? n_pool - 1 : n);
  const int h = max(hw[2 * n], 0), w = max(hw[2 * n + 1], 0);
  const uint8_t* img = pixels + 3 * offsets[n];
  const uint8_t* msk = masks + offsets[n];
  const unsigned mul = 65536u / (unsigned)bw + 1u;

  for (int i = tid; i < 4 * 4 * TRI; i += BLOCK) (&s.tri[0][0][0])[i] = 0;
  for (int i = tid; i < 4 * 256; i += BLOCK) (&s.hist[0][0])[i] = 0;
  for (int i = tid; i < 4 * L * 9; i += BLOCK) (&s.gldm[0][0][0])[i] = 0;
  __syncthreads();

  // ---- counting
  for (int ty = 0; ty < h; ty += TH)
    for (int tx = 0; tx < w; tx += TW) {
      // every load of the tile is issued before the first is used: the mask byte and the three colour bytes of up to
      // CELLS cells per thread, whatever the mask says (a cell outside the image reads pixel 0 and is dropped below)
      unsigned mb[CELLS], cr[CELLS], cg[CELLS], cb[CELLS];
#pragma unroll
      for (int i = 0; i < CELLS; ++i) {
        const int cell = tid + i * BLOCK;
        const int r = cell / PW, c = cell - r * PW;
        const int y = ty - 1 + r, x = tx - 1 + c;
        const bool in = y >= 0 && y < h && x >= 0 && x < w;
        const int64_t p = in ? (int64_t)y * w + x : 0;
        mb[i] = msk[p];
        cr[i] = img[3 * p];
        cg[i] = img[3 * p + 1];
        cb[i] = img[3 * p + 2];
      }
#pragma unroll
      for (int i = 0; i < CELLS; ++i) {
        const int cell = tid + i * BLOCK;
        const int r = cell / PW, c = cell - r * PW;
        const int y = ty - 1 + r, x = tx - 1 + c;
        unsigned word = NONE;
        if (y >= 0 && y < h && x >= 0 && x < w && mb[i] == (unsigned)label) {
          const unsigned R = cr[i], G = cg[i], B = cb[i];
          const unsigned gray = (4899u * R + 9617u * G + 1868u * B + 8192u) >> 14;
          word = ((gray * mul) >> 16) | (((R * mul) >> 16) << 8) | (((G * mul) >> 16) << 16) | (((B * mul) >> 16) << 24);
          if (r >= 1 && r <= TH && c >= 1 && c <= TW) {
            atomicAdd(&s.hist[0][gray], 1);
            atomicAdd(&s.hist[1][R], 1);
            atomicAdd(&s.hist[2][G], 1);
            atomicAdd(&s.hist[3][B], 1);
          }
        }
        s.u.tile[cell] = word;
      }
      __syncthreads();
      for (int cell = tid; cell < TH * TW; cell += BLOCK) {
        const int r = cell / TW + 1, c = cell % TW + 1;
        const unsigned* t = s.u.tile + r * PW + c;
        const unsigned wp = t[0];
        if (wp == NONE) continue;
        const unsigned fwd[4] = {t[1], t[PW - 1], t[PW], t[PW + 1]};             // (0,1) (1,-1) (1,0) (1,1)
        const unsigned back[4] = {t[-1], t[-PW + 1], t[-PW], t[-PW - 1]};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
          const int a = (wp >> (8 * ch)) & 0xFFu;
          int dep = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int q = (fwd[k] >> (8 * ch)) & 0xFFu;                           // 0xFF outside the ROI: never a bin
            if (fwd[k] != NONE) atomicAdd(&s.tri[ch][k][tri_at(max(a, q), min(a, q))], 1);
            dep += (q == a) + ((int)((back[k] >> (8 * ch)) & 0xFFu) == a);
          }
          atomicAdd(&s.gldm[ch][a][dep], 1);
        }
      }
      __syncthreads();
    }

  // ---- the integer matrices, if asked for
  if (counts) {
    int32_t* dst = counts + b * 4 * NCOUNT;
    for (int i = tid; i < 4 * NCOUNT; i += BLOCK) {
      const int ch = i / NCOUNT, r = i - ch * NCOUNT;
      int v;
      if (r < 256) {
        v = s.hist[ch][r];
      } else if (r < 256 + 4 * L * L) {
        const int k = (r - 256) / (L * L), x = ((r - 256) / L) % L, y = (r - 256) % L;
        v = s.tri[ch][k][tri_at(max(x, y), min(x, y))] * (x == y ? 2 : 1);
      } else {
        v = (&s.gldm[ch][0][0])[r - 256 - 4 * L * L];
      }
      dst[i] = v;
    }
  }

  double* orow = out + b * 4 * NF;
  // the gray histogram is empty exactly when the ROI is: the same answer in every thread, the block leaves together
  const int any = __syncthreads_or(tid < 256 && s.hist[0][tid] != 0);
  if (!any) {
    for (int i = tid; i < 4 * NF; i += BLOCK) orow[i] = qnan();
    if (tid == 0) atomicAdd(n_empty, 1ull);
    return;
  }

  // ---- features (the tile is dead: its memory holds the Jacobi matrices now)
  {
    // wave w: angle w & 3 of the channels c0 and c0 + 1; their two Jacobi matrices run side by side in the half-waves
    const int k = wave & 3, c0 = 2 * (wave >> 2);
    const ChannelInfo ci0 = channel_info(s, c0, bw, lane), ci1 = channel_info(s, c0 + 1, bw, lane);
    const long long r0 = glcm_angle(s, c0, k, ci0, lane), r1 = glcm_angle(s, c0 + 1, k, ci1, lane);
    const long long r1up = __shfl(r1, lane & 31, 64);             // lane 32 + a receives row sum a of the second channel
    const int half = lane >> 5;
    static_assert(sizeof(s.u.jac) / sizeof(s.u.jac[0]) == 2 * (BLOCK / ISIC_WAVE), "one matrix per half-wave");
    const double mcc = mcc_pair(s.tri[c0 + half][k], half ? ci1.present : ci0.present, half ? r1up : r0, lane,
                                s.u.jac[2 * wave + half]);
    if ((lane & 31) == 0) s.glcm_f[c0 + half][k][19] = mcc;
  }
  if (wave < 4) {                                                 // first-order and GLDM of channel `wave`
    const int c = wave;
    const ChannelInfo ci = channel_info(s, c, bw, lane);
    first_order(s, c, ci, lane, orow + c * NF);
    gldm_features(s, c, ci, lane, orow + c * NF + NFO + NGLCM);
  }
  __syncthreads();
  if (tid < 4 * NGLCM) {
    const int c = tid / NGLCM, f = tid % NGLCM;
    double sum = 0.0;
    int na = 0;
    for (int k = 0; k < 4; ++k)
      if (s.angle_ok[c][k]) {
        sum += s.glcm_f[c][k][f];
        ++na;
      }
    orow[c * NF + NFO + f] = na ? sum / (double)na : qnan();
  }
}

}  // namespace

extern "C" int isic_radiomics_u8(const uint8_t* pixels, const uint8_t* masks, const int64_t* offsets, const int32_t* hw,
                                 int64_t n_pool, const int64_t* index, int64_t B, int bin_width, int label, double* out,
                                 int32_t* counts, int64_t* n_empty, void* stream) {
  ISIC_CHECK_ARG(B >= 0 && n_pool >= 0);
  ISIC_CHECK_ARG(bin_width >= 8 && bin_width <= 255);
  ISIC_CHECK_ARG(label >= 1 && label <= 255);
  if (B == 0) return ISIC_OK;
  ISIC_CHECK_ARG(n_pool >= 1 && pixels && masks && offsets && hw && index && out && n_empty);
  ISIC_CHECK_ARG(B <= (int64_t)INT_MAX);
  hipLaunchKernelGGL(radiomics_u8_kernel, dim3((unsigned)B), dim3(BLOCK), 0, as_stream(stream), pixels, masks, offsets, hw,
                     n_pool, index, bin_width, label, out, counts, reinterpret_cast<unsigned long long*>(n_empty));
  return isic_launch_status();
}
