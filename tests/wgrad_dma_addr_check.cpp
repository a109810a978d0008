// Host-side check of the LDS-DMA addresses of the all-taps weight-gradient kernels (csrc/wgrad_dma_addr.inc), built and run by
// tests/test_wgrad_dma_addr_cpu.py with the host compiler.  For every tile, wave, slot, lane, stage and prefetch state of the
// geometries below it requires
//   * per LDS destination: what the kernel's arithmetic (dma) brings there == what the former arithmetic (dma_ref) brought
//     there, lane by lane: operand, validity, byte offset -- and the SET of destinations of a tile is the same;
//   * a valid source lies inside its tensor and inside the block's channel slice of its pixel;
//   * an invalid one lies inside the 2048-byte zero page; padding groups and dead prefetches go to the sink;
//   * every wave issues the same number of DMAs per tile as before (the tile top's vmcnt(0) relies on nothing else).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../multimodal-isic_amd/csrc/wgrad_dma_addr.inc"

namespace {

long long g_checked = 0;
int g_failed = 0;

#define REQUIRE(cond, ...)                                  \
  do {                                                      \
    if (!(cond)) {                                          \
      if (g_failed++ < 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                       \
  } while (0)

struct LaneSrc {
  int op; bool ok; long long off;
  bool operator==(const LaneSrc& o) const { return op == o.op && ok == o.ok && (!ok || off == o.off); }
};
typedef std::map<unsigned, std::vector<LaneSrc>> Image;      // LDS destination -> 64 lane sources

// one geometry of one kernel; K: wga::c128 or wga::s2 through the traits below
struct C128 {
  typedef wga::c128::Geom Geom;
  static constexpr int T_H = wga::c128::T_H, T_W = wga::c128::T_W, NDMA = wga::c128::NDMA, STG = wga::c128::STG, SINK = wga::c128::SINK;
  static constexpr int XSLICE = 256, YSLICE = 128, GROUPS = wga::c128::XGROUPS + wga::c128::YGROUPS;
  static int rows(const Geom& g) { return g.H; }
  static int cols(const Geom& g) { return g.W; }
  static long long xpixels(const Geom& g) { return (long long)g.N * g.H * g.W; }
  static long long ypixels(const Geom& g) { return (long long)g.N * g.H * g.W; }
  static wga::Dma ref(const Geom& g, const wga::Tile& t, int w, int j, int l, int s, bool live) { return wga::c128::dma_ref(g, t, w, j, l, s, live); }
  template <bool P> static void walk(const Geom& g, const wga::Tile& t, int w, int s, bool live, wga::Dma (*out)[64]) {
    for (int l = 0; l < 64; ++l) {
      const wga::c128::Lane<P> ln = wga::c128::lane_init<P>(g, w, l);
      const wga::TileOrg org = wga::c128::tile_org(g, t);
      const unsigned m = wga::c128::tile_mask<P>(g, ln, t);
      for (int j = 0; j < NDMA; ++j) out[j][l] = wga::c128::dma<P>(g, ln, org, m, t, w, j, s, live);
    }
  }
};
struct S2 {
  typedef wga::s2::Geom Geom;
  static constexpr int T_H = wga::s2::T_H, T_W = wga::s2::T_W, NDMA = wga::s2::NDMA, STG = wga::s2::STG, SINK = wga::s2::SINK;
  static constexpr int XSLICE = 128, YSLICE = 256, GROUPS = wga::s2::XGROUPS + wga::s2::YGROUPS;
  static int rows(const Geom& g) { return g.Ho; }
  static int cols(const Geom& g) { return g.Wo; }
  static long long xpixels(const Geom& g) { return (long long)g.N * g.Hi * g.Wi; }
  static long long ypixels(const Geom& g) { return (long long)g.N * g.Ho * g.Wo; }
  static wga::Dma ref(const Geom& g, const wga::Tile& t, int w, int j, int l, int s, bool live) { return wga::s2::dma_ref(g, t, w, j, l, s, live); }
  template <bool P> static void walk(const Geom& g, const wga::Tile& t, int w, int s, bool live, wga::Dma (*out)[64]) {
    for (int l = 0; l < 64; ++l) {
      const wga::s2::Lane<P> ln = wga::s2::lane_init<P>(g, w, l);
      const wga::TileOrg org = wga::s2::tile_org(g, t);
      const unsigned m = wga::s2::tile_mask<P>(g, ln, t);
      for (int j = 0; j < NDMA; ++j) out[j][l] = wga::s2::dma<P>(g, ln, org, m, t, w, j, s, live);
    }
  }
};

template <class K>
void check_source(const char* name, const typename K::Geom& g, const wga::Dma& r, const char* which) {
  if (r.ok) {
    const long long off = r.soff + (long long)r.loff;
    const int pix = 2 * (r.op ? g.Cy : g.Cx), slice = r.op ? K::YSLICE : K::XSLICE;
    const long long pixels = r.op ? K::ypixels(g) : K::xpixels(g);
    REQUIRE(off >= 0 && off / pix < pixels, "%s %s: offset %lld outside the tensor of %lld pixels", name, which, off, pixels);
    REQUIRE(off % pix + 16 <= slice && off % 16 == 0, "%s %s: offset %lld leaves the %d-byte channel slice", name, which, off, slice);
  } else {
    REQUIRE(r.loff + 16 <= 2048 && r.loff % 16 == 0, "%s %s: zero-page offset %u", name, which, r.loff);
  }
}

template <class K>
void check(const char* name, const typename K::Geom& g) {
  const int pack = g.pack, Wv = pack == 1 ? K::cols(g) : K::T_W;
  wga::Dma fresh[K::NDMA][64];
  long long before = g_checked;
  for (int n = 0; n * pack < g.N; ++n)
    for (int y0 = 0; y0 < K::rows(g); y0 += K::T_H)
      for (int x0 = 0; x0 < Wv; x0 += K::T_W)
        for (int stage = 0; stage < 2; ++stage)
          for (int live = 0; live < 2; ++live) {
            const wga::Tile t = {n, y0, x0};
            Image was, is;
            for (int w = 0; w < 8; ++w) {
              if (pack > 1) K::template walk<true>(g, t, w, stage, live != 0, fresh);
              else K::template walk<false>(g, t, w, stage, live != 0, fresh);
              for (int j = 0; j < K::NDMA; ++j) {
                const unsigned dst_ref = K::ref(g, t, w, j, 0, stage, live != 0).dst, dst = fresh[j][0].dst;
                for (int l = 0; l < 64; ++l) {
                  const wga::Dma o = K::ref(g, t, w, j, l, stage, live != 0);
                  const wga::Dma& r = fresh[j][l];
                  REQUIRE(o.dst == dst_ref && r.dst == dst, "%s: the destination of a group depends on the lane", name);
                  check_source<K>(name, g, o, "reference");
                  check_source<K>(name, g, r, "kernel");
                  if (!live) REQUIRE(!r.ok && r.dst == (unsigned)K::SINK, "%s: a dead prefetch reads or lands somewhere", name);
                  if (r.dst == (unsigned)K::SINK) REQUIRE(!r.ok, "%s: a group for the sink reads an operand", name);
                  else REQUIRE(r.dst >= (unsigned)(stage * K::STG) && r.dst + 1024 <= (unsigned)((stage + 1) * K::STG) && r.dst % 1024 == 0,
                               "%s: destination %u outside stage %d", name, r.dst, stage);
                  if (o.dst != (unsigned)K::SINK) { was[o.dst].resize(64); was[o.dst][l] = {o.op, o.ok, o.soff + (long long)o.loff}; }
                  if (r.dst != (unsigned)K::SINK) { is[r.dst].resize(64); is[r.dst][l] = {r.op, r.ok, r.soff + (long long)r.loff}; }
                  // an invalid lane's place in the zero page is the swizzled slot, as before
                  if (!o.ok && o.dst != (unsigned)K::SINK) was[o.dst][l].off = o.loff;
                  if (!r.ok && r.dst != (unsigned)K::SINK) is[r.dst][l].off = r.loff;
                  ++g_checked;
                }
              }
            }
            REQUIRE(was.size() == is.size(), "%s tile (%d, %d, %d): %zu destinations, were %zu", name, n, y0, x0, is.size(), was.size());
            if (live) REQUIRE(was.size() == (size_t)K::GROUPS, "%s: %zu groups land in the stage, not %d", name, was.size(), K::GROUPS);
            for (const auto& kv : was) {
              const auto it = is.find(kv.first);
              REQUIRE(it != is.end(), "%s tile (%d, %d, %d): destination %u is not filled", name, n, y0, x0, kv.first);
              if (it == is.end()) continue;
              for (int l = 0; l < 64; ++l) {
                const LaneSrc &o = kv.second[l], &r = it->second[l];
                REQUIRE(o == r && (o.ok || o.off == r.off), "%s tile (%d, %d, %d) dst %u lane %d: op %d ok %d off %lld, was op %d ok %d off %lld", name,
                        n, y0, x0, kv.first, l, r.op, (int)r.ok, r.off, o.op, (int)o.ok, o.off);
              }
            }
          }
  std::printf("%-44s %10lld lane addresses\n", name, g_checked - before);
}

wga::c128::Geom c128(int N, int H, int W, int Cx, int Cy) {
  const int pack = W <= 7 ? 4 : (W <= 15 ? 2 : 1);
  return {N, H, W, Cx, Cy, pack, pack == 4 ? 3 : (pack == 2 ? 4 : 5)};
}
wga::s2::Geom s2(int N, int Hi, int Wi, int Cx, int Cy) {
  const int Wo = Wi / 2, pack = Wo <= 7 ? 4 : (Wo <= 15 ? 2 : 1);
  return {N, Hi, Wi, Hi / 2, Wo, Cx, Cy, pack, pack == 4 ? 3 : (pack == 2 ? 4 : 5)};
}

}  // namespace

int main() {
  // the border geometries of tests/test_wgrad_dma_addr_gpu.py
  check<C128>("c128b 28x28 N3 128->64", c128(3, 28, 28, 128, 64));
  check<C128>("c128b 32x5 N2", c128(2, 5, 32, 128, 128));
  check<C128>("c128b 40x4 N2", c128(2, 4, 40, 128, 128));
  check<C128>("c128b 14x14 N3 256->128 (pack 2)", c128(3, 14, 14, 256, 128));
  check<C128>("c128b 7x7 N5 128->192 (pack 4)", c128(5, 7, 7, 128, 192));
  check<C128>("c128b 9x10 N7", c128(7, 9, 10, 128, 64));
  check<C128>("c128b 33x6 N1", c128(1, 6, 33, 128, 128));
  check<C128>("c128b 15x5 N3 256->64 (pack 2)", c128(3, 5, 15, 256, 64));
  check<C128>("c128b 16x5 N3", c128(3, 5, 16, 128, 64));
  check<C128>("c128b 1x1 N6 (pack 4)", c128(6, 1, 1, 128, 64));
  check<S2>("s2 56x56 N2 64->128", s2(2, 56, 56, 64, 128));
  check<S2>("s2 28x28 N3 128->256 (pack 2)", s2(3, 28, 28, 128, 256));
  check<S2>("s2 14x14 N5 128->256 (pack 4)", s2(5, 14, 14, 128, 256));
  check<S2>("s2 80x8 N2", s2(2, 8, 80, 64, 128));
  check<S2>("s2 30x10 N3 (pack 2, Wo 15)", s2(3, 10, 30, 64, 128));
  check<S2>("s2 32x8 N2 64->256", s2(2, 8, 32, 64, 256));
  check<S2>("s2 2x2 N7 (pack 4)", s2(7, 2, 2, 64, 128));
  // geometries of tests/test_conv_bf16_domain_gpu.py that the above do not repeat
  check<C128>("c128b 8x6 N3 128->192", c128(3, 6, 8, 128, 192));
  check<C128>("c128b 14x14 N7 (pack 2)", c128(7, 14, 14, 128, 128));
  check<S2>("s2 16x12 N3 128->128 (pack 2)", s2(3, 12, 16, 128, 128));
  check<S2>("s2 14x14 N5 256->512 (pack 4)", s2(5, 14, 14, 256, 512));
  // the five layers of the benchmark at a small image count
  check<C128>("bench c128b 128->128 @28", c128(5, 28, 28, 128, 128));
  check<C128>("bench c128b 256->256 @14", c128(5, 14, 14, 256, 256));
  check<C128>("bench c128b 512->512 @7", c128(5, 7, 7, 512, 512));
  check<S2>("bench s2 64->128 @56", s2(5, 56, 56, 64, 128));
  check<S2>("bench s2 128->256 @28", s2(5, 28, 28, 128, 256));
  std::printf("%lld lane addresses checked, %d failures\n", g_checked, g_failed);
  return g_failed ? 1 : 0;
}
