// LDS-DMA source addresses, validity and LDS destinations of the all-taps weight-gradient kernels (conv_wgrad_c128b.hip,
// conv_wgrad_s2.hip), as plain functions for the device AND the host: tests/wgrad_dma_addr_check.cpp walks every
// (tile, wave, slot j, lane) of a list of geometries with the host compiler and compares the two forms below.
//
//   *_dma_ref   the arithmetic the kernels carried inside their tile loops until DESIGN.md "Weight-gradient DMA addresses":
//               group d = wave + 8 j decides at run time between X, dY and padding; everything per DMA and per lane.
//   *_dma       what the kernels run: the KIND of a group is a function of the slot j alone (X first, then dY), and an
//               address is  (valid ? operand + soff : zero page) + loff  with
//                 soff  wave-uniform, 64-bit: tile origin (TileOrg, once per tile) + patch row / column group of slot j;
//                 loff  32-bit, (valid ? lane part : its swizzled slot alone) ^ parity bit of the group -- the lane part is
//                       computed ONCE before the tile loop (*_lane): pixel in group x pixel pitch + swizzled 16-byte slot,
//                       and for packed small images, where the lane's image k and column depend on the group, per slot j;
//                 valid row validity (wave-uniform) && column validity && batch tail.  Unpacked: one unsigned compare of
//                       (scalar + lane constant) against the width.  Packed: one tile per row, so the columns are tile-
//                       invariant -- bit j of a lane mask; the batch tail only bites in the last pack of the batch, which
//                       has a second mask (Lane::full / Lane::last).
//               The two swizzle parities of a group differ in ONE address bit that only the slot contributes (pixel pitches
//               are multiples of the row size), hence the XOR.
// Both return the same struct: `soff + loff` is the byte offset inside the operand slice (valid) or the zero page (not).
#pragma once
#if defined(__HIPCC__)
#define WGA_FN __host__ __device__ __forceinline__
#define WGA_UNROLL _Pragma("unroll")
#else
#define WGA_FN inline
#define WGA_UNROLL
#endif

namespace wga {

struct Tile { int n, y0, x0; };       // n: packed image group; (y0, x0): output pixel of the tile's corner
struct TileOrg { long long x, y; };   // byte offset of the tile's first pixel (slot 0) in X / dY
struct Dma {
  int op;              // 0: X, 1: dY
  bool ok;             // reads the operand (else the zero page)
  long long soff;      // wave-uniform part of the byte offset (operand slice); unused when !ok
  unsigned loff;       // lane part; < 256 when !ok
  unsigned dst;        // LDS byte address relative to the block's first stage; SINK for padding groups and dead prefetches
};

// ================================================================== conv_wgrad_c128b.hip
namespace c128 {
constexpr int T_H = 4, T_W = 32, XPITCH = 40, XROWS = T_H + 2;
constexpr int XB = XROWS * XPITCH * 256, YB = T_H * T_W * 128, STG = XB + YB, SINK = 2 * STG;
constexpr int XGROUPS = XROWS * 9, YGROUPS = 16, NDMA = 9, XSLOTS = 7;      // slots 0..6: X (8 x 7 >= 54), 7, 8: dY

struct Geom { int N, H, W, Cx, Cy, pack, slot_shift; };

WGA_FN unsigned xswz(int lane) { const int px = lane >> 4, s = lane & 15; return (unsigned)(((((s >> 1) ^ px) << 1) | (s & 1)) << 4); }
WGA_FN unsigned yswz(int lane) {
  const int px = lane >> 3, s = lane & 7;
  return (unsigned)(((((s >> 1) ^ ((px >> 1) & 1)) << 1) | (s & 1)) << 4);
}

// ---- reference: the kernel's former dma_one, restated
WGA_FN Dma dma_ref(const Geom& a, const Tile& tl, int wave, int j, int lane, int stage, bool live) {
  const int d = wave + 8 * j;
  const int xl_px = lane >> 4, xl_slot = lane & 15, yl_px = lane >> 3, yl_slot = lane & 7;
  const unsigned xsrc0 = (unsigned)(((((xl_slot >> 1) ^ xl_px) << 1) | (xl_slot & 1)) << 4);
  const unsigned xsrc1 = (unsigned)(((((xl_slot >> 1) ^ (xl_px | 4)) << 1) | (xl_slot & 1)) << 4);
  const unsigned ysrc0 = (unsigned)(((((yl_slot >> 1) ^ ((yl_px >> 1) & 1)) << 1) | (yl_slot & 1)) << 4);
  const unsigned ysrc1 = (unsigned)(((((yl_slot >> 1) ^ (((yl_px >> 1) & 1) | 2)) << 1) | (yl_slot & 1)) << 4);
  const int slot_mask = (1 << a.slot_shift) - 1;
  const int xpix = a.Cx * 2, ypix = a.Cy * 2;
  const unsigned sbase = (unsigned)stage * STG;
  const long long porg = ((long long)tl.n * a.pack * a.H + tl.y0) * a.W + tl.x0;
  const int imgs_left = a.N - tl.n * a.pack;
  Dma r;
  bool real = live;
  if (d < XGROUPS) {
    const int pr = d / 9, g = d - 9 * pr;
    const int vc = -1 + 4 * g + xl_px;
    const int k = a.pack == 1 ? 0 : (vc >> a.slot_shift), rc = a.pack == 1 ? vc : (vc & slot_mask);
    const bool row_ok = (unsigned)(tl.y0 - 1 + pr) < (unsigned)a.H;
    const bool ok = real && row_ok && (unsigned)(tl.x0 + rc) < (unsigned)a.W && (unsigned)k < (unsigned)imgs_left && k < a.pack;
    const long long off = (long long)(((k * a.H + (pr - 1)) * a.W + rc)) * xpix;
    r.op = 0; r.ok = ok; r.soff = porg * xpix + off; r.loff = ((pr + (g >> 1)) & 1) ? xsrc1 : xsrc0;
    r.dst = sbase + (unsigned)((pr * XPITCH + 4 * g) * 256);
  } else if (d < XGROUPS + YGROUPS) {
    const int g2 = d - XGROUPS;
    const int rr = g2 >> 2, c = 8 * (g2 & 3) + yl_px;
    const int k = a.pack == 1 ? 0 : (c >> a.slot_shift), rc = a.pack == 1 ? c : (c & slot_mask);
    const bool ok = real && tl.y0 + rr < a.H && tl.x0 + rc < a.W && k < imgs_left;
    const long long off = (long long)(((k * a.H + rr) * a.W + rc)) * ypix;
    r.op = 1; r.ok = ok; r.soff = porg * ypix + off; r.loff = (g2 & 1) ? ysrc1 : ysrc0;
    r.dst = sbase + (unsigned)(XB + g2 * 1024);
  } else {
    real = false;
    r.op = 0; r.ok = false; r.soff = 0; r.loff = (unsigned)(lane * 16); r.dst = 0;
  }
  if (!real) r.dst = SINK;
  return r;
}

// ---- what the kernel runs
template <bool PACKED>
struct Lane {
  unsigned xl[PACKED ? XSLOTS : 1];           // X lane part (parity 0), per slot when packed
  unsigned yl[PACKED ? NDMA - XSLOTS : 1];    // dY lane part
  unsigned xz, yz;                            // the swizzled slot alone: the lane's offset inside the zero page
  int xpx, ypx;                               // pixel in group (unpacked: the column compare)
  unsigned full, last;                        // packed: bit j = the lane of slot j reads an image -- all packs but the last / the last
};

// columns [0, W) of slot k < imgs; virtual column vc of a packed tile row
WGA_FN bool packed_col(const Geom& a, int vc, int imgs, int* k, int* rc) {
  *k = vc >> a.slot_shift;
  *rc = vc & ((1 << a.slot_shift) - 1);
  return vc >= 0 && *k < a.pack && *k < imgs && *rc < a.W;
}

template <bool PACKED>
WGA_FN Lane<PACKED> lane_init(const Geom& a, int wave, int lane) {
  Lane<PACKED> ln;
  const int xpix = a.Cx * 2, ypix = a.Cy * 2;
  ln.xpx = lane >> 4; ln.ypx = lane >> 3;
  ln.xz = xswz(lane); ln.yz = yswz(lane);
  ln.full = ln.last = 0;
  if constexpr (!PACKED) {
    ln.xl[0] = (unsigned)(ln.xpx * xpix) + ln.xz;
    ln.yl[0] = (unsigned)(ln.ypx * ypix) + ln.yz;
  } else {
    const int tail = a.N - (a.N - 1) / a.pack * a.pack;      // images of the last pack
WGA_UNROLL
    for (int j = 0; j < NDMA; ++j) {
      int k, rc;
      if (j < XSLOTS) {
        const int d = wave + 8 * j, g = d - 9 * (d / 9);
        const int vc = -1 + 4 * g + ln.xpx;
        if (packed_col(a, vc, a.pack, &k, &rc)) ln.full |= 1u << j;
        if (packed_col(a, vc, tail, &k, &rc)) ln.last |= 1u << j;
        ln.xl[j] = (unsigned)((k * a.H * a.W + rc) * xpix) + ln.xz;
      } else {
        const int g2 = wave + 8 * (j - XSLOTS);
        const int vc = 8 * (g2 & 3) + ln.ypx;
        if (packed_col(a, vc, a.pack, &k, &rc)) ln.full |= 1u << j;
        if (packed_col(a, vc, tail, &k, &rc)) ln.last |= 1u << j;
        ln.yl[j - XSLOTS] = (unsigned)((k * a.H * a.W + rc) * ypix) + ln.yz;
      }
    }
  }
  return ln;
}

WGA_FN TileOrg tile_org(const Geom& a, const Tile& tl) {
  const long long porg = ((long long)tl.n * a.pack * a.H + tl.y0) * a.W + tl.x0;
  TileOrg o;
  o.x = porg * (a.Cx * 2); o.y = porg * (a.Cy * 2);
  return o;
}
// packed: the validity mask of tile `tl` (the last pack of the batch may hold fewer images)
template <bool PACKED>
WGA_FN unsigned tile_mask(const Geom& a, const Lane<PACKED>& ln, const Tile& tl) {
  return (tl.n + 1) * a.pack > a.N ? ln.last : ln.full;
}

template <bool PACKED>
WGA_FN Dma dma(const Geom& a, const Lane<PACKED>& ln, const TileOrg& org, unsigned mask, const Tile& tl, int wave, int j, int stage,
               bool live) {
  Dma r;
  const unsigned sbase = (unsigned)stage * STG;
  if (j < XSLOTS) {
    const int d = wave + 8 * j;
    const int pr = d / 9, g = d - 9 * pr;                    // wave-uniform and tile-invariant
    const bool real = live && d < XGROUPS;
    const bool row_ok = real && (unsigned)(tl.y0 - 1 + pr) < (unsigned)a.H;
    const unsigned par = (unsigned)((pr + (g >> 1)) & 1) << 7;
    int opx;
    unsigned l;
    if constexpr (PACKED) {
      r.ok = row_ok && ((mask >> j) & 1);
      opx = (pr - 1) * a.W; l = ln.xl[j];
    } else {
      r.ok = row_ok && (unsigned)(tl.x0 + 4 * g - 1 + ln.xpx) < (unsigned)a.W;
      opx = (pr - 1) * a.W + 4 * g - 1; l = ln.xl[0];
    }
    r.op = 0;
    r.soff = org.x + (long long)opx * (a.Cx * 2);
    r.loff = (r.ok ? l : ln.xz) ^ par;
    r.dst = real ? sbase + (unsigned)((pr * XPITCH + 4 * g) * 256) : (unsigned)SINK;
  } else {
    const int g2 = wave + 8 * (j - XSLOTS);
    const int rr = g2 >> 2, cb = 8 * (g2 & 3);
    const bool row_ok = live && tl.y0 + rr < a.H;
    const unsigned par = (unsigned)(g2 & 1) << 6;
    int opx;
    unsigned l;
    if constexpr (PACKED) {
      r.ok = row_ok && ((mask >> j) & 1);
      opx = rr * a.W; l = ln.yl[j - XSLOTS];
    } else {
      r.ok = row_ok && tl.x0 + cb + ln.ypx < a.W;
      opx = rr * a.W + cb; l = ln.yl[0];
    }
    r.op = 1;
    r.soff = org.y + (long long)opx * (a.Cy * 2);
    r.loff = (r.ok ? l : ln.yz) ^ par;
    r.dst = live ? sbase + (unsigned)(XB + g2 * 1024) : (unsigned)SINK;
  }
  return r;
}
}  // namespace c128

// ================================================================== conv_wgrad_s2.hip
namespace s2 {
constexpr int T_H = 2, T_W = 32, XROWS = 2 * T_H + 1, ODDP = 40, EVENP = 32;
constexpr int XROWB = (ODDP + EVENP) * 128, XB = XROWS * XROWB, YB = T_H * T_W * 256, STG = XB + YB, SINK = 2 * STG;
constexpr int XGROUPS = XROWS * 9, YGROUPS = 16, NDMA = 8, XSLOTS = 6;      // slots 0..5: X (8 x 6 >= 45), 6, 7: dY

struct Geom { int N, Hi, Wi, Ho, Wo, Cx, Cy, pack, slot_shift; };

WGA_FN unsigned xswz(int lane) {
  const int px = lane >> 3, s = lane & 7;
  return (unsigned)(((((s >> 1) ^ ((px >> 1) & 1)) << 1) | (s & 1)) << 4);
}
WGA_FN unsigned yswz(int lane) { const int px = lane >> 4, s = lane & 15; return (unsigned)(((((s >> 1) ^ px) << 1) | (s & 1)) << 4); }

// ---- reference: the kernel's former dma_one, restated
WGA_FN Dma dma_ref(const Geom& a, const Tile& tl, int wave, int j, int lane, int stage, bool live) {
  const int d = wave + 8 * j;
  const int xl_px = lane >> 3, xl_slot = lane & 7, yl_px = lane >> 4, yl_slot = lane & 15;
  const unsigned xsrc0 = (unsigned)(((((xl_slot >> 1) ^ ((xl_px >> 1) & 1)) << 1) | (xl_slot & 1)) << 4);
  const unsigned xsrc1 = (unsigned)(((((xl_slot >> 1) ^ (((xl_px >> 1) & 1) | 2)) << 1) | (xl_slot & 1)) << 4);
  const unsigned ysrc0 = (unsigned)(((((yl_slot >> 1) ^ yl_px) << 1) | (yl_slot & 1)) << 4);
  const unsigned ysrc1 = (unsigned)(((((yl_slot >> 1) ^ (yl_px | 4)) << 1) | (yl_slot & 1)) << 4);
  const int slot_mask = (1 << a.slot_shift) - 1;
  const int xpix = a.Cx * 2, ypix = a.Cy * 2;
  const unsigned sbase = (unsigned)stage * STG;
  const int img0 = tl.n * a.pack;
  const int imgs_left = a.N - img0;
  Dma r;
  bool real = live;
  if (d < XGROUPS) {
    const int pr = d / 9, g = d - 9 * pr;
    const bool odd = g < 5;
    const int gp = odd ? g : g - 5;
    const int vj = tl.x0 + 8 * gp + xl_px - (odd ? 1 : 0);
    const int k = a.pack == 1 ? 0 : (vj >> a.slot_shift), rc = a.pack == 1 ? vj : (vj & slot_mask);
    const int xc = 2 * rc + (odd ? 1 : 0), xr = 2 * tl.y0 - 1 + pr;
    const bool ok = real && (unsigned)xr < (unsigned)a.Hi && vj >= 0 && (unsigned)xc < (unsigned)a.Wi &&
                    (unsigned)k < (unsigned)imgs_left && k < a.pack;
    const long long pix = ((long long)(img0 + k) * a.Hi + xr) * a.Wi + xc;
    r.op = 0; r.ok = ok; r.soff = pix * xpix; r.loff = (gp & 1) ? xsrc1 : xsrc0;
    r.dst = sbase + (unsigned)(pr * XROWB + g * 1024);
  } else if (d < XGROUPS + YGROUPS) {
    const int g2 = d - XGROUPS;
    const int rr = g2 >> 3, c = 4 * (g2 & 7) + yl_px;
    const int vj = tl.x0 + c;
    const int k = a.pack == 1 ? 0 : (vj >> a.slot_shift), rc = a.pack == 1 ? vj : (vj & slot_mask);
    const bool ok = real && tl.y0 + rr < a.Ho && rc < a.Wo && k < imgs_left && k < a.pack;
    const long long pix = ((long long)(img0 + k) * a.Ho + tl.y0 + rr) * a.Wo + rc;
    r.op = 1; r.ok = ok; r.soff = pix * ypix; r.loff = ((g2 >> 1) & 1) ? ysrc1 : ysrc0;
    r.dst = sbase + (unsigned)(XB + g2 * 1024);
  } else {
    real = false;
    r.op = 0; r.ok = false; r.soff = 0; r.loff = (unsigned)(lane * 16); r.dst = 0;
  }
  if (!real) r.dst = SINK;
  return r;
}

// ---- what the kernel runs
template <bool PACKED>
struct Lane {
  unsigned xl[PACKED ? XSLOTS : 1];
  unsigned yl[PACKED ? NDMA - XSLOTS : 1];
  unsigned xz, yz;
  int xpx2, ypx;                              // unpacked: twice the position in group (input columns) / the pixel in group
  unsigned full, last;
};

WGA_FN bool packed_col(int shift, int pack, int vj, int imgs, int* k, int* rc) {
  *k = vj >> shift;
  *rc = vj & ((1 << shift) - 1);
  return vj >= 0 && *k < pack && *k < imgs;
}

template <bool PACKED>
WGA_FN Lane<PACKED> lane_init(const Geom& a, int wave, int lane) {
  Lane<PACKED> ln;
  const int xpix = a.Cx * 2, ypix = a.Cy * 2;
  ln.xpx2 = 2 * (lane >> 3); ln.ypx = lane >> 4;
  ln.xz = xswz(lane); ln.yz = yswz(lane);
  ln.full = ln.last = 0;
  if constexpr (!PACKED) {
    ln.xl[0] = (unsigned)(ln.xpx2 * xpix) + ln.xz;
    ln.yl[0] = (unsigned)(ln.ypx * ypix) + ln.yz;
  } else {
    const int tail = a.N - (a.N - 1) / a.pack * a.pack;
WGA_UNROLL
    for (int j = 0; j < NDMA; ++j) {
      int k, rc;
      if (j < XSLOTS) {
        const int d = wave + 8 * j, g = d - 9 * (d / 9);
        const int odd = g < 5 ? 1 : 0, gp = odd ? g : g - 5;
        const int vj = 8 * gp + (lane >> 3) - odd;
        const bool in_full = packed_col(a.slot_shift, a.pack, vj, a.pack, &k, &rc);
        const bool in_last = packed_col(a.slot_shift, a.pack, vj, tail, &k, &rc);
        const int xc = 2 * rc + odd;
        if (in_full && xc < a.Wi) ln.full |= 1u << j;
        if (in_last && xc < a.Wi) ln.last |= 1u << j;
        ln.xl[j] = (unsigned)((k * a.Hi * a.Wi + xc) * xpix) + ln.xz;
      } else {
        const int g2 = wave + 8 * (j - XSLOTS);
        const int vj = 4 * (g2 & 7) + ln.ypx;
        const bool in_full = packed_col(a.slot_shift, a.pack, vj, a.pack, &k, &rc);
        const bool in_last = packed_col(a.slot_shift, a.pack, vj, tail, &k, &rc);
        if (in_full && rc < a.Wo) ln.full |= 1u << j;
        if (in_last && rc < a.Wo) ln.last |= 1u << j;
        ln.yl[j - XSLOTS] = (unsigned)((k * a.Ho * a.Wo + rc) * ypix) + ln.yz;
      }
    }
  }
  return ln;
}

WGA_FN TileOrg tile_org(const Geom& a, const Tile& tl) {
  const long long img0 = (long long)tl.n * a.pack;
  TileOrg o;
  o.x = ((img0 * a.Hi + 2 * tl.y0) * a.Wi + 2 * tl.x0) * (a.Cx * 2);
  o.y = ((img0 * a.Ho + tl.y0) * a.Wo + tl.x0) * (a.Cy * 2);
  return o;
}
template <bool PACKED>
WGA_FN unsigned tile_mask(const Geom& a, const Lane<PACKED>& ln, const Tile& tl) {
  return (tl.n + 1) * a.pack > a.N ? ln.last : ln.full;
}

template <bool PACKED>
WGA_FN Dma dma(const Geom& a, const Lane<PACKED>& ln, const TileOrg& org, unsigned mask, const Tile& tl, int wave, int j, int stage,
               bool live) {
  Dma r;
  const unsigned sbase = (unsigned)stage * STG;
  if (j < XSLOTS) {
    const int d = wave + 8 * j;
    const int pr = d / 9, g = d - 9 * pr;                    // wave-uniform and tile-invariant
    const int odd = g < 5 ? 1 : 0, gp = odd ? g : g - 5;
    const bool real = live && d < XGROUPS;
    const bool row_ok = real && (unsigned)(2 * tl.y0 - 1 + pr) < (unsigned)a.Hi;
    const unsigned par = (unsigned)(gp & 1) << 6;
    int opx;
    unsigned l;
    if constexpr (PACKED) {
      r.ok = row_ok && ((mask >> j) & 1);
      opx = (pr - 1) * a.Wi; l = ln.xl[j];
    } else {                                                 // input column 2 vj + odd >= 0 exactly when position vj >= 0
      r.ok = row_ok && (unsigned)(2 * tl.x0 + 16 * gp - odd + ln.xpx2) < (unsigned)a.Wi;
      opx = (pr - 1) * a.Wi + 16 * gp - odd; l = ln.xl[0];
    }
    r.op = 0;
    r.soff = org.x + (long long)opx * (a.Cx * 2);
    r.loff = (r.ok ? l : ln.xz) ^ par;
    r.dst = real ? sbase + (unsigned)(pr * XROWB + g * 1024) : (unsigned)SINK;
  } else {
    const int g2 = wave + 8 * (j - XSLOTS);
    const int rr = g2 >> 3, cb = 4 * (g2 & 7);
    const bool row_ok = live && tl.y0 + rr < a.Ho;
    const unsigned par = (unsigned)((g2 >> 1) & 1) << 7;
    int opx;
    unsigned l;
    if constexpr (PACKED) {
      r.ok = row_ok && ((mask >> j) & 1);
      opx = rr * a.Wo; l = ln.yl[j - XSLOTS];
    } else {
      r.ok = row_ok && tl.x0 + cb + ln.ypx < a.Wo;
      opx = rr * a.Wo + cb; l = ln.yl[0];
    }
    r.op = 1;
    r.soff = org.y + (long long)opx * (a.Cy * 2);
    r.loff = (r.ok ? l : ln.yz) ^ par;
    r.dst = live ? sbase + (unsigned)(XB + g2 * 1024) : (unsigned)SINK;
  }
  return r;
}
}  // namespace s2

}  // namespace wga
