"""Case tables, input generators, mirrors of the host plans and fp64 references for the bf16 convolution family of the
ResNet-18 patch encoder (csrc/conv_igemm.hip, conv_c64.hip, conv_halo.hip, conv_pgemm.hip, conv_wgrad.hip, conv_wgrad_c64.hip,
conv_wgrad_c128b.hip, conv_wgrad_s2.hip).  tests/test_conv_bf16_domain_gpu.py runs the cases on the device,
tests/test_conv_bf16_ref_cpu.py shows on the CPU that the method is sound.

Method: inputs, all exactly representable in bf16, for which fp32 accumulation is exact in ANY order, so that every kernel,
whatever its tile order, must produce the correctly rounded (ties to even) value of the exact sum:
  family I ("dyadic dense")   activations, weights, gradients multiples of 1/8 in [-1, 1], addends multiples of 1/8 in [-4, 4]:
                              every product is a multiple of 2^-6 and every partial sum of K <= 10 * 512 terms stays below
                              2^13 -- exact_condition() asserts (terms * max|a| * max|b| + max|addend|) * 2^6 < 2^24.
                              Weight gradient: N * Ho * Wo terms; the grid is coarsened (1/4, then 1/2) where that fails.
  family P ("selector")       the weight has ONE non-zero of {+-1/2, +-1, +-2} per output channel, on every tap position and
                              at both ends of every 64-channel chunk; the activations are full-mantissa bf16 (8 significant
                              bits) times 2^e, e in [-6, 6]: the output is s * x at the shifted pixel, or 0 in the padding,
                              bit for bit.  With an addend (8 bits times 2^e, e in [-4, 4]) every value is a multiple of
                              2^-14 below 2^9: 23 bits, exact in fp32, one rounding.  Weight gradient: dy has one non-zero
                              pixel per output channel (corners, both sides of tile seams, last image, next to the gap
                              columns of packed images): dW[co] is a scaled window of x.
  family S ("dyadic sparse")  for the fused statistics: activations multiples of 1/4 in [-1, 1], weights in {0, +-1/2, +-1}
                              with at most four non-zeros per output channel: outputs are multiples of 1/8 with |v| <= 4
                              (<= 8 with an addend), bf16-exact; one fp32 partial of `px` pixels holds a sum of squares
                              exactly while px * max|v|^2 * 2^6 < 2^24 -- stats_condition() asserts it with the pixels per
                              partial read from each kernel (PIXELS_PER_PARTIAL).
The sign of an exact zero is not pinned; values are compared with ==.

The host plans (conv2d_dispatch, isic_conv_halo_supported, the halo groups, the c64 tiles per block, the pgemm block shares,
wc128b_plan, ws2_plan, wgrad_plan, the workspace sizes) are mirrored for a given CU count: the case table states the kernel
and the tiles per block each case is meant for, and the N of a multi-tile case is derived from the mirror."""
import zlib

import torch
import torch.nn.functional as F

F64 = torch.float64
BF = torch.bfloat16
CUS = 256                                    # MI355X; the device test passes the device's own count
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
SLOTS = (1, 32, 256, 300)


class Box(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def cdiv(a, b):
    return -(-a // b)


# ================================================================== geometry (the arguments of isic_conv2d_igemm_bf16)
def geom(N, Hin, Win, Cin, Hout, Wout, Cout, Kh, Kw, up, down, pad):
    return Box(N=N, Hin=Hin, Win=Win, Cin=Cin, Hout=Hout, Wout=Wout, Cout=Cout, Kh=Kh, Kw=Kw, up=up, down=down, pad=pad)


def fwd(N, H, W, Ci, Co, kh, s, p, kw=None):
    kw = kh if kw is None else kw
    return geom(N, H, W, Ci, (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1, Co, kh, kw, s, 1, p)


def dgrad(N, H, W, Ci, Co, k, s, p):
    """the data gradient of fwd(N, H, W, Ci, Co, k, s, p): in = dY, out = dX"""
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return geom(N, Ho, Wo, Co, H, W, Ci, k, k, 1, s, k - 1 - p)


def args(g):
    return (g.N, g.Hin, g.Win, g.Cin, g.Hout, g.Wout, g.Cout, g.Kh, g.Kw, g.up, g.down, g.pad)


def same3x3(g):
    return g.Kh == 3 and g.Kw == 3 and g.up == 1 and g.down == 1 and g.pad == 1 and g.Hin == g.Hout and g.Win == g.Wout


# ================================================================== mirrors of the host plans
PIXELS_PER_PARTIAL = {          # pixels one fp32 accumulator covers before it reaches the fp64 rows, per tile of a block
    "igemm64": 64, "igemm128": 64,      # conv_igemm.hip: 4 threads per column, 64 rows each, joined in fp64
    "c64t": 64,                          # conv_c64.hip tile per block: the same scheme
    "c64p": 256, "halo-k1": 256, "halo-k2": 256, "pgemm64": 256, "pgemm128": 256,   # x tiles per block: a lane keeps its
    "halo-bnbwd": 256,                   # four pixels, a DPP row adds 16 lanes, the four pixel waves are added in fp32
}                                        # -- and the persistent kernels carry that sum over ALL tiles of the block


def halo_supported(N, H, W, Cin, Cout):
    M = N * H * W
    return (Cin % 64 == 0 and Cout % 128 == 0 and W >= 1 and 256 + 2 * W + 2 <= 384 and M < 2 ** 24 and H * W < 2 ** 16
            and M * Cin <= 0x7FFFFFFF and M * Cout <= 0x7FFFFFFF)


def halo_plan(N, H, W, Cin, Cout, exp=0, cus=CUS):
    p = Box(mtiles=cdiv(N * H * W, 256), nslices=Cout // 128)
    groups = max(cus // p.nslices, 1)
    p.tiles_per_block = cdiv(p.mtiles, groups)
    p.groups = cdiv(p.mtiles, p.tiles_per_block)
    p.blocks = p.groups * p.nslices
    prows = cdiv(256 + 2 * W + 2, 8) * 8
    lds2 = 2 * prows * 128 + 3 * 128 * 128 + 2176 + 3072 + 128 * 128
    p.kpb = 2 if (Cin % 128 == 0 and lds2 <= 160 * 1024 and exp != 1) else 1
    return p


def c64_plan(N, H, W, cus=CUS):
    p = Box(total_tiles=N * cdiv(H, 8) * cdiv(W, 32))
    p.tiles_per_block = cdiv(p.total_tiles, cus)
    p.blocks = cdiv(p.total_tiles, p.tiles_per_block)
    return p


def parity_classes(g, pair=False):
    """the parity classes of the output grid (one for down = 1), as conv2d_dispatch sets them up"""
    out = []
    d = g.down
    for ph in range(d):
        for pw in range(d):
            Hs, Ws = (g.Hout - ph + d - 1) // d, (g.Wout - pw + d - 1) // d
            if Hs <= 0 or Ws <= 0:
                continue
            kh0 = 0 if d == 1 else (g.pad - ph * g.up) % d
            kw0 = 0 if d == 1 else (g.pad - pw * g.up) % d
            nkh = (g.Kh - kh0 + d - 1) // d if kh0 < g.Kh else 0
            nkw = (g.Kw - kw0 + d - 1) // d if kw0 < g.Kw else 0
            c = Box(ph=ph, pw=pw, Hs=Hs, Ws=Ws, kh0=kh0, kw0=kw0, nkh=nkh, nkw=nkw, M=g.N * Hs * Ws)
            c.Ktiles = nkh * nkw * (g.Cin // 64)
            if pair and nkh == 1 and nkw == 1 and ph == 0 and pw == 0:
                c.Ktiles += g.Cin // 64
            out.append(c)
    return out


def pgemm_plan(classes, Cout, stats, cus=CUS):
    p = Box(PN=128 if Cout % 128 == 0 else 64)
    p.nslices = Cout // p.PN
    budget = max(cus // p.nslices, len(classes))
    mt = [cdiv(c.M, 256) for c in classes]
    cost = [float(m) * (c.Ktiles + (12.0 if stats else 6.0)) for m, c in zip(mt, classes)]
    total = sum(cost)
    g = [min(max(int(budget * x / total), 1), m) for x, m in zip(cost, mt)]
    for _ in range(budget - sum(g)):
        best, load = -1, 0.0
        for i in range(len(classes)):
            if g[i] < mt[i] and cost[i] / g[i] > load:
                load, best = cost[i] / g[i], i
        if best < 0:
            break
        g[best] += 1
    p.groups = g
    p.tiles = [cdiv(m, x) for m, x in zip(mt, g)]
    p.tiles_per_block = max(p.tiles)
    p.blocks = sum(g) * p.nslices
    return p


def decode_variant(v):
    c = (v // 10) % 10
    return Box(c64=2 if c == 0 else c - 1, halo=(v // 100) % 10, pgemm=(v // 1000) % 10, exp=(v // 10000) % 10)


def dispatch(g, variant=0, addend=False, stats=False, slots=32, mask=False, pair=False, cus=CUS):
    """conv2d_dispatch -> Box(code, kernel, tiles_per_block, blocks)"""
    r = Box(code=OK, kernel=None, tiles_per_block=1, blocks=0)

    def refuse(code):
        r.code = code
        return r
    if pair and not (g.Kh == 3 and g.Kw == 3 and g.up == 1 and g.down == 2 and g.pad == 1 and not addend and not stats):
        return refuse(UNSUPPORTED)
    if not (0 <= variant < 20000 and variant % 10 == 0):
        return refuse(BAD_ARG)
    cv = decode_variant(variant)
    if not (0 <= cv.c64 <= 2 and cv.halo <= 2 and cv.pgemm <= 2):
        return refuse(BAD_ARG)
    if min(g.N, g.Hin, g.Win, g.Hout, g.Wout, g.Kh, g.Kw, g.up) <= 0 or g.down not in (1, 2):
        return refuse(BAD_ARG)
    if stats and not (slots > 0 and g.down == 1):
        return refuse(BAD_ARG)
    if g.Cin % 64 or g.Cout % 64:
        return refuse(UNSUPPORTED)
    if g.N * g.Hout * g.Wout * g.Cout > 0x7FFFFFFF or g.N * g.Hin * g.Win * g.Cin > 0x7FFFFFFF:
        return refuse(UNSUPPORTED)
    s3 = same3x3(g)
    if g.Cin == 64 and g.Cout == 64 and s3 and cv.c64 != 0:
        if cv.exp != 0:
            return refuse(BAD_ARG)
        if cv.c64 == 2 and not (stats and addend):
            p = c64_plan(g.N, g.Hin, g.Win, cus)
            r.kernel, r.tiles_per_block, r.blocks = "c64p", p.tiles_per_block, p.blocks
            return r
        if mask:
            return refuse(UNSUPPORTED)
        r.kernel, r.blocks = "c64t", g.N * cdiv(g.Hin, 8) * cdiv(g.Win, 32)
        return r
    if (s3 and cv.halo != 1 and not (stats and addend) and halo_supported(g.N, g.Hin, g.Win, g.Cin, g.Cout)
            and (cv.halo == 2 or g.Cin >= 128)):
        p = halo_plan(g.N, g.Hin, g.Win, g.Cin, g.Cout, cv.exp, cus)
        r.kernel, r.tiles_per_block, r.blocks = f"halo-k{p.kpb}", p.tiles_per_block, p.blocks
        return r
    if mask:
        return refuse(UNSUPPORTED)
    classes = parity_classes(g, pair)
    for c in classes:
        if c.M >= 2 ** 24 or c.Hs * c.Ws >= 2 ** 16 or c.nkh > 16 or c.nkw > 16:
            return refuse(UNSUPPORTED)
    if not classes:
        return r
    if (not (stats and addend) and cv.pgemm != 1 and
            (cv.pgemm == 2 or pair or (g.Cout % 128 == 0 and (g.up != 1 or (g.down != 1 and g.Kh * g.Kw > 1) or
                                                              (g.Kh == 1 and g.Kw == 1 and g.down == 1))))):
        p = pgemm_plan(classes, g.Cout, stats, cus)
        r.kernel, r.tiles_per_block, r.blocks = f"pgemm{p.PN}", p.tiles_per_block, p.blocks
        return r
    r.kernel = "igemm64" if g.Cout % 128 else "igemm128"
    r.blocks = cdiv(max(c.M for c in classes), 256) * (g.Cout // (64 if g.Cout % 128 else 128)) * len(classes)
    return r


def maskadd_supported(g):
    if not same3x3(g) or g.N <= 0:
        return 0
    if g.Cin == 64 and g.Cout == 64:
        return 1
    return int(g.Cin >= 128 and halo_supported(g.N, g.Hin, g.Win, g.Cin, g.Cout))


def bnbwd_supported(g):
    return int(same3x3(g) and g.N > 0 and g.Cin >= 128 and halo_supported(g.N, g.Hin, g.Win, g.Cin, g.Cout))


# ---- weight gradient
def wgrad_plan(N, Cin, Hout, Wout, Cout, Kh, Kw):
    M = N * Hout * Wout
    p = Box(big=Cin % 128 == 0 and Cout % 128 == 0)
    tc, bkp = (128, 64) if p.big else (64, 128)
    p.bkp = bkp
    p.ktiles = cdiv(M, bkp)
    p.tiles = (Cout // tc) * (Cin // tc) * Kh * Kw
    splits = min(cdiv(1280, p.tiles), cdiv(p.ktiles, 8))
    splits = min(max(splits, 1), 4096)
    p.ktiles_per_split = cdiv(p.ktiles, splits)
    p.splits = cdiv(p.ktiles, p.ktiles_per_split)
    p.table_bytes = cdiv(M * 8, 256) * 256
    p.elems = Cout * Kh * Kw * Cin
    p.partial_bytes = p.splits * p.elems * 4
    return p


def _pair_plan(N, Ho, Wo, pairs, th, cus):
    p = Box(pack=4 if Wo <= 7 else 2 if Wo <= 15 else 1, pairs=pairs)
    p.slot = {4: 8, 2: 16, 1: 32}[p.pack]
    Wv = Wo if p.pack == 1 else 32
    p.total_tiles = cdiv(N, p.pack) * cdiv(Ho, th) * cdiv(Wv, 32)
    per_pair = cus // pairs if cus >= pairs else 1
    p.tiles_per_block = cdiv(p.total_tiles, per_pair)
    p.blocks_per_pair = cdiv(p.total_tiles, p.tiles_per_block)
    return p


def wc128b_plan(N, H, W, Cin, Cout, cus=CUS):
    if Cin % 128 or Cout % 64 or min(N, H, W) <= 0:
        return None
    p = _pair_plan(N, H, W, (Cin // 128) * (Cout // 64), 4, cus)
    p.bytes = p.pairs * p.blocks_per_pair * 64 * 9 * 128 * 4
    return p


def ws2_plan(N, Hi, Wi, Cin, Cout, cus=CUS):
    if Cin % 64 or Cout % 128 or min(N, Hi, Wi) <= 0 or Hi % 2 or Wi % 2:
        return None
    p = _pair_plan(N, Hi // 2, Wi // 2, (Cin // 64) * (Cout // 128), 2, cus)
    p.bytes = p.pairs * p.blocks_per_pair * 128 * 9 * 64 * 4
    return p


def wc64_plan(N, H, W, cus=CUS):
    p = Box(total_tiles=N * cdiv(H, 4) * cdiv(W, 32))
    p.tiles_per_block = cdiv(p.total_tiles, cus)
    p.blocks = cdiv(p.total_tiles, p.tiles_per_block)
    p.bytes = p.blocks * 64 * 9 * 64 * 4
    return p


def wgrad_geom(N, H, W, Ci, Co, kh, s, p, kw=None):
    kw = kh if kw is None else kw
    return Box(N=N, Hin=H, Win=W, Cin=Ci, Hout=(H + 2 * p - kh) // s + 1, Wout=(W + 2 * p - kw) // s + 1, Cout=Co, Kh=kh, Kw=kw,
               stride=s, pad=p)


def wgrad_dispatch(g, variant=0, cus=CUS):
    """conv2d_wgrad_dispatch -> Box(code, kernel, need (bytes the kernel that runs checks for), tiles_per_block, splits)"""
    r = Box(code=OK, kernel=None, need=0, tiles_per_block=1, splits=1)
    if variant & ~(16 | 32):
        r.code = BAD_ARG
        return r
    if g.Cin % 64 or g.Cout % 64:
        r.code = UNSUPPORTED
        return r
    k3 = g.Kh == 3 and g.Kw == 3
    same = k3 and g.stride == 1 and g.pad == 1 and g.Hin == g.Hout and g.Win == g.Wout
    if g.Cin == 64 and g.Cout == 64 and same:
        p = wc64_plan(g.N, g.Hin, g.Win, cus)
        r.kernel, r.need, r.tiles_per_block = "wc64", p.bytes, p.tiles_per_block
        return r
    if g.Cin % 128 == 0 and same and not variant & 16:
        p = wc128b_plan(g.N, g.Hin, g.Win, g.Cin, g.Cout, cus)
        r.kernel, r.need, r.tiles_per_block, r.pack = "wc128b", p.bytes, p.tiles_per_block, p.pack
        return r
    if (g.Cout % 128 == 0 and k3 and g.stride == 2 and g.pad == 1 and g.Hin == 2 * g.Hout and g.Win == 2 * g.Wout and
            not variant & 16 and ((g.Cin // 64) * (g.Cout // 128) <= 4 or variant & 32)):
        p = ws2_plan(g.N, g.Hin, g.Win, g.Cin, g.Cout, cus)
        r.kernel, r.need, r.tiles_per_block, r.pack = "ws2", p.bytes, p.tiles_per_block, p.pack
        return r
    p = wgrad_plan(g.N, g.Cin, g.Hout, g.Wout, g.Cout, g.Kh, g.Kw)
    r.kernel, r.need, r.splits = ("wtap-big" if p.big else "wtap-small"), p.table_bytes + p.partial_bytes, p.splits
    r.ktiles_per_split, r.bkp = p.ktiles_per_split, p.bkp
    return r


def wgrad_workspace_bytes(g, cus=CUS):
    """isic_conv2d_wgrad_workspace_bytes (the stride is not an argument)"""
    p = wgrad_plan(g.N, g.Cin, g.Hout, g.Wout, g.Cout, g.Kh, g.Kw)
    need = p.table_bytes + p.partial_bytes + 256
    if g.Kh == 3 and g.Kw == 3:
        if g.Cin == 64 and g.Cout == 64:
            need = max(need, wc64_plan(g.N, g.Hout, g.Wout, cus).bytes)
        if g.Cin % 128 == 0:
            need = max(need, wc128b_plan(g.N, g.Hout, g.Wout, g.Cin, g.Cout, cus).bytes)
        if g.Cout % 128 == 0:
            need = max(need, ws2_plan(g.N, 2 * g.Hout, 2 * g.Wout, g.Cin, g.Cout, cus).bytes)
    return need


# ================================================================== generators
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def dyadic(shape, bits, bound, g):
    """multiples of 2^-bits in [-bound, bound]"""
    s = 2 ** bits
    return torch.randint(-bound * s, bound * s + 1, shape, generator=g).float() / s


def full_bf16(shape, emax, g):
    """+-(128 .. 255) * 2^(e - 7), e in [-emax, emax]: eight significant bits, 2^-emax <= |v| < 2^(emax + 1)"""
    m = torch.randint(128, 256, shape, generator=g).float()
    e = torch.randint(-emax, emax + 1, shape, generator=g).float()
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    v = sign * m * torch.exp2(e - 7)
    assert torch.equal(v.bfloat16().float(), v)
    return v


SEL = (0.5, -1.0, 2.0, -0.5, 1.0, -2.0)


def chunk_ends(C):
    return [c for k in range(C // 64) for c in (64 * k, 64 * k + 63)]


def selector_weight(Cout, Kh, Kw, Cin):
    """one non-zero per output channel: the taps in turn, the channels at both ends of every 64-channel chunk"""
    w = torch.zeros(Cout, Kh, Kw, Cin)
    ends = chunk_ends(Cin)
    for co in range(Cout):
        tap = co % (Kh * Kw)
        w[co, tap // Kw, tap % Kw, ends[(co // (Kh * Kw) + co) % len(ends)]] = SEL[co % 6]
    return w


def sparse_weight(Cout, Kh, Kw, Cin, g, nnz=4):
    w = torch.zeros(Cout, Kh * Kw * Cin)
    idx = torch.randint(0, Kh * Kw * Cin, (Cout, nnz), generator=g)
    val = torch.tensor([0.5, -0.5, 1.0, -1.0])[torch.randint(0, 4, (Cout, nnz), generator=g)]
    w.scatter_(1, idx, val)                                  # a repeated index keeps one value: AT MOST nnz non-zeros
    return w.view(Cout, Kh, Kw, Cin)


def exact_condition(terms, amax, bmax, grid_bits, extra=0.0):
    """the trivial bound: every partial sum is a multiple of 2^-grid_bits of magnitude <= terms * amax * bmax + extra"""
    return (terms * amax * bmax + extra) * 2 ** grid_bits < 2 ** 24


def stats_condition(pixels, vmax, grid_bits):
    """one fp32 partial over `pixels` stored values (multiples of 2^-grid_bits, |v| <= vmax): sum and sum of squares exact"""
    return pixels * vmax * 2 ** grid_bits < 2 ** 24 and pixels * vmax * vmax * 2 ** (2 * grid_bits) < 2 ** 24


def pack_mask(bits):
    """bool [..., C] -> uint8 [..., C / 8]: bit j of a byte = channel 8 * byte + j (isic_bn_apply_mask_bf16)"""
    b = bits.reshape(-1, 8).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


def conv_inputs(cid, g, family, addend=False, pair=False):
    """-> Box(x [N, Hin, Win, Cin], w [Cout, Kh, Kw, Cin], addend [N, Hout, Wout, Cout] or None, x2, w2 (pair), vmax, grid)"""
    rng = _gen(cid, family)
    xs, ws, os_ = (g.N, g.Hin, g.Win, g.Cin), (g.Cout, g.Kh, g.Kw, g.Cin), (g.N, g.Hout, g.Wout, g.Cout)
    taps = max(c.nkh * c.nkw for c in parity_classes(g)) if g.down == 2 else g.Kh * g.Kw
    terms = taps * g.Cin + (g.Cin if pair else 0)
    inp = Box(addend=None, x2=None, w2=None)
    if family == "I":
        inp.x, inp.w = dyadic(xs, 3, 1, rng), dyadic(ws, 3, 1, rng)
        if pair:
            inp.x2, inp.w2 = dyadic(xs, 3, 1, rng), dyadic((g.Cout, 1, 1, g.Cin), 3, 1, rng)
        if addend:
            inp.addend = dyadic(os_, 3, 4, rng)
        assert exact_condition(terms, 1, 1, 6, 4.0), (cid, terms)
    elif family == "P":
        inp.x, inp.w = full_bf16(xs, 6, rng), selector_weight(g.Cout, g.Kh, g.Kw, g.Cin)
        if pair:
            inp.x2, inp.w2 = full_bf16(xs, 4, rng), selector_weight(g.Cout, 1, 1, g.Cin)
        if addend:
            inp.addend = full_bf16(os_, 4, rng)
        # s x: multiples of 2^(-6 - 7 - 1) below 2^8; the addend / second term: multiples of 2^(-4 - 7 - 1) below 2^6
        assert 2 ** 14 * (2 ** 8 + 2 ** 6) < 2 ** 24
    else:                                                       # S
        inp.x, inp.w = dyadic(xs, 2, 1, rng), sparse_weight(g.Cout, g.Kh, g.Kw, g.Cin, rng)
        if addend:
            inp.addend = dyadic(os_, 3, 4, rng)
        inp.vmax, inp.grid = (8.0 if addend else 4.0), 3     # <= 4 products of magnitude <= 1, multiples of 1/8
    return inp


# ================================================================== references
def _canvas(g, x):
    """x [N, Hin, Win, C] -> fp64 NCHW canvas on which the convolution is a plain correlation of stride `up` without padding:
    source pixel h sits at row down * h + pad (the rows between are the fractional taps: zeros)"""
    Hc, Wc = (g.Hout - 1) * g.up + g.Kh, (g.Wout - 1) * g.up + g.Kw
    cv = torch.zeros(g.N, x.shape[3], Hc, Wc, dtype=F64)
    hs = [h for h in range(g.Hin) if 0 <= g.down * h + g.pad < Hc]
    ws = [w for w in range(g.Win) if 0 <= g.down * w + g.pad < Wc]
    if hs and ws:
        src = x.double().permute(0, 3, 1, 2)[:, :, hs[0]:hs[-1] + 1, ws[0]:ws[-1] + 1]
        cv[:, :, g.down * hs[0] + g.pad:g.down * hs[-1] + g.pad + 1:g.down, g.down * ws[0] + g.pad:g.down * ws[-1] + g.pad + 1:g.down] = src
    return cv


def conv_ref(g, x, w):
    """out[n, ho, wo, co] = sum in[n, (ho up + kh - pad) / down, (wo up + kw - pad) / down, ci] w[co, kh, kw, ci] in fp64 (NHWC)"""
    y = F.conv2d(_canvas(g, x), w.double().permute(0, 3, 1, 2), None, g.up)
    assert y.shape[2:] == (g.Hout, g.Wout)
    return y.permute(0, 2, 3, 1).contiguous()


def pair_geoms(N, H, W, C, Co):
    """the two data gradients isic_conv2d_dgrad_pair_bf16 joins"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return geom(N, Ho, Wo, Co, H, W, C, 3, 3, 1, 2, 1), geom(N, Ho, Wo, Co, H, W, C, 1, 1, 1, 2, 0)


def round_bf16(exact):
    """the single rounding (ties to even) of an exact fp64 value that fp32 holds exactly"""
    f = exact.float()
    assert torch.equal(f.double(), exact), "the exact result does not fit fp32: the case breaks its own condition"
    return f.bfloat16()


def rne_bits(f32):
    """fp32 -> bf16 bit patterns by integer arithmetic (finite values): add 0x7FFF + the lowest kept bit, shift"""
    b = f32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).to(torch.int32)


def truncate_bf16(exact):
    b = exact.float().contiguous().view(torch.int32) & -65536
    return b.view(torch.float32).bfloat16()


def stats_ref(stored):
    """bf16 [.., C] -> fp64 per-channel sum and sum of squares of the stored tensor"""
    o = stored.double().reshape(-1, stored.shape[-1])
    return o.sum(0), (o * o).sum(0)


def wgrad_ref(g, x, dy, drop=None, gap_fault=False):
    """dW[co][kh][kw][ci] = sum dY[n, ho, wo, co] X[n, ho s + kh - p, wo s + kw - p, ci] in fp64, as nine (Kh Kw) shifted
    products.  Emulated faults: drop = (a, b): the flat output pixels [a, b) are left out (a lost split-K slab);
    gap_fault: the padding column left of image n holds image n - 1's last column (a packed image reads its neighbour)"""
    s, p = g.stride, g.pad
    Hc, Wc = max((g.Hout - 1) * s + g.Kh, g.Hin + p), max((g.Wout - 1) * s + g.Kw, g.Win + p)
    xd = torch.zeros(g.N, Hc, Wc, g.Cin, dtype=F64)
    xd[:, p:p + g.Hin, p:p + g.Win] = x.double()
    if gap_fault and p > 0:
        xd[1:, p:p + g.Hin, p - 1] = x.double()[:-1, :, g.Win - 1]
    d2 = dy.double().reshape(-1, g.Cout).clone()
    if drop:
        d2[drop[0]:drop[1]] = 0
    dw = torch.zeros(g.Cout, g.Kh, g.Kw, g.Cin, dtype=F64)
    for kh in range(g.Kh):
        for kw in range(g.Kw):
            xs = xd[:, kh:kh + s * (g.Hout - 1) + 1:s, kw:kw + s * (g.Wout - 1) + 1:s]
            dw[:, kh, kw] = d2.t() @ xs.reshape(-1, g.Cin)
    return dw


def wgrad_pixels(g):
    """family P: the output pixels (n, ho, wo) the non-zeros of dY sit on -- image corners, both sides of the tile seams of
    every weight-gradient kernel (rows 1|2, 3|4, columns 31|32, flat pixels 63|64, 127|128, 255|256), the last image, and the
    first and last column of the first images (next to the gap columns of packed 7- and 14-wide images)"""
    N, H, W = g.N, g.Hout, g.Wout
    px = []
    for n in sorted({0, N - 1}):
        px += [(n, 0, 0), (n, 0, W - 1), (n, H - 1, 0), (n, H - 1, W - 1)]
    for n in range(1, min(N, 6)):
        px += [(n, 0, 0), (n, min(1, H - 1), W - 1), (n, H - 1, 0), (n, H // 2, W - 1)]
    for h in (1, 2, 3, 4):
        for w in (0, W - 1, 31, 32):
            if h < H and w < W:
                px.append((0, h, w))
    M = N * H * W
    for f in (63, 64, 127, 128, 255, 256, M // 2, M - 2):
        if 0 <= f < M:
            px.append((f // (H * W), (f // W) % H, f % W))
    seen, out = set(), []
    for q in px:
        if q not in seen:
            seen.add(q)
            out.append(q)
    return out


def wgrad_inputs(cid, g, family):
    """-> Box(x, dy, dw0 (the running gradient the call adds to), grid)"""
    rng = _gen(cid, family, "wgrad")
    xs, ys, wsh = (g.N, g.Hin, g.Win, g.Cin), (g.N, g.Hout, g.Wout, g.Cout), (g.Cout, g.Kh, g.Kw, g.Cin)
    M = g.N * g.Hout * g.Wout
    inp = Box()
    if family == "I":
        bits = 3
        while not exact_condition(M, 1, 1, max(2 * bits, 3), 4.0):       # 1/8 -> 1/4 -> {0, +-1/2, +-1}
            bits -= 1
            assert bits >= 1, (cid, M)
        inp.grid = bits
        inp.x, inp.dy, inp.dw0 = dyadic(xs, bits, 1, rng), dyadic(ys, bits, 1, rng), dyadic(wsh, 3, 4, rng)
    else:
        inp.x, inp.dw0 = full_bf16(xs, 6, rng), torch.zeros(wsh)
        inp.dy = torch.zeros(ys)
        px = wgrad_pixels(g)
        for co in range(g.Cout):
            n, h, w = px[co % len(px)]
            inp.dy[n, h, w, co] = SEL[(co // len(px) + co) % 6]
    return inp


# ================================================================== emulated faults (plain torch, reference side)
def flat_conv3x3(x, w, fault=None, tile=256):
    """the 3x3 / stride 1 / pad 1 convolution as the pixels-staged-once kernels see it: tap (kh, kw) of flat pixel m is flat
    pixel m + (kh - 1) W + (kw - 1), masked where it leaves the image.  fault None reproduces conv_ref; otherwise
      "left-unmasked"  the kw = 0 tap is not masked at the left image edge (it reads the previous row's last pixel)
      "seam-shift"     every tile after the first reads its patch one row late
      "skip-ktile"     the last K-tile (tap (2, 2), last 64 channels) of the last tile is skipped"""
    N, H, W, C = x.shape
    M, Co = N * H * W, w.shape[0]
    guard = W + 3
    xp = torch.zeros(M + 2 * guard, C, dtype=F64)
    xp[guard:guard + M] = x.double().reshape(M, C)
    m = torch.arange(M)
    h, wq = (m // W) % H, m % W
    out = torch.zeros(M, Co, dtype=F64)
    last_tile = m >= (cdiv(M, tile) - 1) * tile
    for kh in range(3):
        for kw in range(3):
            vh = (h + kh - 1 >= 0) & (h + kh - 1 < H)
            valid = vh & (wq + kw - 1 >= 0) & (wq + kw - 1 < W)
            if fault == "left-unmasked" and kw == 0:
                valid = vh
            src = m + (kh - 1) * W + (kw - 1) + guard
            if fault == "seam-shift":
                src = src + (m >= tile).long()
            rows = xp[src] * valid[:, None]
            wt = w[:, kh, kw, :].double()
            if fault == "skip-ktile" and kh == 2 and kw == 2:
                part = rows[:, C - 64:] @ wt[:, C - 64:].t()
                out -= part * last_tile[:, None]
            out += rows @ wt.t()
    return out.view(N, H, W, Co)


def parity_fault(g, x, w):
    """the class of the even rows / odd columns of a down = 2 launch written with the mirrored taps"""
    good, bad = conv_ref(g, x, w), conv_ref(g, x, w.flip(2))
    out = good.clone()
    out[:, 0::2, 1::2] = bad[:, 0::2, 1::2]
    return out


def two_roundings(conv_exact, addend):
    """the convolution rounded to bf16 before the addend joins it"""
    return (conv_exact.float().bfloat16().float() + addend.float()).bfloat16()


# ================================================================== case tables
def n_for_tiles(tpb, tiles_of_n, lo=1):
    """the smallest N >= lo for which the mirror gives `tpb` tiles per block"""
    n = lo
    while tiles_of_n(n) < tpb:
        n += 1
    assert tiles_of_n(n) == tpb, (tpb, n)
    return n


G, T, PS, H2, H1, PG = 1110, 1120, 1130, 200, 10200, 2100     # variants: generic, c64 tile, c64 persistent, halo (two loops), pgemm
ALL = ("plain", "add", "stats", "stats+add")
PAS = ("plain", "add", "stats")


def conv_cases(cus=CUS):
    """-> [Box(id, g, runs = ((variant, kernel, tiles per block or None), ...), epi, P (family P as well), abi (also through
    variant 0 / isic_conv2d_igemm_bf16: the kernel the shipped dispatch picks))]"""
    C = []

    def add(cid, g, runs, epi=ALL, P=False, abi=False):
        C.append(Box(id=cid, g=g, runs=tuple(runs), epi=epi, P=P, abi=abi))

    def gen(g):
        return "igemm64" if g.Cout % 128 else "igemm128"
    # ---- the generic kernels <256, 64> and <256, 128>
    for cid, g, P, abi in (
            ("g-m1", fwd(1, 1, 1, 64, 64, 3, 1, 1), True, False),
            ("g-m255", fwd(1, 15, 17, 128, 128, 3, 1, 1), True, False),
            ("g-m256", fwd(1, 16, 16, 64, 128, 3, 1, 1), False, True),
            ("g-m257", fwd(1, 257, 1, 192, 192, 3, 1, 1), True, False),
            ("g-3x3-pad0", fwd(2, 9, 11, 64, 128, 3, 1, 0), True, True),
            ("g-3x3-pad2", fwd(2, 9, 11, 128, 64, 3, 1, 2), True, True),
            ("g-1x3", fwd(2, 8, 9, 64, 64, 1, 1, 1, kw=3), True, True),
            ("g-3x1", fwd(2, 8, 9, 64, 192, 3, 1, 1, kw=1), True, False),
            ("g-5x5-pad2", fwd(3, 10, 7, 64, 128, 5, 1, 2), True, True),
            ("g-7x7-pad3", fwd(2, 9, 9, 64, 64, 7, 1, 3), True, False),
            ("g-2x2-s2-pad0", fwd(3, 10, 12, 128, 192, 2, 2, 0), True, False),
            ("g-3x3-s2-fwd", fwd(3, 9, 11, 64, 64, 3, 2, 1), False, True)):
        add(cid, g, [(G, gen(g), None)], ALL, P, abi)
    for cid, g, abi in (
            ("g-dgrad-3x3s2-odd-co64", dgrad(3, 9, 11, 64, 128, 3, 2, 1), True),      # classes 5x6, 5x5, 4x6, 4x5
            ("g-dgrad-3x3s2-odd-co128", dgrad(3, 9, 11, 128, 64, 3, 2, 1), False),
            ("g-dgrad-1x1s2", dgrad(3, 9, 11, 64, 128, 1, 2, 0), True),               # three classes without a tap
            ("g-dgrad-1x1s2-co192", dgrad(2, 8, 8, 192, 64, 1, 2, 0), False),
            ("g-dgrad-5x5s2", dgrad(2, 9, 10, 64, 64, 5, 2, 2), False)):
        add(cid, g, [(G, gen(g), None)], ("plain", "add"), True, abi)
    # ---- 64 -> 64: tile per block and persistent
    def c64(cid, N, H, W, tpb=None, P=False, abi=False):
        g = fwd(N, H, W, 64, 64, 3, 1, 1)
        add(cid, g, [(T, "c64t", None), (PS, "c64p", tpb)], ALL, P, abi)
    c64("c64-1x1", 1, 1, 1, 1, True)
    c64("c64-8x32", 2, 8, 32, 1, True, True)
    c64("c64-9x33", 2, 9, 33, 1, True)
    c64("c64-7x31", 3, 7, 31, 1, True)
    for t in (2, 3):
        N = n_for_tiles(t, lambda n: c64_plan(n, 3, 5, cus).tiles_per_block)
        c64(f"c64-tiny-{t}tiles", N, 3, 5, t, True, t == 2)
    N = n_for_tiles(3, lambda n: c64_plan(n, 56, 56, cus).tiles_per_block)
    c64("c64-56x56-3tiles", N, 56, 56, 3)
    # ---- conv_halo: both K loops
    def halo(cid, N, H, W, Ci, Co, tpb=None, P=False, abi=False, epi=PAS):
        g = fwd(N, H, W, Ci, Co, 3, 1, 1)
        if halo_supported(N, H, W, Ci, Co):
            k = halo_plan(N, H, W, Ci, Co, 0, cus).kpb
            runs = [(H2, f"halo-k{k}", tpb), (H1, "halo-k1", tpb)]
        else:
            runs = [(H2, gen(g), None)]                       # must leave the kernel
        add(cid, g, runs, epi, P, abi)
    halo("halo-w1", 3, 40, 1, 128, 128, 1, True)
    halo("halo-w63", 2, 5, 63, 64, 128, 1, True)
    halo("halo-w63-c128", 1, 5, 63, 128, 128, 1, False, True)
    halo("halo-w64-leaves", 2, 5, 64, 128, 128, None, True, True)
    halo("halo-c192", 3, 9, 10, 192, 128, 1, True)
    halo("halo-c256-co256", 5, 14, 14, 256, 256, 1, False, True)
    N = n_for_tiles(2, lambda n: halo_plan(n, 7, 7, 128, 512, 0, cus).tiles_per_block)
    halo("halo-co512-c128-2tiles", N, 7, 7, 128, 512, 2, False, True)
    N = n_for_tiles(3, lambda n: halo_plan(n, 7, 7, 64, 512, 0, cus).tiles_per_block)
    halo("halo-co512-c64-3tiles", N, 7, 7, 64, 512, 3, True)
    N = n_for_tiles(2, lambda n: halo_plan(n, 7, 7, 64, 128, 0, cus).tiles_per_block)
    halo("halo-co128-over-256-tiles", max(N, cdiv(256 * 256 + 1, 49)), 7, 7, 64, 128, None)
    # ---- conv_pgemm: 128- and 64-channel slices
    def pg(cid, g, tpb=None, epi=PAS, P=False, abi=False):
        add(cid, g, [(PG, "pgemm64" if g.Cout % 128 else "pgemm128", tpb)], epi, P, abi)
    pg("pgemm-3x3s2-fwd", fwd(3, 10, 10, 64, 128, 3, 2, 1), None, PAS, True, True)
    pg("pgemm-3x3s2-fwd-co64", fwd(33, 12, 12, 128, 64, 3, 2, 1), None, PAS, True)
    pg("pgemm-3x3s2-dgrad-co128", dgrad(5, 10, 14, 128, 256, 3, 2, 1), None, ("plain", "add"), True, True)
    pg("pgemm-3x3s2-dgrad-odd", dgrad(7, 9, 11, 128, 128, 3, 2, 1), None, ("plain", "add"), True, True)
    pg("pgemm-3x3s2-dgrad-co64", dgrad(9, 12, 12, 64, 128, 3, 2, 1), None, ("plain", "add"), True)
    pg("pgemm-1x1s2-fwd", fwd(4, 10, 10, 64, 128, 1, 2, 0), None, PAS, True, True)
    pg("pgemm-1x1s1-fwd", fwd(3, 9, 9, 128, 128, 1, 1, 0), None, PAS, True, True)
    pg("pgemm-s1-forced", fwd(5, 7, 7, 256, 256, 3, 1, 1), None, PAS, True)
    g2 = lambda n: fwd(n, 14, 14, 64, 512, 3, 2, 1)
    N = n_for_tiles(2, lambda n: pgemm_plan(parity_classes(g2(n)), 512, False, cus).tiles_per_block)
    pg("pgemm-co512-2tiles", g2(N), 2, PAS, False, True)
    g3 = lambda n: fwd(n, 14, 14, 64, 512, 1, 2, 0)
    N = n_for_tiles(3, lambda n: pgemm_plan(parity_classes(g3(n)), 512, False, cus).tiles_per_block, 300)
    pg("pgemm-co512-1x1-3tiles", g3(N), 3, PAS, True)
    return C


def pair_cases(cus=CUS):
    """isic_conv2d_dgrad_pair_bf16: (N, H, W, C, Co) of the block; runs = (variant, kernel)"""
    C = []
    for cid, N, H, W, Cc, Co in (("pair-c64-even", 3, 12, 12, 64, 128), ("pair-c64-odd", 3, 9, 11, 64, 64),
                                 ("pair-c128-even", 5, 14, 14, 128, 256), ("pair-c128-odd", 2, 9, 11, 128, 128)):
        g3, g1 = pair_geoms(N, H, W, Cc, Co)
        runs = ((0, f"pgemm{128 if Cc % 128 == 0 else 64}"), (1000, "igemm64" if Cc % 128 else "igemm128"),
                (2000, f"pgemm{128 if Cc % 128 == 0 else 64}"))
        C.append(Box(id=cid, g=g3, g1=g1, runs=runs))
    return C


def maskadd_cases(cus=CUS):
    C = []
    N2 = n_for_tiles(2, lambda n: c64_plan(n, 3, 5, cus).tiles_per_block)
    for cid, g, kernel in (("mask-c64-9x33", fwd(2, 9, 33, 64, 64, 3, 1, 1), "c64p"),
                           ("mask-c64-tiny-2tiles", fwd(N2, 3, 5, 64, 64, 3, 1, 1), "c64p"),
                           ("mask-halo-c128", fwd(3, 9, 10, 128, 128, 3, 1, 1), "halo-k2"),
                           ("mask-halo-c192-co256", fwd(2, 7, 7, 192, 256, 3, 1, 1), "halo-k1"),
                           ("mask-halo-w63", fwd(1, 5, 63, 128, 128, 3, 1, 1), "halo-k1")):
        C.append(Box(id=cid, g=g, kernel=kernel))
    return C


# geometries on which ..._maskadd_supported / ..._dgrad_bnbwd_supported must agree with the mirror (and the entry must refuse
# with ISIC_ERR_UNSUPPORTED where it says 0)
SUPPORT_PROBES = (fwd(1, 5, 63, 128, 128, 3, 1, 1), fwd(1, 5, 64, 128, 128, 3, 1, 1), fwd(2, 5, 64, 256, 128, 3, 1, 1),
                  fwd(2, 8, 8, 128, 64, 3, 1, 1), fwd(2, 8, 8, 64, 128, 3, 1, 1), fwd(2, 8, 8, 128, 192, 3, 1, 1),
                  fwd(2, 8, 8, 128, 128, 3, 2, 1), fwd(2, 8, 8, 128, 128, 1, 1, 0), fwd(2, 8, 8, 64, 64, 3, 1, 1),
                  fwd(2, 8, 8, 192, 256, 3, 1, 1))


def bnbwd_cases(cus=CUS):
    C = [Box(id="bnbwd-c128", g=fwd(3, 10, 10, 128, 128, 3, 1, 1), tpb=1), Box(id="bnbwd-c192-co256", g=fwd(5, 9, 11, 192, 256, 3, 1, 1), tpb=1),
         Box(id="bnbwd-w63", g=fwd(1, 5, 63, 128, 128, 3, 1, 1), tpb=1)]
    N = n_for_tiles(2, lambda n: halo_plan(n, 7, 7, 128, 512, 0, cus).tiles_per_block)
    C.append(Box(id="bnbwd-co512-2tiles", g=fwd(N, 7, 7, 128, 512, 3, 1, 1), tpb=2))
    return C


def wgrad_cases(cus=CUS):
    """-> [Box(id, g, runs = ((variant, kernel, tiles per block or None), ...))]"""
    C = []

    def add(cid, g, runs, **kw):
        C.append(Box(id=cid, g=g, runs=tuple(runs), **kw))
    add("w-c64-9x33", wgrad_geom(2, 9, 33, 64, 64, 3, 1, 1), [(0, "wc64", 1), (16, "wc64", 1)])
    for t in (2, 3):
        N = n_for_tiles(t, lambda n: wc64_plan(n, 3, 5, cus).tiles_per_block)
        add(f"w-c64-tiny-{t}tiles", wgrad_geom(N, 3, 5, 64, 64, 3, 1, 1), [(0, "wc64", t)])
    for cid, N, H, W, Ci, Co in (("w-c128b-w7", 5, 7, 7, 128, 64), ("w-c128b-w8", 3, 6, 8, 128, 192), ("w-c128b-w15", 3, 5, 15, 256, 64),
                                 ("w-c128b-w16", 3, 5, 16, 128, 64), ("w-c128b-w33", 1, 6, 33, 128, 128),
                                 ("w-c128b-w14-odd", 7, 14, 14, 128, 128)):
        g = wgrad_geom(N, H, W, Ci, Co, 3, 1, 1)
        add(cid, g, [(0, "wc128b", None), (16, "wtap-big" if Co % 128 == 0 else "wtap-small", None)])
    for cid, N, H, W, Ci, Co in (("w-s2-wo7", 5, 14, 14, 64, 128), ("w-s2-wo8", 3, 12, 16, 128, 128), ("w-s2-wo15", 3, 10, 30, 64, 128),
                                 ("w-s2-wo16", 2, 8, 32, 64, 256)):
        g = wgrad_geom(N, H, W, Ci, Co, 3, 2, 1)
        add(cid, g, [(0, "ws2", None), (16, "wtap-big" if Ci % 128 == 0 else "wtap-small", None)])
    g = wgrad_geom(5, 14, 14, 256, 512, 3, 2, 1)                  # 16 pairs: the per-tap kernel ships, bit 5 forces the strided one
    add("w-s2-16pairs", g, [(0, "wtap-big", None), (32, "ws2", None)])
    add("w-s2-odd-input", wgrad_geom(3, 9, 11, 64, 128, 3, 2, 1), [(0, "wtap-small", None), (32, "wtap-small", None)])
    add("w-tap-big", wgrad_geom(3, 9, 9, 128, 128, 3, 1, 1), [(16, "wtap-big", None)])
    add("w-tap-small-1split", wgrad_geom(2, 7, 9, 64, 128, 3, 1, 1), [(0, "wtap-small", None)], splits=1)
    add("w-tap-small-8splits", wgrad_geom(40, 14, 14, 64, 128, 3, 1, 1), [(0, "wtap-small", None)], splits=8)
    add("w-tap-1x1-s2", wgrad_geom(4, 10, 10, 64, 128, 1, 2, 0), [(0, "wtap-small", None)])
    add("w-tap-1x1-33splits", wgrad_geom(170, 14, 14, 64, 64, 1, 1, 0), [(0, "wtap-small", None)], splits=33)
    add("w-tap-5x5", wgrad_geom(2, 9, 9, 64, 64, 5, 1, 2), [(0, "wtap-small", None)])
    add("w-tap-3x3-pad0", wgrad_geom(2, 9, 11, 64, 64, 3, 1, 0), [(0, "wtap-small", None)])
    return C


PREP_CASES = ((64, 64, 3, 3), (128, 64, 1, 1), (64, 192, 5, 3), (256, 256, 3, 3))       # the last: 589 824 > 2048 * 256 elements


def prep_master(O, I, Kh, Kw):
    """full-mantissa fp32 masters [O][Kh][Kw][I]; every fourth value an exact tie between two bf16 neighbours"""
    rng = _gen("prep", O, I, Kh, Kw)
    n = O * Kh * Kw * I
    w = (torch.randn(n, generator=rng) * torch.exp2(torch.randint(-8, 9, (n,), generator=rng).float())).contiguous()
    b = w.view(torch.int32)
    b[::4] = (b[::4] & -65536) | 0x8000                     # exactly half a bf16 ulp above the truncated value
    return w.view(O, Kh, Kw, I)


def prep_ref(w):
    """-> (forward copy bits [O][Kh][Kw][I], dgrad copy bits [I][Kh][Kw][O] with both taps flipped), int32 bf16 patterns"""
    bits = rne_bits(w)
    return bits, bits.flip(1, 2).permute(3, 1, 2, 0).contiguous()
