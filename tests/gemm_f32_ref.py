"""Case tables, input generators and references for the exact-fp32 GEMM family (csrc/gemm_f32.hip, gemm_f32p.hip,
gemm_f32t.hip, gemm_f32r.hip) behind isic_test_gemm_f32_variant.  tests/test_gemm_f32_domain_gpu.py runs the cases on the
device, tests/test_gemm_f32_ref_cpu.py shows on the CPU that the method is sound.

Method: inputs for which fp32 is exact in ANY summation order, so the device result equals the fp64 reference bit for bit.
  family I ("dyadic")    A, B multiples of 1/8 in [-1, 1]; bias, C0, addend multiples of 1/8 in [-4, 4]; beta in
                         {0, 1, 0.5, -2}.  Every product is a multiple of 2^-6 and every partial sum of any subset is a
                         multiple of 2^-6 of magnitude <= K + 16: exact while 64 (K + 16) < 2^24 (K <= 50 176 here).
  family P ("selector")  one operand full-mantissa fp32 (normals times 2^e, e in [-20, 20]); the other has exactly one
                         non-zero of {+-0.5, +-1, +-2} per output column (or row), at a chosen k: C[m][n] = s A[m][k(n)]
                         exactly, so any lost operand bit shows.  The k(n) sit at the ends of K, on both sides of the
                         boundaries of the case's plan and (A^T B kernel) in every ring slot of both K-groups.
  tanh                   the pre-activation is exact (family I with a B of <= 16 non-zeros of magnitude <= 1/2 per column
                         and a bias in [-1.5, 1.5]: |p| <= 9.5), so only isic_tanhf is in play: TANH_BOUND.
The sign of a zero is not pinned (an exact zero sum is +0 or -0 depending on the order); values are compared with ==.

The plans of the host dispatch (small_split_plan, g32_plan, tn_plan, rp_ok) are mirrored here for a given CU count: the
case table states which kernel each case is meant for, the device test asserts that this kernel accepts it."""
import zlib

import torch

F64 = torch.float64
BETAS = (0.0, 1.0, 0.5, -2.0)
CUS = 256                                    # MI355X; the device test passes the device's own count to the mirrors
TANH_DOC = 1.5e-7                            # csrc/common.h: "absolute error < 1.5e-7 everywhere"
TANH_BOUND = TANH_DOC + 2.0 ** -25           # ... plus rounding the fp64 reference to fp32 (|tanh| <= 1)
MAX_MACS = 1e9
ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
TP = 8                                       # gemm_f32t.hip: k-steps of loads in flight per wave


class Box(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def cdiv(a, b):
    return -(-a // b)


# ================================================================== mirrors of the host plans
def small_split_plan(M, N, K, plain):
    """gemm_f32.hip -> (ksplit, klen)"""
    klen = cdiv(K, 16) * 16
    tiles = cdiv(M, 64) * cdiv(N, 64)
    tiny = plain and tiles <= 8 and 256 <= K < 2048
    if not plain or (K < 2048 and not tiny) or tiles >= 512:
        return 1, klen
    want = cdiv(1024, tiles)
    want = min(want, K // 64 if tiny else K // 256)
    if want <= 1:
        return 1, klen
    klen = cdiv(cdiv(K, want), 16) * 16
    return cdiv(K, klen), klen


def g32_plan(ta, tb, M, N, K, cus=CUS):
    """gemm_f32p.hip -> Box(ok, why, swap, splits, kt_per_split, partial_bytes, tiles_per_block); `why` names the admission rule
    that refuses"""
    p = Box(ok=False, why=None, swap=False, splits=1, kt_per_split=0, partial_bytes=0, tiles_per_block=0, tiles_per_block_1=0)
    if not (K >= 64 and K % 4 == 0 and M % 4 == 0 and N % 4 == 0 and M * N < 2 ** 31):
        p.why = "shape"
        return p
    if float(M) * N * K < 1.0e8:
        p.why = "macs"
        return p
    p.swap = N > M and M <= 128
    Mr, Nr = (N, M) if p.swap else (M, N)
    mtiles, nslices, Ktiles = cdiv(Mr, 256), cdiv(Nr, 128), cdiv(K, 32)
    if Mr < 192:
        p.why = "rows"
        return p
    if Ktiles < 8 and nslices > 1:
        p.why = "ktiles"
        return p
    tiles = mtiles * nslices
    splits = 1
    if tiles * 2 <= cus and Ktiles >= 16:
        want = min(cus // tiles, Ktiles // 8)
        if want > 1:
            splits = want
    p.kt_per_split = cdiv(Ktiles, splits)
    p.splits = cdiv(Ktiles, p.kt_per_split)
    if M * N * p.splits >= 2 ** 31:
        p.why = "shape"
        return p
    if tiles * p.splits < 96:
        p.why = "items"
        return p
    p.ok = True
    p.partial_bytes = p.splits * M * N * 4 if p.splits > 1 else 0
    p.tiles_per_block = cdiv(mtiles, max(cus // (nslices * p.splits), 1))       # row tiles a persistent block walks
    p.tiles_per_block_1 = cdiv(mtiles, max(cus // nslices, 1))                  # ... when the partials find no room: one split
    return p


def tn_plan(ta, tb, M, N, K, force, cus=CUS):
    """gemm_f32t.hip -> None, or Box(slabs, steps_per_slab, total_steps, bytes)"""
    if not ta or tb or M % 64 or N % 64 or K < 4096:
        return None
    if (not force and M * N > 128 * 256) or M * N > 128 * 1024:
        return None
    tiles = cdiv(M, 128) * cdiv(N, 128)
    total = cdiv(K, 4)
    slabs = cus // tiles
    if slabs >= 8:
        slabs &= ~7
    slabs = max(slabs, 1)
    sps = max(cdiv(total, slabs), 2 * TP)
    slabs = cdiv(total, sps)
    if slabs < 2:
        return None
    return Box(slabs=slabs, steps_per_slab=sps, total_steps=total, bytes=slabs * M * N * 4)


def rp_ok(ta, M, N, K):
    """gemm_f32r.hip, the shape part (leading dimensions and pointers: multiples of 4 floats)"""
    return not ta and M >= 4096 and 16 <= K <= 128 and K % 16 == 0 and N % 64 == 0 and N >= 64


def rp_units(M, N, cus=CUS):
    """gemm_f32r.hip: per 128-column slice, the most units (16-row panel x 64 columns) a block walks with its 8 waves.  A wave
    uses a PREFETCHED unit -- the registers its hand-counted vmcnt(4) / drained wait protects -- only beyond 8 units."""
    panels = cdiv(M, 16)
    grid = min(cdiv(panels * (2 if N >= 128 else 1), 8), cus)
    return [cdiv(panels, grid) * (min(128, N - n0) // 64) for n0 in range(0, N, 128)]


def workspace_bytes(ta, tb, M, N, K, cus=CUS):
    """isic_gemm_f32_workspace_bytes"""
    t = tn_plan(ta, tb, M, N, K, True, cus)
    p = g32_plan(ta, tb, M, N, K, cus)
    ks, _ = small_split_plan(M, N, K, True)
    return max(t.bytes if t else 0, p.partial_bytes if p.ok else 0, ks * M * N * 4 if ks > 1 else 0)


def aligned(c):
    """every operand leading dimension a multiple of 4 floats and no operand pointer one float off"""
    return c.pa % 4 == 0 and c.pb % 4 == 0 and not c.oa and not c.ob


def shipped_choice(c, cus=CUS, have_ws=True):
    """the kernel variant 0 launches for a case (isic_test_gemm_f32_variant's order: 3, 4, 2, 1)"""
    plain = not c.bias and c.act == ACT_NONE
    if plain and aligned(c) and have_ws and tn_plan(c.ta, c.tb, c.M, c.N, c.K, False, cus):
        return 3
    if aligned(c) and c.pc % 4 == 0 and not c.oc and not c.obias and rp_ok(c.ta, c.M, c.N, c.K):
        return 4
    p = g32_plan(c.ta, c.tb, c.M, c.N, c.K, cus)
    if p.ok and aligned(c) and not (p.swap and c.bias):
        return 2
    return 1


def partial_floats(c, variant, cus=CUS):
    """floats of the workspace that kernel `variant` writes for a case given a full workspace"""
    if variant == 3:
        return tn_plan(c.ta, c.tb, c.M, c.N, c.K, True, cus).slabs * c.M * c.N
    if variant == 2:
        p = g32_plan(c.ta, c.tb, c.M, c.N, c.K, cus)
        return p.splits * c.M * c.N if p.splits > 1 else 0
    if variant == 1:
        ks, _ = small_split_plan(c.M, c.N, c.K, not c.bias and c.act == ACT_NONE)
        return ks * c.M * c.N if ks > 1 else 0
    return 0


# ================================================================== the case table
DEFAULTS = dict(bias=0, act=ACT_NONE, beta=0.0, pa=4, pb=4, pc=4, oa=0, ob=0, oc=0, obias=0, ws="full", P=0, add=0, padd=4,
                refuse=(), also=(0, 1), forced_only=0, why=None, inst=None)


def leading(width, pad):
    """the leading dimension of a stored matrix `width` floats wide: pad 3 -> the next value that is NOT a multiple of 4, any
    other pad -> the next multiple of 4 plus pad (pad is then a multiple of 4 itself); always > width"""
    if pad == 3:
        return width + 1 if (width + 1) % 4 else width + 2
    assert pad % 4 == 0 and pad > 0
    return cdiv(width, 4) * 4 + pad


def case(cid, variant, ta, tb, M, N, K, **kw):
    """variant: the kernel the case is meant for (it must return ISIC_OK); also: the other variants it is run with where they
    accept it; refuse: variants that must return ISIC_ERR_UNSUPPORTED and leave the output untouched.  pa / pb / pc / padd:
    the gap between the rows of A / B / C / the addend (lda = leading(width, pa): 3 = not a multiple of 4 floats, 4 or 8 = a
    multiple); oa / ob / oc / obias: the pointer is one float off
    16-byte alignment.  ws: full | short (4 bytes less) | none | misaligned.  P: also run as family P in both roles."""
    c = Box(DEFAULTS, id=cid, variant=variant, ta=ta, tb=tb, M=M, N=N, K=K)
    c.update(kw)
    assert set(c) == set(DEFAULTS) | {"id", "variant", "ta", "tb", "M", "N", "K"}, cid
    return c


TR = ((0, 0), (0, 1), (1, 0), (1, 1))
TRN = {(0, 0): "NN", (0, 1): "NT", (1, 0): "TN", (1, 1): "TT"}
EPI = ((0, ACT_NONE), (1, ACT_RELU), (1, ACT_TANH), (1, ACT_NONE))


def _v1_cases():
    shapes = ((1, 1, 1), (3, 5, 7), (63, 65, 17), (64, 64, 16), (65, 130, 33), (130, 67, 250))
    # (pa, oa, pb, ob): vector and scalar load4 per operand (ld % 4 != 0, or the pointer one float off)
    combos = ((4, 0, 4, 0), (3, 0, 4, 0), (4, 1, 4, 0), (4, 0, 3, 0), (4, 0, 4, 1), (3, 1, 3, 1), (3, 0, 3, 0), (4, 1, 4, 1))
    out = []
    for ti, (ta, tb) in enumerate(TR):
        for ci, (pa, oa, pb, ob) in enumerate(combos):
            M, N, K = shapes[(ti + ci) % 6]
            bias, act = EPI[(ci + ti // 2) % 4]
            beta = 0.0 if act == ACT_TANH else BETAS[(ti + ci // 2) % 4]
            out.append(case(f"v1-{TRN[ta, tb]}-{M}x{N}x{K}-a{pa}{oa}-b{pb}{ob}-e{bias}{act}-beta{beta}", 1, ta, tb, M, N, K, pa=pa, oa=oa,
                            pb=pb, ob=ob, bias=bias, act=act, beta=beta, pc=3 if ci % 2 else 4, oc=ci // 4 % 2,
                            P=int((M, N, K) in ((65, 130, 33), (130, 67, 250))), inst="gemm_f32_kernel"))
    # every shape in every transposition at least once, every beta on the plain epilogue
    for si, (M, N, K) in enumerate(shapes):
        for ti, (ta, tb) in enumerate(TR):
            out.append(case(f"v1-{TRN[ta, tb]}-{M}x{N}x{K}-plain-beta{BETAS[(si + ti) % 4]}", 1, ta, tb, M, N, K,
                            beta=BETAS[(si + ti) % 4], bias=(si + ti) % 2, P=int(K >= 33), inst="gemm_f32_kernel"))
    # split-K: the tiny rule (13 splits of 80 k, the last one 40) and the long rule (74 splits of 272 k, the last one 144):
    # ordered partials with a full workspace, gemm_scale_kernel + atomics with one that is 4 bytes short or absent
    for (ta, tb, M, N, K) in ((0, 0, 100, 70, 1000), (1, 0, 100, 70, 1000), (1, 0, 128, 200, 20000)):
        for ws in ("full", "short", "none"):
            for beta in (0.0, 1.0, 0.5):
                inst = ("gemm_f32_kernel + slab_reduce (split reducer)" if ws == "full" else "gemm_f32_kernel (atomics, beta = 1: no scale pass)"
                        if beta == 1.0 else "gemm_scale_kernel + gemm_f32_kernel (atomics)")
                out.append(case(f"v1-split-{TRN[ta, tb]}-{M}x{N}x{K}-ws{ws}-beta{beta}", 1, ta, tb, M, N, K, ws=ws, beta=beta,
                                pc=3 if ws == "short" else 4, P=int(beta == 0.0 and ws != "short"), inst=inst))
    return out


def _v2_cases():
    out = []
    M, N, K = 6148, 516, 260                                # 25 x 5 tiles, 9 K-tiles (the last one 4 k), one split
    for i, (ta, tb) in enumerate(TR):
        bias, act = EPI[i]
        out.append(case(f"v2-{TRN[ta, tb]}-{M}x{N}x{K}-e{bias}{act}", 2, ta, tb, M, N, K, bias=bias, act=act,
                        beta=0.0 if act == ACT_TANH else BETAS[(i + 2) % 4], P=1,
                        inst=f"gemm_f32p_kernel<{str(not ta).lower()}, {str(bool(tb)).lower()}>"))
    out.append(case("v2-NT-6148x516x260-ldc%4", 2, 0, 1, M, N, K, pc=3, bias=1, act=ACT_RELU, beta=0.5, inst="gemm_f32p_kernel vecC = 0"))
    out.append(case("v2-TN-6148x516x260-C+1", 2, 1, 0, M, N, K, oc=1, beta=-2.0, inst="gemm_f32p_kernel vecC = 0"))
    # an operand the LDS-DMA cannot take: refused by variant 2, served by the generic kernel
    out.append(case("v2-refuse-lda%4", 1, 0, 1, M, N, K, pa=3, refuse=(2,), why="lda % 4"))
    out.append(case("v2-refuse-B+1", 1, 0, 0, M, N, K, ob=1, refuse=(2,), why="B + 1"))
    # swapped roles (C^T = B^T A^T): 4 row tiles of the 772 side, 257 K-tiles in 29 splits of 9; one split without a workspace
    for (ta, tb) in ((1, 0), (0, 1)):
        for ws, beta in (("full", 0.0), ("full", 0.5), ("none", 1.0)):
            out.append(case(f"v2-swap-{TRN[ta, tb]}-128x772x8200-ws{ws}-beta{beta}", 2, ta, tb, 128, 772, 8200, ws=ws, beta=beta,
                            P=int(ws == "full" and beta == 0.0), inst="gemm_f32p_kernel transC" + (" + gemm_f32p_reduce_kernel" if ws == "full" else "")))
    out.append(case("v2-swap-TN-128x772x8200-bias", 1, 1, 0, 128, 772, 8200, bias=1, act=ACT_RELU, refuse=(2,), why="swap + bias"))
    # split-K un-swapped: 2 x 5 tiles, 129 K-tiles in 15 splits of 9 (the last one 3, its last K-tile 4 k)
    M, N, K = 260, 516, 4100
    for (ta, tb) in ((0, 1), (1, 0)):
        out.append(case(f"v2-split-{TRN[ta, tb]}-{M}x{N}x{K}-tanh", 2, ta, tb, M, N, K, bias=1, act=ACT_TANH, P=1,
                        inst="gemm_f32p_reduce_kernel"))
        for beta in BETAS:
            out.append(case(f"v2-split-{TRN[ta, tb]}-{M}x{N}x{K}-relu-beta{beta}", 2, ta, tb, M, N, K, bias=1, act=ACT_RELU, beta=beta,
                            pc=3 if beta == 1.0 else 4, inst="gemm_f32p_reduce_kernel"))
    out.append(case("v2-split-NT-260x516x4100-wsshort", 2, 0, 1, M, N, K, ws="short", bias=1, act=ACT_TANH, inst="one split"))
    out.append(case("v2-split-TN-260x516x4100-wsmisaligned", 2, 1, 0, M, N, K, ws="misaligned", beta=0.5, inst="one split"))
    out.append(case("v2-split-NN-260x516x4100-wsnone", 2, 0, 0, M, N, K, ws="none", beta=-2.0, inst="one split"))
    # more row tiles than blocks: 258 tiles of one slice over 256 CUs -> two tiles per block, the staging waves run ahead into the
    # second tile while the first one's epilogue stores (K = 68: three K-tiles, the last one 4 k; K = 64: two)
    out.append(case("v2-tiles2-NT-66000x128x68", 2, 0, 1, 66000, 128, 68, bias=1, act=ACT_RELU, beta=0.5, P=1, inst="gemm_f32p_kernel<true, true> two tiles per block"))
    out.append(case("v2-tiles2-TN-66000x128x64", 2, 1, 0, 66000, 128, 64, P=1, inst="gemm_f32p_kernel<false, false> two tiles per block"))
    # just under each admission rule: refused by variant 2, correct on variant 0 (the generic kernel)
    out.append(case("v2-under-macs", 1, 0, 1, 24324, 4, 1024, refuse=(2,), why="macs"))
    out.append(case("v2-under-rows", 1, 0, 0, 188, 1024, 4096, refuse=(2,), why="rows"))
    out.append(case("v2-under-ktiles", 1, 0, 1, 12292, 256, 224, refuse=(2,), why="ktiles", bias=1, act=ACT_RELU))
    out.append(case("v2-under-items", 1, 0, 0, 1024, 1024, 256, refuse=(2,), why="items", beta=0.5))
    return out


# the shape next to each "just under" case that the persistent kernel does take (the rule named is the only one that refuses)
V2_JUST_OVER = {"v2-under-macs": (24324, 4, 1028), "v2-under-rows": (192, 1024, 4096), "v2-under-ktiles": (12292, 256, 256),
                "v2-under-items": (6144, 1024, 256)}


def _v3_cases():
    out = []
    for i, K in enumerate((4096, 4097, 4099, 4100 + 64 * 3)):
        out.append(case(f"v3-64x64x{K}", 3, 1, 0, 64, 64, K, beta=BETAS[i], P=int(K != 4096), inst="gemm_tn_skinny_kernel"))
    out.append(case("v3-128x256x9001", 3, 1, 0, 128, 256, 9001, beta=0.5, P=1, inst="gemm_tn_skinny_kernel"))
    out.append(case("v3-128x256x9001-ldc", 3, 1, 0, 128, 256, 9001, pc=3, oc=1, inst="gemm_tn_skinny_kernel + slab_reduce xor16"))
    out.append(case("v3-forced-512x256x4096", 3, 1, 0, 512, 256, 4096, forced_only=1, beta=1.0, inst="gemm_tn_skinny_kernel"))
    out.append(case("v3-forced-64x2048x5000", 3, 1, 0, 64, 2048, 5000, forced_only=1, P=1, inst="gemm_tn_skinny_kernel"))
    # refusals
    out.append(case("v3-refuse-128x1088x4096", 1, 1, 0, 128, 1088, 4096, refuse=(3,), why="M N > 128 x 1024", also=(0,)))
    out.append(case("v3-refuse-wsnone", 1, 1, 0, 64, 64, 4096, ws="none", refuse=(3,), why="no workspace"))
    out.append(case("v3-refuse-wsshort", 1, 1, 0, 64, 64, 4096, ws="short", refuse=(3,), why="workspace 4 bytes short"))
    out.append(case("v3-refuse-bias", 1, 1, 0, 64, 64, 4096, bias=1, refuse=(3,), why="bias"))
    out.append(case("v3-refuse-act", 1, 1, 0, 64, 64, 4096, act=ACT_RELU, refuse=(3,), why="activation"))
    out.append(case("v3-refuse-M%64", 1, 1, 0, 96, 64, 4096, refuse=(3,), why="M % 64"))
    out.append(case("v3-refuse-K4095", 1, 1, 0, 64, 64, 4095, refuse=(3,), why="K < 4096"))
    return out


def _v4_cases():
    out = []
    for kc in range(1, 9):
        K = 16 * kc
        rows = ((64, 4096, kc % 2, 0.0, 0, ACT_NONE), (128, 4099, 0, 0.5, 1, ACT_RELU), (192, 4109, 1, 0.0, 1, ACT_TANH),
                ((64, 128, 192)[kc % 3], 4099 if kc % 2 else 4109, kc % 2, 0.5 if kc % 2 else 0.0, 1, ACT_RELU))
        for (N, M, tb, beta, bias, act) in rows:
            for add in (0, 1):
                if add and act == ACT_TANH:                 # the tanh bound stands alone: nothing is added after a tanh
                    act = ACT_RELU
                out.append(case(f"v4-K{K}-N{N}-M{M}-{'T' if tb else 'N'}-beta{beta}-e{bias}{act}-add{add}", 4, 0, tb, M, N, K, beta=beta,
                                bias=bias, act=act, add=add, padd=8, P=int(add == 0 and act == ACT_NONE or (N == 192 and kc in (1, 8) and not add)),
                                inst=f"gemm_rowpanel_kernel<{kc}, {'true' if add else 'false'}>"))
    # the steady state: more than 8 units per block (the grid is capped at the CU count), so a wave multiplies a unit that was
    # PREFETCHED during the previous one -- the registers the hand-counted vmcnt(4) (beta = 0, full panel) and the drained wait
    # (beta != 0) protect; with and without the addend; a ragged last panel (M % 16 = 3)
    for (M, N, K, tb) in ((40003, 128, 128, 1), (40003, 192, 32, 0), (20003, 192, 128, 0), (40003, 64, 48, 1)):
        for beta in (0.0, 0.5):
            for add in (0, 1):
                out.append(case(f"v4-steady-K{K}-N{N}-M{M}-{'T' if tb else 'N'}-beta{beta}-add{add}", 4, 0, tb, M, N, K, beta=beta, add=add, padd=8,
                                bias=int(beta != 0.0), P=int(beta == 0.0 and not add),
                                inst=f"gemm_rowpanel_kernel<{K // 16}, {'true' if add else 'false'}> steady state"))
    out.append(case("v4-add-K130", 1, 0, 1, 4096, 128, 130, add=1, bias=1, act=ACT_RELU, beta=0.5, refuse=(4,), why="K = 130", inst="add2d_kernel"))
    out.append(case("v4-refuse-M4095", 1, 0, 1, 4095, 64, 64, refuse=(4,), why="M < 4096"))
    out.append(case("v4-refuse-K8", 1, 0, 1, 4096, 64, 8, refuse=(4,), why="K < 16"))
    out.append(case("v4-refuse-K136", 1, 0, 1, 4096, 64, 136, refuse=(4,), why="K > 128"))
    out.append(case("v4-refuse-N96", 1, 0, 1, 4096, 96, 64, refuse=(4,), why="N % 64"))
    out.append(case("v4-refuse-ldc%4", 1, 0, 1, 4096, 64, 64, pc=3, refuse=(4,), why="ldc % 4"))
    out.append(case("v4-refuse-bias+1", 1, 0, 1, 4096, 64, 64, bias=1, obias=1, refuse=(4,), why="bias + 1"))
    return out


CASES = _v1_cases() + _v2_cases() + _v3_cases() + _v4_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# every kernel instantiation of the family -> the `inst` text of a case that launches it (the table of the GPU module)
INSTANTIATIONS = (["gemm_f32_kernel", "gemm_scale_kernel", "split reducer", "add2d_kernel", "gemm_f32p_reduce_kernel",
                   "gemm_tn_skinny_kernel"]
                  + [f"gemm_f32p_kernel<{a}, {b}>" for a in ("true", "false") for b in ("true", "false")]
                  + [f"gemm_rowpanel_kernel<{kc}, {add}>" for kc in range(1, 9) for add in ("false", "true")])

# isic_gemm_f32_rows_ws: the forward form x[rows] W^T + b (gathered row tiles, M % 8 != 0) and the weight-gradient form
# dY^T X[rows] (swapped roles, gathered k rows, K % 32 != 0 and K % 8 != 0); and y = a W[rows]^T with <= 128 rows of a (swapped
# roles, the gathered rows of W form the row tiles, N % 8 != 0)
ROWS_FWD = case("rows-fwd-6148x516x260", 2, 0, 1, 6148, 516, 260, bias=1, act=ACT_RELU, beta=0.5)
ROWS_WGRAD = case("rows-wgrad-128x772x8204", 2, 1, 0, 128, 772, 8204, beta=1.0)
ROWS_SWAP_NT = case("rows-swap-nt-128x772x8200", 2, 0, 1, 128, 772, 8200, beta=-2.0)     # swapped roles, B = W[rows] stored [N][K]
ROWS_FWD_TILES2 = case("rows-fwd-66004x128x68", 2, 0, 1, 66004, 128, 68, bias=1)       # the index is read again for a block's second tile
ROWS_FORMS = {"forward": (ROWS_FWD, "A"), "wgrad": (ROWS_WGRAD, "B"), "swap-nt": (ROWS_SWAP_NT, "B"), "forward-tiles2": (ROWS_FWD_TILES2, "A")}
ROWS_STORE_EXTRA = 300                        # stored rows beyond the gathered count; the last stored row is all NaN

# the run-twice checks on random normals: the split paths documented as order-fixed
REPEAT_CASES = (case("repeat-v2-split", 2, 0, 1, 260, 516, 4100, bias=1, act=ACT_TANH),
                case("repeat-v2-swap-split", 2, 1, 0, 128, 772, 8200),
                case("repeat-v3", 3, 1, 0, 128, 256, 9001, beta=0.5),
                case("repeat-v1-ws", 1, 1, 0, 128, 200, 20000, beta=1.0))


# ================================================================== generators
def input_key(c, family):
    """cases that differ only in beta, workspace, placement or the addend (drawn last) share their inputs and the fp64 product"""
    return f"{c.variant if family != 'I' else 0}/{c.ta}{c.tb}/{c.M}x{c.N}x{c.K}/{c.bias}{int(c.act == ACT_TANH)}/{family}"


def _gen(c, family):
    return torch.Generator().manual_seed(zlib.crc32(input_key(c, family).encode()))


def dyadic(shape, lim, g):
    """multiples of 1/8 in [-lim, lim]"""
    return torch.randint(-8 * lim, 8 * lim + 1, shape, generator=g).to(torch.float32) / 8


def full_mantissa(shape, g):
    e = torch.randint(-20, 21, shape, generator=g).to(torch.float32)
    return torch.randn(shape, generator=g) * torch.exp2(e)


def selector_ks(c, cus=CUS):
    """the k of interest of a case, by priority: the ends of K, (A^T B) every ring slot of both K-groups, both sides of every
    split / slab boundary of the pinned kernel's plan, both sides of every K-tile boundary (16 k: generic and row panel, 32 k:
    persistent; the A^T B kernel has k-steps of 4 rows, all of which the ring list visits)"""
    K = c.K
    ends = list(range(0, 4)) + list(range(K - 4, K))
    ring, bounds, tiles = [], [], []
    if c.variant == 1:
        ks, klen = small_split_plan(c.M, c.N, K, not c.bias and c.act == ACT_NONE)
        bounds = list(range(klen, K, klen)) if ks > 1 else []
        tiles = list(range(16, K, 16))
    elif c.variant == 2:
        p = g32_plan(c.ta, c.tb, c.M, c.N, K, cus)
        bounds = list(range(p.kt_per_split * 32, K, p.kt_per_split * 32)) if p.splits > 1 else []
        tiles = list(range(32, K, 32))
    elif c.variant == 3:
        p = tn_plan(c.ta, c.tb, c.M, c.N, K, True, cus)
        ring = [4 * s + s % 4 for s in range(2 * TP * 2 + 2)]        # slab 0: K-group s & 1, slot (s >> 1) % TP, both ring passes
        bounds = list(range(4 * p.steps_per_slab, K, 4 * p.steps_per_slab))
    elif c.variant == 4:
        tiles = list(range(16, K, 16))

    def sides(bs, seen):
        out = []
        for b in bs:
            for k in (b - 1, b):
                if 0 <= k < K and k not in seen:
                    seen.add(k)
                    out.append(k)
        return out

    ends = [k for k in dict.fromkeys(ends) if 0 <= k < K]
    seen = set(ends) | set(ring)
    bounds = sides(bounds, seen)
    tiles = sides(tiles, seen)
    return Box(ends=ends, ring=ring, bounds=bounds, tiles=tiles, all=list(dict.fromkeys(ends + ring)) + bounds + tiles)


def _thin(ks, room):
    """all of ks, or an even subsample that fits"""
    return ks if len(ks) <= room else [ks[i * len(ks) // room] for i in range(room)]


def selector_positions(c, n_out, g, cus=CUS):
    """k(j) for the n_out outputs of the selector operand: the ends and the ring, then the split / slab boundaries, then the
    K-tile boundaries (each an even subsample where they do not all fit), the rest random"""
    s = selector_ks(c, cus)
    ks = list(dict.fromkeys(s.ends + s.ring))[:n_out]
    ks += _thin(s.bounds, n_out - len(ks))
    ks += _thin(s.tiles, n_out - len(ks))
    fill = torch.randint(0, c.K, (n_out - len(ks),), generator=g).tolist()
    ks = torch.tensor(ks + fill, dtype=torch.int64)
    return ks[torch.randperm(n_out, generator=g)]


def sparse_b(K, N, g):
    """B[K][N] with at most 16 non-zeros per column, one per 1/16th of the k range, multiples of 1/8 of magnitude <= 1/2"""
    nnz = min(16, K)
    B = torch.zeros(K, N)
    cols = torch.arange(N)
    for i in range(nnz):
        lo, hi = i * K // nnz, (i + 1) * K // nnz
        k = lo + torch.randint(0, hi - lo, (N,), generator=g)
        v = torch.randint(1, 5, (N,), generator=g).to(torch.float32) / 8
        B[k, cols] = v * (torch.randint(0, 2, (N,), generator=g) * 2 - 1)
    return B


def tanh_informative(c):
    """the shapes at which the tanh inputs can carry p = 0 and |p| >= 9.25 (sixteen non-zeros of 1/2 and a bias of 1.5)"""
    return c.M >= 2 and c.N >= 3 and c.K >= 16


def inputs(c, family="I", cus=CUS):
    """-> Box(opA [M][K], opB [K][N], bias [N] | None, C0 [M][N], addend [M][N] | None): logical operands, fp32 on the CPU.
    family: I, PA (B is the selector: A's bits are in play), PB (A is the selector)."""
    M, N, K = c.M, c.N, c.K
    g = _gen(c, family)
    inp = Box(bias=None, addend=None, family=family)
    if family == "I":
        inp.opA = dyadic((M, K), 1, g)
        if c.act == ACT_TANH:
            inp.opB = sparse_b(K, N, g)
            inp.bias = torch.randint(-12, 13, (N,), generator=g).to(torch.float32) / 8
            if tanh_informative(c):
                nz = inp.opB != 0
                inp.opA[0] = 1.0
                inp.opB[:, 0] = nz[:, 0] * 0.5
                inp.opB[:, 1] = nz[:, 1] * -0.5
                inp.bias[0], inp.bias[1] = 1.5, -1.25      # p[0][0] = 9.5, p[0][1] = -9.25
                inp.opA[1] = 0.0
                inp.bias[2] = 0.0                           # p[1][2] = 0
        else:
            inp.opB = dyadic((K, N), 1, g)
            if c.bias:
                inp.bias = dyadic((N,), 4, g)
        inp.C0 = dyadic((M, N), 4, g)
        if c.add:
            inp.addend = dyadic((M, N), 4, g)
    else:
        scale = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
        if family == "PA":
            inp.opA = full_mantissa((M, K), g)
            ks = selector_positions(c, N, g, cus)
            inp.opB = torch.zeros(K, N)
            inp.opB[ks, torch.arange(N)] = scale[torch.randint(0, 6, (N,), generator=g)]
        else:
            inp.opB = full_mantissa((K, N), g)
            ks = selector_positions(c, M, g, cus)
            inp.opA = torch.zeros(M, K)
            inp.opA[torch.arange(M), ks] = scale[torch.randint(0, 6, (M,), generator=g)]
        inp.ks = ks
        inp.C0 = torch.zeros(M, N)
    return inp


def family_p_case(c):
    """the plain product of a case (no bias / activation / beta / addend): what family P runs"""
    return Box(c, bias=0, act=ACT_NONE, beta=0.0, add=0)


def random_inputs(c):
    g = _gen(c, "random")
    return Box(opA=torch.randn(c.M, c.K, generator=g), opB=torch.randn(c.K, c.N, generator=g),
               bias=torch.randn(c.N, generator=g) if c.bias else None, C0=torch.randn(c.M, c.N, generator=g), addend=None, family="R")


# ================================================================== references
_PRE = {}


def preactivation(c, inp, cache=True):
    """op(A) op(B) + bias in fp64; shared by the cases that differ only in beta / workspace / output placement"""
    key = input_key(c, inp.family)
    if cache and key in _PRE:
        return _PRE[key]
    p = inp.opA.to(F64) @ inp.opB.to(F64)
    if inp.bias is not None:
        p = p + inp.bias.to(F64)
    if cache:
        if len(_PRE) > 6:
            _PRE.pop(next(iter(_PRE)))
        _PRE[key] = p
    return p


def activate(p, act):
    return torch.relu(p) if act == ACT_RELU else torch.tanh(p) if act == ACT_TANH else p


def reference(c, inp, cache=False):
    """-> Box(pre, out): fp64 pre-activation and act(pre) + beta C0 + addend.  For families I and P (act != tanh) out is exactly
    representable in fp32: out.float() is THE answer."""
    pre = preactivation(c, inp, cache)
    out = activate(pre, c.act)
    if c.beta != 0.0:
        out = out + c.beta * inp.C0.to(F64)
    if inp.addend is not None:
        out = out + inp.addend.to(F64)
    return Box(pre=pre, out=out)


def exact_in_fp32(t64):
    return bool((t64.float().to(F64) == t64).all())


def tanh_error(got32, ref):
    """max |device - tanh(pre)| of a tanh case (beta = 0, no addend), and the exact-saturation / zero conditions"""
    err = float((got32.to(F64) - ref.out).abs().max())
    sat = ref.pre.abs() >= 9.25
    sat_ok = bool((got32[sat].to(F64) == torch.sign(ref.pre[sat])).all())
    zero_ok = bool((got32[ref.pre == 0] == 0).all())
    return err, sat_ok, zero_ok


# ================================================================== storage
def stored(op, trans):
    """the matrix as the ABI stores it: op(X) = X^T when trans"""
    return op.t().contiguous() if trans else op.contiguous()


def padded8(rows, pad_value):
    """an index padded to a multiple of 8 entries as isic_hip/pca.py::_padded8 does, the pad entries = pad_value"""
    pad = -rows.numel() % 8
    return torch.cat([rows, torch.full((pad,), pad_value, dtype=rows.dtype)])


def gather_index(n, n_valid, g):
    """n row numbers < n_valid with repeated and descending rows"""
    idx = torch.randint(0, n_valid, (n,), generator=g, dtype=torch.int32)
    m = min(n // 4, 64)
    idx[:m] = torch.arange(n_valid - 1, n_valid - 1 - m, -1, dtype=torch.int32)          # descending
    idx[m:2 * m] = idx[0]                                                                  # repeated
    return idx
