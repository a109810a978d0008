"""numpy / torch-CPU restatement of the HBM-bound companion kernels of the conv encoder (csrc/encoder_ops.hip): the BatchNorm
forward (statistics, finalize, eval affine, the three apply entries), the 3x3/2 max-pool and the global average pool, forward
and backward, and the NCHW -> NHWC4 packing.  Each function restates the semantics include/isic_hip.h documents; where the
kernel's order of operations is fixed it is emulated, so that the device can be compared bit for bit.

Three conventions:
  * fp32 steps are np.float32 operations (correctly rounded, as the device's +, *, / and sqrtf are with the default
    -fhip-fp32-correctly-rounded-divide-sqrt; `build_rounds_correctly` reads the build's flags).
  * a * b + c may or may not be contracted to one fused multiply-add by the compiler.  `fma32` is the exact fmaf (one
    rounding); every function that contains such an expression returns ALL candidate roundings, stacked on axis 0, and a
    comparison asks the device's value to be one of them.  The "exact" input families of the GPU module are built so that
    the candidates coincide, and then every element is compared for equality.
  * `variant=` selects a named WRONG form of an operation; tests/test_encoder_ops_ref_cpu.py shows that each is rejected on
    the inputs the GPU module uses.

Used by tests/test_encoder_ops_ref_cpu.py (the reference against torch's CPU operators) and
tests/test_encoder_ops_domain_gpu.py (the device against the reference)."""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from bn_bwd_ref import bf16_bits, bf16_value          # noqa: F401  (re-exported)
from conv_bf16_ref import pack_mask                   # noqa: F401  (re-exported)

F32 = np.float32
F64 = np.float64
BF = torch.bfloat16
SENTINEL = 0x7FC1          # a bf16 NaN pattern no kernel writes
BYTE_SENTINEL = 0xEE


# ---------------------------------------------------------------------------------------------- launch geometry
FLAT_APPLY = 2                 # encoder_ops.hip:20  vectors per thread of bn_apply_kernel
STREAM_CAP = 1 << 22           # encoder_ops.hip:788 grid cap of the streaming passes (2^31 vectors at FLAT_APPLY = 2)
STATS_GRID_CAP = 2048          # encoder_ops.hip:845 grid_for(rows, rls * 8, 2048) in isic_bn_stats_bf16
AVG_BWD_GRID_CAP = 8192        # encoder_ops.hip:789 grid_for's default cap, taken by isic_avgpool_bwd_bf16 (:1048)
GRID_Y_MAX = 65535             # encoder_ops.hip:1058 gridDim.y of nchw_to_nhwc4_x4_kernel


def grid_for(n, block, cap=8192):
    """encoder_ops.hip:789"""
    g = (n + block - 1) // block
    return int(1 if g < 1 else (cap if g > cap else g))


def bn_c_ok(C):
    """encoder_ops.hip:793: C / 8 channel groups must divide the 256-thread block"""
    return C % 8 == 0 and C // 8 <= 256 and 256 % (C // 8) == 0


def block_rows(rows, rls, grid, b, variant=None):
    """bn_bwd_math.inc:49 isic_bn_bwd::block_rows -> [begin, end) of block b.
    variant "drop-partial": the end rounded DOWN to whole groups of rls rows (the last partial group is lost)."""
    per_block = ((rows + grid - 1) // grid + rls - 1) // rls * rls
    begin = b * per_block
    end = min(begin + per_block, rows)
    if variant == "drop-partial":
        end = begin + max(end - begin, 0) // rls * rls
    return begin, end


def stats_geometry(rows, C):
    """-> (rls, grid, per_block, k): row lanes per block, blocks, rows per block, fp32 terms a thread adds at most"""
    rls = 256 // (C // 8)
    grid = grid_for(rows, rls * 8, STATS_GRID_CAP)
    per_block = ((rows + grid - 1) // grid + rls - 1) // rls * rls
    return rls, grid, per_block, per_block // rls


def apply_grid(nvec):
    """blocks of bn_apply_kernel (encoder_ops.hip:882): each covers FLAT_APPLY rows of 256 vectors"""
    return grid_for(nvec, 256 * FLAT_APPLY, STREAM_CAP)


def build_rounds_correctly(flags):
    """True when nothing in the hipcc flags gives up the correctly rounded fp32 divide / sqrt (the HIP default) or allows
    value-changing floating-point rewrites."""
    bad = ("-fno-hip-fp32-correctly-rounded-divide-sqrt", "-ffast-math", "-Ofast", "-funsafe-math-optimizations",
           "-freciprocal-math", "-fapprox-func", "-fgpu-approx-transcendentals", "-fassociative-math")
    return not any(f in bad or f.startswith("-ffp-model=fast") for f in flags)


# ---------------------------------------------------------------------------------------------- exact fmaf
def fma32(a, b, c):
    """fmaf(a, b, c) for finite fp32 operands with a normal result: ONE rounding of the exact a * b + c.
    The product of two fp32 values is exact in fp64; TwoSum gives the fp64 sum s and its exact error e.  Rounding s to fp32
    differs from rounding the exact value only when s sits exactly on an fp32 rounding boundary (a midpoint, which fp64
    holds) while e != 0; then the neighbour on e's side is the answer."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    mid = (s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    toward = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    return np.where(mid & (e != 0), toward, s).astype(np.float32)


def fma32_fraction(a, b, c):
    """The same by rational arithmetic, element by element (slow; the check of fma32)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float32) for v in (a, b, c)))
    out = np.empty(a.shape, dtype=np.float32)
    for i in np.ndindex(a.shape):
        out[i] = round_fraction_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def round_fraction_f32(q):
    """nearest-even fp32 of a rational (normal range)"""
    if q == 0:
        return F32(0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    scaled = q / Fraction(2) ** (e - 23)                       # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return F32(sign * math.ldexp(n, e - 23))


def muladd_candidates(a, b, c):
    """a * b + c in fp32: [unfused, fused], stacked on axis 0"""
    a, b, c = (np.asarray(v, dtype=np.float32) for v in (a, b, c))
    return np.stack(np.broadcast_arrays(a * b + c, fma32(a, b, c)))


def distinct_candidates(cands):
    """the largest number of distinct values any element has among the stacked candidates"""
    c = np.sort(np.asarray(cands).reshape(len(cands), -1).view(np.uint32 if cands.dtype == np.float32 else cands.dtype), axis=0)
    return int(1 + (np.diff(c, axis=0) != 0).sum(axis=0).max())


def among(got, cands):
    """element-wise: the bit pattern of got equals that of one of the stacked candidates"""
    view = np.uint32 if np.asarray(got).dtype == np.float32 else np.asarray(got).dtype
    g = np.ascontiguousarray(got).view(view)
    return (np.ascontiguousarray(cands).view(view) == g[None]).any(axis=0)


# ---------------------------------------------------------------------------------------------- BatchNorm statistics
def fsum_columns(v):
    """math.fsum of every column of an fp64 [rows, C] array: the correctly rounded sums"""
    return np.array([math.fsum(v[:, c].tolist()) for c in range(v.shape[1])], dtype=np.float64)


def stats_exact(x):
    """x: fp32 values of bf16 [rows, C], multiples of 2^-17 (real_family sees to that) -> (sum, sumsq, sum |x|) per channel:
    the sums in int64 (exact), each then rounded once to fp64 -- what math.fsum would return, at numpy's speed."""
    x = np.asarray(x, dtype=np.float64)
    xi = np.rint(x * 2.0 ** 17).astype(np.int64)
    assert np.array_equal(xi.astype(np.float64), x * 2.0 ** 17), "a value is no multiple of 2^-17"
    assert x.shape[0] * float(np.abs(xi).max()) ** 2 < 2.0 ** 62, "the int64 sum of squares would overflow"
    s1 = np.array([int(v) / 2 ** 17 for v in xi.sum(0)], dtype=np.float64)              # int / int: correctly rounded
    s2 = np.array([int(v) / 2 ** 34 for v in (xi * xi).sum(0)], dtype=np.float64)
    return s1, s2, np.abs(x).sum(0)


def stats_bound(rows, C, abs_sum):
    """|device sum - exact sum| per channel, derived: a thread adds at most k = per_block / rls terms to an fp32 partial that
    starts at 0 -- k roundings, each at most 2^-24 of the running partial's magnitude <= the thread's sum |term| (to first
    order; the (k + 1) of the bound covers the second-order growth for every k used here, k 2^-24 << 1) -- so the fp32 part
    is (k + 1) 2^-24 sum |term| over the channel.  Everything after is fp64: rls partials added in a block, one atomic add
    per block into the destination, and the destination's own start: at most rls + grid + 1 additions per channel, each
    2^-53 of a running magnitude <= sum |term| (+ the start, which is 0 in the real-data family)."""
    rls, grid, per_block, k = stats_geometry(rows, C)
    return ((k + 1) * 2.0 ** -24 + (rls + grid + 1) * 2.0 ** -53) * np.asarray(abs_sum, dtype=np.float64)


def stats_partition(x, variant=None):
    """bn_stats_kernel as written: block b owns block_rows(b); row lane rl adds rows begin + rl, + rls, ... to fp32 partials
    (sum, and the fp32 square); the partials are added in fp64.  x: fp32 values of bf16 [rows, C] -> (sum, sumsq) fp64.
    variant "drop-partial": see block_rows."""
    x = np.asarray(x, dtype=np.float32)
    rows, C = x.shape
    rls, grid, per_block, k = stats_geometry(rows, C)
    s1, s2 = np.zeros(C, dtype=np.float64), np.zeros(C, dtype=np.float64)
    for b in range(grid):
        begin, end = block_rows(rows, rls, grid, b, variant)
        for rl in range(rls):
            a1, a2 = np.zeros(C, dtype=np.float32), np.zeros(C, dtype=np.float32)
            for r in range(begin + rl, end, rls):
                a1 = a1 + x[r]
                a2 = a2 + x[r] * x[r]              # the square of a bf16 value is exact in fp32: fused or not, one rounding
            s1 += a1.astype(np.float64)
            s2 += a2.astype(np.float64)
    return s1, s2


def integer_family(rows, C, seed):
    """bf16 integers |v| <= 16: u in {-2 .. 2} times a per-channel multiplier 1 .. 8 that differs between the 8 channels of
    a vector, the draw itself differing between vectors.  -> int64 [rows, C]"""
    rng = np.random.default_rng(seed)
    u = rng.integers(-2, 3, size=(rows, C), dtype=np.int8).astype(np.int64)
    return u * (1 + (np.arange(C) * 5 + np.arange(C) // 8) % 8)[None, :]


# ---------------------------------------------------------------------------------------------- BatchNorm finalize
def slot_sum(v, variant=None):
    """bn_finalize_kernel's fixed order: lane sl of 16 adds the slot rows sl, sl + 16, ... to a partial that starts at 0.0,
    then the xor tree 8, 4, 2, 1 joins the 16 partials.  v: fp64 [nslots, C] -> fp64 [C].
    variant "first-16": slots >= 16 forgotten."""
    v = np.asarray(v, dtype=np.float64)
    nslots = v.shape[0] if variant != "first-16" else min(v.shape[0], 16)
    lanes = np.zeros((16,) + v.shape[1:], dtype=np.float64)
    for k in range(nslots):
        lanes[k % 16] = lanes[k % 16] + v[k]
    idx = np.arange(16)
    for o in (8, 4, 2, 1):
        lanes = lanes + lanes[idx ^ o]
    return lanes[0]


def _fma64(a, b, c):
    """fma(a, b, c) in fp64 by rational arithmetic, per element"""
    out = np.empty(len(a), dtype=np.float64)
    for i in range(len(a)):
        q = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        out[i] = q.numerator / q.denominator                   # int / int: correctly rounded
    return out


def finalize(sums, sumsqs, rows, gamma, beta, eps, momentum, running_mean=None, running_var=None, variant=None):
    """isic_bn_finalize.  -> dict: mean, rstd, scale (fp32, the one value each), var_forms_agree (bool [C]: rstd is the same
    whether s2 / n - mean * mean is contracted to an fma or not), shift [2, C] candidates, running_mean / running_var
    [3, C] candidates (unfused; the first product fused into the sum; the second).
    variants: "first-16" (slot_sum); "unbiased-norm": n / (n - 1) applied to the variance that normalises;
    "biased-running": not applied to the running estimate."""
    gamma, beta = np.asarray(gamma, dtype=np.float32), np.asarray(beta, dtype=np.float32)
    n = np.float64(rows)
    s1, s2 = slot_sum(sums, variant), slot_sum(sumsqs, variant)
    mean = s1 / n
    q = s2 / n
    var_raw = q - mean * mean
    var_forms = [np.maximum(v, 0.0) for v in (var_raw, _fma64(-mean, mean, q))]
    rstds = []
    for v in var_forms:
        vn = v * n / (n - 1.0) if variant == "unbiased-norm" and rows > 1 else v
        rstds.append((1.0 / np.sqrt(vn + np.float64(F32(eps)))).astype(np.float32))
    var, rstd = var_forms[0], rstds[0]
    meanf = mean.astype(np.float32)
    sc = gamma * rstd
    out = dict(mean=meanf, rstd=rstd, scale=sc, shift=muladd_candidates(-meanf, sc, beta), var_raw=var_raw,
               var_forms_agree=(rstds[0].view(np.uint32) == rstds[1].view(np.uint32)))
    if running_mean is not None:
        unbiased = var * n / (n - 1.0) if rows > 1 and variant != "biased-running" else var
        out["running_var_forms_agree"] = unbiased.astype(np.float32) == (
            var_forms[1] * n / (n - 1.0) if rows > 1 and variant != "biased-running" else var_forms[1]).astype(np.float32)
        m, keep = F32(momentum), F32(1) - F32(momentum)
        for name, old, new in (("running_mean", running_mean, meanf), ("running_var", running_var, unbiased.astype(np.float32))):
            old = np.asarray(old, dtype=np.float32)
            out[name] = np.stack([keep * old + m * new, fma32(keep, old, m * new), fma32(m, new, keep * old)])
    return out


def finalize_case(nslots, C, rows, seed):
    """Hand-made fp64 slot sums [nslots, C] and parameters.  Ordinary channels: slot values with full fp64 mantissas, so the
    order of the additions shows in the last bits.  The special channels (the first ones, as many as C allows) are made of
    slots that are small integers times a power of two -- every partial sum exact, the mean and its square exact, so
    s2 / n - mean^2 is the same fused or not:
      0  constant channel: s2 / n - mean^2 exactly 0
      1  s2 a hair too small: s2 / n - mean^2 slightly negative (clamped to 0)
      2  mean 100 + 1/4, variance 2^-10
      3  all sums 0."""
    rng = np.random.default_rng(seed)
    n = float(rows)
    mean_t = rng.integers(-64, 65, size=C) / 32.0
    var_t = rng.integers(1, 65, size=C) / 16.0
    w = rng.random((nslots, C)) + 0.5
    w /= w.sum(0, keepdims=True)
    s1 = w * (n * mean_t)[None, :]
    w2 = rng.random((nslots, C)) + 0.5
    w2 /= w2.sum(0, keepdims=True)
    s2 = w2 * (n * (var_t + mean_t * mean_t))[None, :]

    def special(c, m, v_num, v_den_log2):
        """channel c: mean m (a multiple of 1/4), variance v_num 2^-v_den_log2; the whole sum sits in slot nslots - 1 and
        the other slots hold +k, -k pairs of integers that cancel exactly in every order used (they are added as exact
        integers far below 2^53)."""
        if c >= C:
            return
        s1[:, c] = 0.0
        s2[:, c] = 0.0
        s1[nslots - 1, c] = n * m
        s2[nslots - 1, c] = n * (m * m) + n * v_num / 2.0 ** v_den_log2
        for k in range(0, nslots - 2, 2):
            s1[k, c], s1[k + 1, c] = float(k + 1), -float(k + 1)
            s2[k, c], s2[k + 1, c] = float(3 * k + 2), -float(3 * k + 2)

    special(0, 1.75, 0.0, 0)
    special(1, 1.75, 0.0, 0)
    if C > 1:
        s2[:nslots - 1, 1] = 0.0                                          # (nothing that could absorb the missing ulp)
        s2[nslots - 1, 1] = np.nextafter(s2[nslots - 1, 1], 0.0)          # one ulp short: the variance comes out < 0
    special(2, 100.25, 1.0, 10)
    special(3, 0.0, 0.0, 0)
    gamma = (rng.integers(4, 13, size=C) / 8.0).astype(np.float32)
    gamma[::5] *= F32(-1)
    beta = (rng.integers(-16, 17, size=C) / 16.0).astype(np.float32)
    rm0 = rng.standard_normal(C).astype(np.float32)
    rv0 = (rng.random(C) + 0.5).astype(np.float32)
    return dict(sum=s1, sumsq=s2, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0)


FINALIZE_CASES = ([(ns, 64, 90) for ns in (1, 15, 16, 17, 32, 300, 1024)] +
                  [(17, c, 90) for c in (1, 15, 16, 17, 2048)] +
                  [(32, 64, 1), (300, 17, 25690112), (1, 1, 1)])


def two_pass(x):
    """fp64 mean and biased variance per channel of fp32 [rows, C] data, two passes with correctly rounded sums"""
    x = np.asarray(x, dtype=np.float64)
    mean = fsum_columns(x) / x.shape[0]
    d = x - mean[None, :]
    return mean, fsum_columns(d * d) / x.shape[0]


def composition_bound(rows, C, abs_sum, sq_sum, mean, var, eps):
    """What the section A bounds allow after finalize, to first order.  d1 = |error of sum|, d2 = |error of sumsq| from
    stats_bound.  mean = s1 / n: |dmean| <= d1 / n (+ one fp64 rounding).  var = s2 / n - mean^2:
    |dvar| <= d2 / n + 2 |mean| d1 / n + u64 (s2 / n + mean^2) 3 (three fp64 roundings of terms of that magnitude).
    rstd = (var + eps)^-1/2: |drstd| / rstd <= |dvar| / (2 (var + eps)), plus 2^-24 for the fp32 rounding of rstd and
    2^-52 for the fp64 sqrt and divide.  -> (dmean, drstd_rel)"""
    d1, d2 = stats_bound(rows, C, abs_sum), stats_bound(rows, C, sq_sum)
    n = float(rows)
    u64 = 2.0 ** -53
    dmean = d1 / n + u64 * np.abs(mean) + 2.0 ** -24 * np.abs(mean)          # (the fp32 rounding of the stored mean)
    dvar = d2 / n + 2 * np.abs(mean) * d1 / n + 3 * u64 * (sq_sum / n + mean * mean)
    return dmean, dvar / (2 * (var + eps)) + 2.0 ** -24 + 2.0 ** -52


# ---------------------------------------------------------------------------------------------- eval affine
def eval_affine(gamma, beta, rm, rv, eps):
    """isic_bn_eval_affine in fp32 with correctly rounded sqrtf and divide -> (scale [C], shift candidates [2, C])"""
    gamma, beta, rm, rv = (np.asarray(v, dtype=np.float32) for v in (gamma, beta, rm, rv))
    sc = gamma / np.sqrt(rv + F32(eps))
    return sc, muladd_candidates(-rm, sc, beta)


def eval_affine_f64(gamma, beta, rm, rv, eps):
    """the fp64 value of the documented form: gamma / sqrt(rv + eps), beta - rm * scale (eps: the fp32 value passed)"""
    gamma, beta, rm, rv = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (gamma, beta, rm, rv))
    sc = gamma / np.sqrt(rv + np.float64(F32(eps)))
    return sc, beta - rm * sc


# ---------------------------------------------------------------------------------------------- BatchNorm apply
def unpack_mask_bytes(mask, C):
    """uint8 [rows * C / 8] -> bool [rows, C]"""
    return np.unpackbits(np.asarray(mask, dtype=np.uint8), bitorder="little").reshape(-1, C).astype(bool)


def pack_mask_bits(bits):
    """bool [rows, C] -> uint8 [rows * C / 8], through conv_bf16_ref.pack_mask (bit j of a byte = channel 8 byte + j)"""
    return pack_mask(torch.from_numpy(np.ascontiguousarray(bits))).numpy()


def bn_apply(x, scale, shift, relu, residual=None, res_scale=None, res_shift=None, variant=None):
    """y = relu?(x * scale + shift [+ residual]) with residual = bf16(residual_raw * res_scale + res_shift) when res_scale
    is given.  x, residual: fp32 values of bf16 [rows, C].  -> (y bits candidates [K, rows, C] uint16, positive candidates
    [K, rows, C] bool: what the mask bit says, v > 0 on the fp32 value before the rounding).  K = 2, or 4 with res_scale
    (every combination of the two multiply-adds fused or not).
    A ReLU zero is +0 (the device's max returns +0 for max(-0, +0)); without the ReLU the sign of a zero is IEEE's.
    variant "mask-rotated": the mask bit taken from the next channel of the 8-vector."""
    x = np.asarray(x, dtype=np.float32)
    vs = list(muladd_candidates(x, np.asarray(scale, dtype=np.float32)[None, :], np.asarray(shift, dtype=np.float32)[None, :]))
    if residual is not None:
        residual = np.asarray(residual, dtype=np.float32)
        if res_scale is not None:
            inner = muladd_candidates(residual, np.asarray(res_scale, dtype=np.float32)[None, :],
                                      np.asarray(res_shift, dtype=np.float32)[None, :])
            rs = [bf16_value(bf16_bits(r)).reshape(x.shape) for r in inner]
        else:
            rs = [residual]
        vs = [v + r for v in vs for r in rs]
    if relu:
        vs = [np.maximum(v, F32(0)) + F32(0) for v in vs]
    pos = [v > 0 for v in vs]
    if variant == "mask-rotated":
        rows, C = x.shape
        pos = [np.roll(p.reshape(rows, C // 8, 8), -1, axis=2).reshape(rows, C) for p in pos]
    return np.stack([bf16_bits(v).reshape(x.shape) for v in vs]), np.stack(pos)


APPLY_NVEC = (1, 255, 256, 257, 511, 512, 513, 1025)
APPLY_C = (8, 64, 256, 2048)


def apply_shapes():
    """(rows, C) pairs: for each C every vector count of APPLY_NVEC that rows * C / 8 can hit exactly, and otherwise the
    nearest count above it (a ragged tail inside the same 256-vector row of the block)."""
    out = []
    for C in APPLY_C:
        cgs = C // 8
        for nv in APPLY_NVEC:
            rows = max(1, -(-nv // cgs))
            if (rows, C) not in out:
                out.append((rows, C))
    return out


def apply_case(rows, C, seed, exact=True):
    """Operands of one apply case.  exact: x and the residual from a handful of bf16 values (with -0.0), scale / shift /
    res_scale / res_shift on grids of 1/8 and 1/16 -- at most 16 significant bits, so every product with a bf16 value is exact
    in fp32 and so is the sum: the fused and the unfused multiply-add agree on every element.  Distinct constants per
    channel, negative scales, one channel all zero after the ReLU, one whose scale is 0 with shift -0.0.
    not exact: normal data, full-mantissa constants."""
    rng = np.random.default_rng(seed)
    if exact:
        vals = np.array([-2.0, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 2.0, 3.0], dtype=np.float32)
        x = vals[rng.integers(0, len(vals), size=(rows, C))]
        res = vals[rng.integers(0, len(vals), size=(rows, C))]
        c = np.arange(C)
        scale = ((4 + (c * 7 + c // 8) % 9) / 8.0).astype(np.float32)
        scale[c % 5 == 0] *= F32(-1)
        shift = (((c * 11 + c // 8) % 33 - 16) / 16.0).astype(np.float32)
        rsc = ((4 + (c * 3 + c // 8) % 9) / 8.0).astype(np.float32)
        rsc[c % 7 == 0] *= F32(-1)
        rsh = (((c * 13 + c // 8) % 33 - 16) / 16.0).astype(np.float32)
        shift[3 % C], rsh[3 % C] = F32(-100.0), F32(-100.0)                  # all zero after the ReLU
        scale[7 % C], shift[7 % C] = F32(0.0), F32(-0.0)
    else:
        x = bf16_value(bf16_bits(rng.standard_normal((rows, C)).astype(np.float32))).reshape(rows, C)
        res = bf16_value(bf16_bits(rng.standard_normal((rows, C)).astype(np.float32))).reshape(rows, C)
        scale = (rng.standard_normal(C) * 0.7 + 1.0).astype(np.float32)
        scale[::5] *= F32(-1)
        shift = rng.standard_normal(C).astype(np.float32) * F32(0.5)
        rsc = (rng.standard_normal(C) * 0.7 + 1.0).astype(np.float32)
        rsh = rng.standard_normal(C).astype(np.float32) * F32(0.5)
    return dict(x=x, res=res, scale=scale, shift=shift, rsc=rsc, rsh=rsh)


# ---------------------------------------------------------------------------------------------- max-pool
def pool_out(H, W):
    return (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1


def pool_restatement(x, scale, shift, Ho, Wo):
    """relu(x * scale + shift) in fp32 on the fused form, rounded to bf16, 3x3/2 windows scanned row-major with the first
    maximum winning.  (+ 0.0 makes a -0.0 of the ReLU +0.0, as the device's max does.)"""
    N, H, W, C = x.shape
    xf = x.float()
    f = torch.relu(torch.addcmul(shift.view(1, 1, 1, C), xf, scale.view(1, 1, 1, C))).to(BF).float() + 0.0
    fp = F.pad(f, (0, 0, 1, 2, 1, 2), value=-1.0)                # outside the image: below every value after the ReLU
    xp = F.pad(xf, (0, 0, 1, 2, 1, 2), value=float("nan"))
    taps_f = torch.stack([fp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :] for kh in range(3) for kw in range(3)])
    taps_x = torch.stack([xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :] for kh in range(3) for kw in range(3)])
    am = taps_f.argmax(dim=0, keepdim=True)                      # the first of several maxima
    return taps_f.gather(0, am)[0], am[0].to(torch.uint8), taps_x.gather(0, am)[0]


def maxpool_fwd(f, variant=None, raw=None):
    """MaxPool2d(3, 2, 1) of fp32 [N, H, W, C] (finite): the window's taps scanned row-major, the FIRST maximum wins, a tap
    outside the image is below every value.  -> (y fp32 with the winning tap's own bit pattern (the sign of a zero is the
    tap's), code uint8 = kh * 3 + kw[, raw at the argmax]).
    variants: "last-wins": the last maximum; "pad-zero": a tap outside the image counts as 0."""
    f = np.asarray(f, dtype=np.float32)
    N, H, W, C = f.shape
    Ho, Wo = pool_out(H, W)
    pad = F32(0) if variant == "pad-zero" else F32(-np.inf)
    fp = np.full((N, H + 3, W + 3, C), pad, dtype=np.float32)
    fp[:, 1:H + 1, 1:W + 1] = f
    taps = np.stack([fp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh in range(3) for kw in range(3)])
    if variant == "last-wins":
        code = 8 - np.argmax(taps[::-1], axis=0)
    else:
        code = np.argmax(taps, axis=0)                           # numpy: the first of several maxima; -0.0 == +0.0
    y = np.take_along_axis(taps, code[None], axis=0)[0]
    out = (y, code.astype(np.uint8))
    if raw is not None:
        rp = np.full((N, H + 3, W + 3, C), np.nan, dtype=np.float32)
        rp[:, 1:H + 1, 1:W + 1] = raw
        rt = np.stack([rp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2] for kh in range(3) for kw in range(3)])
        out += (np.take_along_axis(rt, code[None], axis=0)[0],)
    return out


def maxpool_bwd(code, dy, H, W):
    """dx [N, H, W, C] bf16 bits: each input pixel gathers the <= 2 x 2 windows that cover it in the kernel's order (ho
    ascending, then wo), adding in fp32 the gradient of every window whose code names the pixel; one rounding to bf16.
    code: uint8 [N, Ho, Wo, C]; dy: fp32 values of bf16."""
    code, dy = np.asarray(code), np.asarray(dy, dtype=np.float32)
    N, Ho, Wo, C = dy.shape
    acc = np.zeros((N, H, W, C), dtype=np.float32)
    hi, wi = np.arange(H), np.arange(W)
    for a in (0, 1):
        ho = (hi >> 1) + a
        kh = hi - (ho * 2 - 1)
        okh = (ho <= (hi + 1) >> 1) & (ho < Ho) & (kh >= 0) & (kh <= 2)
        for b in (0, 1):
            wo = (wi >> 1) + b
            kw = wi - (wo * 2 - 1)
            okw = (wo <= (wi + 1) >> 1) & (wo < Wo) & (kw >= 0) & (kw <= 2)
            hc, wc = np.minimum(ho, Ho - 1), np.minimum(wo, Wo - 1)
            want = (kh[:, None] * 3 + kw[None, :])[None, :, :, None]
            ok = (okh[:, None] & okw[None, :])[None, :, :, None]
            g = dy[:, hc][:, :, wc]
            hit = ok & (code[:, hc][:, :, wc] == want)
            acc = np.where(hit, acc + g, acc)
    return bf16_bits(acc).reshape(N, H, W, C)


def code_inside(codes, H, W):
    """bool [Ho, Wo]: the tap `codes` [Ho, Wo] names lies inside the H x W image"""
    Ho, Wo = pool_out(H, W)
    ho, wo = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    hi, wi = ho * 2 - 1 + codes // 3, wo * 2 - 1 + codes % 3
    return (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)


def handmade_codes(kind, H, W):
    """A code plane [Ho, Wo] for the backward: "all-k" or "checker" (0 and 8 alternating); a window whose tap would fall
    outside the image gets the centre tap 4 instead, which always exists."""
    Ho, Wo = pool_out(H, W)
    if kind == "checker":
        ho, wo = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
        c = np.where((ho + wo) % 2 == 0, 0, 8)
    else:
        c = np.full((Ho, Wo), int(kind.split("-")[1]))
    return np.where(code_inside(c, H, W), c, 4).astype(np.uint8)


POOL_HW = ((1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (5, 4), (7, 9), (13, 16), (16, 13))
HANDMADE = ("all-4", "all-0", "all-8", "all-2", "all-6", "checker")


# ---------------------------------------------------------------------------------------------- average pool
def avgpool_fwd(x, variant=None):
    """AdaptiveAvgPool2d(1) of fp32 values of bf16 [N, HW, C] -> fp32 [N, C] in the kernel's order: wave w of 4 adds the
    pixels w, w + 4, ... in fp32, then ((p0 + p1) + (p2 + p3)) / (float)HW, the division correctly rounded."""
    x = np.asarray(x, dtype=np.float32)
    N, HW, C = x.shape
    part = np.zeros((4, N, C), dtype=np.float32)
    for p in range(HW):
        part[p % 4] = part[p % 4] + x[:, p]
    return ((part[0] + part[1]) + (part[2] + part[3])) / F32(HW)


def avgpool_bwd(dy, HW, variant=None):
    """dx[n, p, c] = bf16(dy[n, c] * (1.f / HW)) -> bits [N, HW, C].  variant "divide": bf16(dy / HW)."""
    dy = np.asarray(dy, dtype=np.float32)
    v = dy / F32(HW) if variant == "divide" else dy * (F32(1) / F32(HW))
    return np.repeat(bf16_bits(v).reshape(dy.shape[0], 1, dy.shape[1]), HW, axis=1)


AVG_HW = (1, 3, 4, 5, 49, 196)
AVG_C = (1, 63, 64, 65, 512)


# ---------------------------------------------------------------------------------------------- layout
def nchw_to_nhwc4(x, is_bf16):
    """x [N, C, H, W]: fp32 values, or uint16 bf16 bit patterns -> uint16 [N, H, W, 4]; fp32 is rounded to nearest even,
    channels C .. 3 are +0."""
    N, C, H, W = x.shape
    bits = np.asarray(x, dtype=np.uint16) if is_bf16 else bf16_bits(x).reshape(x.shape)
    out = np.zeros((N, H, W, 4), dtype=np.uint16)
    out[..., :C] = bits.transpose(0, 2, 3, 1)
    return out


def layout_input(N, C, HW, seed):
    """fp32 [N, C, 1, HW]: normal data with, sprinkled in, values exactly half way between two bf16 (low half-word 0x8000,
    both parities of the kept bit), just below and above such a tie, and +-0."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, 1, HW)).astype(np.float32)
    u = x.view(np.uint32).copy()
    kind = rng.integers(0, 8, size=u.shape)
    u = np.where(kind == 0, (u & np.uint32(0xFFFF0000)) | np.uint32(0x8000), u)
    u = np.where(kind == 1, (u & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF), u)
    u = np.where(kind == 2, (u & np.uint32(0xFFFF0000)) | np.uint32(0x8001), u)
    u = np.where(kind == 3, np.where(u & np.uint32(0x10000), np.uint32(0x80000000), np.uint32(0)), u)
    return u.astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------------------------------------- shared inputs
STATS_C = (8, 16, 64, 128, 512, 2048)
STATS_CAP_CASES = ((16385, 2048), (524289, 64))                  # past the 2048-block cap: k = 9 terms per thread


def stats_shapes():
    """(rows, C): with rls = 2048 / C rows in {1, rls - 1, rls, 8 rls + 1, 3 * 8 rls + 5} (rows >= 1, no duplicates)"""
    out = []
    for C in STATS_C:
        rls = 2048 // C
        for rows in (1, rls - 1, rls, 8 * rls + 1, 3 * 8 * rls + 5):
            if rows >= 1 and (rows, C) not in out:
                out.append((rows, C))
    return out


def real_family(rows, C, seed, mean=0.0):
    """fp32 values of bf16 [rows, C]: normal data, a distinct spread per channel, around `mean`; magnitudes below 2^-10 are
    raised to it"""
    rng = np.random.default_rng(seed)
    spread = (0.5 + (np.arange(C) % 8) / 4.0).astype(np.float32)
    x = rng.standard_normal((rows, C), dtype=np.float32) * spread[None, :] + F32(mean)
    x = bf16_value(bf16_bits(x)).reshape(rows, C)
    return np.where(np.abs(x) < F32(2.0 ** -10), np.copysign(F32(2.0 ** -10), x), x)   # multiples of 2^-17: see stats_exact


POOL_VALUES = np.array([-2.0, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 2.0], dtype=np.float32)


def pool_input(N, H, W, C, seed):
    """a handful of bf16 values, negative ones and both zeros among them: ties are the rule"""
    rng = np.random.default_rng(seed)
    return POOL_VALUES[rng.integers(0, len(POOL_VALUES), size=(N, H, W, C))]


def pool_affine(C, seed):
    """scale on a grid of 1/8, shift of 1/16 (x * scale + shift exact in fp32 for pool_input: fused and unfused agree);
    negative scales; a channel where every window ties at 0.25, one at zero formed as +0.0 and -0.0, one all zero after the
    ReLU."""
    rng = np.random.default_rng(seed)
    scale = (rng.integers(4, 13, size=C) / 8.0).astype(np.float32)
    scale[np.arange(C) % 5 == 0] *= F32(-1)
    shift = (rng.integers(-16, 17, size=C) / 16.0).astype(np.float32)
    scale[3 % C], shift[3 % C] = F32(0.0), F32(0.25)
    scale[7 % C], shift[7 % C] = F32(0.0), F32(-0.0)
    shift[5 % C] = F32(-100.0)
    return scale, shift


def avg_input(N, HW, C, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, HW, C), dtype=np.float32) * (1.0 + (np.arange(C) % 8)[None, None, :]).astype(np.float32)
    return bf16_value(bf16_bits(x)).reshape(N, HW, C)


def avg_bwd_input(N, C, HW, seed):
    """fp32 dy [N, C]: normal data, and planted at the front of every row up to 16 values whose quotient by HW lies next to
    a bf16 rounding tie, found by search, where bf16(dy * (1.f / HW)) and bf16(dy / HW) part (none exist when 1 / HW is a
    power of two).  -> (dy, number planted per row)"""
    rng = np.random.default_rng(seed)
    dy = rng.standard_normal((N, C)).astype(np.float32)
    mid = (rng.standard_normal(4096).astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x8000)
    near = (mid.view(np.float32) * F32(HW)).view(np.uint32)
    cand = np.concatenate([near + np.uint32(d) for d in range(0, 3)] + [near - np.uint32(d) for d in range(1, 3)]).view(np.float32)
    cand = cand[bf16_bits(cand * (F32(1) / F32(HW))) != bf16_bits(cand / F32(HW))]
    k = min(16, C, len(cand))
    dy[:, :k] = cand[:k][None, :]
    return dy, k
