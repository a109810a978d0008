"""numpy emulation of csrc/bn_bwd_math.inc, the BatchNorm(+ReLU) backward arithmetic every kernel takes from there, step
by step: each unfused step in np.float32 arithmetic (correctly rounded, like the device's), each fmaf(a, b, c) as
np.float32(np.float64(a) * np.float64(b) + np.float64(c)).  The product of two fp32 values is exact in fp64, so that
expression is the true fused multiply-add whenever the fp64 SUM is exact; `fma` checks that per element with
fractions.Fraction and returns the mask, and every function below hands the conjunction of its masks on: an element whose
mask is False is "unchecked" (the emulation may be one rounding off there), everything else is the device's value bit for
bit.  The inputs of `make_case` are dyadic and coarse enough that nothing is unchecked (tests/test_bn_bwd_ref_cpu.py).

Used by tests/test_bn_bwd_ref_cpu.py (the reference alone) and tests/test_bn_bwd_math_gpu.py (the device against it)."""
from fractions import Fraction

import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------------------- number formats
def bf16_bits(f):
    """fp32 -> bf16 bit patterns, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_value(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _sum_is_exact(p, c, s):
    """Fraction(p) + Fraction(c) == Fraction(s), element by element (each distinct triple once)."""
    trip = np.stack([p.ravel(), c.ravel(), s.ravel()], axis=1)
    uniq, inv = np.unique(trip, axis=0, return_inverse=True)
    ok = np.array([Fraction(a) + Fraction(b) == Fraction(r) for a, b, r in uniq.tolist()], dtype=bool)
    return ok[inv.ravel()].reshape(p.shape)


def fma(a, b, c):
    """-> (fmaf(a, b, c) as fp32, mask of the elements where that is certain)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b
    s = p + c
    return s.astype(np.float32), _sum_is_exact(p, c, s)


# ---------------------------------------------------------------------------------------------- bn_bwd_math.inc
def gate(mode, g, x=None, y=None, scale=None, shift=None, bits=None):
    """isic_bn_bwd::gate<mode>.  g, x, y: [rows, C] fp32; bits: [rows, C] bool (bit j of byte i = element 8 i + j).
    -> (dz, checked)"""
    g = np.asarray(g, dtype=np.float32)
    sure = np.ones(g.shape, dtype=bool)
    if mode == 0:
        return g.copy(), sure
    if mode == 3:
        return np.where(bits, g, F32(0)), sure
    if mode == 2:
        v, sure = fma(x, scale, shift)
    else:
        v = np.asarray(y, dtype=np.float32)
    return np.where(v > 0, g, F32(0)), sure            # !(v > 0) ? 0 : g


def unpack_mask(mask_bytes, rows, C):
    return np.unpackbits(np.asarray(mask_bytes, dtype=np.uint8), bitorder="little").reshape(rows, C).astype(bool)


def inv_count(rows):
    return F32(1) / F32(rows)


def constants(mean, rstd, gamma, sum_dzx, sum_dz, rows):
    """isic_bn_bwd::constants per channel; sum_*: the fp64 sums.  -> (kA, kB, kD, checked[C])"""
    mean, rstd, gamma = (np.asarray(v, dtype=np.float32) for v in (mean, rstd, gamma))
    inv = inv_count(rows)
    k1 = gamma * rstd
    k2 = np.asarray(sum_dz, dtype=np.float64).astype(np.float32) * inv
    k3 = np.asarray(sum_dzx, dtype=np.float64).astype(np.float32) * inv
    kB = (-k1 * k3) * rstd
    t, sure = fma(k3 * rstd, mean, -k2)
    return k1, kB, k1 * t, sure


def dx_fused(kA, kB, kD, x, dz):
    """isic_bn_bwd::dx -> (fp32 value, checked)"""
    t, s1 = fma(kB, x, kD)
    o, s2 = fma(kA, dz, t)
    return o, s1 & s2


def dx_unfused(kA, kB, kD, x, dz):
    """isic_bn_bwd::dx_unfused: fp32 operations only, nothing to check."""
    kA, kB, kD, x, dz = (np.asarray(v, dtype=np.float32) for v in (kA, kB, kD, x, dz))
    t = kD + kB * x
    return t + kA * dz


def fold(start_f32, total_f64):
    return np.asarray(start_f32, dtype=np.float32) + np.asarray(total_f64, dtype=np.float64).astype(np.float32)


def apply_pass(dz, x, mean, rstd, gamma, sum_dzx, sum_dz, rows, dz_checked=None, unfused=False):
    """One norm of an apply kernel.  -> (bf16 bit patterns of dx [rows, C], checked [rows, C])"""
    kA, kB, kD, csure = constants(mean, rstd, gamma, sum_dzx, sum_dz, rows)
    if unfused:
        o, sure = dx_unfused(kA, kB, kD, x, dz), np.ones(np.shape(dz), dtype=bool)
    else:
        o, sure = dx_fused(kA, kB, kD, x, dz)
    sure = sure & csure[None, :]
    if dz_checked is not None:
        sure = sure & dz_checked
    return bf16_bits(o), sure


# ---------------------------------------------------------------------------------------------- the reduce passes
def _grid(n, block, cap):
    return int(min(max((n + block - 1) // block, 1), cap))


class Sums:
    """Per-thread fp32 partials of a reduce kernel, then their fp64 total per channel."""

    def __init__(self, C, nthreads_rows):
        self.acc = np.zeros((nthreads_rows, C), dtype=np.float32)
        self.sure = np.ones((nthreads_rows, C), dtype=bool)

    def total(self):
        """-> (fp64 total [C], checked [C]): checked where EVERY order of fp64 additions gives that total -- the partials
        of a channel are multiples of one power of two q with sum |partial| / q < 2^53 (the device adds the row lanes of a
        block in order and the blocks with atomics, in any order)."""
        C = self.acc.shape[1]
        out, ok = np.zeros(C, dtype=np.float64), np.zeros(C, dtype=bool)
        for c in range(C):
            fr = [Fraction(v) for v in self.acc[:, c].tolist()]
            tot = sum(fr, Fraction(0))
            den = max(f.denominator for f in fr)
            out[c] = float(tot)
            ok[c] = Fraction(out[c]) == tot and sum(abs(f) for f in fr) * den < 2 ** 53 and bool(self.sure[:, c].all())
        return out, ok

    def step(self, idx, dz, xhat, valid):
        new, s = fma(dz, xhat, self.acc[idx])
        self.acc[idx] = np.where(valid, new, self.acc[idx])
        self.sure[idx] &= s | ~valid


def reduce_flat(dz, xs, means, rstds, dz_checked=None):
    """bn_bwd_reduce_kernel's partition: block b sums the contiguous rows [b per_block, (b + 1) per_block), row lane rl of
    rls = 256 / (C / 8) takes every rls-th of them, in order.  xs / means / rstds: one entry per norm (the pair has two).
    -> ([(sum dz * xhat total, checked)] per norm, (sum dz total, checked))"""
    rows, C = dz.shape
    rls = 256 // (C // 8)
    grid = _grid(rows, rls * 8, 2048)
    per_block = ((rows + grid - 1) // grid + rls - 1) // rls * rls
    lanes = grid * rls
    start = (np.arange(grid)[:, None] * per_block + np.arange(rls)[None, :]).ravel()
    end = np.minimum(rows, (np.arange(grid) + 1) * per_block).repeat(rls)
    dzx = [Sums(C, lanes) for _ in xs]
    sdz = np.zeros((lanes, C), dtype=np.float32)
    for k in range(per_block // rls):
        r = start + k * rls
        valid = (r < end)[:, None]
        rc = np.minimum(r, rows - 1)
        d = np.where(valid, dz[rc], F32(0))
        for S, x, mu, rs in zip(dzx, xs, means, rstds):
            S.step(slice(None), d, (x[rc] - mu[None, :]) * rs[None, :], valid)
            if dz_checked is not None:
                S.sure &= dz_checked[rc] | ~valid
        sdz = sdz + d                                                  # acc_dz += dz: an fp32 addition
    z = Sums(C, lanes)
    z.acc = sdz
    if dz_checked is not None:
        z.sure[:] = dz_checked.all(axis=0)[None, :]
    return [S.total() for S in dzx], z.total()


def pool_backward(argmax, gp, H, W):
    """The gradient of the 3x3 / stride 2 / pad 1 max-pool's input from the pooled gradient gp [N, Ho, Wo, C] (fp32 values
    of bf16) and the argmax codes kh * 3 + kw, rounded to bf16 as the kernels round it.  The sums are exact for the coarse
    gp of make_case, so their order does not matter."""
    N, Ho, Wo, C = gp.shape
    g = np.zeros((N, H, W, C), dtype=np.float64)
    n, ho, wo, c = np.meshgrid(np.arange(N), np.arange(Ho), np.arange(Wo), np.arange(C), indexing="ij")
    hi, wi = ho * 2 - 1 + argmax // 3, wo * 2 - 1 + argmax % 3
    ok = (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
    np.add.at(g, (n[ok], hi[ok], wi[ok], c[ok]), gp[ok].astype(np.float64))
    g32 = g.astype(np.float32)
    assert (g32.astype(np.float64) == g).all() and (bf16_value(bf16_bits(g32)) == g32).all(), "pooled gradient not exact"
    return g32


def reduce_pooled(dz, x, mean, rstd, N, H, W):
    """stem_bn_bwd_reduce_kernel's partition: row lane rl of block b takes the 2x2 pixel blocks q = b rls + rl,
    + grid rls, ...; q -> (n, a, b) row-major over [N, ceil(H/2), ceil(W/2)]; the four pixels (2a + p/2, 2b + p%2) in
    order p = 0..3, a pixel outside the image contributing dz = 0 with the clamped pixel's x.  dz, x: [N, H, W, C]."""
    C = dz.shape[-1]
    rls = 256 // (C // 8)
    Hb, Wb = (H + 1) // 2, (W + 1) // 2
    nblk = N * Hb * Wb
    grid = _grid(nblk, rls * 2, 2048)
    lanes = grid * rls
    S = Sums(C, lanes)
    sdz = np.zeros((lanes, C), dtype=np.float32)
    q = np.arange(lanes)
    while (q < nblk).any():
        live = q < nblk
        qc = np.minimum(q, nblk - 1)
        b, a, n = qc % Wb, (qc // Wb) % Hb, qc // (Wb * Hb)
        for p in range(4):
            hi, wi = 2 * a + (p >> 1), 2 * b + (p & 1)
            valid = (live & (hi < H) & (wi < W))[:, None]
            hc, wc = np.minimum(hi, H - 1), np.minimum(wi, W - 1)
            d = np.where(valid, dz[n, hc, wc], F32(0))
            S.step(slice(None), d, (x[n, hc, wc] - mean[None, :]) * rstd[None, :], live[:, None])
            sdz = sdz + d
        q = q + lanes
    z = Sums(C, lanes)
    z.acc = sdz
    return S.total(), z.total()


# ---------------------------------------------------------------------------------------------- inputs
def make_case(rows, C, seed):
    """Seeded operands of one [rows, C] case, all dyadic: activations and gradients k / 4 with |k| <= 8 (bf16 holds them),
    per-channel parameters on coarse grids, the reduced sums handed to the apply pass rows * m / 2^23 with 24-bit m (so kB
    and kD carry full fp32 mantissas and a rounded product is not an exact one).
      * half of the gradients are zero, and x sits exactly at its channel mean wherever (row + channel) is even; the means
        are k / 8 with a k that is no power of two, so kB * mean needs more than 24 bits;
      * sum dz is zero except on every fourth channel: where it is, dx at x = mean, dz = 0 is nothing but the roundings of
        kB x + kD, which is where the fused and the unfused form part visibly (everywhere else they differ in the last
        fp32 bit, which the bf16 output rarely shows);
      * gamma is negative on every fifth channel, so scale is and the gate recomputed from x flips there;
      * y, the stored output of the gate's mode 1, has +0, -0, positive and negative entries."""
    rng = np.random.default_rng(seed)
    q = lambda lo, hi, size: rng.integers(lo, hi + 1, size=size).astype(np.float32) / F32(4)
    r, c = np.meshgrid(np.arange(rows), np.arange(C), indexing="ij")
    odd = np.array([k for k in range(-11, 12) if abs(k) in (3, 5, 6, 7, 9, 10, 11)], dtype=np.float32) / F32(8)
    mean, mean2 = rng.choice(odd, size=C), rng.choice(odd, size=C)
    rstd, rstd2 = (rng.choice(np.array([0.5, 0.75, 1.0, 1.5, 2.0], dtype=np.float32), size=C) for _ in range(2))
    gamma, gamma2 = (rng.choice(np.array([0.5, 0.75, 1.0, 1.25, 1.5], dtype=np.float32), size=C) for _ in range(2))
    gamma[::5] *= F32(-1)
    beta = q(-4, 4, C)
    at_mean = (r + c) % 2 == 0
    x = np.where(at_mean, mean[None, :], q(-8, 8, (rows, C)))
    x2 = np.where(at_mean, mean2[None, :], q(-8, 8, (rows, C)))
    dy = np.where(rng.random((rows, C)) < 0.5, F32(0), q(-8, 8, (rows, C))).astype(np.float32)
    y = q(-2, 8, (rows, C))
    y[rng.random((rows, C)) < 0.2] = F32(-0.0)
    wide = lambda: rows * rng.integers(-2 ** 23, 2 ** 23 + 1, size=C).astype(np.float64) / 2.0 ** 23
    sum_dz = wide()
    sum_dz[np.arange(C) % 4 != 3] = 0.0
    scale = gamma * rstd
    return dict(rows=rows, C=C, x=x, x2=x2, dy=dy, y=y, mean=mean, rstd=rstd, gamma=gamma, mean2=mean2, rstd2=rstd2,
                gamma2=gamma2, scale=scale, shift=beta - mean * scale, sum_dzx=wide(), sum_dzx2=wide(), sum_dz=sum_dz,
                mask=rng.integers(0, 256, size=rows * C // 8).astype(np.uint8),
                start={k: q(-8, 8, C) for k in ("dgamma", "dbeta", "dgamma2", "dbeta2")})


def case_gate(case, mode):
    """dz of `case` under gate mode 0..3 -> (dz, checked)"""
    return gate(mode, case["dy"], x=case["x"], y=case["y"], scale=case["scale"], shift=case["shift"],
                bits=unpack_mask(case["mask"], case["rows"], case["C"]))


FLAT_SHAPES = [(1, 1, 1, 64), (3, 7, 7, 128), (3, 7, 7, 512)]      # one row; a ragged last apply block; 64 channel groups
POOLED_SHAPES = [(2, 9, 13, 64), (1, 2, 2, 64)]                   # odd sizes: windows clipped below and on the right
WGRAD_SHAPES = [(1, 4, 32), (3, 9, 13)]                           # N, H, W of the 64-channel fused weight gradient


def shape_case(shape):
    """The case of an (N, H, W, C) or (N, H, W) [C = 64] shape; the seed is a function of the shape."""
    N, H, W = shape[:3]
    C = shape[3] if len(shape) == 4 else 64
    return make_case(N * H * W, C, 1000 + 7 * N * H * W + C)


def pooled_case(shape, seed=None):
    """shape_case for the kernels fed by the pooled gradient: `gp` [N, Ho, Wo, C] (k / 4, half of them zero) and argmax
    codes 0..8 drawn at random (a code that points outside the image routes its gradient nowhere), and dy = their max-pool
    backward."""
    N, H, W, C = shape
    cs = shape_case(shape)
    rng = np.random.default_rng(cs["rows"] + 5 if seed is None else seed)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gp = rng.integers(-8, 9, size=(N, Ho, Wo, C)).astype(np.float32) / F32(4)
    gp[rng.random(gp.shape) < 0.5] = F32(0)
    argmax = rng.integers(0, 9, size=gp.shape).astype(np.uint8)
    cs.update(gp=gp, argmax=argmax, Ho=Ho, Wo=Wo, dy=pool_backward(argmax.astype(np.int64), gp, H, W).reshape(-1, C))
    return cs
