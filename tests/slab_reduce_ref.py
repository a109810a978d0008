"""numpy restatement, in float32 with one IEEE add per device add, of the fixed orders in which the split reductions add
their slabs (csrc/slab_sum.inc).  Written from the reducer kernels as they stood before they shared one file:

  form 0  gemm_split_reduce_kernel, colsum_reduce_kernel, wgrad_reduce_kernel<16>, stem_wgrad_reduce_kernel,
          ln_bwd_reduce_kernel: lane g of 16 adds slabs g, g + 16, ... from 0; xor tree 8, 4, 2, 1
  form 1  wgrad_reduce_kernel<4>: the same with 4 lanes; xor tree 2, 1
  form 2  gemm_split_reduce4_kernel, wgrad_c128b_reduce_kernel, wgrad_s2_reduce_kernel: on f32x4, group g of 16 adds slabs
          g, g + 16, ... from 0; the 16 group sums are added in group order, starting from group 0's
  form 3  wgrad_c64_reduce_kernel: two accumulators (slabs b and b + 16, stride 32; a single leftover slab goes to the
          first), joined s0 + s1; then as form 2
  form 4  ct_slab_reduce_kernel: scalars, four accumulators (slabs z, z + 16, z + 32, z + 48, stride 64; leftover slabs go
          to accumulators 0, 1, 2 in turn), joined (a0 + a1) + (a2 + a3); the 16 group sums are added in group order onto 0

An f32x4 add is four independent adds, so forms 2 and 3 are stated per element.  `sequential` is the plain index-order
walk (slab_reduce_kernel of vit_train.hip): not one of the five forms, the tests use it to show that the order matters.
The epilogue of the test entry is `out = beta * out + s` with beta 0 or 1: s itself, or one add."""
import functools

import numpy as np

F = np.float32
FORMS = (0, 1, 2, 3, 4)
VECTOR_FORMS = (2, 3)                               # n % 4 == 0, 16-byte aligned
SLABS = (1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 100, 257)
N_VECTOR = (148, 4)
N_SCALAR = (148, 4, 37, 1)


def n_values(form):
    return N_VECTOR if form in VECTOR_FORMS else N_SCALAR


def _xor(partial, G):
    S, n = partial.shape
    lanes = np.zeros((G, n), F)
    for z in range(S):                              # lane z % G meets its slabs in ascending order
        lanes[z % G] = lanes[z % G] + partial[z]
    idx = np.arange(G)
    o = G // 2
    while o > 0:
        lanes = lanes + lanes[idx ^ o]
        o //= 2
    return lanes[0]


def _lds16(partial, acc, from_zero=False):
    S, n = partial.shape
    groups = []
    for g in range(16):
        a = np.zeros((acc, n), F)
        z = g
        while z + 16 * (acc - 1) < S:
            for k in range(acc):
                a[k] = a[k] + partial[z + 16 * k]
            z += 16 * acc
        k = 0
        while z < S:
            a[k] = a[k] + partial[z]
            z += 16
            k += 1
        groups.append(a[0] if acc == 1 else a[0] + a[1] if acc == 2 else (a[0] + a[1]) + (a[2] + a[3]))
    t = np.zeros(n, F) + groups[0] if from_zero else groups[0]
    for g in range(1, 16):
        t = t + groups[g]
    return t


def slab_sum(form, partial, from_zero=None):
    """the sum over axis 0 of a float32 [slabs][n] stack in the order of `form`.  from_zero: whether the join through LDS
    starts from 0 (form 4's kernel) or from group 0's sum (forms 2 and 3); None = as the form's kernel did"""
    partial = np.asarray(partial)
    assert partial.dtype == F and partial.ndim == 2
    if form == 0:
        return _xor(partial, 16)
    if form == 1:
        return _xor(partial, 4)
    acc = {2: 1, 3: 2, 4: 4}[form]
    return _lds16(partial, acc, (form == 4) if from_zero is None else from_zero)


def sequential(partial):
    s = np.zeros(partial.shape[1], F)
    for z in range(partial.shape[0]):
        s = s + partial[z]
    return s


def epilogue(s, prior, beta):
    assert beta in (0.0, 1.0)
    return (prior + s).astype(F) if beta == 1.0 else s


@functools.lru_cache(maxsize=None)
def case(slabs, n):
    """(partial [slabs][n], prior out [n]): standard_normal x 2^randint(-6, 7), fixed seed per shape.  Read-only."""
    rng = np.random.default_rng([20241, slabs, n])

    def draw(shape):
        return (rng.standard_normal(shape) * np.exp2(rng.integers(-6, 7, shape))).astype(F)

    partial, prior = draw((slabs, n)), draw((n,))
    partial.setflags(write=False)
    prior.setflags(write=False)
    return partial, prior


@functools.lru_cache(maxsize=None)
def expected(form, slabs, n):
    s = slab_sum(form, case(slabs, n)[0])
    s.setflags(write=False)
    return s


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)
