"""The BatchNorm forward, pooling and layout kernels of csrc/encoder_ops.hip over their dispatch domains on the MI355X,
through the C ABI, against tests/encoder_ops_ref.py (tests/test_encoder_ops_ref_cpu.py shows on the CPU that the reference
agrees with torch's operators and rejects the wrong variants).  Every case runs once.  Every output lies between guard areas
pre-filled with a pattern no kernel writes (bf16 0x7FC1, bytes 0xEE, NaN for fp32 / fp64) and is pre-filled with it itself:
"guards intact, every inside element written" is checked for each.  The worst figures are printed at the end (-s).

A  isic_bn_stats_bf16: integer data (sums EQUAL, added to non-zero content), real data within the derived bound, refusals.
B  isic_bn_finalize on hand-made fp64 slot sums: mean / rstd / scale bit-equal, shift and the running statistics one of
   the candidate roundings; statistics + finalize against a two-pass fp64 mean and variance with the propagated bound.
C  isic_bn_eval_affine: scale bit-equal (correctly rounded fp32 divide and sqrt: the build's flags are checked), shift one
   of two candidates; both within the fp64 form's rounding distance.
D  isic_bn_apply_bf16 / _mask_bf16 / _mask_res_affine_bf16: bit-exact on the exact-product family, every element; mask bits;
   res_affine == apply_mask on the materialised residual; random data: every element one of the candidates.
E  max-pool forward (plain, fused generic, fused tiled) EQUAL to the restatement (first maximum in row-major scan, padding
   below every value), batch invariance, the fused form == apply + plain pool on the device; backward with the forward's
   codes and hand-made code planes, bit-equal to fp32 sums in the kernel's order.
   Outside the domain, not fed: +-inf and NaN.  The header says nothing about them, and a window of -inf only leaves tap
   code 0, which can name a pixel outside the image.
F  average pool forward (the kernel's order emulated) and backward, bit-equal; one case past the grid-stride loop.
G  isic_nchw_to_nhwc4_bf16: both kernels, the scalar one also through misaligned views, N past gridDim.y; bit-equal,
   round-to-nearest-even on ties, +-0, channels C..3 exactly +0.
H  refusals of every entry: the expected code, and the guarded outputs untouched.

Kernel instantiation -> a case that launches it (read from the host dispatch conditions of the entries):
  bn_stats_kernel                     A  every shape; one row lane per block at C = 2048, 256 at C = 8; at its 2048-block
                                         cap: 16385x2048, 524289x64
  bn_finalize_kernel                  B  every case; 128 blocks at C = 2048, a block with one live channel at C = 1 and 17
  bn_eval_affine_kernel               C  every C; a second block at C = 65 and 512
  bn_apply_kernel<false>              D  isic_bn_apply_bf16 (ReLU off / on, residual NULL / given) and isic_bn_apply_mask_bf16,
                                         vector counts 1 ... 1025 (ending in a block's first row, second row, on both edges)
  bn_apply_kernel<true>               D  isic_bn_apply_mask_res_affine_bf16, the same shapes
  maxpool_fwd_kernel<false>           E  isic_maxpool3x3s2_fwd_bf16, C = 8, 24, 64, 128, every (H, W)
  maxpool_fwd_kernel<true>            E  the fused entries at C = 8, 24, 128 (C != 64 is what sends them there)
  bn_relu_maxpool_c64_kernel<8, 8>    E  the fused entries at C = 64 (aligned input)
  maxpool_bwd_kernel                  E  every (H, W): the forward's codes, and the hand-made planes
  avgpool_fwd_kernel                  F  every case; a second blockIdx.y at C = 65, 512, 4096
  avgpool_bwd_kernel                  F  every case; past its 8192-block grid-stride loop: 3 x 196 x 4096
  nchw_to_nhwc4_kernel                G  HW = 1, 3, 1030 (HW % 4 != 0); HW = 4, 1028 through an fp32 / bf16 input view or an
                                         output that is not 16-byte aligned
  nchw_to_nhwc4_x4_kernel<false>      G  fp32 input, HW = 4, 1028 (a second block), N = 65537 (past gridDim.y = 65535)
  nchw_to_nhwc4_x4_kernel<true>       G  bf16 input, the same
Arms deliberately not run:
  the fused pool at C = 64 with an input that is not 16-byte aligned (-> maxpool_fwd_kernel<true>): the ABI's tensors are
      16-byte aligned everywhere else and a misaligned 16-byte vector load is not something to try on a shared machine;
  the fused pool at C = 64 with H * W > 2^24 (-> maxpool_fwd_kernel<true>): 2 GB per image;
  STREAM_CAP: a grid-capped bn_apply / plain pool / scalar layout launch needs 2^31 vectors.

Worst error / bound per entry, MI355X (the module prints the table at its end):
  A  statistics, real data          sum 0.000 (every fp32 partial of <= 9 bf16 values came out exact), sumsq 0.158
  B  statistics + finalize          centred data: mean 0.047, rstd 0.188 (of a bound of 3-9e-7 relative);
                                    data around 100: mean 0.071, rstd 0.000 (0.1 % of a bound of 3-6 % relative)
  C  eval affine                    scale against fp64: 0.609 of 1.5 ulp
  every equality check (A integer data, B, C, D, E, F, G): 0 bit patterns differ; every candidate check: 0 outside."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import encoder_ops_ref as R  # noqa: E402
from helpers import DEV, stop_after_a_device_error  # noqa: E402

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = -1, -2
EPS = 1e-5
WORST = {}
ids = lambda s: "x".join(map(str, s))


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _code(*a):
    """the return code of a call that is expected to be refused"""
    from isic_hip.lib import IsicHipError
    try:
        _call(*a)
    except IsicHipError as e:
        return e.code
    return 0


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for key in sorted(WORST):
        print("WORST", key, {k: (round(v, 4) if isinstance(v, float) else v) for k, v in WORST[key].items()})


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    stop_after_a_device_error()


def _note(key, **figures):
    w = WORST.setdefault(key, {})
    for k, v in figures.items():
        w[k] = max(w.get(k, 0), v)


class Guard:
    """an output of n elements between two guard areas, all pre-filled.  kind: "bf16" (int16 0x7FC1), "u8" (0xEE), "f32",
    "f64" (NaN).  offset: elements by which the output is moved off the buffer's alignment."""
    KINDS = {"bf16": (torch.int16, R.SENTINEL), "u8": (torch.uint8, R.BYTE_SENTINEL), "f32": (torch.float32, float("nan")),
             "f64": (torch.float64, float("nan"))}

    def __init__(self, n, kind, offset=0, init=None, guard=2048):
        dtype, self.fill = self.KINDS[kind]
        self.kind, self.n, self.lo = kind, int(n), guard + offset
        self.buf = torch.full((2 * guard + self.n + offset,), self.fill, device=DEV, dtype=dtype)
        self.raw = self.buf[self.lo:self.lo + self.n]
        if init is not None:
            self.raw.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(DEV).view(dtype) if isinstance(init, np.ndarray) else init)
        self.t = self.raw.view(torch.bfloat16) if kind == "bf16" else self.raw

    def _is_fill(self, t):
        return torch.isnan(t) if self.kind in ("f32", "f64") else t == self.fill

    def check(self, what, written=True):
        torch.cuda.synchronize()
        assert bool(self._is_fill(self.buf[:self.lo]).all()) and bool(self._is_fill(self.buf[self.lo + self.n:]).all()), \
            f"{what}: a guard area was written"
        if written:
            assert not bool(self._is_fill(self.raw).any()), f"{what}: an output element was not written"

    def untouched(self, what):
        torch.cuda.synchronize()
        assert bool(self._is_fill(self.buf).all()), f"{what}: a refused call wrote"

    def np(self):
        a = self.raw.cpu().numpy()
        return a.view(np.uint16) if self.kind == "bf16" else a


def _bf16(values):
    """fp32 values that bf16 holds exactly -> device bf16 tensor"""
    values = np.asarray(values, dtype=np.float32)
    bits = R.bf16_bits(values).reshape(values.shape)
    assert np.array_equal(R.bf16_value(bits).reshape(values.shape).view(np.uint32), values.view(np.uint32))
    return torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.bfloat16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _equal(got, want, what, key):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    view = {4: np.uint32, 8: np.uint64}.get(got.dtype.itemsize, got.dtype) if got.dtype.kind == "f" else got.dtype
    n = int((got.view(view) != want.astype(got.dtype).view(view)).sum())
    print(f"{what}: {n} of {want.size} bit patterns differ")
    _note(key, differing=n)
    assert n == 0, f"{what}: {n} of {want.size} bit patterns differ from the reference"


def _among(got, cands, what, key):
    ok = R.among(np.asarray(got).reshape(cands.shape[1:]), cands)
    n = int((~ok).sum())
    print(f"{what}: {n} of {ok.size} are none of the {len(cands)} candidate roundings")
    _note(key, outside_candidates=n)
    assert n == 0, f"{what}: {n} of {ok.size} values are none of the candidate roundings"


# ================================================================================================ A  statistics
def _stats(x_dev, rows, C, start1, start2):
    s1, s2 = Guard(C, "f64", init=start1), Guard(C, "f64", init=start2)
    _call("isic_bn_stats_bf16", x_dev, rows, C, s1.t, s2.t)
    s1.check("sum"), s2.check("sumsq")
    return s1.np(), s2.np()


@pytest.mark.parametrize("shape", R.stats_shapes() + list(R.STATS_CAP_CASES), ids=ids)
def test_stats(shape):
    rows, C = shape
    rls, grid, per_block, k = R.stats_geometry(rows, C)
    # integer data: every fp32 partial and every fp64 sum is exact in any order -> equality, on top of non-zero content
    v = R.integer_family(rows, C, seed=rows * 31 + C)
    assert k * 16 * 16 < 2 ** 24
    start1, start2 = (np.arange(C) % 7 - 3).astype(np.float64), (np.arange(C) % 5 + 1).astype(np.float64)
    s1, s2 = _stats(_bf16(v.astype(np.float32)), rows, C, start1, start2)
    _equal(s1, start1 + v.sum(0), f"stats {shape} integer sum", "A stats integer")
    _equal(s2, start2 + (v * v).sum(0), f"stats {shape} integer sumsq", "A stats integer")
    del v
    # real data against the correctly rounded sums
    x = R.real_family(rows, C, seed=rows * 17 + C)
    e1, e2, a1 = R.stats_exact(x)
    s1, s2 = _stats(_bf16(x), rows, C, np.zeros(C), np.zeros(C))
    r1 = float(np.max(np.abs(s1 - e1) / (R.stats_bound(rows, C, a1) + 1e-300)))
    r2 = float(np.max(np.abs(s2 - e2) / (R.stats_bound(rows, C, e2) + 1e-300)))
    print(f"stats {shape} real: k {k} grid {grid}; worst error / bound: sum {r1:.3f} sumsq {r2:.3f}")
    _note("A stats real", sum=r1, sumsq=r2)
    assert r1 <= 1.0 and r2 <= 1.0


def test_stats_refusals():
    x = _bf16(np.ones((4, 4096), dtype=np.float32))
    s1, s2 = Guard(4096, "f64"), Guard(4096, "f64")
    for C, code in ((24, UNSUPPORTED), (4096, UNSUPPORTED), (4, UNSUPPORTED), (0, BAD_ARG), (-8, BAD_ARG)):
        assert _code("isic_bn_stats_bf16", x, 4, C, s1.t, s2.t) == code, C
    assert _code("isic_bn_stats_bf16", x, 0, 64, s1.t, s2.t) == BAD_ARG
    assert _code("isic_bn_stats_bf16", None, 4, 64, s1.t, s2.t) == BAD_ARG
    assert _code("isic_bn_stats_bf16", x, 4, 64, None, s2.t) == BAD_ARG
    assert _code("isic_bn_stats_bf16", x, 4, 64, s1.t, None) == BAD_ARG
    s1.untouched("sum"), s2.untouched("sumsq")


# ================================================================================================ B  finalize
def _finalize(cs, nslots, C, rows, momentum, running=True):
    out = {k: Guard(C, "f32") for k in ("scale", "shift", "mean", "rstd")}
    rm = Guard(C, "f32", init=cs["rm0"]) if running else None
    rv = Guard(C, "f32", init=cs["rv0"]) if running else None
    _call("isic_bn_finalize", _dev(cs["sum"]), _dev(cs["sumsq"]), nslots, rows, C, _dev(cs["gamma"]), _dev(cs["beta"]), EPS,
          momentum, out["scale"].t, out["shift"].t, out["mean"].t, out["rstd"].t, rm.t if running else None,
          rv.t if running else None)
    for k, g in out.items():
        g.check(k)
    if running:
        rm.check("running_mean"), rv.check("running_var")
        out.update(running_mean=rm, running_var=rv)
    return {k: g.np() for k, g in out.items()}


def _check_finalize(got, f, what, running=True):
    for k in ("mean", "rstd", "scale"):
        _equal(got[k], f[k], f"{what} {k}", "B finalize")
    for k in ("shift",) + (("running_mean", "running_var") if running else ()):
        _among(got[k], f[k], f"{what} {k}", "B finalize")


@pytest.mark.parametrize("case", R.FINALIZE_CASES, ids=ids)
def test_finalize(case):
    nslots, C, rows = case
    cs = R.finalize_case(nslots, C, rows, seed=nslots * 7 + C)
    f = R.finalize(cs["sum"], cs["sumsq"], rows, cs["gamma"], cs["beta"], EPS, 0.1, cs["rm0"], cs["rv0"])
    assert f["var_forms_agree"].all() and f["running_var_forms_agree"].all()
    _check_finalize(_finalize(cs, nslots, C, rows, 0.1), f, f"finalize {case} momentum 0.1")


@pytest.mark.parametrize("momentum", [0.0, 1.0])
def test_finalize_momentum_edges_and_no_running_statistics(momentum):
    nslots, C, rows = 17, 64, 90
    cs = R.finalize_case(nslots, C, rows, seed=nslots * 7 + C)
    f = R.finalize(cs["sum"], cs["sumsq"], rows, cs["gamma"], cs["beta"], EPS, momentum, cs["rm0"], cs["rv0"])
    got = _finalize(cs, nslots, C, rows, momentum)
    _check_finalize(got, f, f"finalize momentum {momentum}")
    if momentum == 0.0:
        assert np.array_equal(got["running_mean"], cs["rm0"]) and np.array_equal(got["running_var"], cs["rv0"])
    _check_finalize(_finalize(cs, nslots, C, rows, momentum, running=False), f, "finalize without running statistics", False)


def test_finalize_refusals():
    C = 64
    cs = R.finalize_case(2, C, 90, seed=1)
    o = [Guard(C, "f32") for _ in range(6)]
    base = [_dev(cs["sum"]), _dev(cs["sumsq"]), 2, 90, C, _dev(cs["gamma"]), _dev(cs["beta"]), EPS, 0.1] + [g.t for g in o]

    def with_(i, v):
        a = list(base)
        a[i] = v
        return a
    for i, v in ((13, None), (14, None), (2, 0), (3, 0), (4, 0), (0, None), (1, None), (5, None), (6, None), (9, None), (10, None),
                 (11, None), (12, None)):
        assert _code("isic_bn_finalize", *with_(i, v)) == BAD_ARG, (i, v)
    for g in o:
        g.untouched("finalize output")


@pytest.mark.parametrize("family", ["unit", "mean100"])
def test_statistics_then_finalize_against_two_pass(family):
    """The one-pass variance s2 / n - mean^2 conditions like mean^2 / var: the propagated bound says so, and the mean-100
    family shows how much of it is used."""
    worst = {"mean": 0.0, "rstd": 0.0}
    for C in (8, 64, 2048):
        rows = 3 * 8 * (2048 // C) + 5
        x = R.real_family(rows, C, seed=rows + C, mean=100.0 if family == "mean100" else 0.0)
        _, e2, a1 = R.stats_exact(x)
        s1, s2 = _stats(_bf16(x), rows, C, np.zeros(C), np.zeros(C))
        cs = dict(sum=s1[None], sumsq=s2[None], gamma=np.ones(C, dtype=np.float32), beta=np.zeros(C, dtype=np.float32),
                  rm0=np.zeros(C, dtype=np.float32), rv0=np.ones(C, dtype=np.float32))
        got = _finalize(cs, 1, C, rows, 0.1)
        mean, var = R.two_pass(x)
        dmean, drstd = R.composition_bound(rows, C, a1, e2, mean, var, EPS)
        rstd = 1.0 / np.sqrt(var + np.float64(np.float32(EPS)))
        rm = float(np.max(np.abs(got["mean"] - mean) / dmean))
        rr = float(np.max(np.abs(got["rstd"] - rstd) / rstd / drstd))
        print(f"stats + finalize {family} C {C} rows {rows}: error / propagated bound: mean {rm:.3f} rstd {rr:.3f} "
              f"(the bound on rstd itself: {float(drstd.max()):.2e} relative)")
        worst = {"mean": max(worst["mean"], rm), "rstd": max(worst["rstd"], rr)}
    _note(f"B stats+finalize {family}", **worst)
    assert worst["mean"] <= 1.0 and worst["rstd"] <= 1.0


# ================================================================================================ C  eval affine
@pytest.mark.parametrize("C", [1, 63, 64, 65, 512])
def test_eval_affine(C):
    from isic_hip import build
    assert R.build_rounds_correctly(build.FLAGS), "the reference's fp32 divide / sqrt emulation needs the correctly rounded ones"
    rng = np.random.default_rng(C)
    gamma, beta, rm = (rng.standard_normal(C).astype(np.float32) for _ in range(3))
    rv = (rng.random(C) * 2).astype(np.float32)
    rv[C // 2] = np.float32(0)
    sc, sh = Guard(C, "f32"), Guard(C, "f32")
    _call("isic_bn_eval_affine", _dev(gamma), _dev(beta), _dev(rm), _dev(rv), EPS, C, sc.t, sh.t)
    sc.check("scale"), sh.check("shift")
    want_sc, want_sh = R.eval_affine(gamma, beta, rm, rv, EPS)
    _equal(sc.np(), want_sc, f"eval affine C {C} scale", "C eval affine")
    _among(sh.np(), want_sh, f"eval affine C {C} shift", "C eval affine")
    sc64, sh64 = R.eval_affine_f64(gamma, beta, rm, rv, EPS)
    r = float(np.max(np.abs(sc.np() - sc64) / (1.5 * 2.0 ** -23 * np.abs(sc64))))
    _note("C eval affine", scale_vs_fp64_over_1p5ulp=r)
    assert r <= 1.0


def test_eval_affine_refusals():
    v = _dev(np.ones(8, dtype=np.float32))
    sc, sh = Guard(8, "f32"), Guard(8, "f32")
    assert _code("isic_bn_eval_affine", v, v, v, v, EPS, 0, sc.t, sh.t) == BAD_ARG
    for i in range(4):
        a = [v, v, v, v]
        a[i] = None
        assert _code("isic_bn_eval_affine", *a, EPS, 8, sc.t, sh.t) == BAD_ARG
    assert _code("isic_bn_eval_affine", v, v, v, v, EPS, 8, None, sh.t) == BAD_ARG
    assert _code("isic_bn_eval_affine", v, v, v, v, EPS, 8, sc.t, None) == BAD_ARG
    sc.untouched("scale"), sh.untouched("shift")


# ================================================================================================ D  apply
def _run_apply(entry, d, rows, C, relu=1, residual=False):
    """one launch of an apply entry on the device operands d -> (y bits [rows, C], mask bytes or None)"""
    n = rows * C
    y = Guard(n, "bf16")
    m = Guard(n // 8, "u8") if entry != "apply" else None
    if entry == "apply":
        _call("isic_bn_apply_bf16", d["x"], d["scale"], d["shift"], d["res"] if residual else None, y.t, rows, C, relu)
    elif entry == "mask":
        _call("isic_bn_apply_mask_bf16", d["x"], d["scale"], d["shift"], d["res"] if residual else None, y.t, m.t, rows, C)
    else:
        _call("isic_bn_apply_mask_res_affine_bf16", d["x"], d["scale"], d["shift"], d["res"], d["rsc"], d["rsh"], y.t, m.t,
              rows, C)
    y.check(f"{entry} y")
    if m is not None:
        m.check(f"{entry} mask", written=False)
    return y.np().reshape(rows, C), (m.np() if m is not None else None), y


def _apply_operands(cs):
    d = {k: _bf16(cs[k]) for k in ("x", "res")}
    d.update({k: _dev(cs[k]) for k in ("scale", "shift", "rsc", "rsh")})
    return d


def _mask_written(mask, want, what):
    """a mask byte may legitimately be the sentinel 0xEE, so "written" is shown by equality with the reference (the guards
    are checked in _run_apply)"""
    _equal(mask, want, what, "D apply exact")


@pytest.mark.parametrize("shape", R.apply_shapes(), ids=ids)
def test_apply_exact_family(shape):
    rows, C = shape
    cs = R.apply_case(rows, C, seed=rows * 13 + C)
    d = _apply_operands(cs)
    for relu in (0, 1):
        for residual in (False, True):
            want, pos = R.bn_apply(cs["x"], cs["scale"], cs["shift"], relu, cs["res"] if residual else None)
            assert R.distinct_candidates(want) == 1
            got, _, _ = _run_apply("apply", d, rows, C, relu, residual)
            _equal(got, want[0], f"apply {shape} relu {relu} residual {residual}", "D apply exact")
            if relu:
                got, mask, _ = _run_apply("mask", d, rows, C, 1, residual)
                _equal(got, want[0], f"apply_mask {shape} residual {residual} y", "D apply exact")
                _mask_written(mask, R.pack_mask_bits(pos[0]), f"apply_mask {shape} residual {residual} mask")
    want, pos = R.bn_apply(cs["x"], cs["scale"], cs["shift"], 1, cs["res"], cs["rsc"], cs["rsh"])
    assert R.distinct_candidates(want) == 1
    got, mask, _ = _run_apply("res_affine", d, rows, C)
    _equal(got, want[0], f"apply_mask_res_affine {shape} y", "D apply exact")
    _mask_written(mask, R.pack_mask_bits(pos[0]), f"apply_mask_res_affine {shape} mask")
    # the kernel's own claim: == apply_mask on a residual materialised by isic_bn_apply_bf16(relu = 0), on the device
    idn = Guard(rows * C, "bf16")
    _call("isic_bn_apply_bf16", d["res"], d["rsc"], d["rsh"], None, idn.t, rows, C, 0)
    idn.check("materialised residual")
    got2, mask2, _ = _run_apply("mask", dict(d, res=idn.t), rows, C, 1, True)
    _equal(got2, got, f"apply_mask on the materialised residual {shape} y", "D apply exact")
    _equal(mask2, mask, f"apply_mask on the materialised residual {shape} mask", "D apply exact")


@pytest.mark.parametrize("entry", ["apply", "mask", "res_affine"])
def test_apply_random_family(entry):
    rows, C = 65, 64                                                  # 520 vectors: a second block with 8 of them
    cs = R.apply_case(rows, C, seed=77, exact=False)
    d = _apply_operands(cs)
    affine = entry == "res_affine"
    want, pos = R.bn_apply(cs["x"], cs["scale"], cs["shift"], 1, cs["res"], cs["rsc"] if affine else None, cs["rsh"] if affine else None)
    got, mask, _ = _run_apply(entry, d, rows, C, 1, True)
    # (value, mask bit) pairs: the device's pair must be one candidate's pair
    bit = R.unpack_mask_bytes(mask, C) if mask is not None else None
    ok = np.zeros((rows, C), dtype=bool)
    for k in range(len(want)):
        ok |= (got == want[k]) & (True if bit is None else bit == pos[k])
    n = int((~ok).sum())
    print(f"{entry} random family: {n} of {ok.size} (value, mask bit) pairs are none of the {len(want)} candidates; "
          f"{int((want[0] != want[1]).sum())} elements have two distinct candidates")
    _note("D apply random", outside_candidates=n)
    assert n == 0
    if entry == "apply":                                              # and without the ReLU
        want0, _ = R.bn_apply(cs["x"], cs["scale"], cs["shift"], 0, None)
        got0, _, _ = _run_apply("apply", d, rows, C, 0, False)
        _among(got0, want0, "apply random family, no ReLU, no residual", "D apply random")


def test_apply_refusals():
    cs = R.apply_case(4, 64, seed=1)
    d = _apply_operands(cs)
    y, m = Guard(4 * 64, "bf16"), Guard(4 * 8, "u8")
    x, sc, sh, res, rsc, rsh = (d[k] for k in ("x", "scale", "shift", "res", "rsc", "rsh"))
    for C, code in ((24, UNSUPPORTED), (4096, UNSUPPORTED), (12, BAD_ARG), (0, BAD_ARG)):
        assert _code("isic_bn_apply_bf16", x, sc, sh, None, y.t, 1, C, 1) == code, C
        assert _code("isic_bn_apply_mask_bf16", x, sc, sh, None, y.t, m.t, 1, C) == code, C
        assert _code("isic_bn_apply_mask_res_affine_bf16", x, sc, sh, res, rsc, rsh, y.t, m.t, 1, C) == code, C
    assert _code("isic_bn_apply_bf16", x, sc, sh, None, y.t, 0, 64, 1) == BAD_ARG
    assert _code("isic_bn_apply_bf16", None, sc, sh, None, y.t, 4, 64, 1) == BAD_ARG
    assert _code("isic_bn_apply_bf16", x, None, sh, None, y.t, 4, 64, 1) == BAD_ARG
    assert _code("isic_bn_apply_bf16", x, sc, None, None, y.t, 4, 64, 1) == BAD_ARG
    assert _code("isic_bn_apply_bf16", x, sc, sh, None, None, 4, 64, 1) == BAD_ARG
    assert _code("isic_bn_apply_mask_bf16", x, sc, sh, None, y.t, None, 4, 64) == BAD_ARG
    assert _code("isic_bn_apply_mask_bf16", x, sc, sh, None, y.t, m.t, 0, 64) == BAD_ARG
    assert _code("isic_bn_apply_mask_res_affine_bf16", x, sc, sh, None, rsc, rsh, y.t, m.t, 4, 64) == BAD_ARG
    assert _code("isic_bn_apply_mask_res_affine_bf16", x, sc, sh, res, None, rsh, y.t, m.t, 4, 64) == BAD_ARG
    assert _code("isic_bn_apply_mask_res_affine_bf16", x, sc, sh, res, rsc, None, y.t, m.t, 4, 64) == BAD_ARG
    assert _code("isic_bn_apply_mask_res_affine_bf16", x, sc, sh, res, rsc, rsh, y.t, None, 4, 64) == BAD_ARG
    y.untouched("y"), m.untouched("mask")


# ================================================================================================ E  max-pool
def _f32_bits_to_bf16(v):
    """fp32 values that are bf16 -> their 16 bits (the sign of a zero kept)"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any()
    return (u >> 16).astype(np.uint16)


def _pool_fwd(x_dev, N, H, W, C, affine=None, sel=True):
    """-> (y bits, codes[, x_sel bits]) of the plain entry (affine None) or a fused one"""
    Ho, Wo = R.pool_out(H, W)
    n = N * Ho * Wo * C
    y, am = Guard(n, "bf16"), Guard(n, "u8")
    if affine is None:
        _call("isic_maxpool3x3s2_fwd_bf16", x_dev, y.t, am.t, N, H, W, C, Ho, Wo)
        xs = None
    elif sel:
        xs = Guard(n, "bf16")
        _call("isic_bn_relu_maxpool3x3s2_fwd_sel_bf16", x_dev, affine[0], affine[1], y.t, am.t, xs.t, N, H, W, C, Ho, Wo)
    else:
        xs = None
        _call("isic_bn_relu_maxpool3x3s2_fwd_bf16", x_dev, affine[0], affine[1], y.t, am.t, N, H, W, C, Ho, Wo)
    y.check("pool y"), am.check("pool argmax")
    shape = (N, Ho, Wo, C)
    out = (y.np().reshape(shape), am.np().reshape(shape))
    if xs is not None:
        xs.check("pool x_sel")
        out += (xs.np().reshape(shape),)
    return out


@pytest.mark.parametrize("hw", R.POOL_HW, ids=ids)
def test_maxpool_forward(hw):
    H, W = hw
    for N in (1, 3):
        for C in (8, 24, 64, 128):
            f = R.pool_input(N, H, W, C, seed=H * 17 + W + C)
            x = _bf16(f)
            want_y, want_code = R.maxpool_fwd(f)
            y, code = _pool_fwd(x, N, H, W, C)
            what = f"maxpool fwd {hw} N {N} C {C}"
            _equal(y, _f32_bits_to_bf16(want_y), what + " y", "E maxpool fwd")
            _equal(code, want_code, what + " argmax", "E maxpool fwd")
            if N == 3:                                                # batch invariance
                for i in range(3):
                    yi, ci = _pool_fwd(x[i:i + 1].contiguous(), 1, H, W, C)
                    assert np.array_equal(yi[0], y[i]) and np.array_equal(ci[0], code[i]), f"{what}: image {i} alone differs"


@pytest.mark.parametrize("hw", R.POOL_HW, ids=ids)
def test_maxpool_fused_forward(hw):
    H, W = hw
    for N in (1, 3):
        for C in (8, 24, 64, 128):                                    # 64: the tiled kernel; the others: maxpool_fwd_kernel<true>
            f = R.pool_input(N, H, W, C, seed=H * 17 + W + C)
            scale, shift = R.pool_affine(C, seed=C)
            ab, _ = R.bn_apply(f.reshape(-1, C), scale, shift, 1)
            assert R.distinct_candidates(ab) == 1                     # both multiply-add forms agree on this data
            a = R.bf16_value(ab[0]).reshape(f.shape)
            want_y, want_code, want_raw = R.maxpool_fwd(a, raw=f)
            x, aff = _bf16(f), (_dev(scale), _dev(shift))
            y, code, xs = _pool_fwd(x, N, H, W, C, aff)
            what = f"fused pool {hw} N {N} C {C}"
            _equal(y, _f32_bits_to_bf16(want_y), what + " y", "E maxpool fused")
            _equal(code, want_code, what + " argmax", "E maxpool fused")
            _equal(xs, _f32_bits_to_bf16(want_raw), what + " x_sel", "E maxpool fused")
            y2, code2 = _pool_fwd(x, N, H, W, C, aff, sel=False)
            assert np.array_equal(y2, y) and np.array_equal(code2, code), what + ": the entry without x_sel differs"
            if R.bn_c_ok(C):                                          # (isic_bn_apply_bf16 has no C = 24)
                full = Guard(f.size, "bf16")
                _call("isic_bn_apply_bf16", x, aff[0], aff[1], None, full.t, N * H * W, C, 1)
                full.check("apply")
                y3, code3 = _pool_fwd(full.t, N, H, W, C)
                assert np.array_equal(y3, y) and np.array_equal(code3, code), what + ": apply + plain pool on the device differs"
            if N == 3:
                for i in range(3):
                    yi, ci, xi = _pool_fwd(x[i:i + 1].contiguous(), 1, H, W, C, aff)
                    assert np.array_equal(yi[0], y[i]) and np.array_equal(ci[0], code[i]) and np.array_equal(xi[0], xs[i]), \
                        f"{what}: image {i} alone differs"


def _pool_bwd(code, dy, N, H, W, C):
    Ho, Wo = R.pool_out(H, W)
    dx = Guard(N * H * W * C, "bf16")
    _call("isic_maxpool3x3s2_bwd_bf16", _dev(np.ascontiguousarray(code, dtype=np.uint8)), _bf16(dy), dx.t, N, H, W, C, Ho, Wo)
    dx.check("pool dx")
    return dx.np().reshape(N, H, W, C)


@pytest.mark.parametrize("hw", R.POOL_HW, ids=ids)
def test_maxpool_backward(hw):
    H, W = hw
    Ho, Wo = R.pool_out(H, W)
    for N, C in ((1, 8), (3, 8), (3, 128)):
        f = R.pool_input(N, H, W, C, seed=H * 17 + W + C)
        _, code = R.maxpool_fwd(f)                                    # == the device's own codes (test_maxpool_forward)
        rng = np.random.default_rng(H * W + C)
        real = R.bf16_value(R.bf16_bits(rng.standard_normal(code.shape).astype(np.float32) *
                                        np.float32(2.0) ** rng.integers(-6, 7, size=code.shape))).reshape(code.shape)
        integer = rng.integers(-8, 9, size=code.shape).astype(np.float32)
        for name, dy in (("real", real), ("integer", integer)):
            _equal(_pool_bwd(code, dy, N, H, W, C), R.maxpool_bwd(code, dy, H, W),
                   f"maxpool bwd {hw} N {N} C {C} own codes, {name} gradient", "E maxpool bwd")
        if C == 8:
            for kind in R.HANDMADE:
                plane = R.handmade_codes(kind, H, W)
                assert R.code_inside(plane, H, W).all()
                codes = np.ascontiguousarray(np.broadcast_to(plane[None, :, :, None], code.shape))
                _equal(_pool_bwd(codes, real, N, H, W, C), R.maxpool_bwd(codes, real, H, W),
                       f"maxpool bwd {hw} N {N} plane {kind}", "E maxpool bwd")


def test_maxpool_refusals():
    N, H, W, C = 1, 5, 4, 8
    Ho, Wo = R.pool_out(H, W)
    x = _bf16(R.pool_input(N, H, W, 16, seed=1))
    v = _dev(np.ones(16, dtype=np.float32))
    n = N * Ho * Wo * 16
    y, am, xs, dx = Guard(n, "bf16"), Guard(n, "u8"), Guard(n, "bf16"), Guard(N * H * W * 16, "bf16")
    code, dy = _dev(np.full(n, 4, dtype=np.uint8)), _bf16(np.ones(n, dtype=np.float32))
    for a in ((N, H, W, C, Ho + 1, Wo), (N, H, W, C, Ho, Wo - 1), (N, H, W, C, H, W), (N, H, W, 12, Ho, Wo), (N, H, W, 0, Ho, Wo),
              (0, H, W, C, Ho, Wo), (N, 0, W, C, Ho, Wo), (N, H, 0, C, Ho, Wo)):
        assert _code("isic_maxpool3x3s2_fwd_bf16", x, y.t, am.t, *a) == BAD_ARG, a
        assert _code("isic_bn_relu_maxpool3x3s2_fwd_bf16", x, v, v, y.t, am.t, *a) == BAD_ARG, a
        assert _code("isic_bn_relu_maxpool3x3s2_fwd_sel_bf16", x, v, v, y.t, am.t, xs.t, *a) == BAD_ARG, a
        assert _code("isic_maxpool3x3s2_bwd_bf16", code, dy, dx.t, *a) == BAD_ARG, a      # Ho, Wo checked like the forward's
    good = (N, H, W, C, Ho, Wo)
    assert _code("isic_maxpool3x3s2_fwd_bf16", None, y.t, am.t, *good) == BAD_ARG
    assert _code("isic_maxpool3x3s2_fwd_bf16", x, None, am.t, *good) == BAD_ARG
    assert _code("isic_bn_relu_maxpool3x3s2_fwd_sel_bf16", x, None, v, y.t, am.t, xs.t, *good) == BAD_ARG
    assert _code("isic_bn_relu_maxpool3x3s2_fwd_sel_bf16", x, v, None, y.t, am.t, xs.t, *good) == BAD_ARG
    assert _code("isic_maxpool3x3s2_bwd_bf16", None, dy, dx.t, *good) == BAD_ARG
    assert _code("isic_maxpool3x3s2_bwd_bf16", code, None, dx.t, *good) == BAD_ARG
    assert _code("isic_maxpool3x3s2_bwd_bf16", code, dy, None, *good) == BAD_ARG
    for g in (y, am, xs, dx):
        g.untouched("pool output")


# ================================================================================================ F  average pool
def _avg(N, HW, C, seed):
    x = R.avg_input(N, HW, C, seed)
    y = Guard(N * C, "f32")
    _call("isic_avgpool_fwd_bf16", _bf16(x), y.t, N, HW, C)
    y.check("avgpool y")
    _equal(y.np(), R.avgpool_fwd(x), f"avgpool fwd N {N} HW {HW} C {C}", "F avgpool")
    dy, planted = R.avg_bwd_input(N, C, HW, seed)
    dx = Guard(N * HW * C, "bf16")
    _call("isic_avgpool_bwd_bf16", _dev(dy), dx.t, N, HW, C)
    dx.check("avgpool dx")
    _equal(dx.np(), R.avgpool_bwd(dy, HW), f"avgpool bwd N {N} HW {HW} C {C} ({planted} tie-adjacent values per row)", "F avgpool")


@pytest.mark.parametrize("HW", R.AVG_HW)
def test_avgpool(HW):
    from isic_hip import build
    assert R.build_rounds_correctly(build.FLAGS)                      # the forward's division is emulated as correctly rounded
    for C in R.AVG_C:
        for N in (1, 3):
            _avg(N, HW, C, seed=HW * 7 + C)


def test_avgpool_past_the_grid_stride_loop():
    N, HW, C = 3, 196, 4096
    assert N * HW * C > R.AVG_BWD_GRID_CAP * 256
    _avg(N, HW, C, seed=5)


def test_avgpool_refusals():
    x, dy = _bf16(np.ones(64, dtype=np.float32)), _dev(np.ones(8, dtype=np.float32))
    y, dx = Guard(8, "f32"), Guard(64, "bf16")
    for a in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert _code("isic_avgpool_fwd_bf16", x, y.t, *a) == BAD_ARG and _code("isic_avgpool_bwd_bf16", dy, dx.t, *a) == BAD_ARG, a
    assert _code("isic_avgpool_fwd_bf16", None, y.t, 1, 8, 8) == BAD_ARG and _code("isic_avgpool_fwd_bf16", x, None, 1, 8, 8) == BAD_ARG
    assert _code("isic_avgpool_bwd_bf16", None, dx.t, 1, 8, 8) == BAD_ARG and _code("isic_avgpool_bwd_bf16", dy, None, 1, 8, 8) == BAD_ARG
    y.untouched("y"), dx.untouched("dx")


# ================================================================================================ G  layout
def _layout(N, C, HW, is_bf16, in_offset=0, out_offset=0):
    x = R.layout_input(N, C, HW, seed=N * 5 + C + HW)
    src = R.bf16_bits(x).reshape(x.shape) if is_bf16 else x
    flat = torch.from_numpy(np.ascontiguousarray(src).reshape(-1).view(np.int16 if is_bf16 else np.float32))
    buf = torch.zeros(flat.numel() + in_offset, dtype=flat.dtype, device=DEV)
    view = buf[in_offset:]
    view.copy_(flat)
    assert buf.data_ptr() % 16 == 0 and (view.data_ptr() % 16 == 0) == (in_offset == 0)
    out = Guard(N * HW * 4, "bf16", offset=out_offset)
    assert (out.raw.data_ptr() % 16 == 0) == (out_offset == 0) and out.raw.data_ptr() % 8 == 0
    H, W = (2, HW // 2) if HW % 2 == 0 else (1, HW)
    _call("isic_nchw_to_nhwc4_bf16", view, int(is_bf16), out.t, N, C, H, W)
    out.check("nhwc4")
    got = out.np().reshape(N, 1, HW, 4)
    what = f"nchw_to_nhwc4 N {N} C {C} HW {HW} {'bf16' if is_bf16 else 'fp32'} offsets {in_offset}/{out_offset}"
    _equal(got, R.nchw_to_nhwc4(src, is_bf16), what, "G layout")
    assert (got[..., C:] == 0).all(), what + ": padding channels are not +0"


@pytest.mark.parametrize("is_bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_layout(C, is_bf16):
    for HW in (1, 3, 4, 1028, 1030):
        for N in (1, 3):
            _layout(N, C, HW, is_bf16)


@pytest.mark.parametrize("is_bf16", [False, True], ids=["fp32", "bf16"])
def test_layout_more_images_than_grid_rows(is_bf16):
    assert 65537 > R.GRID_Y_MAX
    _layout(65537, 3, 4, is_bf16)


@pytest.mark.parametrize("HW", [4, 1028])
def test_layout_scalar_kernel_through_misaligned_views(HW):
    """HW % 4 == 0 would take the four-pixel kernel; a view that is not 16-byte aligned keeps the one-pixel kernel, whose
    accesses (4-byte / 2-byte loads, 8-byte stores) stay naturally aligned"""
    _layout(3, 3, HW, False, in_offset=1)                             # fp32 input moved by one element
    _layout(3, 3, HW, True, in_offset=4)                              # bf16 input moved by 8 bytes
    _layout(3, 3, HW, False, out_offset=4)                            # output moved by 4 bf16
    _layout(3, 4, HW, True, out_offset=4)


def test_layout_refusals():
    x = _dev(np.ones(5 * 16, dtype=np.float32))
    out = Guard(64, "bf16")
    for a in ((1, 5, 4, 4), (1, 0, 4, 4), (0, 3, 4, 4), (1, 3, 0, 4), (1, 3, 4, 0)):
        assert _code("isic_nchw_to_nhwc4_bf16", x, 0, out.t, *a) == BAD_ARG, a
    assert _code("isic_nchw_to_nhwc4_bf16", None, 0, out.t, 1, 3, 4, 4) == BAD_ARG
    assert _code("isic_nchw_to_nhwc4_bf16", x, 0, None, 1, 3, 4, 4) == BAD_ARG
    out.untouched("nhwc4")
