"""The exact-fp32 GEMM family over its dispatch domains on the MI355X, through isic_test_gemm_f32_variant and the ABI entries
isic_gemm_f32_ws / _rows_ws / _add_ws, against the fp64 references of tests/gemm_f32_ref.py.  The inputs are chosen so that
fp32 is exact in any summation order (tests/test_gemm_f32_ref_cpu.py shows it on the CPU): every family I and family P result
must EQUAL the reference -- there is no tolerance in this module except the tanh epilogue's, R.TANH_BOUND = 1.5e-7 (the figure
csrc/common.h documents for isic_tanhf) + 2^-25 (rounding the fp64 reference to fp32).

Around every call: the output lies between NaN guards with ldc > N and a sentinel in the gap columns, pre-filled with NaN when
beta = 0; the operands have ld > width with NaN in the gap and NaN guards around them; the workspace is pre-filled with NaN,
sized exactly as isic_gemm_f32_workspace_bytes says and followed by a guard.  Each case names the kernel it is meant for and
asserts that this variant returns ISIC_OK, then runs variants 0 and 1 as well: all equal the reference, hence each other.
A variant that must refuse returns ISIC_ERR_UNSUPPORTED and leaves the NaN-filled output untouched.

Kernel instantiation -> a case that launches it (read from the host dispatch conditions, mirrored in gemm_f32_ref.py):
  gemm_f32_kernel                        every v1-* case: 1x1x1 ... 130x67x250 in all four transpositions, vector and scalar load4
                                         per operand (ld % 4 != 0, pointer + 1), every epilogue and beta
  ... split-K + the split reducer        v1-split-*-wsfull (tiny rule 100x70x1000: 13 x 80 k; long rule 128x200x20000: 74 x 272 k)
  gemm_scale_kernel + atomics            v1-split-*-wsshort / -wsnone with beta 0 and 0.5 (beta = 1: the atomics alone, no scale pass),
                                         v3-refuse-wsnone (64x64x4096 on the generic kernel; -wsshort still holds its 16 partials)
  gemm_f32p_kernel<true, true>           v2-NT-6148x516x260, v2-split-NT-260x516x4100, v2-swap-NT-128x772x8200, rows-fwd,
                                         rows-swap-nt (gathered row tiles under swapped roles); two row tiles per block:
                                         v2-tiles2-NT-66000x128x68, rows-fwd-66004x128x68 (the index read again for the second tile)
  gemm_f32p_kernel<true, false>          v2-NN-6148x516x260, v2-split-NN-260x516x4100-wsnone
  gemm_f32p_kernel<false, true>          v2-TT-6148x516x260
  gemm_f32p_kernel<false, false>         v2-TN-6148x516x260, v2-split-TN-260x516x4100, v2-swap-TN-128x772x8200 (swapped: the
                                         caller's B is the row-tile operand), rows-wgrad (gathered k rows); two row tiles per
                                         block: v2-tiles2-TN-66000x128x64
  ... vecC = 0                           v2-NT-6148x516x260-ldc%4, v2-TN-6148x516x260-C+1;  transC: every v2-swap case
  gemm_f32p_reduce_kernel                v2-split-* (bias + tanh, bias + ReLU with every beta), v2-swap-*-wsfull
  gemm_tn_skinny_kernel                  v3-64x64x{4096, 4097, 4099, 4292}, v3-128x256x9001, v3-forced-512x256x4096 / -64x2048x5000
  the split reducer (slab_reduce.hip)    lds16 form: the v3 and v1-split-wsfull cases with ldc % 4 == 0; xor16 form:
                                         v3-128x256x9001-ldc, v1-split-*-wsfull at N = 70 (N % 4 != 0)
  gemm_rowpanel_kernel<1..8, false>      v4-K{16 ... 128}-*-add0 (KC = K / 16): at M ~ 4100 every wave has ONE unit, fetched and drained
                                         before the loop; v4-steady-*-add0 (M = 20003 / 40003: 10 or 20 units per block of 8 waves) are the
                                         cases where a wave multiplies a PREFETCHED unit, i.e. where the hand-counted vmcnt(4) (beta = 0)
                                         and the drained wait (beta = 0.5, ragged last panel) protect registers that are used
  gemm_rowpanel_kernel<1..8, true>       v4-K{16 ... 128}-*-add1 through isic_gemm_f32_add_ws; prefetched addend rows: v4-steady-*-add1
  add2d_kernel                           v4-add-K130

Worst |device - tanh| per kernel, MI355X (bound 1.798e-07; e_tanh 1.076e-07 is recorded in tests/test_gated_pool_gpu.py for
random normal inputs -- here the pre-activations lie on the grid of multiples of 1/64 in [-9.5, 9.5]):
  gemm_f32_kernel 9.493e-08, gemm_f32p_kernel / gemm_f32p_reduce_kernel 9.493e-08, gemm_rowpanel_kernel 9.493e-08, the
  shipped choice 9.493e-08 (one epilogue function, isic_tanhf, and the same worst grid point in every kernel).
The module prints the figures at its end (visible with -s)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_f32_ref as R  # noqa: E402
from helpers import DEV, NAN, PAD, Guarded, stop_after_a_device_error  # noqa: E402

pytestmark = pytest.mark.gpu
OK, UNSUPPORTED = 0, -2
SENTINEL = 777.0
WORST_TANH = {}
KERNEL = {0: "shipped choice", 1: "gemm_f32_kernel", 2: "gemm_f32p_kernel / reduce", 4: "gemm_rowpanel_kernel"}


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _code(*a):
    """the return code of a call"""
    from isic_hip.lib import IsicHipError
    try:
        _call(*a)
    except IsicHipError as e:
        return e.code
    return OK


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for v in sorted(WORST_TANH):
        print(f"worst tanh error, {KERNEL[v]}: {WORST_TANH[v]:.3e} (bound {R.TANH_BOUND:.3e})")


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    stop_after_a_device_error()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


class Operand:
    """a stored matrix [rows][width] on the device with leading dimension ld > width, NaN in the gap, PAD NaN floats before and
    after it, optionally one float off 16-byte alignment"""

    def __init__(self, mat, pad=4, offset=0):
        rows, width = mat.shape
        self.ld = R.leading(width, pad)
        n = rows * self.ld
        host = torch.full((2 * PAD + n + 4,), NAN, dtype=torch.float32)
        lo = PAD + offset
        host[lo:lo + n].view(rows, self.ld)[:, :width] = mat
        self.buf = host.to(DEV)
        self.t = self.buf[lo:lo + n]


def _vector(v, offset=0):
    if v is None:
        return None
    host = torch.full((2 * PAD + v.numel() + 4,), NAN, dtype=torch.float32)
    host[PAD + offset:PAD + offset + v.numel()] = v
    return host.to(DEV)[PAD + offset:PAD + offset + v.numel()]


class Output:
    """C[M][ldc] as a Guarded: C0 (beta != 0) or NaN (beta = 0: no kernel may read C then) in the N columns, a sentinel in the gap"""

    def __init__(self, c, C0, beta=None):
        beta = c.beta if beta is None else beta
        self.N, self.ldc = c.N, R.leading(c.N, c.pc)
        init = torch.full((c.M, self.ldc), SENTINEL)
        init[:, :c.N] = C0 if beta != 0.0 else NAN
        self.g = Guarded((c.M, self.ldc), c.oc, init=init)

    @property
    def t(self):
        return self.g.t

    def result(self):
        """the N columns on the CPU, after checking the guards and the gap"""
        assert self.g.ok(finite=False), "a guard around C was written"
        host = self.g.cpu()
        assert bool((host[:, self.N:] == SENTINEL).all()), "a gap column of C was written"
        return host[:, :self.N].contiguous()

    def untouched(self):
        host = self.g.cpu()
        return self.g.ok(finite=False) and bool((host[:, self.N:] == SENTINEL).all()) and bool(torch.isnan(host[:, :self.N]).all())


class Workspace:
    """NaN-filled, exactly `nbytes` long (mode full), 4 bytes less (short), absent (none) or one float off 16-byte alignment
    (misaligned), followed by a NaN guard"""

    def __init__(self, nbytes, mode):
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        off = 1 if mode == "misaligned" else 0
        self.buf = torch.full((off + self.n + PAD,), NAN, device=DEV, dtype=torch.float32)
        self.body = self.buf[off:off + self.n]
        self.ptr = None if mode == "none" else self.buf[off:]
        self.bytes = 0 if mode == "none" else max(nbytes - 4, 0) if mode == "short" else nbytes

    def intact(self):
        return bool(torch.isnan(self.buf[self.buf.numel() - PAD:]).all())

    def written(self):
        """floats up to the last one written (exact inputs never produce a NaN partial)"""
        nz = (~torch.isnan(self.body)).nonzero()
        return int(nz.max()) + 1 if nz.numel() else 0


class Device:
    """the operands of a case on the device"""

    def __init__(self, c, inp):
        self.A = Operand(R.stored(inp.opA, c.ta), c.pa, c.oa)
        self.B = Operand(R.stored(inp.opB, c.tb), c.pb, c.ob)            # tb: stored [N][K]
        self.bias = _vector(inp.bias, c.obias)
        self.addend = Operand(inp.addend, c.padd) if inp.addend is not None else None
        self.nbytes = _call("isic_gemm_f32_workspace_bytes", c.ta, c.tb, c.M, c.N, c.K)


def _gemm_args(c, d, out, ws, act=None, beta=None):
    return (c.ta, c.tb, c.M, c.N, c.K, d.A.t, d.A.ld, d.B.t, d.B.ld, out.t, out.ldc, d.bias if c.bias else None,
            c.act if act is None else act, c.beta if beta is None else beta, ws.ptr, ws.bytes)


def _run(variant, c, d, inp, ws_mode=None):
    """one call of a variant -> (return code, Output, Workspace)"""
    out = Output(c, inp.C0)
    ws = Workspace(d.nbytes, c.ws if ws_mode is None else ws_mode)
    rc = _code("isic_test_gemm_f32_variant", variant, *_gemm_args(c, d, out, ws))
    assert ws.intact(), "the guard behind the workspace was written"
    return rc, out, ws


def _compare(c, v, got, ref, what):
    if c.act == R.ACT_TANH:
        err, sat_ok, zero_ok = R.tanh_error(got, ref)
        print(f"{c.id} variant {v}: tanh error {err:.3e}")
        WORST_TANH[v] = max(WORST_TANH.get(v, 0.0), err)
        assert err <= R.TANH_BOUND, (what, err)
        assert sat_ok, (what, "|p| >= 9.25 must give exactly +-1")
        assert zero_ok, (what, "p = 0 must give 0")
    else:
        want = ref.out.float()
        if not torch.equal(got, want):
            bad = (got != want) | torch.isnan(got)
            idx = bad.nonzero()[:5].tolist()
            raise AssertionError((what, f"{int(bad.sum())} of {bad.numel()} differ", idx,
                                  [(float(got[i, j]), float(want[i, j])) for i, j in idx]))


@pytest.mark.parametrize("c", R.CASES, ids=[c.id for c in R.CASES])
def test_family_I_equals_the_reference_on_the_pinned_kernel_and_the_shipped_one(c):
    cus = _cus()
    inp = R.inputs(c, "I", cus)
    plain = R.Box(c, add=0)
    ref = R.reference(plain, R.Box(inp, addend=None), cache=True)     # the product every variant call computes
    d = Device(c, inp)
    for v in c.refuse:
        out = Output(c, inp.C0, beta=0.0)
        ws = Workspace(d.nbytes, c.ws)
        assert _code("isic_test_gemm_f32_variant", v, *_gemm_args(c, d, out, ws)) == UNSUPPORTED, (c.id, v, c.why)
        assert out.untouched() and ws.intact() and ws.written() == 0, (c.id, v)
    for v in (c.variant,) + tuple(x for x in c.also if x != c.variant):
        rc, out, ws = _run(v, c, d, inp)
        assert rc == OK, (c.id, "variant", v, "returned", rc)
        _compare(c, v, out.result(), ref, (c.id, "variant", v))
        if v == c.variant and c.variant != 4:
            # the pinned kernel's own use of the workspace: ordered partials where they fit (and, persistent kernel, are aligned)
            want = R.partial_floats(c, v, cus)
            if ws.ptr is None or ws.bytes < 4 * want or (v == 2 and c.ws == "misaligned"):
                want = 0
            assert ws.written() == want, (c.id, "workspace floats written", ws.written(), want)
        if v == 0 and c.forced_only:                       # the shipped choice is NOT the A^T B kernel: its partials are not there
            choice = R.shipped_choice(c, cus)
            assert choice != 3 and ws.written() == R.partial_floats(c, choice, cus) != R.partial_floats(c, 3, cus), (c.id, ws.written())
    if c.add:                                              # the same arguments with an addend, through the ABI entry
        full = R.reference(c, inp)
        out = Output(c, inp.C0)
        ws = Workspace(d.nbytes, c.ws)
        rc = _code("isic_gemm_f32_add_ws", *_gemm_args(c, d, out, ws)[:-2], d.addend.t, d.addend.ld, ws.ptr, ws.bytes)
        assert rc == OK and ws.intact(), (c.id, rc)
        _compare(c, c.variant, out.result(), full, (c.id, "isic_gemm_f32_add_ws"))


P_CASES = [c for c in R.CASES if c.P]


@pytest.mark.parametrize("family", ("PA", "PB"))
@pytest.mark.parametrize("c", P_CASES, ids=[c.id for c in P_CASES])
def test_family_P_keeps_every_operand_bit(c, family):
    cus = _cus()
    cp = R.family_p_case(c)
    inp = R.inputs(cp, family, cus)
    ref = R.reference(cp, inp)
    assert R.exact_in_fp32(ref.out)
    d = Device(cp, inp)
    for v in (c.variant,) + tuple(x for x in c.also if x != c.variant):
        rc, out, ws = _run(v, cp, d, inp)
        assert rc == OK, (c.id, family, "variant", v, "returned", rc)
        _compare(cp, v, out.result(), ref, (c.id, family, "variant", v))


@pytest.mark.parametrize("c", R.REPEAT_CASES, ids=[c.id for c in R.REPEAT_CASES])
def test_order_fixed_split_paths_repeat_bit_for_bit(c):
    inp = R.random_inputs(c)
    d = Device(c, inp)
    runs = []
    for _ in range(2):
        rc, out, ws = _run(c.variant, c, d, inp)
        assert rc == OK and ws.written() == R.partial_floats(c, c.variant, _cus()) > 0, c.id
        got = out.result()
        assert bool(torch.isfinite(got).all())
        runs.append(got.view(torch.int32))
    assert torch.equal(runs[0], runs[1]), c.id


def _rows_call(c, A, a_rows, B, b_rows, bias, out, ws):
    return _code("isic_gemm_f32_rows_ws", c.ta, c.tb, c.M, c.N, c.K, A.t, A.ld, a_rows, B.t, B.ld, b_rows, out.t, out.ldc, bias, c.act,
                 c.beta, ws.ptr, ws.bytes)


def _index(rows, nan_row):
    """the index on the device, padded to a multiple of 8 entries that point at the all-NaN stored row (as every entry behind it
    does: whatever is read there is a valid row number)"""
    padded = R.padded8(rows, nan_row)
    return torch.cat([padded, torch.full((PAD,), nan_row, dtype=torch.int32)]).to(DEV)[:padded.numel()]


@pytest.mark.parametrize("form", sorted(R.ROWS_FORMS))
def test_gathered_rows(form):
    c, which = R.ROWS_FORMS[form]
    inp = R.inputs(c, "I", _cus())
    g = torch.Generator().manual_seed(8)
    # the stored matrix that is gathered: x [rows of A][K] (forward), X [k rows of B][N] (weight gradient), W [rows of B][K] (swap-nt)
    count, width = (c.M, c.K) if which == "A" else (c.N, c.K) if c.tb else (c.K, c.N)
    n_store = count + R.ROWS_STORE_EXTRA
    store = R.dyadic((n_store, width), 1, g)
    store[n_store - 1] = NAN                               # the row the pad entries of the index point at
    rows = R.gather_index(count, n_store - 1, g)
    assert count % 8 and bool((rows[1:] < rows[:-1]).any()) and rows.unique().numel() < count
    gathered = store[rows.long()]
    if which == "A":
        inp.opA = gathered
    else:
        inp.opB = gathered.t().contiguous() if c.tb else gathered
    ref = R.reference(c, inp)
    idx = _index(rows, n_store - 1)
    d = Device(c, inp)
    bias = d.bias if c.bias else None
    S = Operand(store, 4)
    for ws_mode in ("full", "none"):
        out, ws = Output(c, inp.C0), Workspace(d.nbytes, ws_mode)
        rc = _rows_call(c, S, idx, d.B, None, bias, out, ws) if which == "A" else _rows_call(c, d.A, None, S, idx, bias, out, ws)
        assert rc == OK and ws.intact(), (form, ws_mode, rc)
        _compare(c, 2, out.result(), ref, (form, ws_mode))
    # the index on the operand that does not form the row tiles: refused, nothing written
    out, ws = Output(c, inp.C0, beta=0.0), Workspace(d.nbytes, "full")
    n_other = (c.N if c.tb else c.K) if which == "A" else (c.K if c.ta else c.M)
    other = _index(torch.zeros(n_other, dtype=torch.int32), 0)
    rc = _rows_call(c, d.A, None, d.B, other, bias, out, ws) if which == "A" else _rows_call(c, d.A, other, d.B, None, bias, out, ws)
    assert rc == UNSUPPORTED and out.untouched() and ws.written() == 0, (form, rc)
    # both indices NULL: isic_gemm_f32_ws
    o1, o2, w1, w2 = Output(c, inp.C0), Output(c, inp.C0), Workspace(d.nbytes, "full"), Workspace(d.nbytes, "full")
    assert _rows_call(c, d.A, None, d.B, None, bias, o1, w1) == OK
    assert _code("isic_gemm_f32_ws", *_gemm_args(c, d, o2, w2)) == OK
    r1, r2 = o1.result(), o2.result()
    assert torch.equal(r1.view(torch.int32), r2.view(torch.int32)) and w1.written() == w2.written()
    _compare(c, 2, r1, ref, (form, "no index"))


def test_workspace_bytes_are_the_largest_need_of_the_kernels_that_can_launch():
    """(that the size suffices is shown by every case above: the workspace is exactly this long, its guard stays intact and the
    pinned kernel's ordered partials are all there)"""
    cus = _cus()
    for c in R.CASES + [c for c, _ in R.ROWS_FORMS.values()]:
        got = _call("isic_gemm_f32_workspace_bytes", c.ta, c.tb, c.M, c.N, c.K)
        assert got == R.workspace_bytes(c.ta, c.tb, c.M, c.N, c.K, cus), c.id
