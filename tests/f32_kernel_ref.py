"""fp64 references, derived per-element bounds, input families and case lists for the fp32 MIL / graph kernels
(rowwise.hip, attn_pool.hip, gat.hip, edge_attn.hip, the SpMM and CSR build of graph.hip, the small entries of
gemm_f32.hip).  Plain torch on the CPU; shared by tests/test_f32_kernel_ref_cpu.py, which shows that the bounds admit a
correct fp32 evaluation and reject the deliberately wrong variants kept here, and tests/test_f32_kernel_domain_gpu.py,
which holds the kernels to the same bounds on the same case lists.

Every operation is one function `<family>_eval(inp, dtype, bug=None)`: in float64 it is the reference (backward values
from autograd of the forward restatement), in float32 it is "a correct fp32 evaluation", and `bug=` turns it into one of
the wrong variants.  Dropout masks come from oracle/philox.py with the element indices include/isic_hip.h documents.

Error model.  u = 2^-24 is the unit roundoff, one ulp is at most 2^-23 of its value.
  * An n-term fp32 sum of products, in ANY order (lane-strided partial sums, shuffle trees, atomics), is within
    (n + 1) u sum|terms| of exact to first order; the bounds use (n + c) u sum|terms| with the small c stated at each use
    (one per further rounding of a term).
  * Library functions: the ROCm device library (OCML) is specified to the OpenCL C numerical-compliance limits
    (OpenCL C 3.0 specification, section 7.4, "Relative error as ULPs"): exp <= 3 ulp, log <= 3 ulp, tanh <= 5 ulp,
    rsqrt <= 2 ulp, sqrt <= 3 ulp, x / y <= 2.5 ulp.  Those figures are used as they stand (EXP_ULP ...); hipcc's default
    correctly rounded division and square root are inside them.
  * A softmax over n scores whose absolute errors are at most es: every probability is within the RELATIVE error
        2 max(es) + u max|s - max s| + (n + 8) (2 EXP_ULP ulp + 3 u) + DIV
    (the common shift cancels, hence 2 max(es); the argument s - max is rounded once; per term one exponential and, in
    an online softmax, one rescaling of the running sum by another exponential, a multiplication and an addition:
    2 EXP_ULP ulp + 3 u, and as much for each of up to 8 merged waves; one division).
  * A result below 2^-126 is subnormal with spacing 2^-149 whatever its value: every bound has the floor 4 x 2^-149
    (a product of a subnormal probability and its normaliser rounds twice, and twice again through a backward pass).
  * Errors are propagated through products and sums with the product rule on the bounds (|a| eb + |b| ea + ea eb).
Nothing is fitted: no constant here was set from a kernel's output.  Where a derivation was found short on the device the
missing term is named next to the bound.

Ambiguous entries.  A ReLU mask recomputed in a backward pass depends on the sign of a value; where the fp64 value is
within its own forward bound of zero either sign is a correct fp32 answer.  Such entries (LayerNorm: the whole row,
whose dx depends on every mask of the row) are left out of the gradient comparison; the input builders resample rows
until the share left out is far below the 1 % cap, and both tests assert the cap.  The leaky-ReLU branch of GAT / GATv2
backward is taken on the sign of a sum of two fp32 INPUTS (al + ar, ks + qd): rounding cannot change the sign of a
non-zero sum, so only an exact zero is ambiguous.  relu-dropout's mask is the sign of an input: never ambiguous."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import philox  # noqa: E402

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
ULP = 2.0 ** -23
EXP_ULP, LOG_ULP, TANH_ULP, RSQRT_ULP, SQRT_ULP, DIV_ULP = 3.0, 3.0, 5.0, 2.0, 3.0, 2.5
EXPR, LOGR, TANHR, RSQRTR, SQRTR, DIV = (k * ULP for k in (EXP_ULP, LOG_ULP, TANH_ULP, RSQRT_ULP, SQRT_ULP, DIV_ULP))
INF = float("inf")
AMBIGUOUS_CAP = 0.01
SUBNORMAL_FLOOR = 4 * 2.0 ** -149
SEED = 1234


def fin(b):
    """a bound: NaN (inf * 0 while propagating an unbounded term) means unbounded"""
    return torch.nan_to_num(b.double(), nan=INF, posinf=INF)


def ratio(got, ref, bound, keep=None):
    """worst |got - ref| / bound over the compared elements (0 / 0 = 0, x / 0 = inf, x / inf = 0)"""
    got, ref, bound = got.detach().double(), ref.detach().double(), fin(bound) + SUBNORMAL_FLOOR
    bound = bound.expand_as(ref) if bound.shape != ref.shape else bound
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, INF), err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isinf(bound) & torch.isfinite(err), torch.zeros_like(r), r)
    if keep is not None:
        r = r[keep.expand_as(r)]
    return float(r.max()) if r.numel() else 0.0


def drop_scale(p):
    return float(philox.dropout_scale(p)) if p > 0 else 1.0


def drop_threshold(p):
    return philox.dropout_threshold(p) if p > 0 else 0


def keep_of(indices, p, seed, stream, clock=None):
    """keep flags (bool tensor, shape of `indices`) of the dropout elements `indices` (int64 tensor)"""
    if p <= 0:
        return torch.ones(indices.shape, dtype=torch.bool)
    if clock is not None:
        stream = stream + clock * 1024
    n = int(indices.max()) + 1 if indices.numel() else 0
    words = torch.from_numpy(philox.random_u32(n, seed, stream).astype(np.int64))
    return words[indices] >= drop_threshold(p)


def softmax_rel(es_max, spread, n):
    """relative error of a probability of an n-term softmax (module docstring)"""
    return 2.0 * es_max + U * spread + (n + 8) * (2 * EXPR + 3 * U) + DIV


def _gen(*key):
    return torch.Generator().manual_seed(SEED + sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


# ====================================================================================================== A. LayerNorm
# y = dropout(relu?(LN(x) gamma + beta)) + residual; dropout element index row * N + j; stream = stream_id + clock * 1024.
LN_EPS = 1e-5
LN_SEED, LN_STREAM = 77, 5
LN_BUGS = ("var_nm1", "drop_after_residual", "mask_from_y", "philox_shift", "dgamma_noscale")
LN_VEC_WIDTHS = (64, 128, 256)
LN_GENERIC_WIDTHS = (1, 3, 63, 65, 100, 129, 255, 257, 511, 513, 1000, 1024)
# the launch caps, read from isic_layernorm_fwd_clk / isic_layernorm_bwd_dxsum_ws (rpw = 256 / N rows per wave pass):
#   vector forward   gridv = ceil(M / (4 waves x rpw x 2 passes)), capped at 4096: binds for M > 4096 x 4 x rpw x 2
#   vector backward  gridv = ceil(M / (16 waves x rpw x 4 passes)), capped at 192: binds for M > 192 x 16 x rpw x 4
#   generic forward  grid = ceil(M / 4), capped at 4096:                           binds for M > 4096 x 4
#   generic backward grid = ceil(M / (4 waves x 8 rows)), capped at 1024:          binds for M > 1024 x 4 x 8
# the row counts below are just past the larger cap of each pair, so the stride loops of all four launches run extra passes
LN_M_PAST_VEC_CAP = 4096 * 4 * 1 * 2 + 5      # N = 256 (rpw = 1): forward cap 32768 rows, backward cap 12288
LN_M_PAST_GENERIC_CAP = 1024 * 4 * 8 + 5      # N = 3: backward cap 32768 rows, forward cap 16384
_LN_OPTS = ((1, 1, 0.25, 3), (0, 0, 0.0, None), (1, 0, 0.25, None), (0, 1, 0.0, 3), (1, 1, 0.0, None), (0, 1, 0.25, None))


def _ln_cases():
    cases, k = [], 0
    for N in LN_VEC_WIDTHS:
        for mis in (0, 1):
            for M in (67, 5, 1):
                relu, res, p, clock = _LN_OPTS[k % len(_LN_OPTS)]
                k += 1
                cases.append(dict(N=N, M=M, family="random", relu=relu, residual=res, p=p, clock=clock, misalign=mis))
    for N in LN_GENERIC_WIDTHS:
        for M in (67, 5, 1):
            relu, res, p, clock = _LN_OPTS[k % len(_LN_OPTS)]
            k += 1
            cases.append(dict(N=N, M=M, family="random", relu=relu, residual=res, p=p, clock=clock, misalign=0))
    for N, mis in ((64, 0), (256, 1), (100, 0), (1024, 0)):
        cases.append(dict(N=N, M=67, family="const", relu=1, residual=1, p=0.25, clock=None, misalign=mis))
        # (relu off: with a common offset of 1e4 the bound of the pre-activation is wider than the activations, every
        #  mask would be ambiguous)
        cases.append(dict(N=N, M=67, family="offset", relu=0, residual=1, p=0.25, clock=3, misalign=mis))
    cases.append(dict(N=256, M=LN_M_PAST_VEC_CAP, family="random", relu=1, residual=1, p=0.25, clock=3, misalign=0))
    cases.append(dict(N=3, M=LN_M_PAST_GENERIC_CAP, family="random", relu=1, residual=1, p=0.25, clock=None, misalign=0))
    for c in cases:
        c["id"] = "N{N}-M{M}-{family}-r{relu}{residual}-p{p}-c{clock}-o{misalign}".format(**c)
    return cases


LN_CASES = _ln_cases()


class Box(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def ln_inputs(case):
    N, M = case["N"], case["M"]
    g = _gen(N, M, case["relu"], case["residual"], len(case["family"]), case["misalign"])
    sign = lambda n: (torch.rand(n, generator=g) < 0.5).float() * 2 - 1      # noqa: E731
    inp = Box(case)
    inp.gamma = sign(N) * (0.5 + torch.rand(N, generator=g))
    inp.beta = sign(N) * (0.25 + 0.75 * torch.rand(N, generator=g))          # |beta| >= 0.25: constant rows stay decided

    def rows(m):
        if case["family"] == "const":
            return (torch.rand(m, 1, generator=g) * 2 - 1).expand(m, N).contiguous()
        x = torch.randn(m, N, generator=g)
        return x + 1e4 if case["family"] == "offset" else x
    inp.x = rows(M)
    inp.dy = torch.randn(M, N, generator=g)
    inp.res = torch.randn(M, N, generator=g) if case["residual"] else None
    inp.dgamma0 = torch.randn(N, generator=g)            # the accumulated outputs start from non-zero buffers
    inp.dbeta0 = torch.randn(N, generator=g)
    inp.dxsum0 = torch.randn(N, generator=g)
    idx = torch.arange(M * N, dtype=torch.int64).view(M, N)
    inp.keep = keep_of(idx, case["p"], LN_SEED, LN_STREAM, case["clock"])
    inp.keep_shift = keep_of(idx + 1, case["p"], LN_SEED, LN_STREAM, case["clock"])
    inp.scale = drop_scale(case["p"])
    if case["relu"] and case["family"] == "random":       # resample the rows that hold an ambiguous mask
        for _ in range(40):
            amb = ln_ambiguous(inp, ln_forward_bounds(inp, ln_eval(inp, F64, backward=False))).any(-1)
            if not bool(amb.any()):
                break
            inp.x[amb] = rows(int(amb.sum()))
    return inp


def ln_eval(inp, dtype, bug=None, backward=True):
    N, M = inp.N, inp.M
    x = inp.x.to(dtype).clone().requires_grad_(True)
    gamma = inp.gamma.to(dtype).clone().requires_grad_(True)
    beta = inp.beta.to(dtype).clone().requires_grad_(True)
    res = inp.res.to(dtype) if inp.res is not None else None
    dy = inp.dy.to(dtype)
    keep = (inp.keep_shift if bug == "philox_shift" else inp.keep)
    ks = keep.to(dtype) * torch.tensor(inp.scale, dtype=F32).to(dtype)
    mean = x.sum(-1, keepdim=True) / N
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / ((N - 1) if (bug == "var_nm1" and N > 1) else N)
    rstd = torch.rsqrt(var + LN_EPS)
    xh = d * rstd
    o = xh * gamma + beta
    a = torch.relu(o) if inp.relu else o
    if bug == "drop_after_residual" and res is not None:
        y = (a + res) * ks
    else:
        y = a * ks
        if res is not None:
            y = y + res
    out = Box(y=y.detach(), mean=mean.detach(), rstd=rstd.detach(), o=o.detach(), d=d.detach(), var=var.detach(),
              xh=xh.detach())
    if not backward:
        return out
    if dtype == F64 and bug is None:                      # the reference: autograd of the restatement
        y.backward(dy)
        out.dx, out.dgamma, out.dbeta = x.grad, gamma.grad, beta.grad
    else:                                                 # the documented backward arithmetic, from the saved mean / rstd
        with torch.no_grad():
            xh_, rs = out.xh, out.rstd
            gg = dy * ks
            if inp.relu:
                m = (out.y > 0) if bug == "mask_from_y" else (xh_ * gamma + beta > 0)
                gg = gg * m.to(dtype)
            ggw = dy * keep.to(dtype) * (m.to(dtype) if inp.relu else 1.0) if bug == "dgamma_noscale" else gg
            out.dgamma, out.dbeta = (ggw * xh_).sum(0), gg.sum(0)
            gv = gg * gamma
            s1 = gv.sum(-1, keepdim=True) / N
            s2 = (gv * xh_).sum(-1, keepdim=True) / N
            out.dx = rs * (gv - s1 - xh_ * s2)
    out.dgamma = out.dgamma.detach() + inp.dgamma0.to(dtype)
    out.dbeta = out.dbeta.detach() + inp.dbeta0.to(dtype)
    out.dxsum = out.dx.detach().sum(0) + inp.dxsum0.to(dtype)
    out.dx = out.dx.detach()
    return out


def ln_forward_bounds(inp, ref):
    """mean: an N-term sum and one division.  d = x - mean inherits the error of the mean (this is where a large common
    offset enters: em ~ N u |offset|).  var: sum of d^2 with d wrong by ed -- the SECOND-order term ed^2 is kept, for a
    constant row d == 0 and it is the whole error.  rstd = rsqrt(var + eps): the exact interval of the argument is mapped
    through rsqrt (first order is not enough when ev ~ var + eps), plus RSQRT_ULP ulp; an interval that reaches zero
    gives an unbounded rstd.  o = d rstd gamma + beta by the product rule, two multiplications and one addition; ReLU
    does not widen it; dropout multiplies by the scale (one rounding); the residual adds one rounding."""
    N = inp.N
    x = inp.x.double()
    gam, bet = inp.gamma.double().abs(), inp.beta.double()
    mean, d, var, rstd, o = ref.mean.double(), ref.d.double(), ref.var.double(), ref.rstd.double(), ref.o.double()
    em = N * U * x.abs().sum(-1, keepdim=True) / N + DIV * mean.abs()
    ed = em + U * d.abs()
    ev = ((2 * d.abs() * ed + ed * ed).sum(-1, keepdim=True) + (N + 2) * U * (d * d).sum(-1, keepdim=True)) / N + DIV * var
    a = var + LN_EPS
    ea = ev + U * a
    lo = torch.rsqrt(a + ea)
    hi = torch.where(a - ea > 0, torch.rsqrt((a - ea).clamp_min(1e-300)), torch.full_like(a, INF))
    er = torch.maximum(rstd - lo, hi - rstd) + RSQRTR * hi
    xh = d * rstd
    exh = fin(ed * (rstd + er) + d.abs() * er + U * xh.abs())
    eo = fin(exh * gam + 2 * U * (xh * gam).abs() + U * o.abs())
    act = torch.relu(o) if inp.relu else o
    ks = inp.keep.double() * inp.scale
    ey = ks * (eo + U * act.abs())
    if inp.res is not None:
        ey = ey + U * ref.y.double().abs()
    return Box(mean=fin(em), rstd=fin(er), y=fin(ey), o=eo, xh=exh, er=fin(er))


def ln_ambiguous(inp, fb):
    """[M][N] bool: the recomputed ReLU mask of the element may go either way"""
    if not inp.relu:
        return torch.zeros(inp.M, inp.N, dtype=torch.bool)
    o = ln_eval(inp, F64, backward=False).o
    return o.abs() <= fb.o


def ln_backward_bounds(inp, ref, fb):
    """The backward kernel recomputes xh = (x - mean) rstd from the SAVED fp32 mean / rstd (errors em, er: exh above),
    gg = dy scale mask (one rounding), g = gg gamma, s1 = sum g / N, s2 = sum g xh / N, dx = rstd (g - s1 - xh s2);
    dgamma = sum_rows gg xh, dbeta = sum_rows gg, dxsum = sum_rows dx, each M-term sums added to a non-zero buffer.
    An ambiguous mask adds its whole possible contribution |dy scale xh| (|dy scale|) to dgamma (dbeta) of its column
    and makes the dx sums of the columns unbounded (the inputs are built so that it does not happen)."""
    N, M = inp.N, inp.M
    gam = inp.gamma.double()
    xh, rstd = ref.xh.double(), ref.rstd.double()
    exh, er = fb.xh, fb.er
    ks = inp.keep.double() * inp.scale
    o = ref.o.double()
    mask = (o > 0).double() if inp.relu else torch.ones_like(o)
    gg = inp.dy.double() * ks * mask
    e_gg = U * gg.abs()
    g = gg * gam
    e_g = e_gg * gam.abs() + U * g.abs()
    s1 = g.sum(-1, keepdim=True) / N
    e_s1 = (e_g.sum(-1, keepdim=True) + N * U * g.abs().sum(-1, keepdim=True)) / N + DIV * s1.abs()
    s2 = (g * xh).sum(-1, keepdim=True) / N
    e_s2 = ((e_g * xh.abs() + g.abs() * exh + e_g * exh).sum(-1, keepdim=True)
            + (N + 1) * U * (g * xh).abs().sum(-1, keepdim=True)) / N + DIV * s2.abs()
    inner = g - s1 - xh * s2
    e_in = (e_g + e_s1 + exh * s2.abs() + xh.abs() * e_s2 + exh * e_s2
            + 3 * U * (g.abs() + s1.abs() + (xh * s2).abs()))
    dx = rstd * inner
    e_dx = fin(er * (inner.abs() + e_in) + rstd * e_in + U * dx.abs())
    amb = ln_ambiguous(inp, fb)
    open_ = amb.double() * (inp.dy.double() * ks).abs()
    e_dgamma = ((e_gg * xh.abs() + gg.abs() * exh + e_gg * exh + U * (gg * xh).abs()).sum(0)
                + M * U * (gg * xh).abs().sum(0) + (open_ * (xh.abs() + exh)).sum(0)
                + U * (inp.dgamma0.double().abs() + ref.dgamma.double().abs()))
    e_dbeta = (e_gg.sum(0) + M * U * gg.abs().sum(0) + open_.sum(0)
               + U * (inp.dbeta0.double().abs() + ref.dbeta.double().abs()))
    e_dxsum = (e_dx.sum(0) + M * U * dx.abs().sum(0) + U * (inp.dxsum0.double().abs() + ref.dxsum.double().abs()))
    if bool(amb.any()):
        e_dxsum = torch.full_like(e_dxsum, INF)
    return Box(dx=e_dx, dgamma=fin(e_dgamma), dbeta=fin(e_dbeta), dxsum=fin(e_dxsum), rows=~amb.any(-1, keepdim=True),
               share=float(amb.any(-1).double().mean()))


def ln_ratios(got, ref, fb, bb=None):
    r = {k: ratio(got[k], ref[k], fb[k]) for k in ("y", "mean", "rstd")}
    if bb is not None:
        r["dx"] = ratio(got["dx"], ref["dx"], bb.dx, keep=bb.rows)
        for k in ("dgamma", "dbeta"):
            r[k] = ratio(got[k], ref[k], bb[k])
        if got.get("dxsum") is not None:
            r["dxsum"] = ratio(got["dxsum"], ref["dxsum"], bb.dxsum)
    return r


# ====================================================================================================== graphs and CSR
def make_graph(n, in_degrees=(), hub_out=0, seed=0, weighted=True, extra=2.0):
    """Directed edges (src, dst, w) on n nodes: node i < len(in_degrees) receives exactly in_degrees[i] edges from distinct
    other sources, node len(in_degrees) sends to hub_out distinct other destinations, the remaining nodes receive about
    `extra` edges each; a few edges are duplicated and a few self loops are present (at most one per node)."""
    rng = np.random.RandomState(SEED + seed)
    src, dst = [], []
    k = len(in_degrees)
    for i, d in enumerate(in_degrees):
        others = np.setdiff1d(np.arange(n), [i])
        s = rng.choice(others, size=d, replace=False)
        src += list(s)
        dst += [i] * d
    if hub_out:
        others = np.arange(k + 1, n)
        t = rng.choice(others, size=hub_out, replace=False)
        src += [k] * hub_out
        dst += list(t)
    m = int(extra * max(n - k - 1, 0))
    if m and n - k - 1 > 1:
        src += list(rng.randint(0, n, size=m))
        dst += list(rng.randint(k + 1, n, size=m))
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    nd = min(5, m) if (m and n - k - 1 > 1) else 0          # duplicates (the last of the random edges again) and self loops
    if nd:
        src, dst = np.concatenate([src, src[-nd:]]), np.concatenate([dst, dst[-nd:]])
    loops = np.arange(k + 1, n, 7, dtype=np.int64)[:20]
    seen = set(zip(src.tolist(), dst.tolist()))
    loops = np.asarray([i for i in loops if (i, i) not in seen], dtype=np.int64)
    keep = src != dst                                       # random self loops out: at most one loop per node
    src, dst = np.concatenate([src[keep], loops]), np.concatenate([dst[keep], loops])
    order = rng.permutation(src.size)
    src, dst = src[order], dst[order]
    w = (0.5 + rng.rand(src.size)).astype(np.float32) if weighted else None
    return src, dst, w


def csr_ref(src, dst, w, n, mode):
    """The documented CSR of isic_gcn_csr_build in numpy / fp64: slots by destination (edges in edge order, the self loop
    of mode 0 last), the transposed structure by source, perm_t, and the per-slot relative bound of val."""
    E = src.size
    wv = np.ones(E) if w is None else w.astype(np.float64)
    eid = np.arange(E)
    if mode == 0:
        loopw = np.ones(n)
        is_loop = src == dst
        loopw[src[is_loop]] = wv[is_loop]
        keep = ~is_loop
        s = np.concatenate([src[keep], np.arange(n)])
        d = np.concatenate([dst[keep], np.arange(n)])
        ww = np.concatenate([wv[keep], loopw])
        ee = np.concatenate([eid[keep], E + np.arange(n)])
    else:
        s, d, ww, ee = src, dst, wv, eid
    by_d = np.lexsort((ee, d))
    by_s = np.lexsort((ee, s))
    cnt_in = np.bincount(d, minlength=n)
    cnt_out = np.bincount(s, minlength=n)
    rowptr = np.concatenate([[0], np.cumsum(cnt_in)])
    rowptr_t = np.concatenate([[0], np.cumsum(cnt_out)])
    if mode == 0:
        deg = np.bincount(d, weights=ww, minlength=n)
        dis = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
        val_e = dis[s] * ww * dis[d]
        # deg: cnt positive terms; deg^-1/2: a square root and a division; two factors and two multiplications
        rel_dis = 0.5 * cnt_in * U + SQRTR + DIV
        rel_e = rel_dis[s] + rel_dis[d] + 2 * U
    elif mode == 1:
        val_e, rel_e = ww, np.zeros(ww.size)
    else:
        val_e = ww / np.maximum(cnt_in[d], 1)
        rel_e = np.full(ww.size, DIV + U)                   # 1 / count, one multiplication
    slot_of = np.empty(s.size, dtype=np.int64)
    slot_of[by_d] = np.arange(s.size)
    g = Box(n=n, mode=mode, nnz=int(s.size), rowptr=rowptr, rowptr_t=rowptr_t,
            col=s[by_d], row=d[by_d], val=val_e[by_d], rel=rel_e[by_d],
            col_t=d[by_s], row_t=s[by_s], val_t=val_e[by_s], rel_t=rel_e[by_s], perm_t=slot_of[by_s],
            w_slot=ww[by_d], cnt_in=cnt_in, cnt_out=cnt_out)
    return g


# ====================================================================================================== D. SpMM
SPMM_BUGS = ("mean_by_out_degree",)
SPMM_ALPHA, SPMM_ADDEND_SCALE = 0.75, 0.1
SPMM_IN_DEGREES = (0, 1, 16, 17, 699, 700)


def _spmm_cases():
    cases, k = [], 0
    widths = [(F, 0) for F in (1, 3, 30, 127, 130, 258, 260, 512)] + [(128, 1), (256, 1)] + [(F, 0) for F in (64, 128, 256)]
    for F, off in widths:
        cases.append(dict(n=801, F=F, bias_offset=off, mode=k % 3, weighted=int(k % 2 == 0), transposed=int(k % 4 >= 2),
                          addend=int(k % 2 == 1), empty=0))
        k += 1
    for n in (1, 5):
        for F in (3, 64, 260):
            cases.append(dict(n=n, F=F, bias_offset=0, mode=k % 3, weighted=1, transposed=k % 2, addend=1, empty=0))
            k += 1
    for mode in (0, 1, 2):                                  # E == 0
        cases.append(dict(n=5, F=64, bias_offset=0, mode=mode, weighted=0, transposed=0, addend=0, empty=1))
    # the mean aggregation on the hub graph, forward and transposed, on the grouped kernel and on a fallback
    cases.append(dict(n=801, F=64, bias_offset=0, mode=2, weighted=1, transposed=0, addend=0, empty=0))
    cases.append(dict(n=801, F=30, bias_offset=0, mode=2, weighted=0, transposed=1, addend=0, empty=0))
    for c in cases:
        c["id"] = "n{n}-F{F}-o{bias_offset}-m{mode}-w{weighted}-t{transposed}-a{addend}-e{empty}".format(**c)
    return cases


SPMM_CASES = _spmm_cases()


def spmm_graph(case):
    n = case["n"]
    if case["empty"]:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), None
    if n == 801:
        return make_graph(n, SPMM_IN_DEGREES, hub_out=700, seed=1, weighted=bool(case["weighted"]))
    if n == 1:
        return np.zeros(1, np.int64), np.zeros(1, np.int64), np.asarray([0.8], np.float32)      # one self loop
    return make_graph(n, (0, 2), hub_out=0, seed=2, weighted=bool(case["weighted"]))


def spmm_inputs(case):
    n, F = case["n"], case["F"]
    g = _gen(n, F, case["mode"], case["transposed"])
    inp = Box(case)
    inp.src, inp.dst, inp.w = spmm_graph(case)
    inp.x = torch.randn(n, F, generator=g)
    inp.bias = torch.randn(F, generator=g)
    inp.addend_t = torch.randn(n, F, generator=g) if case["addend"] else None
    return inp


def spmm_eval(inp, dtype, bug=None, csr=None):
    """out = alpha A x + bias + addend_scale addend with A the dense operator of the documented CSR (A^T if transposed)"""
    n = inp.n
    g = csr or csr_ref(inp.src, inp.dst, inp.w, n, inp.mode)
    val = g.val
    if bug == "mean_by_out_degree" and inp.mode == 2:
        val = g.w_slot / np.maximum(g.cnt_out[g.col], 1)
    A = torch.zeros(n, n, dtype=F64)
    A.index_put_((torch.from_numpy(g.row), torch.from_numpy(g.col)), torch.from_numpy(val), accumulate=True)
    A = (A.t() if inp.transposed else A).to(dtype)
    out = torch.tensor(SPMM_ALPHA, dtype=dtype) * (A @ inp.x.to(dtype)) + inp.bias.to(dtype)
    if inp.addend_t is not None:
        out = out + torch.tensor(SPMM_ADDEND_SCALE, dtype=dtype) * inp.addend_t.to(dtype)
    return Box(out=out, csr=g)


def spmm_bounds(inp, ref):
    """a row of deg entries: deg products summed in any order, scaled by alpha, plus bias and the scaled addend: (deg + 4) u
    on the sum of the magnitudes; val itself is within rel (csr_ref) of the fp64 normalisation"""
    g = ref.csr
    n = inp.n
    Aabs = torch.zeros(n, n, dtype=F64)
    Arel = torch.zeros(n, n, dtype=F64)
    idx = (torch.from_numpy(g.row), torch.from_numpy(g.col))
    Aabs.index_put_(idx, torch.from_numpy(np.abs(g.val)), accumulate=True)
    Arel.index_put_(idx, torch.from_numpy(np.abs(g.val) * g.rel), accumulate=True)
    deg = torch.from_numpy(g.cnt_out if inp.transposed else g.cnt_in).double().view(-1, 1)
    if inp.transposed:
        Aabs, Arel = Aabs.t(), Arel.t()
    xa = inp.x.double().abs()
    mag = SPMM_ALPHA * (Aabs @ xa) + inp.bias.double().abs()
    if inp.addend_t is not None:
        mag = mag + SPMM_ADDEND_SCALE * inp.addend_t.double().abs()
    return Box(out=(deg + 4) * U * mag + SPMM_ALPHA * (Arel @ xa))


# ====================================================================================================== E. small row-wise entries
L2_EPS = float(np.float32(1e-12))        # the eps the kernel receives (a float argument)
L2_WIDTHS = (1, 63, 64, 65, 300)
L2_BUGS = ("clamped_as_unclamped",)


def l2_inputs(N):
    g = _gen(N, 11)
    x = torch.randn(9, N, generator=g)
    x[0] = 0.0                                   # a zero row
    x[1] *= 1e-14                                # norm below eps
    x[2] *= 1e6                                  # norm far above eps
    return Box(N=N, M=9, x=x, dy=torch.randn(9, N, generator=g))


def l2_eval(inp, dtype, bug=None):
    x = inp.x.to(dtype).clone().requires_grad_(True)
    dy = inp.dy.to(dtype)
    norm = torch.linalg.vector_norm(x, dim=-1, keepdim=True).clamp_min(L2_EPS)
    y = x / norm
    out = Box(y=y.detach(), norm=norm.detach().squeeze(-1))
    if dtype == F64 and bug is None:
        y.backward(dy)
        out.dx = x.grad
    else:
        with torch.no_grad():
            dot = (y * dy).sum(-1, keepdim=True)
            if bug != "clamped_as_unclamped":
                dot = torch.where(norm > L2_EPS, dot, torch.zeros_like(dot))
            out.dx = (dy - y * dot) / norm
    return out


def l2_bounds(inp, ref):
    """s = sum x^2: (N + 1) u s; the square root halves the relative error and adds SQRT_ULP ulp; y = x / n one division.
    A clamped row divides by eps itself (the inputs keep sqrt(s) far from eps).  Backward, from the saved fp32 y and n:
    dot = sum y dy, dx = (dy - y dot) / n by the product rule; a clamped row is dy / eps."""
    N = inp.N
    x, dy = inp.x.double(), inp.dy.double()
    n, y = ref.norm.double().view(-1, 1), ref.y.double()
    clamped = n <= L2_EPS
    rel_n = torch.where(clamped, torch.zeros_like(n), torch.full_like(n, 0.5 * (N + 1) * U + SQRTR))
    ey = y.abs() * (rel_n + DIV)
    dot = torch.where(clamped, torch.zeros_like(n), (y * dy).sum(-1, keepdim=True))
    e_dot = torch.where(clamped, torch.zeros_like(n),
                        (ey * dy.abs()).sum(-1, keepdim=True) + (N + 1) * U * (y * dy).abs().sum(-1, keepdim=True))
    e_dx = ((ey * dot.abs() + y.abs() * e_dot + ey * e_dot + 2 * U * (dy.abs() + (y * dot).abs())) / n
            + ref.dx.double().abs() * (rel_n + DIV))
    return Box(y=ey, norm=(n * rel_n).view(-1), dx=e_dx)


SOFTMAX_SHAPES = tuple((M, N) for M in (1, 257) for N in (1, 2, 7, 16, 100))


def softmax_inputs(M, N):
    g = _gen(M, N, 13)
    x = torch.randn(M, N, generator=g) * 2
    x[0::5] = 0.5                                # equal rows
    x[1::5] = x[1::5].clamp(-1.0, 1.0)           # a spread of 80 (to 82: exp(-82) is still a normal fp32)
    x[1::5, 0] += 80.0
    return Box(M=M, N=N, x=x, dp=torch.randn(M, N, generator=g))


def softmax_eval(inp, dtype, bug=None):
    x = inp.x.to(dtype).clone().requires_grad_(True)
    p = torch.softmax(x, dim=-1)
    p.backward(inp.dp.to(dtype))
    return Box(p=p.detach(), dx=x.grad)


def softmax_bounds(inp, ref):
    """forward: exact inputs, so the softmax bound with es = 0.  backward from the saved fp32 p (error ep):
    dot = sum p dp, dx = p (dp - dot)"""
    N = inp.N
    x, dp, p = inp.x.double(), inp.dp.double(), ref.p.double()
    spread = (x.max(-1, keepdim=True).values - x.min(-1, keepdim=True).values)
    ep = p * softmax_rel(0.0, spread, N)
    dot = (p * dp).sum(-1, keepdim=True)
    e_dot = (ep * dp.abs()).sum(-1, keepdim=True) + (N + 1) * U * (p * dp).abs().sum(-1, keepdim=True)
    e_dx = ep * (dp - dot).abs() + (p + ep) * (e_dot + U * (dp.abs() + dot.abs())) + U * ref.dx.double().abs()
    return Box(p=ep, dx=e_dx)


CE_SHAPES = ((1, 1), (1, 7), (255, 2), (256, 7), (257, 15), (1000, 7), (1000, 1), (255, 15))
CE_GRAD_SCALE = 0.37
CE_TINY = float(np.float32(1e-9))                # the kernel's 1e-9f
CE_BUGS = ("no_tiny", "no_mean_in_grad")


def ce_inputs(B, C, mode):
    g = _gen(B, C, mode, 17)
    z = torch.randn(B, C, generator=g) * 3
    labels = torch.randint(0, C, (B,), generator=g)
    if mode == 1:
        z = torch.softmax(z, dim=-1)
        z[0::4][torch.arange(z[0::4].shape[0]), labels[0::4]] = 0.0 if C > 1 else 1.0   # an exact 0 at the label
    return Box(B=B, C=C, mode=mode, x=z.float(), labels=labels)


def ce_eval(inp, dtype, bug=None):
    x = inp.x.to(dtype).clone().requires_grad_(True)
    B = inp.B
    q = torch.log(x + (0.0 if bug == "no_tiny" else torch.tensor(CE_TINY, dtype=dtype))) if inp.mode else x
    lse = torch.logsumexp(q, dim=-1)
    loss = lse - q[torch.arange(B), inp.labels]
    mean = loss.sum() / B
    (mean * CE_GRAD_SCALE * (B if bug == "no_mean_in_grad" else 1)).backward()
    return Box(loss=loss.detach(), mean=mean.detach().view(1), d_in=x.grad, q=q.detach(), lse=lse.detach())


def ce_bounds(inp, ref):
    """q = log(p + 1e-9f) (mode 1): the addition rounds once, so eq = u + LOG_ULP ulp |q|; mode 0: eq = 0.
    se = sum exp(q - max): relative 2 max eq + u spread + EXP_ULP ulp + C u.  lse = max + log se: e_lse = rel_se +
    LOG_ULP ulp |log se| + u |lse|.  loss = lse - q_y.  mean: a B-term sum and a division.
    gradient = (exp(q - lse) - onehot) grad_scale / B (/ (p + 1e-9f) in mode 1): the exponent's argument carries eq + e_lse
    + u |q - lse|, the factor grad_scale / B one division"""
    B, C = inp.B, inp.C
    q, lse, loss = ref.q.double(), ref.lse.double().view(-1, 1), ref.loss.double()
    eq = (U + LOGR * q.abs()) if inp.mode else torch.zeros_like(q)
    mx = q.max(-1, keepdim=True).values
    spread = mx - q.min(-1, keepdim=True).values
    eqm = eq.max(-1, keepdim=True).values
    rel_se = 2 * eqm + U * spread + EXPR + C * U
    e_lse = rel_se + LOGR * (lse - mx).abs() + U * lse.abs()
    eqy = eq[torch.arange(B), inp.labels]
    e_loss = e_lse.view(-1) + eqy + U * loss.abs()
    e_mean = (e_loss.sum() + B * U * loss.abs().sum()) / B + DIV * ref.mean.double().abs()
    sm = torch.exp(q - lse)
    onehot = torch.zeros_like(q)
    onehot[torch.arange(B), inp.labels] = 1.0
    gs = CE_GRAD_SCALE / B
    e_sm = sm * (eq + e_lse + U * (q - lse).abs() + EXPR)
    e_d = (e_sm + U * (sm - onehot).abs()) * gs + (U + DIV) * (sm - onehot).abs() * gs
    if inp.mode:
        den = inp.x.double() + CE_TINY
        e_d = e_d / den + (U + DIV) * ref.d_in.double().abs()
    return Box(loss=e_loss, mean=e_mean.view(1), d_in=e_d)


RD_SIZES = (1, 3, 4, 1023, 1025)
RD_SEED, RD_STREAM, RD_CLOCK, RD_P = 91, 9, 2, 0.3


def rd_inputs(n, p, clock):
    g = _gen(n, 19, int(p * 10))
    idx = torch.arange(n, dtype=torch.int64)
    return Box(n=n, p=p, clock=clock, x=torch.randn(n, generator=g), dy=torch.randn(n, generator=g),
               keep=keep_of(idx, p, RD_SEED, RD_STREAM, clock), scale=drop_scale(p))


def rd_eval(inp, dtype, bug=None):
    ks = inp.keep.to(dtype) * torch.tensor(inp.scale, dtype=F32).to(dtype)
    x = inp.x.to(dtype)
    y = torch.relu(x) * ks
    return Box(y=y, dx=inp.dy.to(dtype) * ks * (x > 0).to(dtype))


def rd_bounds(inp, ref):
    """one multiplication each"""
    return Box(y=U * ref.y.double().abs(), dx=U * ref.dx.double().abs())


def tanh_bwd_bounds(dy, t, ref):
    """1 - t t: the product and the difference round once each (absolute 2 u, t^2 <= 1), then one multiplication"""
    return 2 * U * dy.double().abs() + U * ref.double().abs()


COLSUM_SHAPES = ((1, 1, 1), (1, 130, 130), (70000, 3, 4), (513, 200, 256), (2048, 128, 128))


def colsum_inputs(M, N, ldx):
    g = _gen(M, N, ldx)
    return Box(M=M, N=N, ldx=ldx, X=torch.randn(M, ldx, generator=g), out0=torch.randn(N, generator=g))


def colsum_eval(inp, dtype, beta):
    return inp.X[:, :inp.N].to(dtype).sum(0) + beta * inp.out0.to(dtype)


def colsum_bounds(inp, ref, beta):
    """an M-term sum in any order (chunks, atomics), beta out0 and the final addition"""
    return (inp.M + 1) * U * inp.X[:, :inp.N].double().abs().sum(0) + 2 * U * (beta * inp.out0.double().abs() + ref.double().abs())


# ====================================================================================================== B. attention pool
POOL_BAGS = (1, 2, 7, 8, 9, 15, 0, 16, 17, 63, 64, 65, 196, 513, 0)     # an empty bag in the middle and an empty last bag
POOL_MAX_BAG = 513
POOL_BUGS = ("no_head_mean", "batch_softmax")


def _pool_cases():
    cases = []

    def add(H, A, heads, C, family="random", bags=POOL_BAGS, arm=""):
        cases.append(dict(H=H, A=A, heads=heads, C=C, family=family, bags=bags, arm=arm, accumulate_dh=len(cases) % 2))
    for H, A, heads in ((64, 32, 4), (128, 128, 4), (1, 1, 1)):                # GraphMIL form: z only
        add(H, A, heads, 0, arm="fwd2 / bwd<true>")
    for H, A, C in ((65, 64, 1), (128, 128, 2), (65, 128, 7), (128, 64, 16)):   # teacher form
        add(H, A, 1, C, arm="fwd<2,2> / bwd<true>")
    for i, (H, A) in enumerate(((128, 129), (129, 64), (256, 200), (257, 64), (512, 64), (513, 64), (1024, 64))):
        arm = "fwd<%s,0> / bwd<false>" % (2 if H <= 128 else 4 if H <= 256 else 8 if H <= 512 else 16)
        add(H, A, 1 if i % 2 == 0 else 3, 7 if i % 2 == 0 else 0, arm=arm)
    add(1024, 64, 1, 16, arm="fwd<16,0> / bwd<false>")
    add(64, 32, 6, 0, arm="fwd<2,2> x 2 launches, z accumulated; bwd UNSUPPORTED")
    for family in ("equal", "saturated"):
        add(64, 32, 4, 0, family=family, arm="fwd2 / bwd<true>")
        add(128, 128, 1, 7, family=family, arm="fwd<2,2> / bwd<true>")
        add(257, 64, 3, 0, family=family, arm="fwd<8,0> / bwd<false>")
    add(64, 32, 4, 0, bags=(9,), arm="fwd2 / bwd<true>, B = 1")
    add(129, 64, 1, 7, bags=(1,), arm="fwd<4,0> / bwd<false>, B = 1")
    for c in cases:
        c["id"] = "H{H}-A{A}-h{heads}-C{C}-{family}-B{nb}-acc{accumulate_dh}".format(nb=len(c["bags"]), **c)
    return cases


POOL_CASES = _pool_cases()


def pool_inputs(case):
    H, A, heads, C = case["H"], case["A"], case["heads"], case["C"]
    g = _gen(H, A, heads, C, len(case["family"]), len(case["bags"]))
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(case["bags"])]), dtype=torch.int64)
    T = int(offsets[-1])
    inp = Box(case)
    inp.offsets, inp.T, inp.B = offsets, T, len(case["bags"])
    inp.h = torch.randn(T, H, generator=g)
    inp.t = torch.tanh(torch.randn(T, heads * A, generator=g))
    inp.w3 = torch.randn(heads, A, generator=g) / math.sqrt(A)
    inp.b3 = torch.randn(heads, generator=g)
    if case["family"] == "equal":                         # every score of a bag equal
        inp.t = inp.t[:1].expand(T, heads * A).contiguous()
    elif case["family"] == "saturated":                   # one instance of every bag 80 above the rest
        inp.t = inp.t * 0.01
        inp.w3 = inp.w3 * (80.0 / 0.99) / inp.w3.abs().sum(-1, keepdim=True)
        first = offsets[:-1][offsets[1:] > offsets[:-1]]
        inp.t[first] = (0.99 * torch.sign(inp.w3)).reshape(1, -1)
    inp.W4 = torch.randn(C, H, generator=g) / math.sqrt(H) if C else None
    inp.b4 = torch.randn(C, generator=g) if C else None
    inp.dz = torch.randn(inp.B, H, generator=g)
    inp.dL = torch.randn(inp.B, C, generator=g) if C else None
    inp.dh0 = torch.randn(T, H, generator=g)              # d_h accumulates into it when accumulate_dh
    return inp


def _segments(offsets):
    return [(int(offsets[b]), int(offsets[b + 1])) for b in range(offsets.numel() - 1)]


def pool_eval(inp, dtype, bug=None, backward=True):
    H, A, heads, C, T, B = inp.H, inp.A, inp.heads, inp.C, inp.T, inp.B
    h = inp.h.to(dtype).clone().requires_grad_(True)
    t = inp.t.to(dtype).clone().requires_grad_(True)
    w3, b3 = inp.w3.to(dtype), inp.b3.to(dtype)
    s = (t.view(T, heads, A) * w3.view(1, heads, A)).sum(-1) + b3
    s.retain_grad()
    if bug == "batch_softmax":
        att = torch.softmax(s, dim=0)
    else:
        att = torch.cat([torch.softmax(s[lo:hi], dim=0) for lo, hi in _segments(inp.offsets)], dim=0)
    zs = []
    for lo, hi in _segments(inp.offsets):
        zk = (att[lo:hi].unsqueeze(-1) * h[lo:hi].unsqueeze(1)).sum(0)          # [heads][H]
        zs.append(zk.sum(0) if bug == "no_head_mean" else zk.sum(0) / heads)
    z = torch.stack(zs)
    out = Box(att=att.detach(), z=z.detach(), s=s.detach())
    loss = (z * inp.dz.to(dtype)).sum()
    if C:
        P = h @ inp.W4.to(dtype).t() + inp.b4.to(dtype)
        P.retain_grad()
        bl = torch.stack([(att[lo:hi, :1] * P[lo:hi]).sum(0) for lo, hi in _segments(inp.offsets)])
        out.update(P=P.detach(), pp=torch.softmax(P, -1).detach(), bl=bl.detach(), bp=torch.softmax(bl, -1).detach())
        loss = loss + (bl * inp.dL.to(dtype)).sum()
    if not backward:
        return out
    loss.backward()
    out.d_h = h.grad + (inp.dh0.to(dtype) if inp.accumulate_dh else 0.0)
    out.d_s = s.grad if s.grad is not None else torch.zeros_like(s)
    out.d_u = (t.grad if t.grad is not None else torch.zeros_like(t)) * (1 - t.detach() ** 2)
    if C:
        out.d_P = P.grad
    ds_t = (out.d_s.unsqueeze(-1) * t.detach().view(T, heads, A)).reshape(T, heads * A)
    out.psum = torch.stack([torch.cat([out.d_u[lo:hi].sum(0), ds_t[lo:hi].sum(0), out.d_s[lo:hi].sum(0)])
                            for lo, hi in _segments(inp.offsets)])
    return out


def pool_bounds(inp, ref):
    """s: an A-term dot product plus b3.  att: the softmax bound over the bag with es = the scores' bound.
    z = mean_k sum_n att h: the relative error of att on every term, an nb-term sum (+ 4: the rescalings / merge factors
    multiply the terms), the mean and, for heads > 4, the accumulation of the second launch.
    P = W4 h + b4: an H-term dot product; patch_probs / bag_probs: softmax bounds over the classes.
    bag_logits = sum_n att P.
    Backward, from the saved fp32 att and P (their forward bounds): da = dL . P + dz . h / heads, dot = sum_n att da,
    ds = att (da - dot), d_u = ds w3 (1 - t^2) (1 - t^2 absolute 2 u), d_P = att dL, d_h = mean_k att dz + W4^T d_P
    (+ the accumulated buffer); param_sums: nb-term sums of d_u, ds t and ds."""
    H, A, heads, C, T = inp.H, inp.A, inp.heads, inp.C, inp.T
    h, t = inp.h.double(), inp.t.double()
    w3 = inp.w3.double()
    tw = (t.view(T, heads, A) * w3.view(1, heads, A)).abs().sum(-1)
    s, att = ref.s.double(), ref.att.double()
    es = (A + 2) * U * (tw + inp.b3.double().abs()) + U * s.abs()
    rel = torch.zeros_like(s)
    nbv = torch.zeros(T, 1, dtype=F64)
    for lo, hi in _segments(inp.offsets):
        if hi > lo:
            sp = s[lo:hi].max(0).values - s[lo:hi].min(0).values
            rel[lo:hi] = softmax_rel(es[lo:hi].max(0).values, sp, hi - lo)
            nbv[lo:hi] = hi - lo
    eatt = att * rel
    b = Box(att=eatt)
    ha = h.abs()
    ez = []
    for lo, hi in _segments(inp.offsets):
        nb = hi - lo
        term = ((eatt[lo:hi] + (nb + 4) * U * att[lo:hi]).unsqueeze(-1) * ha[lo:hi].unsqueeze(1)).sum(0).sum(0) / heads
        ez.append(term)
    b.z = torch.stack(ez) + 3 * U * ref.z.double().abs()
    dz = inp.dz.double()
    # backward
    e_da = torch.zeros_like(s)
    da = torch.zeros_like(s)
    for bi, (lo, hi) in enumerate(_segments(inp.offsets)):
        base = (h[lo:hi] * dz[bi]).sum(-1, keepdim=True) / heads
        da[lo:hi] = base
        e_da[lo:hi] = (H + 2) * U * (ha[lo:hi] * dz[bi].abs()).sum(-1, keepdim=True) / heads + 2 * U * base.abs()
    if C:
        W4, P = inp.W4.double(), ref.P.double()
        eP = (H + 2) * U * (ha @ W4.abs().t() + inp.b4.double().abs()) + U * P.abs()
        spP = P.max(-1, keepdim=True).values - P.min(-1, keepdim=True).values
        b.P = eP
        b.pp = ref.pp.double() * softmax_rel(eP.max(-1, keepdim=True).values, spP, C)
        dL = inp.dL.double()
        ebl, cls, e_cls = [], torch.zeros(T, 1, dtype=F64), torch.zeros(T, 1, dtype=F64)
        for bi, (lo, hi) in enumerate(_segments(inp.offsets)):
            nb = hi - lo
            a0, ea0 = att[lo:hi, :1], eatt[lo:hi, :1]
            ebl.append((ea0 * P[lo:hi].abs() + a0 * eP[lo:hi] + ea0 * eP[lo:hi] + (nb + 4) * U * (a0 * P[lo:hi]).abs()).sum(0))
            cls[lo:hi] = (P[lo:hi] * dL[bi]).sum(-1, keepdim=True)
            e_cls[lo:hi] = ((eP[lo:hi] * dL[bi].abs()).sum(-1, keepdim=True)
                            + (C + 1) * U * (P[lo:hi] * dL[bi]).abs().sum(-1, keepdim=True))
        b.bl = torch.stack(ebl) + U * ref.bl.double().abs()
        bl = ref.bl.double()
        spb = bl.max(-1, keepdim=True).values - bl.min(-1, keepdim=True).values
        b.bp = ref.bp.double() * softmax_rel(b.bl.max(-1, keepdim=True).values, spb, C)
        da = da.clone()
        da[:, :1] = da[:, :1] + cls
        e_da = e_da.clone()
        e_da[:, :1] = e_da[:, :1] + e_cls + U * da[:, :1].abs()
    dot, e_dot = torch.zeros_like(s), torch.zeros_like(s)
    for lo, hi in _segments(inp.offsets):
        nb = hi - lo
        dot[lo:hi] = (att[lo:hi] * da[lo:hi]).sum(0, keepdim=True)
        e_dot[lo:hi] = ((eatt[lo:hi] * da[lo:hi].abs() + att[lo:hi] * e_da[lo:hi] + eatt[lo:hi] * e_da[lo:hi]).sum(0, keepdim=True)
                        + (nb + 2) * U * (att[lo:hi] * da[lo:hi]).abs().sum(0, keepdim=True))
    ds = att * (da - dot)
    e_ds = (eatt * (da - dot).abs() + (att + eatt) * (e_da + e_dot + U * (da.abs() + dot.abs())) + U * ds.abs())
    b.d_s = e_ds
    om = (1 - t * t).view(T, heads, A)
    w3v = w3.view(1, heads, A).abs()
    du_abs = ds.abs().unsqueeze(-1) * w3v
    e_du = (e_ds.unsqueeze(-1) * w3v * (om + 2 * U) + du_abs * 2 * U + 3 * U * du_abs * om)
    b.d_u = e_du.reshape(T, heads * A)
    e_dh = ((eatt.sum(-1, keepdim=True) + (heads + 2) * U * att.sum(-1, keepdim=True)) / heads) * dz.abs()[_bag_of(inp)]
    if C:
        dLr = dL[_bag_of(inp)]
        b.d_P = eatt[:, :1] * dLr.abs() + U * ref.d_P.double().abs()
        e_dh = e_dh + ((eatt[:, :1] * dLr.abs()) @ W4.abs() + (C + 3) * U * ((att[:, :1] * dLr.abs()) @ W4.abs()))
    e_dh = e_dh + 2 * U * ref.d_h.double().abs() + (U * inp.dh0.double().abs() if inp.accumulate_dh else 0.0)
    b.d_h = e_dh
    tv = t.view(T, heads, A).abs()
    e_dst = (e_ds.unsqueeze(-1) * tv + U * ds.abs().unsqueeze(-1) * tv).reshape(T, heads * A)
    rows = torch.cat([b.d_u, e_dst, e_ds], dim=1)
    mags = torch.cat([ref.d_u.double().abs(), (ds.abs().unsqueeze(-1) * tv).reshape(T, heads * A), ds.abs()], dim=1)
    b.psum = torch.stack([rows[lo:hi].sum(0) + (hi - lo) * U * mags[lo:hi].sum(0) for lo, hi in _segments(inp.offsets)])
    return b


def _bag_of(inp):
    lens = inp.offsets[1:] - inp.offsets[:-1]
    return torch.repeat_interleave(torch.arange(inp.B), lens)


POOL_FWD_KEYS = ("att", "z", "P", "pp", "bl", "bp")
POOL_BWD_KEYS = ("d_h", "d_s", "d_u", "d_P", "psum")


def pool_ratios(got, ref, b, keys):
    return {k: ratio(got[k], ref[k], b[k]) for k in keys if k in ref and got.get(k) is not None}


# ====================================================================================================== C. GAT, GATv2 / TransformerConv, FAConv
# Slots are the destination-major CSR slots (csr_ref): row = destination, col = source.  Dropout element slot * H + h
# (FA: slot).  The softmax layers share one restatement, `layer` in {"gat", "gatv2", "dot"}.
ATT_SEED, ATT_STREAM, ATT_P = 55, 3, 0.3
ATT_SLOPE = 0.2
FA_EPS = 0.1
# raw in-degrees of nodes 0..8; the 'gcn' CSR adds the self loop: {1, 2, 63, 64, 65, 512, 513, 514, 700}, the 'sum' CSR of
# TransformerConv keeps {0, 1, 62, 63, 64, 511, 512, 513, 699}: both cross the 512 edges the kernels keep in LDS; node 9
# sends 699 edges (700 with its loop): the transposed sweep's long row
ATT_IN_DEGREES = (0, 1, 62, 63, 64, 511, 512, 513, 699)
ATT_N = 1100
GAT_HF = ((1, 1), (3, 16), (4, 63), (4, 64), (2, 65), (8, 130))
EA_HF = GAT_HF + ((4, 256), (8, 128), (4, 257))
FA_F = (1, 63, 64, 65, 130, 260)
ATT_BUGS = ("softmax_outgoing", "philox_transposed", "philox_shift", "bwd_no_drop_scale", "slope_wrong_branch", "no_self_loop")


def _att_cases():
    cases = []
    for layer, shapes in (("gat", GAT_HF), ("gatv2", EA_HF), ("dot", EA_HF), ("fa", tuple((1, F) for F in FA_F))):
        for H, F in shapes:
            for p in (0.0, ATT_P):
                cases.append(dict(layer=layer, n=ATT_N, H=H, F=F, p=p))
        for n in (1, 5):
            cases.append(dict(layer=layer, n=n, H=3 if layer != "fa" else 1, F=16 if layer != "fa" else 63, p=ATT_P))
    for c in cases:
        c["id"] = "{layer}-n{n}-H{H}-F{F}-p{p}".format(**c)
    return cases


ATT_CASES = _att_cases()


def att_graph(n):
    if n == ATT_N:
        return make_graph(n, ATT_IN_DEGREES, hub_out=699, seed=3, weighted=True)
    if n == 1:
        return np.zeros(1, np.int64), np.zeros(1, np.int64), np.asarray([0.8], np.float32)
    return make_graph(n, (0, 2), hub_out=0, seed=4, weighted=True)


def att_csr_mode(layer):
    return 1 if layer == "dot" else 0


def att_inputs(case):
    layer, n, H, F = case["layer"], case["n"], case["H"], case["F"]
    g = _gen(n, H, F, len(layer), int(case["p"] * 10))
    inp = Box(case)
    inp.src, inp.dst, inp.w = att_graph(n)
    inp.csr = csr_ref(inp.src, inp.dst, inp.w, n, att_csr_mode(layer))
    inp.val = torch.from_numpy(inp.csr.val).float()          # FA: the fp32 normalisation (the device test puts the kernel's here)
    inp.dout = torch.randn(n, H, F, generator=g)
    inp.bias = torch.randn(H * F, generator=g)
    inp.scale = drop_scale(case["p"])
    sc = 1.0 / math.sqrt(F)
    if layer in ("gat", "fa"):
        inp.xp = torch.randn(n, H, F, generator=g)
        inp.att_src = torch.randn(H, F, generator=g) * sc
        inp.att_dst = torch.randn(H, F, generator=g) * sc
        inp.x0 = torch.randn(n, H, F, generator=g)
        sref = att_scores(inp, F64)
        inp.al, inp.ar = sref.al.float(), sref.ar.float()    # (the device test puts the kernel's scores here)
    else:
        inp.ks = torch.randn(n, H, F, generator=g)
        inp.qd = torch.randn(n, H, F, generator=g)
        inp.v = torch.randn(n, H, F, generator=g) if layer == "dot" else inp.ks
        inp.att = torch.randn(H, F, generator=g) * sc
        inp.dot_scale = float(np.float32(sc))
        if layer == "gatv2":                                 # no leaky-ReLU argument exactly zero (the ambiguous branch)
            row, col = torch.from_numpy(inp.csr.row), torch.from_numpy(inp.csr.col)
            for _ in range(8):
                zero = (inp.ks[col] + inp.qd[row] == 0).nonzero()
                if zero.shape[0] == 0:
                    break
                inp.qd[row[zero[:, 0]], zero[:, 1], zero[:, 2]] += 0.25
    return inp


def att_scores(inp, dtype):
    xp = inp.xp.to(dtype)
    return Box(al=(xp * inp.att_src.to(dtype)).sum(-1), ar=(xp * inp.att_dst.to(dtype)).sum(-1))


def att_scores_bounds(inp):
    """an F-term dot product"""
    xa, F = inp.xp.double().abs(), inp.F
    return Box(al=(F + 1) * U * (xa * inp.att_src.double().abs()).sum(-1), ar=(F + 1) * U * (xa * inp.att_dst.double().abs()).sum(-1))


def _lrelu(v, slope, swapped_backward=False):
    pos = torch.relu(v)
    neg = v - pos
    f = pos + slope * neg
    if swapped_backward:
        g = slope * pos + neg
        return f.detach() + (g - g.detach())
    return f


def _seg_softmax(l, seg, n):
    H = l.shape[1]
    idx = seg.view(-1, 1).expand(-1, H)
    mx = torch.full((n, H), -INF, dtype=l.dtype).scatter_reduce(0, idx, l.detach(), "amax")
    ex = torch.exp(l - mx[seg])
    den = torch.zeros(n, H, dtype=l.dtype).index_add_(0, seg, ex)
    return ex / den[seg]


def att_eval(inp, dtype, bug=None):
    layer, n, H, F = inp.layer, inp.n, inp.H, inp.F
    g = inp.csr
    if bug == "no_self_loop":
        keep = inp.src != inp.dst
        g = csr_ref(inp.src[keep], inp.dst[keep], None if inp.w is None else inp.w[keep], n, 1)
    row, col = torch.from_numpy(g.row), torch.from_numpy(g.col)
    nnz = g.nnz
    slot = torch.arange(nnz, dtype=torch.int64)
    Hd = 1 if layer == "fa" else H
    didx = slot.view(-1, 1) * Hd + torch.arange(Hd).view(1, -1)
    if bug == "philox_transposed":
        didx = torch.arange(Hd).view(1, -1) * nnz + slot.view(-1, 1)
    if bug == "philox_shift":                               # the word of the next element (for FA: of the next slot)
        didx = didx + 1
    keep = keep_of(didx, inp.p, ATT_SEED, ATT_STREAM).to(dtype)
    scale = torch.tensor(inp.scale, dtype=F32).to(dtype)

    def drop(a):
        ak = a * keep
        if bug == "bwd_no_drop_scale":
            return ak + (ak * (scale - 1)).detach()
        return ak * scale
    swapped = bug == "slope_wrong_branch"
    dout = inp.dout.to(dtype)
    out = Box()
    if layer in ("gat", "fa"):
        xp = inp.xp.to(dtype).clone().requires_grad_(True)
        al = inp.al.to(dtype).clone().requires_grad_(True)
        ar = inp.ar.to(dtype).clone().requires_grad_(True)
        pre = al[col] + ar[row]                                         # [nnz][H]
        pre.retain_grad()
        if layer == "gat":
            alpha = _seg_softmax(_lrelu(pre, ATT_SLOPE, swapped), col if bug == "softmax_outgoing" else row, n)
            o = torch.zeros(n, H, F, dtype=dtype).index_add_(0, row, drop(alpha).unsqueeze(-1) * xp[col])
            o = o + inp.bias.to(dtype).view(1, H, F)
            out.alpha = alpha.detach()
        else:
            coef = torch.tanh(pre)
            val = (inp.val if bug != "no_self_loop" else torch.from_numpy(g.val).float()).to(dtype).view(-1, 1)
            o = torch.zeros(n, H, F, dtype=dtype).index_add_(0, row, (drop(coef) * val).unsqueeze(-1) * xp[col])
            o = o + torch.tensor(FA_EPS, dtype=F32).to(dtype) * inp.x0.to(dtype)
            out.coef = coef.detach()
        o.backward(dout)
        out.out, out.de, out.dal, out.dar = o.detach(), pre.grad, al.grad, ar.grad
        out.dxp = (xp.grad + al.grad.unsqueeze(-1) * inp.att_src.to(dtype) + ar.grad.unsqueeze(-1) * inp.att_dst.to(dtype))
        return out
    ks = inp.ks.to(dtype).clone().requires_grad_(True)
    qd = inp.qd.to(dtype).clone().requires_grad_(True)
    v = ks if layer == "gatv2" else inp.v.to(dtype).clone().requires_grad_(True)
    att = inp.att.to(dtype).clone().requires_grad_(True)
    if layer == "gatv2":
        l = (att.view(1, H, F) * _lrelu(ks[col] + qd[row], ATT_SLOPE, swapped)).sum(-1)
    else:
        l = (qd[row] * ks[col]).sum(-1) * torch.tensor(inp.dot_scale, dtype=dtype)
    l.retain_grad()
    alpha = _seg_softmax(l, col if bug == "softmax_outgoing" else row, n)
    o = torch.zeros(n, H, F, dtype=dtype).index_add_(0, row, drop(alpha).unsqueeze(-1) * v[col])
    o = o + inp.bias.to(dtype).view(1, H, F)
    o.backward(dout)
    zero = torch.zeros(n, H, F, dtype=dtype)
    out.alpha, out.out, out.de = alpha.detach(), o.detach(), (l.grad if l.grad is not None else torch.zeros_like(l))
    out.dqd = qd.grad if qd.grad is not None else zero
    out.dks = ks.grad if ks.grad is not None else zero
    if layer == "dot":
        out.dv = v.grad if v.grad is not None else zero
    else:
        out.datt = att.grad if att.grad is not None else torch.zeros(H, F, dtype=dtype)
    return out


def att_zero_pre_share(inp):
    """share of the leaky-ReLU arguments that are exactly zero (the only ambiguous branch: module docstring)"""
    g = inp.csr
    row, col = torch.from_numpy(g.row), torch.from_numpy(g.col)
    if inp.layer == "gat":
        pre = inp.al.double()[col] + inp.ar.double()[row]
    elif inp.layer == "gatv2":
        pre = inp.ks.double()[col] + inp.qd.double()[row]
    else:
        return 0.0
    return float((pre == 0).double().mean()) if pre.numel() else 0.0


def att_bounds(inp, ref):
    """logit: gat = leaky_relu(al + ar) of fp32 inputs: the sum and the slope round once each (2 u |l|); gatv2 = an F-term
    sum of att leaky_relu(ks + qd) ((F + 3) u on the magnitudes); dot = scale <q, k> ((F + 2) u); fa: coef = tanh(al + ar),
    |tanh a - tanh b| <= |a - b| gives u |pre| + TANH_ULP ulp |coef|.
    alpha: the softmax bound over the row.  out = sum alpha_d v (+ bias): the error of alpha on every term and a
    (deg + 4) u sum.  Backward from the saved fp32 alpha (coef): d = <dout, v> (F-term) with dropout applied, dot = sum
    alpha d, de = alpha (d - dot) (x slope factor for gat; fa: d (1 - t^2) with t wrong by e_coef), then sums of de and of
    alpha_d dout over rows of the CSR (destination side) and of its transpose (source side) by the product rule; datt of
    gatv2 is an nnz-term sum in any order (atomics)."""
    layer, n, H, F = inp.layer, inp.n, inp.H, inp.F
    g = inp.csr
    row, col = torch.from_numpy(g.row), torch.from_numpy(g.col)
    nnz = g.nnz
    Hd = 1 if layer == "fa" else H
    slot = torch.arange(nnz, dtype=torch.int64)
    ks_ = keep_of(slot.view(-1, 1) * Hd + torch.arange(Hd).view(1, -1), inp.p, ATT_SEED, ATT_STREAM).double() * inp.scale
    deg_in = torch.from_numpy(g.cnt_in).double()
    deg_out = torch.from_numpy(g.cnt_out).double()
    dout = inp.dout.double()
    b = Box()

    def by_row(t):           # sum over the slots of each destination
        return torch.zeros((n,) + t.shape[1:], dtype=F64).index_add_(0, row, t)

    def by_col(t):
        return torch.zeros((n,) + t.shape[1:], dtype=F64).index_add_(0, col, t)

    def seg_max(t):
        idx = row.view(-1, 1).expand(-1, t.shape[1])
        return torch.full((n, t.shape[1]), -INF, dtype=F64).scatter_reduce(0, idx, t, "amax")

    if layer == "fa":
        x = inp.xp.double()
        val = inp.val.double().view(-1, 1)
        pre = inp.al.double()[col] + inp.ar.double()[row]
        c = ref.coef.double()
        e_c = U * pre.abs() + TANHR * c.abs()
        cd = c * ks_
        w = (e_c * ks_ + (deg_in[row].view(-1, 1) + 5) * U * cd.abs()) * val.abs()           # [nnz][1]
        b.coef = e_c
        b.out = by_row(w.unsqueeze(-1) * x[col].abs()) + U * ref.out.double().abs() + 2 * U * FA_EPS * inp.x0.double().abs()
        d = (dout[row] * x[col]).sum(-1) * val
        e_d = (F + 2) * U * (dout[row] * x[col]).abs().sum(-1) * val.abs()
        dd, e_dd = d * ks_, e_d * ks_ + U * (d * ks_).abs()
        om = 1 - c * c
        e_g = e_dd * (om + 2 * c.abs() * e_c + e_c * e_c) + dd.abs() * (2 * c.abs() * e_c + e_c * e_c + 2 * U) + U * ref.de.double().abs()
        gabs = ref.de.double().abs()
        sf = torch.ones_like(pre)
    else:
        if layer == "gat":
            v = inp.xp.double()
            pre = inp.al.double()[col] + inp.ar.double()[row]
            l = torch.where(pre > 0, pre, ATT_SLOPE * pre)
            el = 2 * U * l.abs()
            sf = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, ATT_SLOPE))
        elif layer == "gatv2":
            v = inp.ks.double()
            sv = v[col] + inp.qd.double()[row]
            lr = torch.where(sv > 0, sv, ATT_SLOPE * sv)
            att = inp.att.double().view(1, H, F)
            l = (att * lr).sum(-1)
            el = (F + 3) * U * (att * lr).abs().sum(-1)
            sf = torch.ones_like(l)
        else:
            v = inp.v.double()
            qk = inp.qd.double()[row] * inp.ks.double()[col]
            l = qk.sum(-1) * inp.dot_scale
            el = (F + 2) * U * qk.abs().sum(-1) * inp.dot_scale
            sf = torch.ones_like(l)
        alpha = ref.alpha.double()
        spread = seg_max(l) - (-seg_max(-l))
        spread = torch.where(torch.isfinite(spread), spread, torch.zeros_like(spread))
        elm = seg_max(el)
        rel = softmax_rel(elm, spread, deg_in.view(-1, 1))[row]
        ea = alpha * rel
        b.alpha = ea
        ad = alpha * ks_
        w = ea * ks_ + (deg_in[row].view(-1, 1) + 4) * U * ad
        b.out = by_row(w.unsqueeze(-1) * v[col].abs()) + U * ref.out.double().abs() + U * inp.bias.double().abs().view(1, H, F)
        d = (dout[row] * v[col]).sum(-1)
        e_d = (F + 1) * U * (dout[row] * v[col]).abs().sum(-1)
        dd, e_dd = d * ks_, e_d * ks_ + U * (d * ks_).abs()
        dot = by_row(alpha * dd)
        e_dot = by_row(ea * dd.abs() + alpha * e_dd + ea * e_dd) + (deg_in.view(-1, 1) + 2) * U * by_row((alpha * dd).abs())
        diff = dd - dot[row]
        e_g = (ea * diff.abs() + (alpha + ea) * (e_dd + e_dot[row] + U * (dd.abs() + dot[row].abs()))) * sf + 2 * U * ref.de.double().abs()
        gabs = ref.de.double().abs()
    b.de = e_g
    e_dar = by_row(e_g) + deg_in.view(-1, 1) * U * by_row(gabs)
    e_dal = by_col(e_g) + deg_out.view(-1, 1) * U * by_col(gabs)
    do_ = deg_out.view(-1, 1, 1)
    di_ = deg_in.view(-1, 1, 1)
    if layer in ("gat", "fa"):
        b.dar, b.dal = e_dar, e_dal
        asrc, adst = inp.att_src.double().abs(), inp.att_dst.double().abs()
        b.dxp = (e_dal.unsqueeze(-1) * asrc + e_dar.unsqueeze(-1) * adst + by_col(w.unsqueeze(-1) * dout[row].abs())
                 + (do_ + 5) * U * (ref.dal.double().abs().unsqueeze(-1) * asrc + ref.dar.double().abs().unsqueeze(-1) * adst)
                 + U * ref.dxp.double().abs())
        return b
    wv = w.unsqueeze(-1) * dout[row].abs()                 # the value path into a source row
    if layer == "gatv2":
        att = inp.att.double().view(1, H, F).abs()
        sfe = torch.where(sv > 0, torch.ones_like(sv), torch.full_like(sv, ATT_SLOPE))
        term_e, term_m = e_g.unsqueeze(-1) * att * sfe, gabs.unsqueeze(-1) * att * sfe
        b.dqd = by_row(term_e) + (di_ + 3) * U * by_row(term_m) + U * ref.dqd.double().abs()
        b.dks = by_col(term_e + wv) + (2 * do_ + 4) * U * by_col(term_m) + U * ref.dks.double().abs()
        b.datt = (e_g.unsqueeze(-1) * lr.abs()).sum(0) + (nnz + 3) * U * (gabs.unsqueeze(-1) * lr.abs()).sum(0) + U * ref.datt.double().abs()
    else:
        kq = inp.ks.double()[col].abs() * inp.dot_scale
        qq = inp.qd.double()[row].abs() * inp.dot_scale
        b.dqd = by_row(e_g.unsqueeze(-1) * kq) + (di_ + 3) * U * by_row(gabs.unsqueeze(-1) * kq) + U * ref.dqd.double().abs()
        b.dks = by_col(e_g.unsqueeze(-1) * qq) + (do_ + 3) * U * by_col(gabs.unsqueeze(-1) * qq) + U * ref.dks.double().abs()
        b.dv = by_col(wv) + U * ref.dv.double().abs()
    return b


def att_ratios(got, ref, b):
    return {k: ratio(got[k], ref[k], b[k]) for k in b if k in got and got[k] is not None
            and tuple(got[k].shape) == tuple(ref[k].shape)}


ATT_BUGS_OF = {"gat": ATT_BUGS, "gatv2": ATT_BUGS,
               "dot": ("softmax_outgoing", "philox_transposed", "philox_shift", "bwd_no_drop_scale"),   # no leaky ReLU, no self loop
               # no softmax, no leaky ReLU; one head, for which h * nnz + p is p itself: the shifted word stands for a wrong index
               "fa": ("philox_shift", "bwd_no_drop_scale", "no_self_loop")}
