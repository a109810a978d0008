"""The fp32 MIL / graph kernels over their dispatch domains on the MI355X, through the C ABI, against the fp64 references
and derived per-element bounds of tests/f32_kernel_ref.py (tests/test_f32_kernel_ref_cpu.py shows on the CPU that the
bounds admit a correct fp32 evaluation and reject the wrong variants).  Every case runs once; outputs are pre-filled with
NaN between guard areas; the worst error / bound ratio per entry point and family is printed at the end (visible with -s).

A  LayerNorm(+ReLU +dropout +residual) forward, and the atomic / workspace / dxsum backward forms.
B  attention pool forward / backward / backward with parameter sums, one case per dispatch arm, ragged bags with empty ones.
C  GAT, GATv2, TransformerConv and FAConv message passing on a 1100-node graph whose rows cross the 512 edges kept in LDS.
D  isic_spmm_csr_f32 on every kernel it dispatches to, over isic_gcn_csr_build modes 0 / 1 / 2.
E  l2-normalize, row softmax, cross entropy, relu-dropout, tanh backward, column sums.

Kernel template instantiation -> a case that launches it (read from the host dispatch conditions):
  layernorm_fwd_vec_kernel<16|32|64>          A  N64|N128|N256 ... -o0 (aligned); at its grid cap: N256-M32773
  layernorm_fwd_kernel                        A  every -o1 case and every generic width (N1 ... N1024), N = 1025
  layernorm_bwd_vec_kernel<16|32|64, false>   A  N64|N128|N256 -o0: atomic form (no workspace) and workspace form; at its grid cap: N256-M32773
  layernorm_bwd_vec_kernel<16|32|64, true>    A  N64|N128|N256 -o0: dxsum form
  layernorm_bwd_kernel<2>                     A  N1, N3, N63, N65, N100, N64-o1, N128-o1; at its grid cap (and the generic forward's): N3-M32773
  layernorm_bwd_kernel<4>                     A  N129, N255, N256-o1
  layernorm_bwd_kernel<8>                     A  N257, N511
  layernorm_bwd_kernel<16>                    A  N513, N1000, N1024
  ln_bwd_reduce_kernel                        A  every workspace / dxsum form
  attn_pool_fwd2_kernel                       B  H64-A32-h4-C0, H128-A128-h4-C0, H1-A1-h1-C0
  attn_pool_fwd_kernel<2, 2>                  B  H65-A64-h1-C1 ... H128-A64-h1-C16, H64-A32-h6-C0 (two launches)
  attn_pool_fwd_kernel<2, 0>                  B  H128-A129
  attn_pool_fwd_kernel<4, 0>                  B  H129-A64, H256-A200
  attn_pool_fwd_kernel<8, 0>                  B  H257-A64, H512-A64
  attn_pool_fwd_kernel<16, 0>                 B  H513-A64, H1024-A64
  attn_pool_bwd_kernel<true>                  B  every H <= 128, A <= 128 case (with and without param_sums)
  attn_pool_bwd_kernel<false>                 B  H128-A129 and every H > 128 case
  gat_scores / gat_fwd / gat_bwd_dst / _src   C  gat-*, fa-* (scores with H = 1)
  edge_attn_fwd_kernel<0|1>, edge_attn_bwd_dst_kernel<0|1>, edge_attn_bwd_src_kernel<0|1>
                                              C  gatv2-* | dot-*  (datt in registers up to H4-F256 / H8-F128, atomic at H4-F257, H8-F130)
  fa_fwd / fa_bwd_dst / fa_bwd_src            C  fa-*
  spmm_kernel<1>                              D  F1, F3, F30, F127
  spmm_kernel<2>                              D  F130, F258, F128-o1
  spmm_kernel<4>                              D  F260, F512, F256-o1
  spmm_group_kernel<16|32|64>                 D  F64 | F128 | F256 (-o0), hub rows of 700 entries split into items

Worst device error / bound ratio per family, MI355X: not measured (no MI355X run of this module has happened yet; the
module prints the table at its end)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import f32_kernel_ref as R  # noqa: E402
from helpers import DEV, NAN, Guarded, stop_after_a_device_error  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64
UNSUPPORTED = -2
WORST = {}


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
        print("worst device ratio", key, {k: round(v, 3) for k, v in WORST[key].items()})


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    stop_after_a_device_error()


def _note(key, ratios):
    w = WORST.setdefault(key, {})
    for k, v in ratios.items():
        w[k] = max(w.get(k, 0.0), v)


def _check(key, what, ratios):
    print(what, " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    _note(key, ratios)
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


def _place(t, offset=0):
    """a device copy of an input, optionally one float off 16-byte alignment"""
    if t is None:
        return None
    if not offset:
        return t.to(DEV).contiguous()
    buf = torch.zeros(t.numel() + 4, device=DEV, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(*t.shape)
    v.copy_(t)
    return v


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16) + 16, device=DEV, dtype=torch.uint8)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _clock(step):
    return None if step is None else torch.tensor([step, 0], dtype=torch.int64, device=DEV)


# ================================================================== A. LayerNorm
def _ln_backward(form, inp, x, dy, gamma, beta, mean, rstd, off, clock, thr):
    M, N = inp.M, inp.N
    dx = Guarded((M, N), off)
    dgamma, dbeta = Guarded((N,), init=inp.dgamma0), Guarded((N,), init=inp.dbeta0)
    dxsum = Guarded((N,), init=inp.dxsum0) if form == "dxsum" else None
    tail = (M, N, inp.relu, thr, inp.scale, R.LN_SEED, R.LN_STREAM, clock)
    if form == "atomic":
        _call("isic_layernorm_bwd_clk", dy, x, gamma, beta, mean, rstd, dx.t, dgamma.t, dbeta.t, *tail)
    else:
        nbytes = _call("isic_layernorm_bwd_workspace_bytes", N)
        ws = _ws(nbytes)
        if form == "ws":
            _call("isic_layernorm_bwd_ws", dy, x, gamma, beta, mean, rstd, dx.t, dgamma.t, dbeta.t, *tail, ws, nbytes)
        else:
            _call("isic_layernorm_bwd_dxsum_ws", dy, x, gamma, beta, mean, rstd, dx.t, dgamma.t, dbeta.t, dxsum.t, *tail, ws, nbytes)
    assert dx.ok() and dgamma.ok() and dbeta.ok() and (dxsum is None or dxsum.ok()), form
    return dict(dx=dx.cpu(), dgamma=dgamma.cpu(), dbeta=dbeta.cpu(), dxsum=None if dxsum is None else dxsum.cpu())


@pytest.mark.parametrize("case", R.LN_CASES, ids=[c["id"] for c in R.LN_CASES])
def test_layernorm_forward_and_the_three_backward_forms(case):
    inp = R.ln_inputs(case)
    ref = R.ln_eval(inp, F64)
    fb = R.ln_forward_bounds(inp, ref)
    bb = R.ln_backward_bounds(inp, ref, fb)
    assert bb.share <= R.AMBIGUOUS_CAP
    M, N, off = inp.M, inp.N, inp.misalign
    x, dy = _place(inp.x, off), _place(inp.dy, off)
    gamma, beta, res = _place(inp.gamma), _place(inp.beta), _place(inp.res)
    y, mean, rstd = Guarded((M, N), off), Guarded((M,)), Guarded((M,))
    clock, thr = _clock(inp.clock), R.drop_threshold(inp.p)
    _call("isic_layernorm_fwd_clk", x, gamma, beta, res, y.t, mean.t, rstd.t, M, N, R.LN_EPS, inp.relu, thr, inp.scale,
          R.LN_SEED, R.LN_STREAM, clock)
    assert y.ok() and mean.ok() and rstd.ok()
    got = dict(y=y.cpu(), mean=mean.cpu().view(M, 1), rstd=rstd.cpu().view(M, 1))
    vec = N in R.LN_VEC_WIDTHS and not off
    args = (inp, x, dy, gamma, beta, mean.t, rstd.t, off, clock, thr)
    runs = {"atomic": _ln_backward("atomic", *args), "ws": _ln_backward("ws", *args)}
    if vec:
        runs["dxsum"] = _ln_backward("dxsum", *args)
    ratios = R.ln_ratios(got, ref, fb)
    for form, out in runs.items():
        for k, v in R.ln_ratios({**got, **out}, ref, fb, bb).items():
            if k not in ("y", "mean", "rstd"):
                ratios[f"{form}.{k}"] = v
    _check(("layernorm", inp.family), case["id"], ratios)
    # the order-fixed forms are bit-equal across two runs (the atomic form is held to the bounds only)
    for form in ("ws", "dxsum") if vec else ("ws",):
        again = _ln_backward(form, *args)
        for k, v in again.items():
            assert v is None or torch.equal(_bits(v), _bits(runs[form][k])), (form, k)
    if vec:                                                # dxsum is the column sums of the dx it returned
        dxs, dxv = runs["dxsum"]["dxsum"].double(), runs["dxsum"]["dx"].double()
        tol = (M + 1) * R.U * dxv.abs().sum(0) + 2 * R.U * (inp.dxsum0.double().abs() + dxs.abs())
        assert bool(((dxs - inp.dxsum0.double() - dxv.sum(0)).abs() <= tol).all())
    else:                                                  # refused before any device work (read: the checks precede the launches)
        ws = _ws(_call("isic_layernorm_bwd_workspace_bytes", N))
        d = Guarded((N,))
        assert _code("isic_layernorm_bwd_dxsum_ws", dy, x, gamma, beta, mean.t, rstd.t, torch.empty_like(x), d.t, d.t, d.t, M, N,
                     inp.relu, thr, inp.scale, R.LN_SEED, R.LN_STREAM, clock, ws, ws.numel() - 16) == UNSUPPORTED
        assert bool(torch.isnan(d.buf).all())


def test_layernorm_width_1025_forward_runs_and_backward_is_refused():
    case = dict(N=1025, M=5, family="random", relu=0, residual=1, p=0.25, clock=None, misalign=0, id="N1025")
    inp = R.ln_inputs(case)
    ref = R.ln_eval(inp, F64)
    fb = R.ln_forward_bounds(inp, ref)
    x, gamma, beta, res = _place(inp.x), _place(inp.gamma), _place(inp.beta), _place(inp.res)
    y, mean, rstd = Guarded((5, 1025)), Guarded((5,)), Guarded((5,))
    _call("isic_layernorm_fwd_clk", x, gamma, beta, res, y.t, mean.t, rstd.t, 5, 1025, R.LN_EPS, 0, R.drop_threshold(0.25),
          inp.scale, R.LN_SEED, R.LN_STREAM, None)
    assert y.ok() and mean.ok() and rstd.ok()
    _check(("layernorm", "random"), "N1025 forward",
           R.ln_ratios(dict(y=y.cpu(), mean=mean.cpu().view(5, 1), rstd=rstd.cpu().view(5, 1)), ref, fb))
    d = Guarded((5, 1025))
    g = Guarded((1025,))
    assert _code("isic_layernorm_bwd", _place(inp.dy), x, gamma, beta, mean.t, rstd.t, d.t, g.t, g.t, 5, 1025, 0, 0, 1.0, 0, 0) == UNSUPPORTED
    assert bool(torch.isnan(d.buf).all()) and bool(torch.isnan(g.buf).all())


# ================================================================== B. attention pool
@pytest.mark.parametrize("case", R.POOL_CASES, ids=[c["id"] for c in R.POOL_CASES])
def test_attention_pool_forward_and_backward(case):
    inp = R.pool_inputs(case)
    ref = R.pool_eval(inp, F64)
    b = R.pool_bounds(inp, ref)
    H, A, heads, C, T, B = inp.H, inp.A, inp.heads, inp.C, inp.T, inp.B
    h, t, w3, b3 = _place(inp.h), _place(inp.t), _place(inp.w3), _place(inp.b3)
    W4, b4, offsets = _place(inp.W4), _place(inp.b4), inp.offsets.to(DEV)
    max_bag = max(case["bags"])
    att, z = Guarded((T, heads)), Guarded((B, H))
    P = Guarded((T, C)) if C else None
    pp = Guarded((T, C)) if C else None
    bl = Guarded((B, C)) if C else None
    bp = Guarded((B, C)) if C else None
    tt = lambda g: None if g is None else g.t      # noqa: E731
    _call("isic_attn_pool_fwd", h, t, w3, b3, W4, b4, offsets, B, H, A, heads, C, max_bag, att.t, z.t, tt(P), tt(pp), tt(bl), tt(bp))
    outs = dict(att=att, z=z, P=P, pp=pp, bl=bl, bp=bp)
    assert all(g.ok() for g in outs.values() if g is not None)
    got = {k: (None if g is None else g.cpu()) for k, g in outs.items()}
    ratios = R.pool_ratios(got, ref, b, R.POOL_FWD_KEYS)
    for bi, n in enumerate(case["bags"]):                  # an empty bag: zeros and a uniform bag_probs (include/isic_hip.h)
        if n == 0:
            assert bool((got["z"][bi] == 0).all())
            if C:
                assert bool((got["bl"][bi] == 0).all())
                assert bool((got["bp"][bi] == torch.tensor(1.0) / C).all())      # exp(0) / C, one correctly rounded division
    dz, dL = _place(inp.dz), _place(inp.dL)
    fast = H <= 128 and A <= 128
    PW = 2 * heads * A + heads

    def backward(sums):
        d_h = Guarded((T, H), init=inp.dh0 if inp.accumulate_dh else None)
        d_u, d_s = Guarded((T, heads * A)), Guarded((T, heads))
        d_P = Guarded((T, C)) if C else None
        psum = Guarded((B, PW)) if sums else None
        args = (h, t, att.t, tt(P), w3, W4, offsets, B, H, A, heads, C, max_bag, dL, dz, d_h.t, inp.accumulate_dh, d_u.t, d_s.t, tt(d_P))
        if sums:
            _call("isic_attn_pool_bwd_sums", *args, psum.t)
        else:
            _call("isic_attn_pool_bwd", *args)
        o = dict(d_h=d_h, d_u=d_u, d_s=d_s, d_P=d_P, psum=psum)
        assert all(g.ok() for g in o.values() if g is not None)
        return {k: (None if g is None else g.cpu()) for k, g in o.items()}

    if heads > 4:                                          # refused before any device work (read: the check precedes the launch)
        d = Guarded((T, heads * A))
        assert _code("isic_attn_pool_bwd", h, t, att.t, None, w3, None, offsets, B, H, A, heads, 0, max_bag, None, dz, d.t, 0, d.t,
                     d.t, None) == UNSUPPORTED
        assert bool(torch.isnan(d.buf).all())
    else:
        plain = backward(False)
        for k, v in R.pool_ratios(plain, ref, b, R.POOL_BWD_KEYS).items():
            ratios[f"bwd.{k}"] = v
        if fast:
            s1, s2 = backward(True), backward(True)
            for k, v in R.pool_ratios(s1, ref, b, R.POOL_BWD_KEYS).items():
                ratios[f"sums.{k}"] = v
            for k in s1:                                   # fixed summation order: bit-equal across two runs
                assert s1[k] is None or torch.equal(_bits(s1[k]), _bits(s2[k])), k
            # summed over the bags in fp64: the column sums of d_u, d_s t and d_s
            ratios["sums.total"] = R.ratio(s1["psum"].double().sum(0), ref.psum.sum(0), b.psum.sum(0))
            # ... and of the d_u / d_s this very call returned (and its input t): T-term sums of fp32 values, split per bag
            du, ds, tv = s1["d_u"].double(), s1["d_s"].double(), inp.t.double().view(T, heads, A)
            dst = (ds.unsqueeze(-1) * tv).reshape(T, heads * A)
            own = torch.cat([du.sum(0), dst.sum(0), ds.sum(0)])
            mag = torch.cat([du.abs().sum(0), dst.abs().sum(0), ds.abs().sum(0)])
            ratios["sums.own"] = R.ratio(s1["psum"].double().sum(0), own, (T + 2) * R.U * mag)
            for bi, n in enumerate(case["bags"]):
                if n == 0:
                    assert bool((s1["psum"][bi] == 0).all())
        else:
            d = Guarded((B, PW))
            assert _code("isic_attn_pool_bwd_sums", h, t, att.t, tt(P), w3, W4, offsets, B, H, A, heads, C, max_bag, dL, dz, None, 0,
                         torch.empty(T, heads * A, device=DEV), None, None, d.t) == UNSUPPORTED
            assert bool(torch.isnan(d.buf).all())
    _check(("attn_pool", inp.family), case["id"] + " [" + case["arm"] + "]", ratios)


# ================================================================== the CSR build, shared by C and D
_CSR = {}


def _build_csr(key, src, dst, w, n, mode):
    """isic_gcn_csr_build on the device, checked against the numpy CSR; -> (device arrays, reference)"""
    if key in _CSR:
        return _CSR[key]
    E = int(src.size)
    ref = R.csr_ref(src, dst, w, n, mode)
    cap = E + n
    mk = lambda m, dt: torch.full((m + 8,), -7, device=DEV, dtype=dt)      # noqa: E731  (8 sentinel entries behind each array)
    d = R.Box(rowptr=mk(n + 1, torch.int32), col=mk(cap, torch.int32), rowptr_t=mk(n + 1, torch.int32), col_t=mk(cap, torch.int32),
              perm_t=mk(cap, torch.int32), val=torch.full((cap + 8,), NAN, device=DEV), val_t=torch.full((cap + 8,), NAN, device=DEV))
    nbytes = _call("isic_gcn_csr_workspace_bytes", n, E)
    ws = _ws(nbytes)
    _call("isic_gcn_csr_build", torch.from_numpy(src).to(DEV) if E else None, torch.from_numpy(dst).to(DEV) if E else None,
          torch.from_numpy(w).to(DEV) if w is not None and E else None, E, n, mode, d.rowptr, d.col, d.val, d.rowptr_t, d.col_t,
          d.val_t, d.perm_t, ws, nbytes)
    nnz = ref.nnz
    for name, m in (("rowptr", n + 1), ("rowptr_t", n + 1), ("col", cap), ("col_t", cap), ("perm_t", cap)):
        assert bool((d[name][m:] == -7).all()), name
    assert bool(torch.isnan(d.val[cap:]).all()) and bool(torch.isnan(d.val_t[cap:]).all())
    for name in ("rowptr", "rowptr_t"):
        assert np.array_equal(d[name][:n + 1].cpu().numpy(), ref[name]), name
    for name in ("col", "col_t", "perm_t"):
        assert np.array_equal(d[name][:nnz].cpu().numpy(), ref[name]), name
    for name, rel in (("val", ref.rel), ("val_t", ref.rel_t)):
        r = R.ratio(d[name][:nnz].cpu(), torch.from_numpy(ref[name]), torch.from_numpy(np.abs(ref[name]) * rel))
        _note(("csr_build", f"mode{mode}"), {name: r})
        assert r <= 1.0, (name, r)
    _CSR[key] = (d, ref)
    return d, ref


# ================================================================== C. GAT, GATv2 / TransformerConv, FAConv
def _att_run(inp, d):
    """one forward and one backward of the case's layer on the device -> outputs on the CPU (node-shaped [n][H][F])"""
    layer, n, H, F = inp.layer, inp.n, inp.H, inp.F
    nnz = inp.csr.nnz
    thr = R.drop_threshold(inp.p)
    drop = (thr, inp.scale, R.ATT_SEED, R.ATT_STREAM)
    dout = _place(inp.dout)
    node = lambda: Guarded((n, H, F))            # noqa: E731
    out = node()
    o = {}
    if layer in ("gat", "fa"):
        xp, al, ar = _place(inp.xp), _place(inp.al), _place(inp.ar)
        a_s, a_d = _place(inp.att_src), _place(inp.att_dst)
        de, dar, dal, dxp = Guarded((nnz, H)), Guarded((n, H)), Guarded((n, H)), node()
        if layer == "gat":
            alpha = Guarded((nnz, H))
            _call("isic_gat_fwd", xp, al, ar, d.rowptr, d.col, _place(inp.bias), out.t, alpha.t, n, H, F, R.ATT_SLOPE, *drop)
            _call("isic_gat_bwd", dout, xp, alpha.t, al, ar, a_s, a_d, d.rowptr, d.col, d.rowptr_t, d.col_t, d.perm_t, de.t, dar.t,
                  dal.t, dxp.t, n, H, F, R.ATT_SLOPE, *drop)
            o["alpha"] = alpha
        else:
            coef = Guarded((nnz, 1))
            _call("isic_fa_fwd", xp, _place(inp.x0), al, ar, d.rowptr, d.col, d.val, out.t, coef.t, n, F, R.FA_EPS, *drop)
            _call("isic_fa_bwd", dout, xp, coef.t, a_s, a_d, d.rowptr, d.col, d.val, d.rowptr_t, d.col_t, d.val_t, d.perm_t, de.t,
                  dar.t, dal.t, dxp.t, n, F, *drop)
            o["coef"] = coef
        o.update(out=out, de=de, dar=dar, dal=dal, dxp=dxp)
    else:
        mode = 0 if layer == "gatv2" else 1
        ks, qd = _place(inp.ks), _place(inp.qd)
        v = ks if mode == 0 else _place(inp.v)
        att = _place(inp.att) if mode == 0 else None
        alpha, de, dqd, dks = Guarded((nnz, H)), Guarded((nnz, H)), node(), node()
        dv = node() if mode == 1 else None
        datt = Guarded((H, F), init=torch.zeros(H, F)) if mode == 0 else None
        sc = inp.dot_scale
        _call("isic_edge_attn_fwd", mode, ks, qd, v, att, d.rowptr, d.col, _place(inp.bias), out.t, alpha.t, n, H, F, R.ATT_SLOPE, sc,
              *drop)
        _call("isic_edge_attn_bwd", mode, dout, ks, qd, v, att, alpha.t, d.rowptr, d.col, d.rowptr_t, d.col_t, d.perm_t, de.t, dqd.t,
              dks.t, None if dv is None else dv.t, None if datt is None else datt.t, n, H, F, R.ATT_SLOPE, sc, *drop)
        o.update(alpha=alpha, out=out, de=de, dqd=dqd, dks=dks)
        if dv is not None:
            o["dv"] = dv
        if datt is not None:
            o["datt"] = datt
    assert all(g.ok() for g in o.values()), [k for k, g in o.items() if not g.ok()]
    return {k: g.cpu() for k, g in o.items()}


@pytest.mark.parametrize("case", R.ATT_CASES, ids=[c["id"] for c in R.ATT_CASES])
def test_graph_attention_layers_forward_and_backward(case):
    inp = R.att_inputs(case)
    layer, n, H, F = inp.layer, inp.n, inp.H, inp.F
    mode = R.att_csr_mode(layer)
    d, cref = _build_csr(("att", n, mode), inp.src, inp.dst, inp.w, n, mode)
    ratios = {}
    if layer in ("gat", "fa"):                             # the scores entry, then ITS fp32 scores are the layer's inputs
        al, ar = Guarded((n, H)), Guarded((n, H))
        _call("isic_gat_scores", _place(inp.xp), _place(inp.att_src), _place(inp.att_dst), al.t, ar.t, n, H, F)
        assert al.ok() and ar.ok()
        s64, sb = R.att_scores(inp, F64), R.att_scores_bounds(inp)
        ratios["scores.al"], ratios["scores.ar"] = R.ratio(al.cpu(), s64.al, sb.al), R.ratio(ar.cpu(), s64.ar, sb.ar)
        inp.al, inp.ar = al.cpu(), ar.cpu()
        inp.val = d.val[:cref.nnz].cpu()                   # FA: the build's own fp32 normalisation (checked in _build_csr)
    assert R.att_zero_pre_share(inp) <= R.AMBIGUOUS_CAP
    ref = R.att_eval(inp, F64)
    b = R.att_bounds(inp, ref)
    got = _att_run(inp, d)
    if layer == "fa":
        assert tuple(got["coef"].shape) == tuple(ref.coef.shape)
    ratios.update(R.att_ratios(got, ref, b))
    assert set(b) <= set(ratios), sorted(set(b) - set(ratios))
    _check((layer, f"p{inp.p}"), case["id"], ratios)
    if layer == "dot" and n == R.ATT_N:                    # a node without incoming edges: out = bias, zero gradients
        assert int(cref.cnt_in[0]) == 0
        assert torch.equal(got["out"][0].reshape(-1), inp.bias) and bool((got["dqd"][0] == 0).all())
    again = _att_run(inp, d)                               # bit-equal, except datt (every path ends in fp32 atomics)
    for k, v in again.items():
        if k != "datt":
            assert torch.equal(_bits(v), _bits(got[k])), k


# ================================================================== D. SpMM
@pytest.mark.parametrize("case", R.SPMM_CASES, ids=[c["id"] for c in R.SPMM_CASES])
def test_spmm_on_every_kernel_and_csr_mode(case):
    inp = R.spmm_inputs(case)
    n, F = inp.n, inp.F
    key = ("spmm", n, inp.mode, inp.weighted, inp.empty)
    d, cref = _build_csr(key, inp.src, inp.dst, inp.w, n, inp.mode)
    ref = R.spmm_eval(inp, F64, csr=cref)
    b = R.spmm_bounds(inp, ref)
    x = _place(inp.x)
    bias = _place(inp.bias, inp.bias_offset)
    addend = _place(inp.addend_t)
    out = Guarded((n, F))
    rp, col, val = (d.rowptr_t, d.col_t, d.val_t) if inp.transposed else (d.rowptr, d.col, d.val)
    _call("isic_spmm_csr_f32", rp, col, val, x, bias, out.t, n, F, R.SPMM_ALPHA, addend, R.SPMM_ADDEND_SCALE)
    assert out.ok()
    _check(("spmm", f"mode{inp.mode}"), case["id"], {"out": R.ratio(out.cpu(), ref.out, b.out)})
    again = Guarded((n, F))
    _call("isic_spmm_csr_f32", rp, col, val, x, bias, again.t, n, F, R.SPMM_ALPHA, addend, R.SPMM_ADDEND_SCALE)
    assert torch.equal(_bits(again.t), _bits(out.t))


# ================================================================== E. the small row-wise entries
@pytest.mark.parametrize("N", R.L2_WIDTHS)
def test_l2normalize(N):
    inp = R.l2_inputs(N)
    ref = R.l2_eval(inp, F64)
    b = R.l2_bounds(inp, ref)
    M = inp.M
    y, norm, dx = Guarded((M, N)), Guarded((M,)), Guarded((M, N))
    _call("isic_l2normalize_fwd", _place(inp.x), y.t, norm.t, M, N, R.L2_EPS)
    _call("isic_l2normalize_bwd", _place(inp.dy), y.t, norm.t, dx.t, M, N, R.L2_EPS)
    assert y.ok() and norm.ok() and dx.ok()
    got = dict(y=y.cpu(), norm=norm.cpu(), dx=dx.cpu())
    assert bool((got["y"][0] == 0).all()) and float(got["norm"][0]) == float(np.float32(R.L2_EPS)) == float(got["norm"][1])
    _check(("l2normalize", "-"), f"N={N}", {k: R.ratio(got[k], ref[k], b[k]) for k in b})


@pytest.mark.parametrize("M,N", R.SOFTMAX_SHAPES)
def test_softmax_rows(M, N):
    inp = R.softmax_inputs(M, N)
    ref = R.softmax_eval(inp, F64)
    b = R.softmax_bounds(inp, ref)
    p, dx = Guarded((M, N)), Guarded((M, N))
    _call("isic_softmax_rows_fwd", _place(inp.x), p.t, M, N)
    _call("isic_softmax_rows_bwd", p.t, _place(inp.dp), dx.t, M, N)
    assert p.ok() and dx.ok()
    _check(("softmax_rows", "-"), f"M={M} N={N}", {"p": R.ratio(p.cpu(), ref.p, b.p), "dx": R.ratio(dx.cpu(), ref.dx, b.dx)})


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("B,C", R.CE_SHAPES)
def test_cross_entropy(B, C, mode):
    inp = R.ce_inputs(B, C, mode)
    ref = R.ce_eval(inp, F64)
    b = R.ce_bounds(inp, ref)
    x, labels = _place(inp.x), inp.labels.to(DEV)
    loss, mean, d_in = Guarded((B,)), Guarded((1,)), Guarded((B, C))
    _call("isic_cross_entropy", x, labels, B, C, mode, R.CE_GRAD_SCALE, loss.t, mean.t, d_in.t)
    assert loss.ok() and mean.ok() and d_in.ok()
    got = dict(loss=loss.cpu(), mean=mean.cpu(), d_in=d_in.cpu())
    _check(("cross_entropy", f"mode{mode}"), f"B={B} C={C}", {k: R.ratio(got[k], ref[k], b[k]) for k in b})
    only_mean = Guarded((1,))                              # NULL loss_per_sample / d_in: the mean alone, the same bits
    _call("isic_cross_entropy", x, labels, B, C, mode, R.CE_GRAD_SCALE, None, only_mean.t, None)
    assert only_mean.ok() and torch.equal(_bits(only_mean.t), _bits(mean.t))


@pytest.mark.parametrize("n", R.RD_SIZES)
def test_relu_dropout_keeps_exactly_the_oracles_set(n):
    for p, clock in ((R.RD_P, R.RD_CLOCK), (R.RD_P, None), (0.0, None)):
        inp = R.rd_inputs(n, p, clock)
        ref = R.rd_eval(inp, F64)
        b = R.rd_bounds(inp, ref)
        y = Guarded((n,), init=inp.x)
        _call("isic_relu_dropout_fwd_clk_f32", y.t, n, R.drop_threshold(p), inp.scale, R.RD_SEED, R.RD_STREAM, _clock(clock))
        assert y.ok()
        assert torch.equal(y.cpu() != 0, inp.keep & (inp.x > 0))
        dx, dy_inplace = Guarded((n,)), Guarded((n,), init=inp.dy)
        _call("isic_relu_dropout_bwd_out_f32", y.t, _place(inp.dy), dx.t, n, inp.scale)
        _call("isic_relu_dropout_bwd_f32", y.t, dy_inplace.t, n, inp.scale)
        assert dx.ok() and dy_inplace.ok() and torch.equal(_bits(dx.t), _bits(dy_inplace.t))
        _check(("relu_dropout", f"p{p}"), f"n={n} clock={clock}", {"y": R.ratio(y.cpu(), ref.y, b.y), "dx": R.ratio(dx.cpu(), ref.dx, b.dx)})


def test_tanh_backward():
    g = torch.Generator().manual_seed(3)
    for n in (1, 3, 1025):
        dy, t = torch.randn(n, generator=g), torch.tanh(torch.randn(n, generator=g) * 2)
        ref = dy.double() * (1 - t.double() ** 2)
        dx = Guarded((n,))
        _call("isic_tanh_bwd_f32", _place(dy), _place(t), dx.t, n)
        assert dx.ok()
        _check(("tanh_bwd", "-"), f"n={n}", {"dx": R.ratio(dx.cpu(), ref, R.tanh_bwd_bounds(dy, t, ref))})


@pytest.mark.parametrize("M,N,ldx", R.COLSUM_SHAPES)
def test_column_sums_with_and_without_a_workspace(M, N, ldx):
    inp = R.colsum_inputs(M, N, ldx)
    X = _place(inp.X)
    nbytes = _call("isic_colsum_f32_workspace_bytes", M, N)
    ws = _ws(nbytes)
    for beta in (0.0, 1.0):
        ref = R.colsum_eval(inp, F64, beta)
        bound = R.colsum_bounds(inp, ref, beta)
        plain = Guarded((N,), init=inp.out0)
        _call("isic_colsum_f32", X, M, N, ldx, plain.t, beta)
        w1, w2 = Guarded((N,), init=inp.out0), Guarded((N,), init=inp.out0)
        _call("isic_colsum_f32_ws", X, M, N, ldx, w1.t, beta, ws, nbytes)
        _call("isic_colsum_f32_ws", X, M, N, ldx, w2.t, beta, ws, nbytes)
        assert plain.ok() and w1.ok() and w2.ok()
        assert torch.equal(_bits(w1.t), _bits(w2.t))       # chunk sums added in chunk order
        _check(("colsum", f"beta{beta}"), f"M={M} N={N} ldx={ldx}",
               {"plain": R.ratio(plain.cpu(), ref, bound), "ws": R.ratio(w1.cpu(), ref, bound)})
