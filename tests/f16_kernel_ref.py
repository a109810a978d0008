"""References, error models and input families for the fp16 transformer / MAE kernels (plain torch on the CPU; shared by
tests/test_f16_kernel_ref_cpu.py, which proves the bounds sound and sharp, and tests/test_f16_kernel_domain_gpu.py, which
holds the kernels to them).

Attention: three things per case, all computed here and never from a kernel's output.
  attention_ref        fp64 softmax attention, its autograd gradients and the fp64 intermediates the bounds need.
  attention_emulation  the kernels' documented arithmetic in torch fp32 ("what a correct kernel may at worst do"): forward
                       = fp32 scores, unnormalised exp2 probabilities, fp16-ROUNDED P in P.V, the UNROUNDED fp32 sum as
                       normaliser, fp16 result; backward = fp32 throughout, Delta_i = dO_i . O_i from the fp16 forward
                       output, results rounded to fp16.  `bug=` turns it into one of six deliberately wrong kernels.
  attention_bounds     per-element bounds from fp64 quantities only.  With PV = P @ |V|, E = 2^-23 C_EPS max(1, max_j |s_ij|)
                       (per query row; s = scaled scores) and dS = P (dP - Delta):
                         out: 2^-10 PV + 2^-11 |ref| + E PV + 2^-25 max_j P_ij sum_{j: P_ij < 2^-14 max P} |V_j|
                         e_i = sum_d |dO_id| bound_out_id                                   (the error of Delta_i)
                         dq:  sc e_i (P @ |K|)       + 2^-11 |ref| + sc (E |dS|) @ |K|
                         dk:  sc (P e)^T @ |Q|       + 2^-11 |ref| + sc (E |dS|)^T @ |Q|
                         dv:                           2^-11 |ref| + (E P)^T @ |dO|
                       2^-11 |ref| is one fp16 store, and never less than 2^-25: below 2^-14 an fp16 is subnormal with
                       spacing 2^-24 (the peaked family's dk and dv live there; without this floor the correct emulation
                       sits at 500 - 2000 times the bound).  On PV, 2^-11 is the rounding of P to fp16 and as much again covers
                       what that leaves out (unnormalised probabilities below 2^-14 are fp16 subnormals with an absolute
                       error of 2^-25 each, and the fp32 sum that feeds the final rounding): 2^-10.  E is the relative
                       error of a probability whose score was rounded in fp32 (an absolute error of the exponent of a few
                       2^-24 |s|), and of the fp32 sums (never below 2^-24 per term whatever the scores: the floor of 1).
                       A store term is tight by nature -- a rounding can cost the full half ulp -- so the acceptance for
                       the emulation and for a kernel alike is ratio <= 1, with no further multiplier.

Calibration of C_EPS, the one free constant (fp32 score rounding, exp2 / exp approximation, summation order), against the
emulation alone: over every family x T in T_LIST x the device test's six (head width, images, heads) shapes ATT_SHAPES
x two summation orders (keys in index order and reversed) -- the very inputs the device test runs -- the smallest power
of two for which the emulation passes is CALIBRATED_C_PASS; it is doubled once (the device's exponentials and MFMA
summation order are not torch's) and nothing else is added.

    CALIBRATED_C_PASS = 4 (at 2 the emulation's dv exceeds its bound: 1.07, peaked, T = 207, width 64, 3 x 6), C_EPS = 8.
    Worst emulation / bound ratio with C_EPS = 8, over every shape, every T of T_LIST and both orders:
        family     out    dq     dk     dv
        gauss      0.47   0.18   0.18   0.99
        peaked     0.51   0.19   1.00   1.00
        shift      0.51   0.12   0.20   0.97
        last_max   0.54   0.18   0.75   1.00
        const_v    0.00   0.00   0.00   0.99
    (peaked dk / dv at 1.00: results below 2^-14, where a store costs exactly half the subnormal spacing.)
    The kernels on the MI355X, same inputs (tests/test_f16_kernel_domain_gpu.py), head width 64 / 32:
        gauss      0.47 / 0.47   0.15 / 0.18   0.13 / 0.18   0.99 / 0.99
        peaked     0.50 / 0.51   0.18 / 0.19   1.00 / 1.00   1.00 / 1.00
        shift      0.48 / 0.51   0.08 / 0.12   0.13 / 0.20   0.97 / 0.97
        last_max   0.51 / 0.54   0.12 / 0.18   0.17 / 0.75   0.99 / 1.00
        const_v    0.00 / 0.00   0.00 / 0.00   0.00 / 0.00   0.99 / 0.99
    The device sits where the emulation does: nothing here says the bound could be tightened.

LayerNorm-add, GEMM and weight-gradient bounds are the forms the existing kernel tests use (test_layernorm_add_matches_torch,
test_layernorm_add_bwd_matches_fp32_autograd, test_gemm_f16_matches_fp32_matmul, test_wgrad_matches_fp64), as helpers, so
that old and new cases share them."""
import math

import torch
import torch.nn.functional as F

F16 = torch.float16
T_LIST = (1, 2, 15, 16, 17, 31, 32, 33, 49, 192, 193, 196, 207, 208)
FAMILIES = ("gauss", "peaked", "shift", "last_max", "const_v")
# (head width, images, heads): the device test's shapes; the CPU proof runs the same inputs
ATT_SHAPES = tuple((hd, n, H) for hd in (64, 32) for n, H in ((1, 1), (2, 3), (3, 6 if hd == 64 else 16)))
BUGS = ("pad_key", "tile_unmasked", "delta_last", "dk_swap8", "scale_d32", "dq_row_1p1")

CALIBRATED_C_PASS = 4.0          # smallest power of two for which the emulation passes everywhere (see the docstring)
C_EPS = 2.0 * CALIBRATED_C_PASS  # doubled once



# ------------------------------------------------------------------ inputs
def attention_inputs(family, n, T, H, hd, seed=0):
    """qkv [n*T][3*H*hd] and dout [n*T][H*hd], fp16, seeded.  gauss is randn x 1.5 (the older tests' input); the other
    families change it as commented below."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + hd + 13 * H + n)
    x = torch.randn(n, T, 3, H, hd, generator=g) * 1.5
    dout = torch.randn(n * T, H * hd, generator=g)
    if family == "peaked":                       # near one-hot softmax rows
        x[:, :, :2] *= 5.0
    elif family == "shift":                      # every score of a row moves by the same large amount
        x[:, :, 1] += 12.0
    elif family == "last_max":                   # key T-1 is every query's arg-max: the running maximum changes last
        u = torch.randn(H, hd, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        x[:, :, 0] += 6.0 * u
        x[:, T - 1, 1] += 6.0 * u
    elif family == "const_v":                    # out == v0 whatever P is; dq == dk == 0
        x[:, :, 2] = x[0, 0, 2].clone()
    return x.to(F16).reshape(n * T, 3 * H * hd).contiguous(), dout.to(F16).contiguous()


def _split(qkv, n, T, H, hd, dtype):
    x = qkv.to(dtype).view(n, T, 3, H, hd).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]                      # each [n][H][T][hd]


def heads_of(rows, n, T, H, hd):
    """[n*T][H*hd] -> [n][H][T][hd]"""
    return rows.view(n, T, H, hd).permute(0, 2, 1, 3)


def rows_of(t):
    """[n][H][T][hd] -> [n*T][H*hd]"""
    n, H, T, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(n * T, H * hd)


# ------------------------------------------------------------------ fp64 reference
def attention_ref(qkv, dout, n, T, H, hd):
    """fp64 attention of the fp16 inputs.  Every tensor is [n][H][T][hd] except P, dS [n][H][T][T] and smax [n][H][T][1]."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in _split(qkv.cpu(), n, T, H, hd, torch.float64))
    do = heads_of(dout.cpu().double(), n, T, H, hd)
    sc = 1.0 / math.sqrt(hd)
    s = (q @ k.transpose(-1, -2)) * sc
    P = torch.softmax(s, dim=-1)
    out = P @ v
    out.backward(do)
    with torch.no_grad():
        P, s, out = P.detach(), s.detach(), out.detach()
        dS = P * (do @ v.transpose(-1, -2) - (do * out).sum(-1, keepdim=True))
        return dict(out=out, dq=q.grad, dk=k.grad, dv=v.grad, P=P, dS=dS, smax=s.abs().amax(-1, keepdim=True),
                    q=q.detach(), k=k.detach(), v=v.detach(), do=do, sc=sc)


def _store(ref):
    """one fp16 store: half an ulp, 2^-11 |ref| for a normal number and 2^-25 below 2^-14 (subnormal spacing 2^-24)"""
    return (2.0 ** -11 * ref.abs()).clamp(min=2.0 ** -25)


def attention_bounds(ref, c=None):
    c = C_EPS if c is None else c
    P, sc, do = ref["P"], ref["sc"], ref["do"].abs()
    aq, ak, av, adS = ref["q"].abs(), ref["k"].abs(), ref["v"].abs(), ref["dS"].abs()
    E = c * 2.0 ** -23 * ref["smax"].clamp(min=1.0)                    # [n][H][T][1], per query row
    PV = P @ av
    # an unnormalised probability p~ = P / max P below 2^-14 is an fp16 subnormal: absolute error 2^-25, whatever its size,
    # so 2^-25 |V_j| / sum p~ = 2^-25 |V_j| max P per such key (it counts where the dominant key's V is near 0)
    pmax = P.amax(-1, keepdim=True)
    sub = pmax * 2.0 ** -25 * ((P < 2.0 ** -14 * pmax).double() @ av)
    b_out = 2.0 ** -10 * PV + _store(ref["out"]) + E * PV + sub
    e = (do * b_out).sum(-1, keepdim=True)                             # |Delta error| per query row
    b_dq = sc * e * (P @ ak) + _store(ref["dq"]) + sc * ((E * adS) @ ak)
    b_dk = sc * ((P * e).transpose(-1, -2) @ aq) + _store(ref["dk"]) + sc * ((E * adS).transpose(-1, -2) @ aq)
    b_dv = _store(ref["dv"]) + (E * P).transpose(-1, -2) @ do
    return dict(out=b_out, dq=b_dq, dk=b_dk, dv=b_dv)


def attention_ratios(got, ref, bounds, names=("out", "dq", "dk", "dv")):
    """worst |got - ref| / bound per output ([n][H][T][hd] tensors); a non-finite value is an infinite ratio"""
    res = {}
    for k in names:
        g = got[k].double()
        if not bool(torch.isfinite(g).all()):
            res[k] = float("inf")
            continue
        err = (g - ref[k]).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bounds[k])
        res[k] = float(r.max()) if r.numel() else 0.0
    return res


# ------------------------------------------------------------------ fp32 emulation of the kernels (and of wrong ones)
def attention_emulation(qkv, dout, n, T, H, hd, reverse=False, bug=None, out16=None):
    """The kernels' arithmetic in fp32.  reverse: sum over keys (forward, dq) / queries (dk, dv) in reversed index order.
    bug: one of BUGS.  out16: the forward output the backward takes (default: the emulated one)."""
    assert bug is None or bug in BUGS
    q, k, v = (t.contiguous() for t in _split(qkv.cpu(), n, T, H, hd, torch.float32))
    do = heads_of(dout.cpu().float(), n, T, H, hd).contiguous()
    sc = 1.0 / math.sqrt(hd)
    if bug == "scale_d32" and hd == 32:
        sc = 0.125
    scf = torch.tensor(sc, dtype=torch.float32)

    def fwd(kk, vv):
        if reverse:
            kk, vv = kk.flip(-2), vv.flip(-2)
        s = q @ kk.transpose(-1, -2)                                    # raw fp32 scores
        c2 = scf * torch.tensor(1.4426950408889634, dtype=torch.float32)
        shift = -s.amax(-1, keepdim=True) * c2
        p = torch.exp2(s * c2 + shift)                                  # unnormalised
        return (((p.to(F16).float() @ vv) * (1.0 / p.sum(-1, keepdim=True))).to(F16))

    def pad(t, extra):
        return torch.cat([t, torch.zeros(n, H, extra, hd)], dim=2)
    kk, vv = k, v
    if bug == "pad_key":                                                # one zero key row leaks into every softmax
        kk, vv = pad(k, 1), pad(v, 1)
    o16 = fwd(kk, vv)
    if bug == "tile_unmasked" and T % 16:                               # query tile 0 sees the zero rows up to the tile's end
        o16[:, :, :16] = fwd(pad(k, 16 - T % 16), pad(v, 16 - T % 16))[:, :, :16]
    used = o16 if out16 is None else out16.cpu()

    # backward: fp32, natural exponential, P = exp(s - m) * (1 / l)
    s = (q @ kk.transpose(-1, -2)) * scf
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = (p.flip(-1) if reverse else p).sum(-1, keepdim=True)
    p = p * (1.0 / l)
    delta = (do * used.float()).sum(-1, keepdim=True)
    if bug == "delta_last":
        delta[:, :, T - 1] = 0.0
    dS = p * (do @ vv.transpose(-1, -2) - delta)
    if reverse:
        dq = dS.flip(-1) @ kk.flip(-2)
        dk = dS.flip(-2).transpose(-1, -2) @ q.flip(-2)
        dv = p.flip(-2).transpose(-1, -2) @ do.flip(-2)
    else:
        dq, dk, dv = dS @ kk, dS.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do
    dq, dk, dv = (dq * scf).to(F16), (dk[:, :, :T] * scf).to(F16), dv[:, :, :T].to(F16)
    if bug == "dk_swap8":
        dk[:, 0, :, :16] = torch.cat([dk[:, 0, :, 8:16], dk[:, 0, :, :8]], dim=-1)
    if bug == "dq_row_1p1":
        dq[0, :, T // 2] = (dq[0, :, T // 2].float() * 1.1).to(F16)      # one row of dq[M][D]: every head of one token
    return dict(out=o16, dq=dq, dk=dk, dv=dv)


# ------------------------------------------------------------------ LayerNorm-add, GEMM, weight gradient, column sums
def layernorm_add_ref(xs, gamma, beta, eps, act):
    """fp64 LayerNorm (+ erf-GELU) of the fp32 sum of the fp16 addends xs (x, then optional a, b)"""
    s = xs[0].float()
    for a in xs[1:]:
        s = s + a.float()
    ref = F.layer_norm(s.double(), (s.shape[-1],), gamma.double(), beta.double(), eps)
    return F.gelu(ref) if act else ref


def layernorm_add_fwd_errors(y32, y16, ref, scale=None):
    """the bound forms of test_layernorm_add_matches_torch: (fp32 output ok, fp16 output ok); scale = max |ref| of the call"""
    scale = float(ref.abs().max()) if scale is None else scale
    ok32 = float((y32.double().to(ref.device) - ref).abs().max()) <= 2e-6 * scale + 1e-6
    ok16 = bool(((y16.double().to(ref.device) - ref).abs() <= 2.0 ** -11 * ref.abs() + 2e-6 * scale + 2.0 ** -24).all())
    return ok32, ok16


def layernorm_add_bwd_ref(dy, dy_mul, xs, gamma, beta, act, eps, dtype=torch.float64):
    """autograd through LayerNorm (+ GELU) of v = sum of xs (fp32 sum of fp16), in `dtype`: (dv, dgamma, dbeta)"""
    v = xs[0].float()
    for a in xs[1:]:
        v = v + a.float()
    v = v.to(dtype).requires_grad_(True)
    gm, bt = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    y = F.layer_norm(v, (v.shape[-1],), gm, bt, eps)
    y = F.gelu(y) if act else y
    y.backward(dy.to(dtype) * dy_mul)
    return v.grad, gm.grad, bt.grad


def layernorm_add_bwd_gout_tol(ref, dv, f16_only):
    """test_layernorm_add_bwd_matches_fp32_autograd's bound on max |g_out - ref|; dv = the gradient without g_in"""
    sc = float(dv.abs().max())
    return 1e-4 * sc + (2.0 ** -11 if f16_only else 1e-5) * float(ref.abs().max())


def layernorm_add_bwd_param_tol(want, s, M):
    return 1e-4 * float((s * want).abs().max()) + 1e-4 * M ** 0.5


def gemm_bound(ref):
    return 2.0 ** -10 * ref.abs() + 2e-3


def wgrad_bound(dY, X, s):
    return 1e-4 * s * (dY.double().abs().t() @ X.double().abs()) + 1e-6


def colsum_bound(x, s):
    """fp32 sums of at most 4097 / 32 rows per lane chain, 32 lanes, then at most 256 slabs, each in a fixed order"""
    return 1e-5 * s * x.double().abs().sum(0) + 1e-6


def sample_rows(M, limit=20000, edge=300, k=4000):
    """all rows for small M; the first and last `edge` rows plus a seeded sample otherwise"""
    if M <= limit:
        return torch.arange(M)
    g = torch.Generator().manual_seed(M)
    return torch.cat([torch.arange(edge), torch.randint(0, M, (k,), generator=g), torch.arange(M - edge, M)])
