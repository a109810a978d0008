"""The fixed inputs of tests/test_ln_rows_gpu.py and of tools/gen_ln_rows_bits.py, and the SHA-256 digests of what the
fp16 row-LayerNorm entry points (and the entries that share their MXFP8 tail) write for them.

Inputs come from numpy.random.Generator(PCG64(seed)), so their bytes do not depend on the torch version; every case has
a row of equal values (row 1) and a row with a 300.0 outlier (row 2) in each fp16 / fp32 input -- the two mean rules
(s * (1 / N) and s / N) differ on exactly such rows.  M = 37 is no multiple of the 4, 8 or 16 rows a block takes per
pass, so every layout's tail block runs; the large cases exceed each layout's grid cap with a ragged last pass (their
rows repeat a 1021-row base, a prime period, gathered on the device)."""
import hashlib

import numpy as np
import torch

DEV = "cuda:0"
M_SMALL = 37
VIT_WIDTHS = (128, 256, 384, 512)
ADD_WIDTHS = (64, 384, 512, 576, 1024)        # one lane group; CPL 1; CPL 1 full; CPL 2, second piece partly off; CPL 2 full
M_BIG_VIT = 8192 * 64 + 3                     # N = 128: 16 rows per block and pass, grid capped at 8192
M_BIG_ADD = 8192 * 16 + 5                     # one wave per row: 4 rows per block and pass, grid capped at 8192
M_BIG_MX = 8192 * 16 + 5                      # N = 384: 4 rows per block and pass
BASE_ROWS = 1021
EPS = 1e-6


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _rows(rng, m, n, dtype=np.float16, outlier_col=5):
    x = rng.standard_normal((m, n), dtype=np.float32)
    x[1, :] = 0.3
    x[2, outlier_col % n] = 300.0
    return x.astype(dtype)


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(DEV)


def _big(base, m):
    """rows base[i % BASE_ROWS], i < m, gathered on the device (integer indexing only)"""
    return base[torch.arange(m, device=DEV) % base.shape[0]].contiguous()


def _affine(rng, n):
    gamma = (1.0 + 0.25 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    beta = (0.25 * rng.standard_normal(n, dtype=np.float32)).astype(np.float32)
    return _dev(gamma), _dev(beta)


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _out(shape, dtype):
    return torch.zeros(shape, device=DEV, dtype=dtype)


def _vit(out):
    for n in VIT_WIDTHS:
        rng = np.random.Generator(np.random.PCG64(1000 + n))
        x = _dev(_rows(rng, M_SMALL, n))
        gamma, beta = _affine(rng, n)
        y, y32 = _out((M_SMALL, n), torch.int16), _out((M_SMALL, n), torch.float32)
        _call("isic_layernorm_f16", x, gamma, beta, y, y32, M_SMALL, n, EPS)
        out[f"isic_layernorm_f16/N{n}/M{M_SMALL}:y"] = _sha(y)
        out[f"isic_layernorm_f16/N{n}/M{M_SMALL}:y_f32"] = _sha(y32)
        st = _out((M_SMALL, 2), torch.float32)
        _call("isic_row_stats_f16", x, st, M_SMALL, n, EPS)
        out[f"isic_row_stats_f16/N{n}/M{M_SMALL}:stats"] = _sha(st)
        if n == 384:
            q, s = _out((M_SMALL, n), torch.uint8), _out((M_SMALL, n // 32), torch.uint8)
            _call("isic_layernorm_mxfp8_f16", x, gamma, beta, q, s, M_SMALL, n, EPS)
            out[f"isic_layernorm_mxfp8_f16/N{n}/M{M_SMALL}:q"] = _sha(q)
            out[f"isic_layernorm_mxfp8_f16/N{n}/M{M_SMALL}:s"] = _sha(s)
    # past the grid cap
    n, m = 128, M_BIG_VIT
    rng = np.random.Generator(np.random.PCG64(2000 + n))
    x = _big(_dev(_rows(rng, BASE_ROWS, n)), m)
    gamma, beta = _affine(rng, n)
    y = _out((m, n), torch.int16)
    _call("isic_layernorm_f16", x, gamma, beta, y, None, m, n, EPS)
    out[f"isic_layernorm_f16/N{n}/M{m}:y"] = _sha(y)
    del y
    st = _out((m, 2), torch.float32)
    _call("isic_row_stats_f16", x, st, m, n, EPS)
    out[f"isic_row_stats_f16/N{n}/M{m}:stats"] = _sha(st)
    del x, st
    n, m = 384, M_BIG_MX
    rng = np.random.Generator(np.random.PCG64(2000 + n))
    x = _big(_dev(_rows(rng, BASE_ROWS, n)), m)
    gamma, beta = _affine(rng, n)
    q, s = _out((m, n), torch.uint8), _out((m, n // 32), torch.uint8)
    _call("isic_layernorm_mxfp8_f16", x, gamma, beta, q, s, m, n, EPS)
    out[f"isic_layernorm_mxfp8_f16/N{n}/M{m}:q"] = _sha(q)
    out[f"isic_layernorm_mxfp8_f16/N{n}/M{m}:s"] = _sha(s)


def _bwd(out, tag, dy, dy_f32, x, a, b, gamma, beta, act, g_in, m, n):
    ws_bytes = _call("isic_layernorm_add_bwd_f16_workspace_bytes", m, n)
    ws = _out((ws_bytes // 4,), torch.float32)
    g_out, g_out16 = _out((m, n), torch.float32), _out((m, n), torch.int16)
    dgamma, dbeta = _out((n,), torch.float32), _out((n,), torch.float32)
    _call("isic_layernorm_add_bwd_f16", dy, dy_f32, 0.75, x, a, b, gamma, beta, act, EPS, g_in, g_out, g_out16, dgamma,
          dbeta, m, n, 0.5, 0, ws, ws_bytes)
    for name, t in (("g_out", g_out), ("g_out16", g_out16), ("dgamma", dgamma), ("dbeta", dbeta)):
        out[f"isic_layernorm_add_bwd_f16/{tag}:{name}"] = _sha(t)


def _add(out):
    m = M_SMALL
    for n in ADD_WIDTHS:
        rng = np.random.Generator(np.random.PCG64(3000 + n))
        x = _dev(_rows(rng, m, n))
        a = _dev(_rows(rng, m, n, outlier_col=17))
        b = _dev(_rows(rng, m, n, outlier_col=40))
        gamma, beta = _affine(rng, n)
        dy16 = _dev(_rows(rng, m, n, outlier_col=9))
        dy32 = _dev(_rows(rng, m, n, np.float32, outlier_col=9))
        g_in = _dev(_rows(rng, m, n, np.float32, outlier_col=3))
        for act in (0, 1):
            for add in (0, 1):
                aa, bb = (a, b) if add else (None, None)
                tag = f"N{n}/M{m}/act{act}/add{add}"
                y, y32 = _out((m, n), torch.int16), _out((m, n), torch.float32)
                _call("isic_layernorm_add_f16", x, aa, bb, gamma, beta, y, y32, m, n, act, EPS)
                out[f"isic_layernorm_add_f16/{tag}:y"] = _sha(y)
                out[f"isic_layernorm_add_f16/{tag}:y_f32"] = _sha(y32)
                for dy_f32 in (0, 1):
                    for gi in (0, 1):
                        _bwd(out, f"{tag}/dyf32_{dy_f32}/gin{gi}", dy32 if dy_f32 else dy16, dy_f32, x, aa, bb, gamma, beta,
                             act, g_in if gi else None, m, n)
            q, s = _out((m, n), torch.uint8), _out((m, n // 32), torch.uint8)
            _call("isic_layernorm_act_mxfp8_f16", x, gamma, beta, q, s, m, n, act, EPS)
            out[f"isic_layernorm_act_mxfp8_f16/N{n}/M{m}/act{act}:q"] = _sha(q)
            out[f"isic_layernorm_act_mxfp8_f16/N{n}/M{m}/act{act}:s"] = _sha(s)
    # past the grid cap
    n, m = 64, M_BIG_ADD
    rng = np.random.Generator(np.random.PCG64(4000 + n))
    x = _big(_dev(_rows(rng, BASE_ROWS, n)), m)
    a = _big(_dev(_rows(rng, BASE_ROWS, n, outlier_col=17)), m)
    b = _big(_dev(_rows(rng, BASE_ROWS, n, outlier_col=40)), m)
    dy16 = _big(_dev(_rows(rng, BASE_ROWS, n, outlier_col=9)), m)
    gamma, beta = _affine(rng, n)
    tag = f"N{n}/M{m}/act1/add1"
    y, y32 = _out((m, n), torch.int16), _out((m, n), torch.float32)
    _call("isic_layernorm_add_f16", x, a, b, gamma, beta, y, y32, m, n, 1, EPS)
    out[f"isic_layernorm_add_f16/{tag}:y"] = _sha(y)
    out[f"isic_layernorm_add_f16/{tag}:y_f32"] = _sha(y32)
    _bwd(out, f"{tag}/dyf32_0/gin0", dy16, 0, x, a, b, gamma, beta, 1, None, m, n)
    q, s = _out((m, n), torch.uint8), _out((m, n // 32), torch.uint8)
    _call("isic_layernorm_act_mxfp8_f16", x, gamma, beta, q, s, m, n, 1, EPS)
    out[f"isic_layernorm_act_mxfp8_f16/N{n}/M{m}/act1:q"] = _sha(q)
    out[f"isic_layernorm_act_mxfp8_f16/N{n}/M{m}/act1:s"] = _sha(s)


def _mx_tail(out):
    """the entries that share only the MXFP8 tail (four-lane amax, exponent, element bytes, scale byte)"""
    rng = np.random.Generator(np.random.PCG64(5000))
    m, k = M_SMALL, 96
    for f32 in (0, 1):
        x = _rows(rng, m, k, np.float32 if f32 else np.float16)
        x[3, 32:64] = 0                                       # an all-zero block
        q, s = _out((m, k), torch.uint8), _out((m, k // 32), torch.uint8)
        _call("isic_mxfp8_quantize", _dev(x), f32, q, s, m, k)
        out[f"isic_mxfp8_quantize/K{k}/M{m}/f32_{f32}:q"] = _sha(q)
        out[f"isic_mxfp8_quantize/K{k}/M{m}/f32_{f32}:s"] = _sha(s)
    nimg, h, w, c = 2, 9, 11, 64                              # ragged tiles in both directions
    x = _dev(_rows(rng, nimg * h * w, c))
    taps = _dev((0.2 * rng.standard_normal((25, c), dtype=np.float32)).astype(np.float32))
    bias = _dev((0.2 * rng.standard_normal(c, dtype=np.float32)).astype(np.float32))
    q, s = _out((nimg * h * w, c), torch.uint8), _out((nimg * h * w, c // 32), torch.uint8)
    _call("isic_dwconv5x5_mxfp8_f16", x, taps, bias, q, s, nimg, h, w, c)
    out[f"isic_dwconv5x5_mxfp8_f16/{nimg}x{h}x{w}x{c}:q"] = _sha(q)
    out[f"isic_dwconv5x5_mxfp8_f16/{nimg}x{h}x{w}x{c}:s"] = _sha(s)


GROUPS = {"vit": _vit, "add": _add, "mx_tail": _mx_tail}


def digests(group):
    """{case:buffer -> sha256 hex} of one group of entries on this device's library"""
    out = {}
    GROUPS[group](out)
    torch.cuda.synchronize()
    return out
