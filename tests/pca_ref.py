"""fp64 restatement, derived bounds, input families and wrong variants for the device PCA (csrc/pca_gram.hip,
isic_hip/pca.py).  Plain numpy on the CPU; shared by tests/test_pca_ref_cpu.py (the restatement equals sklearn on float64
input, the bounds admit a plain fp32 evaluation and reject the wrong variants kept here) and tests/test_pca_gpu.py (the
device is held to the same bounds on the same cases).

Restatement (isic_hip/pca.py, include/isic_hip_pca.h), everything in float64:
    z_m = x[r_m] - shift,   G = sum_m z_m z_m^T,   colsum = sum_m z_m                                  (gram)
    d = colsum / M,  mean = shift + d,  C = (G - M d d^T) / (M - 1)                                    (finish)
    eigh(C): eigenvalues clamped at 0, descending; the entry of largest magnitude of each component positive;
    a float n_components keeps searchsorted(cumsum(ratio), n_components, side="right") + 1 components   (fit)
    t = x c^T - mean c^T                                                                               (transform)

Error model.  u = 2^-24, gamma(n) = n u / (1 - n u).  Nothing below is fitted to a kernel's output.
  * Gram.  The device rounds z = x - shift once (relative u per factor, 2 u per product) and adds the products of a run of
    RUN = 2048 rows (ISIC_GRAM_RUN) in fp32: a chain of fused multiply-adds inside the MFMA accumulators, in any order
    within (n + 1) u sum|terms| as in tests/f32_kernel_ref.py.  The runs meet in fp64 (2^-53 per add, `runs` adds).  Per
    element:  |dG_ij| <= (gamma(RUN + 3) + runs 2^-52) sum_m |z_mi| |z_mj|.
    The column sums are fp32 sums of RUN / 8 = 256 terms per thread joined by 7 further adds, then fp64:
    |dcolsum_i| <= (gamma(RUN / 8 + 9) + runs 2^-52) sum_m |z_mi|.
  * Covariance.  Propagated with the product rule: E_d = E_colsum / M,
    E_C = (E_G + M (|d| E_d^T + E_d |d|^T + E_d E_d^T)) / (M - 1);  |dC| <= E_C elementwise, so ||dC||_2 <= ||E_C||_2.
    The host eigensolver (LAPACK, fp64) adds D 2^-52 ||C||_2.
  * Eigenvalues (Weyl): |dlambda_i| <= ||dC||_2, plus u lambda_i for the fp32 attribute.
  * Components (Davis-Kahan): ||dv_i||_2 <= 2 ||dC||_2 / gap_i with gap_i the distance of lambda_i to its neighbours
    (the first dropped eigenvalue included), plus u for the fp32 attribute.  Components whose bound exceeds 0.1 carry no
    information and may be left out (at most 10 % of the kept ones; none on the families here, asserted on the CPU).
  * mean: E_d + u |mean|.
  * Transform, against the DEVICE'S OWN fp32 components and mean so that the fit's error stays out of it:
    a length-D fp32 dot product, the bias -mean c^T formed in fp64 and rounded once, one add:
    |dt| <= gamma(D + 3) (sum_j |x_j| |c_j| + |b|).
"""
import numpy as np

U = 2.0 ** -24
RUN = 2048                       # ISIC_GRAM_RUN of include/isic_hip_pca.h: the documented fp32 run length
SEED = 4321
DK_CAP = 0.1                     # a Davis-Kahan bound above this says nothing about the component
DK_SHARE = 0.10                  # at most this share of the kept components may be left out

FIT_SHAPES = ((5000, 64), (3000, 256), (300, 64), (40, 64), (65, 64))
DEVICE_FIT_SHAPES = ((5000, 64), (3000, 256), (40, 64), (65, 64))
GRAM_D = (4, 20, 64, 132, 768, 1024)
GRAM_M = (1, 2, 7, 63, 64, 65, 1000)
GRAM_RUN_M = (RUN - 1, RUN, RUN + 1, 2 * RUN + 3)     # at D = 64
BUGS = ("uncentred", "rows_ignored", "last_run_dropped", "not_mirrored", "divisor_m", "sign_first", "side_left")


def gamma(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------- input families
def family(M, D, seed=0, decay=0.7):
    """fp32 [M, D]: a geometrically decaying spectrum rotated by a random orthogonal matrix, plus a mean of 3 sigma."""
    rng = np.random.default_rng(SEED + 7919 * seed + 31 * M + D)
    sig = np.sqrt(decay ** np.arange(D))
    Q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    x = (rng.standard_normal((M, D)) * sig) @ Q.T + 3.0 * sig[0] * np.sign(rng.standard_normal(D))
    return x.astype(np.float32)


def rows_for(M, seed=0):
    """an int32 index with gaps and one repeated row: about two thirds of the rows, ascending, row 0 of it repeated"""
    rng = np.random.default_rng(SEED + 13 * seed + M)
    keep = np.nonzero(rng.random(M) < 0.66)[0]
    if keep.size == 0:
        keep = np.array([M - 1])
    return np.concatenate([keep, keep[:1]]).astype(np.int32)


def conditions(fit, n_components=0.90):
    """(smallest relative gap between neighbouring kept eigenvalues incl. the first dropped one, margin of the cumulative
    ratio around n_components) -- the families must give >= 1e-3 and >= 1e-4"""
    lam, k = fit["eigenvalues"], fit["k"]
    gaps = -np.diff(lam[:k + 1]) / lam[0]
    cum = np.cumsum(lam / lam.sum())
    return float(gaps.min()), float(np.abs(cum - n_components).min())


# ---------------------------------------------------------------------------------------------------- restatement
def gram_eval(x, rows=None, shift=None, dtype=np.float64, bug=None):
    """float64: the reference.  float32: a plain fp32 evaluation with the device's accumulation scheme (fp32 inside runs
    of RUN rows, fp64 across).  -> (G [D, D] float64, colsum [D] float64)"""
    if bug == "rows_ignored":
        rows = None if rows is None else np.arange(len(rows))
    xs = x if rows is None else x[rows]
    sh = np.zeros(x.shape[1], dtype=x.dtype) if (shift is None or bug == "uncentred") else shift
    z = xs.astype(dtype) - sh.astype(dtype)
    D = x.shape[1]
    G, cs = np.zeros((D, D)), np.zeros(D)
    M = z.shape[0]
    stop = M - (M % RUN if M % RUN else RUN) if bug == "last_run_dropped" else M
    for m0 in range(0, stop, RUN):
        zr = z[m0:min(m0 + RUN, stop)]
        G += (zr.T @ zr).astype(np.float64)
        cs += zr.sum(axis=0, dtype=dtype).astype(np.float64)
    if bug == "not_mirrored":
        G = np.triu(G)
    return G, cs


def gram_bound(x, rows=None, shift=None, shift_err=None):
    """(E_G [D, D], E_colsum [D]) of the module docstring; `shift_err` [D]: how far the shift the device used may lie
    from `shift` (it only widens |z|)"""
    xs = (x if rows is None else x[rows]).astype(np.float64)
    az = np.abs(xs - (0.0 if shift is None else shift.astype(np.float64)))
    if shift_err is not None:
        az = az + shift_err
    runs = -(-xs.shape[0] // RUN)
    return (gamma(RUN + 3) + runs * 2.0 ** -52) * (az.T @ az), (gamma(RUN // 8 + 9) + runs * 2.0 ** -52) * az.sum(axis=0)


def finish(G, colsum, shift, M, bug=None):
    d = colsum / M
    mean = (0.0 if shift is None else shift.astype(np.float64)) + d
    C = (G - M * np.outer(d, d)) / (M if bug == "divisor_m" else M - 1)
    return mean, C


def fit_from_cov(C, n_components=0.90, bug=None):
    lam, vec = np.linalg.eigh(C)
    lam, comps = np.maximum(lam[::-1], 0.0), np.ascontiguousarray(vec[:, ::-1].T)
    idx = np.zeros(len(comps), dtype=np.int64) if bug == "sign_first" else np.argmax(np.abs(comps), axis=1)
    s = np.sign(comps[np.arange(len(comps)), idx])
    comps = comps * np.where(s == 0, 1.0, s)[:, None]
    ratio = lam / lam.sum() if lam.sum() > 0 else np.zeros_like(lam)
    if isinstance(n_components, float):
        k = int(np.searchsorted(np.cumsum(ratio), n_components, side="left" if bug == "side_left" else "right")) + 1
    else:
        k = int(n_components)
    k = max(1, min(k, len(lam)))
    return {"eigenvalues": lam, "all_components": comps, "k": k, "components": comps[:k], "explained_variance": lam[:k],
            "explained_variance_ratio": ratio[:k]}


def fit_eval(x, rows=None, n_components=0.90, dtype=np.float64, bug=None, shift=None):
    """the whole fit; `shift` defaults to the fp32 column mean of the fitted rows (what a single partial_fit uses)"""
    xs = x if rows is None else x[rows]
    if shift is None:
        shift = xs.astype(np.float64).mean(axis=0).astype(np.float32)
    G, cs = gram_eval(x, rows, shift, dtype, bug)
    mean, C = finish(G, cs, shift, xs.shape[0], bug)
    out = fit_from_cov(C, n_components, bug)
    out.update(mean=mean, C=C, G=G, colsum=cs, shift=shift, M=xs.shape[0])
    return out


def transform_eval(x, components, mean, rows=None, dtype=np.float64):
    xs = (x if rows is None else x[rows]).astype(dtype)
    c = components.astype(dtype)
    b = (-(components.astype(np.float64) @ mean.astype(np.float64))).astype(dtype)      # formed in fp64, rounded once
    return xs @ c.T + b


def transform_bound(x, components, mean, rows=None):
    xs = np.abs((x if rows is None else x[rows]).astype(np.float64))
    c = np.abs(components.astype(np.float64))
    b = np.abs(components.astype(np.float64) @ mean.astype(np.float64))
    return gamma(x.shape[1] + 3) * (xs @ c.T + b)


# ---------------------------------------------------------------------------------------------------- fit bounds
def cov_err_norm(x, rows, ref, shift_err=None):
    """||E_C||_2 + the eigensolver's share, and E_d (module docstring)"""
    EG, Ec = gram_bound(x, rows, ref["shift"], shift_err)
    M = ref["M"]
    d = np.abs(ref["colsum"] / M)
    Ed = Ec / M
    EC = (EG + M * (np.outer(d, Ed) + np.outer(Ed, d) + np.outer(Ed, Ed))) / (M - 1)
    return float(np.linalg.norm(EC, 2) + x.shape[1] * 2.0 ** -52 * np.linalg.norm(ref["C"], 2)), Ed


def fit_bounds(x, rows, ref, shift_err=None):
    """-> dict: eigenvalues [k], components [k] (2-norm of the difference of a component), mean [D], checked [k] bool"""
    nC, Ed = cov_err_norm(x, rows, ref, shift_err)
    lam, k = ref["eigenvalues"], ref["k"]
    lo = lam[:k] - lam[1:k + 1] if k < len(lam) else np.append(lam[:k - 1] - lam[1:k], np.inf)
    up = np.append(np.inf, lam[:k - 1] - lam[1:k])
    gap = np.minimum(lo, up)
    with np.errstate(divide="ignore"):
        comp = 2.0 * nC / gap + np.sqrt(x.shape[1]) * U
    return {"norm": nC, "eigenvalues": nC + U * lam[:k], "components": comp, "checked": comp <= DK_CAP,
            "mean": Ed + U * np.abs(ref["mean"])}


def fit_ratios(got, ref, bounds):
    """worst error / bound of a fit `got` (dict with eigenvalue / component / mean arrays of any float dtype)"""
    k = ref["k"]
    if got["k"] != k:
        return {"k": np.inf}
    ev = np.abs(np.asarray(got["explained_variance"], dtype=np.float64) - ref["explained_variance"]) / bounds["eigenvalues"]
    dc = np.linalg.norm(np.asarray(got["components"], dtype=np.float64) - ref["components"], axis=1) / bounds["components"]
    mn = np.abs(np.asarray(got["mean"], dtype=np.float64) - ref["mean"]) / bounds["mean"]
    keep = bounds["checked"]
    return {"k": 0.0, "eigenvalues": float(ev.max()), "components": float(dc[keep].max()) if keep.any() else 0.0,
            "mean": float(mn.max())}


def worst(r):
    return max(r.values())


def ratio(got, ref, bound):
    """worst |got - ref| / bound (0 / 0 = 0; NaN counts as inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------- gap-independent checks
def output_checks(X, T, first, Xt=None, Tt=None, n_components=0.90):
    """Checks of a fitted-and-transformed output that hold whatever the eigen-gaps are (an encoder's latents give no control
    over them).  X [M, D] fp32: the fitted rows; T [M, k]: their transform; first [M] bool: the rows of the first
    partial_fit, whose fp32 column mean (an fp32 sum of n1 terms) is the shift the fit used; Xt [Mt, D], Tt [Mt, k]: rows
    that were only transformed (optional).  Everything is computed in fp64 from X.
    -> (k_ok, covariance error / bound, residual error / bound, transformed-only rows error / bound or None)
      * k is the reference's count unless the cumulative ratio passes n_components within the eigenvalue bound.
      * The columns of T are uncorrelated with variances lambda_i.  With V the fitted components (eigenvectors of C + dC) and e
        the transform's own error, cov(T) = Lambda_hat - V dC V^T + cross terms: every entry is within 2 ||dC||_2 (Weyl and the
        dC term) + 4 u lambda_1 (fp32 components) + the Cauchy-Schwarz bound of the cross terms, e being bounded by the
        length-D fp32 dot product on |x| |c| <= ||x||_2 (||c||_2 = 1).  e_rms is its root mean square over the rows.
      * Reconstruction.  r = ||Xc - Tc (Tc^T Tc)^-1 Tc^T Xc||_F^2 / (M - 1), the energy the best linear map from the output
        back to the centred input leaves, row by row: a permutation of the rows of T destroys it.  Tc B has rank k, so
        r >= sum_{i>k} lambda_i exactly (Eckart-Young); and with B = V:  sqrt(r) <= ||Xc (I - V^T V)||_F / sqrt(M - 1) + sqrt(k)
        e_rms (1 + u sqrt(D)),  ||Xc (I - V^T V)||_F^2 / (M - 1) = trace(C) - trace(V C V^T) <= sum_{i>k} lambda_i + 2 k ||dC||_2
        + 4 k u lambda_1.  The check is one-sided by nature: below the floor only by fp64 rounding (1e-10 trace(C)).
      * Rows that were only transformed must be the same map of their inputs.  The map is recovered from the fitted rows:
        B = (Tc^T Tc)^-1 Tc^T Xc = V - Lambda_hat^-1 V dC + O(e).  With e_j the first j columns of e and
        cross_j = sqrt(j lambda_1) e_rms >= ||e_j^T Xc||_2 / (M - 1)  (||A^T B||_2 <= ||A||_F ||B||_2), the first j rows B_j are
        within  delta_j = (||dC||_2 + 4 u lambda_1 + 3 cross_j) / (lambda_j - 2 ||dC||_2 - 2 cross_j)  of V_j, and pinv(B_j)
        within 1.618 delta_j / (1 - delta_j) of V_j^T (Wedin).  The recovery divides by
        lambda_j, so it is made on the leading k1 columns only, those with delta_j < 0.05 (the output's columns are
        uncorrelated, so the leading columns are a fit of their own; k1 >= 1 is asserted).  Row by row:
        ||(tt - tbar)[:k1] - (xt - xbar) pinv(B_k1)||_2 <= 1.618 delta / (1 - delta) ||xt - xbar||_2 + sqrt(k1) (row bound of e +
        e_rms), independent of every gap and tied to the order of the rows."""
    M, D = X.shape
    T = np.asarray(T, dtype=np.float64)
    k = T.shape[1]
    X64 = X.astype(np.float64)
    n1 = int(first.sum())
    shift = X64[first].mean(axis=0)
    ref = fit_eval(X, shift=shift.astype(np.float32))
    shift_err = gamma(n1 + 2) * np.abs(X64[first]).mean(axis=0) + np.abs(shift - ref["shift"])
    nC, _ = cov_err_norm(X, None, ref, shift_err)
    lam = ref["eigenvalues"]
    cum = np.cumsum(lam) / lam.sum()
    slack = 2.0 * D * nC / lam.sum()
    k_ok = bool(cum[k - 1] > n_components - slack and (k == 1 or cum[k - 2] <= n_components + slack))
    xbar = X64.mean(axis=0)
    mean_norm = np.sqrt((xbar ** 2).sum())
    e_row = lambda Z: gamma(D + 3) * (np.sqrt((Z ** 2).sum(axis=1)) + mean_norm) * (1.0 + U * np.sqrt(D))      # noqa: E731
    e_rms = np.sqrt((e_row(X64) ** 2).sum() / (M - 1))
    sd = np.sqrt(lam[:k] + nC)
    cov = np.cov(T, rowvar=False).reshape(k, k)
    bound = 2.0 * nC + 4.0 * U * lam[0] + (sd[:, None] + sd[None, :]) * e_rms + e_rms ** 2
    r_cov = ratio(cov, np.diag(lam[:k]), bound)
    # reconstruction residual
    Xc, Tc = X64 - xbar, T - T.mean(axis=0)
    B = np.linalg.lstsq(Tc, Xc, rcond=None)[0]                          # [k, D]
    res = ((Xc - Tc @ B) ** 2).sum() / (M - 1)
    floor = lam[k:].sum()
    ceil = (np.sqrt(floor + 2.0 * k * nC + 4.0 * k * U * lam[0]) + np.sqrt(k) * e_rms * (1.0 + U * np.sqrt(D))) ** 2
    trC = float(np.trace(ref["C"]))
    r_res = max((res - floor) / (ceil - floor), (floor - res) / (1e-10 * trC))
    r_t = None
    if Xt is not None:
        cross = np.sqrt(np.arange(1, k + 1) * (lam[0] + nC)) * e_rms
        den = lam[:k] - 2.0 * nC - 2.0 * cross
        dl = np.where(den > 0, (nC + 4.0 * U * lam[0] + 3.0 * cross) / np.where(den > 0, den, 1.0), np.inf)
        k1 = int(np.argmax(dl >= 0.05)) if (dl >= 0.05).any() else k
        assert k1 >= 1, dl[:3]
        delta = dl[k1 - 1]
        Xtc = Xt.astype(np.float64) - xbar
        pred = Xtc @ np.linalg.pinv(B[:k1]) + T.mean(axis=0)[:k1]
        err = np.sqrt(((np.asarray(Tt, dtype=np.float64)[:, :k1] - pred) ** 2).sum(axis=1))
        bt = 1.618 * delta / (1.0 - delta) * np.sqrt((Xtc ** 2).sum(axis=1)) \
            + np.sqrt(k1) * (e_row(Xt.astype(np.float64)) + e_rms)
        r_t = float((err / bt).max()) if len(err) else 0.0
    return k_ok, r_cov, float(r_res), r_t


# ---------------------------------------------------------------------------------------------------- shared fit cases
_CASES = {}


def fit_case(M, D, with_rows):
    """(x, rows, reference fit) of a family member, computed once.  The sample spectrum of a random matrix is random: the
    seed is advanced until the REFERENCE meets the conditions the comparison needs (gaps >= 1e-3 lambda_1, margin >= 1e-4,
    every Davis-Kahan bound <= DK_CAP) -- a choice of input, made before any device or fp32 result exists."""
    key = (M, D, bool(with_rows))
    if key not in _CASES:
        for seed in range(64):
            x = family(M, D, seed)
            rows = rows_for(M, seed) if with_rows else None
            ref = fit_eval(x, rows)
            gap, margin = conditions(ref)
            if gap >= 1e-3 and margin >= 1e-4 and fit_bounds(x, rows, ref)["checked"].all():
                break
        else:
            raise AssertionError(f"no family member for {key}")
        _CASES[key] = (x, rows, ref)
    return _CASES[key]
