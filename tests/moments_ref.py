"""fp64 restatement, derived per-element bounds, cases and wrong variants for the token statistics
(csrc/token_moments.hip, isic_hip/moments.py, utils.concat_patch_moments).  Plain numpy on the CPU; shared by
tests/test_moments_ref_cpu.py (the reference's recorded outputs and a plain fp32 torch evaluation lie inside the bounds,
every wrong variant kept here lies outside) and tests/test_moments_gpu.py (the device is held to the same bounds), and by
tools/moments_bench.py (``torch_composition``: what a user would run without the entry).

Restatement (include/isic_hip_moments.h), everything in float64, per image b and channel d over the T tokens x_t:
    mean = sum x_t / T,  c_t = x_t - mean,  S_k = sum c_t^k  (k = 2, 3, 4)
    max  = max x_t                       median = sort(x)[(T - 1) // 2]          (input elements: bound 0)
    std  = sqrt(S_2 / (T - unbiased)),   sigma = max(std, fp32(eps))
    skew = (S_3 / T) / sigma^3,          kurtosis = (S_4 / T) / sigma^4 - 3
    out[b] = [mean | max | std | median | skew | kurtosis], each D wide.

Error model for an fp32 evaluation that adds its T terms in ANY order.  u = 2^-24, gamma(n) = n u / (1 - n u).  Nothing
below is fitted to a kernel's output.
  * mean: a T-term sum, |d sum| <= gamma(T) sum |x_t|, and one division:  e_m = gamma(T) sum |x_t| / T + u |mean|.
    This is where a large common offset enters: e_m ~ T u |offset|.
  * c_t = fl(x_t - mean^) inherits it:  e_c = e_m + u (|c_t| + e_m).  a_t = |c_t| + e_c bounds the computed |c_t|.
  * powers.  |c^^k - c^k| <= a^k - |c|^k exactly (the SECOND and higher orders are kept: on a constant column c = 0 and
    a^k = e_c^k is the whole error), and the k - 1 multiplications round at most k times in any association, fused or not:
    e_k,t = a_t^k - |c_t|^k + 1.01 k u a_t^k.
  * S_k: the term errors plus the summation, gamma(T) sum a_t^k (1 + 1.01 k u):  E_k.
  * var = S_2 / (T - unbiased): E_var = E_2 / n (1 + u) + u var.  std = sqrt(var): the exact interval
    [max(var - E_var, 0), var + E_var] is mapped through the square root (first order is useless at var ~ 0), plus 2 u of
    the upper end for the root itself.
  * sigma = max(std, eps): max is 1-Lipschitz and eps is exact, so E_sigma = E_std -- and the computed sigma is never
    below eps, which keeps the interval of sigma^k away from zero: [max(sigma - E, eps)^k (1 - (k + 2) u),
    (sigma + E)^k (1 + (k + 2) u)] (k + 2 roundings cover repeated products and a pow within 2 ulp).
  * m_k = S_k / T: E_k / T (1 + u) + u |m_k|.  The quotient m_k / sigma^k is monotone in either argument, so its error is
    the largest distance from the exact value over the four corners of the two intervals, plus u of the largest corner for
    the division; the kurtosis adds u (|q| + E + 3) for the subtraction.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U = 2.0 ** -24
EPS = 1e-6
STATS = ("mean", "max", "std", "median", "skew", "kurtosis")
EXACT = (1, 3)                   # max and median: selections, bound 0
MAX_T = 1024                     # ISIC_MOMENTS_MAX_T
SLAB_SWITCH_T = (256, 512)       # the slab width changes above these T (include/isic_hip_moments.h)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "patch_moments.npz")


def gamma(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------- restatement
def reference(x, eps=EPS, unbiased=False, bug=None):
    """x [B, T, D] (any float dtype) -> [B, 6 D] float64.  ``bug``: one of ``BUGS``, a wrong variant."""
    x = np.asarray(x, dtype=np.float64)
    B, T, D = x.shape
    e = float(np.float32(eps))
    if bug == "unbiased_swapped":
        unbiased = not unbiased
    n = T - (1 if unbiased else 0)
    mean = x.sum(axis=1) / T
    c = x - mean[:, None, :]
    mx = np.abs(x).max(axis=1) if bug == "max_abs" else x.max(axis=1)
    srt = np.sort(x, axis=1)
    if bug == "upper_median":
        med = srt[:, T // 2]
    elif bug == "mid_mean":
        med = 0.5 * (srt[:, (T - 1) // 2] + srt[:, T // 2])
    else:
        med = srt[:, (T - 1) // 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.sqrt((c ** 2).sum(axis=1) / n) if n > 0 else np.full((B, D), np.nan)
        sig = std if bug == "sigma_unclamped" else np.maximum(std, e)
        skew = (c ** 3).sum(axis=1) / T / (sig ** 2 if bug == "skew_over_variance" else sig ** 3)
        kurt = (c ** 4).sum(axis=1) / T / sig ** 4 - (0.0 if bug == "kurtosis_plus_3" else 3.0)
    parts = [mean, mx, std, med, skew, kurt]
    if bug == "order":
        parts = [mean, std, mx, med, skew, kurt]
    return np.concatenate(parts, axis=1)


BUGS = ("upper_median", "mid_mean", "unbiased_swapped", "sigma_unclamped", "kurtosis_plus_3", "skew_over_variance",
        "max_abs", "order")


def _quotient_bound(m, Em, sig, Es, e, k):
    lo = np.maximum(sig - Es, e) ** k * (1.0 - (k + 2) * U)
    hi = (sig + Es) ** k * (1.0 + (k + 2) * U)
    q0 = m / sig ** k
    err = np.zeros_like(m)
    big = np.zeros_like(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        for num in (m - Em, m + Em):
            for den in (lo, hi):
                q = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.inf)
                err = np.maximum(err, np.abs(q - q0))
                big = np.maximum(big, np.abs(q))
    return err + U * big


def bounds(x, eps=EPS, unbiased=False):
    """-> [B, 6 D] float64: the per-element bound of the module docstring (0 for max and median)."""
    x = np.asarray(x, dtype=np.float64)
    B, T, D = x.shape
    e = float(np.float32(eps))
    n = T - (1 if unbiased else 0)
    mean = x.sum(axis=1) / T
    c = np.abs(x - mean[:, None, :])
    em = gamma(T) * np.abs(x).sum(axis=1) / T + U * np.abs(mean)
    ec = em[:, None, :] + U * (c + em[:, None, :])
    a = c + ec
    S, E = {}, {}
    for k in (2, 3, 4):
        ak = a ** k
        S[k] = ((x - mean[:, None, :]) ** k).sum(axis=1)
        E[k] = (ak - c ** k + 1.01 * k * U * ak).sum(axis=1) + gamma(T) * (1.0 + 1.01 * k * U) * ak.sum(axis=1)
    var = S[2] / n
    Ev = E[2] / n * (1.0 + U) + U * var
    std = np.sqrt(var)
    hi = np.sqrt(var + Ev)
    lo = np.sqrt(np.maximum(var - Ev, 0.0))
    Es = np.maximum(std - lo, hi - std) + 2.0 * U * hi
    sig = np.maximum(std, e)
    m3, m4 = S[3] / T, S[4] / T
    Eskew = _quotient_bound(m3, E[3] / T * (1.0 + U) + U * np.abs(m3), sig, Es, e, 3)
    Eq4 = _quotient_bound(m4, E[4] / T * (1.0 + U) + U * np.abs(m4), sig, Es, e, 4)
    Ekurt = Eq4 + U * (np.abs(m4 / sig ** 4) + Eq4 + 3.0)
    z = np.zeros_like(em)
    return np.concatenate([em, z, Es, z, Eskew, Ekurt], axis=1)


def ratios(got, ref, bound):
    """[B, 6 D] of |got - ref| / bound (0 / 0 = 0; a NaN or an error above a zero bound counts as inf)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / bound
    r = np.where(err == 0, 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


def worst(got, ref, bound):
    r = ratios(got, ref, bound)
    return float(r.max()) if r.size else 0.0


def worst_per_stat(got, ref, bound):
    r = ratios(got, ref, bound)
    D = r.shape[1] // 6
    return {s: float(r[:, i * D:(i + 1) * D].max()) for i, s in enumerate(STATS)}


def selections_equal(got, ref):
    """max and median compared with == as numbers"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    D = ref.shape[1] // 6
    return all(bool((got[:, i * D:(i + 1) * D] == ref[:, i * D:(i + 1) * D]).all()) for i in EXACT)


# ---------------------------------------------------------------------------------------------------- inputs
def _ftensor(shape, **kw):
    from oracle.formula import ftensor
    return ftensor(shape, **kw).numpy()


def _no_negative_zero(x):
    return (x + np.float32(0.0)).astype(np.float32)                 # -0.0 + 0.0 = +0.0: no +-0 ties


def make_input(kind, B, T, D, seed=0):
    """fp32 [B, T, D], deterministic.  Kinds: formula (oracle.formula.ftensor), offset (formula + 30), normal (seeded),
    ties (seeded, quantised to quarters: many equal values), const (formula with channel 0 constant 0.5),
    mixed (seeded normal scaled by 2; from D = 4 on channel 0 is constant 0.5; channel 1 all negative, the last channel
    quantised)."""
    rng = np.random.default_rng(90210 + 7919 * seed + 31 * T + 977 * D + B)
    if kind == "formula":
        x = _ftensor((B, T, D), scale=1.5, freq=0.37, phase=0.3)
    elif kind == "offset":
        x = _ftensor((B, T, D), scale=1.5, freq=0.37, phase=0.3) + np.float32(30.0)
    elif kind == "normal":
        x = rng.standard_normal((B, T, D))
    elif kind == "ties":
        x = np.round(rng.standard_normal((B, T, D)) * 4.0) / 4.0
    elif kind == "const":
        x = _ftensor((B, T, D), scale=1.5, freq=0.37, phase=0.3).copy()
        x[:, :, 0] = 0.5
    elif kind == "mixed":
        x = 2.0 * rng.standard_normal((B, T, D))
        if D > 3:
            x[:, :, 0] = 0.5
        if D > 1:
            x[:, :, 1] = -np.abs(x[:, :, 1]) - 1.0
        if D > 2:
            x[:, :, -1] = np.round(x[:, :, -1] * 4.0) / 4.0
    else:
        raise KeyError(kind)
    return _no_negative_zero(np.asarray(x, dtype=np.float32))


# name -> (kind, B, T, D): the cases recorded from the reference in tests/golden/patch_moments.npz
GOLDEN_CASES = {
    "base": ("formula", 3, 196, 768),
    "small": ("formula", 2, 5, 7),
    "single": ("formula", 2, 1, 3),
    "offset": ("offset", 2, 196, 64),
    "long": ("normal", 2, 1024, 33),
    "ties": ("ties", 2, 196, 33),
    "const": ("const", 2, 196, 7),
}
CONST_ROW = (0.5, 0.5, 0.0, 0.5, 0.0, -3.0)     # the reference's six statistics of a constant channel of 0.5


def golden_keys():
    """(key in the npz, case name, unbiased)"""
    out = []
    for name, (_, _, T, _) in GOLDEN_CASES.items():
        for unbiased in (False, True):
            if unbiased and T < 2:
                continue
            out.append((f"{name}_u{int(unbiased)}", name, unbiased))
    return out


def golden_input(name):
    kind, B, T, D = GOLDEN_CASES[name]
    return make_input(kind, B, T, D)


# small cases on which every wrong variant must leave the bounds: even T (the two middle elements differ), a constant
# channel (sigma is clamped there), an all-negative channel (max |x| is not max x), sigma away from 1
VARIANT_CASES = (("mixed", 2, 6, 7), ("mixed", 3, 4, 5), ("mixed", 1, 12, 4), ("mixed", 2, 198, 4))

# the device shapes
DEVICE_T = (1, 2, 5, 196, 197, 1024) + tuple(t + i for t in SLAB_SWITCH_T for i in (0, 1))
DEVICE_D = (1, 7, 64, 65, 768)
DEVICE_B = (1, 3)


# ---------------------------------------------------------------------------------------------------- torch composition
def torch_composition(latent, eps=EPS, unbiased=False):
    """The six statistics composed from torch reductions, in the tensor's own dtype and on its own device: what a caller
    runs without the entry (and the plain fp32 evaluation the bounds must admit)."""
    import torch
    T = latent.shape[1]
    mean = latent.mean(dim=1)
    peak = latent.amax(dim=1)
    spread = latent.std(dim=1, unbiased=bool(unbiased))
    middle = latent.median(dim=1).values
    dev = latent - mean[:, None, :]
    third = dev.pow(3).sum(dim=1) / T
    fourth = dev.pow(4).sum(dim=1) / T
    sigma = torch.clamp(spread, min=eps)
    return torch.cat([mean, peak, spread, middle, third / sigma.pow(3), fourth / sigma.pow(4) - 3.0], dim=1)
