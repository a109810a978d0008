"""The shifted-Gram kernel (csrc/pca_gram.hip) through the C ABI, ``DevicePCA`` and the ``device_pca`` path of
``extract_latents`` on the MI355X, held to the fp64 restatement and the derived bounds of tests/pca_ref.py.

Outputs of the C entry are prefilled with NaN between guard areas.  The module prints the device's worst error / bound per
family and, next to it, the distance of sklearn on the same fp32 input; only the device's is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pca_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENTINEL = -7.25


def gram(x, M, D, ldx=None, rows=None, shift=None, beta=0.0, out=None, x_ptr=None):
    """isic_gram_shifted_f32 on device tensors -> (G [D, D], colsum [D]) float64 numpy + the raw buffer (for a second,
    accumulating call).  The outputs sit in one buffer: guard | G | guard | colsum | guard."""
    from isic_hip.lib import call
    n = GUARD + D * D + GUARD + D + GUARD
    if out is None:
        out = torch.full((n,), float("nan"), device=DEV, dtype=torch.float64)
        for a in (0, GUARD + D * D, GUARD + D * D + GUARD + D):
            out[a:a + GUARD] = SENTINEL
    G, cs = out[GUARD:GUARD + D * D], out[2 * GUARD + D * D:2 * GUARD + D * D + D]
    nbytes = int(call("isic_gram_shifted_f32_workspace_bytes", M, D))
    ws = torch.empty(max(nbytes, 16), device=DEV, dtype=torch.uint8)
    call("isic_gram_shifted_f32", x_ptr if x_ptr is not None else x, M, D, ldx or D, rows, shift, G.data_ptr(), cs.data_ptr(),
         float(beta), ws if nbytes else None, nbytes)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    for a in (0, GUARD + D * D, GUARD + D * D + GUARD + D):
        assert (h[a:a + GUARD] == SENTINEL).all(), "guard area overwritten"
    return h[GUARD:GUARD + D * D].reshape(D, D).copy(), h[2 * GUARD + D * D:2 * GUARD + D * D + D].copy(), out


def dev_rows(rows):
    """int32 index on the device, allocated as a multiple of 8 entries"""
    pad = -len(rows) % 8
    return torch.from_numpy(np.concatenate([rows, np.zeros(pad, dtype=np.int32)])).to(DEV)


def check_gram(x, G, cs, rows=None, shift=None, tag=""):
    Gr, csr = R.gram_eval(x, rows, shift)
    EG, Ec = R.gram_bound(x, rows, shift)
    rg, rc = R.ratio(G, Gr, EG), R.ratio(cs, csr, Ec)
    print(f"gram {tag}: error / bound G {rg:.3e} colsum {rc:.3e}")
    assert rg <= 1.0 and rc <= 1.0
    assert np.array_equal(G.view(np.uint64), G.T.copy().view(np.uint64)), "G is not bit-symmetric"


@pytest.mark.parametrize("M,D", [(M, D) for D in R.GRAM_D for M in R.GRAM_M] + [(M, 64) for M in R.GRAM_RUN_M])
def test_gram_cases(M, D):
    x = R.family(M, D)
    shift = x[: max(1, M // 2)].astype(np.float64).mean(axis=0).astype(np.float32)
    xd, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(shift).to(DEV)
    G, cs, _ = gram(xd, M, D, shift=sd)
    check_gram(x, G, cs, None, shift, f"M {M} D {D}")
    G2, cs2, _ = gram(xd, M, D, shift=sd)
    assert np.array_equal(G.view(np.uint64), G2.view(np.uint64)) and np.array_equal(cs.view(np.uint64), cs2.view(np.uint64))


def test_gram_column_slice_rows_and_null_shift():
    M, D, W = 777, 64, 96
    big = R.family(M, W)
    bd = torch.from_numpy(big).to(DEV)
    x = np.ascontiguousarray(big[:, 16:16 + D])
    shift = x.astype(np.float64).mean(axis=0).astype(np.float32)
    sd = torch.from_numpy(shift).to(DEV)
    G, cs, _ = gram(bd, M, D, ldx=W, shift=sd, x_ptr=bd.data_ptr() + 16 * 4)            # ldx > D: a column slice
    check_gram(x, G, cs, None, shift, "column slice")
    rows = R.rows_for(M)                                                                 # gaps and a repeated row
    assert len(np.unique(rows)) == len(rows) - 1 and rows.max() - rows.min() + 1 > len(rows)
    G, cs, _ = gram(bd, len(rows), D, ldx=W, rows=dev_rows(rows), shift=sd, x_ptr=bd.data_ptr() + 16 * 4)
    check_gram(x, G, cs, rows, shift, "rows on a column slice")
    G, cs, _ = gram(bd, M, D, ldx=W, x_ptr=bd.data_ptr() + 16 * 4)                      # shift NULL: zeros
    check_gram(x, G, cs, None, None, "no shift")
    Gs, _ = R.gram_eval(x, None, shift)
    assert R.ratio(G, Gs, R.gram_bound(x, None, shift)[0]) > 1.0                         # ... and the shift does matter here


def test_gram_accumulates_over_two_calls_and_accepts_no_rows():
    M, D, cut = 3 * R.RUN + 77, 64, R.RUN + 301
    x = R.family(M, D)
    shift = x[:cut].astype(np.float64).mean(axis=0).astype(np.float32)
    xd, sd = torch.from_numpy(x).to(DEV), torch.from_numpy(shift).to(DEV)
    _, _, out = gram(xd[:cut], cut, D, shift=sd)
    G, cs, out = gram(xd[cut:], M - cut, D, shift=sd, beta=1.0, out=out)
    # two calls cut the rows into other runs than one call: each is within its own bound of the exact sum
    Gr, csr = R.gram_eval(x, None, shift)
    Ea, Eb = R.gram_bound(x[:cut], None, shift), R.gram_bound(x[cut:], None, shift)
    assert R.ratio(G, Gr, Ea[0] + Eb[0]) <= 1.0 and R.ratio(cs, csr, Ea[1] + Eb[1]) <= 1.0
    G1, cs1, _ = gram(xd, M, D, shift=sd)
    E1 = R.gram_bound(x, None, shift)
    assert R.ratio(G, G1, Ea[0] + Eb[0] + E1[0]) <= 1.0 and R.ratio(cs, cs1, Ea[1] + Eb[1] + E1[1]) <= 1.0
    assert np.array_equal(G.view(np.uint64), G.T.copy().view(np.uint64))
    # M == 0: beta == 1 leaves the outputs alone, beta == 0 writes zeros
    G0, cs0, out = gram(xd, 0, D, shift=sd, beta=1.0, out=out)
    assert np.array_equal(G0.view(np.uint64), G.view(np.uint64)) and np.array_equal(cs0.view(np.uint64), cs.view(np.uint64))
    G0, cs0, _ = gram(None, 0, D, beta=0.0)
    assert (G0 == 0).all() and (cs0 == 0).all()


# ---------------------------------------------------------------------------------------------------- DevicePCA
def device_fit(pca):
    return {"k": pca.n_components_, "explained_variance": pca.explained_variance_.cpu().numpy(),
            "components": pca.components_.cpu().numpy(), "mean": pca.mean_.cpu().numpy()}


@pytest.mark.parametrize("with_rows", (False, True))
@pytest.mark.parametrize("M,D", R.DEVICE_FIT_SHAPES)
def test_device_pca_against_the_restatement(M, D, with_rows):
    from isic_hip.pca import DevicePCA
    x, rows, ref = R.fit_case(M, D, with_rows)
    xd = torch.from_numpy(x).to(DEV)
    rd = torch.from_numpy(rows).to(DEV) if with_rows else None
    pca = DevicePCA(0.90)
    t = pca.fit_transform(xd, rd)
    torch.cuda.synchronize()
    shift_err = np.abs(pca._shift.double().cpu().numpy() - ref["shift"].astype(np.float64))
    bounds = R.fit_bounds(x, rows, ref, shift_err)
    assert bounds["checked"].sum() >= (1.0 - R.DK_SHARE) * ref["k"]
    got = device_fit(pca)
    r = R.fit_ratios(got, ref, bounds)
    from sklearn.decomposition import PCA
    sk = PCA(n_components=0.90).fit(x if rows is None else x[rows])
    rs = R.fit_ratios({"k": sk.n_components_, "explained_variance": sk.explained_variance_, "components": sk.components_,
                       "mean": sk.mean_}, ref, bounds)
    print(f"DevicePCA ({M}, {D}, rows={with_rows}): k {got['k']}, error / bound device {r} | sklearn on fp32 {rs}")
    assert pca.n_components_ == ref["k"] and pca.n_samples_seen_ == ref["M"]
    assert R.worst(r) <= 1.0
    assert np.abs(pca.explained_variance_ratio_.cpu().numpy() - ref["explained_variance_ratio"]).max() <= \
        2.0 * bounds["norm"] / ref["eigenvalues"].sum() * (1.0 + x.shape[1]) + R.U
    # the transform against the device's own components and mean
    c, m = got["components"], got["mean"]
    rt = R.ratio(t.cpu().numpy(), R.transform_eval(x, c, m, rows), R.transform_bound(x, c, m, rows))
    print(f"  transform error / bound {rt:.3e}")
    assert t.shape == (ref["M"], ref["k"]) and rt <= 1.0
    if not with_rows:                                         # an int n_components keeps that many
        p3 = DevicePCA(3).fit(xd)
        assert p3.n_components_ == 3 and p3.components_.shape == (3, D)
        assert torch.equal(p3.components_, pca.components_[:3])


def test_transform_reads_rows_through_the_index_where_the_gemm_serves_it(monkeypatch):
    """About 26 000 of 40 000 rows x 256 with 32 components: 2e8 multiply-adds, every dimension a multiple of 4 and at least
    96 row tiles of 256 -- the shape isic_gemm_f32_rows_ws serves with the row index on A (no gather); the result is held
    to the same bound as the gathered product"""
    from isic_hip import pca as P
    M, D, k = 40000, 256, 32
    x = R.family(M, D)
    r = R.rows_for(M)
    n = len(r) // 4 * 4
    rows = np.concatenate([r[:n - 1], r[:1]])                 # a multiple of 4 rows, gaps and the repeated row kept
    assert n >= 96 * 256
    xd, rd = torch.from_numpy(x).to(DEV), torch.from_numpy(rows).to(DEV)
    pca = P.DevicePCA(k).fit(xd, rd)
    served = []
    real_call = P.call

    def spy(name, *a, **kw):
        rc = real_call(name, *a, **kw)
        served.append(name)                                   # reached only when the entry did not raise
        return rc

    monkeypatch.setattr(P, "call", spy)
    t = pca.transform(xd, rd)
    torch.cuda.synchronize()
    assert "isic_gemm_f32_rows_ws" in served, "the row-indexed GEMM answered UNSUPPORTED for a shape it documents"
    c, m = pca.components_.cpu().numpy(), pca.mean_.cpu().numpy()
    rt = R.ratio(t.cpu().numpy(), R.transform_eval(x, c, m, rows), R.transform_bound(x, c, m, rows))
    print(f"transform through the row index ({len(rows)} x {k} x {D}): error / bound {rt:.3e}")
    assert t.shape == (len(rows), k) and rt <= 1.0
    tg = pca.transform(xd.index_select(0, rd.long()))        # the gathered product, for the record
    print(f"  max |indexed - gathered| {float((t - tg).abs().max()):.3e}")


def test_device_pca_partial_fit_over_batches():
    from isic_hip.pca import DevicePCA
    x, rows, ref = R.fit_case(5000, 64, False)
    xd = torch.from_numpy(x).to(DEV)
    pca = DevicePCA(0.90)
    for a, b in ((0, 1800), (1800, 1800), (1800, 4100), (4100, 5000)):                  # an empty batch among them
        pca.partial_fit(xd[a:b])
    pca.finalize()
    shift = pca._shift.cpu().numpy()
    shift_err = np.abs(shift.astype(np.float64) - x[:1800].astype(np.float64).mean(axis=0))
    ref_b = dict(ref, shift=shift, colsum=R.gram_eval(x, None, shift)[1])
    r = R.fit_ratios(device_fit(pca), ref, R.fit_bounds(x, None, ref_b, shift_err))
    print(f"DevicePCA over 3 batches: error / bound {r}")
    assert pca.n_samples_seen_ == 5000 and R.worst(r) <= 1.0


def test_device_pca_error_cases():
    from isic_hip.lib import IsicHipError
    from isic_hip.pca import DevicePCA
    xd = torch.from_numpy(R.family(16, 8)).to(DEV)
    with pytest.raises(ValueError):
        DevicePCA().fit(xd[:1])                                                          # M < 2 (sklearn: NaN)
    with pytest.raises(ValueError):
        DevicePCA().fit(xd, torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(IsicHipError):
        DevicePCA().fit(xd.cpu())
    with pytest.raises(IsicHipError):
        DevicePCA().fit(xd, torch.zeros(4, dtype=torch.int32))
    p = DevicePCA().fit(xd)
    with pytest.raises(IsicHipError):
        p.transform(xd.cpu())


# ---------------------------------------------------------------------------------------------------- extract_latents
@pytest.fixture(scope="module")
def latent_runs():
    import save_latent as sl
    tv, te = sl.SyntheticDermImages(n=7, seed=1), sl.SyntheticDermImages(n=3, seed=2)
    runs = {}
    for remove in (True, False):
        base = sl.extract_latents({"device": DEV, "seed": 42, "pca": False}, "missing.pth", remove, datasets=(tv, te),
                                  batch_size=3)
        dev = sl.extract_latents({"device": DEV, "seed": 42, "pca": True, "device_pca": True}, "missing.pth", remove,
                                 datasets=(tv, te), batch_size=3)
        runs[remove] = (base, dev, tv)
    return runs


@pytest.mark.parametrize("remove", (True, False))
def test_extract_latents_with_device_pca(latent_runs, remove):
    base, dev, tv = latent_runs[remove]
    for f in range(2):                                        # train and test patch frames: same rows, same order, same latents
        a, b = base[f], dev[f]
        assert len(a) == len(b) > 0 and list(a.columns) == list(b.columns)
        for c in ("image_path", "segmentation_path", "target", "patch_id", "patch_in_mask"):
            assert list(a[c]) == list(b[c]), c
        assert all(np.array_equal(u, v) for u, v in zip(a["patch_latent"], b["patch_latent"]))
    for f in range(2, 6):
        assert len(base[f]) == len(dev[f]) and list(base[f].columns) == list(dev[f].columns)
    X = np.stack(list(dev[0]["patch_latent"])).astype(np.float32)
    T = np.stack(list(dev[0]["patch_latent_pca"])).astype(np.float64)
    Tt = np.stack(list(dev[1]["patch_latent_pca"]))
    M, D = X.shape
    k = T.shape[1]
    assert T.shape == (M, k) and Tt.shape == (len(dev[1]), k) and Tt.dtype == np.float32 and 0 < k < D

    # ---- gap-independent checks, in fp64 from the patch_latent columns (a seeded encoder gives no control over gaps): the
    # output columns are uncorrelated with variances lambda_i; the residual of the best linear reconstruction of the centred
    # latents from the output, row by row, is the sum of the dropped eigenvalues; the test frame's rows are the same map of
    # their latents (the map recovered from the train frame).  The last two are tied to the order of the rows.
    # The shift the device used is the fp32 column mean of the first batch's kept rows.
    first = set(tv[i]["image_path"] for i in range(3))
    sel = np.array([p in first for p in dev[0]["image_path"]])
    assert sel.any() and not sel.all()                        # the fit did accumulate over several batches
    Xt = np.stack(list(dev[1]["patch_latent"])).astype(np.float32)
    k_ok, ra, rb, rc = R.output_checks(X, T, sel, Xt, Tt)
    print(f"extract_latents device_pca (remove={remove}): M {M} D {D} k {k}; error / bound covariance {ra:.3e} "
          f"residual {rb:.3e} test rows {rc:.3e}")
    assert k_ok and ra <= 1.0 and rb <= 1.0 and rc <= 1.0
