"""``DevicePCA``: the latent PCA of the reference's ``save_latent.py:163-185`` (``sklearn.decomposition.PCA(0.90)``) fitted
and applied on resident latents.

The fit is what sklearn's ``covariance_eigh`` solver computes for a tall input -- the centred Gram matrix and a D x D
symmetric eigenproblem -- with the Gram matrix formed on the device by ``isic_gram_shifted_f32`` (include/isic_hip_pca.h):
one pass over the latents, the shift subtracted while the row tile is staged, one triangle of tiles, fp32 inside runs of
2048 rows and fp64 across them, no atomics.  ``partial_fit`` accumulates it over encoder batches (optionally through a row
index, so the Gram pass skips background patches without a gathered copy; only the first call gathers its rows once, to
form the shift); ``finalize`` solves the eigenproblem.  By decision the D x D
eigenproblem (D <= 1024: at most 8 MB, once per fit) is solved on the host with ``numpy.linalg.eigh`` in fp64: the hot path
is the Gram matrix, a native eigensolver is out of scope.  ``transform`` is the existing exact-fp32 GEMM with
``-mean components^T`` as its bias.
"""
from __future__ import annotations

import numpy as np
import torch

from .lib import ERR_UNSUPPORTED, IsicHipError, call
from .ops import ACT_NONE, _workspace, colsum, gemm


def _check_x(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise IsicHipError(f"DevicePCA.{what}: x must be a device tensor (got a CPU tensor; there is no CPU fallback)")
    if x.dim() != 2 or x.dtype != torch.float32 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise IsicHipError(f"DevicePCA.{what}: x must be a 2-D fp32 tensor with unit inner stride")


def _check_rows(rows, what):
    if rows is None:
        return None
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda:
        raise IsicHipError(f"DevicePCA.{what}: rows must be a device tensor (got a CPU tensor)")
    if rows.dim() != 1 or rows.dtype != torch.int32:
        raise IsicHipError(f"DevicePCA.{what}: rows must be a 1-D int32 tensor")
    return rows.contiguous()


def _padded8(rows):
    """the index padded to a multiple of 8 entries (isic_gemm_f32_rows_ws reads it in groups of 8)"""
    n = rows.numel()
    pad = -n % 8
    if pad == 0 or n == 0:
        return rows
    return torch.cat([rows, rows[:1].expand(pad)])


class DevicePCA:
    """PCA with sklearn's attribute names, fitted on the device.

    ``n_components``: a float in (0, 1) keeps the smallest number of components whose cumulative explained-variance ratio
    exceeds it (sklearn's rule: ``searchsorted(cumsum(ratio), n_components, side="right") + 1``); an int keeps that many.

    After ``finalize()`` (or ``fit``): ``mean_ [D]``, ``components_ [k, D]``, ``explained_variance_ [k]``,
    ``explained_variance_ratio_ [k]`` (fp32 device tensors), ``n_components_``, ``n_samples_seen_``.  The fp64 host arrays
    the fp32 attributes were rounded from are kept as ``mean64_``, ``components64_``, ``explained_variance64_`` and
    ``eigenvalues64_`` (all D of them, descending).

    Differences from sklearn: fewer than two samples raise ``ValueError`` (sklearn returns NaN variances with a warning);
    no whitening; one solver.
    """

    def __init__(self, n_components=0.90):
        if isinstance(n_components, float):
            if not 0.0 < n_components < 1.0:
                raise ValueError("a float n_components must lie in (0, 1)")
        elif not (isinstance(n_components, int) and n_components >= 1):
            raise ValueError("n_components: a float in (0, 1) or a positive int")
        self.n_components = n_components
        self._reset()

    def _reset(self):
        self._G = self._colsum = self._shift = None
        self._ws = None
        self.n_samples_seen_ = 0
        self.n_components_ = None
        self.mean_ = self.components_ = self.explained_variance_ = self.explained_variance_ratio_ = None
        self._bias = None

    # ------------------------------------------------------------------ fit
    def partial_fit(self, x, rows=None):
        """Add the rows of ``x [M, D]`` (those listed in ``rows`` when given) to the fit.  The first call fixes the shift
        as the fp32 column mean of its own rows; later calls accumulate around the same shift."""
        _check_x(x, "partial_fit")
        rows = _check_rows(rows, "partial_fit")
        D = x.shape[1]
        M = int(rows.numel()) if rows is not None else int(x.shape[0])
        if self._G is None:
            self._G = torch.zeros((D, D), device=x.device, dtype=torch.float64)
            self._colsum = torch.zeros((D,), device=x.device, dtype=torch.float64)
        elif self._G.shape[0] != D:
            raise ValueError(f"partial_fit: width {D} after width {self._G.shape[0]}")
        if M == 0:
            return self
        if self._shift is None:
            first = x if rows is None else x.index_select(0, rows.long())
            self._shift = (colsum(first) / float(M)).contiguous()
        nbytes = int(call("isic_gram_shifted_f32_workspace_bytes", M, D))       # bounded, and monotone in M
        if self._ws is None or self._ws.numel() < nbytes:                       # kept across batches, grown only
            self._ws = torch.empty(max(nbytes, 16), device=x.device, dtype=torch.uint8)
        call("isic_gram_shifted_f32", x.data_ptr(), M, D, max(x.stride(0), D), rows, self._shift, self._G, self._colsum,
             1.0 if self.n_samples_seen_ > 0 else 0.0, self._ws, self._ws.numel())
        self.n_samples_seen_ += M
        return self

    def finalize(self):
        """Solve the D x D eigenproblem (fp64, host) and set the fitted attributes."""
        M = self.n_samples_seen_
        if M < 2:
            raise ValueError(f"DevicePCA needs at least two samples to estimate a covariance (got {M})")
        dev = self._G.device
        G = self._G.cpu().numpy()
        d = self._colsum.cpu().numpy() / M
        mean = self._shift.double().cpu().numpy() + d
        C = (G - M * np.outer(d, d)) / (M - 1)
        lam, vec = np.linalg.eigh(C)
        lam, vec = np.maximum(lam[::-1], 0.0), vec[:, ::-1]
        comps = np.ascontiguousarray(vec.T)                              # [D, D], rows = components, descending
        # sklearn's svd_flip(u_based_decision=False): the entry of largest magnitude of every component is positive
        big = np.argmax(np.abs(comps), axis=1)
        sign = np.sign(comps[np.arange(comps.shape[0]), big])
        comps *= np.where(sign == 0, 1.0, sign)[:, None]
        total = lam.sum()
        ratio = lam / total if total > 0 else np.zeros_like(lam)
        if isinstance(self.n_components, float):
            k = int(np.searchsorted(np.cumsum(ratio), self.n_components, side="right")) + 1
        else:
            k = self.n_components
        k = max(1, min(k, comps.shape[0]))
        self.n_components_ = k
        self.eigenvalues64_ = lam
        self.mean64_, self.components64_ = mean, comps[:k].copy()
        self.explained_variance64_, self.explained_variance_ratio64_ = lam[:k].copy(), ratio[:k].copy()
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        self.mean_, self.components_ = f32(mean), f32(self.components64_)
        self.explained_variance_, self.explained_variance_ratio_ = f32(lam[:k]), f32(ratio[:k])
        # transform = x components^T - mean components^T (sklearn >= 1.5); the constant in fp64 from the ROUNDED operands the
        # product runs on, rounded once
        self._bias = f32(-(self.components_.double().cpu().numpy() @ self.mean_.double().cpu().numpy()))
        return self

    def fit(self, x, rows=None):
        self._reset()
        return self.partial_fit(x, rows).finalize()

    # ------------------------------------------------------------------ apply
    def transform(self, x, rows=None):
        """``x[rows] components_^T - mean_ components_^T`` -> fp32 ``[M, n_components_]`` on the fp32 MFMA GEMM.  With
        ``rows`` the GEMM reads its row operand through the index where ``isic_gemm_f32_rows_ws`` serves it (a product of at
        least 1e8 multiply-adds with more than 128 rows and every dimension, ``n_components_`` included, a multiple of 4);
        otherwise the rows are gathered first."""
        if self.components_ is None:
            raise IsicHipError("DevicePCA.transform before fit / finalize")
        _check_x(x, "transform")
        rows = _check_rows(rows, "transform")
        W, b = self.components_, self._bias
        K, N = x.shape[1], W.shape[0]
        if K != W.shape[1]:
            raise ValueError(f"transform: width {K}, fitted on width {W.shape[1]}")
        if rows is None:
            return gemm(x, W, trans_b=True, bias=b)
        M = int(rows.numel())
        y = torch.empty((M, N), device=x.device, dtype=torch.float32)
        if M == 0:
            return y
        ws = _workspace(call("isic_gemm_f32_workspace_bytes", 0, 1, M, N, K), x.device)
        try:
            call("isic_gemm_f32_rows_ws", 0, 1, M, N, K, x.data_ptr(), max(x.stride(0), K), _padded8(rows), W, K, None, y, N, b,
                 ACT_NONE, 0.0, ws, ws.numel() if ws is not None else 0)
        except IsicHipError as e:
            if e.code != ERR_UNSUPPORTED:
                raise
            gemm(x.index_select(0, rows.long()), W, trans_b=True, bias=b, out=y)      # the entry's contract: gather, then GEMM
        return y

    def fit_transform(self, x, rows=None):
        return self.fit(x, rows).transform(x, rows)
