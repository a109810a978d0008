"""Shared helpers for the tests (fixture decoding, tolerances)."""
import os
from collections import OrderedDict

import numpy as np
import torch

from oracle import formula

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
NAN = float("nan")
PAD = 64                                            # NaN floats before and after every guarded output (a multiple of 4)


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def shapes_from_blob(blob):
    out = OrderedDict()
    for s in blob.tolist():
        k, dims = s.split("|")
        out[k] = tuple(int(v) for v in dims.split(",")) if dims else ()
    return out


def formula_params(g):
    return formula.formula_state_dict(shapes_from_blob(g["names"]))


def check_grad(g, key, t, rtol=2e-4, atol=1e-6):
    """Compare tensor ``t`` against golden gradient ``key`` (full or sampled)."""
    a = t.detach().cpu().double().numpy().reshape(-1)
    if f"grad.{key}" in g.files:
        ref = g[f"grad.{key}"].reshape(-1).astype(np.float64)
        scale = max(np.abs(ref).max(), 1e-30)
        np.testing.assert_allclose(a, ref, rtol=rtol, atol=atol + rtol * scale)
        return
    stride = int(g[f"grad.{key}#stride"])
    ref = g[f"grad.{key}#sample"].astype(np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    np.testing.assert_allclose(a[::stride][: ref.size], ref, rtol=rtol, atol=atol + rtol * scale)
    l2 = float(g[f"grad.{key}#l2"])
    assert abs(np.sqrt((a * a).sum()) - l2) <= rtol * max(l2, 1e-30) + atol
    assert a.size == int(g[f"grad.{key}#numel"])


def assert_close(a, b, rtol=1e-5, atol=1e-6, what=""):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    scale = max(np.abs(b).max(), 1e-30) if b.size else 1.0
    err = np.abs(a - b).max() if b.size else 0.0
    assert err <= atol + rtol * scale, f"{what}: max|diff|={err:.3e} > {atol + rtol * scale:.3e} (scale {scale:.3e})"


class Guarded:
    """an fp32 output of `shape`, NaN pre-filled, with PAD NaN floats before and after it; `offset` floats (0 or 1) move
    it off 16-byte alignment"""

    def __init__(self, shape, offset=0, init=None):
        n = int(np.prod(shape))
        self.buf = torch.full((2 * PAD + n + 4,), NAN, device=DEV, dtype=torch.float32)
        self.lo = PAD + offset
        self.n = n
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def ok(self, finite=True):
        intact = bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())
        return intact and (not finite or bool(torch.isfinite(self.t).all()))

    def cpu(self):
        return self.t.detach().cpu()


def stop_after_a_device_error():
    """the body of the GPU modules' autouse fixture: a device error (not a failed comparison) ends the session -- nothing more
    is launched on a GPU that has faulted"""
    import pytest
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further GPU work: {e}", returncode=3)
