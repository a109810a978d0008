"""The fixed-order slab reducers on the MI355X against tests/slab_reduce_ref.py, bit for bit: isic_test_slab_reduce_f32
runs the device functions of csrc/slab_sum.inc (for forms 0 .. 3 through the very kernels the split-K GEMMs, the column
sums and the weight gradients launch) over a contiguous [slabs][n] stack.  The reference was written from the reducers
as they stood before they shared those functions, and tests/test_slab_reduce_cpu.py shows that on these inputs any two
orders give different bits from 64 slabs on, so equality here pins the order and not just the sum.

MI355X result: not measured (no MI355X run of this module has happened yet; profiles/slab_reduce_check.txt)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import slab_reduce_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                          # NaN floats behind the output (a multiple of 4)
BAD_ARG = -1


def _call(*a):
    from isic_hip.lib import call
    return call(*a)


def _code(*a):
    from isic_hip.lib import IsicHipError
    try:
        _call(*a)
    except IsicHipError as e:
        return e.code
    return 0


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further GPU work: {e}", returncode=3)


@pytest.mark.parametrize("beta", (0.0, 1.0))
@pytest.mark.parametrize("form", R.FORMS)
def test_slab_reduce_matches_the_reference_bit_for_bit(form, beta):
    wrong = []
    for slabs in R.SLABS:
        for n in R.n_values(form):
            partial, prior = R.case(slabs, n)
            want = R.bits(R.epilogue(R.expected(form, slabs, n), prior, beta))
            dpart = torch.from_numpy(partial.copy()).to(DEV)
            buf = torch.full((n + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
            if beta != 0.0:
                buf[:n].copy_(torch.from_numpy(prior.copy()))    # beta == 0: the NaN under the output must not be read
            _call("isic_test_slab_reduce_f32", form, dpart, slabs, n, buf, beta)
            host = buf.cpu().numpy()
            assert np.isnan(host[n:]).all(), (form, slabs, n, "guard tail written")
            differing = int(np.count_nonzero(R.bits(host[:n]) != want))
            if differing:
                wrong.append((slabs, n, differing))
    assert not wrong, f"form {form} beta {beta}: (slabs, n, differing elements) {wrong}"


def test_slab_reduce_refuses_what_it_does_not_do():
    partial = torch.zeros(8 * 8 + 4, device=DEV)
    out = torch.zeros(16, device=DEV)
    for form in R.FORMS:
        assert _code("isic_test_slab_reduce_f32", form, partial, 8, 8, out, 0.5) == BAD_ARG
        assert _code("isic_test_slab_reduce_f32", form, partial, 0, 8, out, 0.0) == BAD_ARG
        assert _code("isic_test_slab_reduce_f32", form, partial, 8, 8, out, 1.0) == 0
    for form in (-1, 5):
        assert _code("isic_test_slab_reduce_f32", form, partial, 8, 8, out, 0.0) == BAD_ARG
    for form in R.VECTOR_FORMS:
        assert _code("isic_test_slab_reduce_f32", form, partial, 8, 6, out, 0.0) == BAD_ARG          # n % 4
        assert _code("isic_test_slab_reduce_f32", form, partial[1:], 8, 8, out, 0.0) == BAD_ARG      # 4-byte aligned only
        assert _code("isic_test_slab_reduce_f32", form, partial, 8, 8, out[1:], 0.0) == BAD_ARG
    for form in (0, 1, 4):
        assert _code("isic_test_slab_reduce_f32", form, partial[1:], 8, 6, out[1:], 0.0) == 0
    torch.cuda.synchronize()
