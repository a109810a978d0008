"""The token statistics' restatement and bounds (tests/moments_ref.py) checked without a device: the reference's recorded
outputs and a plain fp32 torch evaluation lie inside the bounds, every wrong variant lies outside, the C entry is declared
where it belongs and checks its arguments before any device work, and the Python layers raise as documented."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moments_ref as R  # noqa: E402
from isic_hip import lib  # noqa: E402

BAD_ARG, UNSUPPORTED = -1, -2
P = 0x1000                       # a dummy, 16-byte aligned, non-NULL pointer: never dereferenced (errors come first)
ENTRY = "isic_token_moments_f32"


@pytest.fixture(scope="module")
def golden():
    with np.load(R.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_entry_is_declared_in_the_new_header_only_and_exported():
    L = lib.lib()
    inc = os.path.dirname(lib.header_path())
    assert '#include "isic_hip_moments.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    assert os.path.join(inc, "isic_hip_moments.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    assert ENTRY in lib.parse_header(os.path.join(inc, "isic_hip_moments.h"))
    assert ENTRY not in L.public and len(L.public) == 96
    assert ENTRY in L.extension and ENTRY in L.fn
    assert f"#define ISIC_MOMENTS_MAX_T {R.MAX_T}\n" in open(os.path.join(inc, "isic_hip_moments.h")).read()
    from isic_hip import build
    assert "isic_hip_moments.h" in map(os.path.basename, build.header_deps())


def test_argument_checks_without_a_device():
    f = lib.lib().fn[ENTRY]
    nan = float("nan")
    #        X  B  T    D   ldx eps  unb out ldo stream
    assert f(None, 2, 5, 7, 7, 1e-6, 0, P, 42, None) == BAD_ARG               # no X with B > 0
    assert f(P, 2, 5, 7, 7, 1e-6, 0, None, 42, None) == BAD_ARG               # no out with B > 0
    assert f(P, -1, 5, 7, 7, 1e-6, 0, P, 42, None) == BAD_ARG                 # B < 0
    assert f(P, 2, 0, 7, 7, 1e-6, 0, P, 42, None) == BAD_ARG                  # T < 1
    assert f(P, 2, 5, 0, 7, 1e-6, 0, P, 42, None) == BAD_ARG                  # D < 1
    assert f(P, 2, 5, 7, 6, 1e-6, 0, P, 42, None) == BAD_ARG                  # ldx < D
    assert f(P, 2, 5, 7, 7, 1e-6, 0, P, 41, None) == BAD_ARG                  # ldo < 6 D
    assert f(P, 2, 5, 7, 7, -1e-6, 0, P, 42, None) == BAD_ARG                 # eps negative
    assert f(P, 2, 5, 7, 7, nan, 0, P, 42, None) == BAD_ARG                   # eps NaN
    assert f(P, 2, 5, 7, 7, 1e-6, 2, P, 42, None) == BAD_ARG                  # unbiased not 0 or 1
    assert f(P, 2, 5, 7, 7, 1e-6, -1, P, 42, None) == BAD_ARG
    assert f(P, 2, 1, 7, 7, 1e-6, 1, P, 42, None) == BAD_ARG                  # unbiased with T < 2
    assert f(P, 2, R.MAX_T + 1, 7, 7, 1e-6, 0, P, 42, None) == UNSUPPORTED    # T > 1024
    assert f(P, 1 << 31, 1, 7, 7, 1e-6, 0, P, 42, None) == UNSUPPORTED        # a grid that would not fit
    assert f(P, 1 << 28, 1, 768, 768, 1e-6, 0, P, 4608, None) == UNSUPPORTED  # 2^28 images x 12 slabs
    assert f(None, 0, 5, 7, 7, 1e-6, 0, None, 42, None) == 0                  # B == 0: nothing to do
    assert f(P, 0, 5, 7, 7, 0.0, 1, P, 42, None) == 0


def test_lower_median_of_an_even_count():
    x = np.array([1.0, 2.0, 3.0, 4.0], dtype=np.float32).reshape(1, 4, 1)
    assert R.reference(x)[0, 3] == 2.0 == float(torch.from_numpy(x).median(dim=1).values)


@pytest.mark.parametrize("key,name,unbiased", R.golden_keys())
def test_recorded_reference_outputs_and_a_plain_fp32_evaluation_lie_inside_the_bounds(golden, key, name, unbiased):
    x = R.golden_input(name)
    ref, bound = R.reference(x, R.EPS, unbiased), R.bounds(x, R.EPS, unbiased)
    assert np.isfinite(bound).all()
    rec = golden[key]
    assert rec.shape == ref.shape and rec.dtype == np.float32
    plain = R.torch_composition(torch.from_numpy(x), R.EPS, unbiased).numpy()
    for what, got in (("recorded reference", rec), ("fp32 torch composition", plain)):
        print(f"{key} {what}: worst error / bound {R.worst_per_stat(got, ref, bound)}")
        assert R.selections_equal(got, ref), (key, what)
        assert R.worst(got, ref, bound) <= 1.0, (key, what)


def test_constant_channel_of_the_recorded_reference(golden):
    for key in ("const_u0", "const_u1"):
        D = golden[key].shape[1] // 6
        assert tuple(golden[key][:, 0::D][0]) == R.CONST_ROW and tuple(golden[key][:, 0::D][1]) == R.CONST_ROW
        assert tuple(R.reference(R.golden_input("const"), R.EPS, key.endswith("1"))[0, 0::D]) == R.CONST_ROW


@pytest.mark.parametrize("bug", R.BUGS)
def test_bounds_reject_the_wrong_variants(bug):
    for kind, B, T, D in R.VARIANT_CASES:
        x = R.make_input(kind, B, T, D)
        for unbiased in (False, True):
            ref, bound = R.reference(x, R.EPS, unbiased), R.bounds(x, R.EPS, unbiased)
            assert R.worst(R.reference(x, R.EPS, unbiased), ref, bound) == 0.0
            assert R.worst(R.reference(x, R.EPS, unbiased, bug=bug), ref, bound) > 1.0, (bug, kind, B, T, D, unbiased)


def test_python_layers_exist_and_raise_as_documented():
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(lib.__file__)))
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import utils
    from isic_hip.moments import token_moments
    for fn in (token_moments, utils.concat_patch_moments):
        with pytest.raises(ValueError):
            fn(torch.zeros(4, 8))                                             # not 3-D
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 4, 8, dtype=torch.float16))                     # not fp32
        with pytest.raises(ValueError):
            fn(torch.zeros(1, R.MAX_T + 1, 2))                                # T > 1024
        with pytest.raises(ValueError):
            fn(torch.zeros(2, 1, 8), unbiased=True)                           # unbiased with one token
        with pytest.raises(RuntimeError):
            fn(torch.zeros(2, 4, 8))                                          # a CPU tensor: no fallback
        with pytest.raises(RuntimeError):
            fn(torch.zeros(2, 4, 8, requires_grad=True))                      # no backward
        with torch.no_grad(), pytest.raises(lib.IsicHipError):
            fn(torch.zeros(2, 4, 8, requires_grad=True))                      # under no_grad it is the CPU tensor that stops it


def test_config_keys_default_to_off():
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(lib.__file__)))
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import train_ae
    assert train_ae.plan({})["latent_moments"] is False
    assert train_ae.plan({"training_plan": {"parameters": {"latent_moments": True}}})["latent_moments"] is True
    assert "concat_patch_moments" not in train_ae.__doc__.split("Not ported")[1]
