"""CPU-only checks of the native heterophily entry points (include/isic_hip.h): both symbols are exported and declared,
and their argument checks answer before any device work, so they run without a GPU."""
import ctypes
import os
import re

from isic_hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("isic_laplacian_lambda2_f64", "isic_segment_stats_f32")


def test_spectral_entry_points_are_exported_and_declared():
    L = lib.lib()
    text = open(os.path.join(ROOT, "include", "isic_hip.h")).read()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.public and hasattr(cdll, name), name
    assert int(re.search(r"#define ISIC_SPECTRAL_MAX_NODES (\d+)", text).group(1)) == 196
    assert int(re.search(r"#define ISIC_SEGMENT_MAX_LEN (\d+)", text).group(1)) == 16384
    assert len(L.public) == 96
    assert L.fn["isic_abi_version"]() == 1


def test_spectral_argument_checks_without_a_device():
    f = lib.lib().fn
    lam2 = f["isic_laplacian_lambda2_f64"]
    for nodes in (0, -3, 197, 1000):
        assert lam2(None, None, None, 4, nodes, None, None) == -2          # ISIC_ERR_UNSUPPORTED
    assert lam2(None, None, None, -1, 16, None, None) == -1                # ISIC_ERR_BAD_ARG
    assert lam2(None, None, None, 3, 16, None, None) == -1                 # no offsets / output
    assert lam2(None, None, None, 0, 196, None, None) == 0                 # nothing to do
    seg = f["isic_segment_stats_f32"]
    assert seg(None, None, 100, 3, 4, 16385, None, None, None, None) == -2
    assert seg(None, None, -1, 3, 4, 10, None, None, None, None) == -1
    assert seg(None, None, 100, -1, 4, 10, None, None, None, None) == -1
    assert seg(None, None, 100, 3, 4, -1, None, None, None, None) == -1
    assert seg(None, None, 100, 3, 4, 16384, None, None, None, None) == -1  # supported bound, NULL pointers
    assert seg(None, None, 100, 0, 4, 16384, None, None, None, None) == 0


def test_laplacian_lambda2_op_is_registered_with_a_fake():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from isic_hip import torch_ops  # noqa: F401
    op = torch.ops.isic_hip.laplacian_lambda2
    schema = op.default._schema
    assert not schema.is_mutable
    with FakeTensorMode():
        e = torch.empty(50, dtype=torch.int64)
        out = op(e, e, torch.empty(8, dtype=torch.int64), 196)
        assert out.shape == (7,) and out.dtype == torch.float64
