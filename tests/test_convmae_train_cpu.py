"""CPU-only checks of the ConvMAE-Base training path: the entry points of include/isic_hip_convmae_train.h are declared,
exported and take `stream` last (isic_hip.h itself keeps its 97), their argument checks answer before any device work,
and the encoder / model options validate their combinations."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)

from isic_hip import lib  # noqa: E402

NAMES = ("isic_dwconv5x5_wgrad_f16_workspace_bytes", "isic_dwconv5x5_wgrad_f16", "isic_layernorm_add_bwd_f16_workspace_bytes",
         "isic_layernorm_add_bwd_f16", "isic_patch_rows_bwd_f16")
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call


def test_convmae_train_entry_points_are_declared_and_exported():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_convmae_train.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = open(os.path.join(inc, "isic_hip_convmae_train.h")).read()
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    L = lib.lib()
    assert len(L.public) == 96
    assert os.path.join(inc, "isic_hip_convmae_train.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name in L.fn and hasattr(cdll, name), name
        if not name.endswith("_workspace_bytes"):
            assert L.extension[name][1][-1][1] == "stream", name


def test_dwconv_wgrad_argument_checks_without_a_device():
    L = lib.lib().fn
    f, wsb = L["isic_dwconv5x5_wgrad_f16"], L["isic_dwconv5x5_wgrad_f16_workspace_bytes"]

    def call(N=4, H=56, W=56, C=256, acc=0, ws=P, nbytes=1 << 30, dw=P, x=P):
        return f(x, P, dw, P, N, H, W, C, 1.0, acc, ws, nbytes, None)
    for c in (32, 96, 200):
        assert call(C=c) == UNSUPPORTED, c
        assert wsb(4, 56, 56, c) == 0
    assert call(N=-1) == BAD_ARG and call(H=0) == BAD_ARG
    assert call(acc=2) == BAD_ARG
    assert call(dw=None) == BAD_ARG and call(x=None) == BAD_ARG
    need = wsb(4, 56, 56, 256)
    assert need > 0 and wsb(4, 57, 55, 384) > 0
    assert call(nbytes=need - 1) == WORKSPACE and call(ws=None) == WORKSPACE


def test_layernorm_add_bwd_argument_checks_without_a_device():
    L = lib.lib().fn
    f, wsb = L["isic_layernorm_add_bwd_f16"], L["isic_layernorm_add_bwd_f16_workspace_bytes"]

    def call(M=1000, N=768, dyf=0, act=0, acc=0, g_out=P, g16=P, ws=P, nbytes=1 << 30):
        return f(P, dyf, 1.0, P, None, None, P, P, act, 1e-6, None, g_out, g16, P, P, M, N, 1.0, acc, ws, nbytes, None)
    for n in (1088, 2048, 96, 100):                                   # N > 1024 or N % 64
        assert call(N=n) == UNSUPPORTED, n
    # accepted shapes, shown through calls that still stop before any device work
    assert call(N=1024, nbytes=0) == WORKSPACE and call(N=64, nbytes=0) == WORKSPACE
    assert call(dyf=2) == BAD_ARG and call(act=2) == BAD_ARG and call(acc=-1) == BAD_ARG and call(M=-1) == BAD_ARG
    assert call(g_out=None, g16=None) == BAD_ARG
    assert call(ws=None) == WORKSPACE
    assert call(nbytes=wsb(1000, 768) - 1) == WORKSPACE


def test_patch_rows_bwd_argument_checks_without_a_device():
    f = lib.lib().fn["isic_patch_rows_bwd_f16"]
    for p_ in (1, 3, 8):
        assert f(P, P, None, 2, 56, 56, 256, p_, 0, None) == UNSUPPORTED, p_
    assert f(P, P, None, 2, 56, 56, 260, 4, 0, None) == UNSUPPORTED          # C % 8
    assert f(P, P, None, 2, 30, 28, 256, 4, 0, None) == UNSUPPORTED          # H % P
    assert f(P, P, None, 2, 56, 56, 256, 4, 2, None) == BAD_ARG
    assert f(None, P, None, 2, 56, 56, 256, 4, 0, None) == BAD_ARG
    assert f(None, None, None, 0, 56, 56, 256, 4, 0, None) == 0               # no images: nothing to do


def test_trainable_option_validation():
    from isic_hip.convmae import ConvMAEBaseEncoder
    from isic_hip.lib import IsicHipError
    from model import MultiModalMILNet
    with pytest.raises(ValueError):
        ConvMAEBaseEncoder(trainable=True, fold_layernorm=True)
    frozen = ConvMAEBaseEncoder()
    assert frozen.fold_layernorm is True and not frozen.trainable
    assert not any(p.requires_grad for p in frozen.parameters())
    with pytest.raises(IsicHipError):
        frozen.train()
    enc = ConvMAEBaseEncoder(trainable=True)
    assert enc.fold_layernorm is False and all(p.requires_grad for p in enc.parameters())
    assert enc.train() is enc and enc.training and not enc.eval().training
    assert ConvMAEBaseEncoder(trainable=True, fold_layernorm=False).fold_layernorm is False
    a, b = frozen.state_dict(), enc.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    with pytest.raises(ValueError):
        MultiModalMILNet(encoder="convmae")
    net = MultiModalMILNet(encoder="convmae_base")
    assert isinstance(net.encoder, ConvMAEBaseEncoder) and net.encoder.trainable and net.encoder.out_dim == 768
    assert net.mil.feature_extractor[0].in_features == 768


def test_train_flops_per_image_counts_the_shapes():
    from isic_hip.convmae import ConvMAEBaseEncoder
    enc = ConvMAEBaseEncoder(trainable=True)

    def mm(m, n, k):                                   # one product, forward
        return 2 * m * n * k
    fwd = mm(56 * 56, 256, 48)
    for C, px in ((256, 56 * 56), (384, 28 * 28)):
        fwd += 2 * (mm(px, C, C) * 2 + 2 * px * C * 25 + mm(px, 4 * C, C) * 2)
    fwd += mm(196, 768, 16 * 256) + mm(28 * 28, 384, 4 * 256) + mm(196, 768, 4 * 384) * 2 + mm(196, 768, 768)
    fwd += 11 * (mm(196, 3 * 768, 768) + mm(196, 768, 768) + 2 * mm(196, 3072, 768) + 2 * mm(196, 196, 768))
    assert enc.flops_per_image() == fwd
    assert enc.train_flops_per_image() == 3 * fwd - mm(56 * 56, 256, 48)        # the stem has no data gradient
