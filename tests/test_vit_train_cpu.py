"""CPU-only checks of the ViT-S/16 training path: the entry points of include/isic_hip_vit_train.h are declared, exported
and take `stream` last (isic_hip.h itself keeps its 97), their argument checks answer before any device work, and the
encoder / model options validate their combinations."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)

from isic_hip import lib  # noqa: E402

NAMES = ("isic_gemm_f16_wgrad_workspace_bytes", "isic_gemm_f16_wgrad", "isic_colsum_f16_workspace_bytes", "isic_colsum_f16",
         "isic_attention_bwd_f16", "isic_gemm_f16_dgelu", "isic_gemm_f16_gelu_pre")
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call


def test_vit_train_entry_points_are_declared_and_exported():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_vit_train.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = open(os.path.join(inc, "isic_hip_vit_train.h")).read()
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    L = lib.lib()
    assert len(L.public) == 96
    assert os.path.join(inc, "isic_hip_vit_train.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name in L.fn and hasattr(cdll, name), name
        if not name.endswith("_workspace_bytes"):
            assert L.extension[name][1][-1][1] == "stream", name


def test_wgrad_argument_checks_without_a_device():
    f = lib.lib().fn["isic_gemm_f16_wgrad"]

    def call(M=1000, N=384, K=384, acc=0, ws=None, wsb=0, dW=P):
        return f(P, P, dW, None, M, N, K, 1.0, acc, ws, wsb, None)
    for n, k in ((100, 384), (384, 100), (320, 384), (384, 64), (8192, 384)):
        assert call(N=n, K=k) == UNSUPPORTED, (n, k)
    assert call(M=-1) == BAD_ARG
    assert call(acc=2) == BAD_ARG
    assert call(dW=None) == BAD_ARG
    assert call(M=200704, N=1152, K=384) == WORKSPACE                    # needs slabs, none given
    ws = lib.lib().fn["isic_gemm_f16_wgrad_workspace_bytes"]
    assert ws(200704, 1152, 384) > 0 and ws(10, 100, 384) == 0


def test_attention_bwd_argument_checks_without_a_device():
    f = lib.lib().fn["isic_attention_bwd_f16"]
    assert f(P, P, P, P, 2, 209, 6, 64, None) == UNSUPPORTED                # T > 208
    assert f(P, P, P, P, 2, 196, 6, 32, None) == UNSUPPORTED                # head width != 64
    assert f(P, P, P, P, 2, 196, 6, 128, None) == UNSUPPORTED
    assert f(P, P, P, P, -1, 196, 6, 64, None) == BAD_ARG
    assert f(None, P, P, P, 2, 196, 6, 64, None) == BAD_ARG
    assert f(None, None, None, None, 0, 196, 6, 64, None) == 0             # no images: nothing to do


def test_layernorm_bwd_colsum_and_gemm_mode_argument_checks_without_a_device():
    L = lib.lib().fn
    cs = L["isic_colsum_f16"]
    assert cs(P, P, 10, 12, 1.0, 0, None, 0, None) == UNSUPPORTED             # cols % 8
    assert cs(P, P, 100000, 384, 1.0, 0, None, 0, None) == WORKSPACE
    dg = L["isic_gemm_f16_dgelu"]
    assert dg(P, P, P, P, 100, 100, 384, None) == UNSUPPORTED
    assert dg(P, P, None, P, 100, 384, 384, None) == BAD_ARG
    gp = L["isic_gemm_f16_gelu_pre"]
    assert gp(P, P, None, P, P, 100, 1536, 100, None) == UNSUPPORTED
    assert gp(P, P, None, P, None, 100, 1536, 384, None) == BAD_ARG


def test_trainable_option_validation():
    from isic_hip.vit import ViTSmallEncoder
    from model import MultiModalMILNet
    with pytest.raises(ValueError):
        ViTSmallEncoder(img_size=32, depth=1, trainable=True, precision="mxfp8")
    with pytest.raises(ValueError):
        ViTSmallEncoder(img_size=32, depth=1, trainable=True, fold_layernorm=True)
    with pytest.raises(ValueError):
        MultiModalMILNet(encoder="bogus")
    frozen = ViTSmallEncoder(img_size=32, depth=1)
    assert frozen.fold_layernorm is True and not any(p.requires_grad for p in frozen.parameters())
    with pytest.raises(Exception):
        frozen.train()
    enc = ViTSmallEncoder(img_size=32, depth=1, trainable=True)
    assert enc.fold_layernorm is False and all(p.requires_grad for p in enc.parameters())
    assert enc.train() is enc and enc.training
    net = MultiModalMILNet(encoder="vit_s16", encoder_kwargs=dict(img_size=32, depth=2))
    assert isinstance(net.encoder, ViTSmallEncoder) and net.encoder.trainable and net.encoder.out_dim == 384
    assert net.mil.feature_extractor[0].in_features == 384
