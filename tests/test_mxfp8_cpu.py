"""CPU-only checks of the MXFP8 path of the ViT-S/16 encoder: the three entry points are declared (include/isic_hip_mxfp8.h,
included by isic_hip.h) and exported, their argument checks answer before any device work, the reference quantiser
(tests/mxfp8_ref.py) passes hand-checked blocks, and the encoder's precision option validates its combinations."""
import ctypes
import os
import re

import pytest
import torch

import mxfp8_ref as mr
from isic_hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("isic_mxfp8_quantize", "isic_layernorm_mxfp8_f16", "isic_gemm_mxfp8")
BAD_ARG, UNSUPPORTED = -1, -2
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call


def test_mxfp8_entry_points_are_declared_and_exported():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_mxfp8.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = open(os.path.join(inc, "isic_hip_mxfp8.h")).read()
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    L = lib.lib()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name in L.fn and hasattr(cdll, name), name
        assert L.extension[name][1][-1][1] == "stream"                     # stream last


def test_gemm_mxfp8_argument_checks_without_a_device():
    g = lib.lib().fn["isic_gemm_mxfp8"]

    def call(M=100, N=384, K=384, act=0, rr=0, ops=(P, P, P, P), res=None, C=P, Cq=None, Cs=None):
        return g(*ops, None, res, C, Cq, Cs, M, N, K, act, rr, None)
    assert call(K=320) == UNSUPPORTED                                      # K % 128
    assert call(N=320) == UNSUPPORTED                                      # N % 128
    assert call(K=64, N=64) == UNSUPPORTED
    assert call(C=P, Cq=P, Cs=P) == BAD_ARG                                # both outputs
    assert call(C=None) == BAD_ARG                                         # no output
    assert call(C=None, Cq=P, Cs=None) == BAD_ARG                          # MX output without its scales
    assert call(ops=(None, P, P, P)) == BAD_ARG                            # NULL operands
    assert call(ops=(P, P, P, None)) == BAD_ARG
    assert call(M=-1) == BAD_ARG
    assert call(act=2) == BAD_ARG
    assert call(rr=196) == BAD_ARG                                         # broadcast residual without a residual
    assert call(M=0) == 0                                                  # nothing to do
    q = lib.lib().fn["isic_mxfp8_quantize"]
    assert q(P, 0, P, P, 10, 48, None) == UNSUPPORTED                      # K % 32
    assert q(P, 2, P, P, 10, 64, None) == BAD_ARG
    assert q(None, 0, P, P, 10, 64, None) == BAD_ARG
    assert q(P, 1, None, P, 10, 64, None) == BAD_ARG
    assert q(P, 1, P, P, 0, 64, None) == 0
    ln = lib.lib().fn["isic_layernorm_mxfp8_f16"]
    assert ln(P, P, P, P, P, 10, 256, ctypes.c_float(1e-6), None) == UNSUPPORTED
    assert ln(P, None, P, P, P, 10, 384, ctypes.c_float(1e-6), None) == BAD_ARG
    assert ln(P, P, P, P, P, -1, 384, ctypes.c_float(1e-6), None) == BAD_ARG


def _block(vals, fill=0.0, dtype=torch.float32):
    b = torch.full((1, 32), fill, dtype=torch.float32)
    for i, v in vals.items():
        b[0, i] = v
    return b.to(dtype)


def test_reference_all_zero_block_and_negative_zeros():
    q, s = mr.quantize(_block({3: -0.0, 7: -0.0}))
    assert int(s) == 0 and q.tolist() == [[0] * 32]                        # +0 everywhere, scale byte 0
    q, s = mr.quantize(_block({0: 1.0, 3: -0.0, 4: -1e-9}))
    assert int(s) == 127 - 8 and q[0, 3] == 0x80 and q[0, 4] == 0x80 and q[0, 1] == 0     # signed zeros inside a live block


def test_reference_amax_at_and_just_above_the_e4m3_maximum():
    for e in (-20, 0, 3):
        top = 448.0 * 2.0 ** e
        q, s = mr.quantize(_block({0: top, 1: -top / 2}))
        assert int(s) == e + 127 and int(q[0, 0]) == 0x7E and int(q[0, 1]) == 0xF6      # 448, -224
        q, s = mr.quantize(_block({0: top * (1 + 2.0 ** -20)}))
        assert int(s) == e + 128 and int(q[0, 0]) == 0x76                              # 224: next exponent
    q, s = mr.quantize(_block({5: 1.0}))
    assert int(s) == 127 - 8 and int(q[0, 5]) == 0x78                                  # 1 * 2^8 = 256


def test_reference_lone_outlier_over_tiny_values_with_subnormals():
    # amax 100 = 0.78 * 2^7 -> e = -2 (100 <= 448 / 4); 100 * 4 = 400 is the tie between 384 and 416 -> even 384 = 0x7C;
    # 1e-3 * 4 = 0.004 = 2.048 * 2^-9 -> the e4m3 subnormal 2 * 2^-9 = 0x02
    q, s = mr.quantize(_block({5: 100.0}, fill=1e-3))
    assert int(s) == 125 and int(q[0, 5]) == 0x7C and int(q[0, 0]) == 0x02
    d = mr.dequantize(q, s)[0]
    assert float(d[5]) == 96.0 and float(d[0]) == 2 * 2.0 ** -9 / 4
    # e = 0: subnormal steps of 2^-9 with ties to even: 0.5 -> 0, 1.5 -> 2, 0.25 -> 0, -2.5 -> -2
    q, s = mr.quantize(_block({0: 448.0, 1: 2.0 ** -10, 2: 3 * 2.0 ** -10, 3: 2.0 ** -11, 4: -5 * 2.0 ** -10}))
    assert int(s) == 127 and q[0, :5].tolist() == [0x7E, 0x00, 0x02, 0x00, 0x82]


def test_reference_fp16_extremes():
    # 65504 = 0.9995 * 2^16 -> e = 8; 65504 / 256 = 255.875 -> 256 = 0x78; +-6e-8 (2^-24) vanish to signed zeros beside it
    q, s = mr.quantize(_block({0: 65504.0, 9: 6e-8, 10: -6e-8}, dtype=torch.float16))
    assert int(s) == 127 + 8 and int(q[0, 0]) == 0x78
    assert int(q[0, 9]) == 0 and int(q[0, 10]) == 0x80
    # a lone fp16 subnormal 2^-24: e = -32, 2^-24 * 2^32 = 256 = 0x78, and it dequantises exactly
    v = float(torch.tensor(6e-8, dtype=torch.float16))
    q, s = mr.quantize(_block({9: v}, dtype=torch.float16))
    assert v == 2.0 ** -24 and int(s) == 127 - 32 and int(q[0, 9]) == 0x78
    assert float(mr.dequantize(q, s)[0, 9]) == v


def test_reference_round_trips_bytes():
    # bytes -> values -> bytes is the identity for every block whose largest element is above 224 at its scale (what the
    # rule produces, except where a block's amax rounds down onto 224 and the next smaller scale also fits)
    g = torch.Generator().manual_seed(3)
    q = torch.randint(0, 256, (37, 384), generator=g, dtype=torch.uint8)
    q = torch.where((q & 0x7F) == 0x7F, q ^ 0x01, q)                     # no NaN encodings
    top = torch.randint(0x77, 0x7F, (37, 12), generator=g, dtype=torch.uint8) | (q[:, ::32] & 0x80)
    q = q.view(37, 12, 32).clone()
    q[:, :, 7] = top
    q = q.view(37, 384)
    s = torch.randint(30, 220, (37, 12), generator=g, dtype=torch.uint8)     # values stay normal fp32 numbers
    q2, s2 = mr.quantize(mr.dequantize(q, s))
    assert torch.equal(q, q2) and torch.equal(s, s2)
    # values -> bytes -> values: within half an e4m3 step of the block's largest value (2^-4 of it)
    x = torch.randn(37, 384, generator=g) * torch.exp2(torch.randint(-30, 30, (37, 1), generator=g).float())
    q, s = mr.quantize(x)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and s.shape == (37, 12)
    d = mr.dequantize(q, s)
    assert bool(((d - x).abs() <= x.abs().view(37, 12, 32).amax(-1).repeat_interleave(32, 1) * 2.0 ** -4).all())


def test_encoder_precision_option():
    from isic_hip.vit import ViTSmallEncoder
    enc = ViTSmallEncoder(img_size=32, depth=1, precision="mxfp8")
    assert enc.precision == "mxfp8" and ViTSmallEncoder(img_size=32, depth=1).precision == "fp16"
    assert list(enc.state_dict()) == list(ViTSmallEncoder(img_size=32, depth=1).state_dict())
    with pytest.raises(ValueError):
        ViTSmallEncoder(img_size=32, depth=1, precision="mxfp8", fold_layernorm=False)
    with pytest.raises(ValueError):
        ViTSmallEncoder(img_size=32, depth=1, precision="mxfp8", fold_layernorm="stats")
    with pytest.raises(ValueError):
        ViTSmallEncoder(img_size=32, depth=1, precision="fp8")


def test_extract_latents_rejects_mxfp8_with_the_resnet_encoder():
    import save_latent as sl
    tv = sl.SyntheticDermImages(n=2, seed=1)
    with pytest.raises(ValueError):
        sl.extract_latents({"device": "cpu", "encoder_precision": "mxfp8"}, "missing.pth", datasets=(tv, tv), batch_size=2)
    with pytest.raises(ValueError):
        sl.extract_latents({"device": "cpu", "encoder": "vit_s16", "encoder_precision": "int8"}, "missing.pth",
                           datasets=(tv, tv), batch_size=2)
