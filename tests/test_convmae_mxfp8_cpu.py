"""CPU-only checks of the MXFP8 path of the ConvMAE-Base encoder: the three entry points of
include/isic_hip_convmae_mxfp8.h are declared, exported, take `stream` last and answer bad arguments before any device
work; the encoder's precision option validates its combinations; save_latent keeps rejecting the pair on a CPU device;
and the CPU emulation (tests/convmae_mxfp8_ref.py) reproduces the figures the GPU bounds of test_convmae_mxfp8_gpu.py
stand on."""
import ctypes
import os
import re

import pytest
import torch

from isic_hip import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("isic_layernorm_act_mxfp8_f16", "isic_dwconv5x5_mxfp8_f16", "isic_patch_rows_mxfp8_nhwc_f16")
BAD_ARG, UNSUPPORTED = -1, -2
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call
EPS = ctypes.c_float(1e-5)


def test_entry_points_are_declared_and_exported():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_convmae_mxfp8.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = open(os.path.join(inc, "isic_hip_convmae_mxfp8.h")).read()
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    assert os.path.join(inc, "isic_hip_convmae_mxfp8.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    L = lib.lib()
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name not in L.public and name in L.fn and hasattr(cdll, name), name
        assert L.extension[name][1][-1][1] == "stream", name


def test_layernorm_act_mxfp8_argument_checks_without_a_device():
    ln = lib.lib().fn["isic_layernorm_act_mxfp8_f16"]

    def call(x=P, g=P, b=P, q=P, s=P, M=100, N=768, act=0):
        return ln(x, g, b, q, s, M, N, act, EPS, None)
    assert call(N=200) == UNSUPPORTED                                      # N % 64
    assert call(N=1088) == UNSUPPORTED                                     # N > 1024
    assert call(N=32) == UNSUPPORTED
    assert call(q=None) == BAD_ARG and call(s=None) == BAD_ARG             # NULL outputs
    assert call(x=None) == BAD_ARG and call(g=None) == BAD_ARG and call(b=None) == BAD_ARG
    assert call(M=-1) == BAD_ARG
    assert call(act=2) == BAD_ARG and call(act=-1) == BAD_ARG
    assert call(N=0) == BAD_ARG
    assert ln(P, P, P, P, P, 100, 768, 0, ctypes.c_float(-1.0), None) == BAD_ARG
    assert call(M=0) == 0 and call(x=None, q=None, s=None, M=0) == 0       # nothing to do
    for N in (64, 256, 384, 768, 1024):                                    # the domain of isic_layernorm_add_f16
        assert call(M=0, N=N) == 0
    # the ViT's entry keeps its own domain: the wider LayerNorm is a new entry, not a widening of the old one
    assert lib.lib().fn["isic_layernorm_mxfp8_f16"](P, P, P, P, P, 10, 256, ctypes.c_float(1e-6), None) == UNSUPPORTED


def test_dwconv5x5_mxfp8_argument_checks_without_a_device():
    dw = lib.lib().fn["isic_dwconv5x5_mxfp8_f16"]

    def call(x=P, w=P, b=P, q=P, s=P, N=2, H=56, W=56, C=256):
        return dw(x, w, b, q, s, N, H, W, C, None)
    assert call(C=48) == UNSUPPORTED and call(C=96) == UNSUPPORTED         # C % 64
    assert call(q=None) == BAD_ARG and call(s=None) == BAD_ARG             # NULL outputs
    assert call(x=None) == BAD_ARG and call(w=None) == BAD_ARG
    assert call(N=-1) == BAD_ARG and call(H=0) == BAD_ARG and call(W=0) == BAD_ARG and call(C=0) == BAD_ARG
    assert call(N=0) == 0 and call(x=None, w=None, b=None, q=None, s=None, N=0) == 0


def test_patch_rows_mxfp8_argument_checks_without_a_device():
    pr = lib.lib().fn["isic_patch_rows_mxfp8_nhwc_f16"]

    def call(x=P, q=P, s=P, N=2, H=56, W=56, C=256, Pp=2):
        return pr(x, q, s, N, H, W, C, Pp, None)
    assert call(Pp=3) == UNSUPPORTED and call(Pp=8) == UNSUPPORTED         # P in {2, 4}
    assert call(C=48) == UNSUPPORTED and call(C=8) == UNSUPPORTED          # C % 32: a block may not straddle a pixel
    assert call(H=57) == UNSUPPORTED and call(W=58, Pp=4) == UNSUPPORTED   # H % P, W % P
    assert call(q=None) == BAD_ARG and call(s=None) == BAD_ARG and call(x=None) == BAD_ARG
    assert call(N=-1) == BAD_ARG and call(H=0) == BAD_ARG and call(Pp=0) == BAD_ARG
    assert call(N=0) == 0 and call(x=None, q=None, s=None, N=0) == 0


def test_encoder_precision_option():
    from isic_hip.convmae import ConvMAEBaseEncoder
    from isic_hip.convmae_mae import convmae_convvit_base_patch16_dec512d8b as factory
    ref = ConvMAEBaseEncoder()
    assert ref.precision == "fp16" and ref.fold_layernorm is True
    enc = ConvMAEBaseEncoder(precision="mxfp8")
    assert enc.precision == "mxfp8" and not any(p.requires_grad for p in enc.parameters())
    assert list(enc.state_dict()) == list(ref.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(enc.state_dict().values(), ref.state_dict().values()))
    assert ConvMAEBaseEncoder(precision="mxfp8", fold_layernorm=True, max_batch=1).precision == "mxfp8"
    assert factory(with_decoder=False, precision="mxfp8").precision == "mxfp8"
    for kw in (dict(precision="fp8"), dict(precision="MXFP8"), dict(precision=None),
               dict(precision="mxfp8", trainable=True), dict(precision="mxfp8", fold_layernorm=False)):
        with pytest.raises(ValueError):
            ConvMAEBaseEncoder(**kw)
    with pytest.raises(lib.IsicHipError):                                  # no CPU fallback
        enc.run_tokens(torch.zeros(1, 3, 224, 224))


def test_extract_latents_rejects_convmae_mxfp8_on_a_cpu_device():
    import save_latent as sl
    ds = sl.SyntheticDermImages(n=2)
    with pytest.raises(ValueError, match="GPU"):
        sl.extract_latents({"encoder": "convmae_base", "encoder_precision": "mxfp8", "device": "cpu"}, "none.pth",
                           datasets=(ds, ds))
    with pytest.raises(ValueError):                                        # the ResNet-18 rejection is unchanged
        sl.extract_latents({"device": "cpu", "encoder_precision": "mxfp8"}, "none.pth", datasets=(ds, ds), batch_size=2)


# depth -> (relative Frobenius error of the emulation against the fp32 oracle (E32), its minimum per-token cosine, the
# emulation against itself with fp64 products (E64)); convmae_ref.init_params(0), x = randn(2, 3, 224, 224) of seed 11
EMULATION_FIGURES = {(0, 0, 0): (0.0499, 0.99844, 8.6e-4), (1, 0, 0): (0.0666, 0.99724, 6.4e-3),
                     (1, 1, 1): (0.0804, 0.99598, 0.0232), None: (0.0914, 0.99459, 0.0455)}


@pytest.mark.parametrize("depth", list(EMULATION_FIGURES), ids=["depth000", "depth100", "depth111", "full"])
def test_emulation_reproduces_its_recorded_figures(depth):
    import convmae_mxfp8_ref as mref
    import convmae_ref as cref
    e32, cos, e64 = EMULATION_FIGURES[depth]
    threads = torch.get_num_threads()
    torch.set_num_threads(16)
    try:
        p = cref.init_params(0)
        x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(11))
        emu = mref.forward_tokens_mxfp8(p, x, depth=depth)
        emu64 = mref.forward_tokens_mxfp8(p, x, depth=depth, products_fp64=True)
        ref = cref.forward_tokens(p, x, depth=depth)
    finally:
        torch.set_num_threads(threads)

    def relf(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())
    got32, got64 = relf(emu, ref), relf(emu, emu64)
    gotcos = float(torch.nn.functional.cosine_similarity(emu.double(), ref.double(), dim=-1).min())
    print(f"depth {depth}: E32 {got32:.4f} min cosine {gotcos:.5f} E64 {got64:.3e}")
    assert got32 == pytest.approx(e32, rel=0.1)
    assert got64 == pytest.approx(e64, rel=0.1)
    assert 1 - gotcos == pytest.approx(1 - cos, rel=0.1)
