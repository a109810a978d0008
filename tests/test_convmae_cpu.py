"""CPU-only checks of the ConvMAE-Base encoder: its state dict is a ConvMAE checkpoint's (keys, shapes, a full MAE
checkpoint with its decoder loads), the default position embedding is the sin-cos formula, the entry points of
include/isic_hip_convmae.h are declared, exported, take `stream` last and answer bad arguments before any device work, and
save_latent validates the encoder / precision pair."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from isic_hip import lib  # noqa: E402

NAMES = ("isic_dwconv5x5_f16", "isic_patch_rows_nhwc_f16", "isic_patch_rows_nchw_f32", "isic_layernorm_add_f16")
BAD_ARG, UNSUPPORTED = -1, -2
P = 0x10000                                         # a non-NULL pointer value: never dereferenced by a rejected call

# the encoder key prefixes of a checkpoint of convmae_convvit_base_patch16_dec512d8b, written out by hand
CHECKPOINT_PREFIXES = (["pos_embed", "patch_embed1.proj", "patch_embed1.norm", "patch_embed2.proj", "patch_embed2.norm",
                        "patch_embed3.proj", "patch_embed3.norm", "patch_embed4", "stage1_output_decode", "stage2_output_decode",
                        "norm"]
                       + [f"blocks{s}.{i}.{m}" for s in (1, 2) for i in range(2)
                          for m in ("norm1", "conv1", "attn", "conv2", "norm2", "mlp.fc1", "mlp.fc2")]
                       + [f"blocks3.{i}.{m}" for i in range(11)
                          for m in ("norm1", "attn.qkv", "attn.proj", "norm2", "mlp.fc1", "mlp.fc2")])


def _enc(**kw):
    from isic_hip.convmae import ConvMAEBaseEncoder
    return ConvMAEBaseEncoder(**kw)


def test_state_dict_keys_and_shapes_match_the_restatement():
    import convmae_ref as ref
    sd = _enc().state_dict()
    shapes = ref.convmae_shapes()
    assert set(sd) == set(shapes)
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in shapes.items())
    assert {k if k == "pos_embed" else k.rsplit(".", 1)[0] for k in sd} == set(CHECKPOINT_PREFIXES)
    enc = _enc()
    assert enc.out_dim == 768 and not any(p.requires_grad for p in enc.parameters())
    assert enc.flops_per_image() / 1e9 == pytest.approx(47.9, abs=0.1)


def _mae_checkpoint():
    import convmae_ref as ref
    sd = {k: v.clone() for k, v in ref.init_params(3).items()}
    g = torch.Generator().manual_seed(1)
    sd["mask_token"] = torch.zeros(1, 1, 512)
    sd["decoder_embed.weight"], sd["decoder_embed.bias"] = torch.randn(512, 768, generator=g), torch.zeros(512)
    sd["decoder_pos_embed"] = torch.zeros(1, 196, 512)
    sd["decoder_blocks.0.attn.qkv.weight"] = torch.randn(1536, 512, generator=g)
    sd["decoder_norm.weight"], sd["decoder_pred.weight"] = torch.ones(512), torch.randn(768, 512, generator=g)
    return sd


def test_full_mae_checkpoint_loads_with_only_decoder_keys_unexpected():
    sd = _mae_checkpoint()
    enc = _enc()
    res = enc.load_state_dict(sd, strict=False)
    assert list(res.missing_keys) == []
    assert set(res.unexpected_keys) == {k for k in sd if k.startswith("decoder_") or k == "mask_token"}
    got = enc.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in got)
    bad = dict(sd)
    bad["blocks1.0.attn.weight"] = torch.zeros(256, 1, 3, 3)
    with pytest.raises(RuntimeError):
        _enc().load_state_dict(bad, strict=False)
    with pytest.raises(RuntimeError):
        _enc().load_state_dict(sd, strict=True)                        # the decoder keys under strict=True


def test_default_pos_embed_is_the_sincos_table():
    import math
    pe = _enc().state_dict()["pos_embed"]
    assert pe.shape == (1, 196, 768) and pe.dtype == torch.float32
    for i, j, k in ((0, 0, 0), (3, 7, 5), (13, 13, 191), (9, 2, 100)):
        w = 10000.0 ** (-k / 192)
        row = pe[0, i * 14 + j]
        for off, val in ((0, math.sin(j * w)), (192, math.cos(j * w)), (384, math.sin(i * w)), (576, math.cos(i * w))):
            assert abs(float(row[off + k]) - val) <= 1e-7, (i, j, k, off)
    import convmae_ref as ref
    assert torch.equal(pe, ref.sincos_pos_embed())


def test_options_and_no_cpu_fallback():
    from isic_hip.lib import IsicHipError
    with pytest.raises(ValueError):
        _enc(fold_layernorm="stats")
    enc = _enc(ln_eps=1e-5, conv_ln_eps=1e-6)
    assert enc.norm.eps == 1e-5 and enc.blocks3[0].norm1.eps == 1e-5
    assert enc.blocks1[0].norm1.eps == 1e-6 and enc.patch_embed2.norm.eps == 1e-6
    d = _enc()
    assert d.norm.eps == 1e-6 and d.blocks1[1].norm2.eps == 1e-5 and d.patch_embed1.norm.eps == 1e-5
    with pytest.raises(IsicHipError):
        d.train()
    with pytest.raises(IsicHipError):
        d.run_tokens(torch.zeros(1, 3, 224, 224))
    with pytest.raises(ValueError):
        d.run_tokens(torch.zeros(1, 3, 128, 128))


def test_convmae_entry_points_are_declared_and_exported():
    inc = os.path.join(ROOT, "include")
    assert '#include "isic_hip_convmae.h"' in open(os.path.join(inc, "isic_hip.h")).read()
    text = open(os.path.join(inc, "isic_hip_convmae.h")).read()
    assert set(re.findall(r"\b(isic_\w+)\s*\(", text)) == set(NAMES)
    L = lib.lib()
    assert len(L.public) == 96
    assert os.path.join(inc, "isic_hip_convmae.h") in [os.path.normpath(p) for p in lib.extension_header_paths()]
    cdll = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in L.extension and name in L.fn and hasattr(cdll, name), name
        assert L.extension[name][1][-1][1] == "stream", name
    assert not any(f.startswith("conv_") and "convmae" in f for f in os.listdir(os.path.join(ROOT, "multimodal-isic_amd", "csrc")))


def test_argument_checks_without_a_device():
    L = lib.lib().fn
    dw = L["isic_dwconv5x5_f16"]
    assert dw(P, P, P, P, 2, 56, 56, 96, None) == UNSUPPORTED            # C % 64
    assert dw(P, P, P, P, -1, 56, 56, 256, None) == BAD_ARG
    assert dw(P, P, P, P, 2, 0, 56, 256, None) == BAD_ARG
    assert dw(None, P, P, P, 2, 56, 56, 256, None) == BAD_ARG
    assert dw(P, None, P, P, 2, 56, 56, 256, None) == BAD_ARG
    assert dw(None, None, None, None, 0, 56, 56, 256, None) == 0        # no images: nothing to do
    pr = L["isic_patch_rows_nhwc_f16"]
    assert pr(P, P, 2, 56, 56, 256, 3, None) == UNSUPPORTED              # P not in {2, 4}
    assert pr(P, P, 2, 56, 56, 12, 2, None) == UNSUPPORTED               # C % 8
    assert pr(P, P, 2, 57, 56, 256, 2, None) == UNSUPPORTED              # H % P
    assert pr(None, P, 2, 56, 56, 256, 2, None) == BAD_ARG
    assert pr(P, P, -2, 56, 56, 256, 2, None) == BAD_ARG
    pc = L["isic_patch_rows_nchw_f32"]
    assert pc(P, P, 2, 3, 224, 224, 4, 40, None) == UNSUPPORTED           # K_out < C*P*P
    assert pc(P, P, 2, 3, 224, 224, 4, 60, None) == UNSUPPORTED           # K_out % 8
    assert pc(P, P, 2, 3, 222, 224, 4, 64, None) == UNSUPPORTED
    assert pc(P, None, 2, 3, 224, 224, 4, 64, None) == BAD_ARG
    ln = L["isic_layernorm_add_f16"]
    assert ln(P, None, None, P, P, P, None, 100, 1088, 0, 1e-6, None) == UNSUPPORTED    # N > 1024
    assert ln(P, None, None, P, P, P, None, 100, 200, 0, 1e-6, None) == UNSUPPORTED     # N % 64
    assert ln(P, None, None, P, P, P, None, 100, 768, 2, 1e-6, None) == BAD_ARG
    assert ln(P, None, None, P, P, None, None, 100, 768, 0, 1e-6, None) == BAD_ARG      # no output
    assert ln(P, None, None, None, P, P, None, 100, 768, 0, 1e-6, None) == BAD_ARG
    assert ln(P, None, None, P, P, P, None, -1, 768, 0, 1e-6, None) == BAD_ARG
    assert ln(None, None, None, None, None, None, None, 0, 768, 0, 1e-6, None) == 0


def test_save_latent_rejects_convmae_with_mxfp8():
    import save_latent
    ds = save_latent.SyntheticDermImages(n=2)
    for name in ("convmae_base", "convmae", "convmae_convvit_base_patch16"):
        with pytest.raises(ValueError):
            save_latent.extract_latents({"encoder": name, "encoder_precision": "mxfp8", "device": "cpu"}, "none.pth",
                                        datasets=(ds, ds))
