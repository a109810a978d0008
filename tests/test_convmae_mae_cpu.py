"""CPU-only checks of the ConvMAE-Base masked autoencoder (isic_hip/convmae_mae.py): its keys and shapes, checkpoint
loading both ways, the masking bookkeeping, patchify / unpatchify, the decoder's position table, the argument errors,
and the entry points of include/isic_hip_mae.h (declared, exported, `stream` last, argument checks before any device
work)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import convmae_mae_ref as mr  # noqa: E402
from isic_hip import lib  # noqa: E402

P = 1 << 20                      # a non-NULL "device" pointer: never dereferenced, the checks answer first
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
ENTRIES = ("isic_dwconv5x5_masked_f16", "isic_dwconv5x5_masked_dgrad_f16", "isic_attention_d32_f16",
           "isic_attention_d32_bwd_f16", "isic_gather_rows_f16", "isic_scatter_rows_f16", "isic_mae_unshuffle_f16",
           "isic_mae_unshuffle_bwd_f16", "isic_mae_loss_f16_workspace_bytes", "isic_mae_loss_f16")


@pytest.fixture(scope="module")
def model():
    from isic_hip.convmae_mae import ConvMAEBase
    return ConvMAEBase()


def test_keys_and_shapes_are_the_encoders_plus_the_decoders(model):
    sd = model.state_dict()
    want = mr.mae_shapes()
    assert list(sd) and set(sd) == set(want)
    assert all(tuple(sd[k].shape) == want[k] for k in want)
    assert not model.decoder_pos_embed.requires_grad
    assert all(p.requires_grad for k, p in model.named_parameters() if k != "decoder_pos_embed")


def test_full_checkpoint_loads_strictly_and_into_the_encoder(model):
    from isic_hip.convmae import ConvMAEBaseEncoder
    from isic_hip.convmae_mae import ConvMAEBase
    ckpt = mr.init_params(3)
    m = ConvMAEBase()
    m.load_state_dict(ckpt, strict=True)
    assert torch.equal(m.decoder_pos_embed, ckpt["decoder_pos_embed"]) and torch.equal(m.mask_token, ckpt["mask_token"])
    res = ConvMAEBaseEncoder().load_state_dict(m.state_dict(), strict=False)
    assert not res.missing_keys
    assert sorted(res.unexpected_keys) == sorted(mr.decoder_shapes())


def test_encoder_init_is_the_encoders_and_seeded(model):
    from isic_hip.convmae import ConvMAEBaseEncoder
    from isic_hip.convmae_mae import ConvMAEBase
    enc = ConvMAEBaseEncoder(seed=0).state_dict()
    sd = model.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in enc.items())
    again = ConvMAEBase(seed=0).state_dict()
    assert all(torch.equal(sd[k], v) for k, v in again.items())
    assert not torch.equal(ConvMAEBase(seed=1).state_dict()["decoder_embed.weight"], sd["decoder_embed.weight"])
    assert abs(float(sd["mask_token"].std()) - 0.02) < 0.005
    assert torch.equal(sd["decoder_norm.weight"], torch.ones(512)) and torch.equal(sd["decoder_pred.bias"], torch.zeros(768))


def test_masking_bookkeeping(model):
    noise = torch.rand(5, 196, generator=torch.Generator().manual_seed(0))
    for ratio in (0.75, 0.5, 0.1):
        m = model.random_masking(5, ratio, noise)
        L = int(196 * (1 - ratio))
        assert m["L"] == L
        assert torch.equal(torch.gather(m["ids_shuffle"], 1, m["ids_restore"]), torch.arange(196).expand(5, 196))
        assert torch.equal(m["mask"].sum(1), torch.full((5,), 196.0 - L))
        assert torch.equal(m["ids_keep"], torch.argsort(noise, 1)[:, :L])
        assert bool((torch.gather(m["mask"], 1, m["ids_keep"]) == 0).all())
        assert torch.equal(m["keep"], (1 - m["mask"]).to(torch.uint8))
        ref = mr.masking(5, ratio, noise)
        assert torch.equal(ref[3], m["mask"]) and torch.equal(ref[1], m["ids_restore"])
    m = model.random_masking(3, 0.0)
    assert torch.equal(m["ids_shuffle"], torch.arange(196).expand(3, 196)) and not bool(m["mask"].any())


def test_patchify_unpatchify_and_the_decoder_position_table(model):
    x = torch.randn(2, 3, 224, 224)
    pt = model.patchify(x)
    assert pt.shape == (2, 196, 768) and torch.equal(model.unpatchify(pt), x)
    assert torch.equal(pt[1, 14 + 2].view(16, 16, 3)[5, 7], x[1, :, 16 + 5, 32 + 7])     # (row, column, channel)
    assert torch.allclose(model.decoder_pos_embed, mr.cr.sincos_pos_embed(512, 14), atol=1e-6, rtol=0)


def test_lesion_mask_and_bad_mask_ratio_raise(model):
    x = torch.zeros(1, 3, 224, 224)
    with pytest.raises(ValueError, match="lesion_mask"):
        model(x, 0.75, lesion_mask=torch.zeros(1, 1, 224, 224))
    for r in (-0.1, 1.0, 1.5, 0.999):
        with pytest.raises(ValueError):
            model.random_masking(1, r)


def test_factory():
    from isic_hip.convmae import ConvMAEBaseEncoder
    from isic_hip.convmae_mae import ConvMAEBase, convmae_convvit_base_patch16_dec512d8b
    e = convmae_convvit_base_patch16_dec512d8b(with_decoder=False)
    assert type(e) is ConvMAEBaseEncoder and not e.trainable
    m = convmae_convvit_base_patch16_dec512d8b(norm_pix_loss=True)
    assert isinstance(m, ConvMAEBase) and m.norm_pix_loss


def test_entry_points_declared_exported_stream_last():
    L = lib.lib()
    assert len(L.public) == 96
    protos = lib.parse_header(os.path.join(os.path.dirname(lib.header_path()), "isic_hip_mae.h"))
    assert set(protos) == set(ENTRIES)
    for name in ENTRIES:
        assert name in L.fn
        if not name.endswith("_workspace_bytes"):
            assert protos[name][1][-1][1] == "stream"


def test_entry_point_argument_checks_without_a_device():
    f = lib.lib().fn
    dw, dg = f["isic_dwconv5x5_masked_f16"], f["isic_dwconv5x5_masked_dgrad_f16"]
    assert dw(P, P, 4, P, P, P, P, 2, 56, 56, 96, None) == UNSUPPORTED           # C % 64
    assert dw(P, P, 3, P, P, P, P, 2, 56, 56, 256, None) == UNSUPPORTED           # H % P
    assert dw(P, None, 4, P, P, P, P, 2, 56, 56, 256, None) == BAD_ARG
    assert dw(None, None, 4, None, None, None, None, 0, 56, 56, 256, None) == 0   # no images
    assert dg(P, P, 0, P, P, 2, 28, 28, 384, None) == BAD_ARG
    a, ab = f["isic_attention_d32_f16"], f["isic_attention_d32_bwd_f16"]
    assert a(P, P, 2, 209, 16, None) == UNSUPPORTED and ab(P, P, P, P, 2, 209, 16, None) == UNSUPPORTED
    assert a(None, P, 2, 196, 16, None) == BAD_ARG and ab(None, P, P, P, 2, 196, 16, None) == BAD_ARG
    for name in ("isic_gather_rows_f16", "isic_scatter_rows_f16"):
        g = f[name]
        assert g(P, P, P, 2, 196, 49, 500, None) == UNSUPPORTED                  # C % 8
        assert g(P, P, P, 2, 196, 197, 512, None) == BAD_ARG                     # L > T
        assert g(P, None, P, 2, 196, 49, 512, None) == BAD_ARG
    assert f["isic_mae_unshuffle_f16"](P, P, None, P, P, 2, 196, 49, 512, None) == BAD_ARG
    assert f["isic_mae_unshuffle_bwd_f16"](P, P, P, None, 2, 196, 49, 512, None) == BAD_ARG
    nb = f["isic_mae_loss_f16_workspace_bytes"](256, 224, 224, 16)
    assert nb == 256 * 196 * 4 and f["isic_mae_loss_f16_workspace_bytes"](2, 224, 224, 15) == 0
    loss = f["isic_mae_loss_f16"]
    assert loss(P, P, P, 0, 10.0, 1.0, P, P, 2, 3, 224, 224, 16, P, 8, None) == WORKSPACE
    assert loss(P, P, P, 2, 10.0, 1.0, P, P, 2, 3, 224, 224, 16, P, 1 << 20, None) == BAD_ARG     # norm_pix
    assert loss(P, P, P, 0, 0.0, 1.0, P, P, 2, 3, 224, 224, 16, P, 1 << 20, None) == BAD_ARG      # mask_sum
    assert loss(P, P, P, 0, 10.0, 1.0, P, P, 2, 3, 224, 224, 32, P, 1 << 20, None) == UNSUPPORTED  # K > 1024


def test_train_ae_config_defaults():
    import importlib
    tae = importlib.import_module("train_ae")
    p = tae.plan({"training_plan": {"parameters": {"masking_ratio": 0.6, "patience": 3}}})
    assert p["masking_ratio"] == 0.6 and p["eval_masking_ratio"] == 0.75 and p["norm_pix_loss"] is False
    tr, va = tae.split([i % 7 for i in range(70)], 0, 42)
    assert len(va) == 7 and len(set(tr) | set(va)) == 70
