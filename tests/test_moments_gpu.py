"""The token statistics on the MI355X: ``isic_token_moments_f32`` through the ABI against the fp64 restatement and the
derived bounds of tests/moments_ref.py (max and median exactly), over every slab width, both load paths, padded layouts,
tie-heavy and constant channels; the reference's recorded outputs; bit-reproducibility; the Python layers and the two
opt-in call sites (``save_latent`` ``device_moments``, ``train_ae`` ``latent_moments``)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moments_ref as R  # noqa: E402
from isic_hip.lib import call  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRY = "isic_token_moments_f32"
SENTINEL = -777.25


def run_entry(x, eps=R.EPS, unbiased=False, ldx=None, ldo=None, misalign=False):
    """x [B, T, D] fp32 numpy -> (out [B, 6 D] numpy, the padding of out or None).  ``ldx`` / ``ldo``: padded leading
    dimensions (the padding of X holds a large value that must not be read into any statistic); ``misalign``: X starts 4 bytes
    past a 16-byte boundary."""
    B, T, D = x.shape
    ldx, ldo = ldx or D, ldo or 6 * D
    store = torch.full((B * T * ldx + 1,), 1e30, dtype=torch.float32)
    off = 1 if misalign else 0
    store[off:off + B * T * ldx].view(B * T, ldx)[:, :D] = torch.from_numpy(x).reshape(B * T, D)
    store = store.to(DEV)
    assert store.data_ptr() % 16 == 0
    out = torch.full((B, ldo), SENTINEL, device=DEV, dtype=torch.float32)
    call(ENTRY, store.data_ptr() + 4 * off, B, T, D, ldx, float(eps), int(unbiased), out, ldo)
    o = out.cpu().numpy()
    return o[:, :6 * D], (o[:, 6 * D:] if ldo > 6 * D else None)


def check(x, got, eps, unbiased, tag):
    ref, bound = R.reference(x, eps, unbiased), R.bounds(x, eps, unbiased)
    per = R.worst_per_stat(got, ref, bound)
    print(f"{tag}: worst error / bound {per}")
    assert R.selections_equal(got, ref), tag
    assert max(per.values()) <= 1.0, (tag, per)


GRID = list(itertools.product(R.DEVICE_T, R.DEVICE_D, R.DEVICE_B))


@pytest.mark.parametrize("T,D,B", GRID)
def test_entry_against_the_restatement(T, D, B):
    """every slab width (T on both sides of 256 and 512), the 16-byte path (D = 64, 768), the element path (D = 1, 7, 65: ldx
    is no multiple of 4) and slab tails; `unbiased` alternates over the grid"""
    unbiased = T > 1 and (T + D + B) % 2 == 1
    x = R.make_input("mixed", B, T, D)
    got, _ = run_entry(x, R.EPS, unbiased)
    check(x, got, R.EPS, unbiased, f"T {T} D {D} B {B} unbiased {unbiased}")


@pytest.mark.parametrize("unbiased", (False, True))
@pytest.mark.parametrize("kind,B,T,D,ldx,ldo,misalign", (
    ("mixed", 3, 197, 65, 68, 6 * 65 + 5, False),      # 16-byte path with a partial vector at the slab tail
    ("mixed", 2, 5, 7, 9, 50, False),                   # element path, padded
    ("mixed", 2, 196, 64, 64, 384, True),               # ldx % 4 == 0 but X not 16-byte aligned: element path
    ("mixed", 2, 600, 20, 24, 121, False),              # W = 16, padded
))
def test_padded_and_misaligned_layouts(kind, B, T, D, ldx, ldo, misalign, unbiased):
    x = R.make_input(kind, B, T, D)
    got, pad = run_entry(x, R.EPS, unbiased, ldx, ldo, misalign)
    check(x, got, R.EPS, unbiased, f"padded T {T} D {D} ldx {ldx} ldo {ldo}")
    assert pad is None or bool((pad == SENTINEL).all())                         # the padding of out is left untouched
    dense, _ = run_entry(x, R.EPS, unbiased)
    assert np.array_equal(dense.view(np.uint32), got.view(np.uint32))       # the layout and the load path change no bit


@pytest.mark.parametrize("unbiased", (False, True))
@pytest.mark.parametrize("kind,B,T,D", (("ties", 3, 196, 64), ("ties", 2, 1024, 7), ("ties", 2, 300, 33), ("const", 2, 196, 7),
                                        ("const", 3, 2, 65), ("offset", 2, 197, 64), ("normal", 1, 513, 64)))
def test_ties_constant_channels_and_offsets(kind, B, T, D, unbiased):
    x = R.make_input(kind, B, T, D)
    got, _ = run_entry(x, R.EPS, unbiased)
    check(x, got, R.EPS, unbiased, f"{kind} T {T} D {D}")
    if kind == "const":
        assert tuple(got[0, 0::D]) == R.CONST_ROW and tuple(got[B - 1, 0::D]) == R.CONST_ROW


def test_all_values_equal_and_two_values():
    """the selection with EVERY value tied, and with two distinct values split around the rank"""
    x = np.full((2, 196, 64), -1.75, dtype=np.float32)
    got, _ = run_entry(x)
    assert (got[:, 64:128] == -1.75).all() and (got[:, 192:256] == -1.75).all()
    y = np.where(np.arange(196)[None, :, None] % 2 == 0, np.float32(-3.0), np.float32(2.0)) * np.ones((2, 1, 64), dtype=np.float32)
    y[:, 0, 1] = 2.0                                                            # channel 1: 97 lows, 99 highs -> rank 97 is high
    got, _ = run_entry(y.astype(np.float32))
    assert got[0, 192] == -3.0 and got[0, 193] == 2.0
    check(y.astype(np.float32), got, R.EPS, False, "two values")


@pytest.mark.parametrize("key,name,unbiased", R.golden_keys())
def test_recorded_reference_outputs(key, name, unbiased):
    """the device against what the reference's concat_patch_moments gave on the CPU: both are fp32 evaluations inside the
    bound, so they lie within twice the bound of each other; max and median are equal"""
    with np.load(R.GOLDEN) as z:
        rec = z[key]
    x = R.golden_input(name)
    got, _ = run_entry(x, R.EPS, unbiased)
    check(x, got, R.EPS, unbiased, f"golden {key}")
    bound = R.bounds(x, R.EPS, unbiased)
    assert R.selections_equal(got, rec)
    assert R.worst(got, rec.astype(np.float64), 2.0 * bound) <= 1.0


def test_two_calls_equal_bits_and_a_row_does_not_depend_on_its_batch():
    for T, D in ((196, 768), (300, 33), (1024, 7)):
        x = R.make_input("mixed", 3, T, D, seed=5)
        a, _ = run_entry(x, R.EPS, True)
        b, _ = run_entry(x, R.EPS, True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        for i in range(3):
            alone, _ = run_entry(x[i:i + 1], R.EPS, True)
            assert np.array_equal(alone.view(np.uint32), a[i:i + 1].view(np.uint32)), (T, D, i)


def test_python_layers_equal_the_entry():
    import utils
    from isic_hip.moments import token_moments
    x = R.make_input("mixed", 3, 196, 96, seed=2)
    want, _ = run_entry(x, 1e-3, True)
    xd = torch.from_numpy(x).to(DEV)
    for fn in (utils.concat_patch_moments, token_moments):
        got = fn(xd, eps=1e-3, unbiased=True)
        assert got.shape == (3, 6 * 96) and got.dtype == torch.float32 and got.device == xd.device
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    dflt, _ = run_entry(x)
    assert np.array_equal(utils.concat_patch_moments(xd).cpu().numpy().view(np.uint32), dflt.view(np.uint32))
    # a channel slice of a wider grid is read in place (ldx = 96); a transposed view is made contiguous
    lo, _ = run_entry(np.ascontiguousarray(x[:, :, :40]))
    assert np.array_equal(token_moments(xd[:, :, :40]).cpu().numpy().view(np.uint32), lo.view(np.uint32))
    xt = np.ascontiguousarray(x.transpose(0, 2, 1))                             # [3, 96, 196]
    tr, _ = run_entry(xt)
    assert np.array_equal(token_moments(xd.transpose(1, 2)).cpu().numpy().view(np.uint32), tr.view(np.uint32))
    assert token_moments(xd[:0]).shape == (0, 6 * 96)
    g = xd.clone().requires_grad_(True)
    with pytest.raises(RuntimeError):
        token_moments(g)
    with torch.no_grad():
        assert torch.equal(token_moments(g), token_moments(xd))


def test_extract_latents_device_moments(tmp_path, monkeypatch):
    import save_latent as sl
    monkeypatch.chdir(tmp_path)                                                 # extract_latents writes dataframes_latents/ here
    cfg = {"device": DEV, "seed": 42, "pca": False}
    data = (sl.SyntheticDermImages(n=4), sl.SyntheticDermImages(n=4, seed=5))
    base = sl.extract_latents(cfg, "missing.pth", datasets=data, batch_size=4)
    dev = sl.extract_latents(dict(cfg, device_moments=True), "missing.pth", datasets=data, batch_size=4)
    for k in (2, 3):                                                            # the pooled frames
        assert list(base[k].columns) == list(dev[k].columns) and len(base[k]) == len(dev[k]) == 4
        for col in ("image_path", "segmentation_path", "target"):
            assert list(base[k][col]) == list(dev[k][col])
        for i in range(4):
            assert np.array_equal(base[k]["latent_pooled_max"].iloc[i], dev[k]["latent_pooled_max"].iloc[i])
            assert np.abs(base[k]["latent_pooled_mean"].iloc[i] - dev[k]["latent_pooled_mean"].iloc[i]).max() <= 1e-5
    for k in (0, 1, 4, 5):                                                      # the patch and raw frames do not depend on the key
        assert len(base[k]) == len(dev[k]) and list(base[k].columns) == list(dev[k].columns)
    assert np.array_equal(np.stack(base[4]["latent"].values), np.stack(dev[4]["latent"].values))


@pytest.mark.parametrize("device_augment", (False, True))
def test_train_ae_latent_moments(tmp_path, device_augment):
    import train_ae
    if device_augment:
        from isic_hip.augment import SyntheticDermPixels
        ds = SyntheticDermPixels(n=70)
    else:
        from save_latent import SyntheticDermImages
        ds = SyntheticDermImages(n=70)
    labels = [i % ds.classes for i in range(len(ds))]
    config = {"device": DEV, "seed": 42, "training_plan": {"parameters": {
        "epochs": 1, "batch_size": 8, "latent_moments": True, "device_augment": device_augment}}}
    lines = []
    path, history = train_ae.train(config, ds, labels, str(tmp_path), log=lines.append)
    assert os.path.exists(path) and len(history) == 1 and len(lines) == 2
    assert os.listdir(tmp_path / "models") == [os.path.basename(path)]
    assert os.listdir(tmp_path / "latent_moments") == ["epoch_0000.npz"]
    _, va = train_ae.split(labels, 0, 42)
    with np.load(tmp_path / "latent_moments" / "epoch_0000.npz") as z:
        feats, target = z["feats"], z["target"]
    assert feats.shape == (7, 6 * 768) and feats.dtype == np.float32 and np.isfinite(feats).all()
    assert target.dtype == np.int64 and np.array_equal(target, np.asarray(labels)[va])
    assert (feats[:, 768:1536] >= feats[:, :768]).all()                         # max >= mean, channel by channel
    # without the key nothing is written (the default)
    assert train_ae.plan({})["latent_moments"] is False
