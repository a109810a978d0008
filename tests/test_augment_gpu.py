"""The device augmentation path on the MI355X: ``isic_augment_u8`` (include/isic_hip_augment.h) against the float64
restatement tests/augment_ref.py, its flips and rotations against torch's, a pool above 2^31 bytes, and the two callers
(``train_ae.py --device-augment``, ``save_latent.extract_latents`` with ``device_resize``).

Tolerances: the image is held to 1e-5 absolute in normalised units -- the fp32 evaluation of the exact-coordinate formulas
stays within 9.6e-7 of float64 (measured on the CPU), and the tolerance is ten times that; the mask, an integer gather, is
exact.  Every element of every output is compared."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = ((1, 1), (7, 5), (600, 450), (450, 600), (37, 53), (224, 224), (300, 200))
TOL = 1e-5


def _items(seed=0):
    """Ragged images with masks of arbitrary byte values (so a wrong tap shows); the 37 x 53 image has no mask."""
    rng = np.random.RandomState(seed)
    return [(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8),
             None if (h, w) == (37, 53) else rng.randint(0, 256, size=(h, w)).astype(np.uint8)) for h, w in SIZES]


def _boxes(h, w):
    """Full, interior, and one touching each edge (where the image is large enough to leave the other edges)."""
    out = [(0, 0, h, w)]
    if h >= 5 and w >= 5:
        ch, cw = max(h // 2, 1), max((2 * w) // 3, 1)
        out += [(1, 1, h - 2, w - 2), (0, 1, ch, cw), (h - ch, 1, ch, cw - 1), (1, 0, ch - 1, cw), (2, w - cw, ch, cw),
                (h - 1, w - 1, 1, 1), (h // 3, w // 4, 1, cw), (h // 3, w // 4, ch, 1)]
    return out


def _cases():
    index, box, op = [], [], []
    code = 0
    for n, (h, w) in enumerate(SIZES):
        for bx in _boxes(h, w):
            for _ in range(2 if len(_boxes(h, w)) > 1 else 16):       # repeated indices; 1 x 1 alone sees all 16 codes
                index.append(n), box.append(bx), op.append(code % 16)
                code += 1
    for c in range(16):                                               # every code on one interior box of the largest
        index.append(2), box.append((13, 7, 431, 402)), op.append(c)
    return index, box, op


def _reference(items, index, box, op, S):
    import augment_ref as ar
    from isic_hip import augment as ag
    masks = [m if m is not None else np.zeros(a.shape[:2], np.uint8) for a, m in items]
    return ar.augment([a for a, _ in items], masks, index, box, op, S, ag.MEAN, ag.STD)


@pytest.mark.parametrize("S", [224, 30, 1, 517])
def test_kernel_matches_the_restatement(S):
    """S = 224 is the product's; 30 and 517 are not multiples of 4 (scalar stores, partial tiles), 1 is the smallest."""
    from isic_hip import augment as ag
    items = _items()
    pool = ag.ImagePool.from_arrays(items, DEV)
    index, box, op = _cases()
    assert len(set(op)) == 16 and len(set(index)) == len(SIZES) >= 6 and len(index) > len(set(zip(index, box)))
    if S == 517:
        index, box, op = index[-40:], box[-40:], op[-40:]
    images, masks = ag.augment(pool, index, box, op, size=S)
    torch.cuda.synchronize()
    want, mwant = _reference(items, index, box, op, S)
    assert images.shape == want.shape and masks.shape == mwant.shape and images.dtype == torch.float32
    err = np.abs(images.double().cpu().numpy() - want)
    print(f"S={S}: {len(index)} outputs, max |kernel - float64| = {err.max():.3e} (tolerance {TOL:.0e})")
    assert np.isfinite(err).all() and float(err.max()) <= TOL
    assert np.array_equal(masks.double().cpu().numpy(), mwant)
    only, none = ag.augment(pool, index, box, op, size=S, want_mask=False)
    assert none is None and torch.equal(only, images)


def test_flips_and_rotations_are_exact_permutations():
    """For a fixed box the output under ``op`` is torch.rot90(vflip(hflip(.))) of the ``op = 0`` output, bit for bit.

    The sixteen codes name the eight symmetries of the square twice over: both flips together are a half turn, so code
    ``c`` and code ``c ^ 0b1011`` (both flips toggled, k + 2) are one map.  On random pixels the eight are all different."""
    from isic_hip import augment as ag
    pool = ag.ImagePool.from_arrays(_items(1), DEV)
    for n, bx in ((2, (13, 7, 431, 402)), (1, (0, 0, 7, 5)), (3, (0, 0, 450, 600))):
        images, masks = ag.augment(pool, [n] * 16, [bx] * 16, list(range(16)))
        for code in range(16):
            for out in (images, masks):
                want = out[0]
                if code & 1:
                    want = torch.flip(want, dims=(2,))
                if code & 2:
                    want = torch.flip(want, dims=(1,))
                want = torch.rot90(want, (code >> 2) & 3, dims=(1, 2))
                assert torch.equal(out[code], want), (n, code)
        for code in range(16):
            assert torch.equal(images[code], images[code ^ 0b1011]), (n, code)
            assert torch.equal(masks[code], masks[code ^ 0b1011]), (n, code)
        assert len({images[c].cpu().numpy().tobytes() for c in range(16)}) == 8          # eight different outputs


def test_pool_above_2_31_bytes_reads_its_last_image():
    """14 600 copies of one 256 x 192 image (2.15 GB of pixels), built by repeating its bytes on the device; the last slot is
    overwritten with a different image, which a 32-bit address could not reach.  Skipped when the device is short of the
    6 GB this takes."""
    from isic_hip import augment as ag
    h, w, n = 256, 192, 14600
    assert 3 * h * w * n > 2 ** 31
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 6 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free: the 2^31-byte pool needs 6")
    rng = np.random.RandomState(5)
    first = (rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8), rng.randint(0, 256, size=(h, w)).astype(np.uint8))
    last = (rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8), rng.randint(0, 256, size=(h, w)).astype(np.uint8))
    try:
        pixels = torch.from_numpy(first[0].reshape(-1)).to(DEV).repeat(n)
        masks = torch.from_numpy(first[1].reshape(-1)).to(DEV).repeat(n)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("out of device memory while building the 2^31-byte pool")
    pixels[-3 * h * w:] = torch.from_numpy(last[0].reshape(-1)).to(DEV)
    masks[-h * w:] = torch.from_numpy(last[1].reshape(-1)).to(DEV)
    pool = ag.ImagePool(pixels, masks, [(h, w)] * n)
    assert pool.pixels.numel() > 2 ** 31 and int(pool.offsets[-1]) * 3 == pool.pixels.numel()
    index, box, op = [n - 1, 0, n - 1, n - 2], [(0, 0, h, w), (0, 0, h, w), (5, 9, 200, 150), (0, 0, h, w)], [0, 0, 7, 0]
    images, mout = ag.augment(pool, index, box, op)
    torch.cuda.synchronize()
    want, mwant = _reference([first, last], [1, 0, 1, 0], box, op, 224)
    assert float(np.abs(images.double().cpu().numpy() - want).max()) <= TOL
    assert np.array_equal(mout.double().cpu().numpy(), mwant)
    assert not torch.equal(images[0], images[1])


def test_same_seed_same_batches_and_epochs_differ():
    from isic_hip import augment as ag
    pool = ag.ImagePool.from_dataset(ag.SyntheticDermPixels(n=12), DEV)
    ids = [3, 3, 7, 0, 11, 5, 5, 9]

    def epochs(seed):
        g = torch.Generator().manual_seed(seed)
        out = []
        for _ in range(2):
            box, op = ag.sample_params(pool.hw_host[ids], g)
            out.append(ag.augment(pool, ids, box, op))
        return out
    a, b = epochs(42), epochs(42)
    for (ia, ma), (ib, mb) in zip(a, b):
        assert torch.equal(ia, ib) and torch.equal(ma, mb)
    assert not torch.equal(a[0][0], a[1][0])                          # consecutive epochs see different pixels
    assert not torch.equal(a[0][0], epochs(43)[0][0])
    assert bool(torch.isfinite(a[0][0]).all()) and set(torch.unique(a[0][1]).tolist()) <= {0.0, 255.0}


def test_train_ae_synthetic_device_augment_end_to_end(tmp_path, capsys, monkeypatch):
    """test_train_ae_synthetic_end_to_end with ``--device-augment``: 2 epochs on 70 synthetic uint8 images, batch 8; the
    saved best state loads strictly into ConvMAEBase and through save_latent.extract_latents into the encoder."""
    from isic_hip.convmae import ConvMAEBaseEncoder
    from isic_hip.convmae_mae import ConvMAEBase
    from save_latent import SyntheticDermImages, extract_latents
    script = os.path.join(ROOT, "multimodal-isic_amd", "train_ae.py")
    r = subprocess.run([sys.executable, script, "--synthetic", "--device-augment", "--epochs", "2", "--batch-size", "8",
                        "--n-images", "70", "--out-dir", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count("Train Loss") == 2 and "Saved Best Model" in r.stdout
    ckpts = [f for f in os.listdir(tmp_path / "models") if f.endswith(".pth")]
    assert len(ckpts) == 1
    sd = torch.load(tmp_path / "models" / ckpts[0], map_location="cpu")
    ConvMAEBase().load_state_dict(sd, strict=True)
    assert not torch.equal(sd["decoder_pred.weight"], ConvMAEBase().state_dict()["decoder_pred.weight"])   # it trained
    res = ConvMAEBaseEncoder().load_state_dict(sd, strict=False)
    assert not res.missing_keys and all(k.startswith("decoder") or k == "mask_token" for k in res.unexpected_keys)
    capsys.readouterr()
    monkeypatch.chdir(tmp_path)                                     # extract_latents writes dataframes_latents/ here
    cfg = {"encoder": "convmae_base", "model_path": str(tmp_path / "models"), "device": DEV, "seed": 1}
    extract_latents(cfg, ckpts[0], datasets=(SyntheticDermImages(n=4), SyntheticDermImages(n=2, seed=5)), batch_size=4)
    assert "not found" not in capsys.readouterr().out


class _CpuTransformed(torch.utils.data.Dataset):
    """The default path's CPU transform (save_latent.extract_latents) over the uint8 items of a SyntheticDermPixels."""

    def __init__(self, pixels):
        self.pixels = pixels

    def __len__(self):
        return len(self.pixels)

    def __getitem__(self, i):
        from save_latent import MEAN, STD
        it = dict(self.pixels[i])
        img = it["image"].permute(2, 0, 1).float().unsqueeze(0) / 255.0
        img = torch.nn.functional.interpolate(img, size=(224, 224), mode="bilinear", align_corners=False)[0]
        it["image"] = (img - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
        m = it["mask"].float()[None, None]
        it["mask"] = torch.nn.functional.interpolate(m, size=(224, 224), mode="nearest")[0, 0]
        return it


def test_extract_latents_device_resize(tmp_path, monkeypatch):
    """``device_resize`` returns the frames of the default path; at 224 x 224 sources (both resizes are the identity) the
    lesion-mask patch flags are equal and the latents agree to the fp32 rounding of the normalisation."""
    from isic_hip.augment import SyntheticDermPixels
    from save_latent import extract_latents
    monkeypatch.chdir(tmp_path)
    px = (SyntheticDermPixels(n=10, size=(224, 224)), SyntheticDermPixels(n=5, size=(224, 224), seed=5))
    cfg = {"device": DEV, "seed": 1}
    dev = extract_latents(dict(cfg, device_resize=True), "none.pth", datasets=px, batch_size=4)
    cpu = extract_latents(cfg, "none.pth", datasets=tuple(_CpuTransformed(p) for p in px), batch_size=4)
    assert len(dev) == len(cpu) == 6
    for d, c in zip(dev, cpu):
        assert list(d.columns) == list(c.columns) and len(d) == len(c) > 0
    for d, c in ((dev[4], cpu[4]), (dev[5], cpu[5])):                 # latent_raw_train / latent_raw_test
        assert list(d["image_path"]) == list(c["image_path"]) and list(d["target"]) == list(c["target"])
        fd, fc = np.stack(list(d["lesion_mask_patches"])), np.stack(list(c["lesion_mask_patches"]))
        assert fd.shape == (len(d), 14, 14) and np.array_equal(fd, fc)
        assert fd[0].any() and not fd[4].any()                        # image 4 has no mask
        ld, lc = np.stack(list(d["latent"])), np.stack(list(c["latent"]))
        assert np.abs(ld - lc).max() <= 0.05 * np.abs(lc).max()
    ragged = (SyntheticDermPixels(n=6), SyntheticDermPixels(n=3, seed=9))
    out = extract_latents(dict(cfg, device_resize=True), "none.pth", datasets=ragged, batch_size=4)
    assert len(out[4]) == 6 and len(out[5]) == 3 and np.stack(list(out[4]["latent"])).shape[1] == 196
