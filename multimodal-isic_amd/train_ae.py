"""Fine-tune the ConvMAE-Base masked autoencoder (the reference's ``train_ae.py``) on the native path.

The loop of the reference: one fold of a 10-fold ``StratifiedKFold`` (``training_plan.parameters.fold``) over the
train/val images, class-balanced sampling (``WeightedRandomSampler`` with weights 1 / class count, with replacement),
AdamW with the encoder at lr 1e-5 and the decoder (every parameter whose name holds "decoder") at lr 1e-3, betas
(0.9, 0.95), weight decay 0.05 -- two ``isic_hip.optim.AdamW`` instances, one per group.  Each epoch reports the train
loss (averaged per image) and the validation loss at ``eval_masking_ratio``; the state with the best validation loss is
saved as ``models/<uuid>.pth`` under the working directory (or ``--out-dir``), the file ``save_latent.extract_latents``
loads through ``model_path``.

Config keys (``training_plan.parameters``; the committed config.yml has none of them, so these defaults apply):
``masking_ratio`` 0.75, ``eval_masking_ratio`` 0.75, ``norm_pix_loss`` False, ``batch_size`` 64, ``epochs`` 100,
``fold`` 0, ``include_lesion_mask`` False (True raises: ``ConvMAEBase`` does not define ``lesion_mask``),
``device_augment`` False, ``latent_moments`` False.  ``--synthetic`` trains on ``save_latent.SyntheticDermImages`` (no
dataset needed).

``latent_moments: true`` (``--latent-moments``) is the reference's latent-space probe (``train_ae.py:186-194``) without its
plot: in every epoch with ``epoch % 10 == 0 or epoch == epochs - 1`` each validation batch also runs
``forward_encoder(images, 0.0)`` and ``utils.concat_patch_moments`` (one HIP launch, ``isic_token_moments_f32``), and the
validation set's descriptors are written to ``<out_dir>/latent_moments/epoch_<eeee>.npz`` as ``feats`` (fp32
``[N_val, 6 * 768]``) and ``target`` (int64).

Augmentation.  The reference trains under ``RandomResizedCrop(224, scale=(0.5, 1.0), ratio=(0.75, 1.33))``, horizontal and
vertical flips and ``RandomRotate90`` (each with probability 0.5), then ``Normalize`` (``train_ae.py:88-100``), and
validates under ``Resize(224)``, ``Normalize`` (``:102-105``).  The default path here does NOT augment: it trains on the
validation transform (decode, square crop, bilinear resize to 224 and normalise on the CPU, per image and per epoch), so
every epoch sees the same pixels.  ``device_augment: true`` (``--device-augment``) is the reference's training
distribution: the decoded uint8 images are uploaded once (``isic_hip.augment.ImagePool``), each step draws its images
from the same class-balanced sampler and its crop / flip / rotation parameters from a generator seeded with ``seed``
(``sample_params``), and one HIP launch (``isic_augment_u8``) produces the batch; validation batches come from the same
launch with identity parameters.  The crop boxes follow RandomResizedCrop's algorithm, but albumentations' random
stream cannot be reproduced, and its fixed-point uint8 resize is not pinned (include/isic_hip_augment.h).  With
``--synthetic`` it trains on ``isic_hip.augment.SyntheticDermPixels``.

Not ported: Neptune logging, the latent-space and reconstruction plots (PCA + UMAP of the descriptors included), the
ISIC2019 CSV merge; the colour augmentations the reference has commented out.
"""
from __future__ import annotations

import argparse
import copy
import os
import sys
import uuid

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset, WeightedRandomSampler

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from isic_hip import optim  # noqa: E402
from isic_hip.convmae_mae import convmae_convvit_base_patch16_dec512d8b  # noqa: E402
from utils import concat_patch_moments  # noqa: E402

SPLITS = 10
DEFAULTS = dict(masking_ratio=0.75, eval_masking_ratio=0.75, norm_pix_loss=False, batch_size=64, epochs=100, fold=0,
                include_lesion_mask=False, device_augment=False, latent_moments=False)


def plan(config):
    p = dict(DEFAULTS)
    p.update({k: v for k, v in ((config.get("training_plan") or {}).get("parameters") or {}).items() if k in DEFAULTS})
    return p


def split(labels, fold, seed):
    from sklearn.model_selection import StratifiedKFold
    kf = StratifiedKFold(n_splits=SPLITS, shuffle=True, random_state=seed)
    folds = list(kf.split(np.zeros(len(labels)), labels))
    return folds[fold]


def balanced_sampler(labels):
    labels = np.asarray(labels)
    counts = {c: int((labels == c).sum()) for c in np.unique(labels)}
    w = torch.as_tensor([1.0 / counts[c] for c in labels], dtype=torch.double)
    return WeightedRandomSampler(weights=w, num_samples=len(w), replacement=True)


def optimizers(model):
    enc = [p for k, p in model.named_parameters() if "decoder" not in k and p.requires_grad]
    dec = [p for k, p in model.named_parameters() if "decoder" in k and p.requires_grad]
    kw = dict(betas=(0.9, 0.95), weight_decay=0.05)
    return [optim.AdamW(enc, lr=1e-5, **kw), optim.AdamW(dec, lr=1e-3, **kw)]


def _chunks(ids, size):
    return [ids[i:i + size] for i in range(0, len(ids), size)]


def device_batches(pool, ids, batch_size, generator=None):
    """Batches of ``pool`` images ``ids`` through ``isic_augment_u8``: augmented with parameters drawn from ``generator``, or
    (``generator=None``) the plain resize to 224 x 224."""
    from isic_hip import augment as ag
    for chunk in _chunks(list(ids), batch_size):
        hw = pool.hw_host[chunk]
        box, op = ag.sample_params(hw, generator) if generator is not None else ag.identity_params(hw)
        yield ag.augment(pool, chunk, box, op, want_mask=False)[0]


def _label_ids(labels):
    """the labels as int64 class indices: integers as they are, anything else (the dx strings of the dataframe) by its
    rank among the sorted distinct values"""
    arr = np.asarray(labels)
    if np.issubdtype(arr.dtype, np.integer):
        return arr.astype(np.int64)
    return np.unique(arr, return_inverse=True)[1].astype(np.int64)


def train(config, dataset, labels, out_dir, checkpoint=None, log=print, device_augment=False):
    """-> (path of the saved best state, [(train_loss, val_loss) per epoch]).  With ``device_augment`` (or the config key
    of that name) ``dataset`` yields uint8 arrays (``isic_hip.augment.uint8_transform`` / ``SyntheticDermPixels``)."""
    p = plan(config)
    device_augment = bool(device_augment or p["device_augment"])
    if p["include_lesion_mask"]:
        raise ValueError("include_lesion_mask: the lesion_mask argument of the reference's MAE fork is undefined here")
    seed = int(config.get("seed", 42))
    device = torch.device(config.get("device", "cuda:0"))
    np.random.seed(seed)
    torch.manual_seed(seed)
    tr, va = split(labels, int(p["fold"]), seed)
    if device_augment:
        from isic_hip.augment import ImagePool
        pool = ImagePool.from_dataset(dataset, device)                      # decoded once; every batch is one launch
        sampler = balanced_sampler(np.asarray(labels)[tr])
        params = torch.Generator().manual_seed(seed)
        n_train, n_val = len(tr), len(va)
        train_batches = lambda: device_batches(pool, [int(tr[i]) for i in sampler], int(p["batch_size"]), params)
        val_targets = torch.from_numpy(_label_ids(labels)[va])                 # the pool's batches carry no labels
        val_batches = lambda: zip(device_batches(pool, va.tolist(), 64), val_targets.split(64))
    else:
        train_loader = DataLoader(Subset(dataset, tr.tolist()), batch_size=int(p["batch_size"]),
                                  sampler=balanced_sampler(np.asarray(labels)[tr]))
        val_loader = DataLoader(Subset(dataset, va.tolist()), batch_size=64, shuffle=False)
        n_train, n_val = len(train_loader.dataset), len(val_loader.dataset)
        train_batches = lambda: (batch["image"].to(device) for batch in train_loader)
        val_batches = lambda: ((batch["image"].to(device), batch["target"]) for batch in val_loader)
    model = convmae_convvit_base_patch16_dec512d8b(norm_pix_loss=bool(p["norm_pix_loss"])).to(device)
    if checkpoint:
        sd = torch.load(checkpoint, map_location=device, weights_only=False)
        model.load_state_dict(sd.get("model", sd), strict=False)
    opts = optimizers(model)
    best, best_state, history = float("inf"), None, []
    for epoch in range(int(p["epochs"])):
        model.train()
        run = 0.0
        for images in train_batches():
            for o in opts:
                o.zero_grad()
            loss, _, _ = model(images, mask_ratio=float(p["masking_ratio"]))
            loss.backward()
            for o in opts:
                o.step()
            run += float(loss) * images.shape[0]
        train_loss = run / n_train
        model.eval()
        run = 0.0
        probe = bool(p["latent_moments"]) and (epoch % 10 == 0 or epoch == int(p["epochs"]) - 1)
        feats, targets = [], []
        with torch.no_grad():
            for images, target in val_batches():
                loss, _, _ = model(images, mask_ratio=float(p["eval_masking_ratio"]))
                run += float(loss) * images.shape[0]
                if probe:                                                     # train_ae.py:186-191
                    latent, _, _ = model.forward_encoder(images, 0.0)
                    feats.append(concat_patch_moments(latent).cpu())
                    targets.append(torch.as_tensor(target).reshape(-1).long().cpu())
        val_loss = run / n_val
        if probe:
            moments_dir = os.path.join(out_dir, "latent_moments")
            os.makedirs(moments_dir, exist_ok=True)
            np.savez(os.path.join(moments_dir, f"epoch_{epoch:04d}.npz"), feats=torch.cat(feats).numpy(),
                     target=torch.cat(targets).numpy())
        history.append((train_loss, val_loss))
        log(f"Epoch [{epoch + 1}/{p['epochs']}], Train Loss: {train_loss:.4f}, Val Loss: {val_loss:.4f}")
        if val_loss < best:
            best = val_loss
            best_state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model_dir = os.path.join(out_dir, "models")
    os.makedirs(model_dir, exist_ok=True)
    path = os.path.join(model_dir, f"{uuid.uuid4().hex}.pth")
    torch.save(best_state if best_state is not None else copy.deepcopy(model.state_dict()), path)
    log(f"Saved Best Model at {path}")
    return path, history


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default=os.path.join(HERE, "config.yml"))
    ap.add_argument("--synthetic", action="store_true", help="train on save_latent.SyntheticDermImages")
    ap.add_argument("--device-augment", action="store_true",
                    help="the reference's training augmentation, on the device from a resident uint8 pool")
    ap.add_argument("--latent-moments", action="store_true",
                    help="every tenth epoch write the validation set's concat_patch_moments descriptors to <out-dir>/latent_moments")
    ap.add_argument("--n-images", type=int, default=256, help="synthetic images")
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--checkpoint", default="", help="a MAE checkpoint to start from (loaded with strict=False)")
    ap.add_argument("--out-dir", default=os.getcwd())
    a = ap.parse_args(argv)
    import yaml
    with open(a.config) as f:
        config = yaml.safe_load(f) or {}
    params = config.setdefault("training_plan", {}).setdefault("parameters", {})
    if a.epochs is not None:
        params["epochs"] = a.epochs
    if a.batch_size is not None:
        params["batch_size"] = a.batch_size
    if a.device_augment:
        params["device_augment"] = True
    if a.latent_moments:
        params["latent_moments"] = True
    device_augment = bool(params.get("device_augment", False))
    if a.synthetic:
        from isic_hip.augment import SyntheticDermPixels
        from save_latent import SyntheticDermImages
        ds = (SyntheticDermPixels if device_augment else SyntheticDermImages)(n=a.n_images)
        labels = [i % ds.classes for i in range(len(ds))]
    else:
        import pandas as pd
        from dataset import DermDataset
        from save_latent import MEAN, STD
        df = pd.read_pickle(config["dir"]["df"])

        def transform(image, mask):
            img = torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1).float().unsqueeze(0) / 255.0
            img = torch.nn.functional.interpolate(img, size=(224, 224), mode="bilinear", align_corners=False)[0]
            img = (img - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
            return {"image": img, "mask": torch.from_numpy(np.ascontiguousarray(mask)).float()}

        if device_augment:
            from isic_hip.augment import uint8_transform as transform
        ds = DermDataset(df, radiomics=None, transform=transform)
        labels = list(df["dx"])
    train(config, ds, labels, a.out_dir, checkpoint=a.checkpoint or None)


if __name__ == "__main__":
    main()
