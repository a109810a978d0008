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
``fold`` 0, ``include_lesion_mask`` False (True raises: ``ConvMAEBase`` does not define ``lesion_mask``).
``--synthetic`` trains on ``save_latent.SyntheticDermImages`` (no dataset needed).  Not ported: Neptune logging, the
latent-space and reconstruction plots, the ISIC2019 CSV merge and ``concat_patch_moments``.
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

SPLITS = 10
DEFAULTS = dict(masking_ratio=0.75, eval_masking_ratio=0.75, norm_pix_loss=False, batch_size=64, epochs=100, fold=0,
                include_lesion_mask=False)


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


def train(config, dataset, labels, out_dir, checkpoint=None, log=print):
    """-> (path of the saved best state, [(train_loss, val_loss) per epoch])."""
    p = plan(config)
    if p["include_lesion_mask"]:
        raise ValueError("include_lesion_mask: the lesion_mask argument of the reference's MAE fork is undefined here")
    seed = int(config.get("seed", 42))
    device = torch.device(config.get("device", "cuda:0"))
    np.random.seed(seed)
    torch.manual_seed(seed)
    tr, va = split(labels, int(p["fold"]), seed)
    train_loader = DataLoader(Subset(dataset, tr.tolist()), batch_size=int(p["batch_size"]),
                              sampler=balanced_sampler(np.asarray(labels)[tr]))
    val_loader = DataLoader(Subset(dataset, va.tolist()), batch_size=64, shuffle=False)
    model = convmae_convvit_base_patch16_dec512d8b(norm_pix_loss=bool(p["norm_pix_loss"])).to(device)
    if checkpoint:
        sd = torch.load(checkpoint, map_location=device, weights_only=False)
        model.load_state_dict(sd.get("model", sd), strict=False)
    opts = optimizers(model)
    best, best_state, history = float("inf"), None, []
    for epoch in range(int(p["epochs"])):
        model.train()
        run = 0.0
        for batch in train_loader:
            for o in opts:
                o.zero_grad()
            images = batch["image"].to(device)
            loss, _, _ = model(images, mask_ratio=float(p["masking_ratio"]))
            loss.backward()
            for o in opts:
                o.step()
            run += float(loss) * images.shape[0]
        train_loss = run / len(train_loader.dataset)
        model.eval()
        run = 0.0
        with torch.no_grad():
            for batch in val_loader:
                images = batch["image"].to(device)
                loss, _, _ = model(images, mask_ratio=float(p["eval_masking_ratio"]))
                run += float(loss) * images.shape[0]
        val_loss = run / len(val_loader.dataset)
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
    if a.synthetic:
        from save_latent import SyntheticDermImages
        ds = SyntheticDermImages(n=a.n_images)
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

        ds = DermDataset(df, radiomics=None, transform=transform)
        labels = list(df["dx"])
    train(config, ds, labels, a.out_dir, checkpoint=a.checkpoint or None)


if __name__ == "__main__":
    main()
