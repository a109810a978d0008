"""Drop-in for the reference's ``save_latent.py`` (`extract_latents`, `:13-204`): frozen-encoder latents of every
image -> pooled / raw / patch-level DataFrames with the reference's columns.

What changes:
  * the encoder.  The reference runs an un-vendored ConvMAE conv-ViT (`save_latent.py:17-18,42-60`) whose code and
    weights are not in the tree.  ``encoder: convmae_base`` selects this build's restatement of it
    (``isic_hip.convmae.ConvMAEBaseEncoder``, 196 x 768 tokens; a checkpoint of the reference's ``train_ae.py`` loads into
    it; ``encoder_precision: mxfp8`` runs its products on the block-scaled FP8 MFMA, on a GPU device only -- as for
    ``encoder: vit_s16``, the one other encoder that takes it).  The default frozen encoder is the ResNet-18 of this
    build truncated after layer3 (``ResNet18Encoder.run_tokens``): 14 x 14 = 196 tokens of 256 channels for a 224 x 224 image, one per 16 x 16-pixel
    patch -- the reference's token geometry (`:77`).  There is no random masking, so ``ids_keep = ids_restore =
    arange(196)`` (the reference passes ``mask_ratio=0``: every patch is kept, in shuffled order);
  * batched inference in HBM, the lesion-mask -> patch-flag step (`:73-87`) as one HIP launch
    (``isic_mask_patch_flags_f32``), and the per-patch Python double loop of ``build_patch_level_df`` (`:109-154`)
    replaced by array operations that produce the same rows in the same order.

  * ``device_resize: true`` (opt-in) moves the resize off the CPU: the loader hands over the decoded uint8 arrays
    (``isic_hip.augment.uint8_transform``), each batch is uploaded as a small ``ImagePool``, and ``isic_augment_u8`` with
    identity parameters produces the normalised 224 x 224 images and the nearest-neighbour masks the patch flags are
    computed from.  ``datasets`` must then yield uint8 arrays (``isic_hip.augment.SyntheticDermPixels``).

  * ``device_pca: true`` (opt-in, read only with ``pca: true``) fits and applies the PCA of `:163-185` on the device
    (``isic_hip.pca.DevicePCA``): the per-batch latents stay resident until the fit is done, every train batch goes through
    ``partial_fit`` (with ``remove_background`` through the row index of its lesion-flagged patches: the Gram kernel reads
    through the index; the first batch is gathered once to form the shift, and ``transform`` gathers where the row-indexed
    GEMM does not serve the shape), and
    ``patch_latent_pca`` is filled from the transformed batches in the frames' row order.  Without the key ``pca: true``
    is the reference's sklearn call, unchanged.

  * ``device_moments: true`` (opt-in) takes ``latent_pooled_max`` and ``latent_pooled_mean`` (`:62-63`) from one
    ``isic_token_moments_f32`` launch per batch (``isic_hip.moments.token_moments``: slices 1 and 0 of its output) instead
    of two torch reductions.  The max is the same element; the mean may differ from torch's in the last bits (another
    summation order), hence opt-in.

  * ``lesion_moments: true`` (opt-in) adds two columns to the pooled frames: ``latent_lesion_moments``, the ``[6 D]`` fp32
    descriptor of ``utils.concat_patch_moments`` over the image's lesion patches only, and ``lesion_patch_count``.  Both come
    from one ``isic_token_moments_masked_f32`` launch per batch (``token_moments(latent, keep=flags)``) on the flags
    ``mask_patch_flags`` already makes; an image without a lesion patch carries a NaN row and count 0.  Without the key the
    frames are unchanged, column for column.

``extract_latents(config, path, remove_background=False, datasets=None)`` keeps the reference's signature and return
tuple; ``datasets=(train_val_dataset, test_dataset)`` lets a caller hand in any dataset with the ``DermDataset`` dict
contract (`dataset.py:45-56`) -- the synthetic one below when there are no image files.
"""
from __future__ import annotations

import os

import numpy as np
import pandas as pd
import torch
from torch.utils.data import DataLoader, Dataset

from isic_hip.encoder import ResNet18Encoder
from isic_hip.lib import call

PATCH = 16                      # save_latent.py:77
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)       # save_latent.py:28


class SyntheticDermImages(Dataset):
    """ISIC-shaped stand-in with the ``DermDataset`` dict contract: a normalised 3x224x224 image, an elliptic lesion
    mask (some images without a mask), a class label; deterministic per index."""

    def __init__(self, n=32, size=224, classes=7, seed=42):
        self.n, self.size, self.classes, self.seed = n, size, classes, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 7919 + i)
        y = i % self.classes
        s = self.size
        img = torch.randn(3, s, s, generator=g) + 0.25 * (y - (self.classes - 1) / 2)
        yy, xx = torch.meshgrid(torch.arange(s), torch.arange(s), indexing="ij")
        cy, cx = (torch.rand(2, generator=g) * 0.5 + 0.25) * s
        ry, rx = (torch.rand(2, generator=g) * 0.25 + 0.08) * s
        mask = ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0).float()
        if i % 5 == 4:
            mask = torch.zeros_like(mask)                       # the 'no_mask' case of dataset.py
        return {"image": img, "mask": mask.unsqueeze(0), "radiomics": torch.zeros(102), "age": torch.tensor(0.0),
                "sex": torch.tensor(0), "loc": torch.tensor(0), "artifacts": torch.zeros(6, dtype=torch.long),
                "target": torch.tensor(y, dtype=torch.long), "image_path": f"synthetic/img_{i:05d}.jpg",
                "segmentation_path": "no_mask" if i % 5 == 4 else f"synthetic/seg_{i:05d}.png"}


def mask_patch_flags(mask, patch=PATCH):
    """`save_latent.py:73-87` on the device: mask (B,H,W) or (B,1,H,W) -> bool [B, H/patch, W/patch]."""
    if mask.dim() == 4:
        mask = mask[:, 0]
    m = mask.contiguous().float()
    B, H, W = m.shape
    flags = torch.empty((B, H // patch, W // patch), device=m.device, dtype=torch.uint8)
    call("isic_mask_patch_flags_f32", m, flags, B, H, W, patch)
    return flags.bool()


def build_patch_level_df(latent_raw_df, remove=True):
    """`save_latent.py:109-158`: one row per kept patch -- image_path, segmentation_path, target, patch_id,
    patch_latent, patch_in_mask -- in image-major, token order; with ``remove`` only lesion-overlapping patches.
    Returns (frame, number of rows written while ``remove`` was on) exactly like the reference's counter."""
    cols = ["image_path", "segmentation_path", "target", "patch_id", "patch_latent", "patch_in_mask"]
    if len(latent_raw_df) == 0:
        return pd.DataFrame(columns=cols), 0
    lat = np.stack(latent_raw_df["latent"].values)                          # [B, T, D]
    ids = np.stack(latent_raw_df["ids_keep"].values).astype(np.int64)       # [B, T]
    flat = np.stack([np.asarray(m).ravel() for m in latent_raw_df["lesion_mask_patches"].values]).astype(bool)
    B, T, _ = lat.shape
    inside = np.take_along_axis(flat, np.minimum(ids, flat.shape[1] - 1), axis=1) & (ids < flat.shape[1])
    keep = inside if remove else np.ones_like(inside)
    b_idx, t_idx = np.nonzero(keep)
    df = pd.DataFrame({
        "image_path": latent_raw_df["image_path"].values[b_idx],
        "segmentation_path": latent_raw_df["segmentation_path"].values[b_idx],
        "target": latent_raw_df["target"].values[b_idx],
        "patch_id": ids[b_idx, t_idx],
        "patch_latent": list(lat[b_idx, t_idx]),
        "patch_in_mask": inside[b_idx, t_idx].astype(np.int64),
    }, columns=cols)
    return df, (int(keep.sum()) if remove else 0)


def _device_resized(loader, device):
    """Batches of a loader that hands over lists of uint8 items -> the dict batches of the default path, image and mask made
    on the device by one ``isic_augment_u8`` launch with identity parameters."""
    from isic_hip import augment as ag
    for items in loader:
        pool = ag.ImagePool.from_arrays([(it["image"], it["mask"]) for it in items], device)
        box, op = ag.identity_params(pool.hw_host)
        images, masks = ag.augment(pool, torch.arange(len(pool)), box, op, size=224, mean=MEAN, std=STD)
        yield {"image": images, "mask": masks, "target": torch.stack([torch.as_tensor(it["target"]) for it in items]),
               "image_path": [it["image_path"] for it in items],
               "segmentation_path": [it["segmentation_path"] for it in items]}


def _extract_from_loader(encoder, loader, device, resident=None, device_moments=False, lesion_moments=False):
    """``resident``: a list that receives (latent [B, T, D], flags [B, T] bool) of every batch, left on the device;
    ``device_moments``: the pooled max and mean come from one ``token_moments`` launch; ``lesion_moments``: the pooled frame
    gains the descriptor of the lesion patches and their number, from one masked launch"""
    pooled_list, raw_list = [], []
    for batch in loader:
        images = batch["image"].to(device)
        latent = encoder.run_tokens(images)                                 # [B, 196, 256] fp32, frozen / eval
        B, T, D = latent.shape
        if device_moments:
            from isic_hip.moments import token_moments
            stats = token_moments(latent)                                   # [B, 6 D]: mean, max, ...
            pooled_mean, pooled_max = stats[:, :D], stats[:, D:2 * D]
        else:
            pooled_max, pooled_mean = latent.max(dim=1).values, latent.mean(dim=1)
        ids = np.tile(np.arange(T, dtype=np.int64), (B, 1))
        target = batch["target"].numpy()
        pooled_list.append(pd.DataFrame({
            "image_path": batch["image_path"], "segmentation_path": batch["segmentation_path"], "target": target,
            "latent_pooled_max": list(pooled_max.cpu().numpy()),                        # :62
            "latent_pooled_mean": list(pooled_mean.cpu().numpy()),                      # :63
            "ids_restore": list(ids), "ids_keep": list(ids)}))
        flags = mask_patch_flags(batch["mask"].to(device))
        if lesion_moments:
            from isic_hip.moments import token_moments
            lesion, count = token_moments(latent, keep=flags.reshape(B, -1), return_counts=True)
            pooled_list[-1]["latent_lesion_moments"] = list(lesion.cpu().numpy())
            pooled_list[-1]["lesion_patch_count"] = count.cpu().numpy().astype(np.int64)
        if resident is not None:
            resident.append((latent, flags.reshape(B, -1)))
        raw_list.append(pd.DataFrame({
            "image_path": batch["image_path"], "segmentation_path": batch["segmentation_path"], "target": target,
            "latent": list(latent.cpu().numpy()), "ids_restore": list(ids), "ids_keep": list(ids),
            "lesion_mask_patches": list(flags.cpu().numpy())}))
    cat = lambda l: pd.concat(l, ignore_index=True) if l else pd.DataFrame()
    return cat(pooled_list), cat(raw_list)


def _device_pca_columns(resident_train, resident_test, remove, n_train, n_test):
    """`save_latent.py:163-185` on the device -> the ``patch_latent_pca`` columns of the train and test patch frames (lists
    of fp32 rows in the row order of ``build_patch_level_df``: image-major, then token order)."""
    from isic_hip.pca import DevicePCA

    def batches(resident):
        for latent, flags in resident:
            x = latent.reshape(-1, latent.shape[-1])
            rows = torch.nonzero(flags.reshape(-1)).reshape(-1).to(torch.int32) if remove else None
            yield x, rows

    pca = DevicePCA(n_components=0.90)
    for x, rows in batches(resident_train):
        pca.partial_fit(x, rows)
    if pca.n_samples_seen_ != n_train:
        raise RuntimeError(f"device_pca: fitted {pca.n_samples_seen_} rows, the train frame has {n_train}")
    if n_train == 0:
        if n_test > 0:
            raise RuntimeError("No train patches to fit PCA. Cannot transform test patches.")
        return [], []
    pca.finalize()
    width = resident_train[0][0].shape[-1]
    print(f"PCA reduced dimensions from {width} to {pca.n_components_}")
    cols = []
    for resident, n in ((resident_train, n_train), (resident_test, n_test)):
        out = [pca.transform(x, rows).cpu().numpy() for x, rows in batches(resident)]
        out = np.concatenate(out) if out else np.zeros((0, pca.n_components_), dtype=np.float32)
        if len(out) != n:
            raise RuntimeError(f"device_pca: transformed {len(out)} rows, the patch frame has {n}")
        cols.append(list(out))
    return cols


def extract_latents(config, path, remove_background=False, datasets=None, batch_size=256):
    device = torch.device(config.get("device", "cuda:0"))
    seed = config.get("seed", 42)
    np.random.seed(seed)
    torch.manual_seed(seed)
    device_resize = bool(config.get("device_resize", False))
    if datasets is None:
        from dataset import DermDataset
        df_tv, df_te = pd.read_pickle(config["dir"]["df"]), pd.read_pickle(config["dir"]["df_test"])

        def transform(image, mask):                                          # A.Resize(224,224) + A.Normalize (:26-30)
            img = torch.from_numpy(np.ascontiguousarray(image)).permute(2, 0, 1).float().unsqueeze(0) / 255.0
            img = torch.nn.functional.interpolate(img, size=(224, 224), mode="bilinear", align_corners=False)[0]
            img = (img - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
            m = torch.from_numpy(np.ascontiguousarray(mask)).float()[None, None]
            m = torch.nn.functional.interpolate(m, size=(224, 224), mode="nearest")[0, 0]
            return {"image": img, "mask": m}
        if device_resize:
            from isic_hip.augment import uint8_transform as transform
        datasets = (DermDataset(df_tv, radiomics=None, transform=transform), DermDataset(df_te, radiomics=None, transform=transform))
    if device_resize:
        loaders = [_device_resized(DataLoader(d, batch_size=batch_size, shuffle=False, collate_fn=list), device)
                   for d in datasets]
    else:
        loaders = [DataLoader(d, batch_size=batch_size, shuffle=False) for d in datasets]
    precision = str(config.get("encoder_precision", "fp16")).lower()
    if precision not in ("fp16", "mxfp8"):
        raise ValueError(f"encoder_precision: 'fp16' or 'mxfp8', got {precision!r}")
    name = str(config.get("encoder", "resnet18")).lower()
    if name in ("convmae_base", "convmae", "convmae_convvit_base_patch16"):
        if precision == "mxfp8" and device.type != "cuda":
            raise ValueError("encoder_precision='mxfp8' with encoder: convmae_base runs on gfx950's block-scaled MFMA: "
                             f"it needs a GPU device, got device: {str(device)!r}")
        from isic_hip.convmae import ConvMAEBaseEncoder          # the reference's encoder: 196 x 768 tokens
        enc = ConvMAEBaseEncoder(precision=precision).to(device)  # "mxfp8": the opt-in MXFP8 products (isic_hip/convmae.py)
    elif name in ("vit_s16", "vit-s/16", "vit_small_patch16_224"):
        from isic_hip.vit import ViTSmallEncoder                # BASELINE.json configs[4]: ViT-S/16, fp16, 196 x 384 tokens
        enc = ViTSmallEncoder(precision=precision).to(device)   # "mxfp8": the opt-in MXFP8 products (isic_hip/vit.py)
    else:
        if precision != "fp16":
            raise ValueError("encoder_precision='mxfp8' needs encoder: vit_s16 (the ResNet-18 encoder is bf16 only)")
        enc = ResNet18Encoder().to(device)
    ckpt = os.path.join(os.getcwd(), config.get("model_path", "models"), path)
    if os.path.exists(ckpt):
        enc.load_state_dict(torch.load(ckpt, map_location=device, weights_only=True), strict=False)          # :46-48
    else:
        print(f"save_latent: checkpoint {ckpt} not found -- encoder keeps its seeded initialisation")
    enc.eval()
    device_pca = bool(config.get("pca", False)) and bool(config.get("device_pca", False))
    resident_train, resident_test = ([], []) if device_pca else (None, None)
    device_moments = bool(config.get("device_moments", False))
    lesion_moments = bool(config.get("lesion_moments", False))
    latent_pooled_train, latent_raw_train = _extract_from_loader(enc, loaders[0], device, resident_train, device_moments,
                                                                 lesion_moments)
    latent_pooled_test, latent_raw_test = _extract_from_loader(enc, loaders[1], device, resident_test, device_moments,
                                                               lesion_moments)
    patch_level_train_df, train_count = build_patch_level_df(latent_raw_train, remove=remove_background)
    patch_level_test_df, test_count = build_patch_level_df(latent_raw_test, remove=remove_background)
    print(f"Total lesion-overlapping patches (train_val): {train_count}")
    print(f"Total lesion-overlapping patches (test): {test_count}")
    if device_pca:                                                           # :163-185 on the device
        tr, te = _device_pca_columns(resident_train, resident_test, remove_background, len(patch_level_train_df),
                                     len(patch_level_test_df))
        patch_level_train_df["patch_latent_pca"], patch_level_test_df["patch_latent_pca"] = tr, te
    elif bool(config.get("pca", False)):                                     # :163-180
        from sklearn.decomposition import PCA
        if len(patch_level_train_df) > 0:
            Xtr = np.vstack(patch_level_train_df["patch_latent"].values)
            pca = PCA(n_components=0.90, whiten=False)
            Xp = pca.fit_transform(Xtr)
            print(f"PCA reduced dimensions from {Xtr.shape[1]} to {Xp.shape[1]}")
            patch_level_train_df["patch_latent_pca"] = list(Xp)
        else:
            patch_level_train_df["patch_latent_pca"] = []
        if len(patch_level_test_df) > 0:
            if len(patch_level_train_df) == 0:
                raise RuntimeError("No train patches to fit PCA. Cannot transform test patches.")
            patch_level_test_df["patch_latent_pca"] = list(pca.transform(np.vstack(patch_level_test_df["patch_latent"].values)))
        else:
            patch_level_test_df["patch_latent_pca"] = []
    else:
        print("PCA disabled via config; using raw patch_latent as patch_latent_pca.")
        patch_level_train_df["patch_latent_pca"] = patch_level_train_df["patch_latent"]
        patch_level_test_df["patch_latent_pca"] = patch_level_test_df["patch_latent"]
    os.makedirs("dataframes_latents", exist_ok=True)                         # :188-190 (save_files = False)
    print("Finished saving train_val and test patch-level and pooled latents.")
    return (patch_level_train_df, patch_level_test_df, latent_pooled_train, latent_pooled_test, latent_raw_train,
            latent_raw_test)
