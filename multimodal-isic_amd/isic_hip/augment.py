"""The MAE fine-tune's batch transform on the device: a resident uint8 image pool and one HIP launch per batch.

The reference fine-tunes under ``RandomResizedCrop(224, scale=(0.5, 1.0), ratio=(0.75, 1.33))``, ``HorizontalFlip(0.5)``,
``VerticalFlip(0.5)``, ``RandomRotate90(0.5)``, ``Normalize`` (``train_ae.py:88-100``) and validates under ``Resize(224)``,
``Normalize`` (``:102-105``).  Here the decoded images and their lesion masks are uploaded once as a ragged pool
(``ImagePool``); ``sample_params`` draws the crop boxes and flip / rotation codes on the host from a seeded CPU generator;
``augment`` turns them into a normalised batch with ``isic_augment_u8`` (include/isic_hip_augment.h).  The same launch with
``identity_params`` is the validation / extraction transform.  There is no CPU fallback: ``augment`` needs the library and a
pool on the device.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch.utils.data import Dataset

from .lib import call

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
MAX_SIDE = 1 << 20                  # the kernel clamps crop sides to this (its coordinates are 32-bit)
ATTEMPTS = 10                       # RandomResizedCrop's
_CHUNK = 256 << 20                  # host staging buffer of from_dataset, bytes of pixels


def uint8_transform(image, mask):
    """A ``DermDataset`` transform that keeps the decoded arrays as they are: HWC uint8 image, HW uint8 mask."""
    return {"image": torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint8)),
            "mask": torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8))}


def _as_u8(a, what):
    a = a.numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError(f"{what}: uint8 expected, got {a.dtype}")
    return np.ascontiguousarray(a)


def _item_arrays(image, mask):
    img = _as_u8(image, "image")
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"image: HWC with 3 channels expected, got shape {img.shape}")
    h, w = img.shape[:2]
    if max(h, w) > MAX_SIDE:
        raise ValueError(f"image side {max(h, w)} above {MAX_SIDE}")
    if mask is None:
        m = np.zeros((h, w), np.uint8)
    else:
        m = _as_u8(mask, "mask")
        if m.ndim == 3 and m.shape[0] == 1:
            m = m[0]
        if m.shape != (h, w):
            raise ValueError(f"mask shape {m.shape} does not match its image ({h}, {w})")
    return img, m


class ImagePool:
    """Decoded images of ragged sizes and their lesion masks, resident on ``device``.

    Device: ``pixels`` (uint8, image n is HWC at byte ``3 * offsets[n]``), ``masks`` (uint8, HW at byte ``offsets[n]``; all
    zero for an image without a mask), ``offsets`` (int64 ``[n + 1]``, in pixels), ``hw`` (int32 ``[n, 2]``).  Host:
    ``hw_host`` (int64 ``[n, 2]``), ``labels``, ``image_path``, ``segmentation_path`` (lists; empty strings / -1 where the
    source had none)."""

    def __init__(self, pixels, masks, hw_host, labels=None, image_path=None, segmentation_path=None):
        n = len(hw_host)
        self.hw_host = torch.as_tensor(np.asarray(hw_host, dtype=np.int64).reshape(n, 2))
        off = torch.zeros(n + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(self.hw_host[:, 0] * self.hw_host[:, 1], 0)
        if pixels.numel() != 3 * int(off[-1]) or masks.numel() != int(off[-1]):
            raise ValueError("pixels / masks do not hold the pixels that hw counts")
        self.pixels, self.masks = pixels, masks
        self.device = pixels.device
        self.offsets = off.to(self.device)
        self.hw = self.hw_host.to(torch.int32).to(self.device)
        self.labels = list(labels) if labels is not None else [-1] * n
        self.image_path = list(image_path) if image_path is not None else [""] * n
        self.segmentation_path = list(segmentation_path) if segmentation_path is not None else [""] * n

    def __len__(self):
        return len(self.hw_host)

    @property
    def nbytes(self):
        return self.pixels.numel() + self.masks.numel()

    @classmethod
    def from_arrays(cls, items, device, **meta):
        """``items``: a list of ``(HWC uint8 image, HW uint8 mask or None)``."""
        arrs = [_item_arrays(im, m) for im, m in items]
        hw = [a.shape[:2] for a, _ in arrs]
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        pixels = torch.from_numpy(cat([a.reshape(-1) for a, _ in arrs])).to(device)
        masks = torch.from_numpy(cat([m.reshape(-1) for _, m in arrs])).to(device)
        return cls(pixels, masks, hw, **meta)

    @classmethod
    def from_dataset(cls, dataset, device, max_bytes=None):
        """Decodes every item of ``dataset`` once.  Items follow the ``DermDataset`` dict contract with ``image`` an HWC
        uint8 tensor and ``mask`` HW (or 1HW) uint8 -- ``DermDataset(df, None, transform=uint8_transform)``, or
        ``SyntheticDermPixels``.  Pixels are staged on the host in chunks and uploaded as they fill.  Raises ``ValueError``
        as soon as the pool (3 + 1 bytes per pixel) would exceed ``max_bytes``, with the bytes needed so far."""
        from torch.utils.data import DataLoader
        px_parts, mk_parts, px_host, mk_host, staged = [], [], [], [], 0
        hw, labels, ipath, spath, total = [], [], [], [], 0

        def flush():
            nonlocal staged
            if px_host:
                px_parts.append(torch.from_numpy(np.concatenate(px_host)).to(device))
                mk_parts.append(torch.from_numpy(np.concatenate(mk_host)).to(device))
                px_host.clear(), mk_host.clear()
                staged = 0

        for i, item in enumerate(DataLoader(dataset, batch_size=None, shuffle=False)):
            img, m = _item_arrays(item["image"], item.get("mask"))
            total += 4 * img.shape[0] * img.shape[1]
            if max_bytes is not None and total > max_bytes:
                raise ValueError(f"image pool needs at least {total} bytes after {i + 1} of {len(dataset)} images: "
                                 f"above max_bytes={max_bytes}")
            hw.append(img.shape[:2])
            px_host.append(img.reshape(-1))
            mk_host.append(m.reshape(-1))
            staged += img.size
            labels.append(int(item["target"]) if "target" in item else -1)
            ipath.append(item.get("image_path", ""))
            spath.append(item.get("segmentation_path", ""))
            if staged >= _CHUNK:
                flush()
        flush()
        empty = torch.zeros(0, dtype=torch.uint8, device=device)
        pixels = torch.cat(px_parts) if px_parts else empty
        masks = torch.cat(mk_parts) if mk_parts else empty
        return cls(pixels, masks, hw, labels=labels, image_path=ipath, segmentation_path=spath)


def sample_params(hw, generator, scale=(0.5, 1.0), ratio=(0.75, 1.33), p_hflip=0.5, p_vflip=0.5, p_rot90=0.5):
    """``hw``: ``[B, 2]`` sizes of the chosen images -> ``(box int32 [B, 4] = (y0, x0, ch, cw), op int32 [B])``.

    RandomResizedCrop's algorithm per image: up to 10 attempts of area ``= h w U(scale)``, aspect ``= exp(U(log r0, log
    r1))``, ``cw = round(sqrt(area aspect))``, ``ch = round(sqrt(area / aspect))``; the first attempt with ``1 <= cw <= w``
    and ``1 <= ch <= h`` is taken and its corner drawn uniformly over the positions that keep it inside; if none fits, the
    centred crop with the image's aspect clamped into ``ratio`` (full width or full height).  ``op``: bit 0 the horizontal
    flip (probability ``p_hflip``), bit 1 the vertical flip (``p_vflip``), bits 2-3 ``k`` of ``np.rot90``: with
    probability ``p_rot90`` uniform in {0, 1, 2, 3}, else 0.

    Draw order, all from ``generator`` (a CPU ``torch.Generator``) and of fixed length whatever is accepted, so a batch's
    parameters depend only on the generator's state and ``B``: first ``torch.rand(B, 10, 4, dtype=float64)`` -- per attempt
    the area, the log-aspect, the row corner, the column corner; then ``torch.rand(B, 3, dtype=float64)`` -- hflip, vflip,
    the rotation gate; then ``torch.randint(0, 4, (B,))`` -- ``k``.  Albumentations draws from its own Python / numpy
    streams in its own order: its sequence for a given seed cannot be matched, only its distribution."""
    hw = torch.as_tensor(np.asarray(hw, dtype=np.int64)).reshape(-1, 2)
    B = hw.shape[0]
    u = torch.rand(B, ATTEMPTS, 4, dtype=torch.float64, generator=generator)
    flips = torch.rand(B, 3, dtype=torch.float64, generator=generator)
    k = torch.randint(0, 4, (B,), generator=generator)
    h, w = hw[:, 0:1].double(), hw[:, 1:2].double()
    area = h * w * (scale[0] + (scale[1] - scale[0]) * u[..., 0])
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    aspect = torch.exp(lo + (hi - lo) * u[..., 1])
    cw = torch.round(torch.sqrt(area * aspect)).long()
    ch = torch.round(torch.sqrt(area / aspect)).long()
    ok = (cw >= 1) & (cw <= hw[:, 1:2]) & (ch >= 1) & (ch <= hw[:, 0:1])
    first = torch.argmax(ok.int(), dim=1, keepdim=True)                      # the first accepted attempt (0 if none)
    take = lambda t: torch.gather(t, 1, first)[:, 0]
    ch_a, cw_a = take(ch), take(cw)
    y0_a = torch.minimum(torch.floor(take(u[..., 2]) * (hw[:, 0] - ch_a + 1).double()).long(), hw[:, 0] - ch_a)
    x0_a = torch.minimum(torch.floor(take(u[..., 3]) * (hw[:, 1] - cw_a + 1).double()).long(), hw[:, 1] - cw_a)
    # the fallback: the whole image, cut to the nearest allowed aspect
    in_ratio = (w / h)[:, 0]
    cw_f, ch_f = hw[:, 1].clone(), hw[:, 0].clone()
    narrow, wide = in_ratio < min(ratio), in_ratio > max(ratio)
    ch_f[narrow] = torch.round(hw[:, 1].double() / min(ratio)).long()[narrow]
    cw_f[wide] = torch.round(hw[:, 0].double() * max(ratio)).long()[wide]
    ch_f = torch.minimum(torch.clamp(ch_f, min=1), hw[:, 0])
    cw_f = torch.minimum(torch.clamp(cw_f, min=1), hw[:, 1])
    any_ok = ok.any(dim=1)
    pick = lambda a, f: torch.where(any_ok, a, f)
    box = torch.stack([pick(y0_a, (hw[:, 0] - ch_f) // 2), pick(x0_a, (hw[:, 1] - cw_f) // 2), pick(ch_a, ch_f),
                       pick(cw_a, cw_f)], dim=1).to(torch.int32)
    rot = torch.where(flips[:, 2] < p_rot90, k, torch.zeros_like(k))
    op = ((flips[:, 0] < p_hflip).long() | ((flips[:, 1] < p_vflip).long() << 1) | (rot << 2)).to(torch.int32)
    return box, op


def identity_params(hw):
    """The whole image, no flip, no rotation: the validation / extraction transform."""
    hw = torch.as_tensor(np.asarray(hw, dtype=np.int64)).reshape(-1, 2)
    box = torch.cat([torch.zeros_like(hw), hw], dim=1).to(torch.int32)
    return box, torch.zeros(hw.shape[0], dtype=torch.int32)


def augment(pool, index, box, op, size=224, mean=MEAN, std=STD, want_mask=True):
    """-> ``(images fp32 [B, 3, size, size], masks fp32 [B, 1, size, size] or None)`` on the pool's device.

    Output ``b`` is crop ``box[b] = (y0, x0, ch, cw)`` of pool image ``index[b]``, resized to ``size`` (bilinear, half-pixel
    centres; the mask nearest neighbour, its byte values unscaled), transformed by ``op[b]`` and normalised.  The
    parameters are validated here, on the host where they are made: ``ValueError`` for an index outside the pool, a box
    outside its image or an ``op`` above 15."""
    index = torch.as_tensor(index, dtype=torch.int64).reshape(-1).cpu()
    box = torch.as_tensor(box).to(torch.int64).reshape(-1, 4).cpu()
    op = torch.as_tensor(op).to(torch.int64).reshape(-1).cpu()
    B = index.numel()
    if box.shape[0] != B or op.numel() != B:
        raise ValueError(f"index, box and op disagree on the batch size: {B}, {box.shape[0]}, {op.numel()}")
    if not 1 <= int(size) <= 1024:
        raise ValueError(f"size: 1..1024, got {size}")
    if B and (int(index.min()) < 0 or int(index.max()) >= len(pool)):
        raise ValueError(f"index outside the pool of {len(pool)} images")
    if B and (int(op.min()) < 0 or int(op.max()) > 15):
        raise ValueError("op: a 4-bit code (bit 0 hflip, bit 1 vflip, bits 2-3 k of rot90), 0..15")
    if B:
        hw = pool.hw_host[index]
        y0, x0, ch, cw = box.unbind(1)
        bad = (y0 < 0) | (x0 < 0) | (ch < 1) | (cw < 1) | (y0 + ch > hw[:, 0]) | (x0 + cw > hw[:, 1])
        if bool(bad.any()):
            b = int(torch.nonzero(bad)[0])
            raise ValueError(f"box {box[b].tolist()} of output {b} lies outside its image {hw[b].tolist()}")
    dev = pool.device
    images = torch.empty((B, 3, size, size), device=dev, dtype=torch.float32)
    masks = torch.empty((B, 1, size, size), device=dev, dtype=torch.float32) if want_mask else None
    call("isic_augment_u8", pool.pixels, pool.masks if want_mask else None, pool.offsets, pool.hw, len(pool),
         index.to(dev), box.to(torch.int32).to(dev), op.to(torch.int32).to(dev), float(mean[0]), float(mean[1]),
         float(mean[2]), float(std[0]), float(std[1]), float(std[2]), images, masks, B, int(size))
    return images, masks


class SyntheticDermPixels(Dataset):
    """ISIC-shaped stand-in for the pool: deterministic uint8 images of varying, non-square sizes (``size=None``; a fixed
    ``size=(h, w)`` otherwise) with an elliptic lesion mask of byte value 255, the ``DermDataset`` dict contract with the
    arrays of ``uint8_transform``.  Every fifth image has no mask, as in ``save_latent.SyntheticDermImages``."""

    def __init__(self, n=32, size=None, classes=7, seed=42):
        self.n, self.size, self.classes, self.seed = n, size, classes, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 7919 + i)
        y = i % self.classes
        if self.size is None:
            h, w = (int(v) for v in torch.randint(160, 321, (2,), generator=g))
            if h == w:
                w += 1
        else:
            h, w = self.size
        # a smooth class-tinted gradient plus noise: every pixel differs from its neighbours, so a misplaced tap shows
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        base = torch.stack([(yy * 255) // max(h - 1, 1), (xx * 255) // max(w - 1, 1),
                            torch.full((h, w), 255 * y // max(self.classes - 1, 1))], dim=2)
        noise = torch.randint(-40, 41, (h, w, 3), generator=g)
        img = (base + noise).clamp(0, 255).to(torch.uint8)
        cy, cx = torch.rand(2, generator=g) * 0.5 + 0.25
        ry, rx = torch.rand(2, generator=g) * 0.25 + 0.08
        mask = ((((yy - cy * h) / (ry * h)) ** 2 + ((xx - cx * w) / (rx * w)) ** 2) <= 1.0).to(torch.uint8) * 255
        no_mask = i % 5 == 4
        if no_mask:
            mask = torch.zeros_like(mask)                       # the 'no_mask' case of dataset.py
        return {"image": img, "mask": mask, "radiomics": torch.zeros(102), "age": torch.tensor(0.0),
                "sex": torch.tensor(0), "loc": torch.tensor(0), "artifacts": torch.zeros(6, dtype=torch.long),
                "target": torch.tensor(y, dtype=torch.long), "image_path": f"synthetic/img_{i:05d}.jpg",
                "segmentation_path": "no_mask" if no_mask else f"synthetic/seg_{i:05d}.png"}
