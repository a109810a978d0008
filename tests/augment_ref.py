"""float64 numpy restatement of the batch transform of include/isic_hip_augment.h: crop, exact-rational bilinear resize,
hflip / vflip / rot90, normalisation; integer nearest neighbour for the mask.  Written forwards (resize, then flip, then
rotate), where the kernel works backwards from the output pixel."""
import numpy as np


def axis_taps(n, S):
    """Per index r of the resized axis (length S) over a crop axis of length n: (i0, i1, weight of i1), exactly."""
    r = np.arange(S, dtype=np.int64)
    num = np.maximum((2 * r + 1) * n - S, 0)
    i0 = np.minimum(num // (2 * S), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    return i0, i1, (num % (2 * S)).astype(np.float64) / (2 * S)


def nearest_index(n, S):
    return np.minimum((np.arange(S, dtype=np.int64) * n) // S, n - 1)


def resize_bilinear(crop, S):
    """crop: [ch, cw, C] any dtype -> float64 [S, S, C]."""
    crop = crop.astype(np.float64)
    y0, y1, wy = axis_taps(crop.shape[0], S)
    x0, x1, wx = axis_taps(crop.shape[1], S)
    wx = wx[None, :, None]
    top = crop[y0][:, x0] * (1 - wx) + crop[y0][:, x1] * wx
    bot = crop[y1][:, x0] * (1 - wx) + crop[y1][:, x1] * wx
    wy = wy[:, None, None]
    return top * (1 - wy) + bot * wy


def resize_nearest(crop, S):
    return crop[nearest_index(crop.shape[0], S)][:, nearest_index(crop.shape[1], S)]


def transform(a, op):
    """a: [S, S, ...]; op bit 0 hflip, bit 1 vflip, bits 2-3 k of np.rot90 -- applied in that order."""
    if op & 1:
        a = a[:, ::-1]
    if op & 2:
        a = a[::-1]
    return np.rot90(a, (op >> 2) & 3)


def augment(images, masks, index, box, op, S, mean, std):
    """images: list of HWC uint8; masks: list of HW uint8 -> (float64 [B, 3, S, S], float64 [B, 1, S, S])."""
    B = len(index)
    out = np.zeros((B, 3, S, S))
    mout = np.zeros((B, 1, S, S))
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    for b in range(B):
        y0, x0, ch, cw = (int(v) for v in box[b])
        img = images[int(index[b])][y0:y0 + ch, x0:x0 + cw]
        v = transform(resize_bilinear(img, S), int(op[b]))
        out[b] = ((v / 255.0 - mean) / std).transpose(2, 0, 1)
        m = masks[int(index[b])][y0:y0 + ch, x0:x0 + cw]
        mout[b, 0] = transform(resize_nearest(m, S), int(op[b])).astype(np.float64)
    return out, mout
