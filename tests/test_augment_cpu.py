"""CPU-only checks of the device augmentation path (isic_hip/augment.py, include/isic_hip_augment.h): the float64
restatement of the kernel's formulas against torch, the parameter sampler's distribution and determinism, the host-side
validation of ``augment`` and the argument checks of ``isic_augment_u8`` (before any device work)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-isic_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import augment_ref as ar  # noqa: E402
from isic_hip import augment as ag  # noqa: E402
from isic_hip import lib  # noqa: E402

P = 1 << 20                      # a non-NULL "device" pointer: never dereferenced, the checks answer first
BAD_ARG = -1
S = 224
CROPS = ((1, 1), (7, 5), (223, 225), (224, 224), (450, 450), (600, 450), (1024, 1024), (1500, 1200))


@pytest.mark.parametrize("ch,cw", CROPS)
def test_restatement_matches_torch_bilinear(ch, cw):
    """augment_ref's image path against ``F.interpolate(bilinear, align_corners=False)`` of the cut-out crop, for the full
    box and for a box inside a larger image (so the taps clamp to the crop, not the image).  Bound, in normalised units:
    3 max(ch, cw) 2^-24 / min(std) + 1e-5 -- torch computes its source coordinate scale * (r + 0.5) - 0.5 in fp32, whose
    rounding error grows with the coordinate, i.e. with the crop's longer side, and moves the weight by as much; the
    restatement's coordinates are exact.  At 224 -> 224 the resize is the identity (checked exactly) and only the fp32
    normalisation of the torch side is left.

    The mask is not compared with torch: the nearest-neighbour rule here is the exact integer floor(r n / S), and torch's
    fp32 ``nearest`` differs from it at isolated rows for some crop lengths (62 and 76 are the first two)."""
    rng = np.random.RandomState(ch * 7919 + cw)
    big = rng.randint(0, 256, size=(ch + 7, cw + 5, 3)).astype(np.uint8)
    full = np.ascontiguousarray(big[3:3 + ch, 2:2 + cw])
    mean, std = np.asarray(ag.MEAN), np.asarray(ag.STD)
    t = torch.from_numpy(full).permute(2, 0, 1).float().unsqueeze(0) / 255.0
    t = torch.nn.functional.interpolate(t, size=(S, S), mode="bilinear", align_corners=False)[0]
    want = ((t - torch.tensor(ag.MEAN).view(3, 1, 1)) / torch.tensor(ag.STD).view(3, 1, 1)).double().numpy()
    bound = 3 * max(ch, cw) * 2.0 ** -24 / std.min() + 1e-5
    zeros = [np.zeros(full.shape[:2], np.uint8), np.zeros(big.shape[:2], np.uint8)]
    got_full, _ = ar.augment([full, big], zeros, [0], [(0, 0, ch, cw)], [0], S, mean, std)
    got_in, _ = ar.augment([full, big], zeros, [1], [(3, 2, ch, cw)], [0], S, mean, std)
    for got in (got_full[0], got_in[0]):
        err = float(np.abs(got - want).max())
        print(f"crop {ch}x{cw}: max |restatement - torch| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    assert np.array_equal(got_full, got_in)
    if (ch, cw) == (S, S):                                                        # the identity: every weight is 0
        assert np.array_equal(ar.resize_bilinear(full, S), full.astype(np.float64))


def test_reference_op_codes_compose_in_order():
    a = np.arange(12 * 12).reshape(12, 12)
    assert np.array_equal(ar.transform(a, 0), a)
    assert np.array_equal(ar.transform(a, 1), np.fliplr(a)) and np.array_equal(ar.transform(a, 2), np.flipud(a))
    assert np.array_equal(ar.transform(a, 1 | 2 | (3 << 2)), np.rot90(np.flipud(np.fliplr(a)), 3))
    assert np.array_equal(ar.nearest_index(5, 7), [0, 0, 1, 2, 2, 3, 4])


def _draw(hw, n, seed):
    g = torch.Generator().manual_seed(seed)
    return ag.sample_params(np.tile(np.asarray(hw), (n, 1)), g)


@pytest.mark.parametrize("hw", [(450, 450), (450, 600)])
def test_sample_params_distribution(hw):
    """20 000 draws.  With x = sqrt(area aspect) and y = sqrt(area / aspect) the real-valued sides, cw = round(x) and
    ch = round(y) give |cw - x| <= 1/2 and |ch - y| <= 1/2, so
        (cw - 1/2)(ch - 1/2) <= x y = area <= (cw + 1/2)(ch + 1/2)   and   (cw - 1/2) / (ch + 1/2) <= x / y <= (cw + 1/2) / (ch - 1/2):
    area in [0.5, 1] h w and aspect in [0.75, 1.33] therefore imply the four inequalities asserted below.  (The fallback
    crop, should ten attempts fail, is the whole image cut to an aspect inside the range: it obeys them as well.)
    Frequencies: flips 0.5 +- 0.02, k != 0 at 0.5 * 3/4 = 0.375 +- 0.02 (five standard deviations of 20 000 draws are
    0.018)."""
    n = 20000
    h, w = hw
    box, op = _draw(hw, n, 1234)
    assert box.dtype == torch.int32 and op.dtype == torch.int32 and box.shape == (n, 4) and op.shape == (n,)
    y0, x0, ch, cw = (box[:, i].double() for i in range(4))
    assert bool(((y0 >= 0) & (x0 >= 0) & (ch >= 1) & (cw >= 1) & (y0 + ch <= h) & (x0 + cw <= w)).all())
    assert bool(((cw + 0.5) * (ch + 0.5) >= 0.5 * h * w).all()) and bool(((cw - 0.5) * (ch - 0.5) <= h * w).all())
    assert bool(((cw + 0.5) / (ch - 0.5) >= 0.75).all()) and bool(((cw - 0.5) / (ch + 0.5) <= 1.33).all())
    frac = (ch * cw / (h * w))
    assert 0.6 < float(frac.mean()) < 0.8 and float(frac.min()) < 0.52          # the scale range is used, not one value
    assert len(torch.unique(y0)) > 50 and len(torch.unique(x0)) > 50             # corners move
    assert bool((op >= 0).all()) and bool((op <= 15).all())
    assert abs(float((op & 1).bool().double().mean()) - 0.5) <= 0.02
    assert abs(float((op & 2).bool().double().mean()) - 0.5) <= 0.02
    k = (op >> 2) & 3
    assert abs(float((k != 0).double().mean()) - 0.375) <= 0.02
    assert all(abs(float((k == v).double().mean()) - 0.125) <= 0.01 for v in (1, 2, 3))
    box2, op2 = _draw(hw, n, 1234)
    assert torch.equal(box, box2) and torch.equal(op, op2)
    box3, _ = _draw(hw, n, 1235)
    assert not torch.equal(box, box3)


def test_sample_params_fallback_obeys_the_ratio_clamp():
    """A 50 x 400 image: any attempt has ch = sqrt(area / aspect) >= sqrt(0.5 * 20000 / 1.33) = 86.7 > 50, so none is accepted
    and every draw is the centred fallback: full height, width round(50 * 1.33) = 66."""
    box, op = _draw((50, 400), 500, 7)
    assert bool((box == torch.tensor([0, 167, 50, 66], dtype=torch.int32)).all())
    assert len(torch.unique(op)) > 8                                              # the flips still vary
    box, _ = _draw((400, 50), 500, 7)                                             # too narrow: full width, round(50 / 0.75)
    assert bool((box == torch.tensor([166, 0, 67, 50], dtype=torch.int32)).all())


def test_identity_params():
    box, op = ag.identity_params([(5, 7), (600, 450)])
    assert box.tolist() == [[0, 0, 5, 7], [0, 0, 600, 450]] and op.tolist() == [0, 0]
    assert box.dtype == torch.int32 and op.dtype == torch.int32


def _host_pool():
    rng = np.random.RandomState(0)
    items = [(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8), None if h == 7 else np.zeros((h, w), np.uint8))
             for h, w in ((7, 5), (20, 30))]
    return ag.ImagePool.from_arrays(items, "cpu")


def test_pool_layout_on_the_host():
    pool = _host_pool()
    assert len(pool) == 2 and pool.offsets.tolist() == [0, 35, 635] and pool.hw.tolist() == [[7, 5], [20, 30]]
    assert pool.pixels.numel() == 3 * 635 and pool.masks.numel() == 635 and pool.nbytes == 4 * 635
    assert pool.pixels.dtype == torch.uint8 and pool.offsets.dtype == torch.int64 and pool.hw.dtype == torch.int32
    with pytest.raises(ValueError):
        ag.ImagePool.from_arrays([(np.zeros((4, 4, 3), np.float32), None)], "cpu")
    with pytest.raises(ValueError):
        ag.ImagePool.from_arrays([(np.zeros((4, 4, 3), np.uint8), np.zeros((4, 5), np.uint8))], "cpu")


def test_pool_from_dataset_and_max_bytes():
    ds = ag.SyntheticDermPixels(n=10)
    sizes = [tuple(ds[i]["image"].shape[:2]) for i in range(10)]
    assert len(set(sizes)) > 5 and all(h != w for h, w in sizes)
    assert torch.equal(ds[3]["image"], ds[3]["image"]) and ds[3]["image"].dtype == torch.uint8
    assert not bool(ds[4]["mask"].any()) and ds[4]["segmentation_path"] == "no_mask" and bool(ds[3]["mask"].any())
    pool = ag.ImagePool.from_dataset(ds, "cpu")
    assert pool.hw_host.tolist() == [list(s) for s in sizes]
    assert pool.labels == [i % 7 for i in range(10)] and pool.image_path[2] == "synthetic/img_00002.jpg"
    o = int(pool.offsets[3])
    h, w = sizes[3]
    assert torch.equal(pool.pixels[3 * o:3 * (o + h * w)].view(h, w, 3), ds[3]["image"])
    assert torch.equal(pool.masks[o:o + h * w].view(h, w), ds[3]["mask"])
    need = 4 * sum(h * w for h, w in sizes)
    assert pool.nbytes == need
    ag.ImagePool.from_dataset(ds, "cpu", max_bytes=need)
    with pytest.raises(ValueError, match="bytes"):
        ag.ImagePool.from_dataset(ds, "cpu", max_bytes=need - 1)


def test_augment_validates_on_the_host_before_the_library(monkeypatch):
    pool = _host_pool()
    monkeypatch.setattr(ag, "call", lambda *a, **k: pytest.fail("the library was called"))
    box, op = ag.identity_params(pool.hw_host)
    for bad_index in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="index"):
            ag.augment(pool, bad_index, box, op)
    for bad_box in ((0, 0, 8, 5), (1, 0, 7, 5), (0, 1, 7, 5), (0, 0, 0, 5), (-1, 0, 7, 5), (0, 0, 7, 6)):
        with pytest.raises(ValueError, match="box"):
            ag.augment(pool, [0, 1], torch.tensor([bad_box, (0, 0, 20, 30)]), op)
    for bad_op in (16, -1):
        with pytest.raises(ValueError, match="op"):
            ag.augment(pool, [0, 1], box, [0, bad_op])
    with pytest.raises(ValueError):
        ag.augment(pool, [0, 1], box, op, size=1025)
    with pytest.raises(ValueError):
        ag.augment(pool, [0, 1], box[:1], op)


def test_entry_point_declared_exported_and_checks_arguments_without_a_device():
    L = lib.lib()
    protos = lib.parse_header(os.path.join(os.path.dirname(lib.header_path()), "isic_hip_augment.h"))
    assert set(protos) == {"isic_augment_u8"} and protos["isic_augment_u8"][1][-1][1] == "stream"
    assert "isic_augment_u8" in L.extension and "isic_augment_u8" not in L.public
    f = L.fn["isic_augment_u8"]
    norm = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)
    args = lambda masks=P, mask_out=P, B=2, S=224, n_pool=3, norm=norm, pixels=P: (
        pixels, masks, P, P, n_pool, P, P, P) + tuple(norm) + (P, mask_out, B, S, None)
    assert f(*args(S=0)) == BAD_ARG and f(*args(S=1025)) == BAD_ARG
    assert f(*args(B=-1)) == BAD_ARG
    assert f(*args(masks=None)) == BAD_ARG                                        # mask_out without masks
    assert f(*args(pixels=None)) == BAD_ARG and f(*args(n_pool=0)) == BAD_ARG
    assert f(*args(norm=norm[:3] + (0.229, 0.0, 0.225))) == BAD_ARG
    assert f(*args(B=0)) == 0 and f(None, None, None, None, 0, None, None, None, *norm, None, None, 0, 224, None) == 0
