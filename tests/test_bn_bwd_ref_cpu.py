"""The numpy emulation of csrc/bn_bwd_math.inc (tests/bn_bwd_ref.py) on its own, on the seeded inputs the GPU test uses:
nothing of the apply and reduce passes is left unchecked, the emulation can tell the fused dx from the unfused one, and
the gate handles the awkward values."""
import functools

import numpy as np
import pytest

import bn_bwd_ref as R

SHAPES = R.FLAT_SHAPES + R.POOLED_SHAPES + R.WGRAD_SHAPES
ids = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _case(shape):
    return R.pooled_case(shape) if shape in R.POOLED_SHAPES else R.shape_case(shape)


def _norm(cs, second):
    n = "2" if second else ""
    return cs["x" + n], cs["mean" + n], cs["rstd" + n], cs["gamma" + n], cs["sum_dzx" + n], cs["sum_dz"], cs["rows"]


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_nothing_of_the_apply_pass_is_unchecked_and_fused_differs_from_unfused(shape):
    cs = _case(shape)
    for mode in range(4):
        dz, sure = R.case_gate(cs, mode)
        assert sure.all(), f"mode {mode}: {(~sure).mean():.4f} of the gates unchecked"
        for second in (False, True):
            fused, checked = R.apply_pass(dz, *_norm(cs, second), dz_checked=sure)
            unfused, _ = R.apply_pass(dz, *_norm(cs, second), dz_checked=sure, unfused=True)
            differ = float((fused != unfused).mean())
            print(f"mode {mode} norm {1 + second}: unchecked {(~checked).mean():.4f}, fused != unfused in {differ:.4f}")
            assert checked.all(), f"mode {mode}: {(~checked).mean():.4f} of the outputs unchecked"
            assert differ >= 0.01, f"mode {mode}: the emulation tells fused from unfused in {differ:.4f} of the elements only"


@pytest.mark.parametrize("shape", R.FLAT_SHAPES + R.WGRAD_SHAPES, ids=ids)
def test_every_sum_of_the_flat_reduce_is_exact(shape):
    cs = _case(shape)
    dz, sure = R.case_gate(cs, 3)
    (dzx, dzx2), sdz = R.reduce_flat(dz, [cs["x"], cs["x2"]], [cs["mean"], cs["mean2"]], [cs["rstd"], cs["rstd2"]], sure)
    assert dzx[1].all() and dzx2[1].all() and sdz[1].all()
    # against plain fp64 sums of the same terms (every term is exact, so the partition does not show in the total)
    xhat = (cs["x"].astype(np.float64) - cs["mean"]) * cs["rstd"]
    assert np.array_equal(dzx[0], (dz.astype(np.float64) * xhat).sum(axis=0))
    assert np.array_equal(sdz[0], dz.astype(np.float64).sum(axis=0))
    assert np.abs(dzx[0]).max() > 0 and np.abs(dzx2[0]).max() > 0


@pytest.mark.parametrize("shape", R.POOLED_SHAPES, ids=ids)
def test_every_sum_of_the_pooled_reduce_is_exact(shape):
    N, H, W, C = shape
    cs = _case(shape)
    dz, sure = R.case_gate(cs, 2)
    x4, dz4 = cs["x"].reshape(N, H, W, C), dz.reshape(N, H, W, C)
    dzx, sdz = R.reduce_pooled(dz4, x4, cs["mean"], cs["rstd"], N, H, W)
    assert sure.all() and dzx[1].all() and sdz[1].all()
    xhat = (cs["x"].astype(np.float64) - cs["mean"]) * cs["rstd"]
    assert np.array_equal(dzx[0], (dz.astype(np.float64) * xhat).sum(axis=0))
    assert np.array_equal(sdz[0], dz.astype(np.float64).sum(axis=0))


def test_fma_marks_an_inexact_fp64_sum_unchecked():
    v, sure = R.fma(np.float32([1.0, 1.0 + 2.0 ** -23]), np.float32([1.0, 1.0 + 2.0 ** -23]), np.float32([0.5, 2.0 ** 40]))
    assert sure.tolist() == [True, False]          # (1 + 2^-23)^2 has 47 bits; next to 2^40 the sum needs 87
    assert v[0] == np.float32(1.5)


def test_the_gate_handles_the_awkward_values():
    g = np.float32([[3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0]])
    x = np.float32([[1.0, 1.0, -1.0, -1.0, 0.0, 0.0, 2.0, 2.0]])
    scale = np.float32([2.0, -2.0, 2.0, -2.0, 2.0, -2.0, 0.5, -0.5])
    shift = np.float32([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 1.0])
    dz, sure = R.gate(2, g, x=x, scale=scale, shift=shift)
    # a negative scale flips the gate; x * scale + shift == 0 (from either side) closes it
    assert sure.all() and dz.tolist() == [[3.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 0.0]]
    y = np.float32([[0.0, -0.0, 2.0 ** -126, -1.0, np.nan, np.inf, 1.0, -np.inf]])
    dz, _ = R.gate(1, g, y=y)
    assert dz.tolist() == [[0.0, 0.0, 3.0, 0.0, 0.0, 3.0, 3.0, 0.0]]          # !(y > 0) ? 0 : g -- a NaN output gates to 0
    bits = R.unpack_mask(np.uint8([0b10100101]), 1, 8)
    assert R.gate(3, g, bits=bits)[0].tolist() == [[3.0, 0.0, 3.0, 0.0, 0.0, 3.0, 0.0, 3.0]]
    assert R.gate(0, g)[0].tolist() == g.tolist()


def test_bf16_rounding_is_to_nearest_even():
    f = np.float32([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -2.5])
    assert R.bf16_bits(f).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0xC020]
    assert np.array_equal(R.bf16_value(R.bf16_bits(np.float32([0.75, -3.0]))), np.float32([0.75, -3.0]))
