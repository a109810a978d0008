"""Every kernel that takes its BatchNorm-backward arithmetic from csrc/bn_bwd_math.inc against the numpy emulation of that
include (tests/bn_bwd_ref.py), bit for bit: the flat apply entries (three ReLU forms, mask bits, the pair), the apply fed by
the pooled gradient, the `dc` output of the 64-channel weight gradient with the apply pass folded in, and the four reduce
entries with the kernels' own partition of the rows.

The emulation marks the elements whose fused multiply-adds it cannot vouch for; tests/test_bn_bwd_ref_cpu.py shows there are
none for these inputs, so "the checked elements" below are all of them (asserted again here, so a comparison cannot go
vacuous).  The inputs are built so that the fused and the unfused form of dx differ in 6-23 % of the bf16 outputs: a kernel
that rounds differently from the include does not pass.  This pins behaviour, not a build: it passes on the commit before
the include existed.  The fused stem weight gradient has no exact check (its dY never leaves LDS);
tests/test_stem_wgrad_fused_gpu.py stays its test."""
import functools

import numpy as np
import pytest
import torch

import bn_bwd_ref as R
from isic_hip.lib import call

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ids = lambda s: "x".join(map(str, s))


def _bf16(values):
    """fp32 values that bf16 holds exactly -> device bf16 tensor"""
    bits = R.bf16_bits(values)
    assert np.array_equal(R.bf16_value(bits), np.asarray(values, dtype=np.float32))
    return torch.from_numpy(bits.view(np.int16)).to(DEV).view(torch.bfloat16)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Host operands, their device copies and the reference's dz per gate mode, computed once per shape and left unchanged."""
    cs = R.pooled_case(shape) if shape in R.POOLED_SHAPES else R.shape_case(shape)
    d = {k: _bf16(cs[k]) for k in ("x", "x2", "dy", "y")}
    d.update({k: _dev(cs[k]) for k in ("mean", "rstd", "gamma", "mean2", "rstd2", "gamma2", "scale", "shift", "sum_dzx",
                                       "sum_dzx2", "sum_dz", "mask")})
    if "gp" in cs:
        d.update(gp=_bf16(cs["gp"]), argmax=_dev(cs["argmax"]))
    gates = {m: R.case_gate(cs, m) for m in range(4)}
    return cs, d, gates


def _expected_dx(cs, gates, mode, second=False):
    n = "2" if second else ""
    dz, sure = gates[mode]
    bits, checked = R.apply_pass(dz, cs["x" + n], cs["mean" + n], cs["rstd" + n], cs["gamma" + n], cs["sum_dzx" + n],
                                 cs["sum_dz"], cs["rows"], dz_checked=sure)
    assert checked.all(), "the reference leaves elements unchecked"
    return bits


def _start(cs, keys=("dgamma", "dbeta")):
    return [_dev(cs["start"][k]) for k in keys]


def _same_bits(got, want, what):
    got = _bits(got).reshape(want.shape)
    n = int((got != want).sum())
    print(f"{what}: {n} of {want.size} bit patterns differ")
    assert n == 0, f"{what}: {n} of {want.size} bit patterns differ from the emulation of bn_bwd_math.inc"


def _check_fold(cs, got, sums):
    for t, start, s in zip(got, ("dgamma", "dbeta"), sums):
        assert np.array_equal(t.cpu().numpy(), R.fold(cs["start"][start], cs[s])), f"{start}_f32"


# ------------------------------------------------------------------------------------------------ the apply entries
@pytest.mark.parametrize("residual", [False, True], ids=["dx", "dx+residual"])
@pytest.mark.parametrize("form", ["none", "from_y", "from_x", "mask"])
@pytest.mark.parametrize("shape", R.FLAT_SHAPES, ids=ids)
def test_apply(shape, form, residual):
    cs, d, gates = _case(shape)
    rows, C = cs["rows"], cs["C"]
    mode = ("none", "from_y", "from_x", "mask").index(form)
    dx = torch.full_like(d["x"], float("nan"))
    dres = torch.full_like(d["x"], float("nan")) if residual else None
    dg, db = _start(cs)
    if form == "mask":
        call("isic_bn_bwd_apply_mask_bf16", d["dy"], d["x"], d["mask"], d["mean"], d["rstd"], d["gamma"], d["sum_dzx"],
             d["sum_dz"], rows, C, dx, dres, dg, db)
    else:
        call("isic_bn_bwd_apply_bf16", d["dy"], d["x"], d["y"] if form == "from_y" else None, d["mean"], d["rstd"], d["gamma"],
             d["sum_dzx"], d["sum_dz"], rows, C, int(form != "none"), d["scale"] if form == "from_x" else None,
             d["shift"] if form == "from_x" else None, dx, dres, dg, db)
    torch.cuda.synchronize()
    _same_bits(dx, _expected_dx(cs, gates, mode), "dx")
    if residual:
        _same_bits(dres, R.bf16_bits(gates[mode][0]), "d_residual")
    _check_fold(cs, (dg, db), ("sum_dzx", "sum_dz"))


@pytest.mark.parametrize("shape", R.FLAT_SHAPES, ids=ids)
def test_apply_pair(shape):
    cs, d, gates = _case(shape)
    rows, C = cs["rows"], cs["C"]
    dx, dx2 = torch.full_like(d["x"], float("nan")), torch.full_like(d["x"], float("nan"))
    dg, db, dg2, db2 = _start(cs, ("dgamma", "dbeta", "dgamma2", "dbeta2"))
    call("isic_bn_bwd_apply_pair_bf16", d["dy"], d["x"], d["mask"], d["mean"], d["rstd"], d["gamma"], d["sum_dzx"], d["sum_dz"],
         d["x2"], d["mean2"], d["rstd2"], d["gamma2"], d["sum_dzx2"], rows, C, dx, dx2, dg, db, dg2, db2)
    torch.cuda.synchronize()
    _same_bits(dx, _expected_dx(cs, gates, 3), "dx")
    _same_bits(dx2, _expected_dx(cs, gates, 3, second=True), "dx2")
    _check_fold(cs, (dg, db), ("sum_dzx", "sum_dz"))
    assert np.array_equal(dg2.cpu().numpy(), R.fold(cs["start"]["dgamma2"], cs["sum_dzx2"]))
    assert np.array_equal(db2.cpu().numpy(), R.fold(cs["start"]["dbeta2"], cs["sum_dz"]))


@pytest.mark.parametrize("shape", R.POOLED_SHAPES, ids=ids)
def test_apply_pooled(shape):
    N, H, W, C = shape
    cs, d, gates = _case(shape)
    dx = torch.full_like(d["x"], float("nan"))
    dg, db = _start(cs)
    call("isic_bn_bwd_apply_pooled_bf16", d["argmax"], d["gp"], d["x"], d["mean"], d["rstd"], d["gamma"], d["sum_dzx"],
         d["sum_dz"], N, H, W, C, cs["Ho"], cs["Wo"], d["scale"], d["shift"], dx, dg, db)
    torch.cuda.synchronize()
    _same_bits(dx, _expected_dx(cs, gates, 2), "dx")
    _check_fold(cs, (dg, db), ("sum_dzx", "sum_dz"))


@pytest.mark.parametrize("form", ["from_x", "mask"])
@pytest.mark.parametrize("shape", R.WGRAD_SHAPES, ids=ids)
def test_wgrad_bnbwd_dc(shape, form):
    N, H, W = shape
    C = 64
    cs, d, gates = _case(shape)
    use_mask = form == "mask"
    assert call("isic_conv2d_wgrad_bnbwd_supported", N, H, W, C, C, 3, 3, 1, 1, int(use_mask)) == 1
    ws = torch.empty(call("isic_conv2d_wgrad_workspace_bytes", N, C, H, W, C, 3, 3), device=DEV, dtype=torch.uint8)
    dc = torch.full_like(d["x"], float("nan"))
    dw = torch.zeros(C, 3, 3, C, device=DEV)
    dg, db = _start(cs)
    call("isic_conv2d_wgrad_bnbwd_bf16", d["x2"], d["dy"], d["x"], d["mask"] if use_mask else None, d["mean"], d["rstd"],
         d["gamma"], d["sum_dz"], d["sum_dzx"], None if use_mask else d["scale"], None if use_mask else d["shift"], dc, dw, dg,
         db, N, H, W, ws, ws.numel())
    torch.cuda.synchronize()
    _same_bits(dc, _expected_dx(cs, gates, 3 if use_mask else 2), "dc")
    _check_fold(cs, (dg, db), ("sum_dzx", "sum_dz"))
    assert bool(torch.isfinite(dw).all()) and float(dw.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ the reduce entries
def _same_sums(got, want, what):
    total, checked = want
    assert checked.all(), f"{what}: the reference cannot vouch for every channel"
    got = got.cpu().numpy()
    print(f"{what}: max |device - emulation| = {np.abs(got - total).max():.3e}")
    assert np.array_equal(got, total), f"{what}: {int((got != total).sum())} of {total.size} channels differ"
    assert np.abs(total).max() > 0


@pytest.mark.parametrize("form", ["none", "from_y", "from_x", "mask", "pair"])
@pytest.mark.parametrize("shape", R.FLAT_SHAPES, ids=ids)
def test_reduce(shape, form):
    cs, d, gates = _case(shape)
    rows, C = cs["rows"], cs["C"]
    mode = 3 if form == "pair" else ("none", "from_y", "from_x", "mask").index(form)
    dz, sure = gates[mode]
    pair = form == "pair"
    want, want_dz = R.reduce_flat(dz, [cs["x"], cs["x2"]][:1 + pair], [cs["mean"], cs["mean2"]][:1 + pair],
                                  [cs["rstd"], cs["rstd2"]][:1 + pair], sure)
    acc = torch.zeros(3, C, device=DEV, dtype=torch.float64)
    if pair:
        call("isic_bn_bwd_reduce_pair_bf16", d["dy"], d["x"], d["mask"], d["mean"], d["rstd"], d["x2"], d["mean2"], d["rstd2"],
             rows, C, acc[0], acc[1], acc[2])
    elif form == "mask":
        call("isic_bn_bwd_reduce_mask_bf16", d["dy"], d["x"], d["mask"], d["mean"], d["rstd"], rows, C, acc[0], acc[1])
    else:
        call("isic_bn_bwd_reduce_bf16", d["dy"], d["x"], d["y"] if form == "from_y" else None, d["mean"], d["rstd"], rows, C,
             int(form != "none"), d["scale"] if form == "from_x" else None, d["shift"] if form == "from_x" else None, acc[0],
             acc[1])
    torch.cuda.synchronize()
    _same_sums(acc[0], want[0], "sum dz * xhat")
    _same_sums(acc[1], want_dz, "sum dz")
    if pair:
        _same_sums(acc[2], want[1], "sum dz * xhat2")


@pytest.mark.parametrize("shape", R.POOLED_SHAPES, ids=ids)
def test_reduce_pooled(shape):
    N, H, W, C = shape
    cs, d, gates = _case(shape)
    dz, sure = gates[2]
    assert sure.all()
    want, want_dz = R.reduce_pooled(dz.reshape(N, H, W, C), cs["x"].reshape(N, H, W, C), cs["mean"], cs["rstd"], N, H, W)
    acc = torch.zeros(2, C, device=DEV, dtype=torch.float64)
    call("isic_bn_bwd_reduce_pooled_bf16", d["argmax"], d["gp"], d["x"], d["mean"], d["rstd"], N, H, W, C, cs["Ho"], cs["Wo"],
         d["scale"], d["shift"], acc[0], acc[1])
    torch.cuda.synchronize()
    _same_sums(acc[0], want, "sum dz * xhat")
    _same_sums(acc[1], want_dz, "sum dz")
