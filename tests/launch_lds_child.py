"""Run by tests/test_launch_lds_gpu.py in a process of its own (the once-per-device opt-in of isic_launch_lds is per
process: in the suite's process other tests may already have launched these kernels).

The three entries that used to set MaxDynamicSharedMemorySize on every launch, to that launch's own byte count, are called
with a rising and then falling need of dynamic LDS: below 48 KB, above it, near the entry's bound, below 48 KB again, and
once beyond the bound (ISIC_ERR_UNSUPPORTED, outputs untouched).  The byte counts are the entries' own `lds` expressions,
restated below and asserted, so a case cannot drift off the side of 48 KB it is meant for.

  isic_attn_pool_fwd        attn_pool_fwd_kernel<16, 0> (H = 1024): heads 1 | 2 | 4 (A = 1536) | 1, and the sizes the
                            kernels of the narrower widths take (heads 1, H 128 | heads 4, H 512); A = 2304 is refused
  isic_attn_pool_bwd_sums   attn_pool_bwd_kernel<false>, teacher form, H = 1024: C 2 | C 16 | C 16, A = 23000 | C 2; A = 24000
                            is refused; attn_pool_bwd_kernel<true> with the parameter sums once
  isic_attn_pool_wide_fwd   pool_wide_att_kernel<true>, heads 8: max_bag 16 | 2048 | 2048 with A = 512 | 16; max_bag 2049 is
                            refused (the domain of include/isic_hip_wide.h ends below 160 KB); the backward once
  isic_knn_graph            knn_kernel (D = 24: the Gram kernel does not take it), k = 4: 100 | 800 | 2300 | 100 nodes; 2500 nodes
                            are refused

References and bounds: tests/f32_kernel_ref.py (pool_eval in fp64, pool_bounds) as tests/test_f32_kernel_domain_gpu.py and
tests/test_wide_rows_gpu.py use them; the k-NN indices against oracle.graphs.pairwise_sqdist + topk wherever the oracle's
neighbouring distances are more than 1e-3 apart (tests/test_graph_gpu.py::test_knn_random_batched_with_gap_guard), which
holds for at least 95 % of the positions of every graph here (checked on the CPU for these seeds: 99.8 % and more).

Every call is followed by a synchronisation: a device error ends the script at once, nothing more is launched."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "multimodal-isic_amd")):
    sys.path.insert(0, p)

import f32_kernel_ref as R  # noqa: E402
from helpers import DEV, Guarded, assert_close  # noqa: E402
from oracle import graphs  # noqa: E402

F64 = torch.float64
UNSUPPORTED = -2
KB = 1024
OPT_IN = 48 * KB                                     # what a kernel gets without the attribute
POOL_BOUND, KNN_BOUND = 160 * KB, 150 * KB
BAGS = (8, 32, 17)
WIDE_BAGS = (8, 16, 11)
KNN_GAP = 1e-3
KNN_GUARDED_SHARE = 0.95


def call(*a):
    from isic_hip.lib import call as c
    rc = c(*a)
    torch.cuda.synchronize()
    return rc


def code(*a):
    from isic_hip.lib import IsicHipError
    try:
        call(*a)
    except IsicHipError as e:
        return e.code
    return 0


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def untouched(*gs):
    return all(bool(torch.isnan(g.buf).all()) for g in gs)


def check(what, ratios):
    print(what, " ".join(f"{k} {v:.3f}" for k, v in ratios.items()), flush=True)
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


def side(lds, where, bound):
    """asserts that `lds` bytes lie where the case is meant to: "small" | "above" | "top" | "beyond" """
    ok = {"small": lds <= OPT_IN, "above": OPT_IN < lds <= bound, "top": 0.95 * bound <= lds <= bound, "beyond": lds > bound}
    assert ok[where], (lds, where, bound)
    return f"{lds} B ({where})"


# ---------------------------------------------------------------- the entries' lds expressions (attn_pool.hip, wide_rows.hip, graph.hip)
def fwd_lds(H, A, nh, C, max_bag):
    return 4 * (nh * A + C * H + max_bag * nh + 2 * 8 * nh + 8 * 16 + 8 * nh * H + 2 * 4 + 4 * 8)


def bwd_lds(H, A, heads, C, max_bag, sums):
    return 4 * (heads * A + C * H + H + max_bag * heads + 16 * heads + (16 * (2 * heads * A + heads) if sums else 0))


def pad4(n):
    return (n + 3) & ~3


def wide_lds(A, heads, max_bag):
    return 4 * (pad4(heads * A) + pad4(max_bag * heads) + 16)


def knn_lds(n):
    return 16 * ((n + 63) // 64 * 64) * 4


_REF = {}


def pool_ref(H, A, heads, C, bags):
    key = (H, A, heads, C, bags)
    if key not in _REF:
        case = dict(H=H, A=A, heads=heads, C=C, family="random", bags=bags, arm="", accumulate_dh=0)
        inp = R.pool_inputs(case)
        ref = R.pool_eval(inp, F64)
        _REF[key] = (inp, ref, R.pool_bounds(inp, ref))
    return _REF[key]


# ---------------------------------------------------------------- isic_attn_pool_fwd
def pool_forward(H, A, heads, where):
    inp, ref, b = pool_ref(H, A, heads, 0, BAGS)
    T, B = inp.T, inp.B
    att, z = Guarded((T, heads)), Guarded((B, H))
    call("isic_attn_pool_fwd", dev(inp.h), dev(inp.t), dev(inp.w3), dev(inp.b3), None, None, inp.offsets.to(DEV), B, H, A, heads, 0,
         max(BAGS), att.t, z.t, None, None, None, None)
    assert att.ok() and z.ok()
    check(f"attn_pool_fwd H{H} A{A} h{heads} {side(fwd_lds(H, A, heads, 0, max(BAGS)), where, POOL_BOUND)}",
          R.pool_ratios(dict(att=att.cpu(), z=z.cpu()), ref, b, ("att", "z")))


def pool_forward_refused(H, A, heads):
    inp, _, _ = pool_ref(H, 64, heads, 0, BAGS)             # refused before anything is read: t need not be A wide
    side(fwd_lds(H, A, heads, 0, max(BAGS)), "beyond", POOL_BOUND)
    att, z = Guarded((inp.T, heads)), Guarded((inp.B, H))
    assert code("isic_attn_pool_fwd", dev(inp.h), dev(inp.t), dev(inp.w3), dev(inp.b3), None, None, inp.offsets.to(DEV), inp.B, H, A,
                heads, 0, max(BAGS), att.t, z.t, None, None, None, None) == UNSUPPORTED
    assert untouched(att, z)
    print(f"attn_pool_fwd H{H} A{A} h{heads} refused", flush=True)


# ---------------------------------------------------------------- isic_attn_pool_bwd_sums (teacher form: W4, one head)
def pool_backward(H, A, C, where, sums=False):
    inp, ref, b = pool_ref(H, A, 1, C, BAGS)
    T, B = inp.T, inp.B
    # the saved att and P are the reference's, rounded to fp32 (the forward of A = 23000 does not fit a workgroup's LDS)
    att, P = dev(ref.att.float()), dev(ref.P.float())
    d_h, d_u, d_s, d_P = Guarded((T, H)), Guarded((T, A)), Guarded((T, 1)), Guarded((T, C))
    psum = Guarded((B, 2 * A + 1)) if sums else None
    call("isic_attn_pool_bwd_sums", dev(inp.h), dev(inp.t), att, P, dev(inp.w3), dev(inp.W4), inp.offsets.to(DEV), B, H, A, 1, C,
         max(BAGS), dev(inp.dL), dev(inp.dz), d_h.t, 0, d_u.t, d_s.t, d_P.t, None if psum is None else psum.t)
    outs = dict(d_h=d_h, d_u=d_u, d_s=d_s, d_P=d_P, psum=psum)
    assert all(g.ok() for g in outs.values() if g is not None)
    check(f"attn_pool_bwd_sums H{H} A{A} C{C} {side(bwd_lds(H, A, 1, C, max(BAGS), sums), where, POOL_BOUND)}",
          R.pool_ratios({k: (None if g is None else g.cpu()) for k, g in outs.items()}, ref, b, R.POOL_BWD_KEYS))


def pool_backward_refused(H, A, C):
    inp, ref, _ = pool_ref(H, 64, 1, C, BAGS)
    side(bwd_lds(H, A, 1, C, max(BAGS), False), "beyond", POOL_BOUND)
    T = inp.T
    d_h, d_u, d_s, d_P = Guarded((T, H)), Guarded((T, 64)), Guarded((T, 1)), Guarded((T, C))
    assert code("isic_attn_pool_bwd_sums", dev(inp.h), dev(inp.t), dev(ref.att.float()), dev(ref.P.float()), dev(inp.w3), dev(inp.W4),
                inp.offsets.to(DEV), inp.B, H, A, 1, C, max(BAGS), dev(inp.dL), dev(inp.dz), d_h.t, 0, d_u.t, d_s.t, d_P.t,
                None) == UNSUPPORTED
    assert untouched(d_h, d_u, d_s, d_P)
    print(f"attn_pool_bwd_sums H{H} A{A} C{C} refused", flush=True)


# ---------------------------------------------------------------- isic_attn_pool_wide_fwd / _bwd
WIDE_H, WIDE_HEADS = 1100, 8


def wide_forward(A, max_bag, where, backward=False):
    inp, ref, b = pool_ref(WIDE_H, A, WIDE_HEADS, 0, WIDE_BAGS)
    T, B, H, heads = inp.T, inp.B, WIDE_H, WIDE_HEADS
    h, t, w3, offsets = dev(inp.h), dev(inp.t), dev(inp.w3), inp.offsets.to(DEV)
    att, z = Guarded((T, heads)), Guarded((B, H))
    call("isic_attn_pool_wide_fwd", h, t, w3, dev(inp.b3), offsets, B, H, A, heads, max_bag, att.t, z.t)
    assert att.ok() and z.ok()
    got = dict(att=att.cpu(), z=z.cpu())
    keys = ("att", "z")
    if backward:                                           # (pad4(heads A) + pad4(H) + pad4(max_bag) + 8) floats: never above 48 KB
        d_h, d_u, d_s = Guarded((T, H)), Guarded((T, heads * A)), Guarded((T, heads))
        call("isic_attn_pool_wide_bwd", h, t, att.t, w3, offsets, B, H, A, heads, max_bag, dev(inp.dz), d_h.t, 0, d_u.t, d_s.t)
        assert d_h.ok() and d_u.ok() and d_s.ok()
        got.update(d_h=d_h.cpu(), d_u=d_u.cpu(), d_s=d_s.cpu())
        keys += ("d_h", "d_u", "d_s")
    check(f"attn_pool_wide_fwd A{A} max_bag {max_bag} {side(wide_lds(A, WIDE_HEADS, max_bag), where, POOL_BOUND)}",
          R.pool_ratios(got, ref, b, keys))


def wide_forward_refused(A, max_bag):
    inp, _, _ = pool_ref(WIDE_H, A, WIDE_HEADS, 0, WIDE_BAGS)
    att, z = Guarded((inp.T, WIDE_HEADS)), Guarded((inp.B, WIDE_H))
    assert code("isic_attn_pool_wide_fwd", dev(inp.h), dev(inp.t), dev(inp.w3), dev(inp.b3), inp.offsets.to(DEV), inp.B, WIDE_H, A,
                WIDE_HEADS, max_bag, att.t, z.t) == UNSUPPORTED
    assert untouched(att, z)
    print(f"attn_pool_wide_fwd A{A} max_bag {max_bag} refused", flush=True)


# ---------------------------------------------------------------- isic_knn_graph, the row-tile kernel
KNN_D, KNN_K = 24, 4


def knn_points(n):
    return torch.randn(n, KNN_D, generator=torch.Generator().manual_seed(1000 + n))


def knn_oracle(x):
    """-> (indices [n, k], distances [n, k], guarded [n, k]): position j is compared where the oracle's distances j - 1, j and
    j + 1 are more than KNN_GAP apart"""
    dv, di = torch.topk(graphs.pairwise_sqdist(x), KNN_K + 1, dim=1, largest=False)
    apart = dv[:, 1:] - dv[:, :-1] > KNN_GAP                                   # [n, k]: between positions j and j + 1
    before = torch.cat([torch.ones(x.shape[0], 1, dtype=torch.bool), apart[:, :-1]], dim=1)
    return di[:, :KNN_K], dv[:, :KNN_K], before & apart


def knn_args(x, n):
    idx = torch.full((n, KNN_K), -7, device=DEV, dtype=torch.int64)
    dist = Guarded((n, KNN_K))
    ws = torch.empty(n, device=DEV, dtype=torch.float32)
    offsets = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    return idx, dist, ("isic_knn_graph", dev(x), offsets, 1, KNN_D, KNN_K, n, n, idx, dist.t, ws)


def knn(n, where):
    x = knn_points(n)
    di, dv, guarded = knn_oracle(x)
    share = float(guarded.float().mean())
    assert share >= KNN_GUARDED_SHARE, (n, share)
    idx, dist, args = knn_args(x, n)
    call(*args)
    assert dist.ok()
    mine = idx.cpu()
    assert bool((mine[guarded] == di[guarded]).all()), (n, int((mine[guarded] != di[guarded]).sum()))
    assert_close(dist.cpu(), dv, rtol=1e-4, atol=1e-3, what="knn distances")
    print(f"knn_graph n {n} {side(knn_lds(n), where, KNN_BOUND)} guarded {share:.4f}", flush=True)


def knn_refused(n):
    side(knn_lds(n), "beyond", KNN_BOUND)
    idx, dist, args = knn_args(knn_points(n), n)
    assert code(*args) == UNSUPPORTED
    assert untouched(dist) and bool((idx == -7).all())
    print(f"knn_graph n {n} refused", flush=True)


def main():
    assert torch.cuda.is_available()
    # forward: the widest kernel walks small -> above -> top -> small; the two narrower kernels of the issue's list in between
    pool_forward(128, 129, 1, "small")
    pool_forward(1024, 129, 1, "small")
    pool_forward(512, 129, 4, "above")
    pool_forward(1024, 129, 2, "above")
    pool_forward(1024, 1536, 4, "top")
    pool_forward(128, 129, 1, "small")
    pool_forward(1024, 129, 1, "small")
    pool_forward_refused(1024, 2304, 4)
    pool_backward(1024, 64, 2, "small")
    pool_backward(1024, 64, 16, "above")
    pool_backward(1024, 23000, 16, "top")
    pool_backward(1024, 64, 2, "small")
    pool_backward_refused(1024, 24000, 16)
    pool_backward(128, 128, 16, "small", sums=True)
    wide_forward(64, 16, "small", backward=True)
    wide_forward(64, 2048, "above")
    wide_forward(512, 2048, "above")                        # the most the domain allows: 80 KB
    wide_forward(64, 16, "small")
    wide_forward_refused(64, 2049)
    knn(100, "small")
    knn(800, "above")
    knn(2300, "top")
    knn(100, "small")
    knn_refused(2500)
    print("LAUNCH_LDS_OK", flush=True)


if __name__ == "__main__":
    main()
