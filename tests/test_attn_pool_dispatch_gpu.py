"""Which C entries one forward + backward of attention pooling launches, in order: ``ops.attn_pool`` (ungated, gated with
separate gate tensors, gated over the stacked operands of ``ops.head_params``, the teacher form, under
``ops.fused_grad_accumulation``) and ``torch.ops.isic_hip.attn_pool``, over the shapes at which the choice of pool entry
changes (H <= 128 / H > 128 / H > 1024, heads <= 4 / heads = 8).  The lists are literals: a refactor of the Python above the
C ABI keeps the same entries in the same order, hence the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS, A, C = [0, 1, 5, 40], 8, 3

GEMM, COLSUM, COPY = "gemm_f32_ws", "colsum_f32_ws", "multi_copy_f32"
UNGATED_FWD = [GEMM]                                   # t = tanh(h W2^T + b2): one GEMM with the tanh epilogue
GATED_FWD = [GEMM, "gate_fwd_f32"]                     # [W2 ; Wg] in one GEMM, then the gate
SUMS_BWD = ["attn_pool_bwd_sums", COLSUM]              # db2 | dw3 | db3 out of per-bag sums: one column sum
PLAIN_BWD = [COLSUM, GEMM, COLSUM]                     # db2, dw3, db3 out of d_u / d_s (after the pool backward)
TAIL = [GEMM, GEMM]                                    # dW2 = d_u^T h, d_h += d_u W2
TEACHER_TAIL = [GEMM, COLSUM]                          # dW4 = d_P^T h, db4

#             H, heads, pool forward, pool backward
SHAPES = {
    "small1": (32, 1, "attn_pool_fwd", "attn_pool_bwd"),
    "small4": (32, 4, "attn_pool_fwd", "attn_pool_bwd"),
    "narrow-big": (129, 2, "attn_pool_fwd", "attn_pool_bwd"),
    "heads8": (64, 8, "attn_pool_fwd", "attn_pool_wide_bwd"),
    "wide": (1028, 2, "attn_pool_wide_fwd", "attn_pool_wide_bwd"),
}


def _ungated(shape, teacher=False):
    H, _heads, fwd, bwd = SHAPES[shape]
    back = SUMS_BWD if H <= 128 and bwd == "attn_pool_bwd" else [bwd] + PLAIN_BWD
    return UNGATED_FWD + [fwd], back + TAIL + (TEACHER_TAIL if teacher else [])


def _gated(shape, stacked, teacher=False):
    _H, heads, fwd, bwd = SHAPES[shape]
    # stacked: the packer's gather (32 tensors per launch, six per head), one weight GEMM over [W2 ; Wg];
    # separate: one launch stacks the four tensors, one weight GEMM per half
    front = [COPY] * ((6 * heads + 31) // 32) if stacked else [COPY]
    return (front + GATED_FWD + [fwd],
            [bwd, "gate_bwd_f32"] + ([GEMM] if stacked else [GEMM, GEMM]) + [GEMM] + (TEACHER_TAIL if teacher else []))


@pytest.fixture
def served(monkeypatch):
    """The names of the C entries that returned, in call order (without the ``isic_`` prefix and the workspace queries)."""
    from isic_hip import ops, torch_ops
    names = []
    real_call = ops.call

    def spy(name, *a, **kw):
        rc = real_call(name, *a, **kw)
        if not name.endswith("_workspace_bytes"):
            names.append(name[len("isic_"):])
        return rc
    monkeypatch.setattr(ops, "call", spy)
    monkeypatch.setattr(torch_ops, "call", spy)
    return names


def _leaf(*shape, gen, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV).requires_grad_(True)


def _operands(H, heads, gen, teacher=False, gate=False):
    from isic_hip.bags import BagOffsets
    offs = BagOffsets.from_lengths(LENGTHS, torch.device(DEV))
    p = dict(h=_leaf(offs.total, H, gen=gen), W2=_leaf(heads * A, H, gen=gen, scale=0.1), b2=_leaf(heads * A, gen=gen, scale=0.1),
             w3=_leaf(heads, A, gen=gen, scale=0.3), b3=_leaf(heads, gen=gen, scale=0.1))
    if gate:
        p.update(Wg=_leaf(heads * A, H, gen=gen, scale=0.1), bg=_leaf(heads * A, gen=gen, scale=0.1))
    if teacher:
        p.update(W4=_leaf(C, H, gen=gen, scale=0.1), b4=_leaf(C, gen=gen, scale=0.1))
    return offs, p


def _run(served, offs, p, heads):
    """One forward + backward of ``ops.attn_pool`` -> (entries of the forward, entries of the backward)."""
    from isic_hip import ops
    gen = torch.Generator().manual_seed(9)
    h = p.pop("h")
    del served[:]
    out = ops.attn_pool(h, p.pop("W2"), p.pop("b2"), p.pop("w3"), p.pop("b3"), offs.device, offs.max_bag, heads=heads, **p)
    fwd = list(served)
    del served[:]
    outs = [out[0]] + ([out[4]] if "W4" in p else [])                          # z (, bag logits)
    torch.autograd.backward(outs, [torch.randn(o.shape, generator=gen).to(DEV) for o in outs])
    torch.cuda.synchronize()
    return fwd, list(served)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_ungated(served, shape):
    H, heads = SHAPES[shape][:2]
    offs, p = _operands(H, heads, torch.Generator().manual_seed(1))
    assert _run(served, offs, p, heads) == _ungated(shape)


@pytest.mark.parametrize("shape", ["small1", "small4", "narrow-big", "wide"])
def test_gated_separate_tensors(served, shape):
    H, heads = SHAPES[shape][:2]
    offs, p = _operands(H, heads, torch.Generator().manual_seed(2), gate=True)
    got = _run(served, offs, p, heads)
    assert got == _gated(shape, stacked=False)
    assert "attn_pool_bwd_sums" not in got[1]


@pytest.mark.parametrize("gate", [False, True])
def test_teacher(served, gate):
    offs, p = _operands(32, 1, torch.Generator().manual_seed(3), teacher=True, gate=gate)
    want = _gated("small1", stacked=False, teacher=True) if gate else _ungated("small1", teacher=True)
    assert _run(served, offs, p, 1) == want


def _heads(H, heads, gated):
    torch.manual_seed(4)
    nn = torch.nn
    layers = nn.ModuleList(nn.Sequential(nn.Linear(H, A), nn.Tanh(), nn.Linear(A, 1)) for _ in range(heads)).to(DEV)
    gates = nn.ModuleList(nn.Sequential(nn.Linear(H, A), nn.Sigmoid()) for _ in range(heads)).to(DEV) if gated else None
    return layers, gates


@pytest.mark.parametrize("shape", ["small1", "small4", "heads8"])
def test_gated_stacked_by_head_params(served, shape):
    from isic_hip import ops
    H, heads = SHAPES[shape][:2]
    offs, p = _operands(H, heads, torch.Generator().manual_seed(5))
    layers, gates = _heads(H, heads, gated=True)
    del served[:]
    W2, b2, w3, b3, Wg, bg = ops.head_params(layers, gates)
    packed = list(served)
    fwd, bwd = _run(served, offs, dict(h=p["h"], W2=W2, b2=b2, w3=w3, b3=b3, Wg=Wg, bg=bg), heads)
    # without fused_grad_accumulation the packer's backward hands the slices to autograd: no launch of its own
    assert (packed + fwd, bwd) == _gated(shape, stacked=True)
    assert all(g[0].weight.grad is not None for g in gates)


@pytest.mark.parametrize("gate", [False, True])
def test_teacher_under_fused_grad_accumulation(served, gate):
    """The parameters live in the optimizer's flat buffer: their gradients are added into it by the producing launches."""
    from isic_hip import ops, optim
    offs, p = _operands(32, 1, torch.Generator().manual_seed(6), teacher=True, gate=gate)
    h = p.pop("h")
    p = {k: torch.nn.Parameter(v.detach()) for k, v in p.items()}
    opt = optim.AdamW(list(p.values()), lr=1e-3)
    opt.zero_grad()
    with ops.fused_grad_accumulation():
        fwd, bwd = _run(served, offs, dict(h=h, **p), 1)
    if gate:
        # db2, dw3, db3, dbg in ONE accumulating copy launch; dW2 and dWg as two GEMMs with beta = 1
        want = (_gated("small1", stacked=False, teacher=True)[0],
                ["attn_pool_bwd", "gate_bwd_f32", COPY, GEMM, GEMM, GEMM] + TEACHER_TAIL)
    else:
        # db2, dw3, db3 live in three places of the flat buffer: one column sum over each slice of the per-bag sums
        want = _ungated("small1", teacher=True)[0], ["attn_pool_bwd_sums", COLSUM, COLSUM, COLSUM] + TAIL + TEACHER_TAIL
    assert (fwd, bwd) == want
    assert float(opt.flat.grad.abs().max()) > 0 and all(float(q.grad.abs().max()) > 0 for q in p.values())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_torch_op_launches_what_the_function_launches(served, shape):
    from isic_hip import torch_ops  # noqa: F401  (registers the ops)
    H, heads = SHAPES[shape][:2]
    offs, p = _operands(H, heads, torch.Generator().manual_seed(7))
    want = _run(served, offs, dict(p), heads)
    assert want == _ungated(shape)
    del served[:]
    z, _att, _t = torch.ops.isic_hip.attn_pool(p["h"], p["W2"], p["b2"], p["w3"], p["b3"], offs.device, offs.max_bag, heads)
    fwd = list(served)
    del served[:]
    z.backward(torch.randn(z.shape, generator=torch.Generator().manual_seed(9)).to(DEV))
    torch.cuda.synchronize()
    assert (fwd, list(served)) == want
