"""``isic_class_metrics_f32`` (csrc/metrics.hip) through the C ABI and ``isic_hip.metrics.class_counts`` on the MI355X, held
to the restatement of tests/metrics_ref.py bit for bit: every integer the device writes equals the literal O(n^2) count
(tests/test_metrics_ref_cpu.py shows that each wrong variant kept there changes such an integer on some case).

The outputs of the C entry are prefilled with a sentinel and sit between guard areas.  ``loss_sum`` is a sum of n fp64
conversions of fp32 values in a fixed order: within n 2^-52 sum|l_i| of ``numpy.sum`` in fp64."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import metrics_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 32
SENTINEL = -7777
BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
_CACHE = {}


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a device error (not a failed comparison) ends the session: nothing more is launched on a GPU that has faulted"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further GPU work: {e}", returncode=3)


def case_counts(case):
    if case not in _CACHE:
        s, y = R.make_case(*case)
        conf, pair2, flags = R.counts(s, y, case[2])
        for a in (s, y, conf, pair2, flags):
            a.setflags(write=False)
        _CACHE[case] = (s, y, conf, pair2, flags)
    return _CACHE[case]


class Out:
    """guard | confusion | guard | pair2 | guard | flags | guard | loss_sum | guard, int64 words, sentinel everywhere"""

    def __init__(self, C):
        self.C = C
        self.sizes = (C * C, C, 2, 1)
        self.starts, at = [], GUARD
        for k in self.sizes:
            self.starts.append(at)
            at += k + GUARD
        self.buf = torch.full((at,), SENTINEL, device=DEV, dtype=torch.int64)

    def ptr(self, k):
        return self.buf.data_ptr() + 8 * self.starts[k]

    def read(self):
        """-> confusion, pair2, flags, loss_sum (fp64), after checking the guards"""
        h = self.buf.cpu().numpy()
        mask = np.ones(len(h), dtype=bool)
        for a, k in zip(self.starts, self.sizes):
            mask[a:a + k] = False
        assert (h[mask] == SENTINEL).all(), "guard area overwritten"
        parts = [h[a:a + k].copy() for a, k in zip(self.starts, self.sizes)]
        return parts[0].reshape(self.C, self.C), parts[1], parts[2], float(parts[3].view(np.float64)[0])


def entry(scores, labels, loss, n, C, out=None, ws_bytes=None, ws=None):
    """one call of the C entry on device tensors (None -> NULL) -> (return code, Out)"""
    from isic_hip.lib import IsicHipError, call
    out = out or Out(C)
    need = int(call("isic_class_metrics_f32_workspace_bytes", n, C))
    if ws is None:
        ws = torch.empty(max(need, 16), device=DEV, dtype=torch.uint8)
    try:
        call("isic_class_metrics_f32", scores, labels, loss, n, C, out.ptr(0), out.ptr(1), out.ptr(2), out.ptr(3),
             ws if need else None, need if ws_bytes is None else ws_bytes)
    except IsicHipError as e:
        return e.code, out
    return 0, out


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)         # (a copy: the shared cases are read-only)


@pytest.mark.parametrize("family,n,C", R.CASES)
def test_counts_equal_the_restatement(family, n, C):
    s, y, conf, pair2, flags = case_counts((family, n, C))
    loss = R.make_loss(n)
    sd, yd, ld = dev(s), dev(y), dev(loss)
    rc, out = entry(sd, yd, ld, n, C)
    assert rc == 0
    got = out.read()
    assert np.array_equal(got[0], conf), "confusion"
    assert np.array_equal(got[1], pair2), ("pair2", got[1], pair2)
    assert np.array_equal(got[2], flags)
    l64 = loss.astype(np.float64)
    assert abs(got[3] - l64.sum()) <= n * 2.0 ** -52 * np.abs(l64).sum()
    rc, out2 = entry(sd, yd, ld, n, C)                               # a second call: identical bits
    assert rc == 0 and torch.equal(out.buf, out2.buf)
    rc, out3 = entry(sd, yd, None, n, C)                             # no loss: the counts are the same, the sum is 0.0
    got3 = out3.read()
    assert rc == 0 and np.array_equal(got3[0], conf) and np.array_equal(got3[1], pair2) and got3[3] == 0.0


@pytest.mark.parametrize("kind", R.BIG_KINDS)
def test_totals_beyond_32_bits(kind):
    s, y, conf, pair2 = R.big_case(kind)
    assert pair2.max() > 2 ** 31
    rc, out = entry(dev(s), dev(y), None, R.BIG_N, 2)
    assert rc == 0
    got = out.read()
    print("pair2", got[1].tolist(), "expected", pair2.tolist())
    assert np.array_equal(got[0], conf) and np.array_equal(got[1], pair2) and got[2].tolist() == [0, 0]


def test_flags_and_class_counts():
    from isic_hip.metrics import ClassMetrics, class_counts
    n, C = R.BLOCK + 40, 7
    s, y = R.make_case("softmax", n, C)
    s, y = s.copy(), y.copy()
    loss = R.make_loss(n)
    cm = class_counts(dev(s), dev(y), dev(loss))                     # clean input: the public call
    conf, pair2, _ = R.counts(s, y, C)
    assert isinstance(cm, ClassMetrics) and np.array_equal(cm.confusion, conf) and np.array_equal(cm.pair2, pair2)
    assert abs(cm.loss - loss.astype(np.float64).mean()) <= n * 2.0 ** -52 * float(np.abs(loss).mean()) + 1e-300
    ref = R.floats(conf, pair2)
    for k in R.FLOAT_KEYS:
        assert abs(getattr(cm, k) - ref[k]) <= 1e-15 or (np.isnan(getattr(cm, k)) and np.isnan(ref[k])), k
    # one NaN, one +inf, one label equal to C (three different samples, one of them past the first block)
    s[3, 2], s[R.BLOCK + 9, 0], y[17] = np.nan, np.inf, C
    conf, pair2, flags = R.counts(s, y, C)
    assert flags.tolist() == [2, 1] and conf.sum() == n - 3
    rc, out = entry(dev(s), dev(y), dev(loss), n, C)
    got = out.read()
    assert rc == 0 and got[2].tolist() == [2, 1]
    assert np.array_equal(got[0], conf) and np.array_equal(got[1], pair2)     # those samples appear in no count
    keep = R.counted(s, y, C)
    l64 = loss.astype(np.float64)[keep]
    assert abs(got[3] - l64.sum()) <= n * 2.0 ** -52 * np.abs(l64).sum()
    with pytest.raises(ValueError, match="NaN or infinity"):
        class_counts(dev(s), dev(y))
    s2 = R.make_case("softmax", n, C)[0]
    with pytest.raises(ValueError, match="outside the range"):
        class_counts(dev(s2), dev(y))
    from isic_hip.lib import IsicHipError
    with pytest.raises(IsicHipError):
        class_counts(torch.from_numpy(s2), torch.from_numpy(y))


def test_domain_errors_and_empty_input():
    n, C = 40, 7
    s, y = R.make_case("softmax", n, C)
    sd, yd = dev(s), dev(y)
    from isic_hip.lib import call
    for bad_c in (1, 17):
        wide = torch.zeros((n, 17), device=DEV)
        rc, out = entry(wide, yd, None, n, bad_c, out=Out(17))
        assert rc == UNSUPPORTED and (out.buf == SENTINEL).all()
        assert int(call("isic_class_metrics_f32_workspace_bytes", n, bad_c)) == 0
    rc, out = entry(sd, yd, None, 2 ** 31, C, ws=torch.empty(16, device=DEV, dtype=torch.uint8), ws_bytes=16)
    assert rc == UNSUPPORTED and (out.buf == SENTINEL).all()
    need = int(call("isic_class_metrics_f32_workspace_bytes", n, C))
    assert need > 0
    rc, out = entry(sd, yd, None, n, C, ws_bytes=need - 1)
    assert rc == WORKSPACE and (out.buf == SENTINEL).all()
    ws = torch.empty(need + 16, device=DEV, dtype=torch.uint8)
    rc, out = entry(sd, yd, None, n, C, ws=ws[8:], ws_bytes=need)     # not 16-byte aligned
    assert rc == WORKSPACE and (out.buf == SENTINEL).all()
    rc, out = entry(sd, yd, None, -1, C)
    assert rc == BAD_ARG
    rc, out = entry(None, yd, None, n, C)
    assert rc == BAD_ARG and (out.buf == SENTINEL).all()
    rc, out = entry(None, None, None, 0, C)                           # n == 0 writes zeros
    got = out.read()
    assert rc == 0 and not got[0].any() and not got[1].any() and not got[2].any() and got[3] == 0.0


def test_captured_launch_replays_on_new_scores():
    """one plain capture of the entry (no parallel branches); the score buffer is overwritten in place between replays"""
    from isic_hip.metrics import class_counts_record
    n, C = R.TILE + 1, 7
    s1, y, conf1, pair1, _ = case_counts(("softmax", n, C))
    s2 = case_counts(("quant2", n, C))[0]                             # other scores under the same labels
    conf2, pair2, _ = R.counts(s2, y, C)
    assert not np.array_equal(pair1, pair2)
    loss = R.make_loss(n)
    sd, yd, ld = dev(s1), dev(y), dev(loss)
    from isic_hip.lib import call
    out = torch.full((C * C + C + 3,), SENTINEL, device=DEV, dtype=torch.int64)
    ws = torch.empty(int(call("isic_class_metrics_f32_workspace_bytes", n, C)), device=DEV, dtype=torch.uint8)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        class_counts_record(sd, yd, ld, out=out, workspace=ws)        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        class_counts_record(sd, yd, ld, out=out, workspace=ws)
    for s_new, conf, pair in ((None, conf1, pair1), (s2, conf2, pair2)):
        if s_new is not None:
            sd.copy_(dev(s_new))
        out.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        h = out.cpu().numpy()
        assert np.array_equal(h[:C * C].reshape(C, C), conf) and np.array_equal(h[C * C:C * C + C], pair)
        assert h[C * C + C:C * C + C + 2].tolist() == [0, 0]
