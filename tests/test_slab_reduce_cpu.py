"""tests/slab_reduce_ref.py on the CPU: the five orders are sums, they are really five different orders on the inputs the
device test uses (so a device that added in another order would be caught bit for bit), and they coincide where they
must."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import slab_reduce_ref as R  # noqa: E402

EPS = float(np.finfo(np.float32).eps)


def _cases(form):
    return [(s, n) for s in R.SLABS for n in R.n_values(form)]


@pytest.mark.parametrize("form", R.FORMS)
def test_each_form_is_a_sum(form):
    """every add rounds once: |result - exact| <= (adds per element) * eps/2 * sum |x|, with slabs adds at the very most"""
    for slabs, n in _cases(form):
        partial, _ = R.case(slabs, n)
        got = R.expected(form, slabs, n)
        assert got.dtype == np.float32 and got.shape == (n,)
        exact = partial.astype(np.float64).sum(axis=0)
        bound = (slabs + 20) * 0.5 * EPS * np.abs(partial.astype(np.float64)).sum(axis=0)
        assert np.all(np.abs(got.astype(np.float64) - exact) <= bound), (form, slabs, n)


def test_forms_agree_up_to_two_slabs():
    """one slab: the slab itself (0 + x); two slabs: x0 + x1 in every order (lanes / groups 0 and 1, joined first)"""
    for slabs in (1, 2):
        for n in R.N_SCALAR:
            partial, _ = R.case(slabs, n)
            want = R.bits(R.sequential(partial))
            for form in R.FORMS:
                if n in R.n_values(form):
                    assert np.array_equal(R.bits(R.expected(form, slabs, n)), want), (form, slabs, n)


def test_forms_are_pairwise_different_orders_from_64_slabs():
    """n = 148, slabs >= 64: every two of the five forms, and each form against the index-order walk, differ somewhere"""
    for slabs in (s for s in R.SLABS if s >= 64):
        partial, _ = R.case(slabs, 148)
        sums = {form: R.bits(R.expected(form, slabs, 148)) for form in R.FORMS}
        sums["sequential"] = R.bits(R.sequential(partial))
        for a, b in itertools.combinations(sums, 2):
            differing = int(np.count_nonzero(sums[a] != sums[b]))
            print(f"slabs {slabs}: forms {a} / {b} differ in {differing} of 148")
            assert differing >= 1, (slabs, a, b)


def test_lds_join_from_zero_or_from_group_zero_is_the_same_sum():
    """a group sum starts from +0, so it is never -0 and `0 + p_0` is p_0: the kernels that start the join from 0 and those
    that start it from group 0's sum share one function (shown on the cases, and on slabs of -0 where it could differ)"""
    for form in (2, 3, 4):
        for slabs, n in _cases(form):
            partial, _ = R.case(slabs, n)
            assert np.array_equal(R.bits(R.slab_sum(form, partial, from_zero=True)), R.bits(R.slab_sum(form, partial, from_zero=False)))
        neg0 = np.full((33, 4), -0.0, np.float32)
        for fz in (True, False):
            assert np.array_equal(R.bits(R.slab_sum(form, neg0, from_zero=fz)), np.zeros(4, np.uint32))


def test_epilogue_and_inputs():
    partial, prior = R.case(17, 37)
    s = R.expected(0, 17, 37)
    assert np.array_equal(R.bits(R.epilogue(s, prior, 0.0)), R.bits(s))
    assert np.array_equal(R.bits(R.epilogue(s, prior, 1.0)), R.bits(prior + s))
    with pytest.raises(AssertionError):
        R.epilogue(s, prior, 0.5)
    # the inputs span 2^-6 .. 2^6 in scale, are fixed, and cannot be written to
    again = R.case.__wrapped__(17, 37)[0]
    assert np.array_equal(R.bits(again), R.bits(partial)) and not partial.flags.writeable
    mags = np.abs(R.case(257, 148)[0])
    assert mags.max() > 64.0 and np.median(mags) < 1.0
