"""tests/acq_ref.py held to the project's eager selection chain (CPU).

The GPU tests (tests/test_acq_select_gpu.py) compare the fused epilogue
and its host decode with the numpy contract exactly; here the contract is
compared with what it stands for - torch.where, max(0), torch.isclose(...,
rtol=1e-8) & active, and pair_acq.tied_choice under the same random.seed -
on every generated case, and the generators are held to the conditions
that make the exact comparison legitimate and able to fail:

  - no case has an entry within 2 fp32 ulps of a threshold that an fma
    contraction could move (acq_ref's docstring says which entries that
    excludes and why);
  - the small-|best| ladders (h0 = 0) contain ties that are unequal to
    the maximum and rungs that are not ties. Rebuilt with h0 = 0.731 the
    sums lie on a 2^-24 grid, six times the threshold, so there only
    equal values can tie: those ladders must still contain non-ties, and
    rungs that collapsed onto the maximum;
  - each of four mutations of the contract changes the expected output of
    at least one case.
"""
from __future__ import annotations

import random

import numpy as np
import pytest
import torch

from coda_amd.selectors.pair_acq import tied_choice
from tests import acq_ref as AR

EVERY_CASE = (AR.all_cases() + AR.state_cases() + AR.graph_cases()
              + tuple(AR.decode_cases().values()))


def eager_chain(case):
    q0 = torch.from_numpy(case.q0)
    h0 = torch.tensor([float(case.h0)], dtype=torch.float32)
    active = torch.from_numpy(case.active)
    q = torch.where(active, h0 + q0, torch.full_like(q0, float("-inf")))
    bv, bi = q.max(0)
    ties = torch.isclose(q, bv, rtol=1e-8) & active
    return q, bv, int(bi), ties, active


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("case", EVERY_CASE, ids=lambda c: c.name)
def test_reference_is_the_eager_chain(case):
    ref = AR.ref_of(case)
    q, bv, bi, ties, active = eager_chain(case)
    assert np.array_equal(bits(q.numpy()), bits(ref.qbuf))
    assert bits(bv.numpy()) == bits(ref.best)
    if case.active.any() and ref.best > -np.inf:
        # (at -inf torch's argmax may sit on a masked entry: the eager
        # path's own business, it goes through the ties below)
        assert bi == ref.first
    else:
        assert ref.first == (-1 if not case.active.any()
                             else int(np.flatnonzero(case.active)[0]))
    assert torch.nonzero(ties, as_tuple=True)[0].tolist() \
        == ref.ties.tolist()
    assert (ref.ties.size == 0) == (not case.active.any())
    # packed words: position high, the entry's own fp32 bits low
    assert (ref.packed >> 32).tolist() == ref.ties.tolist()
    assert np.array_equal((ref.packed & 0xFFFFFFFF).astype(np.uint32),
                          ref.qbuf[ref.ties].view(np.uint32))
    assert (ref.packed >= 0).all()
    if ref.ties.size:
        for seed in (0, 1, 12345):
            random.seed(seed)
            want = tied_choice(q, bv, active)
            random.seed(seed)
            assert random.choice(ref.ties.tolist()) == want
            if ref.ties.size > 1:
                assert AR.pick(ref, seed) == (want, float(q[want]), True)
            else:
                assert AR.pick(ref, seed) == (bi, float(bv), False)
    else:
        with pytest.raises(LookupError):
            AR.pick(ref, 0)


@pytest.mark.parametrize("case", EVERY_CASE, ids=lambda c: c.name)
def test_no_case_is_ambiguous(case):
    assert AR.ref_of(case).ambiguous == 0


def test_ambiguity_counter_counts():
    """The counter is not vacuous: an entry one ulp of the threshold away
    from it is counted, and one at the contraction-proof threshold of
    best = 0 is not."""
    both = np.ones(2, dtype=bool)
    qq = np.array([0.0, -float(AR.ATOL)], dtype=np.float32)
    r = AR.select(qq, both)
    assert r.ambiguous == 0 and r.ties.tolist() == [0, 1]
    # a maximum small enough for fp32 to resolve the threshold's ulps,
    # with an inexact product: the entry at best - thr is counted
    b = np.float32(1.5 * 2.0 ** -40)
    t = AR.threshold(b)
    qq = np.array([b, np.float64(b) - np.float64(t)], dtype=np.float32)
    assert abs(abs(float(qq[1]) - float(b)) - float(t)) \
        <= 2 * float(np.spacing(t))
    assert AR.select(qq, both).ambiguous == 1
    # and an inactive one is not
    assert AR.select(qq, np.array([True, False])).ambiguous == 0


def test_generators_cover_what_they_claim():
    names = {c.name for c in AR.all_cases()}
    for B in AR.SHAPES:
        assert f"at-0-B{B}" in names
    assert AR.per_block(65_537) == 257 and AR.per_block(200_000) == 782
    for B in (65_537, 200_000):
        assert f"dup-one-thread-B{B}" in names
    assert "dup-one-thread-B65536" not in names
    by = {c.name: c for c in AR.all_cases()}
    # duplicates: the first active one wins, the masked one is not counted
    for B in AR.SHAPES[2:]:
        c = by[f"dup-first-inactive-B{B}"]
        r = AR.ref_of(c)
        dup = np.flatnonzero(c.q0 == c.q0.max())
        assert dup.size == 3 and not c.active[dup[0]]
        assert r.first == dup[1] and r.ties.tolist() == dup[1:].tolist()
    # tie counts land where they were aimed, around every cap
    for cap in AR.CAPS:
        for n in (cap, cap + 1, 1000):
            assert AR.ref_of(by[f"ties{n}-cap{cap}-B1000"]).ties.size == n
    # sign bits in the packed low word, positions >= 2^15 in the high one
    refs = [AR.ref_of(c) for c in AR.all_cases()]
    assert any(r.ties.size > 1 and r.best < 0 for r in refs)
    assert any(r.ties.size > 1 and r.ties.max() >= 2 ** 15 for r in refs)
    # inactive entries hold the global maximum
    c = by["random-active-B10000"]
    assert c.q0.max() == 50.0 and AR.ref_of(c).best < 10.0
    # infinities
    assert AR.ref_of(by["one-inf-B1000"]).ties.size == 1
    assert AR.ref_of(by["two-inf-B65537"]).ties.size == 2
    c = by["all-neg-inf-B1000"]
    r = AR.ref_of(c)
    assert r.best == -np.inf and not c.active[0] and r.first > 0
    assert r.ties.tolist() == np.flatnonzero(c.active).tolist()
    # the decode cases straddle the packed / rescan boundary
    dec = AR.decode_cases()
    assert AR.ref_of(dec["packed-8191"]).ties.size == AR.DECODE_CAP
    assert AR.ref_of(dec["rescan-8192"]).ties.size == AR.DECODE_CAP + 1
    near = AR.ref_of(dec["near"])
    assert near.ties.size == 401
    assert np.unique(near.qbuf[near.ties]).size > 100


def test_ladders_contain_what_they_must():
    by = {c.name: c for c in AR.ladder_cases()}
    assert len(by) == 2 * (len(AR.LADDER_BESTS) + 1)
    for best in AR.LADDER_BESTS + (AR.RTOL_BEST,):
        for h0 in (0.0, 0.731):
            c = by[f"ladder-best{best:g}-h{h0:g}"]
            r = AR.ref_of(c)
            rungs = np.array(c.rungs)
            tied = np.isin(rungs, r.ties)
            unequal = r.qbuf[rungs] != r.best
            assert (~tied).any(), c.name            # non-close members
            assert (tied & ~unequal).any(), c.name
            small = best in AR.SMALL_BESTS or best == AR.RTOL_BEST
            if h0 == 0.0:
                assert r.best == np.float32(best)
            if h0 == 0.0 and small:
                # close-and-unequal members: atol decides here
                assert (tied & unequal).sum() >= 2, c.name
            else:
                # one ulp of the maximum is already past the threshold
                assert not (tied & unequal).any(), c.name
            # the masked copy of a close rung is never counted
            assert not c.active[-1] and (c.B - 1) not in r.ties.tolist()
            if best < 0:
                assert (r.packed & 0x80000000).all()


@pytest.mark.parametrize("mutation", AR.MUTATIONS)
def test_each_mutation_changes_some_case(mutation):
    """Floors: a kernel wrong in one of these four ways cannot pass the
    GPU tests, because the cases' expected outputs tell the mutated
    contract from the real one."""
    hit = []
    for c in AR.all_cases():
        r = AR.ref_of(c)
        m = AR.reference(c.q0, c.h0, c.active, mutate=mutation)
        if (m.first != r.first or m.ties.tolist() != r.ties.tolist()
                or bits(m.best) != bits(r.best)):
            hit.append(c.name)
    print(mutation, "changes", len(hit), "cases:", hit[:6])
    assert hit, mutation
