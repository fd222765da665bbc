"""The fused acquisition epilogue and its host decode, exactly (GPU).

ops/hip/pair.hip acq_select and selectors/pair_acq.py
PairAcquisition.result() against the numpy contract of tests/acq_ref.py,
which tests/test_acq_select.py holds to the eager torch chain on the CPU.
No generated case has an entry near enough to the isclose threshold for a
contracted threshold to decide it differently (asserted there), so every
comparison here is bitwise or set-equal: there is no tolerance in this
file.
"""
from __future__ import annotations

import random
import types

import numpy as np
import pytest
import torch

from tests import acq_ref as AR

pytestmark = pytest.mark.gpu

SENTINEL = -0x5A5A5A5A5A5A5A5B
TAIL = 64            # sentinel words behind the tie buffer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext():
    import coda_amd.ops as ops
    assert ops.hip_available(), \
        "HIP extension must be built on GPU boxes (python build_hip.py)"
    return ops._ext


@pytest.fixture()
def production(monkeypatch):
    """Guards off: they synchronize per op and keep the graphs out."""
    import coda_amd.selectors.coda as coda_mod
    import coda_amd.ops as ops_mod
    import coda_amd.util as util_mod
    monkeypatch.setattr(coda_mod, "DEBUG", False)
    monkeypatch.setattr(ops_mod, "DEBUG", False)
    monkeypatch.setattr(util_mod, "DEBUG", False)
    return monkeypatch


class Buffers:
    """Device inputs and outputs of one acq_select call. The tie buffer is
    the contiguous prefix big[:cap + 1] of a sentinel-filled allocation."""

    def __init__(self, B: int, cap: int, dev):
        self.cap = cap
        self.q0 = torch.zeros(B, device=dev)
        self.h0 = torch.zeros(1, device=dev)
        self.active = torch.zeros(B, dtype=torch.bool, device=dev)
        # NaN-filled: an entry the kernel skipped cannot pass for written
        self.qbuf = torch.full((B,), float("nan"), device=dev)
        self.out = torch.full((3,), float("nan"), dtype=torch.float64,
                              device=dev)
        self.big = torch.full((cap + 1 + TAIL,), SENTINEL,
                              dtype=torch.int64, device=dev)
        self.ties = self.big[:cap + 1]
        assert self.ties.is_contiguous()

    def load(self, case):
        assert case.B == self.q0.numel()
        self.q0.copy_(torch.from_numpy(case.q0))
        self.h0.copy_(torch.from_numpy(np.array([case.h0], np.float32)))
        self.active.copy_(torch.from_numpy(case.active))

    def run(self, ext):
        ext.acq_select(self.q0, self.h0, self.active, self.qbuf, self.out,
                       self.ties)

    def fetch(self):
        """(qbuf bits, out, counter, set of the filled slots)"""
        big = self.big.cpu()
        assert (big[self.cap + 1:] == SENTINEL).all(), \
            "wrote behind the tie buffer"
        out = self.out.cpu().tolist()
        n = int(big[0])
        slots = big[1:1 + min(n, self.cap)].tolist()
        return (self.qbuf.cpu().numpy().view(np.int32), out, n, slots)


def check(got, ref: AR.Ref, cap: int, name: str):
    qbits, out, n, slots = got
    assert np.array_equal(qbits, ref.qbuf.view(np.int32)), name
    # out[0] is the fp32 maximum widened to fp64: equal means bit-equal
    # here (no generated maximum is a zero of either sign but +0)
    assert out[0] == float(ref.best), (name, out)
    assert out[1] == ref.first, (name, out)
    assert out[2] == ref.ties.size, (name, out)
    assert n == ref.ties.size, (name, n)
    want = set(ref.packed.tolist())
    assert len(slots) == len(set(slots)), name
    if n <= cap:
        assert set(slots) == want, name
    else:
        assert len(slots) == cap and set(slots) <= want, name


@pytest.mark.parametrize("case", AR.all_cases(), ids=lambda c: c.name)
def test_kernel_against_contract(ext, dev, case):
    buf = Buffers(case.B, case.cap, dev)
    buf.load(case)
    buf.run(ext)
    first = buf.fetch()
    check(first, AR.ref_of(case), case.cap, case.name)
    buf.run(ext)
    again = buf.fetch()
    assert np.array_equal(first[0], again[0])
    assert first[1] == again[1] and first[2] == again[2]
    if first[2] <= case.cap:
        assert set(first[3]) == set(again[3])
    else:       # which cap members make it into the slots is a race
        check(again, AR.ref_of(case), case.cap, case.name)


def test_state_across_calls(ext, dev):
    """Many ties, then one, then three through ONE set of buffers: the
    counter is reset each call and the slots the first call filled do not
    leak into the later results."""
    cases = AR.state_cases()
    assert [AR.ref_of(c).ties.size for c in cases] == [400, 1, 3]
    buf = Buffers(cases[0].B, 511, dev)
    for c in cases:
        buf.load(c)
        buf.run(ext)
        check(buf.fetch(), AR.ref_of(c), 511, c.name)
    # and with the buffer overflowed first
    buf = Buffers(cases[0].B, 7, dev)
    for c in cases:
        buf.load(c)
        buf.run(ext)
        check(buf.fetch(), AR.ref_of(c), 7, c.name)


def test_under_a_graph(ext, dev):
    """One captured call on static buffers, inputs rewritten in place
    between replays."""
    from coda_amd.selectors.coda import _warm_and_capture
    cases = AR.graph_cases()
    buf = Buffers(cases[0].B, 511, dev)
    buf.load(cases[0])
    graph, first = _warm_and_capture(lambda: buf.run(ext), buf.fetch)
    # the warm-up ran the body for real on the first input
    check(first, AR.ref_of(cases[0]), 511, cases[0].name)
    for c in cases[1:] + cases[:1]:
        buf.load(c)
        graph.replay()
        torch.cuda.synchronize()
        check(buf.fetch(), AR.ref_of(c), 511, c.name)


# ---------------------------------------------------------------------
# host decode
# ---------------------------------------------------------------------

def _acquisition(case, dev):
    """A PairAcquisition around a stand-in structure (__init__ reads only
    ps.cand_ids) whose point ids differ from the positions."""
    from coda_amd.selectors.pair_acq import PairAcquisition
    B = case.B
    ids = (3 * torch.arange(B) + 11).to(dev)
    ps = types.SimpleNamespace(cand_ids=ids)
    acq = PairAcquisition(ps, None, ids, torch.arange(B, device=dev), False)
    assert acq.ties.numel() == AR.DECODE_CAP + 1 == case.cap + 1
    acq.active.copy_(torch.from_numpy(case.active))
    return acq


def _fill(ext, acq, case, dev):
    q0 = torch.from_numpy(case.q0).to(dev)
    h0 = torch.from_numpy(np.array([case.h0], np.float32)).to(dev)
    ext.acq_select(q0, h0, acq.active, acq.qbuf, acq.out, acq.ties)


@pytest.mark.parametrize("which", ["untied", "two", "near", "packed-8191",
                                   "rescan-8192"])
def test_host_decode(ext, dev, which):
    case = AR.decode_cases()[which]
    ref = AR.ref_of(case)
    acq = _acquisition(case, dev)
    _fill(ext, acq, case, dev)
    assert int(acq.out[2]) == ref.ties.size
    for seed in (0, 7):
        pos, q, tied = AR.pick(ref, seed)
        random.seed(seed)
        got = acq.result()
        # q: the chosen entry's own fp32, compared as its bits
        assert got[0] == 3 * pos + 11 and got[2] is tied, (which, got)
        assert np.float32(got[1]).view(np.int32) \
            == np.float32(q).view(np.int32), (which, got, q)
        assert float(np.float32(got[1])) == got[1]
    if which in ("two", "packed-8191"):
        assert q < 0            # a sign bit went through the packed word


def test_host_decode_none_active(ext, dev):
    case = AR.decode_cases()["none"]
    acq = _acquisition(case, dev)
    _fill(ext, acq, case, dev)
    with pytest.raises(RuntimeError, match="no active"):
        acq.result()


# ---------------------------------------------------------------------
# in the selector
# ---------------------------------------------------------------------

def _selector_steps(dev, duplicate: bool):
    """12 captured acquisitions, each judged against the qbuf and mask it
    left on the device; returns how many of them had >= 2 ties."""
    import bench
    from coda_amd import CODA, Oracle
    from coda_amd.datasets import Dataset
    from coda_amd.options import LOSS_FNS

    preds, labels = bench.synth_preds(list(range(12)), 600, 8, dev)
    if duplicate:       # an exact copy of every point
        preds = torch.cat([preds, preds], dim=1).contiguous()
        labels = torch.cat([labels, labels])
    ds = Dataset.from_tensors(preds, labels, dev)
    oracle = Oracle(ds, LOSS_FNS["acc"])
    random.seed(0)
    torch.manual_seed(0)
    sel = CODA(ds)

    random.seed(100)
    i, q = sel.get_next_item_to_label()      # eager: no graph yet
    tied_steps = 0
    for step in range(1, 13):
        random.seed(100 + step)
        sel.add_label(i, oracle(int(i)), q)
        random.seed(100 + step)
        i, q = sel.get_next_item_to_label()
        acq = sel._pair_acq
        assert acq is not None and sel._label_graph is not None
        assert sel._merged_acq
        ref = AR.select(acq.qbuf.cpu().numpy(), acq.active.cpu().numpy())
        assert ref.ambiguous == 0, step
        pos, want_q, tied = AR.pick(ref, 100 + step)
        assert int(i) == acq.ids_host[pos], (step, int(i), pos)
        assert np.float32(q).view(np.int32) \
            == np.float32(want_q).view(np.int32), (step, q, want_q)
        assert int(i) not in sel.labeled_idxs
        assert sel.stochastic or not tied
        tied_steps += bool(tied)
        print(f"step {step}: ties {ref.ties.size} best {float(ref.best)!r}")
    print(f"{tied_steps} of 12 captured steps had >= 2 ties "
          f"(duplicate={duplicate})")
    return tied_steps


@pytest.mark.parametrize("pool", ["plain", "doubled"])
def test_selector_returns_what_the_contract_picks(dev, production, pool):
    """A full-pool CODA in production mode: the (id, q) each captured
    acquisition returns is the contract's pick, under the same
    random.seed, from the qbuf and mask that acquisition left on the
    device - so the rounding of the graphed pipeline upstream is not in
    question.

    A selection is decoded where its result is first read - for the first
    captured one that is inside add_label (the warm-up's read), for the
    rest inside get_next_item_to_label - so both calls are preceded by the
    same seed; nothing else in them draws from `random`.

    On the device the plain 12 x 600 x 8 pool has a unique maximum at each
    of its 12 captured steps, so it checks the untied decode only; with an
    exact copy of every point appended, the copies' q are bit-equal and 6
    of the 12 steps go through the tie-break (figures of an MI355X run).
    The tie assertion is made on that pool."""
    production.delenv("CODA_AMD_NO_GRAPH", raising=False)
    tied_steps = _selector_steps(dev, duplicate=pool == "doubled")
    if pool == "doubled":
        assert tied_steps >= 1
