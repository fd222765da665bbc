"""Batch acquisition on the GPU, exactly.

ops/hip/pair.hip acq_select with a `topk` buffer (and groups) against the
numpy contract of tests/acq_topk_ref.py, which tests/test_acq_topk.py
holds to a pure-Python ranking on the CPU; then the selector's captured
batch path against the same contract applied to what the acquisition left
on the device. Bitwise comparisons only: there is no tolerance in this
file. Every buffer is in range by construction; the sentinel tails turn an
over-write into a failed assertion.
"""
from __future__ import annotations

import random

import numpy as np
import pytest
import torch

from tests import acq_ref as AR
from tests import acq_topk_ref as TR

pytestmark = pytest.mark.gpu

SENTINEL = -0x5A5A5A5A5A5A5A5B
GSENT = 0x5A5A5A5A          # int32 sentinel behind group_of
TAIL = 64


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
    """Device inputs and outputs of one acq_select call with batch
    outputs. topk, the tie buffer and group_of are contiguous prefixes of
    sentinel-filled allocations."""

    def __init__(self, B: int, K: int, dev, grouped: bool, cap: int = 511):
        self.K, self.cap, self.grouped = K, cap, grouped
        self.q0 = torch.zeros(B, device=dev)
        self.h0 = torch.zeros(1, device=dev)
        self.active = torch.zeros(B, dtype=torch.bool, device=dev)
        self.qbuf = torch.full((B,), float("nan"), device=dev)
        self.out = torch.full((3,), float("nan"), dtype=torch.float64,
                              device=dev)
        self.big = torch.full((cap + 1 + TAIL,), SENTINEL,
                              dtype=torch.int64, device=dev)
        self.ties = self.big[:cap + 1]
        # topk starts as sentinels too: every slot must be written
        self.tbig = torch.full((K + TAIL,), SENTINEL, dtype=torch.int64,
                               device=dev)
        self.topk = self.tbig[:K]
        self.gbig = torch.full((B + TAIL,), GSENT, dtype=torch.int32,
                               device=dev)
        self.group_of = self.gbig[:B]
        self.G = 0
        assert self.topk.is_contiguous() and self.group_of.is_contiguous()

    def load(self, case):
        assert case.B == self.q0.numel()
        self.q0.copy_(torch.from_numpy(case.q0))
        self.h0.copy_(torch.from_numpy(np.array([case.h0], np.float32)))
        self.active.copy_(torch.from_numpy(case.active))
        if self.grouped:
            self.group_of.copy_(torch.from_numpy(case.group_of))
            self.G = case.G

    def run(self, ext, topk: bool = True):
        args = (self.q0, self.h0, self.active, self.qbuf, self.out,
                self.ties)
        if not topk:
            ext.acq_select(*args)
        elif self.grouped:
            ext.acq_select(*args, self.topk, self.group_of, self.G)
        else:
            ext.acq_select(*args, topk=self.topk)

    def fetch_topk(self) -> np.ndarray:
        tbig = self.tbig.cpu()
        assert (tbig[self.K:] == SENTINEL).all(), "wrote behind topk"
        assert (self.gbig[self.q0.numel():] == GSENT).all().item(), \
            "wrote behind group_of"
        return tbig[:self.K].numpy().copy()

    def fetch_select(self):
        """What the three existing kernels leave, as comparable values:
        qbuf bits, out, the tie counter, the set of filled slots."""
        big = self.big.cpu()
        assert (big[self.cap + 1:] == SENTINEL).all(), \
            "wrote behind the tie buffer"
        n = int(big[0])
        return (self.qbuf.cpu().numpy().view(np.int32).copy(),
                self.out.cpu().numpy().view(np.int64).copy(), n,
                frozenset(big[1:1 + min(n, self.cap)].tolist()))


def _check(buf, case, K):
    got = buf.fetch_topk()
    want = TR.ref_of(case, K)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(
            f"{case.name} K={K}: {bad.size} slots differ, first at "
            f"{bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}")


# ---------------------------------------------------------------------
# 1. kernel == contract
# ---------------------------------------------------------------------

def test_shapes_and_ks_are_the_ones_that_can_go_wrong():
    assert TR.GPU_SHAPES == (1, 2, 255, 256, 257, 300, 65_536, 65_537,
                             200_000)
    assert TR.GPU_KS == (1, 2, 63, 64, 65, 255, 256, 257, 1024)
    swept = {(c.B, c.group_of is not None) for c in TR.sweep_cases()}
    assert swept == {(B, g) for B in TR.GPU_SHAPES for g in (False, True)}
    assert all(c.ks == TR.GPU_KS for c in TR.sweep_cases())


@pytest.mark.parametrize("case", TR.all_cases(), ids=lambda c: c.name)
def test_kernel_against_contract(ext, dev, case):
    for K in case.ks:
        buf = Buffers(case.B, K, dev, case.group_of is not None)
        buf.load(case)
        buf.run(ext)
        _check(buf, case, K)
        # the qbuf it ranked is the contract's
        assert np.array_equal(buf.qbuf.cpu().numpy().view(np.int32),
                              case.qbuf.view(np.int32)), case.name
    buf.run(ext)                # again on the same buffers: same bits
    _check(buf, case, K)


# ---------------------------------------------------------------------
# 2. the existing outputs do not move
# ---------------------------------------------------------------------

_SELECT_CASES = (AR.placement_cases() + AR.ladder_cases()
                 + AR.tie_count_cases())


@pytest.mark.parametrize("case", _SELECT_CASES, ids=lambda c: c.name)
def test_existing_outputs_are_bit_equal(ext, dev, case):
    rng = np.random.default_rng(case.B)
    g = (rng.integers(0, max(case.B // 3, 1), size=case.B)
         .astype(np.int32))
    tc = TR.Case(case.name, case.q0, case.h0, case.active, g,
                 int(g.max()) + 1, (64,))
    plain = Buffers(case.B, 64, dev, False, cap=case.cap)
    plain.load(tc)
    plain.run(ext, topk=False)
    want = plain.fetch_select()
    assert (plain.tbig == SENTINEL).all().item()    # topk untouched
    for grouped in (False, True):
        buf = Buffers(case.B, 64, dev, grouped, cap=case.cap)
        buf.load(tc)
        buf.run(ext)
        got = buf.fetch_select()
        assert np.array_equal(got[0], want[0]), case.name
        assert np.array_equal(got[1], want[1]), case.name
        assert got[2] == want[2], case.name
        if want[2] <= case.cap:     # else: which members fit is a race
            assert got[3] == want[3], case.name
        else:
            assert len(got[3]) == case.cap
        assert np.array_equal(
            buf.fetch_topk(),
            TR.select(tc.qbuf, tc.active, g if grouped else None, 64))


# ---------------------------------------------------------------------
# 3. state across calls
# ---------------------------------------------------------------------

@pytest.mark.parametrize("grouped", [False, True])
def test_state_across_calls(ext, dev, grouped):
    """Many survivors, then one, then none through ONE set of buffers:
    no slot of an earlier call survives, and the best-per-group words are
    zeroed again (a stale winner would outrank the lone survivor)."""
    cases = TR.state_cases()
    K = cases[0].ks[0]
    counts = [(TR.ref_of(c, K) != -1).sum() for c in cases]
    assert counts == [K, 1, 0]
    buf = Buffers(cases[0].B, K, dev, grouped)
    for c in cases + cases[:1]:
        if not grouped:
            c = TR.Case(c.name + "-flat", c.q0, c.h0, c.active, None, 0,
                        c.ks)
        buf.load(c)
        buf.run(ext)
        _check(buf, c, K)


# ---------------------------------------------------------------------
# 4. under a graph
# ---------------------------------------------------------------------

@pytest.mark.parametrize("grouped", [False, True])
def test_under_a_graph(ext, dev, grouped):
    """One captured call on static buffers; q0, h0 and the mask are
    rewritten in place between replays, the last of which empties the
    first input's best group."""
    from coda_amd.selectors.coda import _warm_and_capture
    cases = TR.graph_cases()
    assert len(cases) == 5
    if not grouped:
        cases = tuple(TR.Case(c.name + "-flat", c.q0, c.h0, c.active, None,
                              0, c.ks) for c in cases)
    K = cases[0].ks[0]
    buf = Buffers(cases[0].B, K, dev, grouped)
    buf.load(cases[0])
    graph, first = _warm_and_capture(lambda: buf.run(ext), buf.fetch_topk)
    assert np.array_equal(first, TR.ref_of(cases[0], K))
    for c in cases[1:] + cases[:1]:
        buf.load(c)
        graph.replay()
        torch.cuda.synchronize()
        _check(buf, c, K)
    if grouped:
        a = TR.unpack(TR.ref_of(cases[0], K))[0]
        b = TR.unpack(TR.ref_of(cases[4], K))[0]
        g = cases[0].group_of
        assert g[a[0]] not in set(g[b].tolist())


# ---------------------------------------------------------------------
# argument checks: all before the first launch
# ---------------------------------------------------------------------

def test_arguments_are_validated(ext, dev):
    case = TR.state_cases()[0]
    buf = Buffers(case.B, 8, dev, True)
    buf.load(case)
    args = (buf.q0, buf.h0, buf.active, buf.qbuf, buf.out, buf.ties)
    before = buf.qbuf.cpu().numpy().view(np.int32).copy()
    bad = [
        dict(group_of=buf.group_of, n_groups=buf.G),         # no topk
        dict(topk=buf.topk.int()),
        dict(topk=torch.zeros(1025, dtype=torch.int64, device=dev)),
        dict(topk=torch.zeros(0, dtype=torch.int64, device=dev)),
        dict(topk=torch.zeros(16, dtype=torch.int64, device=dev)[::2]),
        dict(topk=torch.zeros(8, dtype=torch.int64)),        # host
        dict(topk=buf.topk, group_of=buf.group_of.long(), n_groups=buf.G),
        dict(topk=buf.topk, group_of=buf.group_of[:-1], n_groups=buf.G),
        dict(topk=buf.topk, group_of=buf.group_of, n_groups=0),
        dict(topk=buf.topk, group_of=buf.group_of.cpu(), n_groups=buf.G),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            ext.acq_select(*args, **kw)
    torch.cuda.synchronize()
    # nothing ran: qbuf still holds its NaN fill
    assert np.array_equal(buf.qbuf.cpu().numpy().view(np.int32), before)
    assert (buf.tbig == SENTINEL).all().item()


# ---------------------------------------------------------------------
# 5. in the selector
# ---------------------------------------------------------------------

def _pool(dev, duplicate=True):
    import bench
    from coda_amd import Oracle
    from coda_amd.datasets import Dataset
    from coda_amd.options import LOSS_FNS
    preds, labels = bench.synth_preds(list(range(12)), 600, 8, dev)
    if duplicate:       # an exact copy of every point: ties and patterns
        preds = torch.cat([preds, preds], dim=1).contiguous()
        labels = torch.cat([labels, labels])
    ds = Dataset.from_tensors(preds, labels, dev)
    return ds, Oracle(ds, LOSS_FNS["acc"])


def _new_selector(ds):
    import bench
    from coda_amd import CODA
    random.seed(0)
    torch.manual_seed(0)
    # the consensus prior sums with float atomics unless told otherwise;
    # two selectors are compared bit for bit below
    with bench.reproducible_setup():
        return CODA(ds)


def _contract_batch(acq, k, distinct):
    """The contract on what the acquisition left on the device."""
    qbuf = acq.qbuf.cpu().numpy()
    active = acq.active.cpu().numpy()
    g = acq.group_of.cpu().numpy() if distinct else None
    pos, vals = TR.unpack(TR.select(qbuf, active, g, k))
    return [(acq.ids_host[p], float(v)) for p, v in zip(pos.tolist(), vals)]


def test_selector_batches_are_the_contract(dev, production):
    """Twelve labels in batches of 4 on a pool that takes the captured
    pair path: before a round's labels are applied, its batch is the
    contract applied to the qbuf the acquisition left on the device and
    PairAcquisition's groups. Then distinct is switched mid-run, which
    re-captures, and the batches stay exact."""
    production.delenv("CODA_AMD_NO_GRAPH", raising=False)
    ds, oracle = _pool(dev)
    sel = _new_selector(ds)
    random.seed(100)
    i, q = sel.get_next_item_to_label()         # eager: no graph yet
    sel.add_label(i, oracle(int(i)), q)         # captures label + acquire
    assert sel._label_graph is not None and sel._merged_acq
    assert sel._pair_acq.topk is None           # no batch asked for yet

    served_on_device = 0
    plan = [True] * 3 + [False] * 2 + [True]
    prev = None
    for rnd, distinct in enumerate(plan):
        graph_before = sel._label_graph
        pending = sel._acq_pending
        state, stochastic = random.getstate(), sel.stochastic
        batch = sel.get_next_items_to_label(4, distinct=distinct)
        # k > 1 never draws and never marks the run stochastic
        assert random.getstate() == state
        assert sel.stochastic == stochastic
        acq = sel._pair_acq
        if distinct != prev:        # a capture-time choice: re-captured
            assert sel._label_graph is None and graph_before is not None
        else:
            assert sel._label_graph is graph_before
            assert pending is not None
            served_on_device += 1
            want = _contract_batch(acq, 4, distinct)
            assert batch == want, (rnd, batch, want)
        prev = distinct
        ids = [i for i, _ in batch]
        assert len(batch) == 4 and len(set(ids)) == 4
        assert not set(ids) & set(sel.labeled_idxs)
        rows = {tuple(sel.classes[:, i].tolist()) for i in ids}
        assert len(rows) == 4 if distinct else len(rows) <= 4
        qs = [q for _, q in batch]
        assert qs == sorted(qs, reverse=True)
        sel.add_labels(ids, [oracle(i) for i in ids], qs)
        assert sel._label_graph is not None and acq.topk is not None
        assert acq.topk_distinct is distinct
    assert served_on_device == 3
    # a skip drops the pending result; the next batch is acquired again
    nxt = sel.get_next_items_to_label(4)
    sel.skip(nxt[0][0])
    assert sel._acq_pending is None
    again = sel.get_next_items_to_label(4)
    assert again == _contract_batch(sel._pair_acq, 4, True)
    assert nxt[0][0] not in {i for i, _ in again}


def test_first_batch_is_eager_then_on_device(dev, production):
    """The first batch request finds a graph without batch outputs: it is
    served eagerly (eig_batched + the torch twin) and the graphs are
    dropped; one label later the re-captured graph serves the batch."""
    production.delenv("CODA_AMD_NO_GRAPH", raising=False)
    ds, oracle = _pool(dev)
    sel = _new_selector(ds)
    random.seed(100)
    i, q = sel.get_next_item_to_label()
    sel.add_label(i, oracle(int(i)), q)
    first = sel.get_next_items_to_label(8)      # eager; graphs dropped
    assert sel._label_graph is None
    ids = [i for i, _ in first]
    assert len(set(tuple(sel.classes[:, i].tolist()) for i in ids)) == 8
    sel.add_labels(ids[:1], [oracle(ids[0])], [first[0][1]])
    assert sel._label_graph is not None and sel._acq_pending is not None
    on_device = sel.get_next_items_to_label(8)
    assert on_device == _contract_batch(sel._pair_acq, 8, True)


def test_default_path_is_untouched(dev, production):
    """A selector that never asks for a batch: the captured graph gets no
    batch outputs, and its twelve single picks are those of a second
    selector whose batch outputs were switched on before the first
    capture - the three existing kernels' outputs do not depend on the
    new ones, and the captured pipeline upstream is the same."""
    production.delenv("CODA_AMD_NO_GRAPH", raising=False)
    ds, oracle = _pool(dev, duplicate=False)

    def trajectory(with_batch):
        sel = _new_selector(ds)
        out = []
        random.seed(100)
        i, q = sel.get_next_item_to_label()
        if with_batch:          # no graph yet: nothing to drop
            assert sel._label_graph is None
            sel._pair_acq.enable_topk(True)
        for step in range(1, 13):
            out.append((int(i), np.float32(q).view(np.int32).item()))
            random.seed(100 + step)
            sel.add_label(i, oracle(int(i)), q)
            random.seed(100 + step)
            i, q = sel.get_next_item_to_label()
        return out, sel

    plain, sel = trajectory(False)
    assert sel._pair_acq.topk is None and sel._pair_acq.topk_args() == ()
    assert sel._label_graph is not None
    batched, sel2 = trajectory(True)
    acq = sel2._pair_acq
    assert acq.topk is not None and sel2._acq_pending is None
    # and the slots that rode along with the last single pick
    assert acq.result_topk(4) == _contract_batch(acq, 4, True)
    print("single-pick trajectory:", plain)
    assert plain == batched
