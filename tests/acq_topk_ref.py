"""Batch acquisition's contract, as plain numpy.

ops/hip/pair.hip acq_select, given a `topk` buffer, also ranks the qbuf it
leaves (tests/acq_ref.py defines qbuf), and ops/reference.py acq_topk is
the same selection in torch. This module states what both must compute:

  order    active candidates by q descending under float comparison (so
           -0.0 orders as +0.0, -inf is legal and last, +inf first), then
           by position ascending
  groups   with group_of (values in [0, G)), only each group's first
           candidate under that order competes; None = every candidate is
           its own group
  slot[j]  for j < min(K, competing candidates): (position << 32) | fp32
           bits of qbuf[position] of the rank-j candidate - the packing of
           the tie words
  else     -1

No thresholds, no tolerances: every comparison against this is exact. NaN
is out of scope, as in acq_ref.

The generators are seeded and cached; nothing may modify what they return.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from tests import acq_ref as AR

F32 = np.float32
KS = (1, 2, 64, 1024)                       # for the acq_ref inputs
GROUP_SHAPES = (1, 2, 257, 10_000)
# where a wave (64), a block (256), the slice rule and the 1024 cap can
# go wrong
GPU_SHAPES = (1, 2, 255, 256, 257, 300, 65_536, 65_537, 200_000)
GPU_KS = (1, 2, 63, 64, 65, 255, 256, 257, 1024)
MUTATIONS = ("pos_desc", "unmasked", "ungrouped", "raw_zero",
             "first_member")
NEG_ZERO = F32(-0.0)    # the additive identity: -0 + x == x for every x


@dataclasses.dataclass(frozen=True, eq=False)     # hashed by identity
class Case:
    name: str
    q0: np.ndarray          # (B,) fp32
    h0: np.float32
    active: np.ndarray      # (B,) bool
    group_of: object        # (B,) int32 or None
    G: int                  # 0 without groups
    ks: tuple               # the K values this case is checked at
    kind: str = ""

    @property
    def B(self) -> int:
        return self.q0.size

    @property
    def qbuf(self) -> np.ndarray:
        return AR.masked_q(self.q0, self.h0, self.active)


def _image(bits: np.ndarray) -> np.ndarray:
    """Monotone unsigned image of fp32 bit patterns, as int64."""
    u = bits.astype(np.int64)
    neg = (u & 0x80000000) != 0
    return np.where(neg, (~u) & 0xFFFFFFFF, u | 0x80000000)


def pack(qbuf: np.ndarray, pos: np.ndarray) -> np.ndarray:
    pos = np.asarray(pos, dtype=np.int64)
    return (pos << 32) | qbuf[pos].view(np.uint32).astype(np.int64)


def ranked(qbuf, active, group_of=None, mutate=None) -> np.ndarray:
    """Positions of the competing candidates, best first."""
    assert mutate is None or mutate in MUTATIONS
    qbuf = np.asarray(qbuf, dtype=F32)
    active = np.asarray(active, dtype=bool)
    assert qbuf.ndim == 1 and active.shape == qbuf.shape
    assert not np.isnan(qbuf).any()
    if mutate == "unmasked":
        active = np.ones_like(active)
    pos = np.flatnonzero(active)
    if mutate == "raw_zero":
        img = _image(qbuf.view(np.uint32))            # -0 below +0
    else:
        img = _image((qbuf + F32(0.0)).view(np.uint32))
    tie = -pos if mutate == "pos_desc" else pos
    order = pos[np.lexsort((tie, -img[pos]))]
    if group_of is None or mutate == "ungrouped":
        return order
    group_of = np.asarray(group_of)
    assert group_of.shape == qbuf.shape
    if mutate == "first_member":
        # the group's first active member by position stands for it
        _, first = np.unique(group_of[pos], return_index=True)
        winners = np.zeros(qbuf.size, dtype=bool)
        winners[pos[first]] = True
        return order[winners[order]]
    _, first = np.unique(group_of[order], return_index=True)
    return order[np.sort(first)]


def select(qbuf, active, group_of, K: int, mutate=None) -> np.ndarray:
    """The contract: (K,) int64 slots."""
    assert K >= 1
    qbuf = np.asarray(qbuf, dtype=F32)
    order = ranked(qbuf, active, group_of, mutate)[:K]
    out = np.full(K, -1, dtype=np.int64)
    out[:order.size] = pack(qbuf, order)
    return out


def unpack(slots) -> tuple:
    """(positions, fp32 values) of the filled slots."""
    s = np.asarray(slots, dtype=np.int64)
    s = s[s != -1]
    return (s >> 32), (s & 0xFFFFFFFF).astype(np.uint32).view(F32)


# ---------------------------------------------------------------------
# case generators
# ---------------------------------------------------------------------

def _from_acq(c: AR.Case) -> Case:
    return Case("acq-" + c.name, c.q0, c.h0, c.active, None, 0, KS,
                kind="acq")


def _quantized(rng, B: int, levels: int) -> np.ndarray:
    """Values on a coarse grid: whole families of equal fp32 values."""
    return (rng.integers(0, levels, size=B) / F32(8.0) - 1.0).astype(F32)


def _ks_for(B: int) -> tuple:
    return tuple(sorted({1, 2, min(64, max(B - 1, 1)), 64, 1024}))


def _random_groups(rng, B: int) -> np.ndarray:
    """Group sizes from 1 to B/4, members scattered over the positions."""
    sizes = []
    left = B
    while left > 0:
        s = int(rng.integers(1, max(B // 4, 1) + 1))
        s = min(s, left)
        sizes.append(s)
        left -= s
    g = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(g)
    return g.astype(np.int32)


@functools.lru_cache(maxsize=None)
def group_cases() -> tuple:
    out = []
    for n, B in enumerate(GROUP_SHAPES):
        s = 9000 + 50 * n
        ks = _ks_for(B)

        def mk(name, q0, act, g, kind="group"):
            g = np.asarray(g, dtype=np.int32)
            G = int(g.max()) + 1
            out.append(Case(f"{name}-B{B}", q0.astype(F32), NEG_ZERO,
                            act, g, G, ks, kind=kind))

        rng = np.random.default_rng(s)
        q = _quantized(rng, B, 12)
        act = rng.random(B) < 0.8
        if B <= 2:
            act[:] = True
        mk("one-group", q, act, np.zeros(B))
        mk("own-group", q, act, np.arange(B))

        rng = np.random.default_rng(s + 1)
        g = _random_groups(rng, B)
        mk("random-groups", rng.standard_normal(B), rng.random(B) < 0.8, g)
        mk("random-groups-quantized", _quantized(rng, B, 5),
           rng.random(B) < 0.8, g)

        # every group's best member is inactive (a lower one stands in
        # where the group has another active member)
        rng = np.random.default_rng(s + 2)
        g = _random_groups(rng, B)
        q = rng.standard_normal(B).astype(F32)
        act = np.ones(B, dtype=bool)
        for grp in np.unique(g):
            mem = np.flatnonzero(g == grp)
            act[mem[np.argmax(q[mem])]] = False
        mk("best-inactive", q, act, g)

        # whole groups inactive
        rng = np.random.default_rng(s + 3)
        g = _random_groups(rng, B)
        q = rng.standard_normal(B).astype(F32)
        dead = np.unique(g)[::2]
        act = ~np.isin(g, dead)
        mk("dead-groups", q, act, g)

        # equal values inside one group: the earliest position wins, and
        # the group's first member by position is not its best
        rng = np.random.default_rng(s + 4)
        g = _random_groups(rng, B)
        q = rng.standard_normal(B).astype(F32)
        for grp in np.unique(g):
            mem = np.flatnonzero(g == grp)
            if mem.size >= 3:
                q[mem[1:]] = q[mem].max() + F32(0.5)
        mk("equal-inside", q, np.ones(B, dtype=bool), g)

        # equal values across groups: every group's best is the same value
        rng = np.random.default_rng(s + 5)
        g = _random_groups(rng, B)
        q = (-1.0 - rng.random(B)).astype(F32)
        for grp in np.unique(g):
            mem = np.flatnonzero(g == grp)
            q[mem[rng.integers(0, mem.size)]] = F32(0.25)
        mk("equal-across", q, rng.random(B) < 0.9, g)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cut_cases() -> tuple:
    """Equal maxima straddling the per = ceil(B/256) slice boundaries, at
    the rank-K cut: exactly K, K - 1 and K + 1 of them. Below them, a
    second family of equal values, so the cut lands inside a tie either
    way."""
    out = []
    for n, (B, K) in enumerate(((300, 2), (65_537, 64), (65_537, 257),
                                (200_000, 64), (200_000, 1024))):
        per = AR.per_block(B)
        nblk = (B + per - 1) // per
        for m in (K - 1, K, K + 1):
            rng = np.random.default_rng(9500 + 10 * n + (m - K))
            q = (-2.0 - rng.random(B)).astype(F32)
            # pairs (j*per - 1, j*per) around the boundaries, from the
            # middle outwards
            mids = [nblk // 2 + d for d in range(-(m // 4) - 1, m // 4 + 2)]
            pos = []
            for j in mids:
                if 1 <= j < nblk:
                    pos += [j * per - 1, j * per]
            pos = sorted(p for p in set(pos) if 0 <= p < B)
            taken = set(pos)
            extra = [p for p in rng.permutation(B).tolist()
                     if p not in taken]
            pos = (pos + extra)[:m] if len(pos) < m else pos[:m]
            second = extra[m:m + 5]
            q[second] = F32(-1.5)
            q[pos] = F32(0.8125)
            out.append(Case(f"cut-{m}of{K}-B{B}", q, NEG_ZERO,
                            np.ones(B, dtype=bool), None, 0, (K,),
                            kind="cut"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_cases() -> tuple:
    out = []
    # -0.0 next to +0.0, both the maximum; -0.0 comes first by position
    B = 300
    rng = np.random.default_rng(9700)
    q = (-1.0 - rng.random(B)).astype(F32)
    q[[3, 130, 258]] = F32(-0.0)
    q[[5, 131, 257]] = F32(0.0)
    out.append(Case("zeros", q, NEG_ZERO, np.ones(B, dtype=bool), None, 0,
                    (1, 2, 6, 7, 64), kind="zero"))
    g = (np.arange(B) // 2).astype(np.int32)    # (-0 @130, +0 @131) share
    out.append(Case("zeros-grouped", q, NEG_ZERO, np.ones(B, dtype=bool),
                    g, int(g.max()) + 1, (1, 2, 6, 64), kind="zero"))
    # active -inf entries, K beyond the finite count
    for n, B in enumerate((300, 65_537)):
        rng = np.random.default_rng(9710 + n)
        q = rng.standard_normal(B).astype(F32)
        act = np.zeros(B, dtype=bool)
        fin = rng.choice(B, size=10, replace=False)
        act[fin] = True
        ninf = [p for p in rng.permutation(B).tolist()
                if not act[p]][:20]
        q[ninf] = -np.inf
        act[ninf] = True
        q[ninf[0]] = np.inf                         # and one +inf: first
        out.append(Case(f"neg-inf-B{B}", q, NEG_ZERO, act, None, 0,
                        (1, 10, 11, 12, 30, 64, 1024), kind="inf"))
        g = _random_groups(rng, B)
        out.append(Case(f"neg-inf-grouped-B{B}", q, NEG_ZERO, act, g,
                        int(g.max()) + 1, (1, 12, 64, 1024), kind="inf"))
    # K beyond the active count, and nothing active
    for n, B in enumerate((1, 2, 257, 10_000)):
        rng = np.random.default_rng(9720 + n)
        q = rng.standard_normal(B).astype(F32)
        act = np.zeros(B, dtype=bool)
        act[rng.choice(B, size=min(B, 5), replace=False)] = True
        g = _random_groups(rng, B)
        G = int(g.max()) + 1
        ks = (1, 4, 5, 6, 64, 1024)
        out.append(Case(f"few-active-B{B}", q, NEG_ZERO, act, None, 0, ks,
                        kind="few"))
        out.append(Case(f"few-active-grouped-B{B}", q, NEG_ZERO, act, g, G,
                        ks, kind="few"))
        none = np.zeros(B, dtype=bool)
        out.append(Case(f"none-active-B{B}", q, NEG_ZERO, none, None, 0,
                        (1, 64, 1024), kind="none"))
        out.append(Case(f"none-active-grouped-B{B}", q, NEG_ZERO, none, g,
                        G, (1, 64, 1024), kind="none"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sweep_cases() -> tuple:
    """Every GPU shape, with and without groups, checked at every GPU K:
    quantized values (ties everywhere, the rank-K cut among them) and a
    random mask."""
    out = []
    for n, B in enumerate(GPU_SHAPES):
        rng = np.random.default_rng(9800 + n)
        q = _quantized(rng, B, 40)
        # a distinct head, so that small K are not all one value
        head = rng.choice(B, size=min(B, 40), replace=False)
        q[head] += rng.standard_normal(head.size).astype(F32)
        act = rng.random(B) < 0.8
        if B <= 2:
            act[:] = True
        g = _random_groups(rng, B)
        out.append(Case(f"sweep-B{B}", q, F32(0.37), act, None, 0, GPU_KS,
                        kind="sweep"))
        out.append(Case(f"sweep-grouped-B{B}", q, F32(0.37), act, g,
                        int(g.max()) + 1, GPU_KS, kind="sweep"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    cases = (tuple(_from_acq(c) for c in AR.all_cases()) + group_cases()
             + cut_cases() + edge_cases() + sweep_cases())
    assert len({c.name for c in cases}) == len(cases)
    return cases


@functools.lru_cache(maxsize=None)
def ref_of(case: Case, K: int) -> np.ndarray:
    out = select(case.qbuf, case.active, case.group_of, K)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def state_cases() -> tuple:
    """One set of buffers, three inputs in a row: many survivors, one,
    none. Same shape, same groups."""
    B = 10_000
    rng = np.random.default_rng(9900)
    g = rng.integers(0, 2000, size=B).astype(np.int32)  # more than K
    G = int(g.max()) + 1
    q = _quantized(rng, B, 30)
    one = np.zeros(B, dtype=bool)
    one[B - 7] = True
    ks = (64,)
    return (Case("state-many", q, F32(0.37), rng.random(B) < 0.9, g, G, ks),
            Case("state-one", q, F32(-1.5), one, g, G, ks),
            Case("state-none", q, F32(0.37), np.zeros(B, dtype=bool), g, G,
                 ks))


@functools.lru_cache(maxsize=None)
def graph_cases() -> tuple:
    """acq_ref.graph_cases() under one set of groups for the replays of
    one captured call, plus a mask change that empties a group: the best
    group of the first input, all of its members switched off."""
    base = AR.graph_cases()
    B = base[0].B
    rng = np.random.default_rng(9950)
    g = rng.integers(0, 5000, size=B).astype(np.int32)  # more than K
    G = int(g.max()) + 1
    ks = (1024,)
    out = [Case("topk-" + c.name, c.q0, c.h0, c.active, g, G, ks)
           for c in base]
    c = base[0]
    top = ranked(AR.masked_q(c.q0, c.h0, c.active), c.active, g)[0]
    act = c.active.copy()
    act[g == g[top]] = False
    out.append(Case("topk-graph-emptied-group", c.q0, c.h0, act, g, G, ks))
    return tuple(out)
