"""The fused acquisition epilogue's contract, as plain numpy.

ops/hip/pair.hip acq_select (three kernels) turns the pair engine's EIG
vector into what the run labels next, and selectors/pair_acq.py
PairAcquisition.result() decodes its buffers on the host. This module
states what both must compute, with no torch op in it:

  qbuf[i]  = active[i] ? fl32(h0 + q0[i]) : -inf
  best     = max(qbuf)
  first    = the first ACTIVE index holding best, -1 when nothing is active
  ties     = ascending positions of the active entries close to best under
             isclose as ATen defines it for fp32 with rtol = atol = 1e-8:
             q == best, or |q - best| finite and
             <= fl32(1e-8f + fl32(1e-8f * |best|))
  packed   = (position << 32) | fp32 bits of q, one int64 per tie

NaN is out of scope: no generator makes one.

Ambiguity. The kernel's compiler may contract the threshold into one fma,
which moves it by up to an ulp, so an entry whose |q - best| lies within
2 fp32 ulps of the threshold could legitimately go either way. Ref.ambiguous
counts them, and every generator here must produce none (the CPU test
asserts it), so every GPU comparison is exact. One class of entries is not
counted: where the product 1e-8f * |best| is exactly representable in fp32
(best = 0 is the case used), fma and mul+add round the same exact sum once,
the threshold is the same number either way, and an entry AT it is not
ambiguous. The best = 0 ladder carries such a rung (|q - best| == 1e-8f):
it is the only kind of input on which `<=` and `<` differ, and without it
no generated case could tell the two apart.

The generators are seeded and cached; nothing may modify what they return.
"""
from __future__ import annotations

import dataclasses
import functools
import random

import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)
RTOL = F32(1e-8)
ATOL = F32(1e-8)
GRID = 256           # blocks of the part and ties kernels (ACQ_GRID)
BLOCK = 256          # threads per block: a thread strides by this
DECODE_CAP = 8191    # PairAcquisition's 8192-word buffer: counter + slots

SHAPES = (1, 2, 255, 256, 257, 300, 10_000, 65_536, 65_537, 200_000)
LADDER_BESTS = (0.0, 3e-7, -2.5e-6, 1e-3, 0.37, -9.4)
SMALL_BESTS = (0.0, 3e-7, -2.5e-6, 1e-3)   # atol decides: unequal ties
RTOL_BEST = 1.5e-3   # 86 ulps below it lies between atol and the threshold
LADDER_D = (0.0, "ulp", 0.5e-8, 0.9e-8, 1.1e-8, 2e-8, 1e-6)
CAPS = (1, 7, 511)
MUTATIONS = ("lt", "no_rtol", "last_index", "unmasked")


@dataclasses.dataclass(frozen=True, eq=False)     # hashed by identity
class Case:
    name: str
    q0: np.ndarray          # (B,) fp32
    h0: np.float32
    active: np.ndarray      # (B,) bool
    cap: int = 511          # tie slots the kernel test hands over
    rungs: tuple = ()       # ladder cases: positions of the ladder members
    kind: str = ""

    @property
    def B(self) -> int:
        return self.q0.size


@dataclasses.dataclass(frozen=True)
class Ref:
    qbuf: np.ndarray        # (B,) fp32
    best: np.float32
    first: int
    ties: np.ndarray        # ascending positions, int64
    packed: np.ndarray      # int64, ascending with the positions
    ambiguous: int


def masked_q(q0, h0, active) -> np.ndarray:
    q0 = np.asarray(q0, dtype=F32)
    with np.errstate(all="ignore"):
        s = F32(h0) + q0                        # fp32 + fp32: one rounding
    assert s.dtype == F32
    return np.where(np.asarray(active, dtype=bool), s, NEG_INF)


def threshold(best, mutate=None) -> np.float32:
    if mutate == "no_rtol":
        return ATOL
    with np.errstate(all="ignore"):
        return F32(ATOL + F32(RTOL * np.abs(F32(best))))


def select(qbuf, active, mutate=None) -> Ref:
    """The contract from the masked values on (also what the decode and
    the selector tests apply to a qbuf fetched from the device)."""
    assert mutate is None or mutate in MUTATIONS
    qbuf = np.asarray(qbuf, dtype=F32)
    active = np.asarray(active, dtype=bool)
    assert qbuf.ndim == 1 and qbuf.size >= 1 and active.shape == qbuf.shape
    assert not np.isnan(qbuf).any()
    best = F32(qbuf.max())
    hits = np.flatnonzero(active & (qbuf == best))
    if not active.any():
        first = -1
    else:
        first = int(hits[-1] if mutate == "last_index" else hits[0])
    thr = threshold(best, mutate)
    with np.errstate(all="ignore"):
        d = np.abs(qbuf - best)                 # fp32; inf - inf = NaN
        within = (d < thr) if mutate == "lt" else (d <= thr)
        close = (qbuf == best) | (np.isfinite(d) & within)
    if mutate != "unmasked":
        close &= active
    ties = np.flatnonzero(close).astype(np.int64)
    packed = (ties << 32) | qbuf[ties].view(np.uint32).astype(np.int64)

    # entries within 2 ulps of a threshold that contraction can move
    amb = 0
    prod = np.float64(RTOL) * np.float64(np.abs(best))   # exact in fp64
    if np.isfinite(thr) and np.float64(F32(prod)) != prod:
        d64 = np.abs(qbuf.astype(np.float64) - np.float64(best))
        band = 2.0 * np.float64(np.spacing(thr))
        with np.errstate(all="ignore"):
            amb = int((active & np.isfinite(d64)
                       & (np.abs(d64 - np.float64(thr)) <= band)).sum())
    return Ref(qbuf, best, first, ties, packed, amb)


def reference(q0, h0, active, mutate=None) -> Ref:
    return select(masked_q(q0, h0, active), active, mutate)


@functools.lru_cache(maxsize=None)
def ref_of(case: Case) -> Ref:
    return reference(case.q0, case.h0, case.active)


def pick(ref: Ref, seed: int):
    """(position, q value, tied) as result() must decode it: the first
    index when the maximum is alone, else one random.choice, seeded here,
    over the ascending tie positions."""
    if ref.first < 0:
        raise LookupError("nothing active")
    if ref.ties.size <= 1:
        return ref.first, float(ref.best), False
    random.seed(seed)
    pos = random.choice(ref.ties.tolist())
    return pos, float(ref.qbuf[pos]), True


# ---------------------------------------------------------------------
# case generators
# ---------------------------------------------------------------------

def per_block(B: int) -> int:
    return (B + GRID - 1) // GRID


def _background(rng, B: int, top: float) -> np.ndarray:
    """Values a unit or more below `top`: never near the maximum."""
    return (top - 1.0 - 3.0 * rng.random(B)).astype(F32)


def _maxima(name, B, seed, pos, inactive=(), top=0.8125, h0=0.37,
            active=None, cap=511, kind="placement") -> Case:
    rng = np.random.default_rng(seed)
    q0 = _background(rng, B, top)
    q0[list(pos)] = F32(top)
    act = np.ones(B, dtype=bool) if active is None else active.copy()
    act[list(pos)] = True
    act[list(inactive)] = False
    return Case(f"{name}-B{B}", q0, F32(h0), act, cap=cap, kind=kind)


@functools.lru_cache(maxsize=None)
def placement_cases() -> tuple:
    out = []
    for n, B in enumerate(SHAPES):
        per = per_block(B)
        nblk = (B + per - 1) // per
        # negative maxima (h0 = -1.5) on every other shape
        kw = dict(h0=(0.37, -1.5)[n % 2])
        s = 1000 + 20 * n
        out.append(_maxima("at-0", B, s, [0], **kw))
        if B > 1:
            out.append(_maxima("at-last", B, s + 1, [B - 1], **kw))
        k = nblk // 2
        if k >= 1 and k * per < B:
            out.append(_maxima("before-boundary", B, s + 2, [k * per - 1],
                               **kw))
            out.append(_maxima("after-boundary", B, s + 3, [k * per], **kw))
        if B >= 2:
            rng = np.random.default_rng(s + 4)
            pos = sorted(rng.choice(B, size=min(3, B),
                                    replace=False).tolist())
            out.append(_maxima("dup-first-inactive", B, s + 4, pos,
                               inactive=pos[:1], **kw))
        if per > BLOCK:
            i = k * per               # thread 0 of block k, trips 1, 2, ...
            pos = [j for j in (i, i + BLOCK, i + 2 * BLOCK)
                   if j < min(i + per, B)]
            assert len(pos) >= 2
            out.append(_maxima("dup-one-thread", B, s + 5, pos, **kw))
        if per >= 2 and k * per + 1 < B:
            out.append(_maxima("dup-two-threads", B, s + 6,
                               [k * per, k * per + 1], **kw))
        if nblk >= 2:
            p1 = per // 2
            p2 = min((nblk - 1) * per + per // 3, B - 1)
            assert p1 // per != p2 // per
            out.append(_maxima("dup-two-blocks", B, s + 7, [p1, p2], **kw))
    return tuple(out)


def _rung_values(best32: np.float32, extra=()) -> list:
    ulp = float(np.abs(np.spacing(best32)))
    ds = [ulp if d == "ulp" else d for d in LADDER_D] + list(extra)
    return [F32(np.float64(best32) - np.float64(d)) for d in ds]


@functools.lru_cache(maxsize=None)
def ladder_cases() -> tuple:
    """Candidates at best - d, once as h0 = 0 and once as h0 = 0.731 with
    q0 = fl32(target - h0); there the sums lie on a grid of 2^-24 or
    coarser, wider than any threshold below, so only equal values tie."""
    out = []
    B = 300
    for n, best in enumerate(LADDER_BESTS + (RTOL_BEST,)):
        best32 = F32(best)
        extra = ()
        if best == 0.0:
            extra = (float(ATOL),)              # exactly at the threshold
        elif best == RTOL_BEST:
            extra = (86 * float(np.spacing(best32)),)
        targets = _rung_values(best32, extra)
        for h0 in (0.0, 0.731):
            rng = np.random.default_rng(2000 + n)
            tq = _background(rng, B, float(best32))
            pos = sorted(rng.choice(B - 1, size=len(targets),
                                    replace=False).tolist())
            for p, t in zip(pos, targets):
                tq[p] = t
            act = np.ones(B, dtype=bool)
            # a close-but-masked copy of the 0.5e-8 rung
            tq[B - 1] = targets[2]
            act[B - 1] = False
            h32 = F32(h0)
            q0 = (tq.astype(np.float64) - np.float64(h32)).astype(F32)
            out.append(Case(f"ladder-best{best:g}-h{h0:g}", q0, h32, act,
                            rungs=tuple(pos), kind="ladder"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tie_count_cases() -> tuple:
    out = []
    B = 1000
    for cap in CAPS:
        counts = sorted({c for c in (1, 2, 7, cap - 1, cap, cap + 1, B)
                         if c >= 1})
        for n in counts:
            rng = np.random.default_rng(3000 + 7 * cap + n)
            pos = rng.choice(B, size=n, replace=False).tolist()
            neg = n % 2 == 0
            out.append(_maxima(f"ties{n}-cap{cap}", B, 3000 + n, pos,
                               top=(-0.625 if neg else 0.8125), h0=0.0,
                               cap=cap, kind="ties"))
    rng = np.random.default_rng(3999)
    pos = rng.choice(200_000, size=600, replace=False).tolist()
    out.append(_maxima("ties600-cap511", 200_000, 3998, pos, cap=511,
                       kind="ties"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mask_cases() -> tuple:
    out = []
    for n, B in enumerate((1, 2, 257, 10_000, 65_537)):
        s = 4000 + 10 * n
        rng = np.random.default_rng(s)
        q0 = rng.standard_normal(B).astype(F32)
        h0 = F32(0.37)
        out.append(Case(f"all-active-B{B}", q0, h0,
                        np.ones(B, dtype=bool), kind="mask"))
        out.append(Case(f"none-active-B{B}", q0, h0,
                        np.zeros(B, dtype=bool), kind="mask"))
        # the global maximum sits on inactive entries from here on
        q1 = q0.copy()
        hi = rng.choice(B, size=min(3, max(B - 1, 1)),
                        replace=False).tolist() if B > 1 else []
        q1[hi] = F32(50.0)
        one = np.zeros(B, dtype=bool)
        lone = int(rng.choice([i for i in range(min(B, 4096))
                               if i not in hi]))
        one[lone] = True
        out.append(Case(f"single-active-B{B}", q1, h0, one, kind="mask"))
        act = rng.random(B) < 0.8
        act[hi] = False
        act[lone] = True
        out.append(Case(f"random-active-B{B}", q1, h0, act, kind="mask"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def infinity_cases() -> tuple:
    out = []
    for n, B in enumerate((1000, 65_537)):
        rng = np.random.default_rng(5000 + n)
        base = rng.standard_normal(B).astype(F32)
        act = rng.random(B) < 0.8
        a, b, c = sorted(rng.choice(np.arange(1, B), size=3,
                                    replace=False).tolist())
        q = base.copy()
        q[b] = np.inf
        m = act.copy()
        m[b] = True
        out.append(Case(f"one-inf-B{B}", q, F32(0.37), m, kind="inf"))
        q = base.copy()
        q[[a, b, c]] = np.inf
        m = act.copy()
        m[[a, c]] = True
        m[b] = False                            # a masked +inf between
        out.append(Case(f"two-inf-B{B}", q, F32(0.37), m, kind="inf"))
        q = base.copy()
        m = act.copy()
        m[0] = False                            # first index is inactive
        m[[a, b]] = True
        q[m] = -np.inf
        q[c] = -np.inf                          # an inactive -inf as well
        m[c] = False
        out.append(Case(f"all-neg-inf-B{B}", q, F32(0.37), m, kind="inf"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def all_cases() -> tuple:
    cases = (placement_cases() + ladder_cases() + tie_count_cases()
             + mask_cases() + infinity_cases())
    assert len({c.name for c in cases}) == len(cases)
    return cases


def _near_ties(name, B, seed, best, n_close, n_far, cap) -> Case:
    """n_close entries within 0.8e-8 below best (ties under atol), n_far
    between 1.2e-8 and 1e-6 below it (not ties)."""
    rng = np.random.default_rng(seed)
    best32 = F32(best)
    q0 = _background(rng, B, float(best32))
    pos = rng.choice(B, size=1 + n_close + n_far, replace=False)
    q0[pos[0]] = best32
    q0[pos[1:1 + n_close]] = (np.float64(best32)
                              - 0.8e-8 * rng.random(n_close)).astype(F32)
    q0[pos[1 + n_close:]] = (
        np.float64(best32) - 1.2e-8
        - (1e-6 - 1.2e-8) * rng.random(n_far)).astype(F32)
    return Case(name, q0, F32(0.0), np.ones(B, dtype=bool), cap=cap,
                kind="near")


@functools.lru_cache(maxsize=None)
def state_cases() -> tuple:
    """One set of buffers, three inputs in a row: many ties, one, three."""
    B = 10_000
    rng = np.random.default_rng(6000)
    many = rng.choice(B, size=400, replace=False).tolist()
    three = rng.choice(B, size=3, replace=False).tolist()
    return (_maxima("state-many", B, 6001, many, top=-0.625, h0=0.0),
            _maxima("state-one", B, 6002, [B - 7]),
            _maxima("state-three", B, 6003, three, h0=-1.5))


@functools.lru_cache(maxsize=None)
def graph_cases() -> tuple:
    """Three inputs of one shape for three replays of one captured call;
    h0 and the mask change between them as well."""
    B = 65_537
    rng = np.random.default_rng(7000)
    act = rng.random(B) < 0.8
    many = rng.choice(B, size=300, replace=False).tolist()
    three = sorted(rng.choice(B, size=3, replace=False).tolist())
    return (_maxima("graph-many", B, 7001, many, top=-0.625, h0=0.0),
            _maxima("graph-last", B, 7002, [B - 1], active=act),
            _maxima("graph-three", B, 7003, three, inactive=three[:1],
                    h0=-1.5, active=act),
            _near_ties("graph-near", B, 7004, 3e-7, 200, 200, 511))


@functools.lru_cache(maxsize=None)
def decode_cases() -> dict:
    """Inputs for PairAcquisition.result(), whose buffer has DECODE_CAP
    slots: DECODE_CAP ties is the last count it decodes from the packed
    words, DECODE_CAP + 1 the first it rescans."""
    B = 20_000
    rng = np.random.default_rng(8000)
    two = rng.choice(B, size=2, replace=False).tolist()
    last_packed = rng.choice(B, size=DECODE_CAP, replace=False).tolist()
    first_rescan = rng.choice(B, size=DECODE_CAP + 1, replace=False).tolist()
    kw = dict(cap=DECODE_CAP, kind="decode")
    none = _maxima("decode-none", B, 8005, [5], **kw)
    none = dataclasses.replace(none, active=np.zeros(B, dtype=bool))
    return {
        "untied": _maxima("decode-untied", B, 8001, [B - 3], h0=-1.5, **kw),
        "two": _maxima("decode-two", B, 8002, two, top=-0.625, h0=0.0,
                       **kw),
        "near": _near_ties("decode-near", B, 8003, 3e-7, 400, 400,
                           DECODE_CAP),
        "packed-8191": _maxima("decode-8191", B, 8004, last_packed,
                               top=-0.625, h0=0.0, **kw),
        "rescan-8192": _maxima("decode-8192", B, 8006, first_rescan, **kw),
        "none": none,
    }
