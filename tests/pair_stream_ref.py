"""Shared by tests/test_pair_stream.py (CPU) and
tests/test_pair_stream_gpu.py: hand-built pair structures, the kernel
constants the tests depend on (read from the source, not copied), and the
rows of a structure that the cached entropy pass must leave unread."""
from __future__ import annotations

import functools
import itertools
import os
import re

import torch

PAIR_HIP = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "coda_amd", "ops", "hip", "pair.hip")


@functools.lru_cache(maxsize=None)
def kernel_constant(name: str) -> int:
    """The integer `#define name` of pair.hip."""
    with open(PAIR_HIP) as f:
        m = re.search(rf"^#define\s+{name}\s+(\d+)\b", f.read(), re.M)
    assert m, name
    return int(m.group(1))


def finalize_one_pass() -> int:
    """Candidates one pass of the finalize grid covers: FIN_MAX_BLOCKS
    blocks of 4 waves, one candidate per wave at a time."""
    return kernel_constant("FIN_MAX_BLOCKS") * 4


BOUNDARY = (8, 600, 5, 0.5, 128)     # tables of this problem, own structure
BOUNDARY_LIVE = [16, 64, 32, 64, 1]


def _subsets(n):
    """The 2^n - 1 non-empty subsets of range(n)."""
    return [s for r in range(1, n + 1)
            for s in itertools.combinations(range(n), r)]


@functools.lru_cache(maxsize=None)
def boundary_structure():
    """H = 8, C = 5. Class 0's hit sets are the 15 non-empty subsets of
    models {0..3}, class 1's the 63 of {0..5}, class 2's the 31 of
    {0..4}; every other prediction is class 3 (whose sets are the 63
    complements) and nobody predicts class 4. With the base pair that is
    16, 64, 32, 64 and 1 live rows."""
    from coda_amd.ops import pair as pops
    H, _, C = BOUNDARY[:3]
    rows = []
    for c, n in ((0, 4), (1, 6), (2, 5)):
        for s in _subsets(n):
            r = torch.full((H,), 3, dtype=torch.long)
            r[list(s)] = c
            rows.append(r)
    cls = torch.stack(rows)                                  # (109, H)
    ps = pops.build_pairs(cls, torch.arange(cls.shape[0]), C, tile=128)
    assert ps.run_live.tolist() == BOUNDARY_LIVE, ps.run_live.tolist()
    assert ps.K == 128 * C
    return ps


# the (H, N, C, p, tile) problem whose tables go with long_run_structure
# (the skewed case of tests/test_pair_cache_gpu.py)
LONG_RUN = (12, 4000, 3, 0.6, 128)


@functools.lru_cache(maxsize=None)
def long_run_structure():
    """Class 0 with more tiles than one group holds AND a last group that
    is not full: its blocks b % 4 past the group's tiles must return."""
    from coda_amd.ops import pair as pops
    H, N, C = LONG_RUN[:3]
    g = torch.Generator().manual_seed(4)
    agree = torch.rand(N, H, generator=g) < 0.5
    unif = torch.randint(0, C, (N, H), generator=g)
    cls = torch.where(agree, torch.zeros(N, H, dtype=torch.long), unif)
    return pops.build_pairs(cls, torch.arange(N), C, tile=128)


def unread_rows(ps) -> torch.Tensor:
    """(K,) bool: rows in a chunk (ECH-th of a 128-pair tile) that holds
    no live row of its class - what pair_entropy_cached must not read
    when it is given run_off / run_live. The class's base row is live."""
    rows = 128 // kernel_constant("ECH")
    k = torch.arange(ps.K)
    c = ps.pair_c.long()
    live_end = (ps.run_off[:-1] + ps.run_live).long()[c]
    return (k // rows) * rows >= live_end
