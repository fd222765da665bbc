"""Everything the full-pool pair acquisition derives from one candidate
set, under one owner.

The hit structure (ops/pair.py) is static for a fixed set of disagreeing
points, so it is built once and every later step reuses it: labeled or
skipped points are masked, not removed. The pair cache, the active mask,
the shard permutation and the captured acquisition's result buffers are
all sized by that one structure and die with it: CODA holds a single
reference and drops the lot by assigning None to it.
"""
from __future__ import annotations

import random
import struct

import torch

from ..ops import pair as pops
from ..ops.reference import ACQ_TOPK_MAX, group_rows
from ..util import pair_cache_fits


def tied_choice(q: torch.Tensor, best, mask: torch.Tensor = None) -> int:
    """Seeded tie-break (coda/coda.py:306-313): one random.choice over
    the ascending positions where q is close to its maximum (and, when
    given, the mask holds)."""
    ties = torch.isclose(q, best, rtol=1e-8)
    if mask is not None:
        ties = ties & mask
    return random.choice(torch.nonzero(ties, as_tuple=True)[0].tolist())


class PairAcquisition:
    def __init__(self, ps: pops.PairStructure, cls_rows: torch.Tensor,
                 ids: torch.Tensor, perm: torch.Tensor, use_cache: bool):
        self.ps, self.cls_rows = ps, cls_rows
        # point id -> row of the candidate set; rows of labeled or
        # skipped points are masked at gather
        self.row_of = {int(p): i for i, p in enumerate(ids.tolist())}
        self.active = torch.ones(ids.numel(), dtype=torch.bool,
                                 device=ids.device)
        self.perm = perm        # rank-concatenated EIG -> list order
        # pair cache (ops/pair.py PairCache): the per-pair state a label
        # on another class leaves unchanged, so a label re-evaluates one
        # class's pairs, not all K
        self.use_cache = use_cache
        self.cache = None
        self.stale = set()      # classes whose table rows moved
        self.declined = False   # gate/fit said no for this structure
        self.ids_host = self.out = self.qbuf = self.ties = None
        self.out_host = self.ties_host = None
        if ids.is_cuda:
            # result buffers of the captured acquisition: out = [masked
            # max, first argmax, isclose tie count], qbuf = masked q.
            # Tie buffer: [0]=slot counter, [1:] packs (position << 32) |
            # q-value-bits per tie (host-sorted back to ascending
            # position - one D2H fetch serves both the seeded tie-break
            # AND its q value); overflow falls back to the full-scan
            # path.  Host mirrors are PINNED so the per-step result
            # fetches take the fast DMA path.
            self.ids_host = ps.cand_ids.cpu().tolist()
            self.out = torch.zeros(3, dtype=torch.float64,
                                   device=ids.device)
            self.qbuf = torch.empty(ps.cand_ids.numel(), device=ids.device)
            self.ties = torch.zeros(8192, dtype=torch.int64,
                                    device=ids.device)
            self.out_host = torch.empty(3, dtype=torch.float64,
                                        pin_memory=True)
            self.ties_host = torch.empty(8192, dtype=torch.int64,
                                         pin_memory=True)

        # batch acquisition (allocated by enable_topk on the first batch
        # request; a run that never asks for one holds none of it): the
        # prediction-pattern groups, the (1024,) slot buffer acq_select
        # fills in rank order, and its pinned mirror. topk_distinct is
        # what the captured graph was given: None = no batch outputs.
        self.group_of, self.n_groups = None, 0
        self.topk = self.topk_host = None
        self.topk_distinct = None

    # -- batch acquisition ---------------------------------------------
    def groups(self):
        """(group_of (B,) int32, n_groups): the index of each candidate's
        row among the unique rows of the (B, H) class matrix. Static, so
        built once, outside any capture."""
        if self.group_of is None:
            self.group_of, self.n_groups = group_rows(self.cls_rows)
        return self.group_of, self.n_groups

    def enable_topk(self, distinct: bool) -> bool:
        """Have the captured acquisition write batch outputs, one per
        group when distinct. True when that changes what a capture must
        contain (the caller drops its graphs)."""
        if self.topk is None:
            dev = self.active.device
            self.topk = torch.full((ACQ_TOPK_MAX,), -1, dtype=torch.int64,
                                   device=dev)
            self.topk_host = torch.empty(ACQ_TOPK_MAX, dtype=torch.int64,
                                         pin_memory=True)
        if distinct:
            self.groups()
        changed = self.topk_distinct is not distinct
        self.topk_distinct = bool(distinct)
        return changed

    def topk_args(self):
        """acq_select's trailing arguments for the current choice."""
        if self.topk_distinct is None:
            return ()
        if self.topk_distinct:
            return (self.topk, self.group_of, self.n_groups)
        return (self.topk,)

    def result_topk(self, k: int):
        """[(point id, q value)] of the first k filled slots of the batch
        last written; one D2H copy of k words."""
        th = self.topk_host[:k]
        th.copy_(self.topk[:k])
        out = []
        for w in th.tolist():
            if w == -1:
                break
            out.append((self.ids_host[w >> 32], struct.unpack(
                "<f", struct.pack("<I", w & 0xFFFFFFFF))[0]))
        return out

    def deactivate(self, point_id: int):
        row = self.row_of.get(point_id)
        if row is not None:
            self.active[row] = False

    # -- pair cache ----------------------------------------------------
    def drop_cache(self):
        """The one place the cache (and its scratch) is invalidated:
        called by whatever replaces the tables."""
        self.cache = None
        self.stale = set()
        self.declined = False

    def cache_wanted(self, tables) -> bool:
        """The scope gate, as one predicate: the static full-pool
        structure on the fused B-resident route, a cache that fits with
        headroom, and no CODA_AMD_NO_PAIR_CACHE."""
        if not self.use_cache or tables is None:
            return False
        return (pops.pair_cache_gate(tables, self.ps)
                and pair_cache_fits(
                    self.active.device,
                    pops.pair_cache_bytes(self.ps, tables.EG.shape[1])))

    def sync_cache(self, tables):
        """Build the cache where the static structure and the pair
        tables first both exist (never under capture), or bring it up to
        date: one one-class refresh per class whose table rows moved
        since its last read. Returns the cache or None (uncached path)."""
        if self.cache is None:
            if not self.declined:
                if self.cache_wanted(tables):
                    self.cache = pops.pair_cache_build(tables, self.ps,
                                                       self.cls_rows)
                    self.stale = set()
                else:
                    self.declined = True
            return self.cache
        for y in sorted(self.stale):
            y_arg = y if self.cache.pbn is not None else \
                torch.tensor([y], dtype=torch.long,
                             device=self.active.device)
            pops.pair_cache_refresh(self.cache, tables, self.ps,
                                    self.cls_rows, y_arg)
        self.stale = set()
        return self.cache

    # -- captured acquisition: device -> host --------------------------
    def result(self):
        """(point id, q value, tied) of the acquisition last written to
        the result buffers; one host sync."""
        self.out_host.copy_(self.out)
        bv, bi, nt = self.out_host.tolist()
        bi, nt = int(bi), int(nt)
        if bi < 0:
            raise RuntimeError("acquisition ran with no active "
                               "candidates (pool exhausted?)")
        if nt <= 1:
            return self.ids_host[bi], bv, False
        # same tie semantics as the eager path: active candidates
        # ascend by point id in both orderings.  The fused epilogue
        # collected (position, q value) pairs already (unordered
        # slots); sorting restores the ascending order the seeded
        # random.choice tie-break expects.
        if nt < self.ties.numel():
            th = self.ties_host[:1 + nt]
            th.copy_(self.ties[:1 + nt])
            pk = random.choice(sorted(v & 0xFFFFFFFFFFFFFFFF
                                      for v in th[1:].tolist()))
            pos = pk >> 32
            qv = struct.unpack(
                "<f", struct.pack("<I", pk & 0xFFFFFFFF))[0]
        else:  # > buffer capacity: rescan (never seen in practice)
            pos = tied_choice(self.qbuf, self.qbuf.max(), self.active)
            qv = float(self.qbuf[pos])
        return self.ids_host[pos], qv, True
