"""CODA: Consensus-Driven Active Model Selection.

Behavioral parity with the reference algorithm (coda/coda.py:171-346):
a Dirichlet confusion-matrix posterior per model, seeded from an
ensemble-consensus prior; P(model-is-best) via the diagonal-Beta grid
integral; expected-information-gain acquisition over unlabeled points;
greedy selection with seeded random tie-breaking.

MI355X-first differences from the reference implementation (none change
the math):
  - argmax classes and the disagreement prefilter mask are computed ONCE
    and cached (the reference recomputes both every step from the full
    (H,N,C) tensor: coda/coda.py:217,263).
  - the per-chunk hot path (hypothetical Beta updates -> Beta-grid P(best)
    -> EIG) is one fused op (`ops.eig_chunk`), which on GPU is a pair of
    hand-written gfx950 HIP kernels that never materialize the (R,H,P)
    pdf/cdf tensors (reference materializes ~6 of them:
    coda/coda.py:94-111).
  - the model axis may be sharded across ranks (`comm`); cross-model
    reductions become RCCL all-reduces (coda_amd/ops/sharded.py).
"""
from __future__ import annotations

import random

import torch
from sortedcontainers import SortedList

from ..base import ModelSelector
from ..parallel import Comm, get_comm
from .. import ops
from ..ops import pair as pops
from ..ops import sharded as shops
from ..ops import table as tops
from ..util import DEBUG, _check, mirror_fits
from .pair_acq import PairAcquisition, tied_choice

import os
DEBUG_VIZ = os.environ.get("CODA_AMD_DEBUG_VIZ") == "1"

# self._acq_pending when the next acquisition's result waits in the
# device result buffers (a host result waits as its (index, q) tuple)
_ON_DEVICE = object()


def _warm_and_capture(body, read=None):
    """Capture body() into a hipGraph; returns (graph, read()).

    The warm-up executes the body for real on a side stream, as stream
    capture requires; the capture pass then only RECORDS the ops (no
    execution, no state change), so whatever the body computes has
    happened exactly once when this returns and the caller must not
    additionally replay. read() runs between the two, on the warm-up's
    results, before the capture rebinds the body's output tensors."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = read() if read is not None else None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    return g, first


class CODA(ModelSelector):
    supports_batch = True

    def __init__(self, dataset,
                 prefilter_n: int = 0,
                 alpha: float = 0.9,
                 learning_rate: float = 0.01,
                 multiplier: float = 2.0,
                 disable_diag_prior: bool = False,
                 q: str = "eig",
                 comm: Comm = None,
                 chunk_size: int = 100,
                 num_points: int = 256,
                 pi_hat_precision: str = "auto",
                 eig_impl: str = "auto"):
        self.dataset = dataset
        self.device = dataset.preds.device
        self.comm = comm or get_comm()
        self.Hl, self.N, self.C = dataset.preds.shape  # local models
        self.H = getattr(dataset, "total_models", self.Hl)
        self.prefilter_n = prefilter_n
        self.disable_diag_prior = disable_diag_prior
        self.q = q
        self.chunk_size = chunk_size
        self.num_points = num_points
        # EIG implementation: 'fused' = the wave-per-row HIP kernel (GPU) /
        # eager (CPU); 'table' = the factored per-step curve tables + MFMA
        # GEMM (ops/table.py); 'pair' = the hit-sparse pair engine
        # (ops/pair.py - the full-pool no-prefilter fast path). 'auto'
        # resolves per device at eig time.
        self.eig_impl = eig_impl
        # CODA_AMD_NO_PAIR_CACHE=1 forces the uncached pair kernels
        self._use_pair_cache = \
            os.environ.get("CODA_AMD_NO_PAIR_CACHE") != "1"
        self._est_distinct = None    # _hit_sparse's one-off estimate
        # hipGraph capture of the post-label update pipeline (Dirichlet row
        # update -> rank-1 pi_hat -> table row refresh -> posterior rows):
        # ~20 static-shape launches replayed as one graph. Auto on
        # single-device GPU; CODA_AMD_NO_GRAPH=1 disables.
        # (debug guards synchronize per op and cannot run under stream
        # capture - graph replay is a production-mode path)
        self._use_label_graph = (
            self.device.type == "cuda" and not self.comm.is_distributed
            and not DEBUG
            and os.environ.get("CODA_AMD_NO_GRAPH") != "1")

        # hyperparams (reference names: coda/coda.py:189-190)
        self.prior_strength = 1.0 - alpha
        self.update_strength = learning_rate

        preds = dataset.preds
        # one chunked fp32-upcast pass: cached argmax classes (Hl, N) +
        # consensus sum (storage may be fp32/bf16/fp8)
        # - unless the loader's fused ingest already produced them (sharded
        # tasks: datasets.Dataset.init_stats), in which case neither the
        # stats nor the mirror below are recomputed
        stats = getattr(dataset, "init_stats", None)
        if (stats is not None
                and tuple(stats["classes"].shape) == (self.Hl, self.N)
                and tuple(stats["ens_sum"].shape) == (self.N, self.C)):
            self.classes = stats["classes"]
            ens_sum = stats["ens_sum"].clone()  # all-reduced in place below
        else:
            stats = None
            self.classes, ens_sum = ops.init_model_stats(preds)

        # Sharded pair engine = "replicated Betas, sharded candidates":
        # every rank keeps the global (H, C) diagonal-Beta view + the
        # global argmax classes (gathered ONCE - they never change), so
        # tables/pbest/mixture are computed locally and bit-identically
        # on all ranks, EIG work is split by candidate, and the only
        # per-step wire is the (N,) pi_hat delta + a (B,) EIG gather.
        # This replaces the round-1 design that gathered (B, H, P) delta
        # curves per chunk (268 MB/chunk at the 8-GPU config;
        # VERDICT.md round-1 finding #1).
        self._replicated = (
            self.comm.is_distributed and self.H <= 1024
            and self.C <= 32767 and eig_impl in ("auto", "pair"))
        self.classes_global = None
        if self._replicated:
            # gather in int32 (gloo has no int16 collectives), store
            # int16 - at the 8-GPU 1024x1M config that's 2 GB resident
            cls32 = self.classes.to(torch.int32)
            gathered = self.comm.all_gather_cat(
                cls32, dim=0, sizes=self.comm.shard_sizes(self.H))
            order = self.comm.unshard_order(self.H).to(gathered.device)
            self.classes_global = gathered[order].to(torch.int16) \
                .contiguous()                               # (H, N)

        # pi_hat compute dtype: bf16 MFMA on GPU (one packed (N, H*C) GEMM,
        # ~16x the f32 matrix rate, f32 accumulation), fp32 elsewhere.
        if pi_hat_precision == "auto":
            pi_hat_precision = "bf16" if preds.is_cuda else "fp32"
        if preds.dtype == torch.float8_e4m3fn and pi_hat_precision == "fp32":
            pi_hat_precision = "bf16"  # fp8 storage has no fp32 bmm path
        self.pi_hat_precision = pi_hat_precision
        self._adjusted = None  # maintained incrementally after init

        # static class-major mirror of the prediction pool (H, C, N):
        # the per-label rank-1 pi_hat gather preds[h, :, cls_h] reads
        # one element per 64-B sector in row-major layout (at the
        # random-sector floor - 150 us headline, 1.2 ms at 10k models);
        # the mirror makes it a coalesced stream. Built only when HBM
        # has the pool's size + 24 GB headroom to spare (the 128 GB
        # fp8 million-point pool deliberately skips it).
        self._preds_t = None
        if stats is not None:
            # built (or skipped, under the same headroom rule) at ingest
            self._preds_t = stats.get("preds_t")
        elif preds.is_cuda and ops.hip_available() and preds.dim() == 3:
            try:
                need = preds.numel() * preds.element_size()
                if mirror_fits(self.device, need):
                    self._preds_t = preds.permute(0, 2, 1).contiguous()
            except (RuntimeError, torch.OutOfMemoryError):
                self._preds_t = None

        # consensus prior: global mean over H (all-reduce site K1)
        self.comm.all_reduce_(ens_sum)
        pseudo = (ens_sum / self.H).argmax(-1)            # (N,) global pseudo-labels
        soft_conf = ops.confusion_prior(pseudo, preds)    # (Hl, C, C)
        self.dirichlets = ops.init_dirichlets(
            soft_conf, self.prior_strength, disable_diag_prior, multiplier)

        # static disagreement mask (K12): "not all models agree".
        if self._replicated:
            ref = self.classes_global[0]
            self._disagreement = (self.classes_global
                                  != ref.unsqueeze(0)).any(dim=0)
        else:
            # Cross-shard: compare against global model 0's classes (it
            # lives on rank 0 under strided sharding), then OR-reduce.
            ref_row = self.classes[0].clone() if self.comm.rank == 0 \
                else torch.empty_like(self.classes[0])
            self.comm.broadcast_(ref_row, src=0)
            dis = (self.classes != ref_row.unsqueeze(0)).any(dim=0) \
                .to(torch.float32)
            self.comm.all_reduce_(dis)
            self._disagreement = dis > 0                  # (N,) bool
        # host-side copy for the per-step candidate filter (indexing a GPU
        # tensor point-by-point would be one device sync per point)
        self._disagreement_host = self._disagreement.cpu().tolist()

        self.labeled_idxs, self.labels = [], []
        self.unlabeled_idxs = SortedList(range(self.N))
        self.q_vals = []
        self.stochastic = False
        self.step = 0
        self.reset_derived_state()
        self.update_pi_hat()

    def reset_derived_state(self):
        """Put everything derived from the restorable state (the
        Dirichlets and the labeled/unlabeled bookkeeping) back to what a
        fresh selector holds. Called by __init__ and, followed by
        update_pi_hat(), by whatever replaces that state (checkpoint
        restore): a new derived field is added here and nowhere else."""
        self._tables = None          # persistent v2 curve tables
        self._tables_dirty = set()   # class rows touched since last build
        # full-pool pair acquisition over the static candidate set: hit
        # structure, active mask, pair cache, result buffers
        self._pair_acq = None
        self._posterior_version = 0  # bumped by add_label
        self._pbest_rows_cache = (-1, None)
        # _label_graph: the post-label update pipeline (see
        # _use_label_graph). _acq_graph: the full-pool pair acquisition
        # (static hit structure + static table/posterior buffers -> the
        # whole get_next tensor pipeline incl. argmax/tie counting
        # replays as one graph; one host sync per step)
        self._drop_graphs()
        self._merged_acq = False     # _label_graph also acquires
        # the label graph's static inputs (1,) int64 and outputs
        self._g_idx = self._g_y = self._g_pi = self._g_rows = None
        self._alpha_g, self._beta_g = self._gather_global_betas()
        # persistently maintained unlabeled-and-disagreeing candidates
        # (the mask is static; add_label removes one entry). SortedList
        # keeps the reference's ascending order with O(log N) removal -
        # a plain list.remove is an O(N) scan per label.
        self._active_candidates = SortedList(
            i for i in self.unlabeled_idxs if self._disagreement_host[i])

    def _drop_graphs(self):
        """Captured graphs alias the buffers they were captured on, and
        a pending acquisition result was computed by one of them: all
        three go together."""
        self._label_graph = None
        self._acq_graph = None
        self._acq_pending = None
        # the merged graph's mixture0 (= the marginal P(best) get_pbest
        # returns) with the posterior version it belongs to;
        # _acq_mixture: the tensor the last run or recording of
        # _acq_body produced, _label_mixture: the label graph's own
        self._mixture_cache = (-1, None)
        self._acq_mixture = self._label_mixture = None

    def _gather_global_betas(self):
        """Replicated global (H, C) diagonal-Beta view (gathered here;
        kept current locally from classes_global on every label)."""
        if not self._replicated:
            return None, None
        a_l, b_l = ops.dirichlet_to_beta(self.dirichlets)  # (Hl, C)
        sizes = self.comm.shard_sizes(self.H)
        order = self.comm.unshard_order(self.H).to(self.device)
        return tuple(self.comm.all_gather_cat(
            t, dim=0, sizes=sizes)[order].contiguous() for t in (a_l, b_l))

    @classmethod
    def from_args(cls, dataset, args, comm=None):
        return cls(dataset,
                   prefilter_n=args.prefilter_n,
                   alpha=args.alpha,
                   learning_rate=args.learning_rate,
                   multiplier=args.multiplier,
                   disable_diag_prior=args.no_diag_prior,
                   q=args.q,
                   comm=comm,
                   chunk_size=getattr(args, "chunk_size", 100),
                   pi_hat_precision=getattr(args, "pi_hat_precision",
                                            "auto"))

    # ------------------------------------------------------------------
    def _prefilter(self, idxs):
        """Drop points where every model agrees (no information), optionally
        subsample to prefilter_n (reference: coda/coda.py:215-224)."""
        if idxs is self.unlabeled_idxs:
            idxs = self._active_candidates  # incrementally maintained
        else:
            mask = self._disagreement_host
            idxs = [i for i in idxs if mask[i]]
        if self.prefilter_n and len(idxs) > self.prefilter_n:
            idxs = random.sample(idxs, self.prefilter_n)
            self.stochastic = True
        return idxs

    def update_pi_hat(self, recontract: bool = True):
        """Confusion-adjusted class marginals (K5; all-reduce over H).

        Runs the FULL contraction (one packed bf16 MFMA GEMM on GPU).
        Called once at init; per-label updates go through the exact
        rank-1 incremental path in add_label (ops.pi_hat_delta), which
        is O(H*N) instead of O(H*N*C^2). recontract=False keeps the
        maintained adjusted/row_sums and only re-derives pi_hat from
        them: a checkpoint carries the two, because the contraction
        does not reproduce the sum of the increments to the last bit
        (nor, on the bf16 route, to fp32 precision) and a restored run
        has to continue the run it was saved from.
        """
        if not recontract:
            self.pi_hat = self._pi_marginal()
            self._pi_xi_cache = None
            return
        if self.pi_hat_precision == "bf16":
            # N-chunked pack + bf16 MFMA GEMM: never holds the full
            # (N, H*C) operand, so million-point pools fit alongside the
            # prediction tensor in HBM
            adjusted = ops.pi_hat_partial_streamed(self.dirichlets,
                                                   self.dataset.preds)
        else:
            adjusted = ops.pi_hat_partial(self.dirichlets, self.dataset.preds)
        self.comm.all_reduce_(adjusted)
        self._adjusted = adjusted
        self._row_sums = adjusted.sum(dim=-1)
        self.pi_hat = self._pi_marginal()
        self._pi_xi_cache = None

    def _pi_marginal(self):
        """pi_hat (C,) from the maintained adjusted/row_sums WITHOUT
        materializing the (N, C) per-item normalization: the marginal is
        one GEMV, pi = adjusted^T @ (1/rowsum), then self-normalized
        (identical math to the reference's pi_hat_xi.sum(0) route,
        coda/coda.py:229-233). Per-item rows are built on demand
        (candidate gathers in eig_batched; the pi_hat_xi property)."""
        if (self._adjusted.is_cuda and self.C <= 2048
                and ops.hip_available()):
            pi = ops._ext.pi_marginal(self._adjusted, self._row_sums)
        else:
            inv = 1.0 / self._row_sums.clamp_min(1e-12)
            # row-vector @ matrix streams adjusted once; transposed mv is
            # 5x slower on ROCm (strided column reduction)
            pi = inv @ self._adjusted
        return pi / pi.sum()

    @property
    def pi_hat_xi(self):
        """(N, C) per-item class posterior (materialized on demand)."""
        if self._pi_xi_cache is None:
            rs = self._row_sums.clamp_min(1e-12).unsqueeze(-1)
            self._pi_xi_cache = self._adjusted / rs
        return self._pi_xi_cache

    def _pi_xi_rows(self, ids):
        rs = self._row_sums[ids].clamp_min(1e-12).unsqueeze(-1)
        return self._adjusted[ids] / rs

    # ------------------------------------------------------------------
    def _pbest_rows_before(self):
        """(C, Hl) P(best | class row c) under the current posterior.

        Memoized on the posterior version: the rows computed by get_pbest
        right after a label are identical to the next acquisition's
        pbest_before (nothing moves the Dirichlets in between)."""
        ver, cached = self._pbest_rows_cache
        if ver == self._posterior_version and cached is not None:
            return cached
        alpha_cc, beta_cc = self._beta_view()
        a, b = alpha_cc.t().contiguous(), beta_cc.t().contiguous()
        if self.comm.is_distributed and not self._replicated:
            rows = shops.pbest_from_beta_sharded(a, b, self.comm,
                                                 self.num_points)
        else:
            # replicated mode computes the GLOBAL (C, H) rows locally
            rows = ops.pbest_from_beta(a, b, self.num_points)
        self._pbest_rows_cache = (self._posterior_version, rows)
        return rows

    def _beta_view(self):
        """(H?, C) diagonal Betas: global when replicated, else local."""
        if self._replicated:
            return self._alpha_g, self._beta_g
        return ops.dirichlet_to_beta(self.dirichlets)

    def _refresh_tables(self, alpha_cc, beta_cc, want_egw: bool):
        """Build or incrementally refresh the per-step curve tables."""
        acq = self._pair_acq
        if self._tables is None:
            self._tables = tops.table_precompute(
                alpha_cc, beta_cc, num_points=self.num_points)
            if acq is not None:
                acq.drop_cache()
        elif self._tables_dirty:
            tops.table_update_rows(self._tables, alpha_cc, beta_cc,
                                   sorted(self._tables_dirty))
            if acq is not None and acq.cache is not None:
                # whichever path refreshed the rows, the cache owes
                # these classes a refresh before its next read
                acq.stale |= self._tables_dirty
        self._tables_dirty.clear()
        if want_egw:
            self._tables = pops.attach_pair_tables(self._tables)
        return self._tables

    def _sync_pair_cache(self):
        """The pair cache brought up to date with the tables (built on
        first use), or None on the uncached path. Never under capture."""
        acq = self._pair_acq
        if acq is None:
            return None
        had = acq.cache is not None
        cache = acq.sync_cache(self._tables)
        if cache is not None and not had:
            # a graph captured without the cache neither refreshes nor
            # reads it: recapture
            self._drop_graphs()
        return cache

    def _eig_pair(self, candidate_ids):
        """v3 hit-sparse EIG over the candidate set (ops/pair.py).

        Distributed: candidates are split round-robin by their position
        in the (shared, ascending) candidate list; each rank scores its
        slice against the replicated global tables, and the (B,) EIG
        values are all-gathered and re-interleaved - O(B) bytes per
        step on the wire.
        """
        alpha_cc, beta_cc = self._beta_view()
        tables = self._refresh_tables(alpha_cc, beta_cc, want_egw=True)
        pbest_before = self._pbest_rows_before()            # (C, H)
        mixture0, H_before = ops.mixture_entropy(pbest_before, self.pi_hat)

        r, w = self.comm.rank, self.comm.world

        def build(ids_t):
            mine = ids_t[r::w] if self._replicated else ids_t
            cls_rows = self._global_classes(mine)
            wide = self.H > 1024  # beyond the vmask/fused-kernel regime
            return pops.build_pairs(
                cls_rows, mine, self.C, tile=(128 if wide else 0),
                with_vmask=not wide), cls_rows

        if candidate_ids is self._active_candidates:
            # full-pool acquisition: the hit structure is static (argmax
            # classes never change); labeled points are masked at gather
            if self._pair_acq is None:
                ids = torch.tensor(list(candidate_ids), device=self.device)
                self._pair_acq = PairAcquisition(
                    *build(ids), ids, self._interleave_perm(ids.numel()),
                    self._use_pair_cache)
            acq = self._pair_acq
            ps, cls_rows, mask, perm = (acq.ps, acq.cls_rows, acq.active,
                                        acq.perm)
        else:
            cand = torch.tensor(list(candidate_ids), device=self.device)
            ps, cls_rows = build(cand)
            mask, perm = None, self._interleave_perm(cand.numel())
        if ps.cand_ids.numel():
            h_after = None
            if mask is not None:   # the static structure: cached route
                cache = self._sync_pair_cache()
                if cache is not None:
                    h_after = pops.pair_cache_h_after(
                        cache, ps, self.pi_hat, pbest_before, mixture0)
            q = pops.eig_pairs(tables, ps, cls_rows, pbest_before,
                               self.pi_hat, mixture0, H_before,
                               self._adjusted, self._row_sums,
                               h_after=h_after)
        else:  # more ranks than candidates
            q = torch.empty(0, device=self.device)
        if self._replicated:
            sizes = [len(range(rr, (mask.numel() if mask is not None
                                    else perm.numel()), w))
                     for rr in range(w)]
            q = self.comm.all_gather_cat(q, dim=0, sizes=sizes)[perm]
        return (q[mask] if mask is not None else q), candidate_ids

    def _interleave_perm(self, n: int) -> torch.Tensor:
        """Permutation mapping rank-concatenated round-robin slices back
        to list order (identity when not distributed)."""
        if not self._replicated:
            return torch.arange(n, device=self.device)
        w = self.comm.world
        perm = torch.empty(n, dtype=torch.long, device=self.device)
        off = 0
        for rr in range(w):
            cnt = len(range(rr, n, w))
            perm[rr:n:w] = torch.arange(off, off + cnt, device=self.device)
            off += cnt
        return perm

    def _hit_sparse(self) -> bool:
        """True when candidates hit few distinct classes (the pair
        engine's regime): estimated from a 1024-point sample once."""
        if self._est_distinct is None:
            src = self.classes_global if self._replicated else self.classes
            n = src.shape[1]
            g = torch.Generator(device="cpu").manual_seed(0)
            idx = torch.randperm(n, generator=g)[:1024].to(src.device)
            sub = src[:, idx].long().sort(dim=0).values
            distinct = (sub[1:] != sub[:-1]).sum(0) + 1
            self._est_distinct = float(distinct.float().mean())
        return self._est_distinct <= max(self.C / 4.0, 32.0)

    def _global_classes(self, ids: torch.Tensor) -> torch.Tensor:
        """(B, H) int32 argmax classes of every GLOBAL model on the
        given points."""
        src = self.classes_global if self._replicated else self.classes
        return src[:, ids].t().to(torch.int32).contiguous()

    def eig_batched(self):
        """EIG for every candidate point (reference: coda/coda.py:235-281)."""
        candidate_ids = self._prefilter(self.unlabeled_idxs) \
            or self.unlabeled_idxs

        impl0 = self.eig_impl
        full_set = candidate_ids is self._active_candidates
        if impl0 == "auto":
            if self._replicated:
                impl0 = "pair"
            elif (self.device.type == "cuda"
                    and not self.comm.is_distributed and self.H <= 1024
                    and full_set and self._hit_sparse()):
                # full-pool acquisition: the static hit structure pays
                # for itself when candidates hit FEW distinct classes.
                # Prefiltered SUBSETS resample every step, where the v2
                # table chunks (tuned round 1: 1.33 ms/step at
                # prefilter 256) beat a per-step structure rebuild; and
                # when H >~ C the sparsity collapses (nearly every
                # class is hit by some model, K ~ B*C = the dense
                # problem) so v2 stays - measured 20.1 vs 4.0 ms/step
                # at H=4096, 15.2 vs ~5 at H=1024 full-pool.
                impl0 = "pair"
        if impl0 == "pair" and (self._replicated
                                or not self.comm.is_distributed):
            return self._eig_pair(candidate_ids)

        cand = torch.tensor(list(candidate_ids), device=self.device)

        pbest_before = self._pbest_rows_before()            # (C, Hl)
        alpha_cc, beta_cc = ops.dirichlet_to_beta(self.dirichlets)
        if self.comm.is_distributed:
            mixture0, H_before = shops.mixture_entropy_sharded(
                pbest_before, self.pi_hat, self.comm)
        else:
            mixture0, H_before = ops.mixture_entropy(pbest_before, self.pi_hat)

        impl = impl0
        if impl == "auto" or impl == "pair":
            impl = "table" if self.device.type == "cuda" else "fused"
        tables = s_base_all = None
        if impl == "table":
            tables = self._refresh_tables(alpha_cc, beta_cc,
                                          want_egw=False)
            if self.comm.is_distributed:
                s_base_all = tops.s_base_global(tables, self.comm)

        eig_chunks = []
        for s in range(0, cand.numel(), self.chunk_size):
            ids = cand[s:s + self.chunk_size]
            chunk_classes = self.classes[:, ids].t().contiguous()  # (B, Hl)
            pi_xi = self._pi_xi_rows(ids)                          # (B, C)
            if self.comm.is_distributed and tables is not None:
                eig = tops.eig_chunk_table_sharded(
                    tables, s_base_all, chunk_classes, pbest_before,
                    self.pi_hat, pi_xi, mixture0, H_before, self.comm,
                    hsizes=self.comm.shard_sizes(self.H))
            elif self.comm.is_distributed:
                eig = shops.eig_chunk_sharded(
                    alpha_cc, beta_cc, chunk_classes, pbest_before,
                    self.pi_hat, pi_xi, mixture0, H_before, self.comm,
                    num_points=self.num_points)
            elif tables is not None:
                eig = tops.eig_chunk_table(
                    tables, chunk_classes, pbest_before, self.pi_hat,
                    pi_xi, mixture0, H_before)
            else:
                eig = ops.eig_chunk(
                    alpha_cc, beta_cc, chunk_classes, pbest_before,
                    self.pi_hat, pi_xi, mixture0, H_before,
                    num_points=self.num_points)
            eig_chunks.append(eig)

        return torch.cat(eig_chunks), candidate_ids

    # -- hipGraph full-pool acquisition --------------------------------
    def _acq_body(self):
        """The whole get_next tensor pipeline on the STATIC buffers:
        mixture entropy from the label-graph's posterior rows/pi_hat,
        the three pair kernels, labeled-candidate masking, argmax and
        tie counting. Captured once; identical math to _eig_pair."""
        acq = self._pair_acq
        rows, pi = self._g_rows, self._g_pi
        mixture0, H0 = ops.mixture_entropy(rows, pi)
        # kept for get_pbest(); holding it also keeps a capture from
        # handing its block to a later tensor of the same graph
        self._acq_mixture = mixture0
        # cached: one streaming pass over the cache (kept current by
        # _graph_label_update's one-class refresh)
        h_after = None if acq.cache is None else pops.pair_cache_h_after(
            acq.cache, acq.ps, pi, rows, mixture0)
        # H_before enters as an in-graph tensor op (the kernel's scalar
        # argument would be frozen at capture value)
        q0 = pops.eig_pairs(self._tables, acq.ps, acq.cls_rows, rows, pi,
                            mixture0, None, self._adjusted, self._row_sums,
                            h_after=h_after)
        # fused epilogue: qbuf = active ? H0 + q0 : -inf; out =
        # [masked max, first argmax, isclose tie count].  Replaces the
        # ~10-launch torch chain (where/max/isclose/sum/copies,
        # ~120 us/step at B=50k); torch.isclose on finite and infinite
        # values, NaN skipped (tests/acq_ref.py is the contract) - when
        # the tie count is 1 the argmax is unique, and ties go through
        # the seeded host random.choice either way (_acq_result).
        # A run that asked for a batch also gets the (1024,) rank-ordered
        # slots (acq.topk_args(); empty otherwise - today's three kernels)
        ops._ext.acq_select(q0.contiguous(), H0.reshape(1).contiguous(),
                            acq.active, acq.qbuf, acq.out, acq.ties,
                            *acq.topk_args())

    def _acq_result(self):
        idx, q, tied = self._pair_acq.result()
        self.stochastic |= tied
        return idx, q

    def _acq_eligible(self) -> bool:
        return (self.q == "eig" and self._pair_acq is not None
                and self._pair_acq.ps.vmask is not None
                and not DEBUG_VIZ
                and not (self.prefilter_n
                         and len(self._active_candidates)
                         > self.prefilter_n))

    def _graphed_acquire(self, read=None):
        read = read or self._acq_result
        if self._acq_graph is None:
            self._sync_pair_cache()    # outside the capture
            self._acq_graph, first = _warm_and_capture(self._acq_body,
                                                       read)
            return first
        self._acq_graph.replay()
        return read()

    # ------------------------------------------------------------------
    def get_next_item_to_label(self):
        pending, self._acq_pending = self._acq_pending, None
        if pending is not None and self._acq_eligible():
            # the merged label+acquire graph already computed this
            # step's EIG/argmax during add_label
            return self._acq_result() if pending is _ON_DEVICE else pending
        if (self.q == "eig" and self._use_label_graph
                and self._label_graph is not None
                and self._acq_eligible()):
            return self._graphed_acquire()
        if self.q == "eig":
            q_vals, cand = self.eig_batched()
        elif self.q == "iid":
            cand = self._prefilter(self.unlabeled_idxs) or self.unlabeled_idxs
            q_vals = torch.full((len(cand),), 1.0 / len(cand),
                                device=self.device)
        elif self.q == "uncertainty":
            cand = self._prefilter(self.unlabeled_idxs) or self.unlabeled_idxs
            ens_sum = self.dataset.preds.sum(dim=0)
            self.comm.all_reduce_(ens_sum)
            ent = ops.entropy_acquisition(ens_sum / self.H)
            q_vals = ent[torch.tensor(list(cand), device=self.device)]
        else:
            raise NotImplementedError(self.q)

        if DEBUG_VIZ:  # per-step EIG bar chart (reference coda/coda.py:299-303)
            from ..util import plot_bar
            from .. import tracking
            try:
                tracking.log_image(plot_bar(q_vals, title="EIG"),
                                   key="EIG", step=self.step)
            except RuntimeError:
                pass  # no active tracking run

        # greedy with seeded random tie-breaking (coda/coda.py:306-313);
        # max/argmax/tie-count fetched in ONE device sync. The index and
        # count travel as a separate int64 pair (a float32 round-trip
        # corrupts indices beyond 2^24, i.e. pools over ~16.7M points).
        best_val, best_idx = q_vals.max(0)
        n_ties = torch.isclose(q_vals, best_val, rtol=1e-8).sum()
        bv, bi, nt = torch.stack(
            [best_val.double(), best_idx.double(),
             n_ties.double()]).cpu().tolist()
        bi, nt = int(bi), int(nt)
        if nt > 1:
            idx_local = tied_choice(q_vals, best_val)
            self.stochastic = True
            return cand[idx_local], float(q_vals[idx_local])
        return cand[int(bi)], bv

    # -- batch acquisition ---------------------------------------------
    def get_next_items_to_label(self, k, distinct: bool = True):
        """The k best unlabeled points to label next, best first, as
        [(point id, q value)]; fewer when fewer candidates compete.

        k == 1 is get_next_item_to_label(), wrapped: the seeded isclose
        tie-break, its RNG draws and the `stochastic` flag are the
        single-pick path's. k > 1 is deterministic: q descending, then
        position (= point id) ascending, so equal EIG values - the norm
        early in a run - need no draw, and neither the RNG nor
        `stochastic` is touched. With distinct (the default) at most one
        point per prediction pattern is returned: candidates on which
        all H models predict the same classes move the posterior the
        same way for any true class, so the best of each pattern stands
        for it (ops.reference.acq_topk is the rule; the captured pair
        path computes it inside the acquisition graph)."""
        k = int(k)
        if not 1 <= k <= ops.ACQ_TOPK_MAX:
            raise ValueError(f"k must lie in [1, {ops.ACQ_TOPK_MAX}], "
                             f"got {k}")
        if k == 1:
            return [self.get_next_item_to_label()]
        if self.q != "eig":
            raise NotImplementedError(self.q)
        if distinct and self.comm.is_distributed and not self._replicated:
            raise ValueError(
                "this process holds a shard of the model axis, so it "
                "cannot see prediction patterns: pass distinct=False")
        distinct = bool(distinct)
        acq = self._pair_acq
        if self._use_label_graph and self._acq_eligible():
            # the captured acquisition writes the batch itself. Whether
            # it does, and per pattern or not, is a capture-time choice
            # (k is not: the kernel fills all 1024 slots)
            if acq.enable_topk(distinct):
                self._drop_graphs()
            pending, self._acq_pending = self._acq_pending, None

            def read():
                return acq.result_topk(k)

            if pending is not None:
                # computed during add_label. The first label's warm-up
                # decoded its single pick to the host; the slots wait in
                # the device buffer either way (a capture records, it
                # does not run)
                return read()
            if self._label_graph is not None:
                return self._graphed_acquire(read)
        else:
            self._acq_pending = None
        # eager: CPU, the table engine, prefiltered subsets, distributed
        # ranks (every rank ranks the same gathered scores, so they agree
        # without a collective)
        q_vals, cand = self.eig_batched()
        cand = list(cand)
        group_of = None
        if distinct:
            group_of, _ = ops.group_rows(self._global_classes(
                torch.tensor(cand, dtype=torch.long, device=self.device)))
        pos, vals = ops.acq_topk(q_vals, None, group_of, k)
        return [(cand[p], v) for p, v in zip(pos.tolist(), vals.tolist())]

    def add_labels(self, idxs, classes, probs):
        """add_label for each of a batch's answers, in order. On the
        captured path each label still runs an acquisition (one merged
        graph), of which only the round's last is read."""
        for idx, y, p in zip(idxs, classes, probs):
            self.add_label(idx, y, p)

    # -- label update --------------------------------------------------
    def _posterior_update(self, y_t, col):
        """The part of a label update every path shares, on the (1,)
        int64 class tensor y_t and the labeled point's (Hl,) argmax
        classes: Dirichlet row add (K13), the exact rank-1 pi_hat
        increment with its row sums (only Dirichlet row y moved),
        all-reduced over shards, and the renormalized marginal, which is
        returned. Static shapes, y read on the device: it captures."""
        lr = self.update_strength
        on_hip = self.dirichlets.is_cuda and ops.hip_available()
        if on_hip:
            # H-thread scatter: torch's one_hot + dim-1 index_add_ on the
            # (H,C,C) posterior costs ~914 us for H real nonzeros
            # (matters on the eager path the distributed ranks take too)
            ops._ext.dirichlet_add(self.dirichlets, y_t, col, float(lr))
        else:
            onehot = torch.nn.functional.one_hot(col, self.C).to(
                self.dirichlets.dtype)
            self.dirichlets.index_add_(1, y_t, (lr * onehot).unsqueeze(1))
        delta = ops.pi_hat_delta(self.dataset.preds, col,
                                 preds_t=self._preds_t)          # (N,)
        if self.comm.is_distributed:    # never under capture
            self.comm.all_reduce_(delta)
        delta = delta * lr
        if on_hip:
            # fused column update (torch index_add_ over dim 1 with one
            # index runs ~90x slower than this elementwise pass)
            ops._ext.col_add(self._adjusted, self._row_sums, y_t, delta)
        else:
            self._adjusted.index_add_(1, y_t, delta.unsqueeze(1))
            self._row_sums += delta
        return self._pi_marginal()

    # Two ways to finish a label, on purpose. Captured (single device):
    # the tables are committed in-stream from the Dirichlets and the
    # posterior row is computed from the columns the commit kernel
    # returns. Eager (distributed ranks, graph-disabled runs, CPU): the
    # class is marked dirty for a lazy table_update_rows and the row
    # comes from torch sums over the Dirichlets or the replicated view.
    # The columns agree only to the last bits, so merging the two would
    # move the distributed trajectories.
    def _graph_label_update(self):
        """The tensor part of add_label as static-shape ops on the static
        input buffers self._g_idx / self._g_y (both (1,) int64). Writes
        tables in place and leaves the updated posterior rows in
        self._g_rows. Captured once into a hipGraph."""
        y_t = self._g_y
        col = self.classes.index_select(1, self._g_idx).squeeze(1)  # (Hl,)
        self._g_pi.copy_(self._posterior_update(y_t, col))
        a_col, b_col = tops.table_commit_row(self._tables, self.dirichlets,
                                             y_t)
        acq = self._pair_acq
        if acq is not None and acq.cache is not None:
            # class y's table rows just moved: re-evaluate its run of
            # pairs (commit -> refresh -> entropy pass, in stream order;
            # y is read on the device, so this captures)
            pops.pair_cache_refresh(acq.cache, self._tables, acq.ps,
                                    acq.cls_rows, y_t)
        # posterior rows: add_label moves only Dirichlet row y, so only
        # class y's Beta column - hence only pbest row y - changes.
        # _g_rows was seeded with the full (C, Hl) rows at graph init;
        # each label refreshes one row (was a full C-row recompute,
        # 103 us/step at C=1000).
        rows_y = ops.pbest_from_beta(a_col.unsqueeze(0),
                                     b_col.unsqueeze(0),
                                     self.num_points)        # (1, Hl)
        self._g_rows.index_copy_(0, y_t, rows_y)

    def _graphed_add_label(self, idx: int, y: int):
        first = self._label_graph is None
        if first:
            self._sync_pair_cache()    # outside the capture
            self._acq_graph = None     # captured on the buffers below
            self._g_idx = torch.zeros(1, dtype=torch.long,
                                      device=self.device)
            self._g_y = torch.zeros(1, dtype=torch.long, device=self.device)
            self._g_pi = torch.empty_like(self.pi_hat)
            # seeded with the PRE-label rows; the graph body refreshes
            # only the labeled class's row per replay
            self._g_rows = self._pbest_rows_before().clone().contiguous()
            # When the full-pool pair acquisition is active, the NEXT
            # step's acquisition is captured INTO the label graph: one
            # replay per step computes posterior update + next EIG +
            # argmax (the caller's get_next just reads the result).
            self._merged_acq = self._acq_eligible()
        self._g_idx.fill_(idx)
        self._g_y.fill_(y)
        pending = _ON_DEVICE
        if first:
            def body():
                self._graph_label_update()
                if self._merged_acq:
                    self._acq_body()

            # the warm-up applies THIS label's update, so the first
            # label does not replay; its acquisition result, read before
            # the capture, serves the next get_next
            self._label_graph, pending = _warm_and_capture(
                body, self._acq_result if self._merged_acq else None)
            # the capture rebound it to the graph's buffer, which the
            # first replay fills: nothing to serve for this label
            self._label_mixture = (self._acq_mixture if self._merged_acq
                                   else None)
        else:
            self._label_graph.replay()
            if self._label_mixture is not None:
                # the replay's acquisition half computed the mixture of
                # the rows and pi_hat it has just updated
                self._mixture_cache = (self._posterior_version + 1,
                                       self._label_mixture)
        self.pi_hat = self._g_pi
        self._pi_xi_cache = None
        self._pbest_rows_cache = (self._posterior_version + 1,
                                  self._g_rows)
        self._acq_pending = pending if self._merged_acq else None

    def _eager_add_label(self, idx: int, y: int):
        y_t = torch.tensor([y], dtype=torch.long, device=self.device)
        self.pi_hat = self._posterior_update(
            y_t, self.classes[:, idx].contiguous())
        self._pi_xi_cache = None
        if self._replicated:
            # keep the replicated global Beta view current - a local
            # elementwise update from the (gathered-once) global classes,
            # identical on every rank, no collective
            hit = self.classes_global[:, idx].long() == y
            self._alpha_g[:, y] += self.update_strength * hit.float()
            self._beta_g[:, y] += self.update_strength * (~hit).float()
        self._tables_dirty.add(y)
        # incremental posterior rows on the EAGER path too (the
        # distributed ranks and graph-disabled runs): only class y's
        # Beta column moved, so refresh one row instead of the full
        # (C, H) recompute (~300 us/step at C=1000) the version-keyed
        # cache would otherwise trigger.  Valid whenever this process
        # holds the full model axis (single device or replicated mode);
        # the H-sharded v2 path keeps the sharded recompute.
        ver, cached = self._pbest_rows_cache
        if (cached is not None and ver == self._posterior_version
                and (self._replicated or not self.comm.is_distributed)):
            if self._replicated:
                a_col = self._alpha_g[:, y].contiguous()
                b_col = self._beta_g[:, y].contiguous()
            else:
                row = self.dirichlets[:, y, :]
                a_col = row[:, y].contiguous()
                b_col = (row.sum(-1) - a_col).contiguous()
            rows = cached.clone()
            rows[y] = ops.pbest_from_beta(
                a_col.unsqueeze(0), b_col.unsqueeze(0),
                self.num_points)[0]
            self._pbest_rows_cache = (self._posterior_version + 1, rows)

    def add_label(self, idx, true_class, selection_prob):
        """Posterior update (K13) + incremental pi_hat refresh.

        Reference semantics (coda/coda.py:315-323). On single-device GPU
        the whole tensor pipeline replays as one hipGraph."""
        idx, y = int(idx), int(true_class)
        # the candidate mask update must be enqueued BEFORE the replay:
        # the merged graph's acquisition half reads it
        self._deactivate(idx)
        if (self._use_label_graph and self._tables is not None
                and not self._tables_dirty):
            self._graphed_add_label(idx, y)
        else:
            self._eager_add_label(idx, y)
        self._posterior_version += 1
        self.labeled_idxs.append(idx)
        self.labels.append(y)
        self.q_vals.append(selection_prob)
        self.unlabeled_idxs.remove(idx)

    def _deactivate(self, idx: int):
        """Remove a point from the candidate pool (labeled or skipped).
        An acquisition computed before that may select it: a pending
        result is dropped here, for every caller."""
        self._acq_pending = None
        self._mixture_cache = (-1, None)
        try:
            self._active_candidates.remove(idx)
        except ValueError:
            pass  # point was not a disagreeing candidate
        if self._pair_acq is not None:
            self._pair_acq.deactivate(idx)

    def skip(self, idx):
        """Drop a point without labeling it (the demo's "I don't know"
        path, reference demo/app.py:188-189)."""
        idx = int(idx)
        if idx in self.unlabeled_idxs:
            self.unlabeled_idxs.remove(idx)
        self._deactivate(idx)

    # ------------------------------------------------------------------
    def get_pbest(self):
        """Marginal P(best) over models (K15): (H,) in GLOBAL model order."""
        ver, mix = self._mixture_cache
        if (mix is not None and ver == self._posterior_version
                and not self.comm.is_distributed):
            # the merged label+acquire graph already ran these kernels
            # on these rows and this pi_hat: same bits, one copy
            marg_local = mix.clone()
        else:
            rows = self._pbest_rows_before()  # (C, Hl) / (C, H) replicated
            # ops.mixture_entropy's column-sum kernel; the torch
            # reduction over C launches 32 threads (~22 us at C=1000)
            marg_local = ops.mixture_entropy(rows, self.pi_hat)[0]
        if self.comm.is_distributed and not self._replicated:
            gathered = self.comm.all_gather_cat(marg_local, dim=0)
            pbest = gathered[self.comm.unshard_order(self.H).to(gathered.device)]
        else:
            pbest = marg_local
        if DEBUG:
            _check(pbest, "Pbest")
        return pbest

    def get_best_model_prediction(self):
        pbest = self.get_pbest()
        if DEBUG_VIZ:  # reference coda/coda.py:337-341
            from ..util import plot_bar
            from .. import tracking
            try:
                tracking.log_image(plot_bar(pbest, title="PBest"),
                                   key="PBest", step=self.step)
            except RuntimeError:
                pass
        self.step += 1
        return torch.argmax(pbest)
