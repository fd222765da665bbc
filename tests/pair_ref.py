"""fp64 stage references for the v3 pair engine (not itself a test).

Each function is the CONTRACT of one kernel in coda_amd/ops/hip/pair.hip,
written in plain torch on CPU tensors and evaluated in fp64. The
quantised operands the design chose (fp16 delta table, fp32 dall, bf16 A
and egw) are INPUTS here, so what separates a kernel from its reference
is fp32 arithmetic noise only - two to three orders of magnitude below
the end-to-end bf16 tolerance, and below what a single indexing mistake
moves (tests/test_pair.py::TestToleranceFloors).

`f32` / `m_f32` re-run the same reference with every operation rounded
to fp32 in a fixed order (emulated in fp64, so all hosts agree): that
is how the stage tolerances are measured (fp32-vs-fp64 of the reference
itself, never kernel output). The keyword-only `col_keep`, `hit_keep` and
`base_cols` arguments inject the faults of the mutation-floor tests.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import torch

from coda_amd.ops import pair as pops
from coda_amd.ops import reference as R
from coda_amd.ops import table as tops

F32_MIN_NORMAL = 2.0 ** -126      # smallest normal float32
BF16_ULP_REL = 2.0 ** -7          # one bf16 ulp, relative upper bound


def _f32c(x: float, dtype) -> torch.Tensor:
    """A kernel float literal (1e-12f, 1e-30f) at its fp32 value."""
    return torch.tensor(x, dtype=torch.float32).to(dtype)


# ---------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------

def consensus_classes(H: int, N: int, C: int, p: float,
                      seed: int) -> torch.Tensor:
    """(N, H) int64 argmax rows of a consensus-heavy pool: every point
    has a "true" class, each model predicts it with probability p and a
    uniform class otherwise. p = 0 is the independent case; p >= 0.5
    gives most candidates a majority (complement-segment) pair."""
    g = torch.Generator().manual_seed(seed)
    true = torch.randint(0, C, (N, 1), generator=g)
    agree = torch.rand(N, H, generator=g) < p
    unif = torch.randint(0, C, (N, H), generator=g)
    return torch.where(agree, true.expand(N, H), unif)


class Problem(NamedTuple):
    H: int
    N: int
    C: int
    cls_rows: torch.Tensor      # (B, H) int64
    ps: pops.PairStructure
    tables: tops.EigTables      # CPU, with egw / delta16 / dall attached
    pi_hat: torch.Tensor        # (C,)
    pbest_before: torch.Tensor  # (C, H)
    mixture0: torch.Tensor      # (H,)
    H_before: torch.Tensor      # ()
    adjusted: torch.Tensor      # (N, C)
    row_sums: torch.Tensor      # (N,)


@functools.lru_cache(maxsize=None)
def make_problem(H: int, N: int, C: int, p: float, seed: int = 0,
                 tile: int = 0, with_vmask: bool = True,
                 stride: int = 1) -> Problem:
    """One seeded pair-engine problem, tables built on the CPU.

    Heavy-diagonal Dirichlets give the delta curves a realistic range.
    stride > 1 takes the candidate subset ids[1::stride] of the N
    points. Cached: callers share the result and must not modify it.
    """
    g = torch.Generator().manual_seed(1000 + seed)
    eye = torch.eye(C)
    dirichlets = (torch.rand(H, C, C, generator=g) * 3 + 0.5
                  + eye * torch.rand(H, C, 1, generator=g) * 20)
    # keep every diagonal Beta bounded on the grid (alpha >= 1,
    # beta >= 2): a pdf that is singular at 0 or 1 makes the 256-point
    # trapezoid cdf miss 1 by percents PER MODEL, and a majority pair
    # multiplies hundreds of those - tot leaves O(1) (inf at H = 2048)
    dirichlets = dirichlets + 0.5 * eye + (1 - eye) * 1.5 / (C - 1)
    pi_hat = torch.rand(C, generator=g) + 0.2
    pi_hat /= pi_hat.sum()
    adjusted = torch.rand(N, C, generator=g) + 0.1
    row_sums = adjusted.sum(-1)
    alpha_cc, beta_cc = R.dirichlet_to_beta(dirichlets)
    tables = pops.attach_pair_tables(
        tops.table_precompute(alpha_cc, beta_cc))
    pbest_before = R.pbest_from_beta(alpha_cc.t().contiguous(),
                                     beta_cc.t().contiguous())
    mixture0, H_before = R.mixture_entropy(pbest_before, pi_hat)
    cls = consensus_classes(H, N, C, p, seed)
    ids = torch.arange(N)
    if stride > 1:
        ids = ids[1::stride]
    cls_rows = cls[ids].contiguous()
    ps = pops.build_pairs(cls_rows, ids, C, tile=tile,
                          with_vmask=with_vmask)
    return Problem(H, N, C, cls_rows, ps, tables, pi_hat, pbest_before,
                   mixture0, H_before, adjusted, row_sums)


def vbits_from_cls(cls_rows: torch.Tensor,
                   ps: pops.PairStructure) -> torch.Tensor:
    """(K, H) bool v-select: model h predicts class c_k on the pair's
    candidate. Base and pad pairs (pair_b = -1) get all-zero rows."""
    pb = ps.pair_b.long()
    hit = cls_rows.long()[pb.clamp_min(0)] == ps.pair_c.long().unsqueeze(1)
    return hit & (pb >= 0).unsqueeze(1)


def vbits_from_vmask(vmask: torch.Tensor, H: int) -> torch.Tensor:
    """Decode the (K, ceil(H/32)) int32 bitmask to (K, H) bool."""
    h = torch.arange(H)
    words = vmask.long()[:, h >> 5]
    return ((words >> (h & 31)) & 1).bool()


# ---------------------------------------------------------------------
# stage 1: A operand
# ---------------------------------------------------------------------

def ref_dsum(delta: torch.Tensor, dall: torch.Tensor,
             ps: pops.PairStructure, chunk: int = 8192) -> torch.Tensor:
    """(K, P) fp64 dsum[k] = sum_{h in seg(k)} delta[c_k, h], and
    dall[c_k] - that sum for complement (pair_neg) pairs. The table
    (fp16 or fp32) and the fp32 dall are taken as given."""
    K, P = ps.K, delta.shape[-1]
    pc = ps.pair_c.long()
    seg_len = (ps.seg_off[1:] - ps.seg_off[:-1]).long()
    seg_pair = torch.repeat_interleave(torch.arange(K), seg_len)
    seg_h = ps.seg_h.long()
    dsum = torch.zeros(K, P, dtype=torch.float64)
    for s0 in range(0, seg_h.numel(), chunk):
        sp = seg_pair[s0:s0 + chunk]
        dsum.index_add_(0, sp, delta[pc[sp], seg_h[s0:s0 + chunk]].double())
    neg = ps.pair_neg.bool()
    dsum[neg] = dall.double()[pc[neg]] - dsum[neg]
    return dsum


def ref_dsum_es(delta16: torch.Tensor, dall: torch.Tensor,
                ps: pops.PairStructure) -> torch.Tensor:
    """(K, P) bf16 = bf16(float32(exp2(dsum))), dsum exact in fp64."""
    return torch.exp2(ref_dsum(delta16, dall, ps)).float().to(
        torch.bfloat16)


def a_operand_ok(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """(K, P) bool: element within one bf16 ulp of the reference
    (relative 2^-7, absolute floor at the smallest normal f32); where
    the reference is below that floor the value must be too."""
    g, r = got.double(), ref.double()
    ok = (g - r).abs() <= torch.maximum(
        BF16_ULP_REL * r.abs(), torch.tensor(F32_MIN_NORMAL).double())
    ok = torch.where(r < F32_MIN_NORMAL, g <= F32_MIN_NORMAL, ok)
    return ok & torch.isfinite(g)


def a_operand_check(got: torch.Tensor, ref: torch.Tensor):
    """(n_bad, share): elements outside a_operand_ok, and the share of
    elements that differ from the reference at all (values at or below
    the f32 floor on both sides count as equal)."""
    g, r = got.double(), ref.double()
    both_tiny = (r < F32_MIN_NORMAL) & (g <= F32_MIN_NORMAL)
    diff = (g != r) & ~both_tiny
    return int((~a_operand_ok(got, ref)).sum()), float(diff.double().mean())


# ---------------------------------------------------------------------
# stage 2: pairing GEMM + v-select + entropy
# ---------------------------------------------------------------------

def _r32(x: torch.Tensor) -> torch.Tensor:
    """Round an fp64 tensor to the nearest fp32 value (kept in fp64)."""
    return x.float().double()


def _same(x: torch.Tensor) -> torch.Tensor:
    return x


def _sum32(x: torch.Tensor, lanes: int) -> torch.Tensor:
    """fp32 sum over the last axis in ONE fixed order: `lanes` strided
    accumulators walk the axis, then combine pairwise; every add is
    rounded to fp32. Carried out in fp64 with explicit rounding, so
    every host gets the same bits (a torch fp32 matmul or sum does not:
    BLAS blocking, vector width and thread count moved the fp32-vs-fp64
    spread by up to 2.8x between two machines)."""
    n = x.shape[-1]
    if n % lanes:
        x = torch.cat([x, x.new_zeros(*x.shape[:-1], lanes - n % lanes)], -1)
    x = x.reshape(*x.shape[:-1], -1, lanes)
    acc = x[..., 0, :]
    for s in range(1, x.shape[-2]):
        acc = _r32(acc + x[..., s, :])
    while acc.shape[-1] > 1:
        acc = _r32(acc[..., 0::2] + acc[..., 1::2])
    return acc[..., 0]


def _gemm32(a: torch.Tensor, b: torch.Tensor, lanes: int) -> torch.Tensor:
    """(k, P) x (J, P)^T with fp32 FMA accumulation in _sum32's order
    (a product of two bf16 values is exact)."""
    acc = torch.zeros(a.shape[0], b.shape[0], lanes, dtype=torch.float64)
    for s in range(0, a.shape[1], lanes):
        acc = _r32(acc + a[:, None, s:s + lanes] * b[None, :, s:s + lanes])
    while acc.shape[-1] > 1:
        acc = _r32(acc[..., 0::2] + acc[..., 1::2])
    return acc[..., 0]


def ref_select(a16, egw, vbits, pair_c, round_m=False, *, m_f32=False,
               lanes=8, col_keep=None):
    """(K, H) selected M[k, 2h + v] with M = A . egw[c]^T, class by
    class (no (K, 2H, P) gather). m_f32 accumulates M in emulated fp32
    (`lanes` picks the summation order); round_m rounds M to bf16 (the
    wide routes store it)."""
    K, H = vbits.shape
    pc = pair_c.long()
    j = 2 * torch.arange(H).unsqueeze(0) + vbits.long()
    pb = torch.zeros(K, H, dtype=torch.float64)
    for c in torch.unique(pc).tolist():
        idx = (pc == c).nonzero().squeeze(1)
        a, b = a16[idx].double(), egw[c].double()
        M = _gemm32(a, b, lanes) if m_f32 else a @ b.t()     # (k, 2H)
        if round_m:
            M = M.to(torch.bfloat16).double()
        if col_keep is not None:
            M = M * col_keep.double()
        pb[idx] = M.gather(1, j[idx])
    return pb


def ref_entropy(pb, pair_c, pi_hat, pbest_before, mixture0, *,
                f32=False, lanes=8):
    """(K,) entropy epilogue from the selected (K, H) values: normalise
    with the 1e-30 clamp, mix, clamp at 1e-12, -sum m log2 m. f32
    rounds every operation to fp32."""
    R = _r32 if f32 else _same
    total = (lambda x: _sum32(x, lanes)) if f32 else (lambda x: x.sum(-1))
    pc = pair_c.long()
    tot = total(pb).unsqueeze(-1).clamp_min(_f32c(1e-30, torch.float64))
    d = R(R(pb / tot) - pbest_before.double()[pc])
    mm = R(mixture0.double().unsqueeze(0)
           + R(pi_hat.double()[pc].unsqueeze(1) * d))
    mm = mm.clamp_min(_f32c(1e-12, torch.float64))
    return -total(R(mm * R(torch.log2(mm))))


def ref_gemm_entropy(a16, egw, vbits, pair_c, pi_hat, pbest_before,
                     mixture0, round_m=False, *, f32=False, m_f32=None,
                     lanes=8, col_keep=None):
    """(K,) h_after of pair_gemm_entropy / pair_gemm_entropy_cls from
    the bf16 operand VALUES, in fp64 (or its fp32 twin: f32)."""
    m_f32 = f32 if m_f32 is None else m_f32
    pb = ref_select(a16, egw, vbits, pair_c, round_m, m_f32=m_f32,
                    lanes=lanes, col_keep=col_keep)
    return ref_entropy(pb, pair_c, pi_hat, pbest_before, mixture0,
                       f32=f32, lanes=lanes)


# ---------------------------------------------------------------------
# stage 3: per-candidate assembly
# ---------------------------------------------------------------------

def ref_finalize(h_after, ps: pops.PairStructure, adjusted, row_sums,
                 H_before, *, f32=False, lanes=8, hit_keep=None,
                 base_cols=None):
    """(B,) q[b] = H_before - (arow . h_base + sum_{hits of b}
    arow[c] (h_after[k] - h_base[c])) / max(row_sums, 1e-12), one value
    per structure candidate row (pair_eig_finalize's contract)."""
    R = _r32 if f32 else _same
    total = (lambda x: _sum32(x, lanes)) if f32 else (lambda x: x.sum(-1))
    ha = h_after.double()
    h_base = ha[ps.base_pos]
    ids = ps.cand_ids
    B = ids.shape[0]
    inv = R(1.0 / row_sums[ids].double().clamp_min(
        _f32c(1e-12, torch.float64)))
    a = adjusted[ids].double()                               # (B, C)
    nb = a.shape[1] if base_cols is None else base_cols
    base = total(R(a[:, :nb] * h_base[:nb])) if nb else torch.zeros(
        B, dtype=torch.float64)
    counts = (ps.cand_off[1:] - ps.cand_off[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(B), counts)
    pos = torch.arange(rows.numel()) - ps.cand_off[:-1].long()[rows]
    k = ps.cand_pairs.long()
    c_v = ps.pair_c.long()[k]
    term = R(a[rows, c_v] * R(ha[k] - h_base[c_v]))
    if hit_keep is not None:
        term = term * hit_keep.double()
    hits = torch.zeros(B, max(int(counts.max()), 1), dtype=torch.float64)
    hits[rows, pos] = term
    return R(float(H_before) - R(R(base + total(hits)) * inv))


# worst-case relative error of an fp32 sum of P non-negative terms, in
# ANY order (gamma_P ~ P * 2^-24): both pairing-GEMM operands are >= 0
FP32_SUM_NOISE = 256 * 2.0 ** -24


def flip_allowance(a16, egw, vbits, pair_c, pi_hat, pbest_before,
                   mixture0, rel_noise: float = FP32_SUM_NOISE):
    """(K,) h_after slack owed to bf16 rounding FLIPS on the wide routes.

    The wide kernels store M as bf16. An fp32-accumulated entry that
    lies within rel_noise of the midpoint between two bf16 neighbours
    may legitimately round to the OTHER neighbour than the fp64 value
    does, and one flip of a dominant model's entry moves h_after by up
    to 2e-3 - as much as an indexing fault. A scalar tolerance can
    therefore be tight or safe, not both. This returns, per pair, the
    sum over its at-risk entries of the h_after move that flipping that
    entry causes (exact re-evaluation in fp64); pairs without an
    at-risk entry get 0 and are held to the fp32 noise tolerance
    alone.
    """
    assert float(a16.float().min()) >= 0 and float(egw.float().min()) >= 0
    pb64 = ref_select(a16, egw, vbits, pair_c)               # unrounded
    r = pb64.to(torch.bfloat16).double()
    base = ref_entropy(r, pair_c, pi_hat, pbest_before, mixture0)
    e = torch.floor(torch.log2(r.clamp_min(1e-300)))
    up = torch.exp2(e - 7)
    down = torch.where(r == torch.exp2(e), up / 2, up)
    other = torch.where(pb64 >= r, r + up, r - down)
    risk = ((pb64 - (r + other) / 2).abs() <= rel_noise * pb64) & (r > 0)
    k_i, h_i = risk.nonzero(as_tuple=True)
    allow = torch.zeros(pb64.shape[0], dtype=torch.float64)
    for s0 in range(0, k_i.numel(), 4096):
        kk, hh = k_i[s0:s0 + 4096], h_i[s0:s0 + 4096]
        pb2 = r[kk].clone()
        pb2[torch.arange(kk.numel()), hh] = other[kk, hh]
        moved = ref_entropy(pb2, pair_c[kk], pi_hat, pbest_before,
                            mixture0)
        allow.index_add_(0, kk, (moved - base[kk]).abs())
    return allow


class FinalizeInputs(NamedTuple):
    ps: pops.PairStructure
    h_after: torch.Tensor       # (K,) synthetic, uniform in [3, 3.5]
    adjusted: torch.Tensor      # (N, C)
    row_sums: torch.Tensor      # (N,)
    H_before: float
    tiny_row: int               # structure row whose row_sums < 1e-12


@functools.lru_cache(maxsize=None)
def make_finalize_inputs(H: int, N: int, C: int, p: float,
                         stride: int = 1, seed: int = 0) -> FinalizeInputs:
    """Inputs for pair_eig_finalize alone: a tile-16 structure over a
    consensus pool and synthetic per-pair entropies, so q = H_before -
    (weighted mean of h) lies in [0.4, 1] (2.4 on the clamped row).
    row_sums is NOT the row sum of adjusted (a kernel that recomputed
    it would differ), and the first candidate's row is scaled to a sum
    below the 1e-12 clamp."""
    g = torch.Generator().manual_seed(2000 + seed)
    cls = consensus_classes(H, N, C, p, seed)
    ids = torch.arange(N)
    if stride > 1:
        ids = ids[1::stride]
    ps = pops.build_pairs(cls[ids].contiguous(), ids, C, tile=16)
    h_after = torch.rand(ps.K, generator=g) * 0.5 + 3.0
    adjusted = torch.rand(N, C, generator=g) + 0.1
    row_sums = adjusted.sum(-1) * (0.95 + 0.1 * torch.rand(N, generator=g))
    tiny = int(ids[0])
    adjusted[tiny] *= 5e-13 / adjusted[tiny].sum()
    row_sums[tiny] = 5e-13
    return FinalizeInputs(ps, h_after, adjusted, row_sums, 4.0, 0)
