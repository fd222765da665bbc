"""fp64 stage references for the v2 table engine (not itself a test).

Each function is the CONTRACT of one kernel of the table path in
coda_amd/ops/hip/table.hip (es_build*, eig_assemble_k, eig_totals,
eig_entropy, beta_row_tables, table_commit_*), written in plain torch on
CPU tensors and evaluated in fp64 on exactly the tensors the kernel
receives: the fp32 tables, the fp32 dall and a bf16 M are INPUTS, so
what separates a kernel from its reference is fp32 arithmetic noise.

`f32=True` re-runs the same reference with every operation rounded to
fp32 in a fixed order (emulated in fp64 like tests/pair_ref.py, so all
hosts agree): fp32-twin-vs-fp64 of the reference itself is how the
stage tolerances of tests/test_table_kernels.py are measured, never
kernel output. The keyword-only fault arguments (`drop_last`, `comp_ge`,
`drop_quarter`, `vflip`, `swap_v`, `lane0_trapezoid`) inject the faults
of the mutation-floor tests in tests/test_table_ref.py.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import torch

from coda_amd.ops import table as tops
from coda_amd.ops.reference import GRID_HI, GRID_LO
from tests import pair_ref as PR
from tests.pair_ref import _f32c, _r32, _same, _sum32

P = 256
ES_LONG_ROW = 512                 # table.hip: rows above go block-per-row
LOG2E = 1.4426950408889634
# branch codes of an es_build row: bit 0 = complement, bit 1 = long
DIRECT_SHORT, COMP_SHORT, DIRECT_LONG, COMP_LONG = 0, 1, 2, 3
BRANCH_NAMES = ("direct-short", "complement-short", "direct-long",
                "complement-long")
# The synthetic dall is NOT the sum of delta: it is skewed by this
# constant, so a row evaluated through the wrong branch (complement for
# direct or the reverse) is off by 2^(1/16) - 1 = 4.4e-2 relative. With
# a consistent dall both forms are the same number and neither the
# threshold `n > H / 2` nor the two kernels' agreement on it could be
# seen by any value check.
DALL_SKEW = 2.0 ** -4
# smallest |delta| of the synthetic tables: one model more or less in a
# bucket moves the row by at least 1 - 2^-DELTA_FLOOR = 1.08e-2 relative
DELTA_FLOOR = 2.0 ** -6


def grid_weights() -> torch.Tensor:
    """(P,) fp32 trapezoid weights exactly as table_precompute builds
    them."""
    x = torch.linspace(GRID_LO, GRID_HI, P, dtype=torch.float64)
    dx = float(x[1] - x[0])
    w = torch.full((P,), dx)
    w[0] = w[-1] = 0.5 * dx
    return w


# ---------------------------------------------------------------------
# es_build / es_build_gathered
# ---------------------------------------------------------------------

def _rows_sum(rows: torch.Tensor, f32: bool, lanes: int) -> torch.Tensor:
    """(n, P) -> (P,) sum over the rows (fp64, or the fp32 twin with
    `lanes` strided accumulators)."""
    rows = rows.double()
    if rows.shape[0] == 0:
        return torch.zeros(rows.shape[1], dtype=torch.float64)
    if not f32:
        return rows.sum(0)
    return _sum32(rows.t().contiguous(), lanes)


def es_branch(n: int, H: int, comp_ge: bool = False):
    """(complement?, effective length, branch code) of a bucket of n
    models: the kernels' rule `n > H / 2` in integer division."""
    comp = n >= H // 2 if comp_ge else n > H // 2
    eff = H - n if comp else n
    return comp, eff, int(comp) + 2 * int(eff > ES_LONG_ROW)


def ref_es_build(s_base, delta, dall, hvals, offsets, w, *, f32=False,
                 drop_last=False, comp_ge=False, drop_quarter=None,
                 no_complement=False):
    """ES (C, B, P) fp64 = 2^(s_base[c] + dsum) * w and the (B, C)
    branch code of each row. dsum is the sum of delta[c, h] over the
    bucket hvals[b, k0:k1], or dall[c] minus the sum over the positions
    OUTSIDE [k0, k1) when the bucket holds more than H // 2 models.

    Faults: drop_last leaves the last summed model out; comp_ge takes
    the complement at n >= H // 2; drop_quarter = q leaves out the q-th
    of the four contiguous slices a long row is split into.
    no_complement sums every bucket directly (for the CPU check that
    both forms agree; the branch codes stay the kernels')."""
    R = _r32 if f32 else _same
    C, H, _ = delta.shape
    B = hvals.shape[0]
    es = torch.zeros(C, B, P, dtype=torch.float64)
    branch = torch.zeros(B, C, dtype=torch.int64)
    for b in range(B):
        for c in range(C):
            k0, k1 = int(offsets[b, c]), int(offsets[b, c + 1])
            comp, eff, code = es_branch(k1 - k0, H, comp_ge)
            branch[b, c] = code
            comp = comp and not no_complement
            pos = torch.arange(k0, k1)
            if comp:
                pos = torch.cat([torch.arange(0, k0), torch.arange(k1, H)])
            if drop_last:
                pos = pos[:-1]
            if drop_quarter is not None and code >= DIRECT_LONG:
                per = (eff + 3) // 4
                keep = torch.ones(pos.numel(), dtype=torch.bool)
                keep[drop_quarter * per:(drop_quarter + 1) * per] = False
                pos = pos[keep]
            hs = hvals[b].long()[pos]
            dsum = _rows_sum(delta[c, hs], f32,
                             8 if code >= DIRECT_LONG else 2)
            if comp:
                dsum = R(dall[c].double() - dsum)
            es[c, b] = R(R(torch.exp2(R(s_base[c].double() + dsum)))
                         * w.double())
    return es, branch


def ref_es_build_gathered(s_base_all, sel_all, hvals, offsets, w, *,
                          f32=False, drop_last=False):
    """ES (C, B, P) fp64 = 2^(s_base_all[c] + sum_{k in bucket}
    sel_all[b, hvals[b, k]]) * w. No complement."""
    R = _r32 if f32 else _same
    C = s_base_all.shape[0]
    B = hvals.shape[0]
    es = torch.zeros(C, B, P, dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            k0, k1 = int(offsets[b, c]), int(offsets[b, c + 1])
            hs = hvals[b].long()[k0:k1 - 1 if drop_last else k1]
            dsum = _rows_sum(sel_all[b, hs], f32, 4)
            es[c, b] = R(R(torch.exp2(R(s_base_all[c].double() + dsum)))
                         * w.double())
    return es


# ---------------------------------------------------------------------
# eig_assemble_k / eig_totals / eig_entropy
# ---------------------------------------------------------------------

def ref_select(M, cls, *, vflip=None) -> torch.Tensor:
    """(B, C, H) fp64 selected M[c, b, 2h + v], v = [cls[b, h] == c].
    vflip: (B, C) model index whose v bit is inverted (fault)."""
    C, B, H2 = M.shape
    H = H2 // 2
    v = cls.long().unsqueeze(1) == torch.arange(C).view(1, C, 1)  # (B,C,H)
    if vflip is not None:
        v = v.clone()
        bb, cc = torch.meshgrid(torch.arange(B), torch.arange(C),
                                indexing="ij")
        v[bb, cc, vflip] ^= True
    j = 2 * torch.arange(H).view(1, 1, H) + v.long()
    return M.double().permute(1, 0, 2).gather(2, j)


def ref_totals(M, cls, *, f32=False, lanes=8, vflip=None) -> torch.Tensor:
    """(B, C) sum over h of the selected entries (unclamped)."""
    sel = ref_select(M, cls, vflip=vflip)
    return _sum32(sel, lanes) if f32 else sel.sum(-1)


def ref_entropy(M, cls, totals, pi_hat, pbest_before, mixture0, *,
                f32=False, lanes=8, vflip=None) -> torch.Tensor:
    """(B, C) -sum_h m log2 m with m = max(mixture0 + pi_c (pb -
    pbest_before[c]), 1e-12f), pb = selected / max(totals, 1e-30f)."""
    R = _r32 if f32 else _same
    total = (lambda x: _sum32(x, lanes)) if f32 else (lambda x: x.sum(-1))
    sel = ref_select(M, cls, vflip=vflip)
    inv = R(1.0 / totals.double().clamp_min(
        _f32c(1e-30, torch.float64))).unsqueeze(-1)
    d = R(R(sel * inv) - pbest_before.double().unsqueeze(0))
    mm = R(mixture0.double().view(1, 1, -1)
           + R(pi_hat.double().view(1, -1, 1) * d))
    mm = mm.clamp_min(_f32c(1e-12, torch.float64))
    return -total(R(mm * R(torch.log2(mm))))


def ref_assemble(M, cls, pi_hat, pbest_before, mixture0, *, f32=False,
                 lanes=8, vflip=None) -> torch.Tensor:
    """h_after (B, C) of eig_assemble_k: ref_totals, then ref_entropy."""
    tot = ref_totals(M, cls, f32=f32, lanes=lanes, vflip=vflip)
    return ref_entropy(M, cls, tot, pi_hat, pbest_before, mixture0,
                       f32=f32, lanes=lanes, vflip=vflip)


# ---------------------------------------------------------------------
# beta_row_tables / table_commit_*
# ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _grid():
    """x (P,), log2 x, log2(1 - x) in fp64 as LaneGrid::init walks the
    grid, the fp32 step, and the per-group-of-four anchors/deltas."""
    step = (GRID_HI - GRID_LO) / (P - 1)
    x = GRID_LO + torch.arange(P, dtype=torch.float64) * step
    lx, l1mx = torch.log2(x), torch.log2(1.0 - x)
    lx0 = lx[0::4].repeat_interleave(4)
    l1mx0 = l1mx[0::4].repeat_interleave(4)
    dxf = float(torch.tensor(step, dtype=torch.float64).float())
    return lx, l1mx, lx0, l1mx0, _r32(lx - lx0), _r32(l1mx - l1mx0), dxf


def _scan32(local: torch.Tensor) -> torch.Tensor:
    """Inclusive fp32 scan over the last axis (64 lanes), log-step."""
    v = local
    off = 1
    while off < v.shape[-1]:
        shifted = torch.cat([torch.zeros_like(v[..., :off]),
                             v[..., :-off]], -1)
        v = torch.cat([v[..., :off], _r32(v + shifted)[..., off:]], -1)
        off *= 2
    return v


def ref_beta_row_curves(alpha_col, beta_col, update_weight, *, f32=False,
                        swap_v=False, lane0_trapezoid=False):
    """(eg, lc), each (H, 2, P) fp64. Variant v0 = (a, b + w), v1 =
    (a + w, b), the sums rounded to fp32 as the kernel's operands are;
    t2 = base-2 log-pdf, cdf = trapezoid-cumulative pdf (fp32 step),
    lc = log2(max(cdf, 1e-30f)), eg = 2^(t2 - lc).

    The fp32 twin follows LaneGrid: the anchor K = (a-1) log2 x0 +
    (b-1) log2(1-x0) - log2 B in fp64 once per curve and group of four
    points, rounded to fp32; per-point fp32 FMAs on the fp32-rounded
    delta logs; fp32 trapezoids, lane sums and scan.

    Faults: swap_v exchanges the two variants; lane0_trapezoid counts a
    first trapezoid 0.5 (pdf[0] + pdf[3]) dx at lane 0 (what the
    shuffle hands lane 0 without the guard)."""
    uw = torch.tensor(float(update_weight), dtype=torch.float32)
    al, be = alpha_col.float(), beta_col.float()
    a = torch.stack([al, al + uw], -1)                          # (H, 2)
    b = torch.stack([be + uw, be], -1)
    if swap_v:
        a, b = a.flip(1), b.flip(1)
    t2, _, cdf = curves(a, b, f32, lane0_trapezoid=lane0_trapezoid)
    eps = _f32c(1e-30, torch.float64)
    if not f32:
        lc = torch.log2(cdf.clamp_min(eps))
        return torch.exp2(t2 - lc), lc
    lc = _r32(torch.log2(cdf.clamp_min(eps)))
    return _r32(torch.exp2(_r32(t2 - lc))), lc


def curves(a, b, f32=False, *, lane0_trapezoid=False):
    """(t2, pdf, cdf), each (..., P) fp64, of the Beta(a, b) curves on
    the grid; a and b are fp32 tensors of one shape (the kernels'
    operands). t2 = base-2 log-pdf, pdf = 2^t2, cdf = trapezoid-
    cumulative pdf with the fp32 step and cdf[..., 0] = 0. f32 follows
    LaneGrid::pdf4 / cdf4 operation by operation (see
    ref_beta_row_curves, and tests/pbest_ref.py for the v1 kernels that
    share it)."""
    lx, l1mx, lx0, l1mx0, dlx, dl1mx, dxf = _grid()
    a = a.float().double().unsqueeze(-1)
    b = b.float().double().unsqueeze(-1)
    lnB2 = (torch.lgamma(a) + torch.lgamma(b) - torch.lgamma(a + b)) * LOG2E
    am1, bm1 = a - 1.0, b - 1.0
    if not f32:
        t2 = am1 * lx + bm1 * l1mx - lnB2
        pdf = torch.exp2(t2)
        tr = 0.5 * (pdf[..., 1:] + pdf[..., :-1]) * dxf
        first = torch.zeros_like(pdf[..., :1])
        if lane0_trapezoid:
            first = 0.5 * (pdf[..., 0:1] + pdf[..., 3:4]) * dxf
        cdf = torch.cumsum(torch.cat([first, tr], -1), -1)
        return t2, pdf, cdf
    K = _r32(am1 * lx0 + bm1 * l1mx0 - lnB2)
    t2 = _r32(am1 * dlx + _r32(bm1 * dl1mx + K))
    pdf = _r32(torch.exp2(t2))
    tr = _r32(_r32(pdf[..., 1:] + pdf[..., :-1]) * 0.5 * dxf)
    first = torch.zeros_like(pdf[..., :1])
    if lane0_trapezoid:
        first = _r32(_r32(pdf[..., 0:1] + pdf[..., 3:4]) * 0.5 * dxf)
    tr = torch.cat([first, tr], -1).reshape(*pdf.shape[:-1], 64, 4)
    local = _r32(_r32(_r32(tr[..., 0] + tr[..., 1]) + tr[..., 2])
                 + tr[..., 3])
    base = _r32(_scan32(local) - local)
    c0 = _r32(base + tr[..., 0])
    c1 = _r32(c0 + tr[..., 1])
    c2 = _r32(c1 + tr[..., 2])
    c3 = _r32(c2 + tr[..., 3])
    cdf = torch.stack([c0, c1, c2, c3], -1).reshape(pdf.shape)
    return t2, pdf, cdf


class CommitRow(NamedTuple):
    a_col: torch.Tensor     # (H,) fp64 dir[:, y, y]
    b_col: torch.Tensor     # (H,) fp64 dir[:, y, :].sum(-1) - a_col
    EG: torch.Tensor        # (H, 2, P) fp64
    delta: torch.Tensor     # (H, P)
    s_base: torch.Tensor    # (P,)
    dall: torch.Tensor      # (P,)
    eg16: torch.Tensor      # (2H, P) bf16
    egw: torch.Tensor       # (2H, P) bf16
    delta16: torch.Tensor   # (H, P) fp16


def ref_commit_cols(a_col, b_col, weights, update_weight, *, f32=False):
    """Row contents table_commit_cols writes for the fp32 columns
    (a_col, b_col): the curves of ref_beta_row_curves, delta = lc1 -
    lc0, s_base = sum_h lc0, dall = sum_h delta, egw = bf16(eg *
    2^s_base * w)."""
    R = _r32 if f32 else _same
    eg, lc = ref_beta_row_curves(a_col, b_col, update_weight, f32=f32)
    H = eg.shape[0]
    delta = R(lc[:, 1] - lc[:, 0])
    s_base = _rows_sum(lc[:, 0], f32, 2)
    dall = _rows_sum(delta, f32, 2)
    esb = R(R(torch.exp2(s_base)) * weights.double())
    egw = R(eg.reshape(2 * H, P) * esb)
    return CommitRow(a_col.double(), b_col.double(), eg, delta, s_base,
                     dall, eg.reshape(2 * H, P).float().to(torch.bfloat16),
                     egw.float().to(torch.bfloat16),
                     delta.float().to(torch.float16))


def ref_commit_row(dirichlets, y: int, weights, update_weight, *,
                   f32=False) -> CommitRow:
    """table_commit_row's contract: a_col = dir[:, y, y], b_col = the
    rest of Dirichlet row y, both handed on as fp32 values, then
    ref_commit_cols."""
    row = dirichlets[:, y, :].double()
    a = row[:, y]
    tot = _sum32(row, 8) if f32 else row.sum(-1)
    b = tot - a
    out = ref_commit_cols(a.float(), _r32(b).float(), weights,
                          update_weight, f32=f32)
    return out._replace(a_col=a, b_col=_r32(b) if f32 else b)


# ---------------------------------------------------------------------
# input builders (seeded, cached, CPU; callers must not modify)
# ---------------------------------------------------------------------

def designed_classes(H: int, C: int, sizes, seed: int) -> torch.Tensor:
    """(len(sizes), H) int64: in row i a random subset of exactly
    sizes[i] models predicts class 0, the rest go round-robin over
    classes 1..C-1."""
    g = torch.Generator().manual_seed(3000 + seed)
    cls = torch.zeros(len(sizes), H, dtype=torch.int64)
    for i, n in enumerate(sizes):
        perm = torch.randperm(H, generator=g)
        cls[i, perm[n:]] = 1 + torch.arange(H - n) % (C - 1)
    return cls


class EsInputs(NamedTuple):
    cls: torch.Tensor       # (B, H) int64
    hvals: torch.Tensor     # (B, H) int32
    offsets: torch.Tensor   # (B, C+1) int32
    s_base: torch.Tensor    # (C, P)
    delta: torch.Tensor     # (C, H, P), None for the gathered kernel
    dall: torch.Tensor      # (C, P), skewed by DALL_SKEW
    sel_all: torch.Tensor   # (B, H, P), gathered kernel only
    w: torch.Tensor         # (P,)


def _synthetic_delta(shape, g) -> torch.Tensor:
    u = torch.rand(*shape, generator=g) * 2 - 1
    return (u + torch.sign(u) * DELTA_FLOOR).float()


@functools.lru_cache(maxsize=None)
def make_es_inputs(H: int, C: int, sizes: tuple, seed: int = 0,
                   gathered: bool = False) -> EsInputs:
    """Synthetic tables for the es_build kernels (their contract is
    table-agnostic): delta = u + sign(u) 2^-6 with u ~ U[-1, 1), s_base
    = -U[0, 30), dall = fp32 sum of delta + DALL_SKEW. Every ES value is
    a normal fp32 number and one model more or less moves a row by at
    least 1.08e-2 relative. Buckets from the project's own _class_csr."""
    g = torch.Generator().manual_seed(4000 + seed)
    cls = designed_classes(H, C, sizes, seed)
    hvals, offsets = tops._class_csr(cls, C)
    s_base = -(torch.rand(C, P, generator=g) * 30)
    delta = dall = sel_all = None
    if gathered:
        sel_all = _synthetic_delta((len(sizes), H, P), g)
    else:
        delta = _synthetic_delta((C, H, P), g)
        dall = (delta.sum(1) + DALL_SKEW).contiguous()
    return EsInputs(cls, hvals, offsets, s_base, delta, dall, sel_all,
                    grid_weights())


class AssembleInputs(NamedTuple):
    M: torch.Tensor             # (C, B, 2H) fp64, unrounded
    cls: torch.Tensor           # (B, H) int64
    pi_hat: torch.Tensor        # (C,)
    pbest_before: torch.Tensor  # (C, H)
    mixture0: torch.Tensor      # (H,)
    problem: PR.Problem


@functools.lru_cache(maxsize=None)
def make_assemble_inputs(H: int, C: int, B: int, p: float = 0.6,
                         seed: int = 0) -> AssembleInputs:
    """A realistic problem (pair_ref.make_problem: heavy-diagonal
    bounded Dirichlets, CPU table_precompute, consensus classes) and
    M = fp64 GEMM of the fp64 ES with EG. Callers round M once to the
    dtype under test; the rounded M is the input of kernel and
    reference alike."""
    pr = PR.make_problem(H, B, C, p, seed=seed)
    tb = pr.tables
    cls = pr.cls_rows
    hvals, offsets = tops._class_csr(cls, C)
    es, _ = ref_es_build(tb.s_base, tb.delta, tb.dall, hvals, offsets,
                         tb.weights)
    M = torch.bmm(es, tb.EG.reshape(C, 2 * H, P).double().transpose(1, 2))
    return AssembleInputs(M, cls, pr.pi_hat, pr.pbest_before, pr.mixture0,
                          pr)


def make_clamp_inputs() -> AssembleInputs:
    """Hand-made assemble inputs (the contract does not need them
    consistent): row (b=1, c=0) of M is all zero, so its total clamps
    at 1e-30, and mixture0 / pbest_before put some m below 1e-12."""
    g = torch.Generator().manual_seed(5000)
    H, C, B = 5, 2, 3
    M = (torch.rand(C, B, 2 * H, generator=g) + 0.05).double()
    M[0, 1] = 0.0
    cls = torch.randint(0, C, (B, H), generator=g)
    pi_hat = torch.tensor([0.7, 0.3])
    pbest_before = torch.full((C, H), 0.2)
    pbest_before[:, 0] = 0.9
    mixture0 = torch.tensor([0.05, 0.3, 0.3, 0.2, 0.15])
    return AssembleInputs(M, cls, pi_hat, pbest_before, mixture0, None)


BETA_RANGES = {
    "wide": ((0.5, 60.0), (0.5, 60.0)),
    "moderate": ((1.0, 25.0), (1.0, 25.0)),
    "concentrated": ((500.0, 20000.0), (500.0, 20000.0)),
    "singular0": ((0.5, 1.0), (1.0, 5.0)),
}


@functools.lru_cache(maxsize=None)
def make_beta_cols(name: str, H: int, seed: int = 0):
    """(alpha_col, beta_col) fp32 (H,), uniform in BETA_RANGES[name]."""
    g = torch.Generator().manual_seed(
        6000 + 100 * list(BETA_RANGES).index(name) + H + seed)
    (a0, a1), (b0, b1) = BETA_RANGES[name]
    a = a0 + (a1 - a0) * torch.rand(H, generator=g)
    b = b0 + (b1 - b0) * torch.rand(H, generator=g)
    return a.float(), b.float()


class CommitInputs(NamedTuple):
    dirichlets: torch.Tensor    # (H, C, C)
    weights: torch.Tensor       # (P,)
    tables: dict                # name -> tensor, seeded filler contents


TABLE_NAMES = ("EG", "delta", "s_base", "eg16", "egw", "delta16", "dall")


@functools.lru_cache(maxsize=None)
def make_commit_inputs(H: int, C: int, seed: int = 0) -> CommitInputs:
    """Heavy-diagonal Dirichlets bounded as in pair_ref.make_problem
    (alpha >= 1, beta >= 2) and the seven table tensors filled with
    seeded filler in [1, 2) (no row of it resembles a committed row,
    and row y must be overwritten entirely)."""
    g = torch.Generator().manual_seed(7000 + seed)
    eye = torch.eye(C)
    dirichlets = (torch.rand(H, C, C, generator=g) * 3 + 0.5
                  + eye * torch.rand(H, C, 1, generator=g) * 20)
    dirichlets = dirichlets + 0.5 * eye + (1 - eye) * 1.5 / (C - 1)

    def filler(*shape, dtype=torch.float32):
        return (torch.rand(*shape, generator=g) + 1).to(dtype)

    tables = {
        "EG": filler(C, H, 2, P), "delta": filler(C, H, P),
        "s_base": filler(C, P), "dall": filler(C, P),
        "eg16": filler(C, 2 * H, P, dtype=torch.bfloat16),
        "egw": filler(C, 2 * H, P, dtype=torch.bfloat16),
        "delta16": filler(C, H, P, dtype=torch.float16),
    }
    return CommitInputs(dirichlets.contiguous(), grid_weights(), tables)


def rel_err(got: torch.Tensor, ref: torch.Tensor,
            floor: float = 0.0) -> float:
    """max |got - ref| / |ref| over the elements with |ref| >= floor
    (and ref != 0)."""
    g, r = got.double(), ref.double()
    ok = (r.abs() >= floor) & (r != 0)
    return float(((g - r).abs()[ok] / r.abs()[ok]).max()) if bool(
        ok.any()) else 0.0
