"""fp64 stage references for the v1 P(best) / EIG kernels (not itself a
test).

Each function is the CONTRACT of one stage of the oldest kernel family,
coda_amd/ops/hip/pbest.hip (pbest_kernel, pbest_row_kernel, the
phase-1 / phase-2 kernels and their wide twins, eig_hyp_kernel and the
EIG phase kernels), written in plain torch on CPU tensors and evaluated
in fp64 on exactly the fp32 operands the kernel receives. The curve
math (LaneGrid::pdf4 / cdf4, beta_grid.h) is tests/table_ref.curves, shared with the
v2 table references; the entropy epilogue is tests/pair_ref.ref_entropy.

`f32=True` re-runs the same reference with every operation rounded to
fp32 in the kernel's order (emulated in fp64, so all hosts agree):

  pass A  the cdf product as an fp32 (mantissa, exponent) pair,
          renormalised after every model, one log2 at the end;
  pass B  per point log2 cdf, the clamped exponent, exp2, pdf * pe * w,
          four points per lane added in turn, the lane sum times the
          fp32 step, a 64-lane tree; the normaliser as 64 lane-strided
          partial sums and the same tree.

fp32-twin-vs-fp64 of the reference itself is how the stage tolerances
of tests/test_pbest_kernels.py are measured, never kernel output. The
keyword-only fault arguments inject the faults of the mutation-floor
tests in tests/test_pbest_ref.py.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import torch

from tests import pair_ref as PR
from tests import table_ref as TR
from tests.pair_ref import _f32c, _r32, _same

P = TR.P
ROWS_PER_BLOCK = 4                # beta_grid.h: waves (rows) per workgroup
# the kernel's float literals at their fp32 values
LOG2_CLAMP = float(torch.tensor(115.41560327111707, dtype=torch.float32))
EPS = _f32c(1e-30, torch.float64)
BULK_LC = -10.0                   # bulk of a curve: reference cdf >= 2^-10


def _dxf() -> float:
    return TR._grid()[-1]


def _wave_sum32(v: torch.Tensor) -> torch.Tensor:
    """(..., 64) -> (...): the 64-lane butterfly, every add in fp32."""
    n = v.shape[-1]
    while n > 1:
        n //= 2
        v = _r32(v[..., :n] + v[..., n:2 * n])
    return v[..., 0]


def _strided_sum32(m: torch.Tensor) -> torch.Tensor:
    """(..., H) -> (...): lane l adds elements l, l + 64, ... in turn,
    then the lanes combine (pbest_pass_b's normaliser)."""
    H = m.shape[-1]
    if H == 0:
        return m.new_zeros(m.shape[:-1])
    if H % 64:
        m = torch.cat([m, m.new_zeros(*m.shape[:-1], 64 - H % 64)], -1)
    m = m.reshape(*m.shape[:-1], -1, 64)
    acc = m[..., 0, :]
    for s in range(1, m.shape[-2]):
        acc = _r32(acc + m[..., s, :])
    return _wave_sum32(acc)


def _seq_sum32(parts) -> torch.Tensor:
    """0 + p0 + p1 + ... left to right in fp32."""
    acc = torch.zeros_like(parts[0])
    for p in parts:
        acc = _r32(acc + p)
    return acc


# ---------------------------------------------------------------------
# pass A / pass B
# ---------------------------------------------------------------------

def ref_slog2(a, b, *, f32=False, drop_last=False, lane0_trapezoid=False):
    """(R, P) fp64 slog2[r, p] = sum_h log2 max(cdf[r, h, p], 1e-30f)
    over the trapezoid-cumulative cdf of Beta(a[r, h], b[r, h]); a, b
    (R, H) fp32. H = 0 gives the identity 0.

    Faults: drop_last leaves the row's last model out; lane0_trapezoid
    counts a first trapezoid at lane 0 (table_ref.curves)."""
    R_, H = a.shape
    if drop_last:
        a, b, H = a[:, :-1], b[:, :-1], H - 1
    if H == 0:
        return torch.zeros(R_, P, dtype=torch.float64)
    _, _, cdf = TR.curves(a, b, f32, lane0_trapezoid=lane0_trapezoid)
    c = cdf.clamp_min(EPS)
    if not f32:
        return torch.log2(c).sum(1)
    pm = torch.ones(R_, P, dtype=torch.float64)
    pe = torch.zeros(R_, P, dtype=torch.float64)
    for h in range(H):
        pm, ex = torch.frexp(_r32(pm * c[:, h]))
        pe = pe + ex
    return _r32(_r32(torch.log2(pm)) + pe)


def slog2_bulk(a, b) -> torch.Tensor:
    """(R, P) bool: the grid points where EVERY model of the row has a
    reference cdf >= 2^-10. Defined on the fp64 reference alone."""
    _, _, cdf = TR.curves(a, b)
    return (torch.log2(cdf.clamp_min(EPS)) >= BULK_LC).all(1)


def ref_masses(a, b, slog2, *, f32=False, drop_last=False,
               lane0_trapezoid=False, full_w0=False, full_w255=False,
               couple_local=False):
    """(masses (R, H), total (R,)) fp64: pass B for a GIVEN slog2 (R, P),
    masses[r, h] = trapz_p pdf * 2^clamp(slog2 - log2 max(cdf, 1e-30f),
    +-115.41560327111707f) with trapezoid weights 0.5 at points 0 and
    255 and the fp32 step; total = sum_h masses. Unnormalised.

    Faults: drop_last gives the last model no mass; full_w0 / full_w255
    weigh an end point fully; couple_local ignores the given slog2 for
    the row's own ref_slog2; lane0_trapezoid as in ref_slog2."""
    R = _r32 if f32 else _same
    R_, H = a.shape
    if H == 0:
        z = torch.zeros(R_, dtype=torch.float64)
        return torch.zeros(R_, 0, dtype=torch.float64), z
    if couple_local:
        slog2 = ref_slog2(a, b, f32=f32, lane0_trapezoid=lane0_trapezoid)
    _, pdf, cdf = TR.curves(a, b, f32, lane0_trapezoid=lane0_trapezoid)
    w = torch.ones(P, dtype=torch.float64)
    w[0] = 1.0 if full_w0 else 0.5
    w[-1] = 1.0 if full_w255 else 0.5
    lc = R(torch.log2(cdf.clamp_min(EPS)))
    arg = R(slog2.double().unsqueeze(1) - lc).clamp(-LOG2_CLAMP, LOG2_CLAMP)
    term = R(R(pdf * R(torch.exp2(arg))) * w)
    if not f32:
        masses = term.sum(-1) * _dxf()
    else:
        t = term.reshape(R_, H, 64, 4)
        acc = t[..., 0]
        for j in range(1, 4):
            acc = _r32(acc + t[..., j])
        masses = _wave_sum32(_r32(acc * _dxf()))
    if drop_last:
        masses = masses.clone()
        masses[:, -1] = 0.0
    total = _strided_sum32(masses) if f32 else masses.sum(-1)
    return masses, total


def normalise(masses, total, *, f32=False):
    """masses * (1 / max(total, 1e-30f))."""
    R = _r32 if f32 else _same
    inv = R(1.0 / total.clamp_min(EPS))
    return R(masses * inv.unsqueeze(-1))


def ref_pbest(a, b, *, f32=False, **faults):
    """(R, H) fp64 normalised P(best): pbest_kernel's contract."""
    s_faults = {k: v for k, v in faults.items()
                if k in ("drop_last", "lane0_trapezoid")}
    slog2 = ref_slog2(a, b, f32=f32, **s_faults)
    masses, total = ref_masses(a, b, slog2, f32=f32, **faults)
    return normalise(masses, total, f32=f32)


# ---------------------------------------------------------------------
# windowed forms: pbest_row_kernel, pbest_phase1/2_wide
# ---------------------------------------------------------------------

def windows(H: int, hc: int, nwin: int = None):
    """[(h0, h1)] of the model windows of width hc; nwin fixes their
    number (the row kernel always has 4, empty ones included)."""
    hc = min(hc, H) if nwin is None else hc
    n = -(-H // hc) if nwin is None else nwin
    return [(min(k * hc, H), min(k * hc + hc, H)) for k in range(n)]


def _window_models(a, b, k, wins, hc, window_shift):
    h0, h1 = wins[k]
    if window_shift and k >= 1:
        h0, h1 = h0 - hc, h1 - hc
    return a[:, h0:h1], b[:, h0:h1]


def ref_slog2_windows(a, b, hc, *, f32=False, nwin=None, drop_last=False,
                      window_shift=False, lane0_trapezoid=False):
    """(KH, R, P) per-window slog2 partials (pbest_phase1_wide's
    contract). Faults: drop_last per window; window_shift makes window
    k >= 1 read window k - 1's models."""
    wins = windows(a.shape[1], hc, nwin)
    hc = wins[0][1] - wins[0][0] if nwin is None else hc
    return torch.stack([
        ref_slog2(*_window_models(a, b, k, wins, hc, window_shift),
                  f32=f32, drop_last=drop_last and wins[k][1] > wins[k][0],
                  lane0_trapezoid=lane0_trapezoid)
        for k in range(len(wins))])


def ref_masses_windows(a, b, slog2, hc, *, f32=False, nwin=None,
                       drop_last=False, window_shift=False,
                       couple_local=False, **faults):
    """(masses (R, H), tot_part (KH, R)): pass B window by window
    against the given slog2 (pbest_phase2_wide's contract). Faults as
    ref_masses, per window; couple_local couples each window against
    its own partial; window_shift as in ref_slog2_windows."""
    wins = windows(a.shape[1], hc, nwin)
    hc = wins[0][1] - wins[0][0] if nwin is None else hc
    ms, ts = [], []
    for k, (h0, h1) in enumerate(wins):
        m, t = ref_masses(*_window_models(a, b, k, wins, hc, window_shift),
                          slog2, f32=f32, drop_last=drop_last and h1 > h0,
                          couple_local=couple_local, **faults)
        ms.append(m)
        ts.append(t)
    return torch.cat(ms, 1), torch.stack(ts)


def ref_pbest_windows(a, b, hc, *, f32=False, nwin=None, **faults):
    """(R, H) normalised P(best) through the windowed two-pass split:
    partials summed left to right, pass B per window, window totals
    summed left to right. nwin = 4 and hc = ceil(H / 4) is
    pbest_row_kernel; nwin = None is ops._pbest_wide_hip."""
    s_faults = {k: v for k, v in faults.items()
                if k in ("drop_last", "lane0_trapezoid", "window_shift")}
    parts = ref_slog2_windows(a, b, hc, f32=f32, nwin=nwin, **s_faults)
    slog2 = _seq_sum32(parts) if f32 else parts.sum(0)
    masses, tots = ref_masses_windows(a, b, slog2, hc, f32=f32, nwin=nwin,
                                      **faults)
    total = _seq_sum32(tots) if f32 else tots.sum(0)
    return normalise(masses, total, f32=f32)


def ref_pbest_row(a, b, *, f32=False, **faults):
    """pbest_row_kernel: one row, four windows of ceil(H / 4) models."""
    hc = -(-a.shape[1] // ROWS_PER_BLOCK)
    return ref_pbest_windows(a, b, hc, f32=f32, nwin=ROWS_PER_BLOCK,
                             **faults)


# ---------------------------------------------------------------------
# hypothetical update + entropy: stage_hyp, eig_hyp_kernel
# ---------------------------------------------------------------------

def ref_hyp_betas(alpha_cc, beta_cc, cls, w, *, vflip=False, w_both=False,
                  w_neither=False, next_row_class=False):
    """(a, b) fp32, each (B * C, H): the rows stage_hyp stages. Row
    r = b * C + c, model h gets alpha_cc[h, c] + w if cls[b, h] == c,
    else beta_cc[h, c] + w; the sums are fp32 sums, as the kernel's
    operands are.

    Faults: vflip inverts the select; w_both / w_neither add the weight
    to both sides / to none; next_row_class compares with the (b, c) of
    row r + 1 (the last row keeps its own)."""
    H, C = alpha_cc.shape
    B = cls.shape[0]
    r = torch.arange(B * C)
    rc = (r + 1).clamp_max(B * C - 1) if next_row_class else r
    hit = cls.long()[rc // C] == (rc % C).unsqueeze(1)          # (B*C, H)
    if vflip:
        hit = ~hit
    wt = torch.tensor(float(w), dtype=torch.float32)
    add_a = torch.where(hit, wt, torch.zeros(()))
    add_b = wt - add_a
    if w_both:
        add_a = add_b = wt.expand_as(add_a)
    if w_neither:
        add_a = add_b = torch.zeros_like(add_a)
    a = alpha_cc.float().t()[r % C] + add_a
    b = beta_cc.float().t()[r % C] + add_b
    return a.contiguous(), b.contiguous()


def ref_entropy_rows(masses, C, pi_hat, pbest_before, mixture0, *,
                     f32=False):
    """(B * C,) -sum_h m log2 m, m = max(mixture0 + pi_c (pb -
    pbest_before[c]), 1e-12f), pb = masses / max(sum masses, 1e-30f);
    row r belongs to class r % C (pair_ref.ref_entropy)."""
    pc = torch.arange(masses.shape[0]) % C
    return PR.ref_entropy(masses, pc, pi_hat, pbest_before, mixture0,
                          f32=f32, lanes=64)


def ref_h_after(alpha_cc, beta_cc, cls, w, pi_hat, pbest_before, mixture0,
                *, f32=False, **faults):
    """(B, C) h_after of eig_hyp_kernel: ref_hyp_betas -> ref_slog2 ->
    ref_masses -> ref_entropy_rows."""
    a, b = ref_hyp_betas(alpha_cc, beta_cc, cls, w, **faults)
    masses, _ = ref_masses(a, b, ref_slog2(a, b, f32=f32), f32=f32)
    C = alpha_cc.shape[1]
    return ref_entropy_rows(masses, C, pi_hat, pbest_before, mixture0,
                            f32=f32).reshape(-1, C)


# ---------------------------------------------------------------------
# input builders (seeded, cached, CPU; callers must not modify)
# ---------------------------------------------------------------------

BETA_RANGES = {
    "wide": TR.BETA_RANGES["wide"],
    "moderate": TR.BETA_RANGES["moderate"],
    # pdf singular at x -> 0 ...
    "singular_a": ((0.3, 1.0), (1.0, 5.0)),
    # ... and at x -> 1 too
    "singular_ab": ((0.3, 1.0), (0.3, 1.0)),
}
FAMILIES = tuple(BETA_RANGES) + ("competitive",)
# H = 1 rows for the trapezoid end weights: a large pdf at point 0 / 255
END_RANGES = {
    "end0": ((0.3, 0.6), (2.0, 5.0)),
    "end255": ((2.0, 5.0), (0.3, 0.6)),
}
BIG_SHARE = 0.99      # big entries hold at least this much of a row
TOP_CAP = 0.9         # competitive rows, H >= 3: no entry above this


def _draw_row(name: str, H: int, g):
    if name == "competitive":
        n = 500.0 + 19500.0 * torch.rand(1, H, generator=g,
                                         dtype=torch.float64)
        m0 = 0.3 + 0.4 * torch.rand(1, 1, generator=g, dtype=torch.float64)
        u = 2 * torch.rand(1, H, generator=g, dtype=torch.float64) - 1
        a = n * (m0 + u / n.sqrt())
        return a.float(), (n - a).float()
    (a0, a1), (b0, b1) = {**BETA_RANGES, **END_RANGES}[name]
    a = a0 + (a1 - a0) * torch.rand(1, H, generator=g)
    b = b0 + (b1 - b0) * torch.rand(1, H, generator=g)
    return a.float(), b.float()


def row_conditions(name: str, p: torch.Tensor) -> bool:
    """The input conditions of one fp64 reference row p (H,): its big
    entries (>= 1 / (16 H)) hold >= BIG_SHARE of the mass, and a
    competitive row with H >= 3 has no entry above TOP_CAP."""
    ok = float(p[big_entries(p)].sum()) >= BIG_SHARE * float(p.sum())
    if name == "competitive" and p.shape[-1] >= 3:
        ok = ok and float(p.max()) <= TOP_CAP
    return ok


@functools.lru_cache(maxsize=None)
def make_betas(name: str, R: int, H: int, seed: int = 0):
    """(a, b) fp32 (R, H). The four ranges draw uniformly from
    BETA_RANGES[name]. "competitive" is concentrated AND contested: per
    model n = a + b uniform in [500, 20000], per row a common mean in
    [0.3, 0.7], every model's mean within 1 / sqrt(n) of it - about two
    standard deviations of its own Beta - so several models share the
    row's mass (an independent concentrated draw gives one model
    p = 1.000, which any kernel passes after normalisation).

    Rows are drawn one at a time and a row whose fp64 reference misses
    row_conditions is drawn again (decided on the reference alone; at
    H = 2 a 98 / 2 split has its small entry below 1 / 32)."""
    g = torch.Generator().manual_seed(
        8000 + 1000 * (list(FAMILIES) + list(END_RANGES)).index(name)
        + 17 * R + H + seed)
    rows = []
    for _ in range(100 * R):
        a, b = _draw_row(name, H, g)
        if row_conditions(name, ref_pbest(a, b)[0]):
            rows.append((a, b))
        if len(rows) == R:
            break
    assert len(rows) == R, (name, R, H)
    return (torch.cat([r[0] for r in rows]).contiguous(),
            torch.cat([r[1] for r in rows]).contiguous())


def designed_hyp_classes(H: int, C: int, B: int, seed: int = 0):
    """(B, H) int64 argmax classes with a designed census: candidate 0
    has every model on class 0 (row (0, 0) all hits, rows (0, c > 0)
    none), candidate 1 has exactly model H - 1 on class C - 1 and the
    rest on class 0 (row (1, C - 1) exactly one hit), the others are
    uniform."""
    g = torch.Generator().manual_seed(9000 + 31 * H + 7 * C + B + seed)
    cls = torch.randint(0, C, (B, H), generator=g)
    cls[0] = 0
    cls[1] = 0
    cls[1, H - 1] = C - 1
    return cls


class HypInputs(NamedTuple):
    alpha_cc: torch.Tensor      # (H, C)
    beta_cc: torch.Tensor       # (H, C)
    cls: torch.Tensor           # (B, H) int64
    pi_hat: torch.Tensor        # (C,)
    pbest_before: torch.Tensor  # (C, H) fp32, ref_pbest of the Betas
    mixture0: torch.Tensor      # (H,) fp32
    pi_hat_xi: torch.Tensor     # (B, C) dense rows summing to 1


@functools.lru_cache(maxsize=None)
def make_hyp_inputs(H: int, C: int, B: int, seed: int = 0) -> HypInputs:
    """One v1 EIG problem: per-class competitive Betas with n in
    [20, 200] (one update of weight 0.5 or 1 moves a model's share
    visibly), designed classes, and a consistent pbest_before /
    mixture0 computed by the fp64 reference and rounded to fp32."""
    g = torch.Generator().manual_seed(9500 + 31 * H + 7 * C + B + seed)
    n = 20.0 + 180.0 * torch.rand(C, H, generator=g, dtype=torch.float64)
    m0 = 0.4 + 0.3 * torch.rand(C, 1, generator=g, dtype=torch.float64)
    u = 2 * torch.rand(C, H, generator=g, dtype=torch.float64) - 1
    a = (n * (m0 + u / n.sqrt())).float()
    b = (n.float() - a)
    pi_hat = torch.rand(C, generator=g) + 0.2
    pi_hat /= pi_hat.sum()
    pb = ref_pbest(a, b).float()
    mixture0 = (pi_hat.double().unsqueeze(1) * pb.double()).sum(0).float()
    pi_xi = torch.rand(B, C, generator=g) + 0.1
    pi_xi /= pi_xi.sum(-1, keepdim=True)
    return HypInputs(a.t().contiguous(), b.t().contiguous(),
                     designed_hyp_classes(H, C, B, seed), pi_hat, pb,
                     mixture0, pi_xi)


def make_hyp_clamp_inputs() -> HypInputs:
    """Hand-made inputs (the contract does not need them consistent)
    that put mixture0 + pi_c (pb - pbest_before) below 1e-12 for some
    model: pbest_before[:, 0] = 0.9 against a mixture0[0] of 0.05."""
    i = make_hyp_inputs(5, 2, 3, seed=1)
    pbb = torch.full((2, 5), 0.2)
    pbb[:, 0] = 0.9
    return i._replace(pi_hat=torch.tensor([0.7, 0.3]), pbest_before=pbb,
                      mixture0=torch.tensor([0.05, 0.3, 0.3, 0.2, 0.15]))


# ---------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------

def big_entries(ref: torch.Tensor) -> torch.Tensor:
    """Entries of a normalised reference row that hold >= 1 / (16 H)."""
    return ref >= 1.0 / (16 * ref.shape[-1])


def pbest_errs(got, ref):
    """(max abs error over the rows, max relative error on the big
    entries of the reference)."""
    g, r = got.double(), ref.double()
    big = big_entries(r)
    return (float((g - r).abs().max()),
            float(((g - r).abs()[big] / r[big]).max()))


def mass_errs(masses, total, ref_m, ref_t):
    """(max relative mass error on the big entries - those whose
    normalised reference share is >= 1 / (16 H) - and max relative
    total error)."""
    m, rm = masses.double(), ref_m.double()
    big = big_entries(rm / rm.sum(-1, keepdim=True).clamp_min(1e-300))
    return (float(((m - rm).abs()[big] / rm[big]).max()),
            TR.rel_err(total, ref_t))


def slog2_errs(got, ref, bulk):
    """(max abs error over every point, max abs error over the bulk)."""
    d = (got.double() - ref.double()).abs()
    return float(d.max()), float(d[bulk].max())
